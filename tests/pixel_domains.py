"""Seeded stereo pairs in named PIXEL DOMAINS -- test infrastructure, no GPU.

Every other generator of the suite draws whole numbers in 0..255, where each sum a cost function forms is exact in fp32, no
comparison meets a NaN and no square overflows.  This one starts from the same kind of pair (a noisy shifted copy, so that
costs have structure) and moves it into the domains real inputs live in: 16-bit and float-valued samples, denormals, signed
zeros, flat regions, per-pixel NaN nodata (isolated pixels, a border on two sides, a hole) and +-Inf samples.

    u, v = pair("nodata", seed, nch, ny, nx)            # float32 (nch, ny, nx) each
    u, v = pair("u16", seed, 3, 96, 128, vshape=(90, 120))

`CLASSES` lists the names; `degenerate_ok(cls, distance)` says where a trivial volume (all zeros / all +INF) is the point of
the case, and `degeneracy(C)` measures a volume against the non-degeneracy condition the tests assert elsewhere.
"""
import numpy as np

CLASSES = ("u8", "u16", "unit", "signed", "huge", "fltmax", "denormal", "negzero", "const", "flat", "nodata", "nodata_all",
           "inf", "mixed")
FLT_MAX = np.float32(3.4028234663852886e38)
# Where a trivial volume cannot be avoided.  The rule asked for is "const, nodata_all and the huge-class SD cases"; "SD cases" is
# read here as every distance that SQUARES samples or their differences, and the denormal class joins for the same reason at the
# other end of the exponent range -- measured on the reference's volumes of the cases of tests/test_pixel_domains_ref.py and
# tests/test_gpu_pixel_domain.py, these and only these combinations break the condition:
#   huge, fltmax  x sd, btsd   every square is +INF: up to 93 % of the cells +INF, then all-zero pixels
#   huge, fltmax  x ncc        the window sums of squares are +INF, inf - inf = NaN, the clipped cost is 0: 87 % all-zero pixels
#   denormal      x sd, btsd   every square underflows to zero: 86 % all-zero pixels
# (denormal x ncc is NOT trivial: zero variance takes the 1e-7 floor and the cost is the constant nch * 64.)
TRIVIAL_BY_ARITHMETIC = {"huge": ("sd", "btsd", "ncc"), "fltmax": ("sd", "btsd", "ncc"), "denormal": ("sd", "btsd")}


def degenerate_ok(cls, distance="ad"):
    """A trivial volume is the point of the case: one value everywhere, one image without data, or squares that leave fp32."""
    if cls in ("const", "nodata_all"):
        return True
    return distance in TRIVIAL_BY_ARITHMETIC.get(cls, ())


def degeneracy(C):
    """(share of pixels whose costs are all zero, share of cells that are +INF) of a volume (ny, nx, L)."""
    C = np.asarray(C)
    return float(np.mean(np.all(C == 0, axis=2))), float(np.mean(np.isposinf(C)))


def base_pair(seed, nch, ny, nx, vshape=None, shift=3):
    """Whole numbers 0..255: v is u moved `shift` pixels to the right plus noise in -2..2 (clipped), cropped / extended to
    vshape = (vny, vnx)."""
    rng = np.random.default_rng(seed)
    vny, vnx = vshape or (ny, nx)
    cy, cx = max(ny, vny), max(nx, vnx)
    canvas = rng.integers(0, 256, size=(nch, cy, cx))
    # smooth it a little along x so that neighbouring labels have related costs (a pure noise image has none)
    canvas = (canvas + np.roll(canvas, 1, axis=2)) // 2
    u = canvas[:, :ny, :nx]
    v = np.clip(np.roll(canvas, shift, axis=2) + rng.integers(-2, 3, size=canvas.shape), 0, 255)[:, :vny, :vnx]
    return u.astype(np.float32), v.astype(np.float32), rng


def nodata_mask(rng, ny, nx, which):
    """Per-PIXEL nodata: six isolated pixels, a 2-row / 3-column border on two sides (`which` picks the sides, so that the two
    images of a pair differ), one rectangular hole (6x8 on images of the usual test size, smaller on tiny ones)."""
    m = np.zeros((ny, nx), bool)
    m[rng.integers(0, ny, 6), rng.integers(0, nx, 6)] = True
    rows, cols = min(2, max(1, ny // 8)), min(3, max(1, nx // 8))
    if which == 0:
        m[:rows, :] = True
        m[:, :cols] = True
    else:
        m[ny - rows:, :] = True
        m[:, nx - cols:] = True
    hy, hx = min(6, max(1, ny // 5)), min(8, max(1, nx // 5))
    y0, x0 = int(rng.integers(rows, ny - hy - rows + 1)), int(rng.integers(cols, nx - hx - cols + 1))
    m[y0:y0 + hy, x0:x0 + hx] = True
    return m


def _put_inf(rng, a):
    """Isolated +Inf and -Inf SAMPLES (one channel each), four of either sign."""
    nch, ny, nx = a.shape
    for sign in (np.inf, -np.inf):
        a[rng.integers(0, nch, 4), rng.integers(0, ny, 4), rng.integers(0, nx, 4)] = sign


def _to_u16(rng, a):
    return np.clip(a.astype(np.int64) * 257 + rng.integers(-128, 129, size=a.shape), 0, 65535).astype(np.float32)


def pair(cls, seed, nch, ny, nx, vshape=None, shift=3):
    """(u, v) of class `cls`, float32 (nch, ny, nx) and (nch, vny, vnx); deterministic in all its arguments."""
    if cls not in CLASSES:
        raise ValueError("unknown pixel class %r" % (cls,))
    u, v, rng = base_pair(seed, nch, ny, nx, vshape, shift)
    f32 = np.float32
    if cls == "u8":
        pass
    elif cls == "u16":
        u, v = _to_u16(rng, u), _to_u16(rng, v)
    elif cls == "unit":
        u, v = u / f32(255), v / f32(255)
    elif cls == "signed":
        u, v = (u - f32(128)) * f32(1.37), (v - f32(128)) * f32(1.37)
    elif cls == "huge":  # multiples of 1e18 from 2e19 to 2.8e20: every square is +INF
        u, v = (u + f32(20)) * f32(1e18), (v + f32(20)) * f32(1e18)
    elif cls == "fltmax":  # up to FLT_MAX / 4: differences are finite, sums over channels / windows are not
        u, v = u / f32(255) * (FLT_MAX / f32(4)), v / f32(255) * (FLT_MAX / f32(4))
    elif cls == "denormal":  # multiples of 1e-40 (a denormal): kept by the CPU, and by a kernel that does not flush
        u, v = u * f32(1e-40), v * f32(1e-40)
    elif cls == "negzero":
        for a in (u, v):
            r = rng.random(a.shape)
            a[r < 0.15] = -0.0
            a[(r >= 0.15) & (r < 0.30)] = 0.0
    elif cls == "const":
        u[:], v[:] = 77.0, 77.0
    elif cls == "flat":
        # one flat patch where the images match (the same value at the shifted position), one where they do not, one in u alone
        py, px = max(2, ny // 4), max(3, nx // 4)
        y0, x0 = ny // 8, nx // 8
        u[:, y0:y0 + py, x0:x0 + px] = 90.0
        v[:, y0:y0 + py, x0 + shift:x0 + shift + px] = 90.0
        y1, x1 = ny // 2, nx // 2
        u[:, y1:y1 + py, x1:x1 + px] = 31.0
        v[:, y1:y1 + py, x1 + shift:x1 + shift + px] = 200.0
        u[:, ny - py:, :px] = 140.0
    elif cls == "nodata":
        u[:, nodata_mask(rng, u.shape[1], u.shape[2], 0)] = np.nan
        v[:, nodata_mask(rng, v.shape[1], v.shape[2], 1)] = np.nan
    elif cls == "nodata_all":
        v[:] = np.nan
    elif cls == "inf":
        _put_inf(rng, u)
        _put_inf(rng, v)
    elif cls == "mixed":
        u, v = _to_u16(rng, u), _to_u16(rng, v)
        u[:, nodata_mask(rng, u.shape[1], u.shape[2], 0)] = np.nan
        v[:, nodata_mask(rng, v.shape[1], v.shape[2], 1)] = np.nan
        _put_inf(rng, u)
        _put_inf(rng, v)
    return np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)


# the prefilter x distance pairs of tests/test_oracle_vs_ref.py::test_costvolume_sweep
SWEEP_PAIRS = [("none", "ad"), ("none", "sd"), ("none", "census"), ("census", "ad"), ("sobelx", "ad"), ("gblur", "sd"),
               ("sobel_x", "ad"), ("none", "foo"), ("none", "ncc"), ("gblur", "ncc"), ("none", "btad"), ("sobelx", "btsd")]


def effective_distance(distance):
    """What the reference computes for a distance name: unknown names fall back to absolute differences."""
    return distance if distance in ("ad", "sd", "census", "ncc", "btad", "btsd") else "ad"


def census_aligned(nch, win):
    return (nch * (win * win - 1)) % 8 == 0
