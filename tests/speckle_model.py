"""numpy model of the speckle filter, float32 throughout, and the crafted maps of its tests.

    valid      d(p) finite; NaN and +-INF pixels belong to no component and pass to `out` bit for bit
    edge       4-neighbours p, q, both valid, are joined iff fabsf(d(p) - d(q)) <= maxdiff (one float32 subtraction)
    component  of that graph; size(p) = its pixel count
    out        = NaN where valid and size <= maxsize, else d;   size_map = (float)size on valid pixels, 0 elsewhere

The labelling is label-equivalence over whole arrays: every pixel takes the smallest root among itself and the neighbours it is
joined with, every root hangs itself under the smallest value one of its pixels saw, the forest is flattened by pointer jumping,
until nothing changes.  No traversal order anywhere.
"""
import ctypes as C
import os
import subprocess

import numpy as np

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the pair and the options of the command-line test in test_gpu_speckle.py, and the maxsize it filters with
# (test_speckle_model.py checks on the oracle's final map that this size removes a visible part of the valid pixels, not all)
PAIR = dict(nx=96, ny=64, dmin=-16, dmax=0, NDIR=8, P1=8.0, P2=32.0, TSGM=4)
CLI_MAXSIZE = 100
CLI_MAXDIFF = 1.0


def edges(d, maxdiff):
    """(right, down): right[y, x] -- (x, y) and (x + 1, y) are joined; down[y, x] -- (x, y) and (x, y + 1)."""
    d = np.asarray(d, np.float32)
    fin = np.isfinite(d)
    with np.errstate(all="ignore"):
        right = fin[:, :-1] & fin[:, 1:] & (np.abs((d[:, :-1] - d[:, 1:]).astype(np.float32)) <= f32(maxdiff))
        down = fin[:-1, :] & fin[1:, :] & (np.abs((d[:-1, :] - d[1:, :]).astype(np.float32)) <= f32(maxdiff))
    return right, down


def labels(d, maxdiff):
    """[ny][nx] int64: the smallest linear index of every pixel's component (an invalid pixel: its own index)."""
    d = np.asarray(d, np.float32)
    if not (maxdiff >= 0):
        raise ValueError("speckle: maxdiff must be >= 0 and not NaN")
    ny, nx = d.shape
    right, down = edges(d, maxdiff)
    lab = np.arange(ny * nx, dtype=np.int64)
    while True:
        L = lab.reshape(ny, nx)
        m = L.copy()
        m[:, :-1] = np.where(right, np.minimum(m[:, :-1], L[:, 1:]), m[:, :-1])
        m[:, 1:] = np.where(right, np.minimum(m[:, 1:], L[:, :-1]), m[:, 1:])
        m[:-1, :] = np.where(down, np.minimum(m[:-1, :], L[1:, :]), m[:-1, :])
        m[1:, :] = np.where(down, np.minimum(m[1:, :], L[:-1, :]), m[1:, :])
        new = lab.copy()
        np.minimum.at(new, lab, m.ravel())  # every root: the smallest root one of its pixels is joined with
        while True:                         # flatten
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            return lab.reshape(ny, nx)
        lab = new


def sizes(d, maxdiff):
    """[ny][nx] int64: pixels of every pixel's component, 0 on invalid pixels."""
    d = np.asarray(d, np.float32)
    lab = labels(d, maxdiff).ravel()
    n = np.bincount(lab, minlength=lab.size)[lab].reshape(d.shape)
    return np.where(np.isfinite(d), n, 0)


def speckle(d, maxsize, maxdiff=1.0, size=None):
    """(out, size_map), float32 [ny][nx].  `size`: sizes(d, maxdiff), if the caller has it already."""
    if maxsize < 0:
        raise ValueError("speckle: maxsize must be >= 0")
    d = np.asarray(d, np.float32)
    n = sizes(d, maxdiff) if size is None else size
    out = d.copy()
    out[np.isfinite(d) & (n <= maxsize)] = f32(np.nan)
    return out, n.astype(np.float32)


# ---- crafted maps ------------------------------------------------------------------------------------------------------------
FLT_MAX = np.finfo(np.float32).max
DENORM = np.float32(1.4e-45)  # the smallest positive float32


def _spiral(nx, ny):
    """A one-pixel-wide spiral from the top left corner inwards, one pixel of gap between its arms; True on the path, and the
    path's pixels in walking order."""
    m = np.zeros((ny, nx), bool)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = True
    path = [(0, 0)]

    def can(x, y, dx, dy):
        ax, ay, bx, by = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if not (0 <= ax < nx and 0 <= ay < ny) or m[ay, ax]:
            return False
        return not (0 <= bx < nx and 0 <= by < ny) or not m[by, bx]

    while True:
        if not can(x, y, dx, dy):
            dx, dy = -dy, dx
            if not can(x, y, dx, dy):
                return m, path
        x, y = x + dx, y + dy
        m[y, x] = True
        path.append((x, y))


def _serpentine(nx, ny):
    """Every other row full, joined to the next full row at alternating ends: one path, one pixel wide."""
    m = np.zeros((ny, nx), bool)
    m[0::2, :] = True
    for k, y in enumerate(range(1, ny, 2)):
        if y + 1 < ny:
            m[y, nx - 1 if k % 2 == 0 else 0] = True
    return m


def crafted(nx, ny, tw=64, th=16, seed=0):
    """[(name, d, maxdiff)]: the maps the GPU kernels are held to, for one shape.  tw, th: the tile of the kernels (plan_speckle),
    which the seams of some patterns are placed by."""
    nan, inf = f32(np.nan), f32(np.inf)
    yy, xx = np.mgrid[0:ny, 0:nx]
    out = []

    def add(name, d, maxdiff=1.0):
        d = np.asarray(d, np.float32)
        assert d.shape == (ny, nx), (name, d.shape)
        out.append((name, d, maxdiff))

    add("one_component", np.full((ny, nx), 5.0))
    add("all_nan", np.full((ny, nx), nan))
    add("checkerboard", np.where((xx + yy) % 2 == 0, 0.0, 10.0))
    add("serpentine_rows", np.where(_serpentine(nx, ny), 1.0, nan))
    add("serpentine_columns", np.where(_serpentine(ny, nx).T, 1.0, nan))
    m, path = _spiral(nx, ny)
    sp = np.full((ny, nx), nan, np.float32)
    for k, (x, y) in enumerate(path):
        sp[y, x] = 0.25 * k  # a ramp along the path (exact in float32): chained, the ends far apart
    add("spiral", sp, 0.25)
    # blocks that meet only at tile corners: diagonal neighbours, never joined
    add("tile_corners", np.where(((xx // tw) + (yy // th)) % 2 == 0, 1.0, nan))
    if nx >= 3:
        wall = np.full((ny, nx), 3.0, np.float32)
        wall[:, nx // 2] = nan
        add("wall", wall)
        gap = wall.copy()
        gap[ny // 2, nx // 2] = 3.0
        add("wall_with_gap", gap)
    ramp = (0.5 * xx + 1000.0 * yy).astype(np.float32)  # rows apart, steps of exactly 0.5 along a row
    add("ramp_step_equals_maxdiff", ramp, 0.5)
    add("ramp_step_above_maxdiff", ramp, float(np.nextafter(f32(0.5), f32(0))))
    add("zeros_of_both_signs", np.where((xx + yy) % 2 == 0, 0.0, -0.0), 0.0)
    den = (((xx + 2 * yy) % 3).astype(np.float32) * DENORM).astype(np.float32)  # neighbours differ by one or two denormal steps
    add("denormals", den, float(DENORM))
    infs = np.full((ny, nx), 1.0, np.float32)
    infs[:, nx // 2] = inf
    infs[ny // 2, :] = -inf
    add("infinities_split", infs)
    big = np.where((xx + yy) % 2 == 0, FLT_MAX, -FLT_MAX)  # every difference overflows to INF
    add("overflow_finite_maxdiff", big, float(FLT_MAX))
    add("overflow_infinite_maxdiff", big, float("inf"))
    rng = np.random.default_rng(1000 * nx + ny + seed)
    rnd = rng.choice(np.array([0.0, 1.0, 2.5, 4.0], np.float32), size=(ny, nx))
    rnd[rng.random((ny, nx)) < 0.2] = nan
    add("random_levels", rnd)
    return out


def maxsizes(size, npix):
    """The maxsize values a test filters one map with: 0, 1, the largest component's exact size and one below it, every pixel."""
    s = int(size.max())
    return sorted({0, 1, npix} | ({s, s - 1} if s >= 1 else set()))


# ---- plan_speckle on the host (tests/speckle_plan_harness.cc) -------------------------------------------------------------------
PLAN_OUT = ("family", "tw", "th", "ntx", "nty", "planes", "grid_local", "grid_seams", "grid_count", "grid_apply", "scratch_bytes")


def plan_lib(tmpdir):
    so = os.path.join(str(tmpdir), "libspeckle_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mgm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "speckle_plan_harness.cc"), "-o", so], check=True)
    return C.CDLL(so)


def plan(lib, rows):
    """rows: [(nx, ny, num_cu)] -> [dict of PLAN_OUT]"""
    req = np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, 3))
    out = np.zeros((len(req), len(PLAN_OUT)), dtype=np.int64)
    lib.speckle_plan(req.ctypes.data_as(C.c_void_p), C.c_int(len(req)), out.ctypes.data_as(C.c_void_p))
    return [dict(zip(PLAN_OUT, r)) for r in out.tolist()]
