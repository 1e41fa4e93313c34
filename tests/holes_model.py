"""numpy model of hole filling, float32 throughout and bit for bit, and the crafted maps of its tests.

    valid       d(p) finite; NaN and +-INF pixels are holes
    directions  0 (+1,0)  1 (-1,0)  2 (0,+1)  3 (0,-1)  4 (+1,+1)  5 (-1,+1)  6 (+1,-1)  7 (-1,-1); dirs takes the first 2, 4 or 8
    candidate   c_k(p) = d(p + t * step_k) for the smallest t >= 1 with that pixel inside the image and valid; none when the ray
                leaves the image first or when maxdist > 0 and t > maxdist; rays read the original map and pass over holes
    fill value  the n >= 1 candidates ordered by (value, direction index): min v[0], max v[n-1], median v[n/2]
    out         = d on valid pixels and on holes without a candidate, bit for bit;  filled = 1 where a hole received a value

Vectorised: per direction the lines along it become the columns of a sheared copy of the map, walked so that the source lies at
the smaller row, and np.maximum.accumulate carries "the row of the last valid pixel" down every column.  No ray is marched.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from speckle_model import PAIR  # noqa: F401  (the pair of the command-line test: tests/speckle_model.PAIR)

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))  # (sx, sy) of direction k
MODES = ("median", "min", "max")

# the command-line test (tests/test_gpu_holes.py) and the condition tests/test_holes_model.py checks for it on the oracle
CLI_ARGS = "-r -16 -R 0 -t census -s none -O 8"  # PAIR's range, census, no subpixel refinement, 8 directions
CLI_SPECKLE = 100       # MGM_SPECKLE of every run (MGM_SPECKLE_DIFF stays 1)
CLI_RUNS = (("median", 8, 0), ("min", 2, 0), ("median", 8, 3))  # (MGM_FILL_HOLES, _DIRS, _DIST)


def _from_above(a):
    """Per pixel of the bit image a [ny][n] (uint32; the finite ones are the valid pixels) the nearest valid pixel strictly above
    it in its column: (bits, distance), distance 0 where there is none."""
    ny, n = a.shape
    valid = np.isfinite(a.view(np.float32))
    rows = np.arange(ny, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(valid, rows, -1), axis=0)  # the last valid row at or above
    src = np.full((ny, n), -1, np.int64)
    src[1:] = last[:-1]                                                # ... strictly above
    bits = np.take_along_axis(a, np.maximum(src, 0), axis=0)
    return bits, np.where(src >= 0, rows - src, 0)


def rays(d):
    """(cand, dist): [8][ny][nx] -- the bits (uint32) of every pixel's candidate along direction k and its distance t >= 1, 0 where
    the ray leaves the image without meeting a valid pixel.  Computed for every pixel, holes or not; independent of mode, dirs
    and maxdist."""
    d = np.ascontiguousarray(d, np.float32)
    ny, nx = d.shape
    bits = d.view(np.uint32)
    hole = np.uint32(0x7FC00000)
    cand = np.zeros((8, ny, nx), np.uint32)
    dist = np.zeros((8, ny, nx), np.int64)
    yy, xx = np.mgrid[0:ny, 0:nx]
    for k, (sx, sy) in enumerate(STEPS):
        if sy == 0:  # rows: transpose, so that the source lies above (sx = -1) or below (sx = +1)
            a = bits.T[::-1] if sx > 0 else bits.T
            c, t = _from_above(np.ascontiguousarray(a))
            if sx > 0:
                c, t = c[::-1], t[::-1]
            cand[k], dist[k] = c.T, t.T
            continue
        # the lines x - (sx * sy) * y = const become the columns of a sheared image, padded with holes
        s = sx * sy
        col = xx - s * yy + (ny - 1 if s > 0 else 0) if sx else xx
        sh = np.full((ny, nx + (ny - 1 if sx else 0)), hole, np.uint32)
        sh[yy, col] = bits
        if sy > 0:  # the source lies below: turn the image upside down
            c, t = _from_above(np.ascontiguousarray(sh[::-1]))
            c, t = c[::-1], t[::-1]
        else:
            c, t = _from_above(sh)
        cand[k], dist[k] = c[yy, col], t[yy, col]
    return cand, dist


def fill(d, mode="median", dirs=8, maxdist=0, r=None):
    """(out, filled), float32 [ny][nx].  r: rays(d), if the caller has them already."""
    if mode not in MODES or dirs not in (2, 4, 8) or maxdist < 0:
        raise ValueError("fill: mode median / min / max, dirs 2 / 4 / 8, maxdist >= 0")
    d = np.ascontiguousarray(d, np.float32)
    cand, dist = rays(d) if r is None else r
    cand, dist = cand[:dirs], dist[:dirs]
    has = dist >= 1
    if maxdist > 0:
        has &= dist <= maxdist
    hole = ~np.isfinite(d)
    n = has.sum(axis=0)
    # order by (missing, value, direction): np.lexsort is stable and its LAST key is the primary one; the value key compares as
    # IEEE (-0 == +0), so among equal values the direction index decides
    val = np.where(has, cand.view(np.float32), f32(0))
    k = np.broadcast_to(np.arange(dirs)[:, None, None], val.shape)
    order = np.lexsort((k, val, ~has), axis=0)
    srt = np.take_along_axis(cand, order, axis=0)
    pick = {"min": np.zeros_like(n), "max": np.maximum(n - 1, 0), "median": n // 2}[mode]
    chosen = np.take_along_axis(srt, pick[None], axis=0)[0]
    got = hole & (n >= 1)
    out = np.where(got, chosen, d.view(np.uint32)).astype(np.uint32).view(np.float32)
    return out, got.astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- crafted maps ------------------------------------------------------------------------------------------------------------
def nan_payload(payload):
    return np.array([0x7F800000 | payload], np.uint32).view(np.float32)[0]


def crafted(nx, ny, chunk=64, band=64, seed=0):
    """[(name, d)]: the maps the GPU kernels are held to, for one shape.  chunk, band: the row chunk and the band height of the
    kernels (plan_holes), which the seams of some patterns are placed by."""
    nan, inf = f32(np.nan), f32(np.inf)
    yy, xx = np.mgrid[0:ny, 0:nx]
    ramp = (1.0 + xx + 0.5 * yy).astype(np.float32)  # every pixel another value: a wrong source shows
    out = []

    def add(name, d):
        d = np.ascontiguousarray(d, np.float32)
        assert d.shape == (ny, nx), (name, d.shape)
        out.append((name, d))

    add("all_valid", ramp)
    add("all_nan", np.full((ny, nx), nan))
    for name, (x, y) in (("one_centre", (nx // 2, ny // 2)), ("one_top_left", (0, 0)), ("one_top_right", (nx - 1, 0)),
                         ("one_bottom_left", (0, ny - 1)), ("one_bottom_right", (nx - 1, ny - 1))):
        one = np.full((ny, nx), nan, np.float32)
        one[y, x] = 7.0
        add(name, one)
    add("hole_rows", np.where(yy % 3 == 1, nan, ramp))
    add("hole_columns", np.where(xx % 3 == 1, nan, ramp))
    add("hole_diagonals", np.where(((xx + yy) % 4 == 1) | ((xx - yy) % 5 == 2), nan, ramp))
    # one hole across a chunk seam and a band seam at once (as far as the shape reaches), valid pixels only outside it
    x0, x1 = max(min(chunk, nx) - 3, 1 if nx > 2 else 0), min(chunk + 3, nx - 1 if nx > 2 else nx)
    y0, y1 = max(min(band, ny) - 3, 1 if ny > 2 else 0), min(band + 3, ny - 1 if ny > 2 else ny)
    seam = ramp.copy()
    seam[y0:y1, x0:x1] = nan
    add("seam_hole", seam)
    add("checkerboard", np.where((xx + yy) % 2 == 0, ramp, nan))
    rng = np.random.default_rng(1000 * nx + ny + seed)
    levels = np.array([0.0, -0.0, 1.0, 2.5, 4.0], np.float32)
    for name, share in (("random_10", 0.1), ("random_90", 0.9)):
        rnd = rng.choice(levels, size=(ny, nx))
        rnd[rng.random((ny, nx)) < share] = nan
        add(name, rnd)
    # -0 / +0: the candidates of a hole compare equal, the direction index decides whose bits are written
    zeros = np.where((xx + 2 * yy) % 3 == 0, nan, np.where((xx + yy) % 2 == 0, f32(0.0), f32(-0.0))).astype(np.float32)
    add("zeros_of_both_signs", zeros)
    # NaNs with payloads and +-INF holes three rows deep between rows of valid pixels: under a small maxdist the middle rows keep
    # their bits; and a map with no valid pixel at all, where no ray reaches anything
    pay = np.where((xx + yy) % 2 == 0, ramp, nan).astype(np.float32)
    pay[yy % 8 < 3] = nan_payload(0x12345)   # three rows deep: the middle one is two steps from every valid pixel
    pay[(yy % 8 > 3) & (yy % 8 < 7) & (xx % 2 == 0)] = inf
    pay[(yy % 8 > 3) & (yy % 8 < 7) & (xx % 2 == 1)] = -inf
    add("payloads_and_infinities", pay)
    lost = np.full((ny, nx), nan_payload(0x2BCDE), np.float32)
    lost[(xx + yy) % 3 == 0] = inf
    lost[(xx + yy) % 3 == 1] = -inf
    add("unreachable_payloads", lost)
    return out


# ---- plan_holes on the host (tests/holes_plan_harness.cc) ------------------------------------------------------------------------
PLAN_OUT = ("family", "chunk", "band", "nbands", "walk_dirs", "planes", "grid_rows", "grid_walk", "grid_apply", "nlines", "carry_words",
            "scratch_bytes")


def plan_lib(tmpdir):
    so = os.path.join(str(tmpdir), "libholes_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mgm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "holes_plan_harness.cc"), "-o", so], check=True)
    return C.CDLL(so)


def plan(lib, rows):
    """rows: [(nx, ny, dirs, num_cu)] -> [dict of PLAN_OUT]"""
    req = np.ascontiguousarray(np.array(rows, dtype=np.int32).reshape(-1, 4))
    out = np.zeros((len(req), len(PLAN_OUT)), dtype=np.int64)
    lib.holes_plan(req.ctypes.data_as(C.c_void_p), C.c_int(len(req)), out.ctypes.data_as(C.c_void_p))
    return [dict(zip(PLAN_OUT, r)) for r in out.tolist()]
