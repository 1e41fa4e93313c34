"""numpy model of hole classification and the classified fill, float32 throughout and bit for bit, the planted scene
of its tests and plan_holes_classify on the host.

    cls(x,y)  0 where d(x,y) is finite; at a hole 2 (a mismatch) iff an integer xr exists with max(0, x+dmin) <= xr <= min(vnx-1, x+dmax),
              other(xr,y) finite and fabsf(((float)xr + other(xr,y)) - (float)x) <= tau; else 1 (an occlusion)
    fill      holes_model.fill's candidates and ordering; a hole with cls == 1 takes mode_occ, every other hole mode_mis;
              seclow = v[min(1, n-1)], sechigh = v[max(n-2, 0)]

Vectorised: classify loops over the labels (only those that can land inside `other`), every pixel of the map at once.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from holes_model import ROOT, rays

f32 = np.float32
MODES5 = ("median", "min", "max", "seclow", "sechigh")


def classify(d, other, dmin, dmax, tau):
    """cls, float32 [ny][nx].  d [ny][nx], other [ny][vnx]."""
    d, other = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(other, np.float32)
    (ny, nx), (vny, vnx) = d.shape, other.shape
    if vny != ny or dmin > dmax or not (np.isfinite(tau) and tau >= 0):
        raise ValueError("classify: one height, dmin <= dmax, tau finite and >= 0")
    tau = f32(tau)
    x = np.arange(nx, dtype=np.int64)
    fx = x.astype(np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        land = np.where(np.isfinite(other), np.arange(vnx, dtype=np.int64).astype(np.float32)[None, :] + other, f32(np.nan)).astype(np.float32)
        match = np.zeros((ny, nx), bool)
        for delta in range(max(dmin, -(nx - 1)), min(dmax, vnx - 1) + 1):  # (the other labels land outside `other` for every x)
            xr = x + delta
            ok = (xr >= 0) & (xr < vnx)
            a = land[:, np.clip(xr, 0, vnx - 1)]
            match |= ok[None, :] & (np.abs((a - fx[None, :]).astype(np.float32)) <= tau)
    hole = ~np.isfinite(d)
    return np.where(hole, np.where(match, f32(2), f32(1)), f32(0)).astype(np.float32)


def _pick(mode, n):
    return {"min": np.zeros_like(n), "max": np.maximum(n - 1, 0), "median": n // 2, "seclow": np.minimum(1, np.maximum(n - 1, 0)),
            "sechigh": np.maximum(n - 2, 0)}[mode]


def fill_classified(d, cls, mode_occ, mode_mis, dirs=8, maxdist=0, r=None):
    """(out, filled), float32 [ny][nx].  r: holes_model.rays(d), if the caller has them already."""
    if mode_occ not in MODES5 or mode_mis not in MODES5 or dirs not in (2, 4, 8) or maxdist < 0:
        raise ValueError("fill_classified: modes median / min / max / seclow / sechigh, dirs 2 / 4 / 8, maxdist >= 0")
    d, cls = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(cls, np.float32)
    cand, dist = rays(d) if r is None else r
    cand, dist = cand[:dirs], dist[:dirs]
    has = dist >= 1
    if maxdist > 0:
        has &= dist <= maxdist
    hole = ~np.isfinite(d)
    n = has.sum(axis=0)
    val = np.where(has, cand.view(np.float32), f32(0))
    k = np.broadcast_to(np.arange(dirs)[:, None, None], val.shape)
    order = np.lexsort((k, val, ~has), axis=0)  # by (missing, value, direction): holes_model.fill's ordering
    srt = np.take_along_axis(cand, order, axis=0)
    with np.errstate(invalid="ignore"):
        pick = np.where(cls == f32(1), _pick(mode_occ, n), _pick(mode_mis, n))
    chosen = np.take_along_axis(srt, pick[None], axis=0)[0]
    got = hole & (n >= 1)
    out = np.where(got, chosen, d.view(np.uint32)).astype(np.uint32).view(np.float32)
    return out, got.astype(np.float32)


# ---- crafted inputs ---------------------------------------------------------------------------------------------------------------
RANGES = ((0, 0), (3, 9), (-9, -3), (-300, 300), (60, 66))  # (60, 66): wholly outside `other` for the right part of every row
TAUS = (0.0, 0.5, 1.0, 2.5)


def crafted_other(nx, ny, vnx, dmin, dmax, tau, seed=0):
    """other [ny][vnx]: most pixels point back into the map (other = -(a label of the range) + a small offset, among them +-tau and
    +-(tau + 0.5)); NaN, +-INF, +-1e30, FLT_MAX and -0 are sprinkled over it; and per row up to six planted pairs (x, xr) whose
    landing coordinate lies exactly tau from x, and one ulp of `other` to either side of that (next to xr = 0 the ulp survives the
    addition; further right it is rounded away, which the definition's float arithmetic must reproduce)."""
    rng = np.random.default_rng(100003 * nx + 1009 * ny + 17 * vnx + 7 * (dmin % 1000) + int(4 * tau) + seed)
    tau = f32(tau)
    lab = rng.integers(max(dmin, -nx), min(dmax, vnx) + 1, size=(ny, vnx)) if max(dmin, -nx) <= min(dmax, vnx) else np.zeros((ny, vnx), np.int64)
    offs = np.array([0, 0, 0.25, -0.25, tau, -tau, tau + f32(0.5), -tau - f32(0.5), 3.0], np.float32)
    other = (-lab).astype(np.float32) + rng.choice(offs, size=(ny, vnx))
    odd = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, np.finfo(np.float32).max, -0.0], np.float32)
    m = rng.random((ny, vnx)) < 0.15
    other[m] = rng.choice(odd, size=int(m.sum()))
    for y in range(ny):
        for k in range(6):
            x = int(rng.integers(0, nx))
            lo, hi = max(0, x + dmin), min(vnx - 1, x + dmax)
            if lo > hi:
                continue
            xr = lo if k < 3 else int(rng.integers(lo, hi + 1))
            exact = f32(f32(x) + (tau if k % 2 else -tau)) - f32(xr)
            other[y, xr] = (exact, np.nextafter(exact, f32(np.inf)), np.nextafter(exact, f32(-np.inf)))[k % 3]
    return np.ascontiguousarray(other, np.float32)


def crafted_d(nx, ny, seg=256, lane=64, seed=0):
    """[(name, d)]: all holes, no holes, holes on every segment and lane boundary (first and last pixel of every `lane`, and so of
    every `seg`), random holes (NaN, +-INF) over a ramp."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    ramp = (-1.0 - (xx % 7) - 0.5 * (yy % 3)).astype(np.float32)
    nan = f32(np.nan)
    assert seg % lane == 0
    rng = np.random.default_rng(31 * nx + ny + seed)
    rnd = ramp.copy()
    rnd[rng.random((ny, nx)) < 0.3] = nan
    rnd[rng.random((ny, nx)) < 0.03] = np.inf
    rnd[rng.random((ny, nx)) < 0.03] = -np.inf
    return [("all_holes", np.full((ny, nx), nan, np.float32)), ("no_holes", ramp),
            ("boundaries", np.where((xx % lane == 0) | (xx % lane == lane - 1) | (xx == nx - 1), nan, ramp).astype(np.float32)), ("random", rnd)]


# ---- the planted scene -----------------------------------------------------------------------------------------------------------
SCENE = dict(nx=96, ny=24, bg=-2.0, fg=-9.0, x0=40, x1=60, y0=6, y1=17, dmin=-16, dmax=0, share=0.10, seed=7, fill_dist=6)
# fill_dist: the distance bound at which the plain median and the background rule part on this scene -- one less than the occluded
# strip's width (7 columns) and equal to the rows of background above / below the block's middle rows; the reasoning is spelt out in
# tests/test_occlusion_model.py::test_planted_scene_background_fills_the_strip


def planted_scene(wedge=False):
    """(left, right, holes, occluded, strip): the full left map (background bg, a foreground block fg); the right map it forward-maps
    to, right(x + d) = -d with the foreground winning, NaN where nothing lands; the left map with its truly occluded pixels and a
    seeded share of the others set to NaN; the mask of the occluded pixels; the mask of those beside the block's edge.
    wedge: another foreground, whose left edge is a wedge of background that points into it (x >= 54 - 2 |y - 11| on rows 4..18):
    an occluded pixel inside the wedge sees foreground along most of its rays."""
    s = SCENE
    nx, ny = s["nx"], s["ny"]
    left = np.full((ny, nx), f32(s["bg"]), np.float32)
    if wedge:
        for y in range(2, 22):
            left[y, (54 - 2 * abs(y - 11) if 4 <= y <= 18 else 40):75] = f32(s["fg"])
    else:
        left[s["y0"]:s["y1"] + 1, s["x0"]:s["x1"] + 1] = f32(s["fg"])
    right = np.full((ny, nx), f32(np.nan), np.float32)
    owner = np.full((ny, nx), -1, np.int64)  # the left x whose value a right pixel holds
    for y in range(ny):
        for fg_turn in (False, True):  # the foreground is written last: it wins
            for x in range(nx):
                dd = left[y, x]
                if (dd == f32(s["fg"])) != fg_turn:
                    continue
                xr = x + int(dd)
                if 0 <= xr < nx:
                    right[y, xr], owner[y, xr] = -dd, x
    yy, xx = np.mgrid[0:ny, 0:nx]
    xr = xx + left.astype(np.int64)
    inside = (xr >= 0) & (xr < nx)
    occluded = ~inside | (owner[yy, np.clip(xr, 0, nx - 1)] != xx)
    strip = occluded & inside
    rng = np.random.default_rng(s["seed"])
    planted = ~occluded & (rng.random((ny, nx)) < s["share"])
    holes = left.copy()
    holes[occluded | planted] = np.nan
    return left, right, holes, occluded, strip


# ---- plan_holes_classify on the host (tests/holes_classify_plan_harness.cc) ---------------------------------------------------------
PLAN_OUT = ("family", "seg", "span", "grid_x", "grid_y", "lds_bytes")


def plan_lib(tmpdir):
    so = os.path.join(str(tmpdir), "libholes_classify_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mgm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "holes_classify_plan_harness.cc"), "-o", so], check=True)
    return C.CDLL(so)


def plan(lib, rows):
    """rows: [(nx, ny, vnx, L, num_cu)] -> [dict of PLAN_OUT]"""
    req = np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(-1, 5))
    out = np.zeros((len(req), len(PLAN_OUT)), dtype=np.int64)
    lib.holes_classify_plan(req.ctypes.data_as(C.c_void_p), C.c_int(len(req)), out.ctypes.data_as(C.c_void_p))
    return [dict(zip(PLAN_OUT, r)) for r in out.tolist()]
