"""numpy model of sub-pixel label spacing, float32 throughout and bit for bit, over the CPU oracle.

    phase image  v_0 = v.  k > 0, t = k/s, per channel and row, columns clamped to [0, vnx-1], every product rounded and the sums
                 in the order written (numpy float32 arithmetic does not contract):
                   linear  v_k(x) = (1-t)*v(x) + t*v(x+1)
                   cubic   v_k(x) = ((w0*v(x-1) + w1*v(x)) + w2*v(x+1)) + w3*v(x+2)      Keys, a = -1/2
    phase volume C_k = the oracle's cost volume of (u, v_k) over [dmin, dmax], its "no finite cost => zeros" rule included
    fine volume  F(y,x,o') = C_{o' mod s}(y,x,o' div s), o' = 0 .. s*(dmax-dmin); fine label s*dmin + o' stands for (s*dmin + o')/s
    maps         mgm / refinement on F as on any dense volume, then out / s

NaN results: the PLACES of NaNs are the definition's; which NaN (sign, payload) an invalid operation or an operand's payload gives
differs between processors, so comparisons treat NaNs as equal (same_bits: the convention of the oracle's bits_equal).
"""
import ctypes as C
import os
import subprocess

import numpy as np

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERPS = ("linear", "cubic")
# Keys' weights (a = -1/2) at t = 1/4, 1/2, 3/4: all exact in fp32
KEYS = {1: (-9 / 128, 111 / 128, 29 / 128, -3 / 128), 2: (-1 / 16, 9 / 16, 9 / 16, -1 / 16), 3: (-3 / 128, 29 / 128, 111 / 128, -9 / 128)}
PHASES = [(s, k) for s in (1, 2, 4) for k in range(s)]


def weights(s, k, interp):
    """(w0, w1, w2, w3) of v(x-1), v(x), v(x+1), v(x+2) as float32; linear uses w1 and w2 alone."""
    if s not in (1, 2, 4) or not 0 <= k < s or interp not in INTERPS:
        raise ValueError("weights: s 1 / 2 / 4, k 0..s-1, interp linear / cubic")
    q = k * (4 // s)  # quarters
    if q == 0:
        return f32(0), f32(1), f32(0), f32(0)
    if interp == "cubic":
        return tuple(f32(w) for w in KEYS[q])
    t = f32(0.25) * f32(q)
    return f32(0), f32(1) - t, t, f32(0)


def phase_image(v, s, k, interp="cubic"):
    """v_k: float32 of v's shape ((nch,) ny, nx)."""
    v = np.ascontiguousarray(v, np.float32)
    w0, w1, w2, w3 = weights(s, k, interp)
    if k == 0:
        return v.copy()
    nx = v.shape[-1]
    x = np.arange(nx)
    at = lambda off: v[..., np.clip(x + off, 0, nx - 1)]
    with np.errstate(all="ignore"):
        if interp == "linear":
            return (w1 * at(0) + w2 * at(1)).astype(np.float32)
        return (((w0 * at(-1) + w1 * at(0)) + w2 * at(1)) + w3 * at(2)).astype(np.float32)


def phase_pixel(row, x, s, k, interp="cubic"):
    """The same arithmetic for ONE pixel of one row, in scalars: the restatement tests/test_subpix_model.py holds phase_image to."""
    n = len(row)
    px = lambda i: f32(row[min(max(i, 0), n - 1)])
    if k == 0:
        return f32(row[x])
    w0, w1, w2, w3 = weights(s, k, interp)
    with np.errstate(all="ignore"):
        if interp == "linear":
            a, b = f32(w1 * px(x)), f32(w2 * px(x + 1))
            return f32(a + b)
        p0, p1, p2, p3 = f32(w0 * px(x - 1)), f32(w1 * px(x)), f32(w2 * px(x + 1)), f32(w3 * px(x + 2))
        return f32(f32(f32(p0 + p1) + p2) + p3)


def phase_volumes(orc, u, v, dmin, dmax, s, interp="cubic", prefilter="none", distance="ad", truncDist=np.inf, census_win=3):
    return [orc.costvolume(u, phase_image(v, s, k, interp), dmin, dmax, prefilter, distance, truncDist, census_win) for k in range(s)]


def interleave(phases):
    """[C_0 .. C_{s-1}] of (ny, nx, L) -> F (ny, nx, s*(L-1)+1); label L-1 of the phases k > 0 is dropped."""
    s = len(phases)
    ny, nx, L = phases[0].shape
    F = np.empty((ny, nx, s * (L - 1) + 1), np.float32)
    for k, Ck in enumerate(phases):
        F[:, :, k::s] = Ck[:, :, :L if k == 0 else L - 1]
    return F


def fine_volume(orc, u, v, dmin, dmax, s, interp="cubic", prefilter="none", distance="ad", truncDist=np.inf, census_win=3):
    """F over the fine labels s*dmin .. s*dmax."""
    return interleave(phase_volumes(orc, u, v, dmin, dmax, s, interp, prefilter, distance, truncDist, census_win))


def scale(m, s):
    with np.errstate(all="ignore"):
        return (np.ascontiguousarray(m, np.float32) / f32(s)).astype(np.float32)


def run(orc, u, v, dmin, dmax, s, interp, P1, P2, NDIR, TSGM, use_fh=0, fix=1, refine="none", prefilter="none", distance="ad",
        truncDist=np.inf, census_win=3):
    """One run of the model chain: (map in pixels, cost map, F)."""
    F = fine_volume(orc, u, v, dmin, dmax, s, interp, prefilter, distance, truncDist, census_win)
    S, out, cost = orc.mgm(F, s * dmin, P1, P2, NDIR, TSGM, use_fh, fix)
    if refine and refine != "none":
        out, cost = orc.refine(S, s * dmin, refine, out, cost)
    return scale(out, s), cost, F


def pair(orc, post, u, v, dmin, dmax, s, interp, P1, P2, NDIR, TSGM, use_fh=0, fix=1, refine="none", tau=1.0, median=0, **cost):
    """The model of Context.pair_subpix and of the command line: (checked left, left, right, left cost).  post: oracle.post."""
    L, costL, _ = run(orc, u, v, dmin, dmax, s, interp, P1, P2, NDIR, TSGM, use_fh, fix, refine, **cost)
    R, _, _ = run(orc, v, u, -dmax, -dmin, s, interp, P1, P2, NDIR, TSGM, use_fh, fix, refine, **cost)
    if median:
        L, R = post.median(L, median), post.median(R, median)
    return post.leftright(L, R, tau), L, R, costL


def same_bits(a, b):
    """Bit for bit, NaNs equal to one another (see the module's note)."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- the scene of "what the mode buys" (tests/test_subpix_model.py) ------------------------------------------------
def slanted_scene(nx=72, ny=12, step=3, d0=-24, seed=7):
    """(u, v, gt, dmin, dmax): v a textured image, u(x) = v(x + gt(x)) with gt = D/4, D = d0 + x // step -- a plane whose true disparity
    takes every quarter-pixel value in turn, one more quarter every `step` columns -- sampled with the model's own cubic at s = 4, so
    that the fine label D of s = 4 matches u exactly.  gt is (ny, nx) float32, in pixels."""
    rng = np.random.default_rng(seed)
    wide = nx + 16
    tex = rng.integers(0, 256, (ny, wide)).astype(np.float32)
    # a texture that a cubic samples faithfully: three taps of smoothing over white noise
    tex = ((tex + np.roll(tex, 1, 1)) + np.roll(tex, -1, 1)) / f32(3)
    v = np.ascontiguousarray(np.rint(tex)[None, :, :nx], np.float32)
    ph = [phase_image(v, 4, k, "cubic") for k in range(4)]
    x = np.arange(nx)
    D = d0 + x // step
    src = x + D // 4  # floor: D = 4 * (D // 4) + (D % 4)
    u = np.zeros_like(v)
    inside = (src >= 0) & (src < nx)
    for k in range(4):
        m = inside & (D % 4 == k)
        u[0][:, m] = ph[k][0][:, src[m]]
    gt = np.broadcast_to((D / 4.0).astype(np.float32)[None], (ny, nx)).copy()
    gt[:, ~inside] = np.nan
    dmin, dmax = int(np.floor(D.min() / 4)) - 2, int(np.ceil(D.max() / 4)) + 2
    return u, v, gt, dmin, dmax


# ---- plan_subpix on the host (tests/subpix_plan_harness.cc) ------------------------------------------------------------------------
PLAN_OUT = ("family", "grid", "pix", "vec", "chunks")


def plan_lib(tmpdir):
    so = os.path.join(str(tmpdir), "libsubpix_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "mgm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "subpix_plan_harness.cc"), "-o", so], check=True)
    return C.CDLL(so)


def plan(lib, rows):
    """rows: [(npix, labels, slots, in_slots, s, cb, num_cu)] -> [dict of PLAN_OUT]"""
    req = np.ascontiguousarray(np.array(rows, dtype=np.int64).reshape(-1, 7))
    out = np.zeros((len(req), len(PLAN_OUT)), dtype=np.int64)
    lib.subpix_plan(req.ctypes.data_as(C.c_void_p), C.c_int(len(req)), out.ctypes.data_as(C.c_void_p))
    return [dict(zip(PLAN_OUT, r)) for r in out.tolist()]
