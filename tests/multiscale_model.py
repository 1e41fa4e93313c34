"""numpy restatement of the coarse-to-fine (multiscale) mode -- TEST INFRASTRUCTURE ONLY.

The reference has no multiscale program; the definition is the project's own (DESIGN.md "multiscale"), made of reference
steps plus three resampling rules.  This file states it once more, from that definition and the reference lines it cites,
on top of the CPU oracle (oracle.oracle.Oracle: costvolume_ranged, mgm_ranged, refine_ranged, weights) and oracle.post:

  levels            n_{s+1} = (n_s + 1) // 2 for nx, ny, vnx, vny; the effective count is the largest S <= nscales whose
                    coarsest level still has min(nx, ny, vnx, vny) >= 16 (at least 1); nscales outside 1..8 is an error
  zoom_out          out(x,y) = ((a + b) + (c + d)) * 0.25f over the 2x2 block at (2x, 2y), indices clamped (fp32)
  ranges_zoom_out   lo' = floorf(0.5f * min lo), hi' = ceilf(0.5f * max hi) over the same four pixels
  prior -> ranges   U(x,y) = 2.0f * D(x >> 1, y >> 1), then update_dmin_dmax (mgm.cc:120-158) and the two
                    remove_nonfinite_values_Img calls (mgm.cc:387-388) on the level's base ranges
  per level         what main() does for a pair (mgm.cc:372-423) with range images for both runs
"""
import numpy as np

from oracle import oracle as orc_mod
from oracle import post

F = np.float32


# ---- level arithmetic ------------------------------------------------------------------------------------------------
def half(n):
    return (n + 1) // 2


def levels(nx, ny, vnx, vny, nscales):
    """[(nx, ny, vnx, vny)] of the levels that run, full size first; None for a request outside 1..8."""
    if not 1 <= nscales <= 8 or min(nx, ny, vnx, vny) < 1:
        return None
    out = [(nx, ny, vnx, vny)]
    while len(out) < nscales:
        nxt = tuple(half(n) for n in out[-1])
        if min(nxt) < 16:
            break
        out.append(nxt)
    return out


# ---- the three resampling rules --------------------------------------------------------------------------------------
def _blocks(a):
    """The four samples of every 2x2 block of a (..., ny, nx) array, indices clamped at the far border."""
    ny, nx = a.shape[-2:]
    y0, x0 = np.arange(half(ny)) * 2, np.arange(half(nx)) * 2
    y1, x1 = np.minimum(y0 + 1, ny - 1), np.minimum(x0 + 1, nx - 1)
    g = lambda ys, xs: a[..., ys[:, None], xs[None, :]]
    return g(y0, x0), g(y0, x1), g(y1, x0), g(y1, x1)


def zoom_out(img):
    a, b, c, d = _blocks(np.asarray(img, F))
    return ((a + b) + (c + d)) * F(0.25)


def ranges_zoom_out(lo, hi):
    l4, h4 = _blocks(np.asarray(lo, F)), _blocks(np.asarray(hi, F))
    mn = np.minimum(np.minimum(l4[0], l4[1]), np.minimum(l4[2], l4[3]))
    mx = np.maximum(np.maximum(h4[0], h4[1]), np.maximum(h4[2], h4[3]))
    return np.floor(F(0.5) * mn).astype(F), np.ceil(F(0.5) * mx).astype(F)


def zoom_in_prior(D, nx, ny):
    """U(x,y) = 2.0f * D(x >> 1, y >> 1) at the fine level's size."""
    D = np.asarray(D, F)
    return (F(2.0) * D[(np.arange(ny) >> 1)[:, None], (np.arange(nx) >> 1)[None, :]]).astype(F)


def image_minmax(u):
    """img_tools.h:183-199: the finite minimum / maximum, (+INF, -INF) when nothing is finite."""
    fin = u[np.isfinite(u)]
    return (F(fin.min()), F(fin.max())) if fin.size else (F(np.inf), F(-np.inf))


def update_dmin_dmax(U, lo, hi, slack=3, radius=2):
    """mgm.cc:120-158 followed by remove_nonfinite_values_Img(dminI, gmin), (dmaxI, gmax) (mgm.cc:387-388)."""
    U, lo, hi = np.asarray(U, F), np.array(lo, F, copy=True), np.array(hi, F, copy=True)
    ny, nx = U.shape
    gmin, gmax = image_minmax(U)
    sl = F(abs(int(slack)))
    fin = np.isfinite(U)
    with np.errstate(invalid="ignore"):
        a = np.where(fin, U - sl, gmin - sl).astype(F)  # (v - slack: float - int in float)
        b = np.where(fin, U + sl, gmax + sl).astype(F)
    r = int(radius)
    ap = np.pad(a, r, mode="edge")  # valneumann
    bp = np.pad(b, r, mode="edge")
    dmin = np.full((ny, nx), np.inf, F)
    dmax = np.full((ny, nx), -np.inf, F)
    for dj in range(2 * r + 1):
        for di in range(2 * r + 1):
            dmin = np.minimum(dmin, ap[dj:dj + ny, di:di + nx])
            dmax = np.maximum(dmax, bp[dj:dj + ny, di:di + nx])
    ok = np.isfinite(dmin)
    lo[ok], hi[ok] = dmin[ok], dmax[ok]
    lo[~np.isfinite(lo)] = gmin
    hi[~np.isfinite(hi)] = gmax
    return lo, hi


def ranges_from_coarse(D, lo, hi, slack=3, radius=2):
    """The prior -> ranges step as the definition states it: zoom the coarse map in, then update_dmin_dmax."""
    ny, nx = np.asarray(lo).shape
    return update_dmin_dmax(zoom_in_prior(D, nx, ny), lo, hi, slack, radius)


def ranges_from_coarse_fused(D, lo, hi, slack=3, radius=2):
    """The same, reading only the coarse map: the (2r+1)^2 clamped window of fine pixel (i, j) covers the rectangle of
    coarse pixels [clamp(i-r) >> 1, clamp(i+r) >> 1] x [clamp(j-r) >> 1, clamp(j+r) >> 1].  Plain loops: small maps."""
    D, lo, hi = np.asarray(D, F), np.array(lo, F, copy=True), np.array(hi, F, copy=True)
    ny, nx = lo.shape
    g = image_minmax(D)
    gmin, gmax = F(2.0) * g[0], F(2.0) * g[1]
    sl, r = F(abs(int(slack))), int(radius)
    U = (F(2.0) * D).astype(F)
    fin = np.isfinite(U)
    with np.errstate(invalid="ignore"):
        a = np.where(fin, U - sl, gmin - sl).astype(F)
        b = np.where(fin, U + sl, gmax + sl).astype(F)
    for j in range(ny):
        y0, y1 = max(j - r, 0) >> 1, min(j + r, ny - 1) >> 1
        for i in range(nx):
            x0, x1 = max(i - r, 0) >> 1, min(i + r, nx - 1) >> 1
            m, M = a[y0:y1 + 1, x0:x1 + 1].min(), b[y0:y1 + 1, x0:x1 + 1].max()
            if np.isfinite(m):
                lo[j, i], hi[j, i] = m, M
    lo[~np.isfinite(lo)] = gmin
    hi[~np.isfinite(hi)] = gmax
    return lo, hi


def int_hull(lo, hi):
    ilo, ihi = orc_mod.int_ranges(lo, hi)
    return int(ilo.min()), int(ihi.max())


# ---- main()'s post-processing, vectorised (oracle.post has the plain-loop forms; test_multiscale_model pins one on the other)
def leftright(d, other, tau):
    """leftright_test, mgm.cc:68-91 (see oracle.post.leftright for the non-finite cases)."""
    d, other = np.asarray(d, F), np.asarray(other, F)
    ny, nx = d.shape
    x = np.arange(nx, dtype=F)[None, :].repeat(ny, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        r = post.c_round((x + d).astype(np.float64))
        ok = np.isfinite(r) & (r >= -2147483648.0) & (r <= 2147483647.0)
        Lx = np.where(ok, r, -1).astype(np.int64)
        ok &= (Lx >= 0) & (Lx < other.shape[1])
        Li = np.where(ok, Lx, 0)
        rows = np.minimum(np.arange(ny), other.shape[0] - 1)[:, None].repeat(nx, 1)
        Rx = (Li.astype(F) + other[rows, Li]).astype(F)
        ok &= ~(np.abs((Rx - x).astype(F).astype(np.float64)) > np.float64(F(tau)))
    return np.where(ok, d, F(np.nan)).astype(F)


# ---- one run of one level: mgm.cc:376-396 with range images ----------------------------------------------------------
def run_level(oracle, U, V, lo, hi, prm):
    """U, V: (nch, ny, nx) / (nch, vny, vnx); lo, hi: float range images of U's size.  Returns (disparity, cost) after
    the iterations and MEDIAN, before any left-right test."""
    ny, nx = lo.shape
    it = prm["iterations"]
    if it <= 0:  # mgm() is never called: the maps keep the zeros they were allocated with (mgm.cc:360-365)
        out, cost = np.zeros((ny, nx), F), np.zeros((ny, nx), F)
    else:
        ilo, ihi = orc_mod.int_ranges(lo, hi)
        hmin, hmax = int(ilo.min()), int(ihi.max())
        C = oracle.costvolume_ranged(U, V, ilo, ihi, hmin, hmax, prm["prefilter"], prm["distance"], prm["truncDist"], prm["census_win"])
        w8 = oracle.weights(U, prm["aP2"], prm["aThresh"]) if prm["aP2"] != 1.0 else None
        refine = prm["refine"] or "none"
        args = (prm["P1"], prm["P2"], prm["NDIR"], prm["TSGM"], prm["use_fh"], prm["fix_overcount"], w8)
        S, out, cost = oracle.mgm_ranged(C, hmin, ilo, ihi, *args)
        refining = refine in ("vfit", "parabola", "cubic", "parabolaOCV")  # any other name: none (mgm_refine.h:28-35)
        if refining:
            out, cost = oracle.refine_ranged(S, hmin, ilo, ihi, refine, out, cost)
        wl, wh = lo, hi
        for _ in range(1, it):  # mgm.cc:377-388: the volume stays, mgm() is called with the narrowed ranges
            wl, wh = update_dmin_dmax(out, wl, wh, 3, 2)
            slo, shi = orc_mod.int_ranges(wl, wh)
            shmin, shmax = int(slo.min()), int(shi.max())
            S, out, cost = oracle.mgm_ranged(C, hmin, ilo, ihi, *args, srange=(slo, shi, shmin, shmax))
            if refining:
                out, cost = oracle.refine_ranged(S, shmin, slo, shi, refine, out, cost)
    if prm["median"]:
        out = post.median(out, int(prm["median"]))
    return out, cost


DEFAULTS = dict(P1=8.0, P2=32.0, NDIR=4, TSGM=4, use_fh=0, fix_overcount=1, aP2=1.0, aThresh=5.0, prefilter="none", distance="ad",
                truncDist=np.inf, census_win=3, refine="none", iterations=1, median=0, testlrrl=1, tau=1.0, slack=3, radius=2)


def multiscale_pair(oracle, u, v, dmin, dmax, nscales, lo=None, hi=None, **params):
    """The whole mode.  u, v: (nch, ny, nx) NaN-free float32; P1 / P2 as given (already times the channel count).
    Returns dict(outL, costL, outR, costR, nolr, levels=[per level: dims, (lo, hi) per run]); outR / costR None without
    the left-right test."""
    prm = dict(DEFAULTS, **params)
    u, v = np.asarray(u, F), np.asarray(v, F)
    if u.ndim == 2:
        u, v = u[None], v[None]
    _, ny, nx = u.shape
    _, vny, vnx = v.shape
    lv = levels(nx, ny, vnx, vny, nscales)
    if lv is None:
        raise ValueError("nscales must be 1..8")
    S = len(lv)
    us, vs = [u], [v]
    base = [[(np.full((ny, nx), dmin, F) if lo is None else np.asarray(lo, F).reshape(ny, nx),
              np.full((ny, nx), dmax, F) if hi is None else np.asarray(hi, F).reshape(ny, nx))],
            [(np.full((vny, vnx), -dmax, F), np.full((vny, vnx), -dmin, F))]]  # mgm.cc:368
    for s in range(1, S):
        us.append(zoom_out(us[-1]))
        vs.append(zoom_out(vs[-1]))
        for k in range(2):
            base[k].append(ranges_zoom_out(*base[k][-1]))
    nrun = 2 if prm["testlrrl"] else 1
    prev = [None, None]
    info = [None] * S
    res = None
    for s in range(S - 1, -1, -1):
        maps, costs, used = [], [], []
        for k in range(nrun):
            U, V = (us[s], vs[s]) if k == 0 else (vs[s], us[s])
            rl, rh = base[k][s]
            if s < S - 1:
                rl, rh = ranges_from_coarse(prev[k], rl, rh, prm["slack"], prm["radius"])
            o, c = run_level(oracle, U, V, rl, rh, prm)
            maps.append(o), costs.append(c), used.append((rl, rh))
        nolr = maps[0]
        if nrun == 2:  # mgm.cc:420-423: both tests on copies of the unchecked maps
            maps = [leftright(maps[0], maps[1], prm["tau"]), leftright(maps[1], maps[0], prm["tau"])]
        prev = maps
        info[s] = dict(dims=lv[s], ranges=used)
        res = dict(outL=maps[0], costL=costs[0], outR=maps[1] if nrun == 2 else None, costR=costs[1] if nrun == 2 else None, nolr=nolr)
    res["levels"] = info
    return res
