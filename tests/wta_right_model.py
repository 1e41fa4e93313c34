"""numpy model of "right from left" (DESIGN.md 7b): the right view's winners read out of the LEFT run's corrected
aggregated volume S along its diagonals.

    S_R(y, xr, oR) = S(y, xr + e, L-1-oR),  e = oR - dmax,  +INF where xr + e lies outside the left image
    winner         = first strict minimum among the finite entries of S_R(y, xr, .) by rising oR (mgm_core.cc:592-609)
    out, outcost   = (float)e, that value;  NaN, +INF when no entry is finite
    vfit           = VfitMinimum (refine.h:70-92) on S_R(oR-1), S_R(oR), S_R(oR+1) under the gate of mgm_refine.h:58 in the
                     right index, every operation in float32 and in the formula's order
"""
import numpy as np

f32 = np.float32


def right_volume(S, dmin, vnx):
    """S [ny][nx][L] over labels dmin..dmin+L-1 -> S_R [ny][vnx][L] over labels -dmax..-dmin, by index arithmetic."""
    S = np.asarray(S, np.float32)
    ny, nx, L = S.shape
    dmax = dmin + L - 1
    xr = np.arange(vnx)[:, None]
    oR = np.arange(L)[None, :]
    x = xr + oR - dmax
    ok = (x >= 0) & (x < nx)
    o = np.broadcast_to(L - 1 - oR, x.shape)
    SR = np.full((ny, vnx, L), np.inf, np.float32)
    SR[:, ok] = S[:, x[ok], o[ok]]
    return SR


def vfit(v0, v1, v2):
    """refine.h:70-92 on float32 scalars: (v_min, x_min)."""
    v0, v1, v2 = f32(v0), f32(v1), f32(v2)
    if v1 > v0 and v1 > v2:
        return v1, f32(0)
    with np.errstate(all="ignore"):
        slope = f32(v2 - v1)
        if f32(v2 - v1) < f32(v0 - v1):
            slope = f32(v0 - v1)
        x_min = f32(f32(v0 - v2) / f32(f32(2) * slope))
        v_min = f32(v2 + f32(f32(x_min - f32(1)) * slope))
    return v_min, x_min


def wta_right(S, dmin, vnx, refine=None):
    """(out, outcost), float32 [ny][vnx], of the definition above; refine None / "none" / "vfit"."""
    if refine not in (None, "none", "vfit"):
        raise ValueError("right from left: refinement none or vfit only")
    SR = right_volume(S, dmin, vnx)
    ny, _, L = SR.shape
    dmax = dmin + L - 1
    fin = np.isfinite(SR)
    masked = np.where(fin, SR, f32(np.inf))
    arg = np.argmin(masked, axis=2)  # the first of equal minima = the first strict minimum
    has = fin.any(axis=2)
    out = np.where(has, (arg - dmax).astype(np.float32), f32(np.nan)).astype(np.float32)
    cost = np.where(has, np.take_along_axis(masked, arg[..., None], 2)[..., 0], f32(np.inf)).astype(np.float32)
    if refine == "vfit":
        for y in range(ny):
            for xr in range(vnx):
                oR = int(arg[y, xr])
                if has[y, xr] and oR - 1 >= 0 and oR + 2 <= L - 1:  # mgm_refine.h:58
                    vmin, dx = vfit(SR[y, xr, oR - 1], SR[y, xr, oR], SR[y, xr, oR + 1])
                    with np.errstate(all="ignore"):
                        out[y, xr] = f32(f32(oR - dmax) + dx)
                    cost[y, xr] = vmin
    return out, cost
