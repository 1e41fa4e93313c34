"""numpy model of the solution energy, float32 throughout, one rounding per operation.

    C(p, l)    the cost of label l at pixel p; +INF where the pixel does not own it: outside the volume, outside lo..hi of a ragged
               volume, and for a d that is not finite or has |d| >= 2^24
    kinds 0-2  evaluate_energy_4connected (mgm_print_energy.h:17-96): G = 0 + C(p, (int)o), then for t = 0..3, r = p + dir[t],
               q = p + dir[t+1], dirs (-1,0) (0,1) (1,0) (0,-1) (-1,0), both inside the image:
                 0  G += (|o_r - o| <= 1 ? P1 : P2) / 4     1  G += |o_r - o| / 4     2  G += sqrt((o_r - o)^2 + (o_q - o)^2) / 4
    kind 3     the model energy: data = C(p, (int)rint(d)); for the first 4 or 8 neighbours in the order W E S N NW NE SE SW that lie
               inside the image and are finite: a = |d_q - d_p|, w = w8[k](p) or 1,
                 Hirschmueller  V = a == 0 ? 0 : a <= 1 ? fmin(P1*w, P2*w) : P2*w        FH  V = fmin((P1*w)*a, P2*w)
               smooth = 0.5 * (((0 + V_k0) + V_k1) + ...), E = data + smooth; E = NaN where d is not finite
    totals     serial = np.cumsum(E, dtype=float32)[-1]: the fp32 sum in raster order; total / data / smooth = math.fsum over the
               pixels with a finite d, finite = their number
"""
import math

import numpy as np

f32 = np.float32
INF = f32(np.inf)
DIRS4 = [(-1, 0), (0, 1), (1, 0), (0, -1), (-1, 0)]                                 # (dx, dy), mgm_print_energy.h:51-53
SCANS8 = [(-1, 0), (1, 0), (0, 1), (0, -1), (-1, -1), (1, -1), (1, 1), (-1, 1)]     # mgm_weights.h:69
KINDS = {"l1trunc": 0, "l1": 1, "l2": 2, "model": 3}


def labels(d, rounded):
    """(owned bool, label int64) of a map: truncation (kinds 0-2) or round-half-even (kind 3)"""
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore"):
        owned = np.isfinite(d) & (np.abs(d) < f32(16777216.0))
    safe = np.where(owned, d, f32(0))
    lab = (np.rint(safe) if rounded else np.trunc(safe)).astype(np.int64)
    return owned, lab


def data_term(C, dmin, d, rounded, lo=None, hi=None):
    """C [ny][nx][L] float32 (labels dmin..dmin+L-1); lo / hi: the integer range images of a ragged volume (disparities)"""
    C = np.asarray(C, np.float32)
    ny, nx, L = C.shape
    owned, lab = labels(d, rounded)
    o = lab - dmin
    owned = owned & (o >= 0) & (o < L)
    if lo is not None:
        owned &= (lab >= np.asarray(lo).astype(np.int64)) & (lab <= np.asarray(hi).astype(np.int64))
    v = np.take_along_axis(C, np.clip(o, 0, L - 1)[:, :, None], axis=2)[:, :, 0]
    return np.where(owned, v, INF).astype(np.float32)


def shifted(d, dx, dy):
    """(d at p + (dx, dy), inside) with NaN outside the image"""
    ny, nx = d.shape
    out = np.full((ny, nx), np.nan, np.float32)
    ins = np.zeros((ny, nx), bool)
    ys, yd = slice(max(dy, 0), ny + min(dy, 0)), slice(max(-dy, 0), ny + min(-dy, 0))
    xs, xd = slice(max(dx, 0), nx + min(dx, 0)), slice(max(-dx, 0), nx + min(-dx, 0))
    out[yd, xd] = d[ys, xs]
    ins[yd, xd] = True
    return out, ins


def energy_map(C, dmin, d, kind, P1, P2, connectivity=4, use_fh=0, w8=None, lo=None, hi=None):
    """(E, data, smooth) float32 [ny][nx]; smooth of kinds 0-2 is 0 + t_0 + t_1 ... on its own"""
    kind = KINDS.get(kind, kind)
    d = np.asarray(d, np.float32)
    P1, P2 = f32(P1), f32(P2)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if kind == 3:
            data = data_term(C, dmin, d, True, lo, hi)
            s = np.zeros(d.shape, np.float32)
            for k, (dx, dy) in enumerate(SCANS8[:connectivity]):
                dq, ins = shifted(d, dx, dy)
                ok = ins & np.isfinite(dq)
                w = np.ones(d.shape, np.float32) if w8 is None else np.asarray(w8, np.float32)[k]
                a = np.abs((dq - d).astype(np.float32))
                p1w, p2w = (P1 * w).astype(np.float32), (P2 * w).astype(np.float32)
                if use_fh:
                    V = np.fmin((p1w * a).astype(np.float32), p2w)
                else:
                    V = np.where(a == 0, f32(0), np.where(a <= 1, np.fmin(p1w, p2w), p2w))
                s = np.where(ok, (s + V.astype(np.float32)).astype(np.float32), s)
            smooth = (f32(0.5) * s).astype(np.float32)
            E = np.where(np.isfinite(d), (data + smooth).astype(np.float32), f32(np.nan)).astype(np.float32)
            return E, data, smooth
        data = data_term(C, dmin, d, False, lo, hi)
        G = (f32(0) + data).astype(np.float32)
        s = np.zeros(d.shape, np.float32)
        for t in range(4):
            dr, insr = shifted(d, *DIRS4[t])
            dq, insq = shifted(d, *DIRS4[t + 1])
            ok = insr & insq
            er = (dr - d).astype(np.float32)
            if kind == 1:
                term = (np.abs(er) / f32(4)).astype(np.float32)
            elif kind == 2:
                eq = (dq - d).astype(np.float32)
                term = (np.sqrt(((er * er).astype(np.float32) + (eq * eq).astype(np.float32)).astype(np.float32)) / f32(4)).astype(np.float32)
            else:
                term = np.where(np.abs(er) <= 1, P1 / f32(4), P2 / f32(4)).astype(np.float32)
            G = np.where(ok, (G + term).astype(np.float32), G)
            s = np.where(ok, (s + term).astype(np.float32), s)
        return G.astype(np.float32), data, s.astype(np.float32)


def serial_sum(E):
    """the fp32 sum in raster order, 0 + E[0] + E[1] + ..."""
    return np.cumsum(np.asarray(E, np.float32).ravel(), dtype=np.float32)[-1]


def totals(d, E, data, smooth):
    fin = np.isfinite(np.asarray(d, np.float32))
    fs = lambda a: math.fsum(np.asarray(a, np.float64)[fin].tolist()) if np.all(np.isfinite(np.asarray(a)[fin])) else float(np.asarray(a, np.float64)[fin].sum())
    return dict(serial=serial_sum(E), total=fs(E), data=fs(data), smooth=fs(smooth), finite=int(fin.sum()), pixels=int(fin.size))


def energy(C, dmin, d, kind, P1, P2, connectivity=4, use_fh=0, w8=None, lo=None, hi=None):
    """(E, totals dict)"""
    E, data, smooth = energy_map(C, dmin, d, kind, P1, P2, connectivity, use_fh, w8, lo, hi)
    return E, totals(d, E, data, smooth)


def scalar_model_energy(C, dmin, d, P1, P2, connectivity=4, use_fh=0, w8=None, lo=None, hi=None):
    """kind 3 pixel by pixel in plain loops: the restatement the vectorised model is tested against"""
    C = np.asarray(C, np.float32)
    d = np.asarray(d, np.float32)
    ny, nx, L = C.shape
    E = np.empty((ny, nx), np.float32)
    P1, P2 = f32(P1), f32(P2)
    with np.errstate(invalid="ignore", over="ignore"):
        for y in range(ny):
            for x in range(nx):
                o = d[y, x]
                if not np.isfinite(o):
                    E[y, x] = np.nan
                    continue
                data = INF
                if abs(o) < 16777216.0:
                    lab = int(np.rint(o))
                    if 0 <= lab - dmin < L and (lo is None or int(lo[y, x]) <= lab <= int(hi[y, x])):
                        data = C[y, x, lab - dmin]
                s = f32(0)
                for k in range(connectivity):
                    qx, qy = x + SCANS8[k][0], y + SCANS8[k][1]
                    if not (0 <= qx < nx and 0 <= qy < ny) or not np.isfinite(d[qy, qx]):
                        continue
                    w = f32(1) if w8 is None else f32(w8[k][y, x])
                    a = f32(abs(f32(d[qy, qx] - o)))
                    p1w, p2w = f32(P1 * w), f32(P2 * w)
                    if use_fh:
                        V = np.fmin(f32(p1w * a), p2w)
                    else:
                        V = f32(0) if a == 0 else (np.fmin(p1w, p2w) if a <= 1 else p2w)
                    s = f32(s + V)
                E[y, x] = f32(data + f32(f32(0.5) * s))
    return E
