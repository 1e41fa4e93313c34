"""numpy restatement of what the reference's main() does to the disparity maps right after the path -- TEST
INFRASTRUCTURE ONLY (see oracle/oracle.py for who may import this).  Plain loops (small images only), except backproject().

Pinned on the compiled reference (oracle/_ref/libmgm_refpost.so, oracle/_ref/mgm) by tests/test_oracle_vs_ref.py, on maps with
NaN labels and +INF costs, and by tests/test_post_ref.py on the edge maps of tests/post_domains.py."""
import numpy as np


def total_order_key(a):
    """uint32 keys whose unsigned order is the floats' total order: -0 below +0 (NaN samples must have been dropped)."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))


def median(u, radius):
    """median_filter, img_tools.h:203-238: per channel, the (2r+1)^2 window clipped at the border, NaN samples dropped, the
    UPPER median v[n/2] of what is left (nth_element); an all-NaN window leaves the pixel as it is.  +-INF are ordinary
    samples (they order like any value).  ONE departure, the project's own: the samples are ranked by the
    TOTAL order, -0 below +0, where the reference returns whichever zero nth_element happens to leave at v[n/2]."""
    u = np.asarray(u, np.float32)
    u3 = u.reshape((-1,) + u.shape[-2:])
    out = u3.copy()
    nch, ny, nx = u3.shape
    for c in range(nch):
        for y in range(ny):
            for x in range(nx):
                w = u3[c, max(0, y - radius):y + radius + 1, max(0, x - radius):x + radius + 1].ravel()
                w = w[~np.isnan(w)]
                if w.size:
                    out[c, y, x] = w[np.argsort(total_order_key(w), kind="stable")[w.size // 2]]
    return out.reshape(u.shape)


def c_round(v):
    """round() of <math.h>: half away from zero."""
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def leftright(d, other, tau):
    """leftright_test, mgm.cc:68-91: Lx = (int)round(x + d); outside `other` -> NaN; else Rx = Lx + other[Lx, y] and the
    label is dropped iff fabs(Rx - x) > tau.  Consequences for non-finite inputs, all as the compiled reference behaves on
    x86-64 (cvttsd2si of NaN / out-of-range = INT_MIN, which lies outside every image): a NaN or infinite d -> NaN; a NaN in
    `other` makes the comparison false -> the label is KEPT; an infinite value in `other` -> dropped."""
    d = np.asarray(d, np.float32)
    other = np.asarray(other, np.float32)
    ny, nx = d.shape
    out = np.full_like(d, np.nan)
    for y in range(ny):
        for x in range(nx):
            s = np.float32(x) + d[y, x]            # int + float -> float
            r = c_round(np.float64(s))
            if not np.isfinite(r) or r < -2147483648.0 or r > 2147483647.0:
                continue                           # INT_MIN: outside
            Lx = int(r)
            if 0 <= Lx < other.shape[1]:
                Rx = np.float32(Lx) + other[y, Lx]
                if not (abs(np.float64(np.float32(Rx - np.float32(x)))) > np.float64(np.float32(tau))):
                    out[y, x] = d[y, x]
    return out


def c_fmin(a, b):
    """fmin() as glibc orders it on finite / infinite operands: of two equal operands (the two zeros) the LATER one."""
    return a if a < b else b


def c_fmax(a, b):
    return a if a > b else b


def image_minmax(u):
    """image_minmax, img_tools.h:183-199: `v < gmin` / `v > gmax` over the finite samples in scan order, from +INF / -INF --
    of several zeros the FIRST one met."""
    gmin, gmax = np.float32(np.inf), np.float32(-np.inf)
    for v in np.asarray(u, np.float32).ravel():
        if np.isfinite(v):
            if v < gmin:
                gmin = v
            if v > gmax:
                gmax = v
    return gmin, gmax


def update_ranges(outoff, lo, hi, slack=3, radius=2):
    """update_dmin_dmax, mgm.cc:120-158, followed by the two remove_nonfinite_values_Img calls of main() (387-388): returns
    the new (lo, hi).  Per pixel the (2r+1)^2 window with clamped indices; a finite sample v contributes v -+ slack, any other
    gmin - slack / gmax + slack (the finite extrema of the whole map, +INF / -INF when it has none); float32 arithmetic with
    the int slack converted first; the pixel is rewritten iff the folded minimum is finite; what is not finite afterwards
    becomes gmin / gmax (which may themselves be infinite)."""
    o = np.asarray(outoff, np.float32)
    o = o.reshape(o.shape[-2], o.shape[-1])
    ny, nx = o.shape
    lo2 = np.array(lo, np.float32, copy=True).reshape(ny, nx)
    hi2 = np.array(hi, np.float32, copy=True).reshape(ny, nx)
    gmin, gmax = image_minmax(o)
    s = np.float32(abs(int(slack)))
    with np.errstate(over="ignore", invalid="ignore"):
        fin = np.isfinite(o)
        a_all = np.where(fin, o, gmin) - s
        b_all = np.where(fin, o, gmax) + s
    for j in range(ny):
        ys = np.clip(np.arange(j - radius, j + radius + 1), 0, ny - 1)
        for i in range(nx):
            xs = np.clip(np.arange(i - radius, i + radius + 1), 0, nx - 1)
            dmin, dmax = np.float32(np.inf), np.float32(-np.inf)
            for a, b in zip(a_all[np.ix_(ys, xs)].ravel(), b_all[np.ix_(ys, xs)].ravel()):
                dmin, dmax = c_fmin(dmin, a), c_fmax(dmax, b)
            if np.isfinite(dmin):
                lo2[j, i], hi2[j, i] = dmin, dmax
    lo2[~np.isfinite(lo2)] = gmin
    hi2[~np.isfinite(hi2)] = gmax
    return lo2, hi2


def backproject_index(unx, uny, nch, vnx, vny, disp):
    """(inside (ny, nx) bool, k (nch, ny, nx) uint64): which pixels mgm.cc:439 finds inside v, and the element of v's vector
    its float index expression x + q.x + (y + q.y) * v.nx + c * v.npix (mgm.cc:440) converts to -- float32 throughout, the
    reference's association ((x + d) + (y + 0) * vnx) + c * vnpix, ints converted to float first.  k may be nch * vnpix, one
    past the end (the sum rounds up in the last row of the last channel)."""
    f32 = np.float32
    d = np.asarray(disp, f32).reshape(uny, unx)
    with np.errstate(invalid="ignore", over="ignore"):
        px = np.arange(unx, dtype=f32)[None, :] + d
        py = np.arange(uny, dtype=f32)[:, None] + f32(0)
        inside = (px >= 0) & (py >= 0) & (px < f32(vnx)) & (py < f32(vny))
        row = px + py * f32(vnx)
        k = np.stack([row + f32(c * vnx * vny) for c in range(nch)])
    k = np.where(inside[None], k, 0).astype(np.uint64)
    return inside, k


def backproject(u, v, disp):
    """The back-projected image, mgm.cc:433-443: v at the index of backproject_index where x + d lies inside v, else u.
    Vectorised (millions of pixels are fine).  ONE departure, the project's own: an index past the end of v
    reads v's last element, where the reference reads whatever follows its vector."""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    u, v = u.reshape((-1,) + u.shape[-2:]), v.reshape((-1,) + v.shape[-2:])
    nch, uny, unx = u.shape
    _, vny, vnx = v.shape
    inside, k = backproject_index(unx, uny, nch, vnx, vny, disp)
    k = np.minimum(k, np.uint64(v.size - 1))
    return np.where(inside[None], v.ravel()[k], u)
