"""Crafted Lr volumes for the RANGE-PROPORTIONAL winner search (k_wta_rel<SPL,CB>, k_rel_S; mgm_wta.hip): the mapping between the
dense hull and the kernels' layout, the cases, the windows, the expectation and the floors.

The layout (mgm_device.h, RelVolume): every pixel has `slots` (64 or 128) label slots, slot k <-> disparity lo(p) - 1 + k, of
which the pixel OWNS those with a disparity in [lo(p), hi(p)]; what the other slots hold is nobody's business (`poison`).

The expectation is the restatement that exists (tests/wta_crafted.py, pinned by tests/test_wta_crafted_ref.py) and nothing new:

    S      = sum_fix(lr, C, NDIR, fix)                       on the hull
    S      = where(own, S, vout_of(NDIR, fix))               Dvec::get outside a pixel's range: never incremented, C = +INF
    winner = windowed(S, window)                             first strict minimum among the finite entries by rising disparity
    fit    = oracle.refine_ranged(...)                       the gate of mgm_refine.h:58 on the WINDOW

and for k_rel_S what its comment says: S on the labels a pixel owns, +INF -- INF - (NDIR-1)*INF with the fix -- on the others.

The crafted classes are those of tests/wta_crafted.py, generated PER PIXEL AT THE WIDTH OF ITS OWN RANGE and laid at the range
(`crafted`): what a class plants -- two equal minima, a winner on one of the five labels around the gate -- lands inside the own
range at lo, lo+1, hi-2, hi-1, hi whatever the range is.  Pixels are numbered i = y * nx + x; a pixel's range kind goes by
i % 5, its window kind by i % 7, what the classes plant by i % 3, i % 4 and i % 16: every combination occurs.

tests/test_wta_rel_crafted_ref.py pins all of this on the CPU; tests/test_gpu_wta_rel_crafted.py holds the kernels to it.
"""
import numpy as np

import wta_crafted as W
from mgm_amd import synth

f32 = np.float32
INF = f32(np.inf)
POISONS = dict(nan=f32(np.nan), ninf=f32(-np.inf), big=f32(-1e30), zero=f32(0.0))  # what the slots a pixel does not own may hold

# format -> slots, bytes per cost code, cost function, channels, census window, (nx, ny), NDIR, use_fh, TSGM, P1, P2, labels of the hull
# (the aggregation is TAME: natural costs, positive penalties, no weights -- what tests/test_gpu_ragged_oracle.py runs already)
CASES = {
    "s64_c1": (64, 1, "census", 1, 5, (26, 9), 8, 0, 3, 8.0, 32.0, 70),
    "s64_c2": (64, 2, "ad", 3, 3, (23, 7), 4, 1, 3, 6.0, 60.0, 75),
    "s64_c4": (64, 4, "ncc", 1, 5, (26, 9), 1, 1, 3, 2.0, 30.0, 70),
    "s128_c1": (128, 1, "census", 1, 5, (23, 7), 3, 1, 3, 2.0, 30.0, 140),
    "s128_c2": (128, 2, "ad", 3, 3, (26, 9), 5, 0, 4, 24.0, 96.0, 131),
    "s128_c4": (128, 4, "adfrac", 1, 3, (23, 7), 8, 0, 3, 8.0, 32.0, 140),
    "tiny": (64, 1, "census", 1, 5, (3, 1), 4, 0, 3, 8.0, 32.0, 20),
}
SEED = {cls: 700 + n for n, cls in enumerate(W.LR_CLASSES)}  # the seed of every class, for the CPU pins and the device tests alike
DMIN = -9  # every hull starts here: ranges and windows on both sides of zero ((int) truncates towards zero)


def own_mask(dmin, L, lo, hi):
    """[ny][nx][L]: the labels of the hull a pixel owns"""
    d = dmin + np.arange(L)
    return (d >= np.asarray(lo)[..., None]) & (d <= np.asarray(hi)[..., None])


def off_by_fractions(lo, hi):
    """Range images whose (int) is (lo, hi), off by +0.4 / +0.7 or by -0.4 / -0.7 in turn (every other group of seven pixels), as
    windows() of tests/test_gpu_wta_crafted.py has them: a bound whose sign the offset would cross takes it from its neighbour."""
    shape = np.shape(lo)
    lo, hi = np.ravel(lo).astype(np.int64), np.ravel(hi).astype(np.int64)
    up = (np.arange(lo.size) // 7) % 2 == 0
    flo = np.where(up, np.where(lo >= 0, lo + 0.4, lo - 1 + 0.4), np.where(lo <= 0, lo - 0.4, lo + 1 - 0.4))
    fhi = np.where(up, np.where(hi >= 0, hi + 0.7, hi - 1 + 0.7), np.where(hi <= 0, hi - 0.7, hi + 1 - 0.7))
    flo, fhi = flo.astype(np.float32), fhi.astype(np.float32)
    wl, wh = W.int_window(flo, fhi)
    assert (wl == lo).all() and (wh == hi).all() and (flo != np.trunc(flo)).all() and (fhi != np.trunc(fhi)).all()
    return flo.reshape(shape), fhi.reshape(shape)


def ranges(ny, nx, dmin, L, slots, seed):
    """Integer ranges (lo, hi) inside the hull [dmin, dmin + L): by i % 5 a range of 8..20 labels somewhere, a single label, one
    that touches the low end of the hull, one that touches the high end, a wide one (40 labels up to the format's limit).  Pixel 0
    and the last pixel hold the two ends of the hull; with 128 slots pixel 7 is the ONE pixel wider than 62 labels."""
    rng = np.random.default_rng(seed)
    n, limit = ny * nx, min(62, L - 2)
    i = np.arange(n)
    kind = i % 5
    w = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [rng.integers(8, 21, n), 1, rng.integers(5, 31, n), rng.integers(5, 31, n)],
                  rng.integers(min(40, limit), limit + 1, n))
    w = np.minimum(w, L)
    lo = np.select([kind == 2, kind == 3], [dmin, dmin + L - w], dmin + rng.integers(0, L - w + 1))
    if slots == 128 and n > 7:
        w[7], lo[7] = min(L - 3, 126), dmin + 2
    if n <= 3:  # the tiny shape: a single label, the low end, the high end
        w, lo = np.array([1, 6, 9])[:n], np.array([dmin + 4, dmin, dmin + L - 9])[:n]
    lo[0] = dmin
    lo[-1] = dmin + L - w[-1]
    hi = lo + w - 1
    assert (lo >= dmin).all() and (hi <= dmin + L - 1).all() and lo.min() == dmin and hi.max() == dmin + L - 1
    assert (w <= slots - 2).all() and ((w > 62).sum() == (1 if slots == 128 else 0))
    return lo.reshape(ny, nx), hi.reshape(ny, nx)


def case(name):
    """Everything of a format but the costs: dict(slots, cb, dist, win, nx, ny, NDIR, FH, MGM, P1, P2, dmin, L, u, v, lo, hi, flo, fhi)"""
    slots, cb, dist, nch, win, (nx, ny), NDIR, FH, MGM, P1, P2, L = CASES[name]
    u, v, _ = synth.stereo_pair(max(nx, 16), max(ny, 8), -4, 6, seed=3 + len(name) + slots + cb, nch=nch)
    u, v = np.ascontiguousarray(u[:, :ny, :nx]), np.ascontiguousarray(v[:, :ny, :nx])
    if dist == "adfrac":  # float images: the absolute difference is no whole number, the cost code is the fp32 cost itself
        dist, u, v = "ad", (u * f32(0.37) + f32(0.21)).astype(np.float32), (v * f32(0.37)).astype(np.float32)
    lo, hi = ranges(ny, nx, DMIN, L, slots, seed=17 + slots + cb)
    flo, fhi = off_by_fractions(lo, hi)
    return dict(name=name, slots=slots, cb=cb, dist=dist, win=win, nx=nx, ny=ny, NDIR=NDIR, FH=FH, MGM=MGM, P1=P1, P2=P2, dmin=DMIN, L=L, u=u, v=v,
                lo=lo, hi=hi, flo=flo, fhi=fhi)


def costs(oracle, k):
    """the volume's costs on the hull, +INF where a pixel does not own the label (oracle/mgm_oracle.c, pinned on the reference)"""
    return oracle.costvolume_ranged(k["u"], k["v"], k["lo"], k["hi"], k["dmin"], k["dmin"] + k["L"] - 1, "none", k["dist"], np.inf, k["win"])


# ---- the mapping ------------------------------------------------------------------------------------------------------------
def to_rel(lr_dense, dmin, lo, hi, slots, poison):
    """[NDIR][ny][nx][L] on the hull -> [NDIR][npix][slots]: slot k of pixel p holds the label lo(p) - 1 + k, slots whose label
    lies outside [lo(p), hi(p)] hold `poison`"""
    lr_dense = np.asarray(lr_dense, np.float32)
    NDIR, ny, nx, L = lr_dense.shape
    lo, hi = np.ravel(lo).astype(np.int64), np.ravel(hi).astype(np.int64)
    assert (lo >= dmin).all() and (hi <= dmin + L - 1).all() and (hi - lo + 1 <= slots - 2).all() and (hi >= lo).all()
    lab = lo[:, None] - 1 + np.arange(slots)[None, :]
    owned = (lab >= lo[:, None]) & (lab <= hi[:, None])
    at = np.clip(lab - dmin, 0, L - 1)
    rel = np.take_along_axis(lr_dense.reshape(NDIR, ny * nx, L), np.broadcast_to(at[None], (NDIR,) + at.shape), axis=2)
    return np.where(owned[None], rel, f32(poison)).astype(np.float32)


def from_rel(rel, dmin, L, lo, hi, shape, fill=INF):
    """the inverse: [NDIR][npix][slots] -> [NDIR][ny][nx][L], `fill` on the labels a pixel does not own"""
    rel = np.asarray(rel, np.float32)
    NDIR, npix, slots = rel.shape
    lo, hi = np.ravel(lo).astype(np.int64), np.ravel(hi).astype(np.int64)
    d = dmin + np.arange(L)[None, :]
    owned = (d >= lo[:, None]) & (d <= hi[:, None])
    at = np.clip(d - (lo[:, None] - 1), 0, slots - 1)
    dense = np.take_along_axis(rel, np.broadcast_to(at[None], (NDIR,) + at.shape), axis=2)
    return np.where(owned[None], dense, f32(fill)).astype(np.float32).reshape((NDIR,) + tuple(shape) + (L,))


def records(dmin, lo, hi):
    """[npix][4] int32, as the volume's copy holds them: disparity of slot 0, lowest, highest, 0"""
    lo, hi = np.ravel(lo).astype(np.int32), np.ravel(hi).astype(np.int32)
    return np.stack([lo - 1, lo, hi, np.zeros_like(lo)], axis=1)


# ---- the classes, laid at the pixels' own ranges ---------------------------------------------------------------------------------
def crafted(name, seed, NDIR, dmin, L, lo, hi):
    """[NDIR][ny][nx][L]: pixel p holds, on its own labels, its rows of the class generated at the width of its range (same seed,
    same pixel numbering: what the class plants at label k of w lands at lo(p) + k); the labels it does not own hold the class
    generated at the hull's width -- they never reach the device, the expectation must ignore them."""
    ny, nx = lo.shape
    fn = W.LR_CLASSES[name]
    dense = fn(seed + 1000, NDIR, ny, nx, L).reshape(NDIR, ny * nx, L)
    lo_, w_ = np.ravel(lo) - dmin, np.ravel(hi - lo + 1)
    for w in np.unique(w_):
        gen = fn(seed, NDIR, ny, nx, int(w)).reshape(NDIR, ny * nx, int(w))
        for p in np.nonzero(w_ == w)[0]:
            dense[:, p, lo_[p]:lo_[p] + w] = gen[:, p, :]
    return dense.reshape(NDIR, ny, nx, L)


# ---- the windows of the second search -------------------------------------------------------------------------------------------
def windows(lo, hi, seed=6):
    """Integer windows (wl, wh) by i % 7, placed at each pixel's OWN range: inside it, straddling its low end, its high end, wholly
    below it, wholly above it (every other one starts right at hi + 1), a single label of it, empty.  They may leave the hull."""
    ny, nx = lo.shape
    lo, hi = np.ravel(lo).astype(np.int64), np.ravel(hi).astype(np.int64)
    n = lo.size
    i, rng = np.arange(n), np.random.default_rng(seed)
    kind, w = i % 7, hi - lo + 1
    a = lo + (rng.integers(0, 1 << 30, n) % np.maximum(w - 6, 1))  # a label of the own range
    gap = (i // 7) % 2
    wl = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [a, lo - 3, hi - 3, lo - 6, hi + 1 + gap, a], a + 3)
    wh = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [np.minimum(a + 6, hi), lo + 3, hi + 2, lo - 2, hi + 4, a], a + 1)
    return wl.reshape(ny, nx), wh.reshape(ny, nx)


# ---- the expectation --------------------------------------------------------------------------------------------------------------
def masked_S(lr, C, dmin, lo, hi, NDIR, fix):
    """the reference's S on the hull: the ordered sum on the labels a pixel owns, vout on the others"""
    S = W.sum_fix(lr, C, NDIR, fix)
    return np.where(own_mask(dmin, S.shape[2], lo, hi), S, W.vout_of(NDIR, fix)).astype(np.float32)


def expect_search(oracle, S, dmin, flo, fhi, NDIR, fix, refine):
    """(out, outcost) of the search of masked_S's S in the windows [(int)flo, (int)fhi] -- the volume's own range images for the
    un-windowed search -- and the refinement"""
    out, cost, Sh, hmin, wl, wh = W.windowed(S, dmin, flo, fhi, NDIR, fix)
    if refine:
        out, cost = oracle.refine_ranged(Sh, hmin, wl, wh, refine, out, cost)
    return out, cost


def expect_S(lr, C, dmin, lo, hi, NDIR, fix):
    """what k_rel_S writes: S on the labels a pixel owns; on the others +INF, minus (NDIR - 1) * INF with the fix (NaN at every
    pass count: INF - INF, and INF - 0 * INF at one pass)"""
    S = W.sum_fix(lr, C, NDIR, fix)
    with np.errstate(invalid="ignore"):
        other = INF - f32(NDIR - 1) * INF if fix else INF
    return np.where(own_mask(dmin, S.shape[2], lo, hi), S, other).astype(np.float32)


# ---- the floors -------------------------------------------------------------------------------------------------------------------
def floors(name, lr, C, k, verbose=False):
    """What class `name` has to do on case k AFTER the ownership mask, on the restatement alone; each floor is a condition below.
    Without the over-count fix: the natural costs C of a tame aggregation are no TAME_C class (nothing holds one value per planted
    pixel), so with the fix a planted tie survives only where C happens to agree; those calls are compared, not counted.  The
    windowed floors are counted with and without the fix.  Returns what was counted."""
    NDIR, dmin, L, lo, hi, flo, fhi = k["NDIR"], k["dmin"], k["L"], k["lo"], k["hi"], k["flo"], k["fhi"]
    ny, nx = lo.shape
    n, i = ny * nx, np.arange(ny * nx).reshape(ny, nx)
    w = hi - lo + 1
    own = own_mask(dmin, L, lo, hi)
    S = masked_S(lr, C, dmin, lo, hi, NDIR, 0)
    out, cost = W.windowed(S, dmin, flo, fhi, NDIR, 0)[:2]
    has = np.isfinite(cost)
    with np.errstate(invalid="ignore"):
        gate = has & (out - 1 >= lo) & (out + 2 <= hi)
        tie = (own & np.isfinite(S) & (S == cost[..., None])).sum(axis=2) > 1
    got = dict(winner=has.mean(), open=int(gate.sum()), shut=int((has & ~gate).sum()), tie=int((tie & has).sum()), none=int((~has).sum()))
    # every winner is a label the pixel owns
    assert (~has | ((out >= lo) & (out <= hi))).all(), name
    big = n >= 100
    if name == "ties" and big:
        # planted: every fourth pixel with two labels or more holds two equal strict minima inside its own range
        planted = (i % 4 == 0) & (w >= 2)
        assert planted.sum() >= n // 8 and tie[planted].all() and has[planted].all(), got
        # ... and the winner is the LOWER of the two (tie_labels at the width of the range)
        first = np.array([W.tie_labels((p // 4) % 4, int(wp))[0] for p, wp in zip(i.ravel(), w.ravel())]).reshape(ny, nx)
        assert (out[planted] == (lo + first)[planted]).all(), got
    if name == "edges" and big:
        # planted: pixel i with i % 16 < 5 and five labels or more wins on lo, lo+1, hi-2, hi-1, hi; the gate is open on lo+1 and hi-2 alone
        for e, (lab, is_open) in enumerate(((lo, False), (lo + 1, True), (hi - 2, True), (hi - 1, False), (hi, False))):
            m = (i % 16 == e) & (w >= 5)
            got["edge%d" % e] = int(m.sum())
            assert m.sum() >= 4 and (out[m] == lab[m]).all() and (gate[m] == is_open).all(), (e, got)
    if name == "nolabel":
        # every third pixel has no finite label, every other pixel has one
        assert not has[i % 3 == 1].any() and has[i % 3 != 1].all(), got
    if big and name not in ("nolabel",) and not (name == "overflow" and NDIR >= 5):
        # (overflow at five passes or more: a cell stays finite with p = 0.28 / 0.11 -- tests/wta_crafted.py; counted, not promised)
        assert got["winner"] >= 0.75, (name, got)
    if big and name not in W.GATE_EXEMPT and not (name == "overflow" and NDIR >= 5):
        # the gate is open on a quarter of the pixels and shut on a tenth (a fifth of the pixels has a single label: shut)
        assert got["open"] >= n // 4 and got["shut"] >= n // 10, (name, got)
    if name == "order" and NDIR > 2 and big:
        Sr = W.sum_fix(lr[::-1], C, NDIR, 0)
        got["order"] = float(np.mean(Sr.view(np.uint32)[own] != W.sum_fix(lr, C, NDIR, 0).view(np.uint32)[own]))
        assert got["order"] >= 0.25, got
    if name == "nonfinite" and big:
        # a fit that reads a non-finite neighbour inside the own range: 15 % of S, three neighbours, a quarter of the pixels open
        ys, xs = np.nonzero(gate)
        o = out[ys, xs].astype(int) - dmin
        nb = np.stack([S[ys, xs, o - 1], S[ys, xs, o + 1], S[ys, xs, o + 2]])
        got["nonfinite_neighbours"] = int((~np.isfinite(nb)).any(axis=0).sum())
        assert got["nonfinite_neighbours"] >= 8, got
    # the second search: windows at the own range
    wl, wh = windows(lo, hi)
    fwl, fwh = off_by_fractions(wl, wh)
    kind = i % 7
    for fix in (0, 1):
        Sf = masked_S(lr, C, dmin, lo, hi, NDIR, fix)
        o2, c2 = W.windowed(Sf, dmin, fwl, fwh, NDIR, fix)[:2]
        h2 = np.isfinite(c2)
        outside = h2 & ((o2 < lo) | (o2 > hi))
        if fix == 0:
            # windows wholly below / above the own range: vout = 0 is finite, the first label of the window wins at cost 0
            m = (kind == 3) | (kind == 4)
            assert (o2[m] == wl[m]).all() and (c2[m] == 0).all() and outside[m].all(), name
            for kd in (1, 2):  # straddling: how often an unowned label (0) beats every owned one, and how often it loses
                got["unowned_wins%d" % kd] = int((outside & (kind == kd)).sum())
                got["owned_wins%d" % kd] = int((h2 & ~outside & (kind == kd)).sum())
            if name == "negative" and big:
                # sums of [-20, 20): an owned label wins where one of the window is negative, an unowned one where all are positive
                assert min(got["unowned_wins1"], got["unowned_wins2"], got["owned_wins1"], got["owned_wins2"]) >= 1, got
            if name == "zeros" and big:
                # +-0 against vout = +0: equal, so the lower disparity wins -- the unowned one below the range, the owned one at its high end
                assert got["unowned_wins1"] >= 4 and got["owned_wins2"] >= 4, got
                assert (c2[outside | (h2 & (kind == 2))] == 0).all()
        else:
            # with the fix vout is -INF or NaN: never a candidate
            assert not outside.any() and not h2[(kind == 3) | (kind == 4)].any(), name
        assert not h2[kind == 6].any(), name  # an empty window
    if verbose:
        print("floors %-9s %-8s NDIR %d: %s" % (name, k["name"], NDIR, " ".join("%s=%.3g" % kv for kv in got.items())))
    return got
