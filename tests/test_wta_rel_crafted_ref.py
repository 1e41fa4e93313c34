"""What tests/test_gpu_wta_rel_crafted.py holds k_wta_rel and k_rel_S to, pinned on the CPU (tests/wta_rel_crafted.py): the mapping
between the hull and the range-proportional layout and its inverse, the cases (ranges inside the hull, off by fractions of both
signs, the formats' cost sources), the expectation against the ragged oracle's own search, and the floors every crafted class
has to reach AFTER the ownership mask, per class and format."""
import numpy as np
import pytest

import wta_crafted as W
import wta_rel_crafted as R
from helpers import ndiff

FORMATS = list(R.CASES)


@pytest.fixture(scope="module")
def cases(oracle):
    out = {}
    for name in FORMATS:
        k = R.case(name)
        k["C"] = R.costs(oracle, k)
        out[name] = k
    return out


@pytest.mark.parametrize("name", FORMATS)
def test_cases_are_what_the_formats_need(cases, name):
    k = cases[name]
    lo, hi, L, dmin, slots = k["lo"], k["hi"], k["L"], k["dmin"], k["slots"]
    w = hi - lo + 1
    n = lo.size
    assert n % 4 != 0 and (n <= 3 or n >= 100)  # the last quad of four pixels has dead lane groups
    assert lo.min() == dmin and hi.max() == dmin + L - 1 and (w >= 1).all()  # inside the hull, touching both ends
    assert (w == 1).any() and (lo == dmin).sum() >= 1 and (hi == dmin + L - 1).sum() >= 1
    assert dmin < 0 < dmin + L - 1  # ranges on both sides of zero: (int) truncates towards zero
    il, ih = W.int_window(k["flo"], k["fhi"])
    assert (il == lo).all() and (ih == hi).all() and (k["flo"] != lo).all() and (k["fhi"] != hi).all()
    if n > 3:
        assert (k["flo"] > lo).any() and (k["flo"] < lo).any() and (k["fhi"] > hi).any() and (k["fhi"] < hi).any()
    # the width selects the slot count: at most 62 labels -> 64 slots, ONE pixel at 63..126 -> 128
    assert (w.max() <= 62) if slots == 64 else ((w > 62).sum() == 1 and w.max() <= 126)
    # the cost source selects the bytes per code
    C = k["C"]
    own = R.own_mask(dmin, L, lo, hi)
    assert np.isposinf(C[~own]).all()
    fin = C[own & np.isfinite(C)]
    whole = (fin == np.trunc(fin)).all()
    assert {1: whole and fin.max() <= 254 and fin.min() >= 0, 2: whole and fin.max() > 254 and fin.min() >= 0, 4: not whole}[k["cb"]], (name, fin.min(), fin.max())
    assert k["P1"] > 0 and k["P2"] > 0
    # the windows of the second search: all seven kinds, at the own range
    wl, wh = R.windows(lo, hi)
    kind = np.arange(n).reshape(lo.shape) % 7
    assert ((wl >= lo) & (wh <= hi) & (wl <= wh))[(kind == 0) | (kind == 5)].all() and (wl == wh)[kind == 5].all()
    assert ((wl < lo) & (wh >= lo))[kind == 1].all() and ((wl <= hi) & (wh > hi))[kind == 2].all()
    assert (wh < lo)[kind == 3].all() and (wl > hi)[kind == 4].all() and (wl > wh)[kind == 6].all()
    if n > 3:
        assert (wl[kind == 4] == hi[kind == 4] + 1).any() and (wl[kind == 4] > hi[kind == 4] + 1).any()
        assert (wl < dmin).any() and (wh > dmin + L - 1).any()  # some leave the hull too


@pytest.mark.parametrize("name", FORMATS)
def test_mapping_round_trip(cases, name):
    k = cases[name]
    lo, hi, L, dmin, slots, NDIR = k["lo"], k["hi"], k["L"], k["dmin"], k["slots"], k["NDIR"]
    own = R.own_mask(dmin, L, lo, hi)
    rng = np.random.default_rng(1)
    dense = rng.standard_normal((NDIR,) + lo.shape + (L,)).astype(np.float32)
    for pname, poison in R.POISONS.items():
        rel = R.to_rel(dense, dmin, lo, hi, slots, poison)
        assert rel.shape == (NDIR, lo.size, slots) and rel.dtype == np.float32
        # slot k of pixel p holds the label lo(p) - 1 + k: spelled out, pixel by pixel
        for p in (0, lo.size // 2, lo.size - 1):
            y, x = divmod(p, lo.shape[1])
            for s in range(slots):
                d = lo[y, x] - 1 + s
                want = dense[NDIR - 1, y, x, d - dmin] if lo[y, x] <= d <= hi[y, x] else poison
                assert ndiff(rel[NDIR - 1, p, s], np.float32(want)) == 0, (pname, p, s)
        assert ndiff(rel[:, :, 0], np.full((NDIR, lo.size), poison, np.float32)) == 0  # slot 0 is the label below the range
        back = R.from_rel(rel, dmin, L, lo, hi, lo.shape)
        assert ndiff(back, np.where(own[None], dense, np.inf)) == 0, pname
        # the number of poisoned slots: all but the width of the range
        if pname == "big":
            assert ((rel[0] == poison).sum(axis=1) == slots - (hi - lo + 1).ravel()).all()
    rec = R.records(dmin, lo, hi)
    assert rec.dtype == np.int32 and (rec[:, 0] == rec[:, 1] - 1).all() and (rec[:, 3] == 0).all()


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("name", ["s64_c1", "s128_c2", "tiny"])
def test_expectation_is_the_ragged_oracles(oracle, cases, name, fix):
    """masked_S + windowed + refine_ranged against orc_mgm_ranged (pinned on the reference's mgm() with range images) on the Lr
    volumes the oracle itself makes: S on the own labels, labels and costs of the un-windowed search and of the second search"""
    k = cases[name]
    lo, hi, L, dmin, NDIR, C = k["lo"], k["hi"], k["L"], k["dmin"], k["NDIR"], k["C"]
    own = R.own_mask(dmin, L, lo, hi)
    So, oo, co, lr = oracle.mgm_ranged(C, dmin, lo, hi, k["P1"], k["P2"], NDIR, k["MGM"], k["FH"], fix, None, dump_lr=True)
    S = R.masked_S(lr, C, dmin, lo, hi, NDIR, fix)
    assert ndiff(S[own], So[own]) == 0
    assert ndiff(R.expect_S(lr, C, dmin, lo, hi, NDIR, fix)[own], So[own]) == 0
    out, cost = R.expect_search(oracle, S, dmin, k["flo"], k["fhi"], NDIR, fix, None)
    fin = np.isfinite(co)
    assert fin.any() and ndiff(cost, co) == 0 and ndiff(out[fin], oo[fin]) == 0 and np.isnan(out[~fin]).all()
    wl, wh = R.windows(lo, hi)
    fwl, fwh = R.off_by_fractions(wl, wh)
    some = wl <= wh  # (the oracle takes no empty window: those pixels get their own range there and are left out here; floors() has them)
    owl, owh = np.where(some, wl, lo), np.where(some, wh, hi)
    shmin, shmax = int(min(dmin, owl.min())), int(max(dmin + L - 1, owh.max()))
    S2, o2, c2 = oracle.mgm_ranged(C, dmin, lo, hi, k["P1"], k["P2"], NDIR, k["MGM"], k["FH"], fix, None, srange=(owl, owh, shmin, shmax))
    out, cost = R.expect_search(oracle, S, dmin, fwl, fwh, NDIR, fix, None)
    fin = np.isfinite(c2) & some
    assert ndiff(cost[some], c2[some]) == 0 and ndiff(out[fin], o2[fin]) == 0 and np.isnan(out[~fin]).all()
    for m in W.REFINEMENTS[1:]:
        ro, rc = oracle.refine_ranged(S2, shmin, owl, owh, m, np.where(fin, o2, shmin).astype(np.float32), c2)
        out, cost = R.expect_search(oracle, S, dmin, fwl, fwh, NDIR, fix, m)
        assert ndiff(cost[some], rc[some]) == 0 and ndiff(out[fin], ro[fin]) == 0, m


def test_k_rel_S_expectation_on_the_labels_nobody_owns():
    lo, hi = np.array([[-3, 0]]), np.array([[-1, 0]])
    lr = np.ones((8, 1, 2, 6), np.float32)
    C = np.full((1, 2, 6), 2, np.float32)
    for NDIR in (1, 2, 8):
        own = R.own_mask(-4, 6, lo, hi)
        S0, S1 = R.expect_S(lr[:NDIR], C, -4, lo, hi, NDIR, 0), R.expect_S(lr[:NDIR], C, -4, lo, hi, NDIR, 1)
        assert np.isposinf(S0[~own]).all() and np.isnan(S1[~own]).all()  # (INF - 0 * INF at one pass is NaN too)
        assert (S0[own] == NDIR).all() and (S1[own] == NDIR - 2 * (NDIR - 1)).all()


@pytest.mark.parametrize("cls", list(W.LR_CLASSES))
@pytest.mark.parametrize("name", FORMATS)
def test_floors_after_the_ownership_mask(cases, name, cls):
    k = cases[name]
    lr = R.crafted(cls, R.SEED[cls], k["NDIR"], k["dmin"], k["L"], k["lo"], k["hi"])
    assert lr.dtype == np.float32 and lr.shape == (k["NDIR"],) + k["lo"].shape + (k["L"],)
    R.floors(cls, lr, k["C"], k, verbose=True)


# ---- the inputs tell wrong kernels apart --------------------------------------------------------------------------------------
# Restatements with ONE rule of the reference broken, the way a kernel could break it, run on the very inputs of the device
# tests: each must leave the expectation on the class that was made for the rule (so a kernel wrong in that way cannot pass).
def wrong_last_of_equal_minima(S, dmin, wl, wh, NDIR, fix):
    """the LAST of equal minima: the same search on the mirrored label axis"""
    L = S.shape[2]
    out, cost = W.numpy_windowed_wta(S[:, :, ::-1], -(dmin + L - 1), (-wh).astype(np.float32), (-wl).astype(np.float32), NDIR, fix)
    return -out, cost


@pytest.mark.parametrize("name", [n for n in FORMATS if n != "tiny"])
def test_the_inputs_tell_wrong_kernels_apart(oracle, cases, name):
    k = cases[name]
    lo, hi, L, dmin, NDIR, C = k["lo"], k["hi"], k["L"], k["dmin"], k["NDIR"], k["C"]
    own = R.own_mask(dmin, L, lo, hi)
    wl, wh = R.windows(lo, hi)
    fwl, fwh = R.off_by_fractions(wl, wh)
    lr = {cls: R.crafted(cls, R.SEED[cls], NDIR, dmin, L, lo, hi) for cls in W.LR_CLASSES}
    # 1. the tie-break, un-windowed and windowed: `ties`
    S = R.masked_S(lr["ties"], C, dmin, lo, hi, NDIR, 0)
    for a, b in ((lo, hi), (wl, wh)):
        good = W.numpy_windowed_wta(S, dmin, a.astype(np.float32), b.astype(np.float32), NDIR, 0)
        bad = wrong_last_of_equal_minima(S, dmin, a, b, NDIR, 0)
        assert ndiff(good[1], bad[1]) == 0 and ndiff(good[0], bad[0]) >= 8, name
    # 2. a label the pixel does not own read from its slot (the poison) instead of vout -- in the windowed search the candidates
    # `negative` and `zeros` decide between without the fix, and the neighbours of a fit in a window that leaves the own range
    for cls, fix, refine, least in (("negative", 0, None, 8), ("zeros", 0, None, 8), ("edges", 1, "vfit", 1), ("edges", 0, "cubic", 1)):
        S = R.masked_S(lr[cls], C, dmin, lo, hi, NDIR, fix)
        good = R.expect_search(oracle, S, dmin, fwl, fwh, NDIR, fix, refine)
        for pname, poison in R.POISONS.items():
            with np.errstate(invalid="ignore"):
                slot = np.float32(0) + np.float32(NDIR) * poison  # what the sum of NDIR poisoned slots gives, near enough
            if ndiff(slot, W.vout_of(NDIR, fix)) == 0:
                continue  # (this poison IS vout: +0 without the fix, -INF with it from two passes on, NaN with it at one pass)
            Sbad = np.where(own, S, slot).astype(np.float32)
            out, cost, Sh, hmin, il, ih = W.windowed(S if refine else Sbad, dmin, fwl, fwh, NDIR, fix)  # (with a refinement: the right winner, the wrong neighbours)
            if refine:
                Shbad = Sh.copy()
                Shbad[:, :, dmin - hmin:dmin - hmin + L] = Sbad
                out, cost = oracle.refine_ranged(Shbad, hmin, il, ih, refine, out, cost)
            assert ndiff(good[0], out) + ndiff(good[1], cost) >= least, (name, cls, fix, refine, pname)
    # 3. the gate on the wrong interval: the own range instead of the window (second search), the hull instead of the own range
    # (un-windowed): `edges` wins on the labels around both
    for fix in (0, 1):
        S = R.masked_S(lr["edges"], C, dmin, lo, hi, NDIR, fix)
        out, cost, Sh, hmin, il, ih = W.windowed(S, dmin, fwl, fwh, NDIR, fix)
        good = oracle.refine_ranged(Sh, hmin, il, ih, "vfit", out, cost)
        bad = oracle.refine_ranged(Sh, hmin, np.maximum(il, lo), np.minimum(ih, hi), "vfit", out, cost)
        if fix == 0:  # (with the fix nothing outside the own range wins, and a fit that reads vout = -INF / NaN differs from no fit)
            assert ndiff(good[0], bad[0]) >= 1, (name, fix)
        out, cost, Sh, hmin, il, ih = W.windowed(S, dmin, k["flo"], k["fhi"], NDIR, fix)
        good = oracle.refine_ranged(Sh, hmin, il, ih, "vfit", out, cost)
        bad = oracle.refine_ranged(Sh, hmin, np.full_like(il, dmin), np.full_like(ih, dmin + L - 1), "vfit", out, cost)
        assert ndiff(good[0], bad[0]) >= 8, (name, fix)
