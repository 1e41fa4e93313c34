"""mgm_wta_consensus_dev and mgm_consensus_filter_dev: the consensus votes over the Lr volumes of the context's last
aggregation, each pass taken alone, bit for bit against the numpy model (tests/consensus_model.py) on the ORACLE's per-pass Lr of
the same aggregation -- dense volumes, every slot of a batch, ragged volumes on both of their routes --, what the call leaves
untouched, the entry points' refusals, and the filter."""
import os

import numpy as np
import pytest

import mgm_amd
from consensus_model import consensus, consensus_filter
from helpers import ndiff
from mgm_amd import synth
from oracle import oracle as orc_mod

pytestmark = pytest.mark.gpu

TOLS = (0.0, 0.5, 1.0, 2.5)


def same(got, want):
    """bit for bit, NaN payloads aside -- and NaN in the same places"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


def votes_of(ctx, cv, NDIR, d, tol, want_winners=True, want_votes=True):
    """(votes [ny][nx], winners [NDIR][ny][nx]) as host arrays (None for what was not asked for); d a host map or None"""
    dd = ctx.upload_image(d) if d is not None else None
    v, w = ctx.wta_consensus_dev(cv, NDIR, dd, tol, votes=None if want_votes else False, want_winners=want_winners)
    res = (v.download()[0] if v is not None else None, w.download() if w is not None else None)
    for h in (dd, v, w):
        if h is not None:
            h.free()
    return res


def families(ctx, fn):
    """fn() with the timing table on: its result and the names the table lists that begin with k_wta_consensus"""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        res = fn()
        names = [n for n, _ in ctx.timings()]
    finally:
        ctx.timing(False)
    return res, {n for n in names if n.startswith("k_wta_consensus")}


def maps_to_judge(out, vfit, L, dmin, seed):
    """the unrefined winner, the vfit map, and the winner shifted by up to +-3 labels and fractions with NaN and +-INF sprinkled in"""
    rng = np.random.default_rng(seed)
    shifted = (out + rng.choice(np.array([0, 0, 0.5, -0.5, 1, -1, 1.5, 2.5, -2.5, 3, -3], np.float32), out.shape)).astype(np.float32)
    shifted[rng.random(out.shape) < 0.1] = np.nan
    shifted.flat[::17] = np.inf
    shifted.flat[5::23] = -np.inf
    return {"winner": out, "vfit": vfit, "shifted": shifted}


def check_against(ctx, cv, lr, dmin, NDIR, maps, lo=None, hi=None, what=""):
    """every map at every tolerance against the model on lr; the winners once more without votes and without d"""
    n = 0
    for name, d in maps.items():
        for tol in TOLS:
            gv, gw = votes_of(ctx, cv, NDIR, d, tol)
            wv, ww = consensus(lr, dmin, NDIR, d, tol, lo, hi)
            assert same(gv, wv), "%s %s tol %g votes: %d of %d differ" % (what, name, tol, ndiff(gv, wv), wv.size)
            assert same(gw, ww), "%s %s tol %g winners: %d of %d differ" % (what, name, tol, ndiff(gw, ww), ww.size)
            n += int((wv > 0).sum())
    gv, gw = votes_of(ctx, cv, NDIR, None, 1.0, want_votes=False)
    assert gv is None and same(gw, consensus(lr, dmin, NDIR, None, 1.0, lo, hi)[1]), what
    gv, gw = votes_of(ctx, cv, NDIR, maps["winner"], 1.0, want_winners=False)
    assert gw is None and same(gv, consensus(lr, dmin, NDIR, maps["winner"], 1.0, lo, hi)[0]), what
    assert n > 0, "no vote anywhere: the comparison is vacuous"


# shapes of one and several workgroups whose pixel counts are no multiple of 4 * PPW; label counts on a streaming instance (64, 128,
# 256) or padded to one (100 -> 128, 37 -> 64; the stride is read from the run); Hirschmueller and FH; 2, 4 and 8 passes.  A grid, not the product.
GRID = [
    # L, nx, ny, dmin, NDIR, MGM, FH, inf_frac
    (64, 37, 5, -30, 8, 3, 0, 0.03),
    (64, 37, 5, 3, 4, 3, 1, 0.0),
    (64, 13, 10, -70, 2, 1, 0, 0.03),
    (128, 13, 10, -64, 8, 3, 1, 0.03),
    (128, 13, 10, -200, 4, 4, 0, 0.0),
    (128, 37, 5, 5, 2, 3, 1, 0.03),
    (256, 37, 5, -128, 8, 3, 0, 0.03),
    (100, 37, 5, -50, 8, 3, 0, 0.03),
    (37, 13, 10, -20, 4, 3, 1, 0.03),
]


@pytest.mark.parametrize("case", GRID, ids=lambda c: "L%d-%dx%d-d%d-O%d-T%d-fh%d-inf%g" % c)
def test_matches_the_model_on_the_oracles_passes(ctx, oracle, case):
    L, nx, ny, dmin, NDIR, T, FH, inf_frac = case
    C = synth.raw_volume(nx, ny, L, seed=5000 + L + nx + NDIR, inf_frac=inf_frac)
    S, out, outc, lr = oracle.mgm(C, dmin, 8.0, 32.0, NDIR, T, FH, 1, dump_lr=True)
    vfit, _ = oracle.refine(S, dmin, "vfit", out, outc)
    cv = ctx.upload_volume(C, dmin)
    try:
        _, o, c = ctx.aggregate(cv, 8.0, 32.0, NDIR, T, FH, 1, None, "vfit", want_S=False)
        assert same(o, vfit)
        for p in range(NDIR):
            assert ndiff(ctx.debug_lr(cv, p), lr[p]) == 0, "pass %d: the device's Lr is not the oracle's" % p
        (_, fam) = families(ctx, lambda: votes_of(ctx, cv, NDIR, out, 1.0))
        assert "k_wta_consensus" in fam and len(fam) == 2, fam
        Lk = ctx.debug_lr_ptr(0, 0)[1]  # (a label count off the table may have run padded to one on it)
        assert ("k_wta_consensus_any" in fam) == (Lk % 64 != 0) and Lk >= L, (L, Lk, fam)
        check_against(ctx, cv, lr, dmin, NDIR, maps_to_judge(out, vfit, L, dmin, L + nx), what=str(case))
    finally:
        cv.free()


def test_the_generic_kernel_when_forced(ctx, oracle, monkeypatch):
    monkeypatch.setenv("MGM_HIP_WTA_CONSENSUS_ANY", "1")
    L, nx, ny, dmin, NDIR = 128, 37, 5, -64, 8
    C = synth.raw_volume(nx, ny, L, seed=5100, inf_frac=0.03)
    S, out, outc, lr = oracle.mgm(C, dmin, 8.0, 32.0, NDIR, 3, 0, 1, dump_lr=True)
    cv = ctx.upload_volume(C, dmin)
    try:
        ctx.aggregate(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, None, want_S=False)
        (_, fam) = families(ctx, lambda: votes_of(ctx, cv, NDIR, out, 1.0))
        assert fam == {"k_wta_consensus", "k_wta_consensus_any"}, fam
        check_against(ctx, cv, lr, dmin, NDIR, maps_to_judge(out, out, L, dmin, 3), what="forced")
    finally:
        cv.free()


def test_every_slot_of_a_batch_and_what_the_call_leaves_untouched(ctx, oracle):
    """a batch of two: both slots against the model; the maps of mgm_wta_windowed_dev and mgm_wta_runnerup_dev are the same before
    and after the votes"""
    L, nx, ny, dmin, NDIR = 128, 13, 10, -100, 8
    Cs = [synth.raw_volume(nx, ny, L, seed=5200 + v, inf_frac=0.03) for v in range(2)]
    ref = [oracle.mgm(C, dmin, 8.0, 32.0, NDIR, 3, 0, 1, dump_lr=True) for C in Cs]
    cvs = [ctx.upload_volume(C, dmin) for C in Cs]
    lo = ctx.upload_image(np.full((ny, nx), dmin + 5, np.float32))
    hi = ctx.upload_image(np.full((ny, nx), dmin + 90, np.float32))

    def others(cv):
        a = ctx.wta_windowed_dev(cv, NDIR, 1, "vfit", lo, hi)
        b = ctx.wta_runnerup_dev(cv, NDIR, 1, 1)
        res = [im.download()[0] for im in a + b]
        for im in a + b:
            im.free()
        return res
    try:
        _, outs, costs = ctx.aggregate_batch_dev(cvs, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
        for h in outs + costs:
            h.free()
        before = [others(cv) for cv in cvs]
        for v in (1, 0):
            S, out, outc, lr = ref[v]
            check_against(ctx, cvs[v], lr, dmin, NDIR, maps_to_judge(out, out, L, dmin, 7 + v), what="slot %d" % v)
        after = [others(cv) for cv in cvs]
        for b, a in zip(before, after):
            assert all(same(x, y) for x, y in zip(b, a))
        assert np.isfinite(before[0][0]).any()
    finally:
        for h in cvs + [lo, hi]:
            h.free()


def ragged_ranges(kind, nx, ny, dmin, dmax, seed):
    """alternating windows (as the runner-up search's refusal test has them), or random windows of 3 to 40 labels"""
    if kind == "alternating":
        lo = np.full((ny, nx), dmin, np.float32)
        hi = np.full((ny, nx), dmax, np.float32)
        lo[:, ::2] = dmin + 3
        hi[::2, 1::2] = dmax - 2
        return lo, hi
    rng = np.random.default_rng(seed)
    w = rng.integers(3, 41, (ny, nx))
    lo = rng.integers(dmin, dmax - w + 2)
    lo.flat[0], lo.flat[-1] = dmin, dmax - w.flat[-1] + 1
    return lo.astype(np.float32), (lo + w - 1).astype(np.float32)


@pytest.mark.parametrize("kind,nx,ny,dmin,dmax,NDIR,FH", [("alternating", 37, 5, -8, 0, 4, 0), ("random", 37, 9, -60, 0, 8, 0), ("random", 26, 10, -90, 10, 8, 1)])
def test_ragged_volumes_on_both_routes(oracle, kind, nx, ny, dmin, dmax, NDIR, FH):
    """MGM_HIP_REL=0: the dense hull, masked by the pixel's range; MGM_HIP_REL=2: the range-proportional copy.  The route is read from
    the timing table; both equal the model on the ragged oracle's passes, and each other."""
    u, v, _ = synth.stereo_pair(max(nx, 16), max(ny, 8), max(dmin, -8), 0, seed=11 + nx)
    u, v = np.ascontiguousarray(u[:, :ny, :nx]), np.ascontiguousarray(v[:, :ny, :nx])
    dminI, dmaxI = ragged_ranges(kind, nx, ny, dmin, dmax, 21 + ny)
    lo, hi = orc_mod.int_ranges(dminI, dmaxI)
    hmin, hmax = int(lo.min()), int(hi.max())
    Ca = oracle.costvolume_ranged(u, v, lo, hi, hmin, hmax, "none", "census", np.inf, 5)
    S, out, outc, lr = oracle.mgm_ranged(Ca, hmin, lo, hi, 8.0, 32.0, NDIR, 3, FH, 1, None, dump_lr=True)
    zlo, zhi = lo - hmin, hi - hmin
    maps = maps_to_judge(out, out, hmax - hmin + 1, hmin, 5)
    got = {}
    with mgm_amd.Context(0) as ctx:
        os.environ["MGM_HIP_REL"] = "2"
        try:
            cv = ctx.costvolume(u, v, dminI, dmaxI, "none", "census", float("inf"), 5)
        finally:
            os.environ.pop("MGM_HIP_REL", None)
        assert cv.dims == (nx, ny, hmin, hmax)
        for mode in ("2", "0"):
            os.environ["MGM_HIP_REL"] = mode
            try:
                ctx.timing(True)
                ctx.timing_reset()
                _, o, c = ctx.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, FH, 1, None, None)
                names = [n for n, _ in ctx.timings()]
                ctx.timing(False)
            finally:
                os.environ.pop("MGM_HIP_REL", None)
            assert same(o.download()[0], out)
            o.free(), c.free()
            assert ("k_pass_rel" in names) == (mode == "2"), (mode, names)
            (_, fam) = families(ctx, lambda: votes_of(ctx, cv, NDIR, out, 1.0))
            assert ("k_wta_consensus_rel" in fam) == (mode == "2") and len(fam) == 2, (mode, fam)
            check_against(ctx, cv, lr, hmin, NDIR, maps, zlo, zhi, what="%s route %s" % (kind, mode))
            got[mode] = [votes_of(ctx, cv, NDIR, maps["shifted"], tol) for tol in TOLS]
        for a, b in zip(got["2"], got["0"]):
            assert same(a[0], b[0]) and same(a[1], b[1])
        cv.free()


def test_refusals_leave_the_context_usable(ctx, oracle):
    nx, ny, L, dmin, NDIR = 37, 16, 64, -60, 4
    u, v, _ = synth.stereo_pair(nx, ny, -20, 0, seed=9)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    a = ctx.costvolume_dev(du, dv, dmin, dmin + L - 1, "none", "census")
    Ca = oracle.costvolume(u, v, dmin, dmin + L - 1, "none", "census")
    b = ctx.upload_volume(synth.raw_volume(nx, ny, L, seed=62), dmin)
    _, out, _, lr = oracle.mgm(Ca, dmin, 8.0, 32.0, NDIR, 3, 0, 1, dump_lr=True)
    ctx.aggregate(a, 8.0, 32.0, NDIR, 3, 0, 1, None, None, want_S=False)
    d = ctx.upload_image(out)
    INV = mgm_amd.MGM_ERR_INVALID

    def good(cv=a, lr_=lr, out_=out):
        gv, gw = votes_of(ctx, cv, NDIR, out_, 1.0)
        wv, ww = consensus(lr_, dmin, NDIR, out_, 1.0)
        return same(gv, wv) and same(gw, ww)

    def refused(fn, *args, **kw):
        with pytest.raises(mgm_amd.MgmError) as e:
            fn(*args, **kw)
        return e.value.code == INV

    def raw(cv, ndir, dh, tol, vh, wh):
        r = ctx.lib.mgm_wta_consensus_dev(ctx.h, cv.h if cv is not None else None, ndir, dh.h if dh is not None else None, tol,
                                          vh.h if vh is not None else None, wh.h if wh is not None else None)
        return r

    assert good()
    ok, ok2, win = ctx.new_image(nx, ny), ctx.new_image(nx, ny), ctx.new_image(nx, ny, NDIR)
    w1, w2, w3 = ctx.new_image(nx, ny + 1), ctx.new_image(nx, ny, 2), ctx.new_image(nx, ny, NDIR + 1)
    # null arguments; neither output; votes without d
    assert raw(None, NDIR, d, 1.0, ok, None) == INV and raw(a, NDIR, d, 1.0, None, None) == INV and raw(a, NDIR, None, 1.0, ok, None) == INV
    assert raw(a, NDIR, None, 1.0, None, win) == mgm_amd.MGM_OK and good()  # (d may be NULL when only winners is asked for)
    # sizes and channels
    for dh, vh, wh in ((w1, ok, None), (d, w1, None), (d, w2, None), (w2, ok, None), (d, ok, w3), (d, ok, ok2), (d, None, w1)):
        assert raw(a, NDIR, dh, 1.0, vh, wh) == INV, (dh, vh, wh)
    # aliasing
    assert raw(a, NDIR, d, 1.0, d, None) == INV and raw(a, NDIR, ok, 1.0, ok, win) == INV
    one = ctx.new_image(nx, ny, 1)
    # tol negative or not finite
    for tol in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert raw(a, NDIR, d, tol, ok, None) == INV, tol
    assert good()
    # a volume that was not part of the last aggregation; the right volume with another NDIR; NDIR out of range
    assert refused(ctx.wta_consensus_dev, b, NDIR, d) and good()
    assert raw(a, 8, d, 1.0, ok, None) == INV and raw(a, 0, d, 1.0, ok, None) == INV and raw(a, 9, d, 1.0, ok, None) == INV and good()
    # the filter: minvotes < 0, sizes, out == votes
    assert refused(ctx.consensus_filter_dev, d, ok, -1) and refused(ctx.consensus_filter_dev, d, w1, 3) and refused(ctx.consensus_filter_dev, d, ok, 3, out=w2)
    assert refused(ctx.consensus_filter_dev, d, ok, 3, out=ok) and refused(ctx.consensus_filter_dev, d, d, 3)
    assert good()
    # a volume refilled since its aggregation
    assert ctx.costvolume_dev(du, dv, dmin, dmin + L - 1, "none", "census", into=a) is a
    assert refused(ctx.wta_consensus_dev, a, NDIR, d)
    ctx.aggregate(a, 8.0, 32.0, NDIR, 3, 0, 1, None, None, want_S=False)
    assert good()
    # another aggregation became the context's last
    ctx.aggregate(b, 8.0, 32.0, NDIR, 3, 0, 1, None, None, want_S=False)
    assert refused(ctx.wta_consensus_dev, a, NDIR, d)
    ctx.aggregate(a, 8.0, 32.0, NDIR, 3, 0, 1, None, None, want_S=False)
    assert good()
    # a trimmed context
    ctx.trim()
    assert refused(ctx.wta_consensus_dev, a, NDIR, d)
    ctx.aggregate(a, 8.0, 32.0, NDIR, 3, 0, 1, None, None, want_S=False)
    assert good()
    for h in (a, b, d, ok, ok2, win, w1, w2, w3, one, du, dv):
        h.free()


def test_an_earlier_chunk_of_a_chunked_batch_is_refused(ctx, oracle):
    """a workspace limit that holds two volumes' passes: a batch of three runs as several launches, and only the last one's passes
    are still there -- its volume votes, the first one is MGM_ERR_INVALID"""
    nx, ny, L, dmin, NDIR = 96, 40, 128, -5, 8
    Cs = [synth.raw_volume(nx, ny, L, seed=71 + v) for v in range(3)]
    cvs = [ctx.upload_volume(C, dmin) for C in Cs]
    ctx.set_workspace_limit(int(2.6 * 4 * nx * ny * L * NDIR))
    try:
        ctx.timing(True)
        ctx.timing_reset()
        _, outs, costs = ctx.aggregate_batch_dev(cvs, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
        ctx.synchronize()
        launches = sum(1 for n, _ in ctx.timings() if n in ("k_pass2", "k_pass"))
        ctx.timing(False)
        assert launches >= 2
        _, out, _, lr = oracle.mgm(Cs[2], dmin, 8.0, 32.0, NDIR, 3, 0, 1, dump_lr=True)
        wv, ww = consensus(lr, dmin, NDIR, out, 1.0)
        gv, gw = votes_of(ctx, cvs[2], NDIR, out, 1.0)
        assert same(gv, wv) and same(gw, ww)
        d = ctx.upload_image(out)
        with pytest.raises(mgm_amd.MgmError) as e:
            ctx.wta_consensus_dev(cvs[0], NDIR, d)
        assert e.value.code == mgm_amd.MGM_ERR_INVALID
        gv, _ = votes_of(ctx, cvs[2], NDIR, out, 1.0)
        assert same(gv, wv)
    finally:
        ctx.set_workspace_limit(0)
    for h in cvs + outs + costs + [d]:
        h.free()


def test_a_refilled_range_proportional_copy_is_refused(oracle):
    nx, ny, dmin, dmax, NDIR = 37, 9, -60, 0, 8
    u, v, _ = synth.stereo_pair(nx, ny, -8, 0, seed=13)
    dminI, dmaxI = ragged_ranges("random", nx, ny, dmin, dmax, 33)
    lo, hi = orc_mod.int_ranges(dminI, dmaxI)
    hmin, hmax = int(lo.min()), int(hi.max())
    with mgm_amd.Context(0) as ctx:
        du, dv, dlo, dhi = (ctx.upload_image(x) for x in (u, v, dminI, dmaxI))
        os.environ["MGM_HIP_REL"] = "2"
        try:
            cv = ctx.costvolume_ranged_dev(du, dv, dlo, dhi, hmin, hmax, "none", "census", float("inf"), 5)
            ctx.timing(True)
            _, o, c = ctx.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
            names = [n for n, _ in ctx.timings()]
            ctx.timing(False)
            assert "k_pass_rel" in names, names
            votes, _ = ctx.wta_consensus_dev(cv, NDIR, o)
            assert (votes.download() > 0).any()
            assert ctx.costvolume_ranged_dev(du, dv, dlo, dhi, hmin, hmax, "none", "census", float("inf"), 5, into=cv) is cv
            with pytest.raises(mgm_amd.MgmError) as e:
                ctx.wta_consensus_dev(cv, NDIR, o)
            assert e.value.code == mgm_amd.MGM_ERR_INVALID
            _, o2, c2 = ctx.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
            votes2, _ = ctx.wta_consensus_dev(cv, NDIR, o2)
            assert same(votes2.download(), votes.download())
        finally:
            os.environ.pop("MGM_HIP_REL", None)


def test_the_filter(ctx):
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    d = np.array([[1.5, nan, 3.0, inf, -2.0, 0.0, -0.0, 7.25]], np.float32)
    v = np.array([[8.0, 8.0, 5.0, 6.0, 0.0, nan, 6.0, 5.999]], np.float32)
    dd, dv = ctx.upload_image(d), ctx.upload_image(v)
    for k in (0, 1, 6, 8, 9):
        o = ctx.consensus_filter_dev(dd, dv, k)
        assert same(o.download()[0], consensus_filter(d, v, k)), k
        o.free()
    assert same(consensus_filter(d, v, 0), d) and np.isnan(consensus_filter(d, v, 6)[0, [2, 4, 7]]).all()
    o = ctx.consensus_filter_dev(dd, dv, 6, out=dd)  # out aliasing d
    assert o is dd and same(dd.download()[0], consensus_filter(d, v, 6))
    # a larger map, several workgroups, in place
    rng = np.random.default_rng(5)
    D = (rng.random((45, 257)) * 60 - 30).astype(np.float32)
    V = rng.integers(0, 9, D.shape).astype(np.float32)
    D[rng.random(D.shape) < 0.1] = nan
    a, b = ctx.upload_image(D), ctx.upload_image(V)
    ctx.consensus_filter_dev(a, b, 6, out=a)
    assert same(a.download()[0], consensus_filter(D, V, 6))
    for h in (dd, dv, a, b):
        h.free()
