"""mgm_wta_runnerup_dev and mgm_uniqueness_dev: the runner-up search over the Lr volumes of the context's last
aggregation and the confidence / uniqueness filter, bit for bit against the numpy model (tests/runnerup_model.py) on the
corrected S the same aggregation hands out; the entry points' refusals; -c FILE and MGM_UNIQUENESS of the command line against
the same steps through the Python API."""
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
from helpers import ndiff
from mgm_amd import synth
from runnerup_model import CLI_RADIUS, CLI_RATIO, PAIR, runnerup, uniqueness

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
CONV = os.path.join(ROOT, "mgm_amd", "bin", "imgconv")
NAMES = ("out2", "cost2", "out1", "cost1")


def first_label(kind, L):
    """dmin of a range of L labels that is all negative, all positive or straddles 0."""
    return {"neg": -2 - (L - 1), "pos": 3, "mid": -(L // 2)}[kind]


def same(got, want):
    """bit for bit, NaN payloads aside -- and NaN in the same places"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


def radii(L):
    return (0, 1, 2, 5, L)


def search(ctx, cv, NDIR, fix, radius, want_first=True):
    """the entry's maps as host arrays (None for those not asked for)"""
    imgs = ctx.wta_runnerup_dev(cv, NDIR, fix, radius, want_first=want_first)
    res = [im.download()[0] if im is not None else None for im in imgs]
    for im in imgs:
        if im is not None:
            im.free()
    return res


def compare(got, Sd, dmin, radius, what=""):
    want = runnerup(Sd, dmin, radius)
    for name, g, w in zip(NAMES, got, want):
        assert same(g, w), "%s radius %d %s: %d of %d differ" % (what, radius, name, ndiff(g, w), w.size)
    return want


def check(ctx, C, dmin, NDIR=8, fix=1, MGM_=3, FH=0, P1=8.0, P2=32.0, rs=None):
    """aggregate C, search at every radius, compare with the model on the downloaded S; returns {radius: the model's maps}"""
    cv = ctx.upload_volume(C, dmin)
    try:
        S, _, _ = ctx.aggregate(cv, P1, P2, NDIR, MGM_, FH, fix, None, None, want_S=True)
        Sd = S.download()
        S.free()
        return {r: compare(search(ctx, cv, NDIR, fix, r), Sd, dmin, r) for r in (rs if rs is not None else radii(C.shape[2]))}
    finally:
        cv.free()


# L: 1..4 (fewer labels than 2*radius + 2), 63 / 65 / 300 / 1100 (strides with padding lanes or off the table), every streaming
# instance (64 .. 1024, at most 4 and up to 8 passes); sizes whose pixel counts are no multiple of 4 * PPW -- 1x1, 37x1, 37x5,
# 130x3, 257x2, from 384 labels up 37x5 at most (a wave per PPW pixels: one turn of the grid-stride loop; several turns are
# test_several_turns_of_the_grid_stride_loop's); NDIR 1, 3, 4, 8; over-count fix on and off; TSGM 1 and 3; Hirschmueller and FH; +INF costs or none; ranges all
# negative / all positive / across 0.  Every case runs the radii 0, 1, 2, 5 and L.  A grid, not the product.
GRID = [
    # L, nx, ny, range, NDIR, fix, MGM, FH, inf_frac
    (1, 37, 1, "neg", 4, 1, 1, 0, 0.0),
    (2, 37, 5, "mid", 8, 0, 3, 0, 0.03),
    (3, 1, 1, "pos", 1, 1, 3, 1, 0.0),
    (4, 130, 3, "mid", 3, 1, 3, 0, 0.03),
    (63, 37, 5, "neg", 8, 1, 3, 1, 0.03),
    (63, 257, 2, "mid", 4, 0, 1, 0, 0.0),
    (64, 130, 3, "mid", 8, 1, 3, 0, 0.03),
    (64, 257, 2, "pos", 3, 0, 3, 1, 0.0),
    (64, 1, 1, "neg", 1, 1, 1, 0, 0.0),
    (65, 130, 3, "mid", 8, 0, 1, 0, 0.03),
    (65, 37, 5, "pos", 4, 1, 3, 1, 0.0),
    (128, 257, 2, "neg", 8, 1, 3, 0, 0.03),
    (128, 37, 5, "mid", 4, 0, 3, 1, 0.03),
    (192, 130, 3, "mid", 8, 1, 1, 0, 0.0),
    (192, 37, 1, "pos", 3, 1, 3, 0, 0.03),
    (256, 257, 2, "mid", 8, 1, 3, 1, 0.03),
    (256, 130, 3, "neg", 4, 1, 3, 0, 0.0),
    (256, 37, 5, "pos", 1, 0, 1, 0, 0.03),
    (300, 257, 2, "mid", 8, 1, 3, 0, 0.03),
    (300, 37, 5, "neg", 4, 0, 1, 1, 0.0),
    (384, 37, 5, "mid", 8, 1, 3, 0, 0.03),
    (384, 37, 1, "pos", 4, 1, 1, 0, 0.0),
    (512, 37, 5, "neg", 8, 0, 3, 0, 0.03),
    (512, 37, 1, "mid", 3, 1, 3, 1, 0.0),
    (768, 37, 5, "mid", 8, 1, 1, 0, 0.03),
    (768, 1, 1, "pos", 4, 0, 3, 0, 0.0),
    (1024, 37, 5, "mid", 8, 1, 3, 0, 0.03),
    (1024, 37, 1, "neg", 1, 1, 1, 0, 0.0),
    (1100, 37, 1, "mid", 8, 1, 3, 0, 0.03),
    (1100, 37, 5, "pos", 4, 0, 1, 0, 0.0),
]


@pytest.mark.parametrize("case", GRID, ids=lambda c: "L%d-%dx%d-%s-O%d-fix%d-T%d-fh%d-inf%g" % c)
def test_matches_the_model(ctx, case):
    L, nx, ny, rng, NDIR, fix, T, FH, inf_frac = case
    C = synth.raw_volume(nx, ny, L, seed=3000 + L + nx, inf_frac=inf_frac)
    res = check(ctx, C, first_label(rng, L), NDIR, fix, T, FH)
    assert np.isnan(res[L][0]).all() and np.isposinf(res[L][1]).all()          # a radius of L: no runner-up anywhere
    if L > 1:
        assert np.isfinite(res[0][1]).any()                                    # ... and the test is not vacuous


@pytest.mark.parametrize("case", [GRID[1], GRID[4], GRID[6], GRID[15], GRID[18]], ids=lambda c: "L%d-%dx%d" % c[:3])
def test_the_generic_kernel_matches_the_model(ctx, case, monkeypatch):
    """MGM_HIP_WTA_RUNNERUP_ANY=1: every label count on the kernel that strides the labels over the lanes."""
    monkeypatch.setenv("MGM_HIP_WTA_RUNNERUP_ANY", "1")
    L, nx, ny, rng, NDIR, fix, T, FH, inf_frac = case
    C = synth.raw_volume(nx, ny, L, seed=4000 + L + nx, inf_frac=0.03)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        check(ctx, C, first_label(rng, L), NDIR, fix, T, FH)
        assert families(ctx) == {"k_wta_runnerup_any"}
    finally:
        ctx.timing(False)


def families(ctx):
    """the kernel families the runner-up searches since the last timing_reset ran on (their second name in the timing table)"""
    names = [n for n, _ in ctx.timings()]
    assert "k_wta_runnerup" in names
    return {n for n in names if n.startswith("k_wta_runnerup_")}


# (L, nx, ny, NDIR, forced generic, workgroups per CU or 0, the family): pixel counts beyond what one turn of the grid takes.
# MGM_HIP_WTA_RUNNERUP_WG=1 caps the grid at one workgroup per CU -- at most 304 * 4 waves of PPW = 3 / 8 / 1 pixels, fewer than
# the 5200 / 11565 / 5200 pixels of the first three (tests/test_runnerup_plan.py holds the planner to that); the last one runs
# the grid as it is: 800000 pixels of 2 labels on the generic kernel against the cap of 768 workgroups per CU (two turns on 256 CUs).
TURNS = [
    (256, 130, 40, 8, 0, 1, "k_wta_runnerup_stream"),
    (64, 257, 45, 4, 0, 1, "k_wta_runnerup_stream"),
    (300, 130, 40, 8, 0, 1, None),
    (2, 1000, 800, 1, 1, 0, "k_wta_runnerup_any"),
]


@pytest.mark.parametrize("case", TURNS, ids=lambda c: "L%d-%dx%d-O%d-any%d-wg%d" % c[:6])
def test_several_turns_of_the_grid_stride_loop(ctx, case, monkeypatch):
    L, nx, ny, NDIR, force, wg, family = case
    if force:
        monkeypatch.setenv("MGM_HIP_WTA_RUNNERUP_ANY", "1")
    if wg:
        monkeypatch.setenv("MGM_HIP_WTA_RUNNERUP_WG", str(wg))
    C = synth.raw_volume(nx, ny, L, seed=5000 + L + nx, inf_frac=0.03)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        res = check(ctx, C, first_label("mid", L), NDIR, 1, 1, 0, rs=(0, 1))
        assert family is None or families(ctx) == {family}
    finally:
        ctx.timing(False)
    assert np.isfinite(res[0][3]).all() and np.isfinite(res[0][1]).mean() > 0.9   # winners everywhere, runner-ups nearly


@pytest.mark.parametrize("L,nx,ny", [(64, 130, 3), (3, 37, 5), (256, 257, 2), (70, 37, 1)])
def test_ties(ctx, L, nx, ny):
    """integer costs 0 / 1 and no penalties: S = NDIR * C - (NDIR - 1) * C in two values; in the row of a single value the
    winner is label 0 of the range and the runner-up label radius + 1"""
    rng = np.random.default_rng(L)
    C = rng.integers(0, 2, (ny, nx, L)).astype(np.float32)
    C[0] = 1.0
    dmin = first_label("mid", L)
    res = check(ctx, C, dmin, 8, 1, 3, 0, P1=0.0, P2=0.0)
    for r, (o2, c2, o1, c1) in res.items():
        assert (o1[0] == dmin).all() and (c1[0] == 1).all()
        if r + 1 < L:
            assert (o2[0] == dmin + r + 1).all() and (c2[0] == 1).all()
        else:
            assert np.isnan(o2[0]).all() and np.isposinf(c2[0]).all()


@pytest.mark.parametrize("L", [9, 64, 200])
@pytest.mark.parametrize("fix", [0, 1])
def test_crafted_pixels(ctx, L, fix):
    """One pass along +x, TSGM 1, no penalties: S is C wherever C is finite, so each pixel's S is crafted through its costs.  The
    all-INF pixel is the last of its row: no pixel follows it in that pass."""
    nx, ny, dmin, radius = 12, 2, -4, 2
    INF = np.float32(np.inf)
    rng = np.random.default_rng(7)
    C = rng.integers(10, 31, (ny, nx, L)).astype(np.float32)
    C[:, 1] = INF
    C[:, 1, 4] = 3.0                                   # exactly one finite label
    C[:, 2] = INF
    C[:, 2, 3:6] = (2.0, 1.0, 2.0)                     # finite labels only within `radius` of the winner
    C[:, 3, 0] = 0.0                                   # the winner at label 0
    C[:, 4, L - 1] = 0.0                               # the winner at label L - 1
    C[:, 5, 5], C[:, 5, 3:5], C[:, 5, 2] = 0.0, 0.5, 1.0   # the runner-up just below the exclusion zone, cheaper labels inside it
    C[:, 6, 3], C[:, 6, 4:6], C[:, 6, 6] = 0.0, 0.5, 1.0   # ... just above it
    C[:, nx - 1] = INF                                 # no finite label
    o2, c2, o1, c1 = check(ctx, C, dmin, 1, fix, 1, 0, P1=0.0, P2=0.0, rs=(radius,))[radius]
    lab = lambda o: np.float32(o + dmin)
    for m in (o2, o1):
        assert np.isnan(m[:, nx - 1]).all()
    for m in (c2, c1):
        assert np.isposinf(m[:, nx - 1]).all()
    assert (o1[:, 1] == lab(4)).all() and (c1[:, 1] == 3).all() and np.isnan(o2[:, 1]).all() and np.isposinf(c2[:, 1]).all()
    assert (o1[:, 2] == lab(4)).all() and (c1[:, 2] == 1).all() and np.isnan(o2[:, 2]).all() and np.isposinf(c2[:, 2]).all()
    assert (o1[:, 3] == lab(0)).all() and (c1[:, 3] == 0).all() and (o2[:, 3] >= lab(3)).all() and (c2[:, 3] >= 10).all()
    assert (o1[:, 4] == lab(L - 1)).all() and (o2[:, 4] <= lab(L - 4)).all() and (c2[:, 4] >= 10).all()
    assert (o1[:, 5] == lab(5)).all() and (o2[:, 5] == lab(2)).all() and (c2[:, 5] == 1).all()
    assert (o1[:, 6] == lab(3)).all() and (o2[:, 6] == lab(6)).all() and (c2[:, 6] == 1).all()


@pytest.mark.parametrize("L,nx", [(64, 130), (256, 257)])
def test_compact_census_volume(ctx, L, nx):
    """a volume built on the device from single-word census descriptors: one byte per cost, read under the over-count fix"""
    ny, dmin = 6, -(L - 8)
    u, v, _ = synth.stereo_pair(nx, ny, -12, 0, seed=9)
    du, dv = ctx.upload_image(u), ctx.upload_image(v[:, :, : nx - 3])
    cv = ctx.costvolume_dev(du, dv, dmin, dmin + L - 1, "none", "census", census_win=5)
    S, o0, c0 = ctx.aggregate_dev(cv, 8.0, 32.0, 8, 3, 0, 1, None, "vfit", want_S=True)
    Sd = S.download()
    for r in (1, 5):
        compare(search(ctx, cv, 8, 1, r), Sd, dmin, r, "census")
    for h in (du, dv, cv, S, o0, c0):
        h.free()


def test_two_byte_cost_codes(ctx):
    """absolute differences of a 3-channel pair: costs up to 765, two bytes per code, read under the over-count fix"""
    nx, ny, L, dmin = 130, 3, 128, -100
    u, v, _ = synth.stereo_pair(nx, ny, -75, 0, seed=12, nch=3)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    cv = ctx.costvolume_dev(du, dv, dmin, dmin + L - 1, "none", "ad", float("inf"), 3)
    S, o0, c0 = ctx.aggregate_dev(cv, 8.0, 32.0, 8, 3, 0, 1, None, None, want_S=True)
    Sd = S.download()
    assert cv.download().max() > 255
    for r in (0, 2):
        compare(search(ctx, cv, 8, 1, r), Sd, dmin, r, "ad x 3")
    for h in (du, dv, cv, S, o0, c0):
        h.free()


def test_both_slots_of_a_batch(ctx):
    nx, ny, L, dmin, NDIR = 130, 3, 128, -100, 8
    Cs = [synth.raw_volume(nx, ny, L, seed=s, inf_frac=0.02) for s in (31, 32)]
    cvs = [ctx.upload_volume(C, dmin) for C in Cs]
    S, outs, costs = ctx.aggregate_batch_dev(cvs, 8.0, 32.0, NDIR, 3, 0, 1, None, "vfit", want_S=True)
    for k in (1, 0):
        compare(search(ctx, cvs[k], NDIR, 1, 1), S[k].download(), dmin, 1, "slot %d" % k)
    for h in cvs + S + outs + costs:
        h.free()


def test_only_the_runner_up(ctx):
    """out1 / cost1 NULL: the same two maps"""
    nx, ny, L, dmin = 37, 5, 64, -30
    cv = ctx.upload_volume(synth.raw_volume(nx, ny, L, seed=61, inf_frac=0.02), dmin)
    S, _, _ = ctx.aggregate(cv, 8.0, 32.0, 4, 3, 0, 1, None, None, want_S=True)
    o2, c2, o1, c1 = search(ctx, cv, 4, 1, 1, want_first=False)
    w = runnerup(S.download(), dmin, 1)
    assert o1 is None and c1 is None and same(o2, w[0]) and same(c2, w[1])
    cv.free(), S.free()


def test_the_call_leaves_the_contexts_record_alone(ctx):
    """the two other searches of the last aggregation give the same maps before and after a runner-up call"""
    nx, ny, L, dmin, NDIR = 130, 3, 64, -40, 8
    cv = ctx.upload_volume(synth.raw_volume(nx, ny, L, seed=71, inf_frac=0.02), dmin)
    ctx.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, "vfit")
    lo = ctx.upload_image(np.full((ny, nx), dmin + 5, np.float32))
    hi = ctx.upload_image(np.full((ny, nx), dmin + L - 9, np.float32))

    def others():
        a = ctx.wta_right_dev(cv, NDIR, 1, "vfit", nx + 2)
        b = ctx.wta_windowed_dev(cv, NDIR, 1, "vfit", lo, hi)
        res = [im.download()[0] for im in a + b]
        for im in a + b:
            im.free()
        return res

    before = others()
    got = search(ctx, cv, NDIR, 1, 2)
    after = others()
    assert all(same(x, y) for x, y in zip(before, after)) and np.isfinite(before[1]).any() and np.isfinite(before[3]).any()
    assert same(got[0], search(ctx, cv, NDIR, 1, 2)[0]) and np.isfinite(got[1]).any()
    for h in (cv, lo, hi):
        h.free()


def test_uniqueness_against_the_model(ctx):
    nan, inf = np.nan, np.inf
    # plain, conf == ratio, just below it, 0/0, INF/INF, no runner-up, negative costs (three ways), a NaN d, -INF, NaN costs
    c1 = np.array([1.0, 3.0, 3.0001, 0.0, inf, 2.0, -4.0, -1.0, -1.0, 1.0, -inf, nan, 1.0, 0.0, 5.0], np.float32)
    c2 = np.array([2.0, 4.0, 4.0, 0.0, inf, inf, -2.0, 3.0, 0.0, 8.0, 1.0, 1.0, nan, 7.0, 5.0], np.float32)
    d = np.array([5.0, 6.0, 7.0, 8.0, nan, 9.0, 10.0, 11.0, 12.0, nan, 13.0, 14.0, 15.0, -0.5, inf], np.float32)
    rng = np.random.default_rng(3)
    n = 37 * 5 - len(d)
    c1 = np.concatenate([c1, rng.random(n).astype(np.float32) * 40]).reshape(5, 37)
    c2 = np.concatenate([c2, rng.random(n).astype(np.float32) * 40 + 20]).reshape(5, 37)
    d = np.concatenate([d, rng.random(n).astype(np.float32) * 64 - 32]).reshape(5, 37)
    dd, d1, d2 = ctx.upload_image(d), ctx.upload_image(c1), ctx.upload_image(c2)
    for ratio in (0.25, 0.0, 1.0, 0.6):
        wo, wc = uniqueness(d, c1, c2, ratio)
        assert wc[0, 1] == 0.25 and wc[0, 2] < 0.25                       # conf exactly at the ratio keeps d, just below it does not
        o, c = ctx.uniqueness_dev(dd, d1, d2, ratio)                       # both
        assert same(o.download()[0], wo) and same(c.download()[0], wc)
        o2, none = ctx.uniqueness_dev(dd, d1, d2, ratio, want_conf=False)  # only out
        assert none is None and same(o2.download()[0], wo)
        none, c2_ = ctx.uniqueness_dev(dd, d1, d2, ratio, out=False)       # only conf
        assert none is None and same(c2_.download()[0], wc)
        for h in (o, c, o2, c2_):
            h.free()
    wo, wc = uniqueness(d, c1, c2, 0.25)
    assert not np.isnan(wo[0, 1]) and np.isnan(wo[0, 2]) and not np.isnan(wo[0, 3]) and np.isnan(wo[0, 6])
    o, c = ctx.uniqueness_dev(dd, d1, d2, 0.25, out=dd)                    # out aliasing d
    assert o is dd and same(dd.download()[0], wo) and same(c.download()[0], wc)
    for h in (dd, d1, d2, c):
        h.free()


def test_refusals_leave_the_context_usable(ctx):
    nx, ny, L, dmin, NDIR = 37, 5, 64, -30, 4
    a = ctx.upload_volume(synth.raw_volume(nx, ny, L, seed=41, inf_frac=0.02), dmin)
    b = ctx.upload_volume(synth.raw_volume(nx, ny, L, seed=42), dmin)
    S, _, _ = ctx.aggregate(a, 8.0, 32.0, NDIR, 3, 0, 1, None, "vfit", want_S=True)
    Sd = S.download()

    def good():
        compare(search(ctx, a, NDIR, 1, 1), Sd, dmin, 1)
        return True

    def refused(code, fn, *args, **kw):
        with pytest.raises(mgm_amd.MgmError) as e:
            fn(*args, **kw)
        return e.value.code == code

    assert good()
    # a ragged volume (built from range images)
    u, v, _ = synth.stereo_pair(nx, ny, -8, 0, seed=3)
    lo = np.full((ny, nx), -8, np.float32)
    hi = np.zeros((ny, nx), np.float32)
    lo[:, ::2] = -5
    ragged = ctx.costvolume(u, v, lo, hi, "none", "ad")
    assert refused(mgm_amd.MGM_ERR_UNSUPPORTED, ctx.wta_runnerup_dev, ragged, NDIR, 1, 1) and good()
    # a volume that was not part of the last aggregation; the right volume with another NDIR; a negative radius
    assert refused(mgm_amd.MGM_ERR_INVALID, ctx.wta_runnerup_dev, b, NDIR, 1, 1) and good()
    assert refused(mgm_amd.MGM_ERR_INVALID, ctx.wta_runnerup_dev, a, 8, 1, 1) and good()
    assert refused(mgm_amd.MGM_ERR_INVALID, ctx.wta_runnerup_dev, a, NDIR, 1, -1) and good()
    # images of another size, of two channels
    w1, w2, w3 = ctx.new_image(nx, ny + 1), ctx.new_image(nx, ny + 1), ctx.new_image(nx, ny, 2)
    ok = ctx.new_image(nx, ny)
    assert refused(mgm_amd.MGM_ERR_INVALID, ctx.wta_runnerup_dev, a, NDIR, 1, 1, out2=w1, cost2=w2) and good()
    assert refused(mgm_amd.MGM_ERR_INVALID, ctx.wta_runnerup_dev, a, NDIR, 1, 1, out2=ok, cost2=w3) and good()
    # the filter: ratios outside [0, 1] or not finite, both outputs NULL, another size
    o2, c2, o1, c1 = ctx.wta_runnerup_dev(a, NDIR, 1, 1)
    for ratio in (-0.1, 1.5, float("nan"), float("inf")):
        assert refused(mgm_amd.MGM_ERR_INVALID, ctx.uniqueness_dev, o1, c1, c2, ratio)
    assert refused(mgm_amd.MGM_ERR_INVALID, ctx.uniqueness_dev, o1, c1, c2, 0.5, out=False, want_conf=False)
    assert refused(mgm_amd.MGM_ERR_INVALID, ctx.uniqueness_dev, o1, c1, w1, 0.5)
    assert refused(mgm_amd.MGM_ERR_INVALID, ctx.uniqueness_dev, o1, c1, c2, 0.5, out=w1)
    wo, wc = uniqueness(*[im.download()[0] for im in (o1, c1, c2)], 0.5)
    fo, fc = ctx.uniqueness_dev(o1, c1, c2, 0.5)
    assert same(fo.download()[0], wo) and same(fc.download()[0], wc) and good()
    for h in (a, b, S, ragged, w1, w2, w3, ok, o2, c2, o1, c1, fo, fc):
        h.free()


def test_pipelined_context_runs_the_deferred_aggregation_first():
    nx, ny, L, dmin, NDIR = 130, 3, 64, -20, 8
    C = synth.raw_volume(nx, ny, L, seed=51, inf_frac=0.02)
    res = []
    for depth in (1, 2):
        with mgm_amd.Context(0) as c2:
            if depth > 1:
                c2.set_pipeline(depth)
            cv = c2.upload_volume(C, dmin)
            c2.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, "vfit")
            res.append(search(c2, cv, NDIR, 1, 1))
    assert all(same(x, y) for x, y in zip(res[1], res[0])) and np.isfinite(res[0][1]).any()


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def read_tif(path):
    npy = path + ".npy"
    subprocess.run([CONV, path, npy], check=True, timeout=60)
    return np.load(npy).astype(np.float32).squeeze()


def test_command_line(ctx, tmp_path):
    """the 96 x 40 synthetic pair at the ratio tests/test_runnerup_model.py chose on the oracle (it rejects 8 % of the pixels)"""
    p = PAIR
    nx, ny, dmin, dmax, NDIR = p["nx"], p["ny"], p["dmin"], p["dmax"], p["NDIR"]
    u, v, _ = synth.stereo_pair(nx, ny, dmin, dmax)
    fu, fv = str(tmp_path / "u.npy"), str(tmp_path / "v.npy")
    np.save(fu, u[0]), np.save(fv, v[0])
    args = "-r -16 -R 0 -t census -s vfit -O 8".split()
    f = {k: str(tmp_path / (k + ".tif")) for k in ("plain", "out", "conf", "nolr", "rfl", "rflnolr", "c0", "conf0")}
    env = dict(MGM_UNIQUENESS=repr(CLI_RATIO), MGM_UNIQUENESS_RADIUS=str(CLI_RADIUS))
    r0 = run_cli(args + [fu, fv, f["plain"]], {})
    r1 = run_cli(args + ["-c", f["conf"], "-l", f["nolr"], fu, fv, f["out"]], env)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert r1.stdout == r0.stdout and r0.stdout.splitlines() == ["-16 0", "01234567", "01234567"]

    # the same steps through the Python API: both runs in one batched launch, the search and the filter on each slot, the
    # map before the left-right test, the test both ways
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    cvL = ctx.costvolume_dev(du, dv, dmin, dmax, "none", "census")
    cvR = ctx.costvolume_dev(dv, du, -dmax, -dmin, "none", "census")
    _, outs, costs = ctx.aggregate_batch_dev([cvL, cvR], p["P1"], p["P2"], NDIR, p["TSGM"], 0, 1, None, "vfit")
    unfiltered = outs[0].download()[0]
    conf = None
    for cv, o in zip((cvL, cvR), outs):
        o2, c2, _, c1 = ctx.wta_runnerup_dev(cv, NDIR, 1, CLI_RADIUS)
        _, cf = ctx.uniqueness_dev(o, c1, c2, CLI_RATIO, out=o)
        conf = cf.download()[0] if conf is None else conf
    nolr = outs[0].download()[0]
    final = ctx.leftright_dev(outs[0], outs[1], 1.0).download()[0]
    assert same(read_tif(f["conf"]), conf) and same(read_tif(f["nolr"]), nolr) and same(read_tif(f["out"]), final)
    rejected = np.isnan(nolr) & ~np.isnan(unfiltered)
    print("the filter rejected %.4f of the left run's pixels" % rejected.mean())
    assert 0.01 <= rejected.mean() <= 0.5 and not same(read_tif(f["plain"]), final)

    # -c alone: the same confidence map, the maps of the plain command
    r2 = run_cli(args + ["-c", f["conf0"], fu, fv, f["c0"]], {})
    assert r2.returncode == 0 and r2.stdout == r0.stdout
    assert same(read_tif(f["conf0"]), conf) and same(read_tif(f["c0"]), read_tif(f["plain"]))

    # right from left: only the left map is filtered, the right map is read out of the left run as it is
    r3 = run_cli(args + ["-l", f["rflnolr"], fu, fv, f["rfl"]], dict(env, MGM_RIGHT_FROM_LEFT="1"))
    assert r3.returncode == 0 and r3.stdout.splitlines() == ["-16 0", "01234567", "right from left"]
    _, oL, cL = ctx.aggregate_dev(cvL, p["P1"], p["P2"], NDIR, p["TSGM"], 0, 1, None, "vfit")
    o2, c2, _, c1 = ctx.wta_runnerup_dev(cvL, NDIR, 1, CLI_RADIUS)
    ctx.uniqueness_dev(oL, c1, c2, CLI_RATIO, out=oL, want_conf=False)
    oR, _ = ctx.wta_right_dev(cvL, NDIR, 1, "vfit", nx)
    assert same(read_tif(f["rflnolr"]), oL.download()[0])
    assert same(read_tif(f["rfl"]), ctx.leftright_dev(oL, oR, 1.0).download()[0])

    # what the mode does not combine with: exit code 2
    for extra, e in ((["-S", "2"], {}), ([], {"TSGM_ITER": "2"}), (["-m", fu, "-M", fu], {}), ([], {"MGM_DEVICES": "0,1"})):
        r = run_cli(args + extra + [fu, fv, f["out"]], dict(env, **e))
        assert r.returncode == 2 and "does not combine with" in r.stderr, (extra, e, r.stderr)
