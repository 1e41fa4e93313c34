"""mgm_wta_right_dev ("right from left"): the right view's winners read out of the left run's Lr volumes, bit
for bit against the numpy model (tests/wta_right_model.py) on the corrected S the same aggregation hands out; the entry
point's refusals; the command-line switch MGM_RIGHT_FROM_LEFT=1 against Context.pair_right_from_left."""
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
from helpers import ndiff
from mgm_amd import synth
from wta_right_model import wta_right

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
CONV = os.path.join(ROOT, "mgm_amd", "bin", "imgconv")


def first_label(kind, L):
    """dmin of a range of L labels that is all negative, all positive or straddles 0."""
    return {"neg": -2 - (L - 1), "pos": 3, "mid": -(L // 2)}[kind]


def same(got, want):
    """bit for bit, NaN payloads aside -- and NaN in the same places"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


def check(ctx, C, dmin, vnx, NDIR=8, fix=1, refine=None, MGM_=3, FH=0, P1=8.0, P2=32.0):
    """aggregate C, search the right view, compare with the model on the downloaded S; returns the model's maps"""
    cv = ctx.upload_volume(C, dmin)
    try:
        S, _, _ = ctx.aggregate(cv, P1, P2, NDIR, MGM_, FH, fix, None, refine, want_S=True)
        Sd = S.download()
        S.free()
        o, c = ctx.wta_right_dev(cv, NDIR, fix, refine, vnx)
        go, gc = o.download()[0], c.download()[0]
        o.free(), c.free()
    finally:
        cv.free()
    wo, wc = wta_right(Sd, dmin, vnx, refine)
    assert same(gc, wc), "outcost: %d of %d differ" % (ndiff(gc, wc), wc.size)
    assert same(go, wo), "out: %d of %d differ" % (ndiff(go, wo), wo.size)
    return wo, wc


# L: 1, 2, 3 and 63 (below a wave), 64 / 128 / 192 / 256 (the streaming instances), 65 and 300 (padded label strides);
# sizes: nx < L, nx = L - 1, L + 1, one past a segment of 64 / 128 / 256 right pixels, one row and several;
# vnx = nx, nx + 5, nx - 3; ranges all negative / all positive / across 0; NDIR 1, 4, 8; over-count fix on and off;
# refinement none and vfit; MGM 1 and 3; Hirschmueller and FH potentials.  A grid, not the product.
GRID = [
    # L, nx, ny, vnx - nx, range, NDIR, fix, refine, MGM, FH
    (1, 37, 1, 0, "neg", 4, 1, None, 1, 0),
    (1, 37, 5, 5, "pos", 8, 0, "vfit", 3, 0),
    (2, 37, 5, -3, "mid", 1, 1, "vfit", 3, 1),
    (3, 37, 1, 5, "neg", 8, 1, "vfit", 1, 0),
    (3, 130, 3, 0, "pos", 4, 0, None, 3, 1),
    (63, 37, 5, 0, "mid", 8, 1, "vfit", 3, 0),
    (63, 130, 3, -3, "neg", 4, 0, None, 1, 1),
    (64, 37, 1, 5, "pos", 1, 1, "vfit", 3, 0),
    (64, 130, 3, 0, "mid", 8, 1, "vfit", 3, 1),
    (64, 257, 2, -3, "neg", 4, 1, None, 3, 0),
    (65, 130, 3, 5, "mid", 8, 0, "vfit", 1, 0),
    (65, 37, 5, 0, "pos", 4, 1, None, 3, 1),
    (128, 130, 3, -3, "pos", 8, 1, "vfit", 3, 0),
    (128, 257, 2, 0, "mid", 4, 0, "vfit", 3, 1),
    (192, 257, 2, 5, "neg", 8, 1, "vfit", 1, 0),
    (192, 37, 5, 0, "mid", 1, 0, None, 3, 0),
    (256, 257, 2, 0, "mid", 8, 1, "vfit", 3, 1),
    (256, 255, 2, 5, "neg", 4, 1, None, 3, 0),
    (256, 130, 3, -3, "pos", 8, 0, "vfit", 1, 0),
    (256, 37, 1, 0, "mid", 4, 1, "vfit", 3, 0),
    (300, 257, 2, -3, "mid", 8, 1, "vfit", 3, 0),
    (300, 37, 5, 5, "neg", 4, 0, None, 1, 1),
]


@pytest.mark.parametrize("case", GRID, ids=lambda c: "L%d-%dx%d%+d-%s-O%d-fix%d-%s-T%d-fh%d" % c)
def test_matches_the_model(ctx, case):
    L, nx, ny, dv, rng, NDIR, fix, refine, T, FH = case
    C = synth.raw_volume(nx, ny, L, seed=1000 + L + nx, inf_frac=0.03)
    check(ctx, C, first_label(rng, L), nx + dv, NDIR, fix, refine, T, FH)


@pytest.mark.parametrize("case", [GRID[2], GRID[5], GRID[8], GRID[16], GRID[20]], ids=lambda c: "L%d-%dx%d" % c[:3])
def test_the_generic_kernel_matches_the_model(ctx, case, monkeypatch):
    """MGM_HIP_WTA_RIGHT_ANY=1: every label count on the kernel that walks the diagonals in memory."""
    monkeypatch.setenv("MGM_HIP_WTA_RIGHT_ANY", "1")
    L, nx, ny, dv, rng, NDIR, fix, refine, T, FH = case
    C = synth.raw_volume(nx, ny, L, seed=2000 + L + nx, inf_frac=0.03)
    check(ctx, C, first_label(rng, L), nx + dv, NDIR, fix, refine, T, FH)


@pytest.mark.parametrize("L,nx,ny", [(64, 130, 3), (3, 37, 5), (256, 257, 2)])
def test_ties_along_whole_diagonals(ctx, L, nx, ny):
    """small integer costs and no penalties: S = NDIR * C - (NDIR - 1) * C in few values; among equal minima the smallest
    right label (the largest left disparity) wins"""
    rng = np.random.default_rng(L)
    C = rng.integers(0, 2, (ny, nx, L)).astype(np.float32)
    C[0] = 1.0  # a row of one value: every entry of every diagonal ties
    dmin = first_label("mid", L)
    wo, _ = check(ctx, C, dmin, nx + 2, 8, 1, None, 3, 0, P1=0.0, P2=0.0)
    dmax = dmin + L - 1
    xr = np.arange(nx + 2)
    e_first = np.maximum(-dmax, -xr)  # the smallest e with 0 <= xr + e
    reach = (xr + e_first < nx) & (e_first <= -dmin)
    assert np.array_equal(wo[0][reach], e_first[reach].astype(np.float32)) and np.isnan(wo[0][~reach]).all()


def test_right_columns_without_a_finite_entry(ctx):
    """+INF costs along whole diagonals x + d = xr: those columns of the right view have no finite entry (NaN, +INF), as have the
    columns no left pixel reaches; every left pixel keeps finite costs at its other labels."""
    nx, ny, L, dmin = 130, 3, 64, -40
    C = synth.raw_volume(nx, ny, L, seed=5)
    x = np.arange(nx)[:, None]
    d = dmin + np.arange(L)[None, :]
    dead = [20, 21, 22, 23, 24, 77, 129]
    C[:, np.isin(x + d, dead)] = np.inf
    for fix in (1, 0):
        wo, wc = check(ctx, C, dmin, nx + 5, 8, fix, "vfit", 3, 0)
        assert np.isnan(wo[:, dead]).all() and np.isinf(wc[:, dead]).all() and np.isfinite(wc).sum() > wc.size // 2


def test_slot_one_of_a_batch(ctx):
    nx, ny, L, dmin, NDIR = 130, 3, 128, -100, 8
    Cs = [synth.raw_volume(nx, ny, L, seed=s, inf_frac=0.02) for s in (31, 32)]
    cvs = [ctx.upload_volume(C, dmin) for C in Cs]
    S, outs, costs = ctx.aggregate_batch_dev(cvs, 8.0, 32.0, NDIR, 3, 0, 1, None, "vfit", want_S=True)
    for k in (1, 0):
        o, c = ctx.wta_right_dev(cvs[k], NDIR, 1, "vfit", nx - 3)
        wo, wc = wta_right(S[k].download(), dmin, nx - 3, "vfit")
        assert same(c.download()[0], wc) and same(o.download()[0], wo)
        o.free(), c.free()
    for h in cvs + S + outs + costs:
        h.free()


@pytest.mark.parametrize("L,nx", [(64, 130), (256, 257)])
def test_compact_census_volume(ctx, L, nx):
    """a volume built on the device from single-word census descriptors: one byte per cost, read under the over-count fix"""
    ny, dmin = 6, -(L - 8)
    u, v, _ = synth.stereo_pair(nx, ny, -12, 0, seed=9)
    du, dv = ctx.upload_image(u), ctx.upload_image(v[:, :, : nx - 3])
    cv = ctx.costvolume_dev(du, dv, dmin, dmin + L - 1, "none", "census", census_win=5)
    S, o0, c0 = ctx.aggregate_dev(cv, 8.0, 32.0, 8, 3, 0, 1, None, "vfit", want_S=True)
    o, c = ctx.wta_right_dev(cv, 8, 1, "vfit", nx - 3)
    wo, wc = wta_right(S.download(), dmin, nx - 3, "vfit")
    assert same(c.download()[0], wc) and same(o.download()[0], wo)
    for h in (du, dv, cv, S, o0, c0, o, c):
        h.free()


def test_refusals_leave_the_context_usable(ctx):
    nx, ny, L, dmin, NDIR = 37, 5, 64, -30, 4
    C = synth.raw_volume(nx, ny, L, seed=41, inf_frac=0.02)
    a = ctx.upload_volume(C, dmin)
    b = ctx.upload_volume(synth.raw_volume(nx, ny, L, seed=42), dmin)
    S, _, _ = ctx.aggregate(a, 8.0, 32.0, NDIR, 3, 0, 1, None, "vfit", want_S=True)
    wo, wc = wta_right(S.download(), dmin, nx, "vfit")

    def good():
        o, c = ctx.wta_right_dev(a, NDIR, 1, "vfit", nx)
        ok = same(c.download()[0], wc) and same(o.download()[0], wo)
        o.free(), c.free()
        return ok

    def refused(code, *args, **kw):
        with pytest.raises(mgm_amd.MgmError) as e:
            ctx.wta_right_dev(*args, **kw)
        return e.value.code == code

    assert good()
    # a ragged volume (built from range images)
    u, v, _ = synth.stereo_pair(nx, ny, -8, 0, seed=3)
    lo = np.full((ny, nx), -8, np.float32)
    hi = np.zeros((ny, nx), np.float32)
    lo[:, ::2] = -5
    ragged = ctx.costvolume(u, v, lo, hi, "none", "ad")
    assert refused(mgm_amd.MGM_ERR_UNSUPPORTED, ragged, NDIR, 1, None, nx) and good()
    # a volume that was not part of the last aggregation; the right volume with another NDIR
    assert refused(mgm_amd.MGM_ERR_INVALID, b, NDIR, 1, None, nx) and good()
    assert refused(mgm_amd.MGM_ERR_INVALID, a, 8, 1, None, nx) and good()
    # images of another height
    wrong = ctx.new_image(nx, ny + 1)
    assert refused(mgm_amd.MGM_ERR_INVALID, a, NDIR, 1, None, nx, out=wrong, outcost=ctx.new_image(nx, ny + 1)) and good()
    # a refinement the mode does not have
    for name in ("cubic", "parabola", "parabolaOCV"):
        assert refused(mgm_amd.MGM_ERR_UNSUPPORTED, a, NDIR, 1, name, nx)
    assert good()
    for h in (a, b, S, ragged, wrong):
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
            o, c = c2.wta_right_dev(cv, NDIR, 1, "vfit", nx + 5)
            res.append((o.download()[0], c.download()[0]))
    assert same(res[1][0], res[0][0]) and same(res[1][1], res[0][1]) and np.isfinite(res[0][1]).any()


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def read_tif(path):
    npy = path + ".npy"
    subprocess.run([CONV, path, npy], check=True, timeout=60)
    return np.load(npy).astype(np.float32).squeeze()


def test_command_line(ctx, tmp_path):
    """the 96 x 40 synthetic pair (tests/test_wta_right_model.py checks on the oracle that it clears the sanity bound with room)"""
    nx, ny, dmin, dmax = 96, 40, -16, 0
    u, v, _ = synth.stereo_pair(nx, ny, dmin, dmax)
    fu, fv = str(tmp_path / "u.npy"), str(tmp_path / "v.npy")
    np.save(fu, u[0]), np.save(fv, v[0])
    args = "-r -16 -R 0 -t census -s vfit -O 8".split() + [fu, fv]
    one, two = str(tmp_path / "one.tif"), str(tmp_path / "two.tif")
    r1 = run_cli(args + [one], dict(MGM_RIGHT_FROM_LEFT="1"))
    assert r1.returncode == 0, r1.stderr
    assert r1.stdout.splitlines() == ["-16 0", "01234567", "right from left"]
    r2 = run_cli(args + [two], {})
    assert r2.returncode == 0 and r2.stdout.splitlines() == ["-16 0", "01234567", "01234567"]
    got, ref = read_tif(one), read_tif(two)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    L_, R_, c_ = ctx.pair_right_from_left(du, dv, dmin, dmax, 8.0, 32.0, 8, 4, refine="vfit", distance="census", tau=1.0)
    assert same(got, L_.download()[0])
    assert R_.shape == (1, ny, nx)
    with np.errstate(invalid="ignore"):
        agree = np.mean((np.isnan(got) & np.isnan(ref)) | (np.abs(got - ref) <= 1))
    print("checked left maps of the one-run and the two-run command agree within 1 px on %.3f of the pixels" % agree)
    assert agree >= 0.8
    r3 = run_cli(args + [one], dict(MGM_RIGHT_FROM_LEFT="1", TSGM_ITER="2"))
    assert r3.returncode == 2 and "does not combine with TSGM_ITER" in r3.stderr
    for h in (du, dv, L_, R_, c_):
        h.free()
