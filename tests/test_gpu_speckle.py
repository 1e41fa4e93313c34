"""The speckle filter on the device (mgm_speckle_dev) against the numpy model of tests/speckle_model.py, bit for bit
on `out` and on `size_map`: crafted maps on shapes placed around the kernels' tile (read from plan_speckle, not written here),
every call form, scratch reuse, the refusals, and the command line's MGM_SPECKLE against the same steps through the Python API."""
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
from helpers import ndiff
from mgm_amd import synth
from speckle_model import CLI_MAXDIFF, CLI_MAXSIZE, PAIR, crafted, maxsizes, plan, plan_lib, sizes, speckle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
CONV = os.path.join(ROOT, "mgm_amd", "bin", "imgconv")


def _tile():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c = plan(plan_lib(tmp), [(1920, 1080, 256)])[0]
    return c["tw"], c["th"]


TW, TH = _tile()  # the planner's tile: the shapes below sit around its seams
SMALL = [(1, 1), (1, 9), (7, 1), (3, 4)]
AROUND = [(nx, ny) for nx in (TW - 1, TW, TW + 1, 2 * TW + 1) for ny in (TH - 1, TH, TH + 1, 2 * TH + 1)]
RAGGED = (2 * TW + 7, 2 * TH + 5)  # 3 x 3 tiles, the last of each axis ragged
SHAPES = SMALL + AROUND + [RAGGED]
assert all(nx <= 200 and ny <= 200 for nx, ny in SHAPES)


def same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


@pytest.fixture
def tctx(ctx):
    """the session's context with its timing table on and empty: every test asserts from it that k_speckle ran"""
    ctx.timing(True)
    ctx.timing_reset()
    yield ctx
    ctx.timing_reset()
    ctx.timing(False)


def ran(ctx, calls):
    """k_speckle is listed once per call, each of its four kernels inside it; clears the table"""
    names = [n for n, _ in ctx.timings()]
    ctx.timing_reset()
    return names.count("k_speckle") == calls and all(names.count("k_speckle_" + k) == calls for k in ("local", "seams", "count", "apply"))


@pytest.mark.parametrize("nx,ny", SHAPES, ids=lambda v: str(v))
def test_matches_the_model(tctx, nx, ny):
    ctx = tctx
    out = ctx.new_image(nx, ny)
    calls = 0
    for name, d, maxdiff in crafted(nx, ny, TW, TH):
        size = sizes(d, maxdiff)
        dd = ctx.upload_image(d)
        ms = maxsizes(size, nx * ny)
        for k, maxsize in enumerate(ms):
            want_out, want_size = speckle(d, maxsize, maxdiff, size=size)
            _, sm = ctx.speckle_dev(dd, maxsize, maxdiff, out=out, want_size=(k == 0))
            calls += 1
            assert same(out.download()[0], want_out), (name, maxsize)
            if sm is not None:
                assert same(sm.download()[0], want_size), (name, maxsize)
                sm.free()
        s = int(size.max())
        if s >= 1:  # at exactly the component's size it goes, one below it stays
            big = size == s
            assert np.isnan(speckle(d, s, maxdiff, size=size)[0][big]).all() and not np.isnan(speckle(d, s - 1, maxdiff, size=size)[0][big]).any()
        dd.free()
    out.free()
    assert ran(ctx, calls)


def test_call_forms(tctx):
    ctx = tctx
    nx, ny = RAGGED
    name, d, maxdiff = crafted(nx, ny, TW, TH)[-1]
    assert name == "random_levels"
    size = sizes(d, maxdiff)
    maxsize = 6
    want_out, want_size = speckle(d, maxsize, maxdiff, size=size)
    assert 0 < np.isnan(want_out[np.isfinite(d)]).mean() < 1
    dd = ctx.upload_image(d)
    o, s = ctx.speckle_dev(dd, maxsize, maxdiff, want_size=True)             # both, new images
    assert same(o.download()[0], want_out) and same(s.download()[0], want_size) and same(dd.download()[0], d)
    o2, s2 = ctx.speckle_dev(dd, maxsize, maxdiff, want_size=True)           # the same call again: the same bits
    assert o2.download().tobytes() == o.download().tobytes() and s2.download().tobytes() == s.download().tobytes()
    o3, none = ctx.speckle_dev(dd, maxsize, maxdiff)                         # only out
    assert none is None and same(o3.download()[0], want_out)
    none, s3 = ctx.speckle_dev(dd, maxsize, maxdiff, out=False, want_size=True)  # only size_map
    assert none is None and same(s3.download()[0], want_size) and same(dd.download()[0], d)
    o4, s4 = ctx.speckle_dev(dd, maxsize, maxdiff, out=dd, want_size=True)   # in place
    assert o4 is dd and same(dd.download()[0], want_out) and same(s4.download()[0], want_size)
    o5, _ = ctx.speckle_dev(dd, maxsize, maxdiff, out=dd)                    # idempotent
    assert same(dd.download()[0], want_out)
    assert ran(ctx, 6)
    for h in (dd, o, s, o2, s2, o3, s3, s4):
        h.free()


def test_a_small_map_right_after_a_larger_one(tctx):
    """the scratch planes keep the larger call's parents and counts: nothing of them may leak into the smaller one"""
    ctx = tctx
    calls = 0
    for big, small in ((RAGGED, (3, 4)), (RAGGED, (TW + 1, TH + 1)), ((2 * TW + 1, 2 * TH + 1), (TW - 1, TH - 1))):
        for pattern in ("one_component", "serpentine_rows", "random_levels"):
            for nx, ny in (big, small):
                name, d, maxdiff = [c for c in crafted(nx, ny, TW, TH) if c[0] == pattern][0]
                want_out, want_size = speckle(d, 5, maxdiff)
                dd = ctx.upload_image(d)
                o, s = ctx.speckle_dev(dd, 5, maxdiff, want_size=True)
                calls += 1
                assert same(o.download()[0], want_out) and same(s.download()[0], want_size), (pattern, nx, ny)
                for h in (dd, o, s):
                    h.free()
    # ... and after the workspace has been handed back
    ctx.trim()
    d = crafted(7, 1, TW, TH)[0][1]
    dd = ctx.upload_image(d)
    o, s = ctx.speckle_dev(dd, 7, 1.0, want_size=True)
    assert np.isnan(o.download()).all() and (s.download() == 7).all()
    assert ran(ctx, calls + 1)
    for h in (dd, o, s):
        h.free()


def test_refusals_leave_the_context_usable(tctx):
    ctx = tctx
    nx, ny = TW + 1, TH + 1
    _, d, maxdiff = crafted(nx, ny, TW, TH)[-1]
    want_out, want_size = speckle(d, 4, maxdiff)
    dd = ctx.upload_image(d)
    calls = [0]

    def good():
        o, s = ctx.speckle_dev(dd, 4, maxdiff, want_size=True)
        calls[0] += 1
        ok = same(o.download()[0], want_out) and same(s.download()[0], want_size)
        o.free(), s.free()
        return ok

    def refused(fn, *args, **kw):
        with pytest.raises(mgm_amd.MgmError) as e:
            fn(*args, **kw)
        return e.value.code == mgm_amd.MGM_ERR_INVALID

    assert good()
    assert refused(ctx.speckle_dev, dd, -1, 1.0) and good()
    for maxdiff_bad in (-0.5, float("nan"), float("-inf")):
        assert refused(ctx.speckle_dev, dd, 4, maxdiff_bad) and good()
    assert refused(ctx.speckle_dev, dd, 4, 1.0, out=False, want_size=False) and good()   # neither output
    w1, w2 = ctx.new_image(nx, ny + 1), ctx.new_image(nx, ny, 2)
    assert refused(ctx.speckle_dev, dd, 4, 1.0, out=w1) and refused(ctx.speckle_dev, dd, 4, 1.0, out=w2) and good()
    assert refused(ctx.speckle_dev, w2, 4, 1.0) and good()                               # a map of two channels
    ok = ctx.new_image(nx, ny)
    for size_map in (dd, ok):  # size_map must be an image of its own: not d, not out
        assert ctx.lib.mgm_speckle_dev(ctx.h, dd.h, 4, 1.0, ok.h, size_map.h) == mgm_amd.MGM_ERR_INVALID and good()
    assert same(dd.download()[0], d)
    assert ran(ctx, calls[0])
    for h in (dd, w1, w2, ok):
        h.free()


def test_pipelined_context_runs_the_deferred_aggregation_first():
    nx, ny, L, dmin, NDIR = 130, 3, 64, -20, 8
    Cv = synth.raw_volume(nx, ny, L, seed=51, inf_frac=0.02)
    res = []
    for depth in (1, 2):
        with mgm_amd.Context(0) as c2:
            c2.timing(True)
            if depth > 1:
                c2.set_pipeline(depth)
            cv = c2.upload_volume(Cv, dmin)
            _, o, _ = c2.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, "vfit")
            f, s = c2.speckle_dev(o, 3, 1.0, want_size=True)
            res.append((f.download()[0], s.download()[0], o.download()[0]))
            assert "k_speckle" in [n for n, _ in c2.timings()]
    assert all(same(x, y) for x, y in zip(res[1], res[0]))
    want = speckle(res[0][2], 3, 1.0)
    assert same(res[0][0], want[0]) and same(res[0][1], want[1]) and np.isnan(want[0]).any()


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def read_tif(path):
    npy = path + ".npy"
    subprocess.run([CONV, path, npy], check=True, timeout=60)
    return np.load(npy).astype(np.float32).squeeze()


def test_command_line(tctx, tmp_path):
    """the 96 x 64 synthetic pair at the maxsize tests/test_speckle_model.py chose on the oracle's final map"""
    ctx = tctx
    p = PAIR
    nx, ny, dmin, dmax, NDIR = p["nx"], p["ny"], p["dmin"], p["dmax"], p["NDIR"]
    u, v, _ = synth.stereo_pair(nx, ny, dmin, dmax)
    fu, fv = str(tmp_path / "u.npy"), str(tmp_path / "v.npy")
    np.save(fu, u[0]), np.save(fv, v[0])
    args = "-r -16 -R 0 -t census -s vfit -O 8".split()
    f = {k: str(tmp_path / (k + ".tif")) for k in ("plain", "pcost", "pback", "pnolr", "out", "cost", "back", "nolr", "s2", "s2f", "rfl", "rflf")}
    env = dict(MGM_SPECKLE=str(CLI_MAXSIZE), MGM_SPECKLE_DIFF=repr(CLI_MAXDIFF), MGM_HIP_KERNELS="1")
    r0 = run_cli(args + ["-l", f["pnolr"], fu, fv, f["plain"], f["pcost"], f["pback"]], {})
    r1 = run_cli(args + ["-l", f["nolr"], fu, fv, f["out"], f["cost"], f["back"]], env)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert r1.stdout == r0.stdout and r0.stdout.splitlines() == ["-16 0", "01234567", "01234567"]   # stdout is unchanged
    kernels = [l for l in r1.stderr.splitlines() if l.startswith("[mgm kernels]")][0].split()
    assert kernels.count("k_speckle") == 1 and kernels.index("k_speckle") > max(i for i, k in enumerate(kernels) if k == "k_leftright")
    assert kernels.index("k_speckle") < kernels.index("k_backproject")

    # the model on the unfiltered command's output
    plain = read_tif(f["plain"])
    want, _ = speckle(plain, CLI_MAXSIZE, CLI_MAXDIFF)
    got = read_tif(f["out"])
    assert same(got, want)
    valid = np.isfinite(plain)
    share = (valid & np.isnan(got)).sum() / valid.sum()
    print("MGM_SPECKLE=%d removed %d of %d valid pixels, share %.4f" % (CLI_MAXSIZE, (valid & np.isnan(got)).sum(), valid.sum(), share))
    assert (valid & np.isnan(got)).sum() >= 1 and share <= 0.5
    # the -l map and the cost map are the plain command's; the back-projected image is made from the filtered map
    assert same(read_tif(f["nolr"]), read_tif(f["pnolr"])) and same(read_tif(f["cost"]), read_tif(f["pcost"]))
    assert not same(read_tif(f["back"]), read_tif(f["pback"]))

    # the same steps through the Python API
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    cvL = ctx.costvolume_dev(du, dv, dmin, dmax, "none", "census")
    cvR = ctx.costvolume_dev(dv, du, -dmax, -dmin, "none", "census")
    _, outs, costs = ctx.aggregate_batch_dev([cvL, cvR], p["P1"], p["P2"], NDIR, p["TSGM"], 0, 1, None, "vfit")
    final = ctx.leftright_dev(outs[0], outs[1], 1.0)
    assert same(final.download()[0], plain)
    ctx.timing_reset()
    ctx.speckle_dev(final, CLI_MAXSIZE, CLI_MAXDIFF, out=final)
    assert ran(ctx, 1)
    assert same(final.download()[0], got)
    assert same(ctx.backproject_dev(du, dv, final).download()[0], read_tif(f["back"]))

    # ... with -S 2 (once, on the full-size level's final map) and with the right map read out of the left run
    r2 = run_cli(args + ["-S", "2", fu, fv, f["s2"]], {})
    r3 = run_cli(args + ["-S", "2", fu, fv, f["s2f"]], env)
    assert r2.returncode == 0 and r3.returncode == 0 and r3.stdout == r2.stdout, r2.stderr + r3.stderr
    assert r3.stderr.split().count("k_speckle") == 1
    ms = ctx.multiscale_pair(du, dv, dmin, dmax, 2, P1=p["P1"], P2=p["P2"], NDIR=NDIR, TSGM=p["TSGM"], distance="census", refine="vfit")
    assert same(ms["outL"].download()[0], read_tif(f["s2"]))
    ctx.speckle_dev(ms["outL"], CLI_MAXSIZE, CLI_MAXDIFF, out=ms["outL"])
    want2 = speckle(read_tif(f["s2"]), CLI_MAXSIZE, CLI_MAXDIFF)[0]
    assert same(read_tif(f["s2f"]), want2) and same(ms["outL"].download()[0], want2) and not same(want2, read_tif(f["s2"]))

    r4 = run_cli(args + [fu, fv, f["rfl"]], {"MGM_RIGHT_FROM_LEFT": "1"})
    r5 = run_cli(args + [fu, fv, f["rflf"]], dict(env, MGM_RIGHT_FROM_LEFT="1"))
    assert r4.returncode == 0 and r5.returncode == 0 and r5.stdout == r4.stdout, r4.stderr + r5.stderr
    assert r5.stdout.splitlines() == ["-16 0", "01234567", "right from left"] and r5.stderr.split().count("k_speckle") == 1
    chkL, _, _ = ctx.pair_right_from_left(du, dv, dmin, dmax, P1=p["P1"], P2=p["P2"], NDIR=NDIR, TSGM=p["TSGM"], distance="census", refine="vfit")
    assert same(chkL.download()[0], read_tif(f["rfl"]))
    ctx.speckle_dev(chkL, CLI_MAXSIZE, CLI_MAXDIFF, out=chkL)
    want3 = speckle(read_tif(f["rfl"]), CLI_MAXSIZE, CLI_MAXDIFF)[0]
    assert same(read_tif(f["rflf"]), want3) and same(chkL.download()[0], want3) and not same(want3, read_tif(f["rfl"]))
