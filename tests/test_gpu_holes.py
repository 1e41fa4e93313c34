"""Hole filling on the device (mgm_fill_holes_dev) against the numpy model of tests/holes_model.py, bit for bit on
`out` and on `filled`, NaN positions and payloads included: crafted maps on shapes placed around the kernels' row chunk and band
(read from plan_holes, not written here), every mode, direction set and distance bound, every call form, scratch reuse, the
refusals, and the command line's MGM_FILL_HOLES against the model applied to the unfilled command's output."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import mgm_amd
from holes_model import CLI_ARGS, CLI_RUNS, CLI_SPECKLE, MODES, PAIR, crafted, fill, plan, plan_lib, rays, same_bits
from mgm_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
CONV = os.path.join(ROOT, "mgm_amd", "bin", "imgconv")


def _plan():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        lib = plan_lib(tmp)
        c = plan(lib, [(1920, 1080, 8, 256)])[0]
        chunk, band = c["chunk"], c["band"]
        # the band of every shape used below is the one read here (the plan may choose it by the shape)
        around = [(nx, ny) for nx in (chunk - 1, chunk, chunk + 1, 2 * chunk + 1) for ny in (band - 1, band, band + 1, 2 * band + 1)]
        ragged = (2 * chunk + 7, 2 * band + 5)
        for c2 in plan(lib, [(nx, ny, 8, 256) for nx, ny in around + [ragged]]):
            assert (c2["chunk"], c2["band"]) == (chunk, band)
    return chunk, band, around, ragged


CHUNK, BAND, AROUND, RAGGED = _plan()  # the planner's chunk and band: the shapes sit around their seams
SMALL = [(1, 1), (1, 9), (7, 1), (3, 4)]
SHAPES = SMALL + AROUND + [RAGGED]      # RAGGED: 3 x 3 chunks / bands, the last of each axis ragged
assert all(nx <= 200 and ny <= 200 for nx, ny in SHAPES)
DIRS = (2, 4, 8)
DISTS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1)


@pytest.fixture
def tctx(ctx):
    """the session's context with its timing table on and empty: every test asserts from it that k_holes ran"""
    ctx.timing(True)
    ctx.timing_reset()
    yield ctx
    ctx.timing_reset()
    ctx.timing(False)


def ran(ctx, calls, calls2=0):
    """k_holes is listed once per call with its kernels inside it (`calls2` of the calls had dirs = 2: no column or diagonal
    kernels); clears the table"""
    names = [n for n, _ in ctx.timings()]
    ctx.timing_reset()
    want = {"k_holes": calls, "k_holes_rows": calls, "k_holes_apply": calls, "k_holes_carry": calls - calls2, "k_holes_walk": calls - calls2}
    return all(names.count(k) == v for k, v in want.items()) and all(n in want for n in names if n.startswith("k_holes"))


@pytest.mark.parametrize("nx,ny", SHAPES, ids=lambda v: str(v))
def test_matches_the_model(tctx, nx, ny):
    ctx = tctx
    out, filled = ctx.new_image(nx, ny), ctx.new_image(nx, ny)
    names = []
    for name, d in crafted(nx, ny, CHUNK, BAND):
        names.append(name)
        r = rays(d)
        dd = ctx.upload_image(d)
        calls = calls2 = 0
        for mode in MODES:
            for dirs in DIRS:
                for maxdist in DISTS:
                    want_out, want_filled = fill(d, mode, dirs, maxdist, r=r)
                    ctx._chk(ctx.lib.mgm_fill_holes_dev(ctx.h, dd.h, mode.encode(), dirs, maxdist, out.h, filled.h))
                    calls, calls2 = calls + 1, calls2 + (dirs == 2)
                    got_out, got_filled = out.download()[0], filled.download()[0]
                    assert same_bits(got_out, want_out), (name, mode, dirs, maxdist)
                    assert same_bits(got_filled, want_filled), (name, mode, dirs, maxdist)
        assert same_bits(dd.download()[0], d), name
        assert ran(ctx, calls, calls2), name
        dd.free()
    assert {"all_valid", "all_nan", "one_centre", "one_top_left", "one_bottom_right", "hole_rows", "hole_columns", "hole_diagonals", "seam_hole",
            "checkerboard", "random_10", "random_90", "zeros_of_both_signs", "payloads_and_infinities", "unreachable_payloads"} <= set(names)
    out.free(), filled.free()


def test_the_crafted_maps_reach_what_they_are_there_for():
    """On the ragged 3 x 3 shape: the seam hole really spans a chunk seam and a band seam, distances reach past a chunk, ties and
    zeros of both signs decide output bits, untouched payloads exist."""
    nx, ny = RAGGED
    c = dict(crafted(nx, ny, CHUNK, BAND))
    seam = ~np.isfinite(c["seam_hole"])
    ys, xs = np.nonzero(seam)
    assert xs.min() < CHUNK <= xs.max() and ys.min() < BAND <= ys.max()
    assert rays(c["one_top_left"])[1].max() > CHUNK + 1
    z = c["zeros_of_both_signs"]
    assert (np.signbit(fill(z, "min")[0]) != np.signbit(fill(z, "max")[0])).any()
    p = c["payloads_and_infinities"]
    o, f = fill(p, "median", 8, 1)
    stay = ~np.isfinite(p) & (f == 0)
    assert stay.any() and np.isinf(p[stay]).any() and (np.isnan(p[stay]) & ((p[stay].view(np.uint32) & 0x3FFFFF) != 0)).any()
    assert fill(c["unreachable_payloads"], "median")[1].sum() == 0
    for name in ("random_10", "random_90"):
        assert 0 < fill(c[name], "median", 2, 1)[1].sum() < (~np.isfinite(c[name])).sum()


def test_call_forms(tctx):
    ctx = tctx
    nx, ny = RAGGED
    d = dict(crafted(nx, ny, CHUNK, BAND))["random_90"]
    mode, dirs, maxdist = "median", 8, 2
    want_out, want_filled = fill(d, mode, dirs, maxdist)
    hole = ~np.isfinite(d)
    assert 0 < want_filled[hole].mean() < 1
    dd = ctx.upload_image(d)
    o, f = ctx.fill_holes_dev(dd, mode, dirs, maxdist, want_filled=True)              # both, new images
    assert same_bits(o.download()[0], want_out) and same_bits(f.download()[0], want_filled) and same_bits(dd.download()[0], d)
    o2, f2 = ctx.fill_holes_dev(dd, mode, dirs, maxdist, want_filled=True)            # the same call again: the same bytes
    assert o2.download().tobytes() == o.download().tobytes() and f2.download().tobytes() == f.download().tobytes()
    o3, none = ctx.fill_holes_dev(dd, mode, dirs, maxdist)                            # only out
    assert none is None and same_bits(o3.download()[0], want_out)
    none, f3 = ctx.fill_holes_dev(dd, mode, dirs, maxdist, out=False, want_filled=True)  # only filled, d untouched
    assert none is None and same_bits(f3.download()[0], want_filled) and same_bits(dd.download()[0], d)
    o4, f4 = ctx.fill_holes_dev(dd, mode, dirs, maxdist, out=dd, want_filled=True)    # in place
    assert o4 is dd and same_bits(dd.download()[0], want_out) and same_bits(f4.download()[0], want_filled)
    o5, f5 = ctx.fill_holes_dev(dd, mode, dirs, maxdist, out=dd, want_filled=True)    # NOT idempotent: the second application fills more
    again = fill(want_out, mode, dirs, maxdist)
    assert same_bits(dd.download()[0], again[0]) and same_bits(f5.download()[0], again[1]) and again[1].sum() > 0
    dflt = ctx.upload_image(d)
    o6, _ = ctx.fill_holes_dev(dflt)                                                  # the defaults: median, 8, 0
    assert same_bits(o6.download()[0], fill(d)[0])
    assert ran(ctx, 7)
    for h in (dd, dflt, o, f, o2, f2, o3, f3, f4, f5, o6):
        h.free()


def test_scratch_reuse(tctx):
    """the scratch keeps the earlier call's candidates and carries: nothing of them may leak into the next one"""
    ctx = tctx
    calls = calls2 = 0

    def check(nx, ny, pattern, mode, dirs, maxdist):
        nonlocal calls, calls2
        d = dict(crafted(nx, ny, CHUNK, BAND))[pattern]
        want = fill(d, mode, dirs, maxdist)
        dd = ctx.upload_image(d)
        o, f = ctx.fill_holes_dev(dd, mode, dirs, maxdist, want_filled=True)
        calls, calls2 = calls + 1, calls2 + (dirs == 2)
        ok = same_bits(o.download()[0], want[0]) and same_bits(f.download()[0], want[1])
        for h in (dd, o, f):
            h.free()
        return ok

    for big, small in ((RAGGED, (3, 4)), (RAGGED, (CHUNK + 1, BAND + 1)), ((2 * CHUNK + 1, 2 * BAND + 1), (CHUNK - 1, BAND - 1))):
        for pattern in ("random_10", "random_90", "all_nan"):
            assert check(*big, "random_10", "median", 8, 0)          # a small map right after a larger one
            assert check(*small, pattern, "median", 8, 0), (small, pattern)
    for pattern in ("random_90", "one_centre"):                       # dirs = 2 right after dirs = 8 on the same shape
        assert check(*RAGGED, "random_10", "max", 8, 0)
        assert check(*RAGGED, pattern, "max", 2, 0) and check(*RAGGED, pattern, "max", 4, 0)
    ctx.trim()                                                        # ... and after the workspace has been handed back
    assert check(7, 1, "one_centre", "min", 8, 0) and check(*RAGGED, "random_90", "median", 8, 0)
    assert ran(ctx, calls, calls2)


def test_refusals_leave_the_context_usable(tctx):
    ctx = tctx
    nx, ny = CHUNK + 1, BAND + 1
    d = dict(crafted(nx, ny, CHUNK, BAND))["random_90"]
    want_out, want_filled = fill(d, "median", 8, 0)
    dd = ctx.upload_image(d)
    calls = [0]

    def good():
        o, f = ctx.fill_holes_dev(dd, "median", 8, 0, want_filled=True)
        calls[0] += 1
        ok = same_bits(o.download()[0], want_out) and same_bits(f.download()[0], want_filled)
        o.free(), f.free()
        return ok

    def refused(fn, *args, **kw):
        with pytest.raises(mgm_amd.MgmError) as e:
            fn(*args, **kw)
        return e.value.code == mgm_amd.MGM_ERR_INVALID

    assert good()
    for mode in (None, "", "mean", "Median", "median ", "none"):
        assert refused(ctx.fill_holes_dev, dd, mode, 8, 0) and good(), mode
    for dirs in (-1, 0, 1, 3, 6, 16):
        assert refused(ctx.fill_holes_dev, dd, "median", dirs, 0) and good(), dirs
    assert refused(ctx.fill_holes_dev, dd, "median", 8, -1) and good()
    assert refused(ctx.fill_holes_dev, dd, "median", 8, 0, out=False, want_filled=False) and good()   # neither output
    w1, w2 = ctx.new_image(nx, ny + 1), ctx.new_image(nx, ny, 2)
    assert refused(ctx.fill_holes_dev, dd, "median", 8, 0, out=w1) and refused(ctx.fill_holes_dev, dd, "median", 8, 0, out=w2) and good()
    assert refused(ctx.fill_holes_dev, w2, "median", 8, 0) and good()                                 # a map of two channels
    ok = ctx.new_image(nx, ny)
    for filled in (dd, ok):  # filled must be an image of its own: not d, not out
        assert ctx.lib.mgm_fill_holes_dev(ctx.h, dd.h, b"median", 8, 0, ok.h, filled.h) == mgm_amd.MGM_ERR_INVALID and good()
    assert ctx.lib.mgm_fill_holes_dev(ctx.h, dd.h, b"median", 8, 0, None, w1.h) == mgm_amd.MGM_ERR_INVALID and good()  # filled of another size
    o, _ = ctx.fill_holes_dev(dd, "max", 8, 2 ** 31 - 1)                                             # the largest bound is a bound like any other
    assert same_bits(o.download()[0], fill(d, "max", 8, 0)[0])
    assert same_bits(dd.download()[0], d)
    assert ran(ctx, calls[0] + 1)
    for h in (dd, w1, w2, ok, o):
        h.free()


def test_pipelined_context_runs_the_deferred_aggregation_first():
    from speckle_model import speckle
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
            s, _ = c2.speckle_dev(o, 3, 1.0)
            f, m = c2.fill_holes_dev(s, "median", 8, 0, want_filled=True)
            res.append((f.download()[0], m.download()[0], o.download()[0]))
            assert "k_holes" in [n for n, _ in c2.timings()]
    assert all(same_bits(x, y) for x, y in zip(res[1], res[0]))
    holes = speckle(res[0][2], 3, 1.0)[0]
    want = fill(holes, "median", 8, 0)
    assert same_bits(res[0][0], want[0]) and same_bits(res[0][1], want[1]) and want[1].sum() > 0


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def read_tif(path):
    npy = path + ".npy"
    subprocess.run([CONV, path, npy], check=True, timeout=60)
    return np.load(npy).astype(np.float32).squeeze()


def write_png(path, a):
    """an 8-bit grey PNG of the integer image a [ny][nx]"""
    a = np.asarray(a)
    assert (a == np.rint(a)).all() and a.min() >= 0 and a.max() <= 255
    h, w = a.shape

    def chunk(t, d):
        return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))
    raw = b"".join(b"\0" + a[y].astype(np.uint8).tobytes() for y in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def test_command_line(tmp_path):
    """the 96 x 64 synthetic pair as PNGs, at the settings whose effect tests/test_holes_model.py checked on the oracle's map"""
    p = PAIR
    u, v, _ = synth.stereo_pair(p["nx"], p["ny"], p["dmin"], p["dmax"])
    fu, fv = str(tmp_path / "u.png"), str(tmp_path / "v.png")
    write_png(fu, u[0]), write_png(fv, v[0])
    args = CLI_ARGS.split()
    base = dict(MGM_SPECKLE=str(CLI_SPECKLE), MGM_HIP_KERNELS="1")

    def run(tag, extra_args, env):
        f = {k: str(tmp_path / ("%s_%s.tif" % (tag, k))) for k in ("out", "cost", "back", "nolr")}
        r = run_cli(args + extra_args + ["-l", f["nolr"], fu, fv, f["out"], f["cost"], f["back"]], dict(base, **env))
        assert r.returncode == 0, r.stderr
        return r, {k: read_tif(f[k]) for k in f}

    r0, m0 = run("disp0", [], {})
    assert r0.stdout.splitlines() == ["-16 0", "01234567", "01234567"]
    disp0 = m0["out"]
    hole = ~np.isfinite(disp0)
    r = rays(disp0)
    print("disp0: %d holes of %d (%.2f %%)" % (hole.sum(), hole.size, 100.0 * hole.mean()))
    assert 0.02 <= hole.mean() <= 0.40
    for mode, dirs, maxdist in CLI_RUNS:
        r1, m1 = run("%s_%d_%d" % (mode, dirs, maxdist), [], dict(MGM_FILL_HOLES=mode, MGM_FILL_HOLES_DIRS=str(dirs), MGM_FILL_HOLES_DIST=str(maxdist)))
        want, filled = fill(disp0, mode, dirs, maxdist, r=r)
        print("MGM_FILL_HOLES=%s _DIRS=%d _DIST=%d filled %d of %d holes" % (mode, dirs, maxdist, filled.sum(), hole.sum()))
        assert same_bits(m1["out"], want) and filled.sum() > 0 and not same_bits(want, disp0), (mode, dirs, maxdist)
        assert r1.stdout == r0.stdout                                                     # stdout, the -l map and the cost map are unchanged
        assert same_bits(m1["nolr"], m0["nolr"]) and same_bits(m1["cost"], m0["cost"])
        assert not same_bits(m1["back"], m0["back"])                                      # the back-projected image is made from the filled map
        kernels = [l for l in r1.stderr.splitlines() if l.startswith("[mgm kernels]")][0].split()
        assert kernels.count("k_holes") == 1 and kernels.index("k_speckle") < kernels.index("k_holes") < kernels.index("k_backproject")
        if (mode, dirs, maxdist) == ("median", 8, 0):
            assert np.isfinite(m1["out"]).all()
        if maxdist == 3:
            assert 0 < (hole & (filled == 0)).sum() < hole.sum()
    assert "k_holes" not in r0.stderr.split()
    # MGM_FILL_HOLES=none and an empty value are "off"
    for off in ("none", ""):
        r2, m2 = run("off" + off, [], dict(MGM_FILL_HOLES=off))
        assert same_bits(m2["out"], disp0) and "k_holes" not in r2.stderr.split()

    # ... with -S 2 (once, on the full-size level's final map) and with the uniqueness filter, each against its own unfilled output
    for tag, extra_args, env in (("s2", ["-S", "2"], {}), ("uniq", [], {"MGM_UNIQUENESS": "0.25"})):
        r3, m3 = run(tag + "0", extra_args, env)
        r4, m4 = run(tag + "f", extra_args, dict(env, MGM_FILL_HOLES="median"))
        want, filled = fill(m3["out"], "median", 8, 0)
        assert r4.stdout == r3.stdout and r4.stderr.split().count("k_holes") == 1
        assert same_bits(m4["out"], want) and filled.sum() > 0, tag
        assert same_bits(m4["nolr"], m3["nolr"]) and same_bits(m4["cost"], m3["cost"])

    # ... and in --batch mode per job: two command lines in one process, each against the model on its own unfilled output
    def batch(tag, env):
        outs = [str(tmp_path / ("batch_%s_%d.tif" % (tag, k))) for k in range(2)]
        lines = [" ".join(args + [fu, fv, outs[0]]), " ".join(args[:-1] + ["4", fu, fv, outs[1]])]   # (-O 8, -O 4)
        (tmp_path / ("batch_%s.txt" % tag)).write_text("\n".join(lines) + "\n")
        r = run_cli(["--batch", str(tmp_path / ("batch_%s.txt" % tag))], dict(base, **env))
        assert r.returncode == 0, r.stderr
        return r, [read_tif(o) for o in outs]

    assert args[-2:] == ["-O", "8"]
    r5, plain = batch("plain", {})
    r6, filled_maps = batch("fill", dict(MGM_FILL_HOLES="max", MGM_FILL_HOLES_DIRS="4"))
    assert r6.stdout == r5.stdout and r6.stderr.split().count("k_holes") == 2 and same_bits(plain[0], disp0) and not same_bits(plain[1], disp0)
    for got, unfilled in zip(filled_maps, plain):
        want, filled = fill(unfilled, "max", 4, 0)
        assert same_bits(got, want) and filled.sum() > 0
