"""Hole classification and the classified fill on the device (mgm_classify_holes_dev, mgm_fill_holes_classified_dev)
against the numpy model of tests/occlusion_model.py, bit for bit: crafted maps around the kernel's segment, lanes and span (read
from plan_holes_classify, not written here), every range, tau and mode pair, every call form, the refusals and what they leave of
the context, mgm_ms_params.outR_nolr, and the command line's MGM_FILL_HOLES_OCC against the same steps through the Python API."""
import ctypes as C
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

import mgm_amd
from holes_model import CLI_ARGS, CLI_SPECKLE, PAIR, crafted, fill, rays, same_bits
from mgm_amd import synth
from occlusion_model import MODES5, RANGES, TAUS, classify, crafted_d, crafted_other, fill_classified, plan, plan_lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
CONV = os.path.join(ROOT, "mgm_amd", "bin", "imgconv")
f32 = np.float32


def _plan():
    with tempfile.TemporaryDirectory() as tmp:
        lib = plan_lib(tmp)
        c = plan(lib, [(1920, 1080, 1920, 65, 256)])[0]
        return c["seg"], lib.holes_classify_max_span()


SEG, MAX_SPAN = _plan()
LANE = 64
NXS = (1, 63, 64, 65, 130, 257)
NYS = (1, 3, 70)
assert SEG == 256 and any(nx > SEG for nx in NXS) and any(nx == LANE for nx in NXS)  # more than one segment, a lane seam inside one


@pytest.fixture
def tctx(ctx):
    """the session's context with its timing table on and empty"""
    ctx.timing(True)
    ctx.timing_reset()
    yield ctx
    ctx.timing_reset()
    ctx.timing(False)


def names(ctx):
    n = [k for k, _ in ctx.timings() if k.startswith("k_holes")]
    ctx.timing_reset()
    return n


@pytest.mark.parametrize("nx", NXS)
def test_classify_matches_the_model(tctx, nx):
    ctx = tctx
    calls = 0
    for ny in NYS:
        maps = crafted_d(nx, ny, SEG, LANE)
        dds = [(name, d, ctx.upload_image(d)) for name, d in maps]
        cls = ctx.new_image(nx, ny)
        for vnx in (nx + 7, max(1, nx - 5)):
            for dmin, dmax in RANGES:
                for tau in TAUS:
                    other = crafted_other(nx, ny, vnx, dmin, dmax, tau)
                    oo = ctx.upload_image(other)
                    for name, d, dd in dds:
                        got = ctx.classify_holes_dev(dd, oo, dmin, dmax, tau, cls=cls)
                        calls += 1
                        assert got is cls and same_bits(cls.download()[0], classify(d, other, dmin, dmax, tau)), (ny, vnx, dmin, dmax, tau, name)
                    oo.free()
        for name, d, dd in dds:
            assert same_bits(dd.download()[0], d)
            dd.free()
        cls.free()
    assert {"all_holes", "no_holes", "boundaries", "random"} == {n for n, _ in maps}
    assert names(ctx) == ["k_holes_classify"] * calls


def test_classify_on_several_spans_and_strided_rows(tctx):
    """a range of 2401 labels over a map wider than the largest span (the span loop runs twice per segment), and a map with more
    rows than the launch has workgroup rows (a workgroup strides over rows)"""
    ctx = tctx
    for nx, ny, vnx, dmin, dmax, tau in ((1300, 2, 1307, -1200, 1200, 0.5), (3, 65536 + 5, 4, -2, 1, 1.0)):
        assert vnx > MAX_SPAN or ny > 65535
        other = crafted_other(nx, ny, vnx, dmin, dmax, tau)
        for name, d in crafted_d(nx, ny, SEG, LANE)[2:]:
            dd, oo = ctx.upload_image(d), ctx.upload_image(other)
            cls = ctx.classify_holes_dev(dd, oo, dmin, dmax, tau)
            want = classify(d, other, dmin, dmax, tau)
            assert same_bits(cls.download()[0], want), (nx, ny, name)
            assert (want == 1).any() and (want == 2).any()
            for h in (dd, oo, cls):
                h.free()


FILL_SHAPES = [(3, 4), (65, 65), (135, 133)]


@pytest.mark.parametrize("nx,ny", FILL_SHAPES, ids=lambda v: str(v))
def test_classified_fill_matches_the_model(tctx, nx, ny):
    ctx = tctx
    out, filled = ctx.new_image(nx, ny), ctx.new_image(nx, ny)
    calls = calls2 = 0
    for k, (name, d) in enumerate(crafted(nx, ny, 64, 64)):
        r = rays(d)
        rng = np.random.default_rng(k)
        cls = rng.choice(np.array([0, 1, 1, 2, np.nan, 7], np.float32), size=d.shape).astype(np.float32)  # 0, 1, 2, NaN and 7 at holes
        occ = cls == 1
        dd, cc = ctx.upload_image(d), ctx.upload_image(cls)
        for dirs, maxdist, pairs in ((8, 0, [(a, b) for a in MODES5 for b in MODES5]), (8, 3, [(a, b) for a in MODES5 for b in MODES5]),
                                    (4, 0, [("sechigh", "median"), ("seclow", "max"), ("min", "sechigh")]),
                                    (2, 3, [("sechigh", "median"), ("seclow", "max"), ("median", "seclow")])):
            one = {m: fill_classified(d, np.ones_like(d), m, m, dirs, maxdist, r=r) for m in MODES5}   # every hole under rule m
            for mo, mm in pairs:
                want = np.where(occ, one[mo][0].view(np.uint32), one[mm][0].view(np.uint32)).view(np.float32)  # the rule is per pixel
                if (mo, mm) in (("sechigh", "median"), ("seclow", "max")):
                    assert same_bits(want, fill_classified(d, cls, mo, mm, dirs, maxdist, r=r)[0])
                ctx._chk(ctx.lib.mgm_fill_holes_classified_dev(ctx.h, dd.h, cc.h, mo.encode(), mm.encode(), dirs, maxdist, out.h, filled.h))
                calls, calls2 = calls + 1, calls2 + (dirs == 2)
                assert same_bits(out.download()[0], want) and same_bits(filled.download()[0], one[mo][1]), (name, mo, mm, dirs, maxdist)
        assert same_bits(dd.download()[0], d) and same_bits(cc.download()[0], cls), name
        # filled only; then out aliasing d
        want = fill_classified(d, cls, "sechigh", "median", 8, 0, r=r)
        none, f = ctx.fill_holes_classified_dev(dd, cc, out=False, want_filled=True)
        assert none is None and same_bits(f.download()[0], want[1]) and same_bits(dd.download()[0], d)
        o, none = ctx.fill_holes_classified_dev(dd, cc, out=dd)
        assert o is dd and none is None and same_bits(dd.download()[0], want[0])
        calls += 2
        for h in (dd, cc, f):
            h.free()
    got = names(ctx)
    want_n = {"k_holes": calls, "k_holes_rows": calls, "k_holes_apply": calls, "k_holes_carry": calls - calls2, "k_holes_walk": calls - calls2}
    assert all(got.count(k) == v for k, v in want_n.items()) and set(got) == set(want_n)
    out.free(), filled.free()


def test_refusals_and_what_they_leave_of_the_context(tctx):
    ctx = tctx
    nx, ny, vnx = 65, 65, 72
    d = dict(crafted(nx, ny, 64, 64))["random_90"]
    other = crafted_other(nx, ny, vnx, -9, -3, 1.0)
    want_plain = fill(d, "median", 8, 0)
    dd, oo, cls = ctx.upload_image(d), ctx.upload_image(other), ctx.new_image(nx, ny)
    INVALID = mgm_amd.MGM_ERR_INVALID

    def good():
        o, f = ctx.fill_holes_dev(dd, "median", 8, 0, want_filled=True)
        ok = same_bits(o.download()[0], want_plain[0]) and same_bits(f.download()[0], want_plain[1])
        o.free(), f.free()
        return ok

    assert good()                                                     # fill_holes_dev before the new calls ...
    L = ctx.lib
    two, tall, wide = ctx.new_image(nx, ny, 2), ctx.new_image(nx, ny + 1), ctx.new_image(nx + 1, ny)
    two_o, tall_o = ctx.new_image(vnx, ny, 2), ctx.new_image(vnx, ny + 1)
    classify_bad = [(None, oo.h, -9, -3, 1.0, cls.h), (dd.h, None, -9, -3, 1.0, cls.h), (dd.h, oo.h, -9, -3, 1.0, None),     # NULL
                    (two.h, oo.h, -9, -3, 1.0, cls.h), (dd.h, two_o.h, -9, -3, 1.0, cls.h), (dd.h, oo.h, -9, -3, 1.0, two.h),  # channels
                    (dd.h, tall_o.h, -9, -3, 1.0, cls.h),                                                                      # other->ny
                    (dd.h, oo.h, -9, -3, 1.0, tall.h), (dd.h, oo.h, -9, -3, 1.0, wide.h),                                      # cls's size
                    (dd.h, oo.h, -9, -3, 1.0, dd.h), (dd.h, dd.h, -9, -3, 1.0, dd.h), (dd.h, cls.h, -9, -3, 1.0, cls.h),       # cls aliases an input
                    (dd.h, oo.h, -3, -9, 1.0, cls.h), (dd.h, oo.h, 1, 0, 1.0, cls.h),                                          # dmin > dmax
                    (dd.h, oo.h, -9, -3, -1.0, cls.h), (dd.h, oo.h, -9, -3, float("nan"), cls.h), (dd.h, oo.h, -9, -3, float("inf"), cls.h),
                    (dd.h, oo.h, -9, -3, -float("inf"), cls.h)]
    for args in classify_bad:
        assert L.mgm_classify_holes_dev(ctx.h, *args) == INVALID and good(), args
    assert L.mgm_classify_holes_dev(None, dd.h, oo.h, -9, -3, 1.0, cls.h) == INVALID
    got = ctx.classify_holes_dev(dd, oo, -9, -3, 1.0, cls=cls)       # the extremes that are allowed
    assert same_bits(got.download()[0], classify(d, other, -9, -3, 1.0))
    for dmin, dmax, tau in ((-2 ** 31, 2 ** 31 - 1, 0.0), (5, 5, 3.0e38), (-2 ** 31, -2 ** 31, 1.0), (2 ** 31 - 1, 2 ** 31 - 1, 1.0)):
        ctx.classify_holes_dev(dd, oo, dmin, dmax, tau, cls=cls)
        assert same_bits(cls.download()[0], classify(d, other, min(max(dmin, -1000), 1000), max(min(dmax, 1000), -1000), tau)), (dmin, dmax, tau)
    with pytest.raises(mgm_amd.MgmError) as e:                       # the binding frees what it made and raises
        ctx.classify_holes_dev(dd, oo, 1, 0, 1.0)
    assert e.value.code == INVALID and good()

    ctx.classify_holes_dev(dd, oo, -9, -3, 1.0, cls=cls)
    ok, own = ctx.new_image(nx, ny), ctx.new_image(nx, ny)
    s, m = b"sechigh", b"median"
    fill_bad = [(None, cls.h, s, m, 8, 0, ok.h, None), (dd.h, None, s, m, 8, 0, ok.h, None), (dd.h, cls.h, None, m, 8, 0, ok.h, None),
                (dd.h, cls.h, s, None, 8, 0, ok.h, None), (dd.h, cls.h, s, m, 8, 0, None, None)]                              # NULL, neither output
    fill_bad += [(dd.h, cls.h, a, b, 8, 0, ok.h, None) for a, b in ((b"none", m), (s, b"none"), (b"", m), (s, b"Median"), (b"second", m),
                                                                    (s, b"sechigh "), (b"mean", b"mean"))]                    # names
    fill_bad += [(dd.h, cls.h, s, m, dirs, 0, ok.h, None) for dirs in (-1, 0, 1, 3, 6, 16)]
    fill_bad += [(dd.h, cls.h, s, m, 8, -1, ok.h, None)]
    fill_bad += [(dd.h, cls.h, s, m, 8, 0, ok.h, f) for f in (dd.h, cls.h, ok.h)] + [(dd.h, cls.h, s, m, 8, 0, None, dd.h)]   # filled aliases
    fill_bad += [(two.h, cls.h, s, m, 8, 0, ok.h, None), (dd.h, two.h, s, m, 8, 0, ok.h, None), (dd.h, cls.h, s, m, 8, 0, two.h, None),
                 (dd.h, tall.h, s, m, 8, 0, ok.h, None), (dd.h, cls.h, s, m, 8, 0, wide.h, None), (dd.h, cls.h, s, m, 8, 0, ok.h, tall.h)]
    for args in fill_bad:
        assert L.mgm_fill_holes_classified_dev(ctx.h, *args) == INVALID and good(), args
    assert L.mgm_fill_holes_classified_dev(None, dd.h, cls.h, s, m, 8, 0, ok.h, None) == INVALID
    for kw in (dict(mode_occ="second"), dict(mode_mis=None), dict(dirs=3), dict(maxdist=-1), dict(out=False)):
        with pytest.raises(mgm_amd.MgmError) as e:
            ctx.fill_holes_classified_dev(dd, cls, **kw)
        assert e.value.code == INVALID and good(), kw
    o, f = ctx.fill_holes_classified_dev(dd, cls, "seclow", "max", 4, 2 ** 31 - 1, out=ok, want_filled=True)
    want = fill_classified(d, cls.download()[0], "seclow", "max", 4, 0)
    assert o is ok and same_bits(ok.download()[0], want[0]) and same_bits(f.download()[0], want[1])
    assert good() and same_bits(dd.download()[0], d)                  # ... and after them: identical bits
    for h in (dd, oo, cls, two, tall, wide, two_o, tall_o, ok, own, f):
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
            other = c2.upload_image(-o.download()[0])
            cls = c2.classify_holes_dev(s, other, -3, 3, 1.0)
            f, m = c2.fill_holes_classified_dev(s, cls, "sechigh", "median", want_filled=True)
            res.append((f.download()[0], m.download()[0], cls.download()[0], o.download()[0]))
            assert {"k_holes", "k_holes_classify"} <= {n for n, _ in c2.timings()}
    assert all(same_bits(x, y) for x, y in zip(res[1], res[0]))
    holes = speckle(res[0][3], 3, 1.0)[0]
    cls = classify(holes, -res[0][3], -3, 3, 1.0)
    want = fill_classified(holes, cls, "sechigh", "median")
    assert same_bits(res[0][2], cls) and same_bits(res[0][0], want[0]) and same_bits(res[0][1], want[1]) and want[1].sum() > 0


# ---- mgm_ms_params.outR_nolr -------------------------------------------------------------------------------------------------------------
PAIR_KW = dict(P1=PAIR["P1"], P2=PAIR["P2"], NDIR=PAIR["NDIR"], TSGM=PAIR["TSGM"], distance="census", refine="none")


def pair_images(ctx):
    p = PAIR
    u, v, _ = synth.stereo_pair(p["nx"], p["ny"], p["dmin"], p["dmax"])
    return u, v, ctx.upload_image(u), ctx.upload_image(v)


def by_hand(ctx, du, dv, NDIR=PAIR["NDIR"], rfl=False):
    """(checked left map, right map before its left-right test) of the pair: both runs (or the right map out of the left run), the
    left-right test at tau 1"""
    p = PAIR
    cvL = ctx.costvolume_dev(du, dv, p["dmin"], p["dmax"], "none", "census")
    _, oL, cL = ctx.aggregate_dev(cvL, p["P1"], p["P2"], NDIR, p["TSGM"], 0, 1, None, None)
    if rfl:
        oR, cR = ctx.wta_right_dev(cvL, NDIR, 1, None, dv.shape[2])
    else:
        cvR = ctx.costvolume_dev(dv, du, -p["dmax"], -p["dmin"], "none", "census")
        _, oR, cR = ctx.aggregate_dev(cvR, p["P1"], p["P2"], NDIR, p["TSGM"], 0, 1, None, None)
        cvR.free()
    chk = ctx.leftright_dev(oL, oR, 1.0)
    for h in (cvL, oL, cL, cR):
        h.free()
    return chk, oR


def test_multiscale_right_map_before_its_leftright_test(ctx):
    p = PAIR
    u, v, du, dv = pair_images(ctx)
    chk, oR = by_hand(ctx, du, dv)
    base = {}
    for S in (1, 2):
        plain = ctx.multiscale_pair(du, dv, p["dmin"], p["dmax"], S, **PAIR_KW)
        more = ctx.multiscale_pair(du, dv, p["dmin"], p["dmax"], S, want_right_nolr=True, **PAIR_KW)
        assert plain["outR_nolr"] is None and more["outR_nolr"] is not None
        for k in ("outL", "costL", "outR", "costR", "nolr"):                 # NULL: the same maps as with it
            assert same_bits(plain[k].download()[0], more[k].download()[0]), (S, k)
        rn = more["outR_nolr"].download()[0]
        assert not same_bits(rn, more["outR"].download()[0])
        # the map is the one the left map was checked against
        from multiscale_model import leftright
        assert same_bits(leftright(more["nolr"].download()[0], rn, 1.0), more["outL"].download()[0]), S
        if S == 1:
            assert same_bits(rn, oR.download()[0]) and same_bits(more["outL"].download()[0], chk.download()[0])
        base[S] = {k: plain[k].download()[0] for k in ("outL", "costL", "outR", "costR", "nolr")}
        for res in (plain, more):
            for k, im in res.items():
                if k != "levels" and im is not None:
                    im.free()
    # an old caller: struct_size ends before outR_nolr, whatever lies behind it is not read
    for S in (1, 2):
        res = dict(outL=ctx.new_image(p["nx"], p["ny"]), costL=ctx.new_image(p["nx"], p["ny"]), outR=ctx.new_image(p["nx"], p["ny"]),
                   costR=ctx.new_image(p["nx"], p["ny"]), nolr=ctx.new_image(p["nx"], p["ny"]))
        mark = np.full((p["ny"], p["nx"]), 42.0, np.float32)
        untouched = ctx.upload_image(mark)
        n = C.c_int(0)
        old = mgm_amd.MsParams.outR_nolr.offset
        assert old == C.sizeof(mgm_amd.MsParams) - C.sizeof(C.c_void_p)
        prm = mgm_amd.MsParams(old, S, 3, 2, p["dmin"], p["dmax"], None, None, p["P1"], p["P2"], p["NDIR"], p["TSGM"], 0, 1, 1.0, 5.0, b"none",
                               b"census", float("inf"), 3, b"none", 1, 0, 1, 1.0, C.pointer(n), None, untouched.h)
        ctx._chk(ctx.lib.mgm_multiscale_pair_dev(ctx.h, du.h, dv.h, C.byref(prm), res["outL"].h, res["costL"].h, res["outR"].h, res["costR"].h,
                                                 res["nolr"].h))
        for k in res:
            assert same_bits(res[k].download()[0], base[S][k]), (S, k)
        assert same_bits(untouched.download()[0], mark)
        # ... a new caller with a map of the wrong size is refused
        prm.struct_size = C.sizeof(mgm_amd.MsParams)
        wrong = ctx.new_image(p["nx"] + 1, p["ny"])
        prm.outR_nolr = wrong.h.value
        assert ctx.lib.mgm_multiscale_pair_dev(ctx.h, du.h, dv.h, C.byref(prm), res["outL"].h, res["costL"].h, res["outR"].h, res["costR"].h,
                                               res["nolr"].h) == mgm_amd.MGM_ERR_INVALID
        for im in list(res.values()) + [untouched, wrong]:
            im.free()
    for h in (du, dv, chk, oR):
        h.free()


# ---- the command line ----------------------------------------------------------------------------------------------------------------
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


CLI_ENV = dict(MGM_SPECKLE=str(CLI_SPECKLE), MGM_FILL_HOLES="median", MGM_FILL_HOLES_OCC="sechigh", MGM_HIP_KERNELS="1")


def api_steps(ctx, chk, other, tag):
    """speckle, classify, classified fill on the checked left map and the unchecked right map, through the Python API: the map the
    command line must write, bit for bit.  Asserts that the case means something and prints its counts."""
    p = PAIR
    s, _ = ctx.speckle_dev(chk, CLI_SPECKLE, 1.0)
    cls = ctx.classify_holes_dev(s, other, p["dmin"], p["dmax"], 1.0)
    out, filled = ctx.fill_holes_classified_dev(s, cls, "sechigh", "median", 8, 0, want_filled=True)
    plain, _ = ctx.fill_holes_dev(s, "median", 8, 0)
    c, f, o, m, holes = cls.download()[0], filled.download()[0], out.download()[0], plain.download()[0], s.download()[0]
    n1, n2, nd = int(((c == 1) & (f == 1)).sum()), int(((c == 2) & (f == 1)).sum()), int((o.view(np.uint32) != m.view(np.uint32)).sum())
    print("%s: %d holes, filled %d occlusions and %d mismatches, %d pixels differ from MGM_FILL_HOLES=median" % (tag, (c != 0).sum(), n1, n2, nd))
    assert n1 > 0 and n2 > 0 and nd > 0, tag
    # the device steps against the model on the same inputs
    want_c = classify(holes, other.download()[0], p["dmin"], p["dmax"], 1.0)
    assert same_bits(c, want_c) and same_bits(o, fill_classified(holes, want_c, "sechigh", "median")[0])
    for h in (s, cls, out, filled, plain):
        h.free()
    return o


def kernels_of(r):
    return [l for l in r.stderr.splitlines() if l.startswith("[mgm kernels]")]


@pytest.mark.parametrize("variant", ["single", "s2", "right_from_left", "batch"])
def test_command_line(ctx, tmp_path, variant):
    """MGM_SPECKLE=100 MGM_FILL_HOLES=median MGM_FILL_HOLES_OCC=sechigh on the 96 x 64 synthetic pair of tests/test_gpu_holes.py"""
    p = PAIR
    u, v, du, dv = pair_images(ctx)
    fu, fv = str(tmp_path / "u.png"), str(tmp_path / "v.png")
    write_png(fu, u[0]), write_png(fv, v[0])
    args = CLI_ARGS.split()
    assert args[-2:] == ["-O", "8"]
    fo = str(tmp_path / "out.tif")
    if variant == "batch":
        outs = [str(tmp_path / ("batch_%d.tif" % k)) for k in range(2)]
        (tmp_path / "batch.txt").write_text(" ".join(args + [fu, fv, outs[0]]) + "\n" + " ".join(args[:-1] + ["4", fu, fv, outs[1]]) + "\n")
        r = run_cli(["--batch", str(tmp_path / "batch.txt")], CLI_ENV)
        assert r.returncode == 0, r.stderr
        for out, NDIR in zip(outs, (8, 4)):
            chk, oR = by_hand(ctx, du, dv, NDIR)
            assert same_bits(read_tif(out), api_steps(ctx, chk, oR, "batch -O %d" % NDIR)), NDIR
            chk.free(), oR.free()
        assert r.stderr.split().count("k_holes_classify") == 2 and r.stderr.split().count("k_holes") == 2
    else:
        extra, env = {"single": ([], {}), "s2": (["-S", "2"], {}), "right_from_left": ([], {"MGM_RIGHT_FROM_LEFT": "1"})}[variant]
        r = run_cli(args + extra + [fu, fv, fo, str(tmp_path / "cost.tif"), str(tmp_path / "back.tif")], dict(CLI_ENV, **env))
        assert r.returncode == 0, r.stderr
        if variant == "s2":
            res = ctx.multiscale_pair(du, dv, p["dmin"], p["dmax"], 2, want_right_nolr=True, **PAIR_KW)
            assert len(res["levels"]) == 2
            chk, oR = res["outL"], res["outR_nolr"]
            for k in ("costL", "outR", "costR", "nolr"):
                res[k].free()
        else:
            chk, oR = by_hand(ctx, du, dv, rfl=variant == "right_from_left")
        assert same_bits(read_tif(fo), api_steps(ctx, chk, oR, variant))
        chk.free(), oR.free()
        k = kernels_of(r)[0].split()
        assert k.count("k_holes_classify") == 1 and k.count("k_holes") == 1
        assert k.index("k_speckle") < k.index("k_holes_classify") < k.index("k_holes") < k.index("k_backproject")
        if variant == "single":   # MGM_FILL_HOLES_OCC=none and an empty value are today's behaviour; TESTLRRL=0 has no right view
            r1 = run_cli(args + [fu, fv, str(tmp_path / "median.tif")], dict(CLI_ENV, MGM_FILL_HOLES_OCC=""))
            r2 = run_cli(args + [fu, fv, str(tmp_path / "none.tif")], dict(CLI_ENV, MGM_FILL_HOLES_OCC="none"))
            assert r1.returncode == 0 and r2.returncode == 0 and "k_holes_classify" not in (r1.stderr + r2.stderr).split()
            assert same_bits(read_tif(str(tmp_path / "median.tif")), read_tif(str(tmp_path / "none.tif")))
            assert not same_bits(read_tif(str(tmp_path / "median.tif")), read_tif(fo))
            r3 = run_cli(args + [fu, fv, str(tmp_path / "never.tif")], dict(CLI_ENV, TESTLRRL="0"))
            assert r3.returncode == 2 and "needs the right view" in r3.stderr and not os.path.exists(str(tmp_path / "never.tif"))
    du.free(), dv.free()
