"""The coarse-to-fine (multiscale) driver on the device against its numpy model (tests/multiscale_model.py on the CPU
oracle): the three resampling primitives, mgm_multiscale_pair_dev on the fountain23 pair (full size and a crop matrix), the
`mgm -S` command line.  Every comparison is bit for bit with NaN == NaN."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import mgm_amd
import multiscale_model as msm
from helpers import GOLDEN, ndiff
from oracle import oracle as orc_mod

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
F = np.float32
CLI_KW = dict(P1=8.0 * 3, P2=32.0 * 3, NDIR=8, TSGM=4, distance="census", census_win=5, refine="vfit")


@pytest.fixture(scope="module")
def fountain():
    d = np.load(os.path.join(GOLDEN, "cfg1_fountain23.npz"))
    uL = np.ascontiguousarray(d["uL"].astype(F).transpose(2, 0, 1))
    uR = np.ascontiguousarray(d["uR"].astype(F).transpose(2, 0, 1))
    return uL, uR, d["uL"], d["uR"]


@pytest.fixture(scope="module")
def crop(fountain):
    uL, uR = fountain[:2]
    return np.ascontiguousarray(uL[:, 150:342, 300:556]), np.ascontiguousarray(uR[:, 150:342, 300:556])  # 256 x 192 x 3


@pytest.fixture(scope="module")
def big_oracle():
    return orc_mod.Oracle(threads=orc_mod.usable_cpus(16))


@pytest.fixture(scope="module")
def fountain_model(big_oracle, fountain):
    """The model's answer for the full-size case (about 10 s on 16 threads), shared by the library and the command-line test."""
    return msm.multiscale_pair(big_oracle, fountain[0], fountain[1], -120, 30, 3, **CLI_KW)


# ---- the three primitives ---------------------------------------------------------------------------------------------
SIZES = [(1, 1, 1), (1, 17, 1), (16, 16, 1), (17, 33, 1), (700, 500, 3), (1920, 1080, 1)]


def ranges_for(rng, ny, nx):
    """negative, fractional and lo == hi ranges"""
    lo = rng.integers(-150, 60, size=(ny, nx)).astype(F) + np.where(rng.random((ny, nx)) < 0.5, rng.random((ny, nx)), 0).astype(F)
    hi = lo + np.where(rng.random((ny, nx)) < 0.2, 0, rng.integers(0, 60, size=(ny, nx)) + rng.random((ny, nx))).astype(F)
    return lo.astype(F), hi.astype(F)


@pytest.mark.parametrize("nx,ny,nch", SIZES)
def test_zoom_out_primitives(ctx, nx, ny, nch):
    rng = np.random.default_rng(nx * 7 + ny)
    img = (rng.random((nch, ny, nx)) * 255).astype(F)
    img[:, ::3, ::2] = np.floor(img[:, ::3, ::2])
    d = ctx.upload_image(img)
    z = ctx.zoom_out_dev(d)
    assert z.shape == (nch, msm.half(ny), msm.half(nx))
    assert ndiff(z.download(), msm.zoom_out(img)) == 0
    again = ctx.zoom_out_dev(d, out=z)  # refilled in place
    assert again is z and ndiff(z.download(), msm.zoom_out(img)) == 0
    lo, hi = ranges_for(rng, ny, nx)
    dl, dh = ctx.upload_image(lo), ctx.upload_image(hi)
    l2, h2 = ctx.ranges_zoom_out_dev(dl, dh)
    wl, wh = msm.ranges_zoom_out(lo, hi)
    assert ndiff(l2.download()[0], wl) == 0 and ndiff(h2.download()[0], wh) == 0
    for im in (d, z, dl, dh, l2, h2):
        im.free()


@pytest.mark.parametrize("nx,ny,nch", SIZES)
def test_ranges_from_coarse_primitive(ctx, nx, ny, nch):
    rng = np.random.default_rng(nx * 11 + ny)
    cny, cnx = msm.half(ny), msm.half(nx)
    lo, hi = ranges_for(rng, ny, nx)
    base = (rng.integers(-120, 30, size=(cny, cnx)) + rng.random((cny, cnx))).astype(F)
    maps = {}
    for frac in (0.0, 0.1, 1.0):
        m = base.copy()
        m[rng.random(m.shape) < frac] = np.nan
        maps[frac] = m
    combos = [(3, 2, 0.1), (0, 0, 0.0), (7, 16, 0.1), (3, 2, 1.0), (3, 2, 0.0), (0, 16, 1.0), (7, 0, 0.1)]
    if nx * ny > 10 ** 6:
        combos = combos[:4]
    for slack, radius, frac in combos:
        D = maps[frac]
        dl, dh, dD = ctx.upload_image(lo), ctx.upload_image(hi), ctx.upload_image(D)
        hull = ctx.ranges_from_coarse_dev(dD, dl, dh, slack, radius)
        wl, wh = msm.ranges_from_coarse(D, lo, hi, slack, radius)
        assert ndiff(dl.download()[0], wl) == 0 and ndiff(dh.download()[0], wh) == 0, (slack, radius, frac)
        assert hull == msm.int_hull(wl, wh), (slack, radius, frac, hull)
        dl.update(lo), dh.update(hi)
        assert ctx.ranges_from_coarse_dev(dD, dl, dh, slack, radius, want_hull=False) is None
        assert ndiff(dl.download()[0], wl) == 0 and ndiff(dh.download()[0], wh) == 0
        for im in (dl, dh, dD):
            im.free()


def test_primitives_refuse_bad_sizes(ctx):
    a, b, c = ctx.new_image(20, 10), ctx.new_image(20, 10), ctx.new_image(11, 5)  # the coarse map of 20x10 is 10x5
    with pytest.raises(mgm_amd.MgmError) as e:
        ctx.ranges_from_coarse_dev(c, a, b)
    assert e.value.code == mgm_amd.MGM_ERR_INVALID
    with pytest.raises(mgm_amd.MgmError) as e:
        ctx.ranges_zoom_out_dev(a, c)
    assert e.value.code == mgm_amd.MGM_ERR_INVALID
    with pytest.raises(mgm_amd.MgmError) as e:
        ctx.zoom_out_dev(a, out=c)
    assert e.value.code == mgm_amd.MGM_ERR_INVALID
    for im in (a, b, c):
        im.free()


# ---- the driver -------------------------------------------------------------------------------------------------------
def run_device(ctx, u, v, dmin, dmax, S, lo=None, hi=None, **kw):
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    dl = ctx.upload_image(lo) if lo is not None else None
    dh = ctx.upload_image(hi) if hi is not None else None
    res = ctx.multiscale_pair(du, dv, dmin, dmax, S, lo=dl, hi=dh, **kw)
    got = {k: (res[k].download()[0] if res[k] is not None else None) for k in ("outL", "costL", "outR", "costR", "nolr")}
    got["levels"] = res["levels"]
    for im in [du, dv, dl, dh] + [res[k] for k in ("outL", "costL", "outR", "costR", "nolr")]:
        if im is not None:
            im.free()
    return got


def compare(got, want, what):
    for k in ("outL", "outR", "costL", "nolr"):  # left and right disparity, left cost, the map before the left-right test
        if want[k] is None:
            assert got[k] is None, (what, k)
        else:
            assert ndiff(got[k], want[k]) == 0, (what, k, ndiff(got[k], want[k]))
    assert len(got["levels"]) == len(want["levels"]), what
    for lg, lw in zip(got["levels"], want["levels"]):
        assert (lg["nx"], lg["ny"], lg["vnx"], lg["vny"]) == lw["dims"], what


def test_full_size_fountain_three_scales(fountain_model, fountain):
    """-r -120 -R 30, census 5x5, NDIR 8, TSGM 4, vfit, S = 3 at 700x500x3 -- and the path the feature exists for: every level
    below the coarsest runs the range-proportional pass kernel."""
    u, v = fountain[:2]
    kw, want = CLI_KW, fountain_model
    widths = [int((orc_mod.int_ranges(*lv["ranges"][k])[1] - orc_mod.int_ranges(*lv["ranges"][k])[0] + 1).max())
              for lv in want["levels"][:-1] for k in range(2)]
    print("widest window per fine level and run (labels):", widths)
    with mgm_amd.Context(0) as ctx:
        ctx.timing(True)
        got = run_device(ctx, u, v, -120, 30, 3, **kw)
        names = [n for n, _ in ctx.timings()]
        ctx.timing(False)
    compare(got, want, "fountain23 S=3")
    # the launches between two prior -> ranges steps (and after the last) belong to one fine-level run
    marks = [i for i, n in enumerate(names) if n == "k_ranges_from_coarse"]
    assert len(marks) == 4, names  # two fine levels x two runs
    per_level = [names[marks[0]:marks[2]], names[marks[2]:]]
    for lv, seg in enumerate(per_level):
        passes = [n for n in seg if n.startswith("k_pass")]
        print("fine level", 1 - lv, "pass kernels:", passes)
        assert passes and all(n == "k_pass_rel" for n in passes), (lv, seg)
    assert all(w <= 126 for w in widths), widths


def crop_case(ctx, big_oracle, crop, S, what, lo=None, hi=None, v=None, dmin=-120, dmax=30, **kw):
    u, v0 = crop
    v = v0 if v is None else v
    want = msm.multiscale_pair(big_oracle, u, v, dmin, dmax, S, lo=lo, hi=hi, **kw)
    got = run_device(ctx, u, v, dmin, dmax, S, lo=lo, hi=hi, **kw)
    compare(got, want, what)
    return got, want


COSTS = {"ad": dict(distance="ad"), "census": dict(distance="census", census_win=5), "ncc": dict(distance="ncc", census_win=3)}
POTENTIALS = {"hirsch": dict(use_fh=0, P1=24.0, P2=96.0), "fh": dict(use_fh=1, P1=6.0, P2=60.0)}


@pytest.mark.parametrize("refine", ["none", "vfit", "cubic"])
@pytest.mark.parametrize("ndir", [4, 8])
@pytest.mark.parametrize("pot", sorted(POTENTIALS))
@pytest.mark.parametrize("cost", sorted(COSTS))
@pytest.mark.parametrize("S", [1, 2, 3, 4])
def test_crop_matrix(ctx, big_oracle, crop, S, cost, pot, ndir, refine):
    kw = dict(COSTS[cost], **POTENTIALS[pot], NDIR=ndir, TSGM=3, refine=refine)
    got, _ = crop_case(ctx, big_oracle, crop, S, (S, cost, pot, ndir, refine), **kw)
    assert len(got["levels"]) == S


BASE = dict(distance="census", census_win=5, P1=24.0, P2=96.0, NDIR=8, TSGM=4, refine="vfit")


@pytest.mark.parametrize("name,extra", [
    ("aP2=4", dict(aP2=4.0, aThresh=12.0, distance="ad")),
    ("MEDIAN=1", dict(median=1)),
    ("TESTLRRL=0", dict(testlrrl=0)),
    ("TSGM_ITER=2", dict(iterations=2)),
    ("P2=inf", dict(P2=float("inf"))),
])
def test_crop_single_cases(ctx, big_oracle, crop, name, extra):
    got, _ = crop_case(ctx, big_oracle, crop, 3, name, **dict(BASE, **extra))
    if name == "aP2=4":
        assert all(lv["weighted"] == [True, True] for lv in got["levels"])


def test_crop_base_ranges_from_images(ctx, big_oracle, crop):
    """-m / -M at level 0: ranges with negative, fractional and tight entries, as main() leaves them (mgm.cc:342-353)."""
    ny, nx = crop[0].shape[1:]
    rng = np.random.default_rng(5)
    lo = (-110 + 30 * rng.random((ny, nx))).astype(F)
    lo[:, ::5] = np.floor(lo[:, ::5])
    hi = (lo + 60 + 60 * rng.random((ny, nx))).astype(F)
    hi[::7] = np.ceil(lo[::7] + 1)
    crop_case(ctx, big_oracle, crop, 3, "-m/-M", lo=lo, hi=hi, **BASE)


def test_crop_right_image_eight_columns_narrower(ctx, big_oracle, crop):
    crop_case(ctx, big_oracle, crop, 3, "narrow right image", v=np.ascontiguousarray(crop[1][:, :, :-8]), **BASE)


def test_one_scale_is_the_single_scale_path(crop):
    """S = 1 equals the existing calls: uniform volumes, one batched launch, the two left-right tests."""
    u, v = crop
    ny, nx = u.shape[1:]
    with mgm_amd.Context(0) as ctx:
        got = run_device(ctx, u, v, -120, 30, 1, **BASE)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        cl = ctx.costvolume_dev(du, dv, -120, 30, "none", "census", float("inf"), 5)
        cr = ctx.costvolume_dev(dv, du, -30, 120, "none", "census", float("inf"), 5)
        _, outs, costs = ctx.aggregate_batch_dev([cl, cr], 24.0, 96.0, 8, 4, 0, 1, None, "vfit")
        L = ctx.leftright_dev(outs[0], outs[1], 1.0)
        R = ctx.leftright_dev(outs[1], outs[0], 1.0)
        assert ndiff(got["nolr"], outs[0].download()[0]) == 0
        assert ndiff(got["outL"], L.download()[0]) == 0 and ndiff(got["outR"], R.download()[0]) == 0
        assert ndiff(got["costL"], costs[0].download()[0]) == 0 and ndiff(got["costR"], costs[1].download()[0]) == 0
        assert len(got["levels"]) == 1 and got["levels"][0]["hull"] == [(-120, 30), (-30, 120)] and got["levels"][0]["batched"]


def test_more_levels_than_fit_returns_the_effective_count(crop):
    u, v = crop
    with mgm_amd.Context(0) as ctx:
        got = run_device(ctx, u, v, -120, 30, 8, **BASE)  # 256x192 -> ... -> 32x24 -> 16x12 does not count
        got4 = run_device(ctx, u, v, -120, 30, 4, **BASE)
    assert len(got["levels"]) == 4 == len(mgm_amd.multiscale_levels(256, 192, nscales=8))
    for k in ("outL", "outR", "costL", "nolr"):
        assert ndiff(got[k], got4[k]) == 0


def test_one_context_across_shapes(crop):
    """A 2-scale pair, a dense single volume of another shape, a 4-scale pair of a third shape, the first pair again: all equal
    to what fresh contexts give (the planner's caches must not leak from one shape to the next)."""
    from mgm_amd import synth
    u, v = crop
    u2, v2 = np.ascontiguousarray(u[:, :150, :200]), np.ascontiguousarray(v[:, :150, :200])
    su, sv, _ = synth.stereo_pair(180, 100, -40, 0, seed=3)

    def dense(ctx):
        du, dv = ctx.upload_image(su), ctx.upload_image(sv)
        cv = ctx.costvolume_dev(du, dv, -63, 0, "none", "census", float("inf"), 5)
        _, o, c = ctx.aggregate_dev(cv, 2.0, 20000.0, 8, 3, 1, 1, None, "vfit")
        return dict(o=o.download()[0], c=c.download()[0])

    steps = [lambda c: run_device(c, u, v, -120, 30, 2, **BASE), dense, lambda c: run_device(c, u2, v2, -120, 30, 4, **BASE),
             lambda c: run_device(c, u, v, -120, 30, 2, **BASE)]
    fresh = []
    for f in steps[:3]:
        with mgm_amd.Context(0) as c:
            fresh.append(f(c))
    fresh.append(fresh[0])
    with mgm_amd.Context(0) as c:
        for n, f in enumerate(steps):
            got = f(c)
            for k, w in fresh[n].items():
                if isinstance(w, np.ndarray):
                    assert ndiff(got[k], w) == 0, (n, k)


def test_errors_leave_the_context_clean(crop):
    u, v = crop
    ny, nx = u.shape[1:]
    with mgm_amd.Context(0) as ctx:
        run_device(ctx, u, v, -120, 30, 2, **BASE)  # (the context has been through a pair: its workspace exists)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        small = ctx.new_image(nx // 2, ny)
        full = ctx.new_image(nx, ny)
        lib = ctx.lib

        def call(S, lo=None, hi=None, null_outputs=False, census_win=5):
            import ctypes as C
            ctx.trim()
            before = ctx.mem_info()[0]
            o, k = ctx.new_image(nx, ny), ctx.new_image(nx, ny)
            p = mgm_amd.MsParams(C.sizeof(mgm_amd.MsParams), S, 3, 2, -120, 30, lo.h if lo else None, hi.h if hi else None, 24.0, 96.0, 8, 4, 0, 1,
                                 1.0, 5.0, b"none", b"census", float("inf"), census_win, b"vfit", 1, 0, 1, 1.0, None, None)
            r = lib.mgm_multiscale_pair_dev(ctx.h, du.h, dv.h, C.byref(p), None if null_outputs else o.h, None if null_outputs else k.h, None, None, None)
            msg = lib.mgm_last_error(ctx.h).decode()
            o.free(), k.free()
            ctx.trim()
            after = ctx.mem_info()[0]
            return r, msg, before, after

        for args in (dict(S=0), dict(S=9), dict(S=2, lo=small, hi=full), dict(S=2, null_outputs=True)):
            r, msg, before, after = call(**args)
            assert r == mgm_amd.MGM_ERR_INVALID and "mgm_multiscale_pair" in msg, (args, r, msg)
            assert after >= before, (args, before, after)
        # a failure AFTER the pyramids, the range images and the first level's objects exist (the census window is refused by the
        # coarsest level's cost volume: nch * (win * win - 1) must be a positive multiple of 8): everything the driver made is freed
        r, msg, before, after = call(S=3, census_win=1)
        assert r == mgm_amd.MGM_ERR_INVALID and "census" in msg, (r, msg)
        assert after >= before, ("late failure", before, after)
        # ... and the context still computes
        again = run_device(ctx, u, v, -120, 30, 2, **BASE)
    with mgm_amd.Context(0) as fresh:
        want = run_device(fresh, u, v, -120, 30, 2, **BASE)
    assert ndiff(again["outL"], want["outL"]) == 0 and ndiff(again["costL"], want["costL"]) == 0


# ---- the command line -------------------------------------------------------------------------------------------------
def write_png(path, rgb):
    """8-bit RGB PNG, filter 0 on every row."""
    h, w, _ = rgb.shape
    raw = b"".join(b"\x00" + rgb[y].astype(np.uint8).tobytes() for y in range(h))
    chunk = lambda t, d: struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


CLI_ARGS = "-r -120 -R 30 -t census -s vfit -O 8"
CLI_ENV = dict(CENSUS_NCC_WIN="5", TSGM="4")


def expected_stdout(nlevels, ndir=8, runs=2, iters=1):
    return "-120 30\n" + ("".join(str(p) for p in range(ndir)) + "\n") * (nlevels * runs * iters)


def test_cli_three_scales_on_the_fountain_pngs(fountain_model, fountain, tmp_path):
    u, v, rawL, rawR = fountain
    write_png(tmp_path / "L.png", rawL), write_png(tmp_path / "R.png", rawR)
    f = lambda n: str(tmp_path / n)
    cmd = [OURS] + CLI_ARGS.split() + ["-S", "3", "-l", f("nolr.npy"), f("L.png"), f("R.png"), f("disp.npy"), f("cost.npy")]
    r = subprocess.run(cmd, env=dict(os.environ, **CLI_ENV), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want = fountain_model
    assert r.stdout == expected_stdout(3)
    for name, key in (("disp.npy", "outL"), ("cost.npy", "costL"), ("nolr.npy", "nolr")):
        assert ndiff(np.load(f(name)).reshape(500, 700), want[key]) == 0, name


def test_cli_batch_mixes_scales_and_plain_lines_equal_S1(big_oracle, crop, tmp_path):
    u, v = crop
    np.save(tmp_path / "L.npy", np.ascontiguousarray(u.transpose(1, 2, 0)))
    np.save(tmp_path / "R.npy", np.ascontiguousarray(v.transpose(1, 2, 0)))
    f = lambda n: str(tmp_path / n)
    line = lambda tag, extra: " ".join(CLI_ARGS.split() + extra + [f("L.npy"), f("R.npy"), f(tag + "_disp.npy"), f(tag + "_cost.npy")])
    (tmp_path / "list.txt").write_text("\n".join([line("a", ["-S", "1"]), line("b", ["-S", "3"]), line("c", []), line("d", ["-S", "3"])]) + "\n")
    env = dict(os.environ, **CLI_ENV)
    r = subprocess.run([OURS, "--batch", f("list.txt")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == expected_stdout(1) + expected_stdout(3) + expected_stdout(1) + expected_stdout(3)
    want3 = msm.multiscale_pair(big_oracle, u, v, -120, 30, 3, **CLI_KW)
    want1 = msm.multiscale_pair(big_oracle, u, v, -120, 30, 1, **CLI_KW)
    for tag, want in (("a", want1), ("b", want3), ("c", want1), ("d", want3)):
        assert ndiff(np.load(f(tag + "_disp.npy")).reshape(192, 256), want["outL"]) == 0, tag
        assert ndiff(np.load(f(tag + "_cost.npy")).reshape(192, 256), want["costL"]) == 0, tag
    # a plain command line and the same line with -S 1: stdout and every output byte for byte
    outs = {}
    for tag, extra in (("plain", []), ("s1", ["-S", "1"])):
        files = [f(tag + "_disp.tif"), f(tag + "_cost.tif"), f(tag + "_back.tif")]
        q = subprocess.run([OURS] + CLI_ARGS.split() + extra + [f("L.npy"), f("R.npy")] + files, env=env, capture_output=True, text=True, timeout=600)
        assert q.returncode == 0, q.stderr
        outs[tag] = (q.stdout, [open(p, "rb").read() for p in files])
    assert outs["plain"] == outs["s1"]
