"""Sub-pixel label spacing on the device (mgm_subpix.hip) against the numpy model over the CPU oracle
(tests/subpix_model.py), bit for bit (NaNs equal to one another: see the model's note): the phase images, the fine volume in both of
its forms, the form it is left in, refills and scratch reuse, the rescale, Context.pair_subpix, the command line, the error paths."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import mgm_amd
import subpix_model as M
from mgm_amd import synth
from oracle import post
from holes_model import fill
from speckle_model import speckle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
CONV = os.path.join(ROOT, "mgm_amd", "bin", "imgconv")
INF = float("inf")


def pair(nx, ny, vnx=None, nch=1, seed=1):
    """integer grey levels 0..255, (nch, ny, nx) and (nch, ny, vnx)"""
    rng = np.random.default_rng(1000 * nx + 10 * ny + seed)
    vnx = vnx or nx
    w = max(nx, vnx) + 8
    base = rng.integers(0, 256, (nch, ny, w)).astype(np.float32)
    base = np.rint((base + np.roll(base, 1, 2)) / np.float32(2))
    return np.ascontiguousarray(base[:, :, 3:3 + nx]), np.ascontiguousarray(base[:, :, :vnx])


# ---- phase images ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("vnx", [1, 2, 3, 64, 67])
def test_phase_images(ctx, vnx, nch):
    rng = np.random.default_rng(vnx + nch)
    v = (rng.integers(0, 256, (nch, 5, vnx)) + rng.random((nch, 5, vnx))).astype(np.float32)
    dv = ctx.upload_image(v)
    into = None
    for interp in M.INTERPS:
        for s, k in M.PHASES:
            into = ctx.subpix_phase_dev(dv, s, k, interp, into=into)     # the first call makes the image, the others refill it
            assert M.same_bits(into.download(), M.phase_image(v, s, k, interp)), (interp, s, k)
    into.free(), dv.free()


def test_phase_image_of_special_pixels(ctx):
    v = np.tile(np.arange(1, 20, dtype=np.float32), (1, 4, 1))
    v[0, 0, [3, 9]] = np.nan
    v[0, 1, [0, 7]] = np.inf
    v[0, 1, 12] = -np.inf
    v[0, 2, 4:8] = [1e-41, -3e-42, 1e-45, -0.0]                          # denormals survive the products that are exact
    v[0, 3, [18, 17]] = [np.inf, -np.inf]                                 # INF - INF at the clamped edge
    dv = ctx.upload_image(v)
    for interp in M.INTERPS:
        for s, k in M.PHASES:
            got = ctx.subpix_phase_dev(dv, s, k, interp)
            want = M.phase_image(v, s, k, interp)
            assert M.same_bits(got.download(), want), (interp, s, k)
            if k:
                assert np.isnan(want).sum() > 2
            got.free()
    got = ctx.subpix_phase_dev(dv, 4, 0, "linear")
    assert np.array_equal(got.download().view(np.uint32), v.view(np.uint32))   # v_0: the same bits
    got.free(), dv.free()


# ---- the fine volume, downloaded -------------------------------------------------------------------------------------------------
# (nx, vnx, nch, dmin, L, s, interp, prefilter, distance, truncDist): every axis value with each s at least once
VOLUMES = [
    (1, 1, 1, 0, 1, 2, "cubic", "none", "census", INF), (1, 1, 1, -1, 2, 4, "linear", "none", "ad", INF),
    (5, 5, 1, -2, 3, 2, "cubic", "none", "census", INF), (5, 5, 1, -1, 3, 4, "cubic", "none", "sd", 300.0),
    (64, 64, 1, -40, 33, 2, "linear", "none", "census", 12.0), (64, 64, 1, -40, 33, 4, "cubic", "none", "census", INF),
    (67, 67, 1, -70, 64, 2, "cubic", "none", "census", INF), (67, 67, 1, -70, 64, 4, "cubic", "none", "census", 9.0),
    (130, 130, 1, -30, 65, 2, "cubic", "none", "census", INF), (130, 130, 1, -30, 65, 4, "linear", "none", "census", INF),
    (67, 80, 1, 3, 33, 2, "cubic", "none", "ad", INF), (64, 50, 3, 3, 33, 4, "cubic", "none", "ad", 40.0),
    (5, 5, 1, -1, 2, 2, "linear", "none", "sd", INF), (1, 1, 1, 0, 1, 4, "cubic", "none", "sd", INF),
    (64, 64, 1, -20, 33, 2, "cubic", "sobelx", "ad", INF), (67, 67, 1, -20, 33, 4, "cubic", "sobelx", "sd", 5000.0),
    (67, 67, 1, -8, 17, 2, "cubic", "none", "ncc", INF), (64, 64, 1, -8, 17, 4, "linear", "none", "ncc", INF),
    (130, 130, 1, -8, 17, 2, "cubic", "none", "btad", INF), (67, 67, 1, 1, 3, 4, "cubic", "none", "btad", 20.0),
    (130, 130, 3, -40, 64, 2, "linear", "none", "ad", INF), (130, 130, 1, 10, 2, 4, "cubic", "none", "census", INF),
    (64, 64, 1, 60, 5, 2, "cubic", "none", "census", INF), (64, 64, 1, -66, 5, 4, "cubic", "none", "ad", INF),   # pixels outside v for every label: zeros
    (5, 5, 1, -128, 257, 4, "cubic", "none", "census", INF),                                                  # 1025 labels: beyond the fast kernels
    (5, 5, 1, -128, 257, 2, "cubic", "none", "census", INF),                                                  # 513 labels from a padded phase
]


@pytest.mark.parametrize("case", VOLUMES, ids=lambda c: "%dx%d_%dch_d%d_L%d_s%d_%s_%s_%s_%g" % c)
def test_fine_volume(ctx, oracle, case):
    nx, vnx, nch, dmin, L, s, interp, pre, dist, trunc = case
    u, v = pair(nx, 3, vnx, nch)
    dmax = dmin + L - 1
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    F = ctx.costvolume_subpix_dev(du, dv, dmin, dmax, s, interp, pre, dist, trunc, 5)
    assert F.dims == (nx, 3, s * dmin, s * dmax)
    want = M.fine_volume(oracle, u, v, dmin, dmax, s, interp, pre, dist, trunc, 5)
    assert M.same_bits(F.download(), want)
    if (dmin, L) in ((60, 5), (-66, 5)):
        assert (want[:, 8:56] == 0).all() and np.isfinite(want).any()
    for o in (F, du, dv):
        o.free()


def test_s1_is_the_ordinary_build(ctx, oracle):
    u, v = pair(67, 3)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    for dist in ("census", "ad"):
        F = ctx.costvolume_subpix_dev(du, dv, -9, 5, 1, "linear", "none", dist, INF, 5)
        assert F.dims == (67, 3, -9, 5) and M.same_bits(F.download(), oracle.costvolume(u, v, -9, 5, "none", dist, np.inf, 5))
        F.free()
    du.free(), dv.free()


# ---- the form F is left in -------------------------------------------------------------------------------------------------------
AGG = dict(P1=3.0, P2=24.0, NDIR=8, MGM=2, use_fh=1)


def maps(ctx, cv, refine="vfit"):
    _, o, c = ctx.aggregate_dev(cv, AGG["P1"], AGG["P2"], AGG["NDIR"], AGG["MGM"], AGG["use_fh"], 1, refine=refine)
    r = o.download()[0], c.download()[0]
    o.free(), c.free()
    return r


@pytest.mark.parametrize("L,s", [(33, 2), (33, 4), (64, 2), (65, 4), (129, 2)])   # L' = 65, 129, 127, 257, 257: never a multiple of 64, so F's codes are the padded copy; the phases' are both kinds
def test_census_volume_takes_the_kernels_of_a_direct_build(ctx, oracle, L, s):
    nx, ny, dmin = 67, 8, -L + 3
    dmax = dmin + L - 1
    Lf = s * (L - 1) + 1
    u, v = pair(nx, ny)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    F = ctx.costvolume_subpix_dev(du, dv, dmin, dmax, s, "cubic", "none", "census", INF, 5)
    got = maps(ctx, F)
    took = ctx.last_pass_kernel()
    # an ordinary census volume of the same nx, ny and label count, on a v wide enough for its range
    uw, vw = pair(nx, ny, nx + Lf)
    dvw = ctx.upload_image(vw)
    D = ctx.costvolume_dev(du, dvw, 0, Lf - 1, "none", "census", INF, 5)
    maps(ctx, D)
    assert took == ctx.last_pass_kernel() and "k_pass" in took
    # ... and the maps are those of the model's F, uploaded as fp32
    Fm = M.fine_volume(oracle, u, v, dmin, dmax, s, "cubic", "none", "census", np.inf, 5)
    up = ctx.upload_volume(Fm, s * dmin)
    want = maps(ctx, up)
    assert M.same_bits(got[0], want[0]) and M.same_bits(got[1], want[1])
    assert M.same_bits(F.download(), Fm)                                 # (the stale fp32 copy is made from the codes on demand)
    for o in (F, D, up, du, dv, dvw):
        o.free()


@pytest.mark.parametrize("s", [2, 4])
def test_ad_volume_of_integer_and_fractional_phases(ctx, oracle, s):
    """phase 0 of an 8-bit pair holds whole numbers (the builder keeps it as codes), the other phases do not: F is fp32"""
    nx, ny, dmin, dmax = 67, 8, -40, -8
    u, v = pair(nx, ny)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    F = ctx.costvolume_subpix_dev(du, dv, dmin, dmax, s, "cubic", "none", "ad", INF, 3)
    Fm = M.fine_volume(oracle, u, v, dmin, dmax, s, "cubic", "none", "ad", np.inf, 3)
    assert (Fm[:, :, ::s] == np.rint(Fm[:, :, ::s])).all() and not (Fm[:, :, 1::s] == np.rint(Fm[:, :, 1::s])).all()
    got = maps(ctx, F)
    up = ctx.upload_volume(Fm, s * dmin)
    want = maps(ctx, up)
    assert M.same_bits(got[0], want[0]) and M.same_bits(got[1], want[1]) and M.same_bits(F.download(), Fm)
    for o in (F, up, du, dv):
        o.free()


# ---- refill and reuse ------------------------------------------------------------------------------------------------------------
def test_refill_other_geometry_trim(oracle):
    def chain(c, steps):
        res = []
        F = None
        for kind, (nx, seed, dmin, dmax, s, dist) in steps:
            u, v = pair(nx, 6, seed=seed)
            du, dv = c.upload_image(u), c.upload_image(v)
            if kind == "trim":
                c.trim()
            if kind == "plain":   # the context's ordinary build + aggregation
                cv = c.costvolume_dev(du, dv, dmin, dmax, "none", dist, INF, 5)
                res.append(maps(c, cv) + (cv.download(),))
                cv.free()
            else:
                into = F if kind == "refill" else None
                G = c.costvolume_subpix_dev(du, dv, dmin, dmax, s, "cubic", "none", dist, INF, 5, into=into)
                res.append(maps(c, G) + (G.download(),))
                if kind != "refill" and F is not None:
                    F.free()
                F = G
            du.free(), dv.free()
        if F is not None:
            F.free()
        return res

    a, b = (67, 1, -20, 12, 2, "census"), (67, 2, -20, 12, 2, "census")
    other, ad = (40, 3, -5, 3, 4, "census"), (67, 4, -20, 12, 2, "ad")
    plain = (67, 5, -30, 1, 1, "census")
    steps = [("plain", plain), ("new", a), ("refill", b), ("new", other), ("new", ad), ("refill", a), ("trim", b), ("plain", plain)]
    with mgm_amd.Context(0) as c:
        got = chain(c, steps)
    assert all(M.same_bits(x, y) for x, y in zip(got[0], got[-1]))      # the ordinary path: the same bits before and after
    for (kind, st), g in zip(steps, got):
        with mgm_amd.Context(0) as fresh:
            want = chain(fresh, [("plain" if kind == "plain" else "new", st)])[0]
        assert all(M.same_bits(x, y) for x, y in zip(g, want)), (kind, st)
    nx, seed, dmin, dmax, s, dist = b
    u, v = pair(nx, 6, seed=seed)
    assert M.same_bits(got[2][2], M.fine_volume(oracle, u, v, dmin, dmax, s, "cubic", "none", dist, np.inf, 5))


# ---- the rescale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 4])
def test_rescale(ctx, s):
    m = np.array([[np.nan, np.inf, -np.inf, -0.0, 0.0, 3.0, -7.25, 1e-45, 2.5e-45, 3e38, -1e-38, 511.0]], np.float32)
    m = np.tile(m, (3, 30))[None]
    d = ctx.upload_image(m)
    out = ctx.subpix_scale_dev(d, s)
    want = M.scale(m, s)
    assert M.same_bits(out.download(), want) and M.same_bits(d.download(), m)
    assert ctx.subpix_scale_dev(d, s, out=d) is d and M.same_bits(d.download(), want)   # in place
    assert np.signbit(want[0, 0, 3]) and np.isnan(want[0, 0, 0])
    out.free(), d.free()


# ---- Context.pair_subpix ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_pair():
    return synth.stereo_pair(48, 16, -8, 0)[:2]


@pytest.mark.parametrize("s,use_fh,refine", [(2, 0, "none"), (2, 1, "vfit"), (4, 1, "none"), (4, 0, "vfit")])
def test_pair_subpix(ctx, oracle, small_pair, s, use_fh, refine):
    u, v = small_pair
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    kw = dict(P1=4.0, P2=20.0, NDIR=4, TSGM=2, use_fh=use_fh, refine=refine, tau=1.0)
    res = ctx.pair_subpix(du, dv, -8, 0, s, "cubic", prefilter="none", distance="census", truncDist=INF, census_win=5, **kw)
    want = M.pair(oracle, post, u, v, -8, 0, s, "cubic", kw["P1"], kw["P2"], 4, 2, use_fh, 1, refine, 1.0, distance="census", census_win=5)
    for g, w, name in zip(res, want, ("checked", "left", "right", "cost")):
        assert M.same_bits(g.download()[0], w), name
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any()
    frac = want[1][np.isfinite(want[1])] * s
    assert refine != "none" or (frac == np.rint(frac)).all() and (want[1] != np.rint(want[1])).any()   # fine labels, in pixels
    for o in res + (du, dv):
        o.free()


# ---- error paths -----------------------------------------------------------------------------------------------------------------
def test_error_paths(ctx):
    u, v = pair(20, 4)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    d3 = ctx.upload_image(np.zeros((3, 4, 20), np.float32))
    other = ctx.new_image(21, 4)

    def refused(fn, *a, **kw):
        with pytest.raises(mgm_amd.MgmError) as e:
            fn(*a, **kw)
        assert e.value.code == mgm_amd.MGM_ERR_INVALID, e.value

    for s in (0, 3, 8, -2):
        refused(ctx.subpix_phase_dev, dv, s, 0)
        refused(ctx.costvolume_subpix_dev, du, dv, -3, 0, s)
        refused(ctx.subpix_scale_dev, dv, s)
    for s, k in ((1, 1), (2, 2), (4, 4), (2, -1)):
        refused(ctx.subpix_phase_dev, dv, s, k)
    for interp in ("nearest", "", None, "Cubic"):
        refused(ctx.subpix_phase_dev, dv, 2, 1, interp)
        refused(ctx.costvolume_subpix_dev, du, dv, -3, 0, 2, interp)
    refused(ctx.costvolume_subpix_dev, du, dv, 1, 0, 2)                  # dmax < dmin
    refused(ctx.costvolume_subpix_dev, du, d3, -3, 0, 2)                 # channel counts
    refused(ctx.subpix_phase_dev, dv, 2, 1, "cubic", into=other)        # an image of another geometry, and v itself
    refused(ctx.subpix_phase_dev, dv, 2, 1, "cubic", into=dv)
    refused(ctx.subpix_scale_dev, dv, 2, out=other)
    F = ctx.costvolume_subpix_dev(du, dv, -3, 0, 2, "cubic", "none", "census", INF, 5)
    refused(ctx.costvolume_subpix_dev, du, dv, -3, 0, 4, "cubic", "none", "census", INF, 5, into=F)   # F has s = 2's labels
    refused(ctx.costvolume_subpix_dev, du, dv, -4, 0, 2, "cubic", "none", "census", INF, 5, into=F)
    refused(ctx.costvolume_subpix_dev, du, dv, -3, 0, 2, "cubic", "none", "census", INF, 1)   # the ordinary build's own refusal (no window)
    # the context and F are as they were
    G = ctx.costvolume_subpix_dev(du, dv, -3, 0, 2, "cubic", "none", "census", INF, 5)
    assert M.same_bits(F.download(), G.download())
    for o in (F, G, du, dv, d3, other):
        o.free()


# ---- the command line ------------------------------------------------------------------------------------------------------------
NEW_KERNELS = ("k_subpix_phase", "k_cv_interleave", "k_scale_map")
CLI = dict(nx=96, ny=40, dmin=-8, dmax=0)


def run_cli(args, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("MGM_SUBPIX")}
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


@pytest.fixture(scope="module")
def cli_pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("subpixcli")
    u, v, _ = synth.stereo_pair(CLI["nx"], CLI["ny"], CLI["dmin"], CLI["dmax"])
    fu, fv = str(d / "u.png"), str(d / "v.png")
    write_png(fu, u[0]), write_png(fv, v[0])
    args = ["-r", str(CLI["dmin"]), "-R", str(CLI["dmax"]), "-s", "vfit", "-t", "census", "-O", "8"]

    def run(tag, env, extra=()):
        f = {k: str(d / ("%s_%s.tif" % (tag, k))) for k in ("out", "cost", "nolr")}
        r = run_cli(args + list(extra) + ["-l", f["nolr"], fu, fv, f["out"], f["cost"]], dict(env, MGM_HIP_KERNELS="1"))
        return r, ({k: read_tif(f[k]) for k in f} if r.returncode == 0 else None)
    return u, v, run


def kernels_of(r):
    return [l for l in r.stderr.splitlines() if l.startswith("[mgm kernels]")][0].split()


@pytest.mark.parametrize("s", [2, 4])
def test_command_line_matches_the_model_chain(oracle, cli_pair, s):
    u, v, run = cli_pair
    r, m = run("s%d" % s, dict(MGM_SUBPIX=str(s)))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["%d %d" % (CLI["dmin"], CLI["dmax"]), "01234567", "01234567"]   # stdout stays what it is
    # the defaults of the command line: P1 8, P2 32, TSGM 4, Hirschmueller's potentials, CENSUS_NCC_WIN 3, tau 1, no median
    chk, left, _, cost = M.pair(oracle, post, u, v, CLI["dmin"], CLI["dmax"], s, "cubic", 8.0, 32.0, 8, 4, 0, 1, "vfit", 1.0,
                                distance="census", census_win=3)
    assert M.same_bits(m["out"], chk) and M.same_bits(m["nolr"], left) and M.same_bits(m["cost"], cost)
    k = kernels_of(r)
    assert k.count("k_cv_interleave") == 2 and k.count("k_scale_map") == 2 and k.count("k_subpix_phase") == 2 * (s - 1)
    if s == 2:   # MGM_SUBPIX_INTERP: another volume, the model's again
        r2, m2 = run("s2lin", dict(MGM_SUBPIX="2", MGM_SUBPIX_INTERP="linear"))
        lin = M.pair(oracle, post, u, v, CLI["dmin"], CLI["dmax"], 2, "linear", 8.0, 32.0, 8, 4, 0, 1, "vfit", 1.0, distance="census", census_win=3)
        assert r2.returncode == 0 and M.same_bits(m2["out"], lin[0]) and not M.same_bits(lin[0], chk)
        # ... and with MGM_SPECKLE and MGM_FILL_HOLES=median: those models on the model's map, everything in pixels
        r3, m3 = run("s2post", dict(MGM_SUBPIX="2", MGM_SPECKLE="30", MGM_FILL_HOLES="median"))
        want = fill(speckle(chk, 30, 1.0)[0], "median", 8, 0)[0]
        assert r3.returncode == 0 and M.same_bits(m3["out"], want) and not M.same_bits(want, chk)
        assert M.same_bits(m3["nolr"], left) and r3.stdout == r.stdout


def test_command_line_off_is_the_program_as_it_was(cli_pair):
    _, _, run = cli_pair
    r0, m0 = run("unset", {})
    r1, m1 = run("one", dict(MGM_SUBPIX="1", MGM_SUBPIX_INTERP="linear"))
    assert r0.returncode == 0 and r1.returncode == 0 and r0.stdout == r1.stdout
    for k in m0:
        assert np.array_equal(m0[k].view(np.uint32), m1[k].view(np.uint32)), k
    for r in (r0, r1):
        assert not set(kernels_of(r)) & set(NEW_KERNELS)
    assert kernels_of(r0) == kernels_of(r1)


def test_command_line_refusals(cli_pair):
    _, _, run = cli_pair
    cases = [(dict(MGM_SUBPIX="2"), ["-m", "lo.tif", "-M", "hi.tif"], "range images (-m/-M)"), (dict(MGM_SUBPIX="4"), ["-S", "2"], "-S > 1"),
             (dict(MGM_SUBPIX="2", TSGM_ITER="2"), [], "TSGM_ITER != 1"), (dict(MGM_SUBPIX="2", TSGM_ITER="0"), [], "TSGM_ITER != 1"),
             (dict(MGM_SUBPIX="2", MGM_RIGHT_FROM_LEFT="1"), [], "MGM_RIGHT_FROM_LEFT=1"),
             (dict(MGM_SUBPIX="4", MGM_DEVICES="0,1"), [], "several MGM_DEVICES")]
    for n, (env, extra, why) in enumerate(cases):
        r, _ = run("refused%d" % n, env, extra)
        assert r.returncode == 2 and "mgm: MGM_SUBPIX does not combine with %s\n" % why in r.stderr, (env, extra, r.stderr)
    for bad in ("3", "0", "8", "2.0", "two", "", "-2"):
        r, _ = run("bad", dict(MGM_SUBPIX=bad))
        assert r.returncode == 2 and "MGM_SUBPIX must be" in r.stderr, bad
    r, _ = run("badinterp", dict(MGM_SUBPIX="2", MGM_SUBPIX_INTERP="nearest"))
    assert r.returncode == 2 and "MGM_SUBPIX_INTERP must be" in r.stderr
    help_text = run_cli(["--help"], {}).stdout
    assert "MGM_SUBPIX=1" in help_text and "MGM_SUBPIX_INTERP=cubic" in help_text
