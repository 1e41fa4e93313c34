"""The pruned winner search as a pipeline (k_wta_pruned, mgm_amd/csrc/mgm_wta.hip): a wave asks for the costs and minima of its next turn
before it searches the current one, and the lane that brings a pixel's winner keeps S at the two labels beside it instead of reading them
again.  What that can get wrong is the prologue, the steady state and the drain of the turns -- waves that run 0, 1, 2, 3 and 5 of them --
and the neighbour bookkeeping: a winner at the first or last label of its chunk (its neighbour comes from memory), at label 0 or 255 (no
refinement), beside a chunk of +INF, in a pixel without any finite label.  Every case: the maps bit for bit against the oracle's, without
refinement and with vfit, and against the same call under MGM_HIP_WTA_PRUNE=0; the two counters against the emulation's (pixels, chunks)
EXACTLY (tests/wta_prune_model.py)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_wta_pruned_instances as T
import wta_group_inputs as G
import wta_prune_model as M
from helpers import ndiff

pytestmark = pytest.mark.gpu
ROOT = T.ROOT


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return T.Planner(tmp_path_factory.mktemp("wta_pipeline"))


# ---- turns per wave: MGM_HIP_TUNE is read once per process, so one fresh child process per setting ------------------------------------
# With wta_prune_wg=1 the grid is one workgroup per CU: 256 x 4 waves x 16 pixels = 16 384 pixels per turn of the grid (8 192 with one
# group of eight pixels per wave).  7 x 1: one wave runs one turn, its three neighbours none.  131 x 127 = 16 637: some waves two turns,
# the others one (three and two at 8 192).  257 x 129 = 33 153 = 1 mod 16: three and two (five and four).  Under the default switches the
# grid holds every pixel in one turn.
SIZES = [(7, 1), (131, 127), (257, 129)]
ROWS = [  # name, potentials, NDIR: k_wta_pruned<., 8, true>, <., 4, true> and -- 5 passes -- the body of <1, 8, false>
    ("fh8", G.FH, 8),
    ("hi4", G.HI, 4),
    ("hi5", G.HI, 5),
]
REFINES = ["vfit", None]
# (the default of wta_prune_ppw is 1: the instances with two groups of pixels per wave are asked for by name)
SETTINGS = {"default": "", "wg1": "wta_prune_wg=1", "wg1_ppw1": "wta_prune_wg=1,wta_prune_ppw=1", "ppw2": "wta_prune_ppw=2",
            "wg1_ppw2": "wta_prune_wg=1,wta_prune_ppw=2"}

SCRIPT = r"""
import os, sys, hashlib, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import mgm_amd
import wta_group_inputs as G
import wta_prune_model as M
def words(a):  # bytes to digest: NaN is NaN whatever its sign and payload, every other float its own bits
    a = np.array(a, np.float32, copy=True)
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a).tobytes()
ctx = mgm_amd.Context(0)
ctx.timing(True)
for nx, ny in %r:
    C = M.ramp_volume(nx, ny, 256, G.SEED)
    for name, (FH, P1, P2), NDIR in %r:
        for refine in %r:
            got = {}
            for prune in ("1", "0"):
                os.environ["MGM_HIP_WTA_PRUNE"] = prune
                cv = ctx.upload_volume(C, M.RAMP_DMIN)
                ctx.timing_reset()
                _, o, c = ctx.aggregate_dev(cv, P1, P2, NDIR, G.MGM, FH, 1, None, refine)
                ran = [n for n, _ in ctx.timings()]
                assert "k_wta" in ran, ran
                got[prune] = (ctx.wta_stats(), words(o.download()[0]), words(c.download()[0]))
                for x in (o, c, cv):
                    x.free()
            (px, ch), label, cost = got["1"]
            assert got["0"][0] == (0, 0), "MGM_HIP_WTA_PRUNE=0 must take the plain search"
            same = label == got["0"][1] and cost == got["0"][2]
            print("RAN", "%%dx%%d" %% (nx, ny), name, refine, px, ch, int(same), hashlib.sha256(label + cost).hexdigest())
ctx.close()
""" % (ROOT, os.path.join(ROOT, "tests"), SIZES, ROWS, REFINES)


@pytest.mark.parametrize("key", list(SETTINGS))
def test_turns_per_wave(oracle, planner, key):
    env = dict(os.environ, MGM_HIP_TUNE=SETTINGS[key])
    r = subprocess.run([sys.executable, "-c", SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "RAN":
            got[tuple(w[1:4])] = (int(w[4]), int(w[5]), int(w[6]), w[7])
    for nx, ny in SIZES:
        for name, pot, NDIR in ROWS:
            ref = G.reference(oracle, "ramp", nx, ny, pot, NDIR)
            for refine in REFINES:
                what = "%s %dx%d %s %s" % (key, nx, ny, name, refine)
                assert planner.pruned(nx, ny, 1, NDIR, G.MGM, pot[0], refine), "%s: the planner does not prune this launch" % what
                k = ("%dx%d" % (nx, ny), name, str(refine))
                assert k in got, "%s did not run:\n%s" % (what, r.stdout[-2000:])
                px, ch, same, digest = got[k]
                h = hashlib.sha256(T.words(ref["vout"] if refine else ref["out"]) + T.words(ref["voutc"] if refine else ref["outc"]))
                print("%s: counters (%d, %d), emulation (%d, %d)" % (what, px, ch, nx * ny, ref["chunks"]))
                assert (px, ch) == (nx * ny, ref["chunks"]), "%s: counters (%d, %d), emulation (%d, %d)" % (what, px, ch, nx * ny, ref["chunks"])
                assert digest == h.hexdigest(), "%s: the maps differ from the oracle's" % what
                assert same == 1, "%s: the maps differ from the plain search's" % what


# ---- the neighbour bookkeeping ------------------------------------------------------------------------------------------------------
def reference_of(oracle, C, pot, NDIR):
    """What T.check compares with: the oracle's maps without refinement and with vfit, its Lr, the emulation's chunk count."""
    S, out, outc, lr = oracle.mgm(C, M.RAMP_DMIN, pot[1], pot[2], NDIR, G.MGM, pot[0], 1, dump_lr=True)
    vout, voutc = oracle.refine(S, M.RAMP_DMIN, "vfit", out, outc)
    return dict(C=C, lr=lr, out=out, outc=outc, vout=vout, voutc=voutc, chunks=M.pruned_search(C, lr, M.RAMP_DMIN, 1)[2])


def check_volume(ctx, planner, ref, pot, NDIR, refine, what):
    ny, nx, L = ref["C"].shape
    assert planner.pruned(nx, ny, 1, NDIR, G.MGM, pot[0], refine), "%s: the planner does not prune this launch" % what
    cv = ctx.upload_volume(ref["C"], M.RAMP_DMIN)
    try:
        T.check(ctx, [ref], [cv], pot[1], pot[2], NDIR, G.MGM, pot[0], 1, refine, True, what)
    finally:
        cv.free()


@pytest.mark.parametrize("pot,NDIR", [(G.HI, 8), (G.FH, 8), (G.HI, 4), (G.HI, 5)], ids=["hi8", "fh8", "hi4", "hi5"])
def test_winners_at_chunk_edges_and_range_ends(ctx, oracle, planner, pot, NDIR):
    """Labels 31 and 32: S beside the winner lies in the next chunk, loaded or not -- the fetch from memory.  Labels 0 and 255: the gate
    b - 1 >= 0, b + 2 <= 255 keeps vfit out, the map holds the integer label and S."""
    C, where = M.planted_volume(256)
    ref = reference_of(oracle, C, pot, NDIR)
    for label in (0, 31, 32, 255):
        at = where == label
        assert (ref["out"][at] == label + M.RAMP_DMIN).mean() > 0.9, "the planted label %d does not win" % label
    moved = ref["vout"] != ref["out"]
    assert moved[(where == 31) | (where == 32)].any(), "vfit moves no winner at a chunk edge: the case does not reach the fetch"
    ends = (ref["out"] == M.RAMP_DMIN) | (ref["out"] == M.RAMP_DMIN + 255)
    assert ends.sum() > 0.4 * ends.size and not moved[ends].any()
    check_volume(ctx, planner, ref, pot, NDIR, "vfit", "planted NDIR %d FH %d" % (NDIR, pot[0]))


@pytest.mark.parametrize("pot,NDIR", [(G.FH, 8), (G.HI, 4)], ids=["fh8", "hi4"])
def test_winner_beside_a_chunk_of_inf(ctx, oracle, planner, pot, NDIR):
    """ramp_volume's +INF chunks: where the winner is the first or last label of its chunk and the chunk beside it is +INF throughout,
    that chunk is never loaded and the value vfit takes from it is not finite."""
    ref = G.reference(oracle, "ramp", 61, 19, pot, NDIR)
    C = ref["C"]
    dead = np.isinf(C).reshape(19, 61, 8, 32).all(axis=3)
    b = (ref["out"] - M.RAMP_DMIN).astype(np.int64)
    ch = b // 32
    beside = np.where(b % 32 == 0, ch - 1, np.where(b % 32 == 31, ch + 1, -1))
    hit = (beside >= 0) & (beside < 8) & np.take_along_axis(dead, np.clip(beside, 0, 7)[..., None], axis=2)[..., 0]
    print("ramp 61x19 NDIR %d: %d chunks of +INF, %d winners at a chunk edge, %d of them beside a chunk of +INF" % (NDIR, int(dead.sum()), int((beside >= 0).sum()), int(hit.sum())))
    assert dead.sum() >= 61 * 19 // 20 and (beside >= 0).sum() >= 20
    check_volume(ctx, planner, ref, pot, NDIR, "vfit", "ramp 61x19 NDIR %d vfit" % NDIR)


def test_pixel_without_a_finite_label(ctx, oracle):
    """dead_pixel_volume: no winner, so no lane brought one -- the group's first lane writes NaN and +INF.  Behind the dead pixel Lr is
    NaN along every scan line; the counters are held to the emulation on the DEVICE's Lr and minima, as in
    test_gpu_wta_pruned_instances.test_one_pixel_without_a_finite_label."""
    C1 = M.dead_pixel_volume()
    ny, nx, L = C1.shape
    S, out, outc, lr = oracle.mgm(C1, M.RAMP_DMIN, 8.0, 32.0, 8, 1, 0, 1, dump_lr=True)
    vout, voutc = oracle.refine(S, M.RAMP_DMIN, "vfit", out, outc)
    assert np.isnan(out).any()
    cv = ctx.upload_volume(C1, M.RAMP_DMIN)
    try:
        for refine, eo, ec in (("vfit", vout, voutc), (None, out, outc)):
            maps1, lr1, lmin1, (px, ch), names1 = T.run(ctx, [cv], 8.0, 32.0, 8, 1, 0, 1, refine, True)
            maps0, lr0, lmin0, stats0, names0 = T.run(ctx, [cv], 8.0, 32.0, 8, 1, 0, 1, refine, False)
            assert ndiff(maps1[0][0], eo) == 0 and ndiff(maps1[0][1], ec) == 0
            assert ndiff(maps1[0][0], maps0[0][0]) == 0 and ndiff(maps1[0][1], maps0[0][1]) == 0
            assert stats0 == (0, 0) and lmin0 is None
            if lmin1 is not None:  # searched pruned
                emu = M.pruned_search(C1, np.stack(lr1), M.RAMP_DMIN, 1, minima=np.stack(lmin1[0]))[2]
                print("dead pixel %s: counters (%d, %d), emulation on the device's Lr and minima %d" % (refine, px, ch, emu))
                assert (px, ch) == (nx * ny, emu)
            else:                  # the refusal of the pruned path
                assert (px, ch) == (0, 0)
    finally:
        cv.free()
