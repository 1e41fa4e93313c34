"""The pruned winner search with a pixel on eight lanes and eight pixels per wave (k_wta_pruned, mgm_amd/csrc/mgm_wta.hip) on what that
layout can get wrong: launches of a group, a wave and a workgroup of pixels exactly, one short and one over; neighbouring pixels that
load one chunk and eight (the rounds of step (c) and the lanes that sit them out); ties between chunks that arrive out of label order;
the instances a tuning switch selects.  Every case asserts what tests/test_gpu_wta_pruned_instances.py asserts (its `check`): the maps
against the oracle and against the same call under MGM_HIP_WTA_PRUNE=0, the minima, the counters against the emulation's chunk count
EXACTLY, `k_wta` in the timing table -- and that the planner harness says the launch prunes.  What the inputs are worth is measured on
the CPU in tests/test_wta_groups.py."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_wta_pruned_instances as T
import wta_group_inputs as G
import wta_prune_model as M

pytestmark = pytest.mark.gpu
ROOT = T.ROOT


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return T.Planner(tmp_path_factory.mktemp("wta_groups"))


def run_case(ctx, planner, refs, pot, NDIR, refine, what):
    """`refs`: one reference (wta_group_inputs.reference) per volume of the batch."""
    ny, nx, L = refs[0]["C"].shape
    FH, P1, P2 = pot
    assert planner.pruned(nx, ny, len(refs), NDIR, G.MGM, FH, refine), "%s: the planner does not prune this launch" % what
    cvs = [ctx.upload_volume(r["C"], M.RAMP_DMIN) for r in refs]
    try:
        T.check(ctx, refs, cvs, P1, P2, NDIR, G.MGM, FH, 1, refine, True, what)
    finally:
        for h in cvs:
            h.free()


# pixels: 7, 8, 9 -- one group of eight short, exact, over; 16 -- what a wave takes per turn with two groups per lane group;
# 63, 64, 65 -- a workgroup's four waves at that width, short, exact, over; 129 -- two such workgroups and one pixel
SHAPES = [(7, 1), (8, 1), (9, 1), (4, 4), (9, 7), (8, 8), (13, 5), (43, 3)]


@pytest.mark.parametrize("pot,NDIR,refine", [(G.FH, 8, "vfit"), (G.HI, 4, None)], ids=["fh8_vfit", "hi4_none"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_launch_shape(ctx, oracle, planner, shape, pot, NDIR, refine):
    nx, ny = shape
    r = G.reference(oracle, "ramp", nx, ny, pot, NDIR)
    run_case(ctx, planner, [r], pot, NDIR, refine, "ramp %dx%d NDIR %d %s" % (nx, ny, NDIR, refine))


@pytest.mark.parametrize("refine", ["vfit", None], ids=["vfit", "none"])
@pytest.mark.parametrize("name", sorted(G.GROUP_CASES))
def test_group_case(ctx, oracle, planner, name, refine):
    gen, nx, ny, pot, NDIR, floor = G.GROUP_CASES[name]
    run_case(ctx, planner, [G.case_reference(oracle, name)], pot, NDIR, refine, "%s %s" % (name, refine))


@pytest.mark.parametrize("refine", ["vfit", None], ids=["vfit", "none"])
@pytest.mark.parametrize("pot,NDIR", [(G.FH, 6), (G.HI, 2)], ids=["fh6", "hi2"])
def test_mixed_on_the_instances_for_any_pass_count(ctx, oracle, planner, pot, NDIR, refine):
    """k_wta_pruned<1, 8, false> and <1, 4, false>: NDIR is a run-time value."""
    r = G.reference(oracle, "mixed", 33, 17, pot, NDIR)
    assert not np.isnan(r["out"]).any()
    run_case(ctx, planner, [r], pot, NDIR, refine, "mixed 33x17 NDIR %d %s" % (NDIR, refine))


def test_batch_of_two_periodic_volumes(ctx, oracle, planner):
    refs = [G.reference(oracle, "periodic", 33, 17, G.HI, 4, seed=s) for s in (7, 8)]
    run_case(ctx, planner, refs, G.HI, 4, "vfit", "periodic 33x17 x2 NDIR 4 vfit")


# ---- the instances a switch selects: MGM_HIP_TUNE is read once per process, so one fresh child process per setting ----------------
CHILD_CASES = [  # name, generator, nx, ny, potentials, NDIR, refinement
    ("mixed", "mixed", 33, 17, G.FH, 8, "vfit"),
    ("periodic", "periodic", 33, 17, G.HI, 4, None),
    ("ramp13x5", "ramp", 13, 5, G.FH, 8, "vfit"),
    # 16637 pixels: with wta_prune_wg=1 the grid is one workgroup per CU, 256 x 4 waves x 16 pixels = 16384 per turn of the
    # grid-stride loop, so the second turn runs (under wta_prune_ppw=1 alone the grid covers every pixel in one turn)
    ("ramp131x127", "ramp", 131, 127, G.HI, 4, "vfit"),
]
SCRIPT = r"""
import sys, hashlib, numpy as np
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
for name, gen, nx, ny, (FH, P1, P2), NDIR, refine in %r:
    C = G.GENERATORS[gen](nx, ny, G.SEED) if gen in G.GENERATORS else M.ramp_volume(nx, ny, 256, G.SEED)
    cv = ctx.upload_volume(C, M.RAMP_DMIN)
    ctx.timing_reset()
    _, o, c = ctx.aggregate_dev(cv, P1, P2, NDIR, G.MGM, FH, 1, None, refine)
    px, ch = ctx.wta_stats()
    ran = [n for n, _ in ctx.timings()]
    assert "k_wta" in ran and "k_pass2" in ran, ran
    h = hashlib.sha256()
    h.update(words(o.download()[0]))
    h.update(words(c.download()[0]))
    print("RAN", name, px, ch, h.hexdigest())
    for x in (o, c, cv):
        x.free()
ctx.close()
""" % (ROOT, os.path.join(ROOT, "tests"), CHILD_CASES)


@pytest.mark.parametrize("tune", ["wta_prune_ppw=1", "wta_prune_wg=1"])
def test_tuning_switch(oracle, planner, tune):
    env = dict(os.environ, MGM_HIP_TUNE=tune, MGM_HIP_WTA_PRUNE="1")
    r = subprocess.run([sys.executable, "-c", SCRIPT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "RAN":
            got[w[1]] = (int(w[2]), int(w[3]), w[4])
    assert sorted(got) == sorted(c[0] for c in CHILD_CASES), r.stdout[-2000:]
    for name, gen, nx, ny, pot, NDIR, refine in CHILD_CASES:
        assert planner.pruned(nx, ny, 1, NDIR, G.MGM, pot[0], refine), "%s: the planner does not prune this launch" % name
        ref = G.reference(oracle, gen, nx, ny, pot, NDIR)
        h = hashlib.sha256()
        h.update(T.words(ref["vout"] if refine else ref["out"]))
        h.update(T.words(ref["voutc"] if refine else ref["outc"]))
        print("%s %s: %s, emulation (%d, %d)" % (tune, name, got[name][:2], nx * ny, ref["chunks"]))
        assert got[name][:2] == (nx * ny, ref["chunks"]), "%s %s: counters %s, emulation (%d, %d)" % (tune, name, got[name][:2], nx * ny, ref["chunks"])
        assert got[name][2] == h.hexdigest(), "%s %s: the maps differ from the oracle's" % (tune, name)
