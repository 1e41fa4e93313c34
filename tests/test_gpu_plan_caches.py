"""The planner's per-context caches, one fixed A, B, A, B sequence each on ONE context, every step against the oracle.

A context keeps four objects from launch to launch (mgm_amd/csrc/mgm_plan.hip), each keyed by the VALUE it was made from
(mgm_amd/csrc/mgm_planner.h):
  * the dense hand-off region with its per-pass sign-bit tags (run_passes): cleared whenever the plan's `HandLayout` -- per
    laid-out pass the base, bands, slot lines and slope, the floats per slot, the volume groups, the band height -- differs from
    the one the region was last written for;
  * the dense plans and task tables, up to 24 of them (`dense_plans`: the bytes of the `DenseRequest`, i.e. everything
    `plan_dense` reads -> the plan and its table on the device; the oldest is dropped);
  * the range-proportional hand-off region (run_rel, the `HandLayout` of the `RelPlan`);
  * the range-proportional plans and task tables, up to 24 (`rel_plans`, the bytes of the `RelRequest`).
A and B below share the shape and the batch size but differ in what
the cached object is built from -- the update function, FH / Hirschmueller (the exchanged-role walk), TSGM 3 / 4 (slope 1
or 2), one / two / four bytes per cost (whether the anti-diagonal bands fit the LDS), 64 / 128 slots, weights.  A key that
missed one of them would hand B the object A left behind; where the key does name everything, the sequence pins it against
later edits."""
import os

import numpy as np
import pytest

import mgm_amd
from helpers import labels_equal, ndiff
from mgm_amd import synth
from oracle.oracle import int_ranges

pytestmark = pytest.mark.gpu


def threads(oracle, n=16):
    from oracle.oracle import usable_cpus
    oracle.set_threads(min(n, usable_cpus()))


def dense_step(ctx, oracle, cvs, Cs, dmin, P1, P2, NDIR, MGM, FH, w8=None, w8h=None, names=None):
    ctx.timing(True)
    ctx.timing_reset()
    _, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, FH, 1, [w8] * len(cvs) if w8 is not None else None, "vfit")
    ran = [n for n, _ in ctx.timings()]
    ctx.timing(False)
    bad = []
    for k, C in enumerate(Cs):
        S, o, c = oracle.mgm(C, dmin, P1, P2, NDIR, MGM, FH, 1, w8h)
        ro, rc = oracle.refine(S, dmin, "vfit", o, c)
        go, gc = outs[k].download()[0], outcs[k].download()[0]
        if ndiff(gc, rc) or not labels_equal(go, ro, rc):
            bad.append((k, ndiff(gc, rc), ndiff(go, ro)))
        outs[k].free(), outcs[k].free()
    if names is not None:
        assert any(n in ran for n in names), ran
    return bad


def test_dense_hand_off_region_sequence(ctx, oracle):
    """The region is keyed on (shape, label slots, volume groups, passes laid out, band height, TSGM <= 3): Hirschmueller TSGM 3,
    FH TSGM 1 (other neighbours, other potentials) and the two-valued weights' kernels alternate on one region; the tags of
    each pass must keep alternating correctly across all of them."""
    nx, ny, L, dmin = 150, 110, 128, -100
    Cs = [synth.raw_volume(nx, ny, L, seed=60 + k, inf_frac=0.01) for k in range(2)]
    cvs = [ctx.upload_volume(C, dmin) for C in Cs]
    u = synth.stereo_pair(nx, ny, -40, 0, seed=61)[0]
    du = ctx.upload_image(u)
    w2 = ctx.weights_dev(du, 4.0, 12.0)  # (1 and one other value: the W2 kernels)
    w2h = oracle.weights(u, 4.0, 12.0)
    steps = [(8.0, 32.0, 8, 3, 0, None), (2.0, 20.0, 8, 1, 1, None), (8.0, 32.0, 8, 3, 0, "w2")]
    threads(oracle)
    try:
        for rep in range(2):
            for P1, P2, NDIR, MGM, FH, wk in steps:
                bad = dense_step(ctx, oracle, cvs, Cs, dmin, P1, P2, NDIR, MGM, FH, w2 if wk else None, w2h if wk else None, names=("k_pass2",))
                assert not bad, (rep, P1, P2, MGM, FH, wk, bad)
    finally:
        oracle.set_threads(1)
        for h in cvs + [du, w2]:
            h.free()


def test_dense_task_table_sequence(ctx, oracle):
    """One shape, tables for one and for two volumes, all eight passes and four, label counts that pick other wave sharing /
    workgroups per CU -- alternated, every table fetched back from the cache at least once."""
    nx, ny, dmin = 140, 96, -40
    vols = {L: [synth.raw_volume(nx, ny, L, seed=L + k) for k in range(2)] for L in (64, 256)}
    cvs = {L: [ctx.upload_volume(C, dmin) for C in vols[L]] for L in vols}
    steps = [(64, 1, 8, 3, 0), (256, 2, 8, 3, 1), (64, 2, 4, 3, 0), (256, 1, 8, 4, 0)]
    threads(oracle)
    try:
        for rep in range(2):
            for L, nb, NDIR, MGM, FH in steps:
                bad = dense_step(ctx, oracle, cvs[L][:nb], vols[L][:nb], dmin, 8.0, 32.0, NDIR, MGM, FH)
                assert not bad, (rep, L, nb, NDIR, MGM, FH, bad)
    finally:
        oracle.set_threads(1)
        for hs in cvs.values():
            for h in hs:
                h.free()


def test_dense_task_table_tsgm_3_and_4_alternate(ctx, oracle):
    """TSGM 3 and 4 on one shape, batch and occupancy: the form-0 passes walk slope 1 or 2, which the simulated schedule is made
    of -- each request has a plan of its own, fetched back on the second round."""
    nx, ny, L, dmin = 140, 96, 64, -40
    C = synth.raw_volume(nx, ny, L, seed=71)
    cv = ctx.upload_volume(C, dmin)
    threads(oracle)
    try:
        for rep in range(2):
            for MGM in (3, 4):
                bad = dense_step(ctx, oracle, [cv], [C], dmin, 8.0, 32.0, 8, MGM, 0, names=("k_pass2",))
                assert not bad, (rep, MGM, bad)
    finally:
        oracle.set_threads(1)
        cv.free()


def test_dense_task_table_unweighted_and_general_weights_alternate(ctx, oracle):
    """The same launch without weights and with a three-valued weight image (the general weighted kernels: progress words, no
    queues, another hand-off lag in the simulated schedule), alternated."""
    nx, ny, L, dmin = 140, 96, 64, -40
    C = synth.raw_volume(nx, ny, L, seed=72)
    cv = ctx.upload_volume(C, dmin)
    u = synth.stereo_pair(nx, ny, -30, 0, seed=73)[0]
    du = ctx.upload_image(u)
    w3 = ctx.weights_dev(du, 4.0, 12.0)
    w3h = w3.download()
    third = 2.5
    assert third not in np.unique(w3h)
    w3h[3, 20:50, 30:90] = third  # (1, the weights' other value and a third: not the two-valued kernels)
    w3.update(w3h)
    threads(oracle)
    try:
        for rep in range(2):
            for w8, w8h in ((None, None), (w3, w3h)):
                bad = dense_step(ctx, oracle, [cv], [C], dmin, 8.0, 32.0, 8, 3, 0, w8, w8h, names=("k_pass2",))
                assert not bad, (rep, w8 is not None, bad)
    finally:
        oracle.set_threads(1)
        for h in (cv, du, w3):
            h.free()


def test_dense_task_table_cache_evicts_and_returns(ctx, oracle):
    """More than 24 distinct dense plans (the cache's bound) on one context, then the first again: the evicted table is built
    anew, never read from a freed buffer or from a neighbour's entry."""
    ny, L, dmin = 36, 64, -20
    shapes = [40 + 3 * k for k in range(26)] + [40, 43, 118]
    threads(oracle)
    try:
        for nx in shapes:
            C = synth.raw_volume(nx, ny, L, seed=nx, inf_frac=0.01)
            cv = ctx.upload_volume(C, dmin)
            bad = dense_step(ctx, oracle, [cv], [C], dmin, 8.0, 32.0, 4, 3, 0)
            cv.free()
            assert not bad, (nx, bad)
    finally:
        oracle.set_threads(1)


def ragged_volume(ctx, oracle, nx, ny, dmin, dmax, half, seed, cost="census", nch=1):
    u, v, gt = synth.stereo_pair(nx, ny, dmin * 3 // 4, 0, seed=seed, nch=nch)
    rng = np.random.default_rng(seed)
    lo = np.clip(gt - half + rng.integers(-2, 3, gt.shape), dmin, dmax).astype(np.float32)
    hi = np.clip(gt + half + rng.integers(-2, 3, gt.shape), dmin, dmax).astype(np.float32)
    lo[0, 0], hi[0, 1] = dmin, dmax  # (batched volumes share their hull)
    ilo, ihi = int_ranges(lo, hi)
    win = 5 if cost == "census" else 3
    cv = ctx.costvolume(u, v, lo, hi, "none", cost, float("inf"), win)
    Ca = oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, "none", cost, np.inf, win)
    return cv, (Ca, ilo, ihi)


def rel_step(ctx, oracle, cvs, hosts, dmin, P1, P2, NDIR, MGM, FH):
    ctx.timing(True)
    ctx.timing_reset()
    _, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, FH, 1, None, "vfit")
    ran = [n for n, _ in ctx.timings()]
    ctx.timing(False)
    assert "k_pass_rel" in ran, ran
    bad = []
    for k, (Ca, lo, hi) in enumerate(hosts):
        S, o, c = oracle.mgm_ranged(Ca, dmin, lo, hi, P1, P2, NDIR, MGM, FH, 1)
        ro, rc = oracle.refine_ranged(S, dmin, lo, hi, "vfit", o, c)
        go, gc = outs[k].download()[0], outcs[k].download()[0]
        if ndiff(gc, rc) or not labels_equal(go, ro, rc):
            bad.append((k, ndiff(gc, rc), ndiff(go, ro)))
        outs[k].free(), outcs[k].free()
    return bad


# a landscape shape: the column passes have more lines than pixels per line (FH walks them with exchanged roles)
REL_SHAPE = (150, 60, -120, 0)


@pytest.fixture
def rel_mode():
    os.environ["MGM_HIP_REL"] = "2"
    yield
    os.environ.pop("MGM_HIP_REL", None)


def rel_volumes(ctx, oracle):
    nx, ny, dmin, dmax = REL_SHAPE
    vols = {}
    for name, half, cost in (("c64", 10, "census"), ("c128", 45, "census"), ("ncc", 10, "ncc"), ("ad3", 10, "ad")):
        made = [ragged_volume(ctx, oracle, nx, ny, dmin, dmax, half, 500 + 7 * k + half, cost, 3 if cost == "ad" else 1) for k in range(2)]
        vols[name] = ([m[0] for m in made], [m[1] for m in made])
    return vols


def test_rel_hand_off_region_sequence(oracle, rel_mode):
    """The range-proportional hand-off region of one shape and batch size: FH (exchanged-role columns) and Hirschmueller, 64 and 128
    slots, one-byte census costs, two-byte colour differences and fp32 NCC costs (whether the anti-diagonal bands fit the LDS) --
    alternated on one context."""
    dmin = REL_SHAPE[2]
    threads(oracle)
    try:
        with mgm_amd.Context(0) as ctx:
            vols = rel_volumes(ctx, oracle)
            steps = [("c64", 1), ("c64", 0), ("c128", 1), ("ncc", 1), ("ad3", 0), ("c128", 0), ("ncc", 0), ("ad3", 1)]
            for rep in range(2):
                for name, FH in steps:
                    for nb in (1, 2):
                        cvs, hosts = vols[name]
                        bad = rel_step(ctx, oracle, cvs[:nb], hosts[:nb], dmin, 2.0 if FH else 8.0, 30.0, 8, 3, FH)
                        assert not bad, (rep, name, FH, nb, bad)
    finally:
        oracle.set_threads(1)


def test_rel_task_table_sequence(oracle, rel_mode):
    """The range-proportional task table of one shape: TSGM 3 / 4 (slope 1 or 2 on the form-0 passes), four / eight passes, FH /
    Hirschmueller (the workgroups per CU of a single volume and the exchanged-role walk), one / two volumes -- alternated."""
    dmin = REL_SHAPE[2]
    threads(oracle)
    try:
        with mgm_amd.Context(0) as ctx:
            vols = rel_volumes(ctx, oracle)
            cvs, hosts = vols["c64"]
            steps = [(8, 3, 1, 1), (8, 4, 1, 1), (4, 3, 0, 1), (8, 3, 0, 2), (8, 4, 0, 1), (8, 3, 1, 2), (4, 4, 1, 2)]
            for rep in range(2):
                for NDIR, MGM, FH, nb in steps:
                    bad = rel_step(ctx, oracle, cvs[:nb], hosts[:nb], dmin, 2.0 if FH else 8.0, 30.0, NDIR, MGM, FH)
                    assert not bad, (rep, NDIR, MGM, FH, nb, bad)
    finally:
        oracle.set_threads(1)
