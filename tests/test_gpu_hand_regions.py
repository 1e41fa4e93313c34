"""The two regions of self-validating hand-off slots (mgm_ctx::hand, mgm_ctx::hand_rel) across launches of one context, every step
bit for bit against the oracle: the dense region's per-pass tags when the passes are launched together, alone and one by one; both
regions across a trim.  The tags' state machine itself is tested on the host (tests/test_hand_tags.py); here the launches really
hand slabs from band to band -- MGM_HIP_TUNE=show_plan=1 shows 120 tasks for the eight passes of the dense shape (11 for pass 2
alone) and 102 / 96 for the range-proportional one (Hirschmueller / FH), several bands per pass -- so a tag handed out wrongly
validates a stale slab and changes the result.
The dense cases run with MGM_HIP_CHECK_TAGS=1: after every launch the library scans the slots of the launched passes for the tag."""
import numpy as np
import pytest

import mgm_amd
from helpers import labels_equal, ndiff
from mgm_amd import synth
from oracle.oracle import int_ranges, usable_cpus

pytestmark = pytest.mark.gpu

P1, P2, MGM = 8.0, 32.0, 3


@pytest.fixture(scope="module")
def dense(oracle):
    """One context, one volume of 160x130x128, and the oracle's eight Lr volumes and refined maps of it (Hirschmueller, TSGM 3)."""
    C = synth.raw_volume(160, 130, 128, seed=7)
    oracle.set_threads(min(16, usable_cpus()))
    try:
        S, o, c, lr = oracle.mgm(C, 0, P1, P2, 8, MGM, 0, 1, None, dump_lr=True)
        ro, rc = oracle.refine(S, 0, "vfit", o, c)
    finally:
        oracle.set_threads(1)
    with mgm_amd.Context(0) as ctx:
        cv = ctx.upload_volume(C, 0)
        yield ctx, cv, lr, ro, rc
        cv.free()


def test_dense_tags_of_passes_launched_together_alone_and_one_by_one(dense, monkeypatch):
    ctx, cv, lr, _, _ = dense
    monkeypatch.setenv("MGM_HIP_CHECK_TAGS", "1")
    ctx.aggregate_passes_at_dev(cv, P1, P2, MGM, 0, 0, 8, 0, 8, 8)
    for k in (2, 2, 5, 5, 2):  # passes 2 and 5 alone, twice each; pass 2 once more: from here on its tag is not the other passes'
        ctx.aggregate_passes_at_dev(cv, P1, P2, MGM, 0, k, 1, k, 8, 8)
    for k in range(8):
        ctx.aggregate_passes_at_dev(cv, P1, P2, MGM, 0, k, 1, k, 8, 8)
    for k in range(8):
        assert ndiff(ctx.debug_lr(cv, k), lr[k]) == 0, ("one by one", k)
    ctx.aggregate_passes_at_dev(cv, P1, P2, MGM, 0, 0, 8, 0, 8, 8)
    for k in range(8):
        assert ndiff(ctx.debug_lr(cv, k), lr[k]) == 0, ("together", k)


def test_dense_region_across_a_trim(dense, monkeypatch):
    ctx, cv, _, ro, rc = dense
    monkeypatch.setenv("MGM_HIP_CHECK_TAGS", "1")
    for step in ("before", "after"):
        _, out, outc = ctx.aggregate_dev(cv, P1, P2, 8, MGM, 0, 1, None, "vfit")
        go, gc = out.download()[0], outc.download()[0]
        out.free(), outc.free()
        assert ndiff(gc, rc) == 0 and labels_equal(go, ro, rc), (step, ndiff(gc, rc), ndiff(go, ro))
        ctx.trim()


def test_rel_region_across_potentials_and_a_trim(oracle, monkeypatch):
    """150x110, a hull of 128 labels, windows of 49: Hirschmueller, FH (another layout: the region is cleared), a trim, Hirschmueller
    (the first layout again, on a new buffer) -- each against the ragged oracle."""
    monkeypatch.setenv("MGM_HIP_REL", "2")
    nx, ny, dmin, dmax = 150, 110, -127, 0
    u, v, gt = synth.stereo_pair(nx, ny, -95, 0, seed=41)
    lo, hi = np.clip(gt - 24, dmin, dmax).astype(np.float32), np.clip(gt + 24, dmin, dmax).astype(np.float32)
    a, b = np.unravel_index(gt.argmin(), gt.shape), np.unravel_index(gt.argmax(), gt.shape)
    lo[a], hi[a], lo[b], hi[b] = dmin, dmin + 48, dmax - 48, dmax  # (the hull is all 128 labels)
    ilo, ihi = int_ranges(lo, hi)
    assert int((ihi - ilo).max()) + 1 == 49 and (int(ilo.min()), int(ihi.max())) == (dmin, dmax)
    Ca = oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, "none", "census", np.inf, 5)
    oracle.set_threads(min(16, usable_cpus()))
    try:
        want = {}
        for FH, p1 in ((0, 8.0), (1, 2.0)):
            S, o, c = oracle.mgm_ranged(Ca, dmin, ilo, ihi, p1, 30.0, 8, MGM, FH, 1)
            want[FH] = (p1,) + tuple(oracle.refine_ranged(S, dmin, ilo, ihi, "vfit", o, c))
    finally:
        oracle.set_threads(1)
    with mgm_amd.Context(0) as ctx:
        cv = ctx.costvolume(u, v, lo, hi, "none", "census", float("inf"), 5)
        for step, FH in enumerate((0, 1, None, 0)):
            if FH is None:
                ctx.trim()
                continue
            p1, ro, rc = want[FH]
            ctx.timing(True)
            ctx.timing_reset()
            _, out, outc = ctx.aggregate_dev(cv, p1, 30.0, 8, MGM, FH, 1, None, "vfit")
            ran = [n for n, _ in ctx.timings()]
            ctx.timing(False)
            assert "k_pass_rel" in ran, (step, ran)
            go, gc = out.download()[0], outc.download()[0]
            out.free(), outc.free()
            assert ndiff(gc, rc) == 0 and labels_equal(go, ro, rc), (step, FH, ndiff(gc, rc), ndiff(go, ro))
