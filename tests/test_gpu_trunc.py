"""Special truncation values (truncDist = +INF, 0, -0, -3, 2.5, NaN) on every fill path, against the oracle, bit for bit.

The reference clips every cost with MIN_(e, truncDist) (mgm_costvolume.h:16, 401-412): a truncDist of -0 makes EVERY cost
-0 (a bit count or a difference is never below -0), a negative one makes every cost negative, a NaN one makes every cost
NaN -- and then no hypothesis is finite, so the pixel's costs are all 0 (414-421).  The fast fill paths take truncDist only
where the result has their form (whole numbers 0..254, a clear sign bit); everything else must take the general kernel and
keep the reference's words.  The range-proportional copy of a ragged volume holds non-negative costs only: a -0 must keep
the volume on its dense hull (k_rel_gather), not become +0 and not stall the hand-off tags.

Checked per case: the downloaded volume (uniform: oracle.costvolume, ragged: oracle.costvolume_ranged) and one aggregation
for each of NDIR 1 / 8 x fix 0 / 1 (labels where the cost is finite, costs everywhere)."""
import math
import os

import numpy as np
import pytest

import mgm_amd
from helpers import labels_equal, ndiff
from mgm_amd import synth
from oracle.oracle import int_ranges

pytestmark = pytest.mark.gpu

TRUNCS = [float("inf"), 0.0, -0.0, -3.0, 2.5, float("nan")]
# (prefilter, distance, channels, census window)
COSTS = {
    "census1": ("none", "census", 1, 5),     # one descriptor word: the compact / range-proportional fills
    "census2": ("none", "census", 1, 7),     # 48 bits: two words, fp32 costs (thirds / halves never arise: whole bit counts)
    "census3c": ("none", "census", 3, 5),    # colour: three words, averaged over the channels
    "ad": ("none", "ad", 1, 3),
    "ad3": ("none", "ad", 3, 3),
    "sd": ("none", "sd", 1, 3),
    "sd3": ("none", "sd", 3, 3),
    "sobel_ad": ("sobelx", "ad", 1, 3),
    "ncc": ("none", "ncc", 1, 3),
    "btad": ("none", "btad", 1, 3),
}
NX, NY = 64, 40


def tname(t):
    return "nan" if math.isnan(t) else ("-0" if t == 0 and math.copysign(1, t) < 0 else str(t))


def case_images(cost, L):
    pre, dist, nch, win = COSTS[cost]
    dmin = -(L * 3 // 4)
    dmax = dmin + L - 1
    u, v, gt = synth.stereo_pair(NX, NY, dmin * 3 // 4, max(0, dmax * 3 // 4), seed=L + nch, nch=nch)
    return pre, dist, win, dmin, dmax, u, v, gt


@pytest.mark.parametrize("L", [128, 151])
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
@pytest.mark.parametrize("cost", list(COSTS))
def test_truncation_values_on_every_fill_path(ctx, oracle, cost, ragged, L):
    pre, dist, win, dmin, dmax, u, v, gt = case_images(cost, L)
    if ragged:
        rng = np.random.default_rng(L)
        lo = np.clip(gt - 12 + rng.integers(-3, 4, gt.shape), dmin, dmax).astype(np.float32)
        hi = np.clip(gt + 14 + rng.integers(-3, 4, gt.shape), dmin, dmax).astype(np.float32)
        hi = np.maximum(hi, lo)
        ilo, ihi = int_ranges(lo, hi)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    dlo, dhi = (ctx.upload_image(lo[None]), ctx.upload_image(hi[None])) if ragged else (None, None)
    bad = []
    os.environ["MGM_HIP_REL"] = "2"  # (the range-proportional kernels wherever the volume has such a copy)
    try:
        for t in TRUNCS:
            if ragged:
                cv = ctx.costvolume_ranged_dev(du, dv, dlo, dhi, dmin, dmax, pre, dist, t, win)
                Ca = oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, pre, dist, t, win)
            else:
                cv = ctx.costvolume_dev(du, dv, dmin, dmax, pre, dist, t, win)
                Ca = oracle.costvolume(u, v, dmin, dmax, pre, dist, t, win)
            n = ndiff(cv.download(), Ca)
            if n:
                bad.append((tname(t), "volume", n))
            for NDIR, fix in ((1, 0), (1, 1), (8, 0), (8, 1)):
                P1, P2, MGM, FH = (8.0, 32.0, 3, 0) if fix else (2.0, 20.0, 3, 1)
                _, o, c = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, FH, fix, None, None)
                if ragged:
                    _, oa, ca = oracle.mgm_ranged(Ca, dmin, ilo, ihi, P1, P2, NDIR, MGM, FH, fix, want_S=False)
                else:
                    _, oa, ca = oracle.mgm(Ca, dmin, P1, P2, NDIR, MGM, FH, fix)
                go, gc = o.download()[0], c.download()[0]
                if ndiff(gc, ca) or not labels_equal(go, oa, ca):
                    bad.append((tname(t), NDIR, fix, ndiff(gc, ca), ndiff(go, oa)))
                o.free(), c.free()
            cv.free()
    finally:
        os.environ.pop("MGM_HIP_REL", None)
        for h in (du, dv, dlo, dhi):
            if h is not None:
                h.free()
    assert not bad, (cost, ragged, L, bad)


def test_truncation_refill_keeps_the_format_honest(ctx, oracle):
    """One handle refilled through the special values in turn (a -0 fill after a compact one, a compact one after a -0 fill ...):
    the volume's compact / padded / range-proportional state must follow each fill."""
    for L, ragged in ((128, False), (151, False), (128, True)):
        pre, dist, win, dmin, dmax, u, v, gt = case_images("census1", L)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        lo = np.clip(gt - 10, dmin, dmax).astype(np.float32)
        hi = np.clip(gt + 10, dmin, dmax).astype(np.float32)
        ilo, ihi = int_ranges(lo, hi)
        dlo, dhi = ctx.upload_image(lo[None]), ctx.upload_image(hi[None])
        cv = None
        for t in (float("inf"), -0.0, 3.0, -0.0, 0.0, float("nan"), -0.0, float("inf")):
            if ragged:
                cv = ctx.costvolume_ranged_dev(du, dv, dlo, dhi, dmin, dmax, pre, dist, t, win, into=cv)
                Ca = oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, pre, dist, t, win)
                _, oa, ca = oracle.mgm_ranged(Ca, dmin, ilo, ihi, 8.0, 32.0, 1, 3, 0, 0, want_S=False)
            else:
                cv = ctx.costvolume_dev(du, dv, dmin, dmax, pre, dist, t, win, into=cv)
                Ca = oracle.costvolume(u, v, dmin, dmax, pre, dist, t, win)
                _, oa, ca = oracle.mgm(Ca, dmin, 8.0, 32.0, 1, 3, 0, 0)
            _, o, c = ctx.aggregate_dev(cv, 8.0, 32.0, 1, 3, 0, 0, None, None)
            assert ndiff(c.download()[0], ca) == 0 and labels_equal(o.download()[0], oa, ca), (L, ragged, tname(t))
            assert ndiff(cv.download(), Ca) == 0, (L, ragged, tname(t))
            o.free(), c.free()
        for h in (cv, du, dv, dlo, dhi):
            h.free()


def test_debug_lr_refuses_a_volume_refilled_to_another_slot_count(oracle):
    """mgm_debug_download_lr on the range-proportional path reads the Lr volumes of the context's last aggregation through the
    volume's records and slot count: after the volume has been refilled (64 -> 128 slots per pixel, other windows) it must refuse
    (MGM_ERR_INVALID) rather than read the old launch at the new stride.  Before and after the refill it matches the oracle."""
    nx, ny, dmin, dmax = 90, 52, -150, 0
    u, v, gt = synth.stereo_pair(nx, ny, -110, 0, seed=404)
    P1, P2, NDIR, MGM, FH = 2.0, 30.0, 8, 3, 1
    os.environ["MGM_HIP_REL"] = "1"
    try:
        with mgm_amd.Context(0) as ctx:
            du, dv = ctx.upload_image(u), ctx.upload_image(v)
            cv = None
            for step, half in enumerate((12, 50, 12)):  # windows of ~25 labels (64 slots), ~101 (128 slots), ~25 again
                lo = np.clip(gt - half, dmin, dmax).astype(np.float32)
                hi = np.clip(gt + half, dmin, dmax).astype(np.float32)
                ilo, ihi = int_ranges(lo, hi)
                cv = ctx.costvolume_ranged_dev(du, dv, ctx.upload_image(lo[None]), ctx.upload_image(hi[None]), dmin, dmax, "none", "census",
                                               float("inf"), 5, into=cv)
                if step:  # the context's last aggregation ran on this handle's previous contents
                    with pytest.raises(mgm_amd.MgmError) as e:
                        ctx.debug_lr(cv, 0)
                    assert e.value.code == mgm_amd.MGM_ERR_INVALID, (step, e.value)
                ctx.timing(True)
                ctx.timing_reset()
                _, o, c = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, FH, 1, None, None)
                assert "k_pass_rel" in [n for n, _ in ctx.timings()], step
                ctx.timing(False)
                Ca = oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, "none", "census", np.inf, 5)
                _, oa, ca, lra = oracle.mgm_ranged(Ca, dmin, ilo, ihi, P1, P2, NDIR, MGM, FH, 1, want_S=False, dump_lr=(0, NDIR - 1))
                assert ndiff(c.download()[0], ca) == 0 and labels_equal(o.download()[0], oa, ca), step
                own = (dmin + np.arange(dmax - dmin + 1))[None, None, :]
                own = (own >= ilo[..., None]) & (own <= ihi[..., None])
                for n, p in enumerate((0, NDIR - 1)):
                    lr = ctx.debug_lr(cv, p)
                    assert int(np.sum((lr.view(np.uint32) != lra[n].view(np.uint32)) & own)) == 0, (step, p)
    finally:
        os.environ.pop("MGM_HIP_REL", None)
