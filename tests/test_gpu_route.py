"""Which kernels take an aggregation call: one table of calls, one per route the host code can decide on (mgm_planner.h:
plan_agg_route, plan_subbatch, plan_dense_kernels; the drivers in mgm_api.hip and mgm_plan.hip).  Every row is held to the
oracle AND to the ordered list of kernels the call launched -- probes (k_weight_values, k_compact, k_pad, ...) included -- as
recorded for that row on the commit before the route planners existed (5fa7fa3): the planners ask for the same facts in the same
order and end at the same kernels.  A fresh context per row, so that a list does not depend on what ran before it."""
import os

import numpy as np
import pytest

import mgm_amd
from helpers import labels_equal, ndiff
from mgm_amd import synth
from oracle.oracle import int_ranges, usable_cpus

pytestmark = pytest.mark.gpu

NX, NY = 150, 110  # (several bands in both axes: tests/test_gpu_plan_caches.py)


def uploaded(L, nb=1, nan=False, nx=NX, ny=NY, dmin=-40):
    def make(ctx, oracle):
        Cs = [synth.raw_volume(nx, ny, L, seed=900 + L + k, inf_frac=0.01) for k in range(nb)]
        if nan:
            Cs[0][7, 11, 3] = np.nan
            Cs[0][12, 5, :] = np.nan
        return [ctx.upload_volume(C, dmin) for C in Cs], [(C, dmin, None, None) for C in Cs], None
    return make


def colour_ad(dmin, dmax):
    def make(ctx, oracle):
        u, v, _ = synth.stereo_pair(NX, NY, dmin * 3 // 4, max(0, dmax * 3 // 4), seed=77, nch=3)
        cv = ctx.costvolume_dev(ctx.upload_image(u), ctx.upload_image(v), dmin, dmax, "none", "ad", float("inf"), 3)
        return [cv], [(oracle.costvolume(u, v, dmin, dmax, "none", "ad", np.inf, 3), dmin, None, None)], u
    return make


def ragged(dmin, dmax, width, nb=1, cost="census", nx=NX, ny=NY):
    """Windows of exactly `width` labels around the true disparity in a hull of [dmin, dmax] that every volume of a batch shares."""
    def make(ctx, oracle):
        cvs, hosts, u0 = [], [], None
        for k in range(nb):
            u, v, gt = synth.stereo_pair(nx, ny, dmin * 3 // 4, 0, seed=300 + 7 * k + width)
            rng = np.random.default_rng(40 + k)
            lo = np.clip(gt - width // 2 + rng.integers(-2, 3, size=gt.shape), dmin, dmax - width + 1).astype(np.float32)
            hi = (lo + width - 1).astype(np.float32)
            lo[0, 0], hi[0, 0] = dmin, dmin + width - 1
            lo[0, 1], hi[0, 1] = dmax - width + 1, dmax
            ilo, ihi = int_ranges(lo, hi)
            cvs.append(ctx.costvolume(u, v, lo, hi, "none", cost, float("inf"), 5))
            hosts.append((oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, "none", cost, np.inf, 5), dmin, ilo, ihi))
            u0 = u if u0 is None else u0
        return cvs, hosts, u0
    return make


# name, volumes, (P1, P2, NDIR, MGM, FH), weights (None / "image": 1 and one other value / "three"), refinement, MGM_HIP_REL,
# workspace limit in volumes' worth of Lr (0: none)
ROWS = [
    ("l64_second_build", uploaded(64), (8.0, 32.0, 8, 3, 0), None, "vfit", None, 0),
    ("l128_second_build_fh", uploaded(128), (2.0, 20.0, 8, 1, 1), None, "vfit", None, 0),
    ("l100_padded_one_byte", uploaded(100), (8.0, 32.0, 8, 3, 0), None, "vfit", None, 0),
    ("l151_ad_padded_two_bytes", colour_ad(-120, 30), (24.0, 96.0, 8, 3, 0), None, "vfit", None, 0),
    ("negative_p1_first_build", uploaded(64), (-2.0, 32.0, 8, 3, 0), None, "vfit", None, 0),
    ("nan_cost_exact", uploaded(64, nan=True), (8.0, 32.0, 8, 3, 0), None, None, None, 0),
    ("ragged_p2_inf_exact", ragged(-60, 0, 21), (8.0, float("inf"), 4, 3, 0), None, None, None, 0),
    ("ragged_rel_fh", ragged(-60, 0, 21), (2.0, 30.0, 8, 3, 1), None, "vfit", None, 0),
    ("ragged_rel_weighted", ragged(-60, 0, 21), (8.0, 32.0, 8, 3, 0), "three", "vfit", None, 0),
    ("ragged_rel_batch_of_two", ragged(-60, 0, 21, nb=2), (8.0, 32.0, 8, 3, 0), None, "vfit", None, 0),
    ("ragged_t2_fh_128_fp32_slots_dense_hull", ragged(-200, 10, 100, cost="ncc"), (2.0, 40.0, 8, 2, 1), None, "vfit", None, 0),
    ("two_valued_weights_w2", uploaded(128), (8.0, 32.0, 8, 3, 0), "image", "vfit", None, 0),
    ("batch_of_three_workspace_for_two", uploaded(128, nb=3), (8.0, 32.0, 8, 3, 0), None, "vfit", None, 2.6),
    ("l2049_exact", uploaded(2049, nx=24, ny=16, dmin=-2000), (8.0, 32.0, 4, 3, 0), None, "vfit", None, 0),
]

# The kernels of each row's call, in launch order, as the parent commit (5fa7fa3) ran them on an MI355X: recorded once with
# run_row() below on that commit's library (docs/experiments.md, "route planners").
PARENT_KERNELS = {
    "l64_second_build": ["k_compact", "k_pass2", "k_wta"],
    "l128_second_build_fh": ["k_compact", "k_pass2", "k_wta"],
    "l100_padded_one_byte": ["k_nanscan", "k_pad", "k_pass2", "k_wta"],
    "l151_ad_padded_two_bytes": ["k_pass2", "k_wta"],  # (the padded two-byte copy is the one the cost kernel wrote: nothing to pad)
    "negative_p1_first_build": ["k_compact", "k_pass", "k_wta"],
    "nan_cost_exact": ["k_compact", "k_pass_exact", "k_wta"],
    "ragged_p2_inf_exact": ["k_expand", "k_pass_exact", "k_wta"],
    "ragged_rel_fh": ["k_pass_rel", "k_wta"],
    "ragged_rel_weighted": ["k_pass_rel", "k_wta"],
    "ragged_rel_batch_of_two": ["k_pass_rel", "k_wta", "k_wta"],
    # (the pad tries in order: one byte, two bytes, fp32 -- NCC costs fit neither compact form)
    "ragged_t2_fh_128_fp32_slots_dense_hull": ["k_rel_gather", "k_pad", "k_pad", "k_pad", "k_pass2", "k_wta", "k_refine"],
    "two_valued_weights_w2": ["k_compact", "k_pass2", "k_wta"],
    "batch_of_three_workspace_for_two": ["k_compact", "k_compact", "k_pass2", "k_wta", "k_wta", "k_compact", "k_pass2", "k_wta"],
    "l2049_exact": ["k_pass_exact", "k_wta"],
}


def run_row(ctx, oracle, row):
    """-> (kernel names in launch order, [(volume, words of the cost map that differ, labels equal)])"""
    name, make, (P1, P2, NDIR, MGM, FH), wkind, refine, rel, limit = row
    if rel is not None:
        os.environ["MGM_HIP_REL"] = rel
    try:
        cvs, hosts, u = make(ctx, oracle)
        nx, ny = cvs[0].dims[:2]
        w8 = w8h = None
        if wkind == "image":
            w8 = ctx.weights_dev(ctx.upload_image(u if u is not None else synth.stereo_pair(nx, ny, -40, 0, seed=61)[0]), 4.0, 12.0)
            w8h = w8.download()
        elif wkind == "three":
            w8h = np.random.default_rng(3).choice(np.array([1.0, 2.5, 4.0], np.float32), size=(8, ny, nx), p=[0.6, 0.25, 0.15])
            w8 = ctx.upload_image(w8h)
        if limit:
            L = cvs[0].dims[3] - cvs[0].dims[2] + 1
            ctx.set_workspace_limit(int(limit * 4 * nx * ny * L * NDIR))
        ctx.synchronize()
        ctx.timing(True)
        ctx.timing_reset()
        _, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, FH, 1, [w8] * len(cvs) if w8 is not None else None, refine)
        ctx.synchronize()
        ran = [n for n, _ in ctx.timings()]
        ctx.timing(False)
        ctx.set_workspace_limit(0)
    finally:
        os.environ.pop("MGM_HIP_REL", None)
    oracle.set_threads(min(16, usable_cpus()))
    try:
        res = []
        for k, (C, dmin, lo, hi) in enumerate(hosts):
            if lo is None:
                S, o, c = oracle.mgm(C, dmin, P1, P2, NDIR, MGM, FH, 1, w8h)
                ro, rc = oracle.refine(S, dmin, refine, o, c) if refine else (o, c)
            else:
                S, o, c = oracle.mgm_ranged(C, dmin, lo, hi, P1, P2, NDIR, MGM, FH, 1, w8h)
                ro, rc = oracle.refine_ranged(S, dmin, lo, hi, refine, o, c) if refine else (o, c)
            go, gc = outs[k].download()[0], outcs[k].download()[0]
            res.append((k, ndiff(gc, rc), labels_equal(go, ro, rc)))
    finally:
        oracle.set_threads(1)
    return ran, res


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r[0])
def test_route_and_kernels(oracle, row):
    with mgm_amd.Context(0) as ctx:
        ran, res = run_row(ctx, oracle, row)
    print(row[0], ran)
    assert all(d == 0 and same for _, d, same in res), (row[0], res)
    assert ran == PARENT_KERNELS[row[0]], (row[0], ran)
