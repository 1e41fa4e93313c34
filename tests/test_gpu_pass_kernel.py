"""The pass kernel instance a launch runs, now chosen by the plan (PassKernelChoice, mgm_planner.h) and launched from a table:
one aggregation per row, a fresh context each, held to the oracle bit for bit (the NaN-cost row as tests/test_gpu_route.py holds
its own: the map's class is undefined in the reference there) AND to the instance the commit before the
choice moved (5df326f) launched for the same call, read back through mgm_debug_last_pass_kernel.

Families these rows reach: k_pass at 16 and at 4 lines per band; k_pass2 Hirschmueller and FH at 1, 4 and 12 labels per lane
with compact one-byte costs, deep rings, the per-XCD queues and the one-band build (and without queues at 40x20, which has
fewer than 32 work items), FH with TSGM 2 (no tags, shallow rings), the general weighted kernels, W2, two-byte costs, two and
four volumes per wave; k_pass_exact; k_pass_rel with the producer publishing E, weighted, FH with one, two (FH2) and three
min-convolutions, 128 slots, two-byte and fp32 cost codes.  Only the host sweep (tests/test_pass_kernel_plan.py) reaches the
rest: development builds (no queue and no W2 instances), two bands per CU (queue kernels that are not one-band builds), fp32
costs on the second build, shallow rings by switch, the one-after-the-other FH build of k_pass_rel (rel_multi=0)."""
import numpy as np
import pytest

import mgm_amd
from helpers import labels_equal, ndiff
from mgm_amd import synth
from oracle.oracle import usable_cpus
from test_gpu_route import colour_ad, ragged, uploaded

pytestmark = pytest.mark.gpu

WIDE = dict(nx=24, ny=16)  # the wide label counts
H, FH = (8.0, 32.0, 8, 3, 0), (2.0, 30.0, 8, 3, 1)

# name, volumes, (P1, P2, NDIR, MGM, FH), weights (None / "image": 1 and one other value / "three"); every row refines with vfit
# but the NaN-cost one, which is tests/test_gpu_route.py's row
ROWS = [
    ("first_build_l64", uploaded(64), (-2.0, 32.0, 8, 3, 0), None),
    ("first_build_l600_bands_of_four", uploaded(600, dmin=-500, **WIDE), (-2.0, 32.0, 8, 3, 0), None),
    ("second_h_l64", uploaded(64), H, None),
    ("second_h_l256", uploaded(256, dmin=-200), H, None),
    ("second_h_l768", uploaded(768, dmin=-700, **WIDE), H, None),
    ("second_fh_l64", uploaded(64), FH, None),
    ("second_fh_l256", uploaded(256, dmin=-200), FH, None),
    ("second_fh_l768", uploaded(768, dmin=-700, **WIDE), FH, None),
    ("second_fh_t2_no_tags", uploaded(128), (2.0, 30.0, 8, 2, 1), None),
    ("general_weights", uploaded(128), H, "three"),
    ("two_valued_weights_w2", uploaded(128), H, "image"),
    ("two_byte_costs_l151_padded", colour_ad(-120, 30), (24.0, 96.0, 8, 3, 0), None),
    ("subv2_four_of_l128", uploaded(128, nb=4), H, None),
    ("subv4_eight_of_l64", uploaded(64, nb=8), FH, None),
    ("no_queues_40x20_two_passes", uploaded(256, nx=40, ny=20, dmin=-200), (8.0, 32.0, 2, 3, 0), None),
    ("nan_cost_exact", uploaded(64, nan=True), H, None),
    ("rel_pube", ragged(-60, 0, 21), H, None),
    ("rel_weighted", ragged(-60, 0, 21), H, "three"),
    ("rel_fh_t1", ragged(-60, 0, 21), (2.0, 30.0, 8, 1, 1), None),
    ("rel_fh_t3", ragged(-60, 0, 21), FH, None),
    ("rel_fh2", ragged(-60, 0, 21), (2.0, 30.0, 8, 2, 1), None),
    ("rel_128_slots", ragged(-200, 10, 100), FH, None),
    ("rel_two_byte_costs", ragged(-60, 0, 21, cost="sd"), FH, None),
    ("rel_fp32_slots", ragged(-60, 0, 21, cost="ncc"), FH, None),
]

# The instance of each row's launch as the parent commit (5df326f) ran it on an MI355X: its library under one kernel trace
# (rocprofv3 --kernel-trace over a script that runs launch() for every row), the k_pass* names in launch order
# (docs/experiments.md, "pass kernel instance").  The parent's launch cascade restated (tests/pass_kernel_model.py) gives the same 24.
PARENT_INSTANCE = {
    "first_build_l64": "k_pass<1, false, false, 16>",
    "first_build_l600_bands_of_four": "k_pass<12, false, false, 4>",
    "second_h_l64": "k_pass2<1, false, false, 3, 1, 1, true, true, true, false>",
    "second_h_l256": "k_pass2<4, false, false, 3, 1, 1, true, true, true, false>",
    "second_h_l768": "k_pass2<12, false, false, 3, 1, 1, true, false, false, false>",  # (24x16: fewer than 32 work items, no queues)
    "second_fh_l64": "k_pass2<1, true, false, 3, 1, 1, true, true, true, false>",
    "second_fh_l256": "k_pass2<4, true, false, 3, 1, 1, true, true, true, false>",
    "second_fh_l768": "k_pass2<12, true, false, 3, 1, 1, true, false, false, false>",
    "second_fh_t2_no_tags": "k_pass2<2, true, false, 2, 1, 1, false, false, false, false>",
    "general_weights": "k_pass2<2, false, true, 3, 1, 1, false, false, false, false>",
    "two_valued_weights_w2": "k_pass2<2, false, false, 3, 1, 1, true, true, true, true>",
    "two_byte_costs_l151_padded": "k_pass2<3, false, false, 3, 2, 1, true, true, true, false>",
    "subv2_four_of_l128": "k_pass2<4, false, false, 3, 1, 2, true, false, false, false>",
    "subv4_eight_of_l64": "k_pass2<4, true, false, 3, 1, 4, true, false, false, false>",
    "no_queues_40x20_two_passes": "k_pass2<4, false, false, 3, 1, 1, true, false, false, false>",
    "nan_cost_exact": "k_pass_exact",
    "rel_pube": "k_pass_rel<false, true, 0, 4, 1, false>",
    "rel_weighted": "k_pass_rel<false, false, 0, 4, 1, false>",
    "rel_fh_t1": "k_pass_rel<true, false, 1, 4, 1, false>",
    "rel_fh_t3": "k_pass_rel<true, false, 3, 4, 1, false>",
    "rel_fh2": "k_pass_rel<true, false, 2, 4, 1, true>",
    "rel_128_slots": "k_pass_rel<true, false, 3, 8, 1, false>",
    "rel_two_byte_costs": "k_pass_rel<true, false, 3, 4, 2, false>",
    "rel_fp32_slots": "k_pass_rel<true, false, 3, 4, 4, false>",
}


def refine_of(row):
    return None if row[0] == "nan_cost_exact" else "vfit"


def launch(ctx, oracle, row):
    """The row's call -> (host volumes, host weights, output maps, kernel names of the timing table)"""
    name, make, (P1, P2, NDIR, MGM, fh), wkind = row
    cvs, hosts, u = make(ctx, oracle)
    nx, ny = cvs[0].dims[:2]
    w8 = w8h = None
    if wkind == "image":
        w8 = ctx.weights_dev(ctx.upload_image(u if u is not None else synth.stereo_pair(nx, ny, -40, 0, seed=61)[0]), 4.0, 12.0)
        w8h = w8.download()
    elif wkind == "three":
        w8h = np.random.default_rng(3).choice(np.array([1.0, 2.5, 4.0], np.float32), size=(8, ny, nx), p=[0.6, 0.25, 0.15])
        w8 = ctx.upload_image(w8h)
    ctx.synchronize()
    ctx.timing(True)
    ctx.timing_reset()
    _, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, fh, 1, [w8] * len(cvs) if w8 is not None else None, refine_of(row))
    ctx.synchronize()
    ran = [n for n, _ in ctx.timings()]
    ctx.timing(False)
    return hosts, w8h, [(o.download()[0], c.download()[0]) for o, c in zip(outs, outcs)], ran


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r[0])
def test_instance_and_maps(oracle, row):
    name, _, (P1, P2, NDIR, MGM, fh), _ = row
    with mgm_amd.Context(0) as ctx:
        hosts, w8h, maps, ran = launch(ctx, oracle, row)
        instance = ctx.last_pass_kernel()
    print(name, instance, ran)
    oracle.set_threads(min(16, usable_cpus()))
    try:
        for (C, dmin, lo, hi), (go, gc) in zip(hosts, maps):
            if lo is None:
                S, o, c = oracle.mgm(C, dmin, P1, P2, NDIR, MGM, fh, 1, w8h)
                ro, rc = oracle.refine(S, dmin, refine_of(row), o, c) if refine_of(row) else (o, c)
            else:
                S, o, c = oracle.mgm_ranged(C, dmin, lo, hi, P1, P2, NDIR, MGM, fh, 1, w8h)
                ro, rc = oracle.refine_ranged(S, dmin, lo, hi, "vfit", o, c)
            assert ndiff(gc, rc) == 0 and labels_equal(go, ro, rc), name
    finally:
        oracle.set_threads(1)
    assert instance == PARENT_INSTANCE[name], (name, instance)
    assert instance.split("<")[0] in ran, (name, instance, ran)  # the timing table lists the launch under its family's name
