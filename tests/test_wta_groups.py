"""What the inputs of tests/wta_group_inputs.py are worth, on the CPU (the oracle and the numpy emulation of the pruned search alone),
before tests/test_gpu_wta_groups.py relies on them: groups of eight consecutive pixels in which one pixel loads one or two chunks and
another seven or eight, and pixels whose smallest S ties across two loaded chunks with the winner BELOW the seed chunk.  And the
form of the chunk bound the kernel evaluates -- sum_fix of the minima at the chunk's largest finite cost -- against the fold over the
chunk's labels, bit for bit."""
import numpy as np
import pytest

import wta_group_inputs as G
import wta_prune_model as M
from helpers import ndiff


@pytest.mark.parametrize("name", sorted(G.GROUP_CASES))
def test_group_case_floor(oracle, name):
    """Found with seed 7, dmin -100, TSGM 3, fix 1:
      mixed 33x17     FH 2/20000 NDIR 8: 40 of 71 groups       Hirschmueller 8/32 NDIR 8: 41 of 71
      mixed 16x3      FH: 5 of 6                               Hirschmueller: 6 of 6
      periodic 33x17  Hirschmueller NDIR 8: 54 tied pixels, 30 with the winner below the seed      NDIR 4: 193 and 95
      periodic 16x3   Hirschmueller NDIR 8: 35 and 14"""
    gen, nx, ny, pot, NDIR, floor = G.GROUP_CASES[name]
    r = G.case_reference(oracle, name)
    assert not np.isnan(r["out"]).any(), "a pixel without a label"
    assert ndiff(r["Sm"], r["S"]) == 0
    assert ndiff(r["label"], r["out"]) == 0 and ndiff(r["cost"], r["outc"]) == 0
    assert ndiff(r["vlabel"], r["vout"]) == 0 and ndiff(r["vcost"], r["voutc"]) == 0
    fin = np.isfinite(r["C"])
    assert r["C"][fin].max() <= 133 and np.array_equal(r["C"][fin], np.rint(r["C"][fin])), "the compact path takes whole costs up to 254"
    if floor == "mixed":
        spread, groups = G.groups_spread(r["load"])
        print("%s: %d of %d groups hold a pixel loading >= 7 chunks and one loading <= 2; %.2f chunks per pixel" % (name, spread, groups, r["chunks"] / (nx * ny)))
        assert groups == (nx * ny + 7) // 8
        assert 4 * spread >= groups
    else:
        tied, below = G.ties_across_chunks(r)
        print("%s: %d pixels tie across two loaded chunks, %d of them with the winner's chunk below the seed; %.2f chunks per pixel" % (name, tied, below, r["chunks"] / (nx * ny)))
        assert tied >= 20 and below >= 10


BOUND_ROWS = ["r97_fh8_vfit", "r97_fh3_t4_frac_vfit", "r97_hi7_t1_frac_none", "r97_hi5_nofix_vfit", "p330_adt30_fh5_t4_vfit", "r97_hi1_vfit"]


def bound_forms_differ(C, lr, fix, LB=None):
    """Words in which the largest-finite-cost form of the chunk bound differs from the fold over the chunk's labels."""
    with np.errstate(invalid="ignore"):
        minima = M.chunk_minima(lr)
        LB = M.lower_bound(C, lr, fix, minima) if LB is None else LB
        return ndiff(G.chunk_bound_largest_cost(C, minima, fix), G.chunk_bound_fold(C, LB)), minima.shape[1] * minima.shape[2] * minima.shape[3]


@pytest.mark.parametrize("name", BOUND_ROWS)
def test_chunk_bound_at_the_largest_finite_cost_instance_rows(oracle, name):
    fix = M.INSTANCE_CASES[name][6]
    for r in M.case_reference(oracle, name):
        d, n = bound_forms_differ(r["C"], r["lr"], fix, r["LB"])
        print("%s: %d chunks, %d differ" % (name, n, d))
        assert d == 0


@pytest.mark.parametrize("name", sorted(G.GROUP_CASES))
def test_chunk_bound_at_the_largest_finite_cost_group_inputs(oracle, name):
    r = G.case_reference(oracle, name)
    assert bound_forms_differ(r["C"], r["lr"], 1, r["LB"])[0] == 0


def test_chunk_bound_at_the_largest_finite_cost_nan_minima(oracle):
    """dead_pixel_volume: minima that are NaN (INF - INF behind the dead pixel) -- both forms drop the bound to +INF."""
    C = M.dead_pixel_volume()
    S, out, outc, lr = oracle.mgm(C, M.RAMP_DMIN, 8.0, 32.0, 8, 1, 0, 1, dump_lr=True)
    with np.errstate(invalid="ignore"):
        assert np.isnan(M.chunk_minima(lr)).any()
    d, n = bound_forms_differ(C, lr, 1)
    assert d == 0
