"""Which launches a filling of a cost volume makes, in which order, and what a refill skips.

Every map can stay bit-exact while a filling launches something else, or a refill forgets what the volume learnt: this file
pins the cost side of the timing table -- the names beginning k_census, k_filter2d, k_cost_ and k_rel_gather, in order -- for
every form a filling is written in (mgm_fillplan.h), and compares the downloaded volume with the oracle bit for bit.

Left images of 44x20 (42x20 where a case says "odd width": the _w4 kernels depend on nx mod 4), synthetic 8-bit pairs, 64
labels from -32 unless stated.  Before a case is compared the oracle's volume meets the non-degeneracy condition of
tests/test_gpu_pixel_domain.py (at most half of the pixels all-zero, at most half of the cells +INF).  Two kinds of case cannot
meet it with a 44-pixel right image and 64 labels, so they deviate:
  - 151 labels, and windows of 101 labels in a hull of 128: the right image is 240 pixels wide and the labels start at 0, so
    that no disparity leaves it;
  - windows of 21 labels: the hull has 40 labels (21 of 64 would leave two thirds of the cells +INF) and the same wide right image.
The expected names follow launch_cost's dispatch (mgm_cost_fast.hip) as read from the code; when this file was written no device was
at hand to confirm them against the build before the filling became a plan, which they are meant to hold for as well.
"""
import numpy as np
import pytest

import pixel_domains as pd
from helpers import ndiff
from mgm_amd import synth
from oracle.oracle import int_ranges

pytestmark = pytest.mark.gpu

INF = float("inf")
NY = 20
DMIN, DMAX = -32, 31
COST_SIDE = ("k_census", "k_filter2d", "k_cost_", "k_rel_gather")
CENSUS = ["k_census", "k_census"]


def pair(nx, nch=1, vnx=None, seed=4100):
    """An 8-bit pair whose left image is nx x 20; vnx: a wider right image (the left one continued by noise of the same kind)."""
    u, v, gt = synth.stereo_pair(vnx or nx, NY, -12, 0, seed=seed, nch=nch)
    return np.ascontiguousarray(u[:, :, :nx]), v, gt[:, :nx]


def cost_side(ctx, fn):
    """fn() with the timing table on: (its result, the cost-side names in order)."""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        out = fn()
        names = [n for n, _ in ctx.timings()]
    finally:
        ctx.timing(False)
        ctx.timing_reset()
    return out, [n for n in names if n.startswith(COST_SIDE)], names


def nontrivial(C, tag):
    zero, inf = pd.degeneracy(C)
    assert zero <= 0.5 and inf <= 0.5, ("degenerate volume", tag, zero, inf)


def fill(ctx, oracle, u, v, want, pre="none", dist="ad", td=INF, win=3, dmin=DMIN, dmax=DMAX, into=None, tag=None):
    """One filling: the cost-side launches are `want`, the volume is the oracle's.  Returns the volume."""
    a = oracle.costvolume(u, v, dmin, dmax, pre, dist, td, win)
    nontrivial(a, tag)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    cv, got, _ = cost_side(ctx, lambda: ctx.costvolume_dev(du, dv, dmin, dmax, pre, dist, td, win, into=into))
    print(tag, got)
    assert got == want, (tag, got, want)
    assert ndiff(a, cv.download()) == 0, tag
    du.free()
    dv.free()
    return cv


def test_grey_ad_one_byte(ctx, oracle):
    u, v, _ = pair(44)
    fill(ctx, oracle, u, v, ["k_cost_diffx_1b"], tag="grey AD").free()


def test_grey_ad_with_a_difference_of_255_widens_and_the_refill_starts_there(ctx, oracle):
    u, v, _ = pair(44)
    u[0, 7, 20], v[0, 7, 15] = 255.0, 0.0  # (disparity -5: inside the labels)
    cv = fill(ctx, oracle, u, v, ["k_cost_diffx_1b", "k_cost_diffx_2b"], tag="grey AD, 255")
    fill(ctx, oracle, u, v, ["k_cost_diffx_2b"], into=cv, tag="grey AD, 255, refill").free()


def test_colour_ad_and_grey_sd_two_bytes(ctx, oracle):
    u3, v3, _ = pair(44, nch=3)
    fill(ctx, oracle, u3, v3, ["k_cost_diffx_2b"], tag="colour AD").free()
    u, v, _ = pair(44)
    fill(ctx, oracle, u, v, ["k_cost_diffx_2b"], dist="sd", tag="grey SD").free()


def test_half_integer_pair_gives_up_the_compact_form_after_two_fillings(ctx, oracle):
    u, v, _ = pair(44)
    vh = v + np.float32(0.5)  # (every difference ends in .5: no compact form of any width)
    both = ["k_cost_diffx_1b", "k_cost_btx_diff_w4"]
    cv = fill(ctx, oracle, u, vh, both, tag="half-integer AD")
    fill(ctx, oracle, u, vh, both, into=cv, tag="half-integer AD, refill 1")
    fill(ctx, oracle, u, vh, ["k_cost_btx_diff_w4"], into=cv, tag="half-integer AD, refill 2")
    fill(ctx, oracle, u, v, ["k_cost_btx_diff_w4"], into=cv, tag="8-bit AD after two misfits").free()


def test_151_labels_write_the_padded_copy_and_the_aggregation_pads_nothing(ctx, oracle):
    u, v, _ = pair(44, vnx=240)
    cv = fill(ctx, oracle, u, v, ["k_cost_diffx_1b"], dmin=0, dmax=150, tag="grey AD, 151 labels")
    outs, _, names = cost_side(ctx, lambda: ctx.aggregate_dev(cv, 2.0, 20.0, 8, 3))
    for h in outs:
        if h is not None:
            h.free()
    print("151 labels, aggregation", names)
    assert any(n.startswith("k_pass") for n in names) and "k_pad" not in names, names
    cv.free()


def test_census_one_word(ctx, oracle):
    u, v, _ = pair(44)
    fill(ctx, oracle, u, v, CENSUS + ["k_cost_census8x_w4"], dist="census", win=5, tag="census 5x5").free()
    u, v, _ = pair(42)
    fill(ctx, oracle, u, v, CENSUS + ["k_cost_census8x"], dist="census", win=5, tag="census 5x5, odd width").free()


def test_census_with_a_fractional_truncation_takes_the_fp32_kernel(ctx, oracle):
    u, v, _ = pair(44)
    fill(ctx, oracle, u, v, CENSUS + ["k_cost_general"], dist="census", td=7.5, win=5, tag="census 5x5, truncDist 7.5").free()


def test_census_two_words_ncc_and_birchfield_tomasi(ctx, oracle):
    u, v, _ = pair(44)
    fill(ctx, oracle, u, v, CENSUS + ["k_cost_btx_census_w4"], dist="census", win=7, tag="census 7x7").free()
    fill(ctx, oracle, u, v, ["k_cost_ncc"], dist="ncc", tag="NCC").free()
    fill(ctx, oracle, u, v, ["k_cost_btx_bt_w4"], dist="btad", tag="BTAD").free()


def ragged(ctx, oracle, u, v, gt, width, hull, want, dist, win, into=None, tag=None):
    """A ragged filling with windows of `width` labels around the truth (moved to the labels 0..) in a hull of `hull` labels."""
    lo = np.clip(gt + 12 + (hull - width) // 2 - 6, 0, hull - width).astype(np.float32)
    hi = lo + np.float32(width - 1)
    ilo, ihi = int_ranges(lo, hi)
    a = oracle.costvolume_ranged(u, v, ilo, ihi, 0, hull - 1, "none", dist, INF, win)
    nontrivial(a, tag)
    du, dv, dlo, dhi = (ctx.upload_image(x) for x in (u, v, lo, hi))
    cv, got, _ = cost_side(ctx, lambda: ctx.costvolume_ranged_dev(du, dv, dlo, dhi, 0, hull - 1, "none", dist, INF, win, into=into))
    print(tag, got)
    assert got == want, (tag, got, want)
    assert ndiff(a, cv.download()) == 0, tag
    for h in (du, dv, dlo, dhi):
        h.free()
    return cv


def test_ragged_census_is_written_as_its_range_proportional_copy(ctx, oracle):
    u, v, gt = pair(44, vnx=240)
    ragged(ctx, oracle, u, v, gt, 21, 40, CENSUS + ["k_cost_census_rel"], "census", 5, tag="ragged census, windows of 21").free()


def test_ragged_census_with_wide_windows_takes_128_slots_and_the_refill_starts_there(ctx, oracle):
    u, v, gt = pair(44, vnx=240)
    cv = ragged(ctx, oracle, u, v, gt, 101, 128, CENSUS + ["k_cost_census_rel", "k_cost_census_rel"], "census", 5, tag="ragged census, windows of 101")
    ragged(ctx, oracle, u, v, gt, 101, 128, CENSUS + ["k_cost_census_rel"], "census", 5, into=cv, tag="ragged census, windows of 101, refill").free()


def test_ragged_grey_ad_is_gathered_from_the_fp32_hull(ctx, oracle):
    u, v, gt = pair(44, vnx=240)
    ragged(ctx, oracle, u, v, gt, 21, 40, ["k_cost_general", "k_rel_gather"], "ad", 3, tag="ragged AD, windows of 21").free()
