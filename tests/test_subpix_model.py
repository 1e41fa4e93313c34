"""The numpy model of sub-pixel label spacing (tests/subpix_model.py) on the CPU: its phase arithmetic against a scalar
restatement, the interleave against the definition, and what the mode buys -- a property of the definition, shown through the
oracle's aggregation alone."""
import numpy as np
import pytest

import subpix_model as M
from mgm_amd import synth

f32 = np.float32


def special_row(nx, seed):
    rng = np.random.default_rng(seed)
    row = (rng.integers(0, 256, nx) + rng.random(nx)).astype(np.float32)
    for i, val in enumerate((np.nan, np.inf, -np.inf, 1e-41, -0.0, 3e38)):
        if nx > 6:
            row[(2 * i + 1) % nx] = val
    return row


@pytest.mark.parametrize("nx", [1, 2, 3, 4, 7, 64])
def test_phase_image_is_the_scalar_arithmetic(nx):
    """... including widths 1, 2 and 3, where the clamps of x-1, x+1 and x+2 overlap."""
    rows = np.stack([special_row(nx, 10 * nx + j) for j in range(3)])
    img = rows.reshape(1, 3, nx)
    for interp in M.INTERPS:
        for s, k in M.PHASES:
            got = M.phase_image(img, s, k, interp)
            want = np.array([[M.phase_pixel(r, x, s, k, interp) for x in range(nx)] for r in rows], np.float32).reshape(1, 3, nx)
            assert got.dtype == np.float32 and M.same_bits(got, want), (interp, s, k)
            if k == 0:
                assert np.array_equal(got.view(np.uint32), img.view(np.uint32))   # v_0 is v, the same bits, NaN payloads included


def test_the_weights_are_exact_and_sum_to_one():
    for interp in M.INTERPS:
        for s, k in M.PHASES:
            w = M.weights(s, k, interp)
            assert all(float(x) * 128 == int(float(x) * 128) for x in w)
            assert sum(float(x) for x in w) == 1.0
    # a constant row stays the constant under either kernel, and the half-pixel cubic is symmetric
    img = np.full((1, 2, 9), 37.0, np.float32)
    for interp in M.INTERPS:
        for s, k in M.PHASES:
            assert np.array_equal(M.phase_image(img, s, k, interp), img)
    assert M.weights(2, 1, "cubic") == M.weights(2, 1, "cubic")[::-1] and M.weights(4, 1, "cubic") == M.weights(4, 3, "cubic")[::-1]


def test_s1_is_the_oracles_volume(oracle):
    u, v, _ = synth.stereo_pair(40, 6, -9, 3)
    for dist, pre in (("ad", "none"), ("census", "none")):
        assert M.same_bits(M.fine_volume(oracle, u, v, -9, 3, 1, "cubic", pre, dist, np.inf, 3), oracle.costvolume(u, v, -9, 3, pre, dist, np.inf, 3))


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("dmin,dmax", [(-7, -2), (-3, 4), (2, 9), (5, 5)])
def test_interleave_by_offset_and_the_dropped_label(oracle, s, dmin, dmax):
    """F(o') = C_{o' mod s}(o' div s) with o' counted from s*dmin -- a negative s*dmin must not disturb mod / div -- and label dmax of
    the phases k > 0 appears nowhere."""
    u, v, _ = synth.stereo_pair(24, 4, -6, 6, seed=5)
    ph = M.phase_volumes(oracle, u, v, dmin, dmax, s, "cubic")
    F = M.interleave(ph)
    L = dmax - dmin + 1
    assert F.shape == (4, 24, s * (L - 1) + 1)
    for o in range(F.shape[2]):
        d_fine = s * dmin + o
        k, i = (d_fine - s * dmin) % s, (d_fine - s * dmin) // s
        assert M.same_bits(F[:, :, o], ph[k][:, :, i])
        assert i < L - 1 or k == 0
    assert M.same_bits(F[:, :, ::s], ph[0])   # the integer labels are phase 0, all of them


def test_a_pixel_outside_for_every_label_reads_zero_in_every_phase(oracle):
    """Every phase is built over the same [dmin, dmax], so a pixel lies outside the other image for all phases or for none: the
    builder's "no finite cost => zeros" rule then gives zeros in all of F's labels."""
    u, v, _ = synth.stereo_pair(20, 3, 0, 4, seed=3)
    dmin, dmax = 15, 18   # x + d >= 20 for x >= 5: those pixels see nothing
    for s in (2, 4):
        F = M.fine_volume(oracle, u, v, dmin, dmax, s, "linear")
        assert np.array_equal(F[:, 5:, :], np.zeros_like(F[:, 5:, :]))
        assert np.isinf(F[:, 2, -1]).all() and np.isfinite(F[:, 2, 0]).all()   # x = 2: d = 15 inside, d = 18 outside


def test_what_the_mode_buys(oracle):
    """A textured plane whose true disparity runs through the quarter-pixel values: the mean absolute error over the plane's interior
    falls from s = 1 to 2 to 4 without refinement, and from s = 1 to 2 with vfit (the figures are DESIGN.md 7g's)."""
    u, v, gt, dmin, dmax = M.slanted_scene()
    inner = np.isfinite(gt)
    inner[:, :8] = inner[:, -8:] = False
    inner[:2] = inner[-2:] = False
    assert inner.sum() > 300 and len(np.unique((4 * gt[inner]).astype(int) % 4)) == 4
    P1, P2, NDIR, TSGM = 2.0, 16.0, 4, 1
    mae = {}
    for refine in ("none", "vfit"):
        for s in (1, 2, 4):
            out, _, _ = M.run(oracle, u, v, dmin, dmax, s, "cubic", P1, P2, NDIR, TSGM, 0, 1, refine, distance="ad")
            mae[refine, s] = float(np.abs(out - gt)[inner].mean())
    print("mean absolute error, pixels:", {k: round(e, 4) for k, e in mae.items()})
    assert mae["none", 2] < mae["none", 1] and mae["none", 4] < mae["none", 2]
    assert mae["vfit", 2] < mae["vfit", 1]


def test_scale_is_exact():
    m = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 3.0, -7.0, 1e-45, 2.5e-45, 3e38], np.float32)
    for s in (1, 2, 4):
        r = M.scale(m, s)
        assert np.isnan(r[0]) and r[1] == np.inf and r[2] == -np.inf and np.signbit(r[3]) and not np.signbit(r[4])
        assert np.array_equal(r[5:7], m[5:7] / f32(s)) and np.array_equal((r[5:7] * f32(s)), m[5:7])
