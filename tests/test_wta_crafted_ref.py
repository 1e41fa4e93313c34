"""The expectation tests/test_gpu_wta_crafted.py holds the winner search and the refinements to, pinned on the CPU:
the numpy restatement of tests/wta_crafted.py against the oracle's own sum and search (mgm_core.cc:582-609, with and
without range images), the oracle's four refinements against the compiled reference on S volumes of every crafted class
-- non-finite, huge, denormal and signed-zero values included --, the labels the stand-alone refinement is fed, and the
floors every class has to reach before anything is compared with it."""
import numpy as np
import pytest

import wta_crafted as W
from helpers import ndiff
from mgm_amd import synth

METHODS = ("vfit", "parabola", "cubic", "parabolaOCV")
NDIRS = (1, 2, 5, 8)


def small_volume():
    C = synth.raw_volume(23, 11, 40, seed=5, inf_frac=0.05)
    C[4, 7, :] = np.inf  # one pixel without a finite cost
    return C


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("NDIR", NDIRS)
def test_sum_fix_wta_is_the_oracles(oracle, NDIR, fix):
    """(NDIR 1 with the fix: 0 * INF = NaN on every +INF cost)"""
    C, dmin = small_volume(), -7
    So, oo, co, lr = oracle.mgm(C, dmin, 8.0, 32.0, NDIR, 3, 0, fix, dump_lr=True)
    S, idx, cost = W.sum_fix_wta(lr, C, NDIR, fix)
    fin = np.isfinite(co)
    assert fin.any() and not fin[4, 7]
    assert ndiff(S, So) == 0 and ndiff(cost, co) == 0
    assert ndiff((idx + np.float32(dmin))[fin], oo[fin]) == 0
    assert np.isnan(idx[~fin]).all()


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("NDIR", NDIRS)
def test_windowed_is_the_oracles_search_with_narrowed_ranges(oracle, NDIR, fix):
    C, dmin = small_volume(), -7
    ny, nx, L = C.shape
    full_lo, full_hi = np.full((ny, nx), dmin, np.int32), np.full((ny, nx), dmin + L - 1, np.int32)
    lr = oracle.mgm(C, dmin, 8.0, 32.0, NDIR, 3, 0, fix, dump_lr=True)[3]
    S = W.sum_fix(lr, C, NDIR, fix)
    rng = np.random.default_rng(3)
    centre = rng.integers(dmin - 4, dmin + L + 4, size=(ny, nx))
    lo = (centre - rng.integers(0, 6, size=(ny, nx))).astype(np.float32) + np.float32(0.4)
    hi = (centre + rng.integers(0, 6, size=(ny, nx))).astype(np.float32) + np.float32(0.7)
    out, cost, Sh, hmin, wl, wh = W.windowed(S, dmin, lo, hi, NDIR, fix)
    hmax = hmin + Sh.shape[2] - 1
    assert hmin < dmin and hmax > dmin + L - 1  # windows straddle both ends
    So, oo, co = oracle.mgm_ranged(C, dmin, full_lo, full_hi, 8.0, 32.0, NDIR, 3, 0, fix, srange=(wl, wh, hmin, hmax))
    fin = np.isfinite(co)
    assert fin.any()
    assert ndiff(cost, co) == 0 and ndiff(out[fin], oo[fin]) == 0
    d = np.arange(hmin, hmax + 1)
    inwin = (d >= wl[..., None]) & (d <= wh[..., None])
    assert ndiff(Sh[inwin], So[inwin]) == 0


def crafted_S(name, cname, L, NDIR=8, fix=1):
    ny, nx = (33, 97) if L == 12 else (10, 13)
    lr = W.LR_CLASSES[name](21, NDIR, ny, nx, L)
    C = W.C_CLASSES[cname](22, ny, nx, L)
    return W.sum_fix_wta(lr, C, NDIR, fix)


@pytest.mark.parametrize("L", [12, 256])
@pytest.mark.parametrize("name", list(W.LR_CLASSES))
def test_oracle_refinements_are_the_references_on_crafted_S(oracle, reference, name, L):
    dmin = -5
    nan_results = 0
    for cname in ("ints", "negative", "nan"):
        S, idx, cost = crafted_S(name, cname, L)
        lab = np.where(np.isnan(idx), np.float32(dmin), idx + np.float32(dmin)).astype(np.float32)  # (dmin where none is finite, as the existing tests do)
        for m in METHODS:
            ro, rc = reference.refine(S, dmin, m, lab, cost)
            oo, oc = oracle.refine(S, dmin, m, lab, cost)
            assert ndiff(oo, ro) == 0 and ndiff(oc, rc) == 0, (name, cname, m)
            nan_results += int(np.isnan(ro).sum())
    print("%s L=%d: %d NaN results" % (name, L, nan_results))


@pytest.mark.parametrize("name", list(W.LR_CLASSES))
def test_oracle_ranged_refinements_are_the_references_on_crafted_S(oracle, reference, name):
    if not reference.has_ranged():
        pytest.skip("this build of the reference harness has no range images")
    dmin, L, NDIR = -5, 12, 4
    rng = np.random.default_rng(8)
    for cname in ("ints", "negative", "nan"):
        for fix in (0, 1):
            S = crafted_S(name, cname, L, NDIR, fix)[0]
            ny, nx, _ = S.shape
            centre = rng.integers(dmin - 4, dmin + L + 4, size=(ny, nx))
            lo = (centre - rng.integers(0, 7, size=(ny, nx))).astype(np.float32) + np.float32(0.4)
            hi = (centre + rng.integers(0, 7, size=(ny, nx))).astype(np.float32) + np.float32(0.7)
            out, cost, Sh, hmin, wl, wh = W.windowed(S, dmin, lo, hi, NDIR, fix)
            lab = np.where(np.isnan(out), np.float32(hmin), out).astype(np.float32)
            for m in METHODS:
                ro, rc = reference.refine_ranged(Sh, hmin, lo, hi, m, lab, cost)
                oo, oc = oracle.refine_ranged(Sh, hmin, wl, wh, m, lab, cost)
                assert ndiff(oo, ro) == 0 and ndiff(oc, rc) == 0, (name, cname, fix, m)


@pytest.mark.parametrize("name", list(W.LR_CLASSES))
def test_oracle_refinements_on_the_labels_the_test_chooses(oracle, reference, name):
    """tests/test_gpu_wta_crafted.py, part C: S is the class's one-pass volume as it stands (signed zeros kept), the labels are
    W.refine_labels.  The reference never sees a NaN label ((int) of it is undefined there): the oracle must leave it alone."""
    dmin = -5
    for L, (ny, nx) in ((12, (7, 19)), (256, (12, 47))):
        S = W.LR_CLASSES[name](31, 1, ny, nx, L)[0]
        lab = W.refine_labels(32, ny, nx, dmin, L)
        cost = np.random.default_rng(33).uniform(-3, 3, (ny, nx)).astype(np.float32)
        nan = np.isnan(lab)
        assert nan.any() and len(np.unique(np.trunc(lab[~nan]))) == L + 4
        assert (lab[~nan] != np.trunc(lab[~nan])).any()
        for m in METHODS:
            oo, oc = oracle.refine(S, dmin, m, lab, cost)
            ro, rc = reference.refine(S, dmin, m, np.where(nan, np.float32(dmin - 2), lab), cost)
            assert ndiff(oo[~nan], ro[~nan]) == 0 and ndiff(oc[~nan], rc[~nan]) == 0, (name, L, m)
            assert np.isnan(oo[nan]).all() and ndiff(oc[nan], cost[nan]) == 0
            moved = (~nan) & (oo.view(np.uint32) != lab.view(np.uint32))
            assert moved.any() or name in ("flat",), (name, L, m)


SHAPES = ((5, 13, 12), (10, 13, 64), (10, 13, 100), (5, 13, 192), (5, 13, 256), (3, 11, 8), (10, 13, 4), (5, 13, 384), (1, 9, 2049),
          (1, 1, 64), (13, 10, 3))


@pytest.mark.parametrize("name", list(W.LR_CLASSES))
def test_floors(name):
    """every class reaches its floors (tests/wta_crafted.py) at every shape family of the device tests, at 1, 3, 4, 5 and 8 passes,
    without the over-count fix and with it under every tame cost class"""
    for ny, nx, L in SHAPES:
        for NDIR in (1, 3, 4, 5, 8):
            lr = W.LR_CLASSES[name](11, NDIR, ny, nx, L)
            assert lr.dtype == np.float32 and lr.shape == (NDIR, ny, nx, L)
            for cname in W.TAME_C:
                C = W.C_CLASSES[cname](5, ny, nx, L)
                for fix in ((0, 1) if cname == "ints" else (1,)):
                    W.floors(name, lr, C, NDIR, fix, L, verbose=(NDIR == 8 and cname == "ints" and L in (12, 256)))


def test_cost_classes_hold_what_they_name():
    ny, nx, L = 10, 13, 64
    planted = W.PLANTED(np.arange(ny * nx).reshape(ny, nx))
    for cname, fn in W.C_CLASSES.items():
        C = fn(5, ny, nx, L)
        assert C.dtype == np.float32 and C.shape == (ny, nx, L)
        if cname != "inf1":
            assert np.isfinite(C[planted]).all() and (C[planted] == C[planted][:, :1]).all(), cname
    assert np.isposinf(W.c_ints(5, ny, nx, L)).any() and np.isposinf(W.c_inf1(5, ny, nx, L)).any()
    assert (W.c_negative(5, ny, nx, L) < 0).any() and np.isnan(W.c_nan(5, ny, nx, L)).any()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(2) * W.c_huge(5, ny, nx, L)).any()
