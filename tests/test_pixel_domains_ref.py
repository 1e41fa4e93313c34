"""The oracle against the compiled reference on every PIXEL DOMAIN of tests/pixel_domains.py (CPU only): 16-bit and float
samples, denormals, signed zeros, flat regions, NaN nodata, +-Inf.  Bit for bit, NaN == NaN.  This is what makes the oracle a
sound yardstick for the GPU tests of the same domains (tests/test_gpu_pixel_domain.py).

Before anything is compared, every case that is not `degenerate_ok` must satisfy the NON-DEGENERACY CONDITION on the
reference's own volume (the oracle's where the reference is absent): at most half of the pixels all-zero, at most half of the
cells +INF -- a comparison of two trivial volumes proves nothing.

The reference reads CENSUS_NCC_WIN once per process: the window-5 and window-7 legs run in a child process each.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import pixel_domains as pd  # noqa: E402
from helpers import labels_equal, ndiff  # noqa: E402

# (nch, (ny, nx), right image (vny, vnx) or None, dmin, dmax): windows cross both borders of the right image, most labels inside
GEOMS = [(1, (96, 128), None, -12, 9), (3, (75, 181), (70, 175), -9, 12)]
TRUNCS = (np.inf, 20.0)
WINDOWED = [(p, d) for (p, d) in pd.SWEEP_PAIRS if "census" in (p, d) or d == "ncc"]
MAX_ZERO_SHARE = MAX_INF_SHARE = 0.5


def check_condition(C, cls, dist, tag):
    if pd.degenerate_ok(cls, pd.effective_distance(dist)):
        return
    zero, inf = pd.degeneracy(C)
    assert zero <= MAX_ZERO_SHARE and inf <= MAX_INF_SHARE, ("degenerate volume", tag, zero, inf)


def sweep(orc, ref, cls, win, pairs, seed0=0):
    """Every (geometry, prefilter, distance, truncDist) of one class at the process's window: the condition on the reference
    side (the oracle's without one), then oracle == reference.  Returns the number of volumes compared."""
    n = 0
    for g, (nch, (ny, nx), vshape, dmin, dmax) in enumerate(GEOMS):
        u, v = pd.pair(cls, seed0 + 100 * g + pd.CLASSES.index(cls), nch, ny, nx, vshape)
        for pre, dist in pairs:
            if "census" in (pre, dist) and not pd.census_aligned(nch, win):
                continue
            for td in TRUNCS:
                tag = (cls, nch, ny, nx, pre, dist, td, win)
                a = orc.costvolume(u, v, dmin, dmax, pre, dist, td, win)
                b = ref.costvolume(u, v, dmin, dmax, pre, dist, td) if ref is not None else a
                check_condition(b, cls, dist, tag)
                if ref is not None:
                    assert ndiff(a, b) == 0, tag
                    n += 1
        if ref is not None:
            for aP, aT in ((4.0, 5.0), (0.3, 12.0), (4.0, 1e30)):
                assert ndiff(orc.weights(u, aP, aT), ref.weights(u, aP, aT)) == 0, (cls, nch, aP, aT)
            if pd.census_aligned(nch, win):
                assert np.array_equal(orc.census(u, win // 2), ref.census(u, win // 2)), (cls, nch, win)
    return n


@pytest.fixture(scope="module")
def ref_or_none(request):
    try:
        return request.getfixturevalue("reference")
    except pytest.skip.Exception:
        return None


@pytest.mark.parametrize("cls", pd.CLASSES)
def test_costvolume_weights_census_vs_reference(oracle, ref_or_none, cls):
    win = ref_or_none.census_win() if ref_or_none is not None else 3
    sweep(oracle, ref_or_none, cls, win, pd.SWEEP_PAIRS)
    if ref_or_none is None:
        pytest.skip("compiled reference absent: only the non-degeneracy condition was checked, on the oracle")


@pytest.mark.parametrize("win", [5, 7])
def test_window_legs_in_a_child_process(win):
    from oracle.oracle import Reference
    if not Reference.available():
        pytest.skip("compiled reference (oracle/_ref) not available here")
    env = dict(os.environ, CENSUS_NCC_WIN=str(win), OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(win)], env=env, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert ("window %d ok" % win) in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("cls", ["nodata", "inf", "u16", "mixed"])
def test_ranged_costvolume_vs_reference(oracle, reference, cls):
    if not reference.has_ranged():
        pytest.skip("oracle/_ref/libmgm_ref.so predates the ranged entry points")
    from oracle import oracle as orc_mod
    from test_oracle_vs_ref import ragged_ranges
    win = reference.census_win()
    rng = np.random.default_rng(600 + pd.CLASSES.index(cls))
    for g, (nch, (ny, nx), vshape, hmin, hmax) in enumerate(GEOMS):
        u, v = pd.pair(cls, 40 + g, nch, ny, nx, vshape)
        for kind in ("smooth", "mixed"):
            dminI, dmaxI = ragged_ranges(rng, ny, nx, hmin, hmax, kind)
            lo, hi = orc_mod.int_ranges(dminI, dmaxI)
            for pre, dist in [("none", "ad"), ("none", "census"), ("sobelx", "sd"), ("none", "ncc"), ("gblur", "btad")]:
                for td in TRUNCS:
                    a = oracle.costvolume_ranged(u, v, lo, hi, hmin, hmax, pre, dist, td, win)
                    b = reference.costvolume_ranged(u, v, dminI, dmaxI, hmin, hmax, pre, dist, td)
                    assert ndiff(a, b) == 0, (cls, nch, kind, pre, dist, td)


AGG_CONFIGS = [(8, 3, 0, 8.0, 32.0), (8, 4, 1, 2.0, 9.0)]  # (NDIR, TSGM, FH, P1, P2): Hirschmueller / Felzenszwalb-Huttenlocher


@pytest.mark.parametrize("cls", ["nodata", "inf", "u16"])
def test_aggregation_and_refinement_vs_reference(oracle, reference, cls):
    """mgm() + the refinement on volumes built from non-8-bit / non-finite images: S, costs, labels wherever the cost is finite
    (elsewhere the reference's label is its uninitialised `float minP`, mgm_core.cc:594)."""
    win = reference.census_win()
    nch, ny, nx, dmin, dmax = 1, 40, 56, -10, 7
    u, v = pd.pair(cls, 900 + pd.CLASSES.index(cls), nch, ny, nx)
    for pre, dist in [("none", "ad"), ("none", "census"), ("none", "ncc")]:
        Cv = reference.costvolume(u, v, dmin, dmax, pre, dist, np.inf)
        check_condition(Cv, cls, dist, (cls, pre, dist))
        assert ndiff(oracle.costvolume(u, v, dmin, dmax, pre, dist, np.inf, win), Cv) == 0
        for (NDIR, MGM, FH, P1, P2) in AGG_CONFIGS:
            a = oracle.mgm(Cv, dmin, P1, P2, NDIR, MGM, FH, 1)
            b = reference.mgm(Cv, dmin, P1, P2, NDIR, MGM, FH, 1)
            tag = (cls, dist, NDIR, MGM, FH)
            assert ndiff(a[0], b[0]) == 0, tag
            assert ndiff(a[2], b[2]) == 0, tag
            assert labels_equal(a[1], b[1], a[2]), tag
            oo = np.where(np.isfinite(a[2]), a[1], dmin).astype(np.float32)
            for meth in ("vfit", "cubic"):
                ra, rb = oracle.refine(a[0], dmin, meth, oo, a[2]), reference.refine(b[0], dmin, meth, oo, b[2])
                assert ndiff(ra[0], rb[0]) == 0 and ndiff(ra[1], rb[1]) == 0, tag + (meth,)


# ---- the generator itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", pd.CLASSES)
def test_generator_is_deterministic_per_seed(cls):
    a, b = pd.pair(cls, 5, 3, 24, 40, (22, 36)), pd.pair(cls, 5, 3, 24, 40, (22, 36))
    assert a[0].shape == (3, 24, 40) and a[1].shape == (3, 22, 36) and a[0].dtype == np.float32
    assert all(ndiff(x, y) == 0 for x, y in zip(a, b))
    if cls != "const":
        c = pd.pair(cls, 6, 3, 24, 40, (22, 36))
        assert ndiff(a[0], c[0]) != 0


def test_generator_classes_hold_what_they_promise():
    g = lambda cls: pd.pair(cls, 3, 3, 48, 64)
    u, v = g("u16")
    assert u.max() > 40000 and np.array_equal(u, np.rint(u)) and u.min() >= 0 and u.max() <= 65535
    u, v = g("unit")
    assert 0 <= u.min() and u.max() <= 1 and np.any(u != np.rint(u))
    u, v = g("signed")
    assert u.min() < 0 < u.max() and np.any(u != np.rint(u))
    with np.errstate(over="ignore"):
        u, v = g("huge")
        assert np.all(np.isinf(u * u)) and np.all(np.isfinite(u))
        u, v = g("fltmax")
        assert np.all(np.isfinite(u)) and np.any(np.isinf(u + u + u + u + u))
    u, v = g("denormal")
    tiny = np.finfo(np.float32).tiny
    assert np.mean((u > 0) & (u < tiny)) > 0.3 and u.max() < 3e-38  # (denormals and the smallest normal numbers)
    u, v = g("negzero")
    assert np.any(np.signbit(u) & (u == 0)) and np.any(~np.signbit(u) & (u == 0))
    u, v = g("const")
    assert np.all(u == u.flat[0]) and np.all(v == u.flat[0])
    for cls in ("nodata", "mixed"):
        u, v = g(cls)
        for a in (u, v):
            nan = np.isnan(a)
            # per PIXEL: the same in every channel (mixed: except where one of the eight Inf samples fell on a nodata pixel)
            assert int((nan.any(axis=0) & ~nan.all(axis=0)).sum()) <= (8 if cls == "mixed" else 0)
            assert 0.02 < nan[0].mean() < 0.25
        assert not np.array_equal(np.isnan(u[0]), np.isnan(v[0]))
    u, v = g("nodata_all")
    assert np.all(np.isnan(v)) and not np.any(np.isnan(u))
    for cls in ("inf", "mixed"):
        u, v = g(cls)
        for a in (u, v):
            assert np.any(np.isposinf(a)) and np.any(np.isneginf(a))
    assert pd.degenerate_ok("const") and pd.degenerate_ok("nodata_all", "ncc") and pd.degenerate_ok("huge", "sd")
    assert not pd.degenerate_ok("huge", "ad") and not pd.degenerate_ok("nodata", "ncc") and not pd.degenerate_ok("u16", "sd")
    assert pd.degenerate_ok("denormal", "sd") and not pd.degenerate_ok("denormal", "ncc")


def _child(win):  # (what the child process runs)
    from oracle.oracle import Oracle, Reference
    orc, ref = Oracle(threads=int(os.environ.get("OMP_NUM_THREADS", "1"))), Reference()
    assert ref.census_win() == win, (ref.census_win(), win)
    n = sum(sweep(orc, ref, cls, win, WINDOWED, seed0=1000 * win) for cls in pd.CLASSES)
    print("window %d ok: %d volumes" % (win, n))


if __name__ == "__main__":
    _child(int(sys.argv[1]))
