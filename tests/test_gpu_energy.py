"""mgm_energy_dev (mgm_energy.hip) against the numpy model (tests/energy_model.py, pinned on the reference binary by
tests/test_energy_model_ref.py): maps and the serial fp32 sum bit for bit (NaN == NaN), the fp64 totals within the bound of any
summation order, on crafted maps -- no aggregation needed -- over every copy a cost volume can be current in."""
import math

import numpy as np
import pytest

import energy_model as em
import mgm_amd
from mgm_amd import synth
from oracle.oracle import int_ranges

pytestmark = pytest.mark.gpu
F = np.float32
INF = float("inf")
SIZES = [(1, 7), (7, 1), (2, 2), (3, 3), (63, 2), (64, 3), (65, 5), (130, 4), (96, 40)]  # (nx, ny)


def same(a, b):
    a, b = np.asarray(a, F).ravel(), np.asarray(b, F).ravel()
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def crafted_map(nx, ny, dmin, L, seed, lo=None, hi=None, specials=True):
    """labels in range, outside the volume, outside the pixel's own range, fractional (x.5 for rintf), NaN, +-INF, +-2^24"""
    rng = np.random.default_rng(seed)
    d = rng.integers(dmin, dmin + L, (ny, nx)).astype(F)
    pick = lambda p: rng.random((ny, nx)) < p
    out = pick(0.1)
    d[out] = rng.choice([dmin - 1, dmin - 7, dmin + L, dmin + L + 5], out.sum()).astype(F)
    if lo is not None:
        m = pick(0.15)
        d[m] = (np.where(rng.random((ny, nx)) < 0.5, lo - 1, hi + 1).astype(F))[m]
    fr = pick(0.25)
    d[fr] += rng.choice([0.25, 0.5, 0.75, 1.5, -0.5], fr.sum()).astype(F)
    if specials:
        for k, val in enumerate((np.nan, np.inf, -np.inf, 2.0 ** 24, -2.0 ** 24)):
            d.ravel()[(seed + 3 * k) % d.size] = val
    return d


def check(ctx, cv, C, dmin, d, kind, P1, P2, conn=4, fh=0, w8=None, lo=None, hi=None, what=None):
    dd = ctx.upload_image(d)
    dw = ctx.upload_image(w8) if w8 is not None else None
    E, t = ctx.energy_dev(cv, dd, kind, P1, P2, conn, fh, dw)
    E2, t2 = ctx.energy_dev(cv, dd, kind, P1, P2, conn, fh, dw)
    _, t3 = ctx.energy_dev(cv, dd, kind, P1, P2, conn, fh, dw, want_map=False)
    E4, none = ctx.energy_dev(cv, dd, kind, P1, P2, conn, fh, dw, want_totals=False)
    got, got2, got4 = E.download()[0], E2.download()[0], E4.download()[0]
    for im in (dd, dw, E, E2, E4):
        if im is not None:
            im.free()
    wantE, want = em.energy(C, dmin, d, kind, P1, P2, conn, fh, w8, lo, hi)
    assert same(got, wantE), (what, kind, np.argwhere(~(np.isnan(got) & np.isnan(wantE)) & (got.view(np.uint32) != wantE.view(np.uint32)))[:5])
    assert same(got, got2) and same(got, got4) and none is None
    assert same([t["serial"]], [want["serial"]]), (what, kind, t["serial"], want["serial"])
    assert (t["finite"], t["pixels"]) == (want["finite"], want["pixels"]) == (int(np.isfinite(d).sum()), d.size)
    for k in ("serial", "total", "data", "smooth"):  # two calls give equal bits; with and without the map
        for other in (t2, t3):
            assert np.float64(t[k]).tobytes() == np.float64(other[k]).tobytes() or (math.isnan(t[k]) and math.isnan(other[k])), (what, k)
    return got, t, want


def test_sizes_uploaded_fp32_volume(ctx):
    """random non-integer costs, every size, every kind: the borders where every edge term vanishes, widths around a wave"""
    for nx, ny in SIZES:
        rng = np.random.default_rng(100 * nx + ny)
        dmin, L = -5, 9
        C = (rng.random((ny, nx, L)) * 37.5).astype(F)
        C[rng.random(C.shape) < 0.04] = np.inf
        cv = ctx.upload_volume(C, dmin)
        d = crafted_map(nx, ny, dmin, L, nx + ny)
        w8 = (rng.random((8, ny, nx)) * 2.5).astype(F)  # (free-form and asymmetric: w_pq and w_qp are unrelated)
        for kind in (0, 1, 2):
            check(ctx, cv, C, dmin, d, kind, 2.5, 11.0, what=(nx, ny))
        for conn in (4, 8):
            for fh in (0, 1):
                check(ctx, cv, C, dmin, d, 3, 1.5, 7.25, conn, fh, None, what=(nx, ny, conn, fh))
                check(ctx, cv, C, dmin, d, 3, 1.5, INF, conn, fh, w8, what=(nx, ny, conn, fh, "w8, P2 inf"))
        cv.free()


def ran_during(ctx, fn):
    ctx.timing(True)
    ctx.timing_reset()
    try:
        r = fn()
        names = [n for n, _ in ctx.timings()]
    finally:
        ctx.timing(False)
    return r, names


def pair(nx, ny, nch=1, seed=5):
    u, v, gt = synth.stereo_pair(nx, ny, -12, 4, seed=seed, nch=nch)
    return u, v, gt


FORMATS = ["census byte codes", "two-byte colour ad", "padded label count 151", "ragged on its hull", "ragged, range-proportional copy only",
           "fine volume s=2"]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("size", [(65, 5), (96, 40)], ids=["65x5", "96x40"])
def test_every_copy_of_a_volume(ctx, fmt, size):
    """the energy is read from the copy that is current: no whole volume is decoded for it (no k_expand inside the call), and where
    the fp32 array was stale it still is afterwards (the download that follows has to expand)"""
    nx, ny = size
    nch = 3 if fmt == "two-byte colour ad" else 1
    u, v, gt = pair(nx, ny, nch)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    lo = hi = None
    scale = 1
    if fmt == "census byte codes":
        cv, stale = ctx.costvolume_dev(du, dv, -40, 23, "none", "census", INF, 3), True
    elif fmt == "two-byte colour ad":
        cv, stale = ctx.costvolume_dev(du, dv, -40, 23, "none", "ad", INF, 3), True
    elif fmt == "padded label count 151":
        cv, stale = ctx.costvolume_dev(du, dv, -100, 50, "none", "census", INF, 3), True
    elif fmt == "ragged on its hull":
        rng = np.random.default_rng(2)
        lof = (gt - rng.integers(1, 6, gt.shape)).astype(F)
        hif = (lof + rng.integers(1, 12, gt.shape)).astype(F)
        cv, stale = ctx.costvolume(u, v, lof, hif, "none", "sd", 300.5, 3), False
        lo, hi = int_ranges(lof, hif)
    elif fmt == "ragged, range-proportional copy only":
        rng = np.random.default_rng(3)
        lof = (gt - rng.integers(1, 6, gt.shape)).astype(F)
        hif = (lof + rng.integers(1, 12, gt.shape)).astype(F)
        cv, stale = ctx.costvolume(u, v, lof, hif, "none", "census", INF, 3), True
        lo, hi = int_ranges(lof, hif)
    else:
        cv, stale, scale = ctx.costvolume_subpix_dev(du, dv, -12, 4, 2, "cubic", "none", "census", INF, 3), None, 2
    _, _, dmin, dmax = cv.dims
    L = dmax - dmin + 1
    if scale == 2:
        assert (dmin, dmax) == (-24, 8)  # labels and d in fine units
    d = crafted_map(nx, ny, dmin, L, 7 * nx + ny, lo, hi)
    dd = ctx.upload_image(d)
    w8img = ctx.weights_dev(du, 4.0, 12.0)
    runs = [(0, 4, 0, None), (1, 4, 0, None), (2, 4, 0, None), (3, 4, 0, None), (3, 8, 1, w8img), (3, 8, 0, w8img)]
    outs, names = ran_during(ctx, lambda: [ctx.energy_dev(cv, dd, k, 3.0, 9.5, conn, fh, w) for k, conn, fh, w in runs])
    assert names.count("k_energy") == len(runs) and "k_expand" not in names, names
    C, names = ran_during(ctx, cv.download)
    if stale is not None:
        assert ("k_expand" in names) == stale, (fmt, names)  # the energy calls left the volume's copies as they were
    w8 = w8img.download()
    for (k, conn, fh, w), (E, t) in zip(runs, outs):
        wantE, want = em.energy(C, dmin, d, k, 3.0, 9.5, conn, fh, w8 if w is not None else None, lo, hi)
        assert same(E.download()[0], wantE), (fmt, k, conn, fh)
        assert same([t["serial"]], [want["serial"]]) and t["finite"] == want["finite"]
        E.free()
    # ... and on the fp32 array the download has just made current: the same bits
    for (k, conn, fh, w), (E, t) in zip(runs[3:5], outs[3:5]):
        E2, t2 = ctx.energy_dev(cv, dd, k, 3.0, 9.5, conn, fh, w)
        assert np.float64(t2["total"]).tobytes() == np.float64(t["total"]).tobytes() or math.isnan(t["total"])
        E2.free()
    for o in (du, dv, dd, w8img, cv):
        o.free()


def test_fp64_totals_within_the_bound_of_any_summation_order(ctx):
    """non-negative finite addends: |total - fsum(model map)| <= n * 2^-52 * fsum, for data, smooth and total"""
    for nx, ny in ((65, 5), (130, 4), (96, 40), (257, 33)):
        rng = np.random.default_rng(nx)
        dmin, L = -3, 8
        C = (rng.random((ny, nx, L)) * 100).astype(F)
        cv = ctx.upload_volume(C, dmin)
        d = crafted_map(nx, ny, dmin, L, 9, specials=False)
        d = np.clip(d, dmin, dmin + L - 1).astype(F)
        d[rng.random(d.shape) < 0.05] = np.nan  # holes: left out of the sums and of `finite`
        w8 = (rng.random((8, ny, nx)) * 2).astype(F)
        for kind, conn, fh, w in ((0, 4, 0, None), (1, 4, 0, None), (3, 8, 0, w8), (3, 4, 1, None)):
            if kind != 3 and np.isnan(d).any():
                dk = np.nan_to_num(d, nan=0.0).astype(F)  # (kinds 0-2: a NaN neighbour makes the addends NaN)
            else:
                dk = d
            dd = ctx.upload_image(dk)
            dw = ctx.upload_image(w) if w is not None else None
            _, t = ctx.energy_dev(cv, dd, kind, 2.0, 8.0, conn, fh, dw, want_map=False)
            E, data, smooth = em.energy_map(C, dmin, dk, kind, 2.0, 8.0, conn, fh, w)
            fin = np.isfinite(dk)
            n = int(fin.sum())
            assert t["finite"] == n and t["pixels"] == dk.size
            for key, m in (("total", E), ("data", data), ("smooth", smooth)):
                vals = np.asarray(m, np.float64)[fin]
                assert np.all(np.isfinite(vals)) and np.all(vals >= 0)
                ref = math.fsum(vals.tolist())
                print(nx, ny, kind, key, t[key], ref, abs(t[key] - ref), n * 2.0 ** -52 * ref)
                assert abs(t[key] - ref) <= n * 2.0 ** -52 * ref, (nx, ny, kind, key, t[key], ref)
            for im in (dd, dw):
                if im is not None:
                    im.free()
        cv.free()


def test_invalid_arguments(ctx):
    C = np.zeros((4, 6, 5), F)
    cv = ctx.upload_volume(C, 0)
    d, small, two, w8 = ctx.upload_image(np.ones((4, 6), F)), ctx.new_image(5, 4), ctx.new_image(6, 4, 2), ctx.upload_image(np.ones((8, 4, 6), F))
    E = ctx.new_image(6, 4)

    def refused(fn):
        with pytest.raises(mgm_amd.MgmError) as e:
            fn()
        assert e.value.code == mgm_amd.MGM_ERR_INVALID, e.value

    refused(lambda: ctx.energy_dev(cv, d, 4, 1, 2))
    refused(lambda: ctx.energy_dev(cv, d, -1, 1, 2))
    refused(lambda: ctx.energy_dev(cv, d, 0, -1.0, 2))
    refused(lambda: ctx.energy_dev(cv, d, 0, INF, 2))
    refused(lambda: ctx.energy_dev(cv, d, 0, float("nan"), 2))
    refused(lambda: ctx.energy_dev(cv, d, 0, 1, -2.0))
    refused(lambda: ctx.energy_dev(cv, d, 0, 1, float("nan")))
    refused(lambda: ctx.energy_dev(cv, d, 3, 1, 2, connectivity=6))
    refused(lambda: ctx.energy_dev(cv, small, 0, 1, 2))
    refused(lambda: ctx.energy_dev(cv, two, 0, 1, 2))
    refused(lambda: ctx.energy_dev(cv, d, 3, 1, 2, w8=two))
    refused(lambda: ctx.energy_dev(cv, d, 3, 1, 2, w8=small))
    refused(lambda: ctx.energy_dev(cv, d, 0, 1, 2, want_map=False, want_totals=False))
    lib, q = ctx.lib, mgm_amd.EnergyParams(0, 1.0, 2.0, 4, 0, None)
    tot = mgm_amd.EnergyTotals()
    import ctypes
    assert lib.mgm_energy_dev(ctx.h, cv.h, d.h, ctypes.byref(q), d.h, None) == mgm_amd.MGM_ERR_INVALID       # E == d
    assert lib.mgm_energy_dev(ctx.h, cv.h, d.h, ctypes.byref(q), small.h, None) == mgm_amd.MGM_ERR_INVALID   # E of another size
    assert lib.mgm_energy_dev(ctx.h, None, d.h, ctypes.byref(q), E.h, None) == mgm_amd.MGM_ERR_INVALID
    assert lib.mgm_energy_dev(ctx.h, cv.h, None, ctypes.byref(q), E.h, None) == mgm_amd.MGM_ERR_INVALID
    assert lib.mgm_energy_dev(ctx.h, cv.h, d.h, None, E.h, ctypes.byref(tot)) == mgm_amd.MGM_ERR_INVALID
    # what is valid: P2 = +INF, P1 = 0, kinds 0-2 ignore connectivity and w8
    ctx.energy_dev(cv, d, 0, 0.0, INF, connectivity=0)[0].free()
    ctx.energy_dev(cv, d, 3, 0.0, INF, 8, 1, w8)[0].free()
    for o in (d, small, two, w8, E, cv):
        o.free()


def test_the_last_aggregation_is_left_alone(ctx):
    """mgm_wta_windowed_dev gives the same maps before and after energy calls, with and without totals"""
    nx, ny = 96, 40
    u, v, _ = pair(nx, ny)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    cv = ctx.costvolume_dev(du, dv, -40, 23, "none", "census", INF, 3)
    _, out, cost = ctx.aggregate_dev(cv, 2.0, 9.0, 8, 3, 0, 1, None, "vfit")
    lo, hi = ctx.upload_image(np.full((ny, nx), -20, F)), ctx.upload_image(np.full((ny, nx), 5, F))
    a, ac = ctx.wta_windowed_dev(cv, 8, 1, "none", lo, hi)
    before = (a.download(), ac.download())
    E, t = ctx.energy_dev(cv, a, 0, 2.0, 9.0)
    E3, _ = ctx.energy_dev(cv, out, 3, 2.0, 9.0, 8, want_totals=False)
    assert t["finite"] == nx * ny and math.isfinite(t["serial"])
    b, bc = ctx.wta_windowed_dev(cv, 8, 1, "none", lo, hi)
    assert same(before[0], b.download()) and same(before[1], bc.download())
    assert np.isfinite(E.download()).all()  # (an integer map inside the range of a census volume)
    for o in (du, dv, cv, out, cost, lo, hi, a, ac, b, bc, E, E3):
        o.free()
