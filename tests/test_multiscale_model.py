"""The coarse-to-fine (multiscale) mode, the part that needs no device: mgm_multiscale_levels (pure host arithmetic in
libmgm_hip.so) against the numpy model, the model's own invariants, and that header, binding and --help name the feature."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
import multiscale_model as msm
from helpers import ndiff
from oracle import oracle as orc_mod
from oracle import post

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def lib_levels(lib, nx, ny, vnx, vny, nscales):
    dims = (ctypes.c_int * 32)(*([-7] * 32))
    S = lib.mgm_multiscale_levels(nx, ny, vnx, vny, nscales, dims)
    return S, [tuple(dims[4 * s + k] for k in range(4)) for s in range(max(S, 0))], list(dims[4 * max(S, 0):])


def test_levels_against_the_model_for_every_small_size():
    lib = mgm_amd.load_library()  # (no context: the entry point must work without a device)
    sizes = [(nx, ny, nx, ny) for nx in range(1, 41) for ny in range(1, 41)]
    sizes += [(700, 500, 700, 500), (1920, 1080, 1920, 1080), (700, 500, 692, 500), (692, 500, 700, 500), (64, 64, 31, 64), (64, 64, 64, 33),
              (256, 192, 248, 192), (4097, 33, 4097, 33)]
    for nx, ny, vnx, vny in sizes:
        for nscales in range(0, 10):
            want = msm.levels(nx, ny, vnx, vny, nscales)
            S, dims, rest = lib_levels(lib, nx, ny, vnx, vny, nscales)
            if want is None:
                assert S == -mgm_amd.MGM_ERR_INVALID, (nx, ny, vnx, vny, nscales, S)
                continue
            assert S == len(want) and dims == want, (nx, ny, vnx, vny, nscales, S, dims, want)
            assert all(x == -7 for x in rest), "wrote past the levels that run"
            assert S >= 1 and (S == 1 or min(want[-1]) >= 16)
            assert lib.mgm_multiscale_levels(nx, ny, vnx, vny, nscales, None) == S  # dims may be NULL
    assert lib.mgm_multiscale_levels(0, 5, 5, 5, 2, None) == -mgm_amd.MGM_ERR_INVALID
    assert mgm_amd.multiscale_levels(700, 500, nscales=3) == [(700, 500, 700, 500), (350, 250, 350, 250), (175, 125, 175, 125)]
    assert mgm_amd.multiscale_levels(700, 500, 692, 500, nscales=8)[-1] == (22, 16, 22, 16)
    with pytest.raises(mgm_amd.MgmError):
        mgm_amd.multiscale_levels(700, 500, nscales=9)


def random_ranges(rng, ny, nx):
    lo = rng.integers(-90, 40, size=(ny, nx)).astype(F) + np.where(rng.random((ny, nx)) < 0.5, rng.random((ny, nx)), 0).astype(F)
    hi = lo + np.where(rng.random((ny, nx)) < 0.2, 0, rng.integers(0, 50, size=(ny, nx)) + rng.random((ny, nx))).astype(F)
    return lo.astype(F), hi.astype(F)


@pytest.mark.parametrize("shape", [(1, 1), (17, 1), (16, 16), (33, 17), (50, 70)])
def test_zoomed_out_ranges_contain_every_halved_fine_range(shape):
    ny, nx = shape
    lo, hi = random_ranges(np.random.default_rng(ny * 100 + nx), ny, nx)
    lo2, hi2 = msm.ranges_zoom_out(lo, hi)
    assert lo2.shape == (msm.half(ny), msm.half(nx)) and lo2.dtype == F
    ys, xs = (np.arange(ny) >> 1)[:, None], (np.arange(nx) >> 1)[None, :]
    assert np.all(lo2[ys, xs] <= F(0.5) * lo) and np.all(hi2[ys, xs] >= F(0.5) * hi)
    assert np.all(lo2 == np.floor(lo2)) and np.all(hi2 == np.ceil(hi2)) and np.all(lo2 <= hi2)


def test_zoom_out_is_the_2x2_mean_with_clamped_indices():
    rng = np.random.default_rng(4)
    img = (rng.random((3, 5, 7)) * 255).astype(F)
    z = msm.zoom_out(img)
    assert z.shape == (3, 3, 4) and z.dtype == F
    for c in range(3):
        for y in range(3):
            for x in range(4):
                x1, y1 = min(2 * x + 1, 6), min(2 * y + 1, 4)
                want = ((img[c, 2 * y, 2 * x] + img[c, 2 * y, x1]) + (img[c, y1, 2 * x] + img[c, y1, x1])) * F(0.25)
                assert z[c, y, x] == want
    assert np.array_equal(msm.zoom_out(np.full((1, 9, 9), 37.0, F)), np.full((1, 5, 5), 37.0, F))


def coarse_maps(rng, cny, cnx):
    d = (rng.integers(-60, 20, size=(cny, cnx)) + rng.random((cny, cnx))).astype(F)
    some = d.copy()
    some[rng.random((cny, cnx)) < 0.1] = np.nan
    single = np.full((cny, cnx), np.nan, F)
    single[cny // 2, cnx // 3] = F(-12.25)
    return dict(none=d, some=some, all=np.full((cny, cnx), np.nan, F), single=single)


@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (16, 16), (33, 17), (41, 58)])
@pytest.mark.parametrize("slack,radius", [(3, 2), (0, 0), (7, 16), (-3, 1)])
def test_fused_window_rule_equals_zoom_in_then_update(shape, slack, radius):
    ny, nx = shape
    rng = np.random.default_rng(ny * 1000 + nx + slack)
    lo, hi = random_ranges(rng, ny, nx)
    ref = orc_mod.RefPost() if orc_mod.RefPost.available() else None
    for kind, D in coarse_maps(rng, msm.half(ny), msm.half(nx)).items():
        a = msm.ranges_from_coarse(D, lo, hi, slack, radius)
        b = msm.ranges_from_coarse_fused(D, lo, hi, slack, radius)
        assert ndiff(a[0], b[0]) == 0 and ndiff(a[1], b[1]) == 0, (shape, kind, slack, radius)
        assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1])) and np.all(a[0] <= a[1])
        if kind == "all":  # nothing to go by: the base ranges stay
            assert ndiff(a[0], lo) == 0 and ndiff(a[1], hi) == 0
        if ref is not None:  # the compiled reference's update_dmin_dmax + its two remove_nonfinite calls on the zoomed-in map
            U = msm.zoom_in_prior(D, nx, ny)
            rl, rh = ref.update_ranges(U, lo, hi, slack, radius)
            assert ndiff(a[0], rl) == 0 and ndiff(a[1], rh) == 0, (shape, kind, slack, radius, "reference")


def test_vectorised_leftright_is_the_plain_loop_one():
    rng = np.random.default_rng(11)
    for ny, nx, onx in ((9, 31, 31), (7, 40, 32), (5, 16, 24)):
        d = (rng.integers(-12, 12, size=(ny, nx)) + rng.random((ny, nx))).astype(F)
        o = (rng.integers(-12, 12, size=(ny, onx)) + rng.random((ny, onx))).astype(F)
        d[rng.random(d.shape) < 0.1] = np.nan
        o[rng.random(o.shape) < 0.1] = np.nan
        d[0, 0], o[0, 1], d[1, 1] = np.inf, -np.inf, F(3e9)
        for tau in (1.0, 2.5):
            assert ndiff(msm.leftright(d, o, tau), post.leftright(d, o, tau)) == 0


def test_header_binding_and_help_name_the_feature():
    hdr = open(os.path.join(ROOT, "include", "mgm_hip.h")).read()
    names = ["mgm_multiscale_levels", "mgm_zoom_out_dev", "mgm_ranges_zoom_out_dev", "mgm_ranges_from_coarse_dev", "mgm_multiscale_pair_dev"]
    for n in names:
        assert n in hdr and n in mgm_amd.ABI_SYMBOLS, n
    assert "struct_size" in hdr and "mgm_ms_params" in hdr
    for n in ("zoom_out_dev", "ranges_zoom_out_dev", "ranges_from_coarse_dev", "multiscale_pair"):
        assert callable(getattr(mgm_amd.Context, n)), n
    assert callable(mgm_amd.multiscale_levels)
    assert ctypes.sizeof(mgm_amd.MsParams) >= 100 and mgm_amd.MsParams._fields_[0][0] == "struct_size"
    exe = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "-S nscales" in r.stdout and "MGM_MS_SLACK" in r.stdout and "MGM_MS_RADIUS" in r.stdout
    bad = subprocess.run([exe, "-S", "9", "a.png", "b.png", "c.tif"], capture_output=True, text=True)
    assert bad.returncode == 1 and "-S" in bad.stderr
