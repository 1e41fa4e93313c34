"""The numpy model of the speckle filter (tests/speckle_model.py) against a naive flood fill written on its own, the
invariants the definition promises, SciPy's labelling of the finite mask where SciPy is installed, what the binding, the header
and --help expose, the command line's refusals, and -- on the oracle's final map of the pair the GPU command-line test uses --
the maxsize that test filters with."""
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
from helpers import ndiff
from mgm_amd import synth
from speckle_model import CLI_MAXDIFF, CLI_MAXSIZE, PAIR, crafted, labels, maxsizes, sizes, speckle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
f32 = np.float32
SHAPES = [(1, 1), (1, 9), (7, 1), (3, 4), (17, 5), (40, 23)]  # (nx, ny)


def same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


def flood(d, maxdiff):
    """The definition with a stack: sizes [ny][nx], 0 on invalid pixels."""
    d = np.asarray(d, np.float32)
    ny, nx = d.shape
    size = np.zeros((ny, nx), np.int64)
    seen = np.zeros((ny, nx), bool)
    md = f32(maxdiff)
    with np.errstate(all="ignore"):
        for y0 in range(ny):
            for x0 in range(nx):
                if seen[y0, x0] or not np.isfinite(d[y0, x0]):
                    continue
                seen[y0, x0] = True
                stack, comp = [(x0, y0)], []
                while stack:
                    x, y = stack.pop()
                    comp.append((x, y))
                    for qx, qy in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
                        if 0 <= qx < nx and 0 <= qy < ny and not seen[qy, qx] and np.isfinite(d[qy, qx]) \
                                and abs(f32(d[y, x] - d[qy, qx])) <= md:
                            seen[qy, qx] = True
                            stack.append((qx, qy))
                for x, y in comp:
                    size[y, x] = len(comp)
    return size


def random_maps(n=300):
    rng = np.random.default_rng(77)
    for k in range(n):
        nx, ny = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        levels = np.array([0.0, 1.0, 2.5, 4.0, -0.0, 7.0], np.float32)[: int(rng.integers(2, 7))]
        d = rng.choice(levels, size=(ny, nx))
        d[rng.random((ny, nx)) < rng.choice([0.0, 0.2, 0.6])] = np.nan
        if k % 7 == 0:
            d[rng.random((ny, nx)) < 0.05] = np.inf
        yield d, float(rng.choice([0.0, 1.0, 1.5, 3.0, np.inf]))


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_model_matches_the_flood_fill_on_the_crafted_maps(nx, ny):
    for name, d, maxdiff in crafted(nx, ny, tw=8, th=4):
        assert np.array_equal(sizes(d, maxdiff), flood(d, maxdiff)), name


def test_model_matches_the_flood_fill_on_random_maps():
    n = 0
    for d, maxdiff in random_maps():
        assert np.array_equal(sizes(d, maxdiff), flood(d, maxdiff)), (d.shape, maxdiff)
        n += 1
    assert n == 300


def test_what_the_crafted_maps_are_there_for():
    nx, ny = 40, 23
    c = {name: (d, md) for name, d, md in crafted(nx, ny, tw=8, th=4)}
    sz = {name: sizes(d, md) for name, (d, md) in c.items()}
    assert (sz["one_component"] == nx * ny).all() and (sz["all_nan"] == 0).all() and (sz["checkerboard"] == 1).all()
    for name in ("serpentine_rows", "serpentine_columns", "spiral"):  # ONE path, long, one pixel wide
        fin = np.isfinite(c[name][0])
        assert fin.sum() > (nx * ny) // 3 and (sz[name][fin] == fin.sum()).all(), name
    assert sz["tile_corners"].max() == 8 * 4                      # blocks that touch at corners stay apart
    assert sorted(set(sz["wall"].ravel())) == [0, 19 * ny, 20 * ny] and sz["wall_with_gap"].max() == nx * ny - ny + 1
    assert (sz["ramp_step_equals_maxdiff"] == nx).all() and (sz["ramp_step_above_maxdiff"] == 1).all()  # chained; split
    assert (sz["zeros_of_both_signs"] == nx * ny).all()
    assert 1 < sz["denormals"].max() < nx * ny                    # joined at one denormal step, not at two
    assert sorted(set(sz["infinities_split"].ravel())) == sorted({0, 20 * 11, 19 * 11})
    assert (sz["overflow_finite_maxdiff"] == 1).all() and (sz["overflow_infinite_maxdiff"] == nx * ny).all()


def test_invariants():
    maps = [(d, md) for nx, ny in ((17, 5), (40, 23)) for _, d, md in crafted(nx, ny, tw=8, th=4)] + list(random_maps(40))
    for d, maxdiff in maps:
        size = sizes(d, maxdiff)
        fin = np.isfinite(d)
        # no traversal order: transposed and flipped maps give the transposed and flipped sizes (and so the same outputs)
        for fwd in (lambda a: a.T, lambda a: a[::-1], lambda a: a[:, ::-1], lambda a: a[::-1, ::-1].T):
            assert np.array_equal(sizes(np.ascontiguousarray(fwd(d)), maxdiff), fwd(size))
        for maxsize in maxsizes(size, d.size) + [5]:
            out, sm = speckle(d, maxsize, maxdiff, size=size)
            assert same(out[~fin], d[~fin]) and (sm[~fin] == 0).all() and (sm[fin] >= 1).all()
            stay = fin & ~np.isnan(out)
            assert np.array_equal(np.isnan(out[fin]), size[fin] <= maxsize) and same(out[stay], d[stay])
            if maxsize == 0:
                assert out.tobytes() == np.asarray(d, np.float32).tobytes()
            # idempotent: the components that stay are the components they were
            again, sm2 = speckle(out, maxsize, maxdiff)
            assert same(again, out) and np.array_equal(sm2[stay], sm[stay])
        with np.errstate(all="ignore"):
            assert np.array_equal(sizes(d, np.inf), sizes(np.where(fin, 0.0, np.nan), 0.0))  # +INF: the finite mask's components


def test_the_chained_ramp_is_one_component_and_goes_at_its_exact_size():
    N = 50
    d = np.arange(N + 1, dtype=np.float32)[None, :]
    assert (sizes(d, 1.0) == N + 1).all() and (sizes(d, 0.5) == 1).all()
    assert np.isnan(speckle(d, N + 1, 1.0)[0]).all() and same(speckle(d, N, 1.0)[0], d)


def test_sizes_are_scipys_for_an_infinite_maxdiff():
    ndimage = pytest.importorskip("scipy.ndimage")
    maps = [d for _, d, _ in crafted(40, 23, tw=8, th=4)] + [d for d, _ in random_maps(60)]
    for d in maps:
        fin = np.isfinite(d)
        lab, n = ndimage.label(fin)  # (4-connectivity is its default structure)
        want = np.where(fin, np.bincount(lab.ravel(), minlength=n + 1)[lab], 0)
        assert np.array_equal(sizes(d, np.inf), want)


def test_binding_and_header_list_the_entry_point():
    assert "mgm_speckle_dev" in mgm_amd.ABI_SYMBOLS
    assert "mgm_speckle_dev(" in open(os.path.join(ROOT, "include", "mgm_hip.h")).read()
    assert callable(getattr(mgm_amd.Context, "speckle_dev", None))
    assert hasattr(mgm_amd.load_library(), "mgm_speckle_dev")


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


def test_help_states_the_step():
    r = run_cli(["--help"], {})
    assert r.returncode == 0
    for word in ("MGM_SPECKLE=0", "MGM_SPECKLE_DIFF=1", "after MEDIAN and the left-right test", "before the back-projected image"):
        assert word in r.stdout, word


@pytest.mark.parametrize("env,word", [({"MGM_SPECKLE": "-1"}, "MGM_SPECKLE must"), ({"MGM_SPECKLE": "2.5"}, "MGM_SPECKLE must"),
                                      ({"MGM_SPECKLE": "nan"}, "MGM_SPECKLE must"), ({"MGM_SPECKLE": "many"}, "MGM_SPECKLE must"),
                                      ({"MGM_SPECKLE": "3000000000"}, "MGM_SPECKLE must"),
                                      ({"MGM_SPECKLE": "5", "MGM_SPECKLE_DIFF": "-0.5"}, "MGM_SPECKLE_DIFF must"),
                                      ({"MGM_SPECKLE": "5", "MGM_SPECKLE_DIFF": "nan"}, "MGM_SPECKLE_DIFF must"),
                                      ({"MGM_SPECKLE_DIFF": "1x"}, "MGM_SPECKLE_DIFF must")])
def test_cli_refuses_bad_parameters_before_any_work(env, word):
    """Exit code 1 and one line on stderr when the command line is parsed: no device, no input file."""
    r = run_cli(["no_u.png", "no_v.png", "no_out.tif"], env)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.splitlines()) == 1 and r.stdout == ""


def test_the_maxsize_of_the_command_line_test_removes_a_visible_part(oracle):
    """The oracle's final left map of the 96 x 64 synthetic census pair (vfit, 8 directions, both runs, the left-right test at
    tau 1) and the model at CLI_MAXSIZE / CLI_MAXDIFF: the filter must remove at least one valid pixel and at most half of them,
    or the command-line comparison on the GPU would compare maps the filter never touched (or emptied)."""
    from multiscale_model import leftright
    p = PAIR
    u, v, _ = synth.stereo_pair(p["nx"], p["ny"], p["dmin"], p["dmax"])
    maps = []
    for a, b, lo, hi in ((u, v, p["dmin"], p["dmax"]), (v, u, -p["dmax"], -p["dmin"])):
        Cv = oracle.costvolume(a, b, lo, hi, "none", "census")
        S, out, outc = oracle.mgm(Cv, lo, p["P1"], p["P2"], p["NDIR"], p["TSGM"])
        maps.append(oracle.refine(S, lo, "vfit", out, outc)[0])
    final = leftright(maps[0], maps[1], 1.0)
    valid = np.isfinite(final)
    size = sizes(final, CLI_MAXDIFF)
    out, _ = speckle(final, CLI_MAXSIZE, CLI_MAXDIFF, size=size)
    removed = valid & np.isnan(out)
    share = removed.sum() / valid.sum()
    print("valid pixels: %d of %d; components: %d; removed at maxsize %d: %d pixels, share %.4f"
          % (valid.sum(), valid.size, len(np.unique(labels(final, CLI_MAXDIFF)[valid])), CLI_MAXSIZE, removed.sum(), share))
    assert valid.sum() > valid.size // 2
    assert removed.sum() >= 1 and share <= 0.5
