"""The numpy model of hole filling (tests/holes_model.py) against plain loops that march every ray, the properties
the definition promises, the direction table (a star around one valid pixel), the maxdist bound, what the binding, the header and
--help expose, the command line's refusals, and -- on the oracle's final map of the pair the GPU command-line test uses -- the
condition that makes that test mean something."""
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
from holes_model import CLI_ARGS, CLI_RUNS, CLI_SPECKLE, MODES, PAIR, STEPS, crafted, fill, rays, same_bits
from mgm_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
f32 = np.float32
SHAPES = [(1, 1), (1, 9), (7, 1), (3, 4), (12, 9), (9, 12)]  # (nx, ny), at most 12 x 9 pixels
DIRS = (2, 4, 8)
DISTS = (0, 1, 2, 5)


def march(d, mode, dirs, maxdist):
    """The definition with loops: every hole marches every ray."""
    d = np.ascontiguousarray(d, np.float32)
    ny, nx = d.shape
    out, filled = d.copy(), np.zeros((ny, nx), np.float32)
    for y in range(ny):
        for x in range(nx):
            if np.isfinite(d[y, x]):
                continue
            cands = []
            for k in range(dirs):
                sx, sy = STEPS[k]
                t = 1
                while 0 <= x + t * sx < nx and 0 <= y + t * sy < ny and (maxdist == 0 or t <= maxdist):
                    q = d[y + t * sy, x + t * sx]
                    if np.isfinite(q):
                        cands.append(q)
                        break
                    t += 1
            if not cands:
                continue
            # a stable sort of the candidates taken in direction order: insertion, an element moves past strictly larger ones only
            v = []
            for c in cands:
                i = len(v)
                while i > 0 and v[i - 1] > c:
                    i -= 1
                v.insert(i, c)
            out[y, x] = {"min": v[0], "max": v[-1], "median": v[len(v) // 2]}[mode]
            filled[y, x] = 1
    return out, filled


def small_maps():
    """(name, d): the crafted maps of every small shape, and random ones with +-INF holes and zeros of both signs"""
    for nx, ny in SHAPES:
        for name, d in crafted(nx, ny, chunk=4, band=3):
            yield "%s %dx%d" % (name, nx, ny), d
    rng = np.random.default_rng(11)
    for k in range(40):
        nx, ny = int(rng.integers(1, 13)), int(rng.integers(1, 10))
        d = rng.choice(np.array([0.0, -0.0, 1.0, 2.5, -3.0], np.float32), size=(ny, nx))
        d[rng.random((ny, nx)) < rng.choice([0.2, 0.5, 0.85])] = np.nan
        d[rng.random((ny, nx)) < 0.08] = np.inf if k % 2 else -np.inf
        yield "random %d" % k, d


def test_model_matches_the_marched_rays():
    n = 0
    names = set()
    for name, d in small_maps():
        assert d.shape[1] <= 12 and d.shape[0] <= 12
        r = rays(d)
        names.add(name.split()[0])
        for mode in MODES:
            for dirs in DIRS:
                for maxdist in DISTS:
                    want = march(d, mode, dirs, maxdist)
                    got = fill(d, mode, dirs, maxdist, r=r)
                    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (name, mode, dirs, maxdist)
                    n += 1
    assert {"all_nan", "all_valid", "zeros_of_both_signs", "payloads_and_infinities", "unreachable_payloads", "random"} <= names
    assert n == (6 * len(crafted(3, 4)) + 40) * 36


def test_the_tie_rule_decides_the_bits():
    """A hole between -0 (to its right: direction 0) and +0 (to its left: direction 1): equal values, so direction 0's candidate comes
    first.  min takes -0, max and the (upper) median take +0; with the two swapped it is the other way round."""
    neg, pos = f32(-0.0), f32(0.0)
    for left, right in ((pos, neg), (neg, pos)):
        d = np.array([[left, np.nan, right]], np.float32)
        for mode, want in (("min", right), ("max", left), ("median", left)):
            for fn in (fill, march):
                got = fn(d, mode, 2, 0)[0][0, 1]
                assert got == 0 and np.signbit(got) == np.signbit(want), (mode, fn.__name__)
    # the crafted map of both zeros has holes whose candidates are zeros of both signs
    d = dict(crafted(12, 9, 4, 3))["zeros_of_both_signs"]
    o_min, o_max = fill(d, "min")[0], fill(d, "max")[0]
    assert (np.signbit(o_min) != np.signbit(o_max)).any() and (o_min[np.isnan(d)] == 0).all()


def test_properties():
    maps = [d for nx, ny in ((12, 9), (40, 23)) for _, d in crafted(nx, ny, chunk=8, band=4)]
    for d in maps:
        hole = ~np.isfinite(d)
        r = rays(d)
        # no traversal order: the transposed and the flipped map give the transposed and flipped result, with the directions renamed
        for fwd, perm in ((lambda a: a[:, ::-1], (1, 0, 2, 3, 5, 4, 7, 6)), (lambda a: a[::-1], (0, 1, 3, 2, 6, 7, 4, 5))):
            c2, t2 = rays(np.ascontiguousarray(fwd(d)))
            for k in range(8):
                assert np.array_equal(fwd(r[1][k]), t2[perm[k]]) and np.array_equal(fwd(r[0][k])[t2[perm[k]] > 0], c2[perm[k]][t2[perm[k]] > 0])
        for mode in MODES:
            res = {(dirs, md): fill(d, mode, dirs, md, r=r) for dirs in DIRS for md in (0, 1, 2, 5, 40)}
            for (dirs, md), (out, filled) in res.items():
                assert same_bits(out[~hole], d[~hole]) and (filled[~hole] == 0).all()          # valid pixels: copied
                stay = hole & (filled == 0)
                assert same_bits(out[stay], d[stay])                                           # holes without a candidate: their bits
                got = out[filled == 1]
                assert np.isfinite(got).all() and np.isin(got.view(np.uint32), d[~hole].view(np.uint32)).all()  # one of the input's values
            for md in (0, 1, 2, 5, 40):                                                        # the filled set grows with dirs ...
                assert (res[(2, md)][1] <= res[(4, md)][1]).all() and (res[(4, md)][1] <= res[(8, md)][1]).all()
            for dirs in DIRS:                                                                  # ... and with maxdist; 0 holds them all
                for a, b in ((1, 2), (2, 5), (5, 40), (40, 0)):
                    assert (res[(dirs, a)][1] <= res[(dirs, b)][1]).all()
        for dirs in DIRS:
            for md in (0, 2):
                lo, mid, hi = (fill(d, m, dirs, md, r=r)[0] for m in ("min", "median", "max"))
                got = fill(d, "min", dirs, md, r=r)[1] == 1
                assert (lo[got] <= mid[got]).all() and (mid[got] <= hi[got]).all()
    # a map without holes comes back bit for bit
    d = dict(crafted(12, 9, 4, 3))["all_valid"]
    for mode in MODES:
        out, filled = fill(d, mode)
        assert same_bits(out, d) and (filled == 0).all()


def test_not_idempotent():
    """dirs = 2 fills a row's holes from its row only: a second application with 4 directions ... and even the same application again
    may fill more.  One valid pixel in a corner: the first application fills its row, column and diagonal, the second everything."""
    d = np.full((5, 6), np.nan, np.float32)
    d[0, 0] = 3.0
    once, f1 = fill(d, "median", 8, 0)
    twice, f2 = fill(once, "median", 8, 0)
    assert 0 < f1.sum() < d.size - 1 and np.isnan(once).any() and not np.isnan(twice).any() and f2.sum() > 0


def star(nx, ny, x, y, dirs):
    """the pixels that lie on one of the first `dirs` rays THROUGH (x, y): p + t * step_k = (x, y) for a t >= 1"""
    m = np.zeros((ny, nx), bool)
    for sx, sy in STEPS[:dirs]:
        t = 1
        while 0 <= x - t * sx < nx and 0 <= y - t * sy < ny:
            m[y - t * sy, x - t * sx] = True
            t += 1
    return m


@pytest.mark.parametrize("nx,ny", [(11, 9), (12, 9), (5, 9)])
def test_the_star_pins_the_direction_table(nx, ny):
    for x, y in ((nx // 2, ny // 2), (0, 0), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)):
        d = np.full((ny, nx), np.nan, np.float32)
        d[y, x] = 4.5
        for dirs in DIRS:
            for mode in MODES:
                out, filled = fill(d, mode, dirs, 0)
                want = star(nx, ny, x, y, dirs)
                assert np.array_equal(filled == 1, want), (x, y, dirs)
                rest = ~want
                rest[y, x] = False
                assert (out[want] == 4.5).all() and out[y, x] == 4.5 and np.isnan(out[rest]).all()
        # each direction on its own: direction k serves exactly the pixels p with p + t * step_k = (x, y)
        cand, dist = rays(d)
        for k, (sx, sy) in enumerate(STEPS):
            want = np.zeros((ny, nx), np.int64)
            t = 1
            while 0 <= x - t * sx < nx and 0 <= y - t * sy < ny:
                want[y - t * sy, x - t * sx] = t
                t += 1
            assert np.array_equal(dist[k], want), k


def test_maxdist_is_the_last_distance_that_fills():
    for k, (sx, sy) in enumerate(STEPS):
        for maxdist in (1, 2, 5):
            n = 2 * maxdist + 5
            d = np.full((n, n), np.nan, np.float32)
            c = n // 2
            d[c, c] = 2.0
            dirs = 2 if k < 2 else (4 if k < 4 else 8)
            filled = fill(d, "median", dirs, maxdist)[1]
            at, beyond = (c - maxdist * sx, c - maxdist * sy), (c - (maxdist + 1) * sx, c - (maxdist + 1) * sy)
            assert filled[at[1], at[0]] == 1 and filled[beyond[1], beyond[0]] == 0, (k, maxdist)
            assert fill(d, "median", dirs, 0)[1][beyond[1], beyond[0]] == 1


def test_binding_and_header_list_the_entry_point():
    import inspect
    assert "mgm_fill_holes_dev" in mgm_amd.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "mgm_hip.h")).read()
    assert "mgm_fill_holes_dev(mgm_ctx *ctx, const mgm_img *d, const char *mode, int dirs, int maxdist" in hdr
    fn = getattr(mgm_amd.Context, "fill_holes_dev", None)
    assert callable(fn)
    assert list(inspect.signature(fn).parameters)[1:] == ["d", "mode", "dirs", "maxdist", "out", "want_filled"]
    assert hasattr(mgm_amd.load_library(), "mgm_fill_holes_dev")


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


def test_help_states_the_step():
    r = run_cli(["--help"], {})
    assert r.returncode == 0
    for word in ("MGM_FILL_HOLES=none", "MGM_FILL_HOLES_DIRS=8", "MGM_FILL_HOLES_DIST=0", "after MGM_SPECKLE", "before the back-projected image",
                 "(+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,+1) (+1,-1) (-1,-1)"):
        assert word in r.stdout, word


@pytest.mark.parametrize("env,word", [({"MGM_FILL_HOLES": "mean"}, "MGM_FILL_HOLES must"), ({"MGM_FILL_HOLES": "1"}, "MGM_FILL_HOLES must"),
                                      ({"MGM_FILL_HOLES": "Median"}, "MGM_FILL_HOLES must"),
                                      ({"MGM_FILL_HOLES": "median", "MGM_FILL_HOLES_DIRS": "3"}, "MGM_FILL_HOLES_DIRS must"),
                                      ({"MGM_FILL_HOLES": "median", "MGM_FILL_HOLES_DIRS": "16"}, "MGM_FILL_HOLES_DIRS must"),
                                      ({"MGM_FILL_HOLES_DIRS": "eight"}, "MGM_FILL_HOLES_DIRS must"),
                                      ({"MGM_FILL_HOLES_DIRS": "8x"}, "MGM_FILL_HOLES_DIRS must"),
                                      ({"MGM_FILL_HOLES": "min", "MGM_FILL_HOLES_DIST": "-1"}, "MGM_FILL_HOLES_DIST must"),
                                      ({"MGM_FILL_HOLES": "min", "MGM_FILL_HOLES_DIST": "2.5"}, "MGM_FILL_HOLES_DIST must"),
                                      ({"MGM_FILL_HOLES": "min", "MGM_FILL_HOLES_DIST": "nan"}, "MGM_FILL_HOLES_DIST must"),
                                      ({"MGM_FILL_HOLES_DIST": "3000000000"}, "MGM_FILL_HOLES_DIST must")])
def test_cli_refuses_bad_parameters_before_any_work(env, word):
    """Exit code 1 and one line on stderr when the command line is parsed: no device, no input file."""
    r = run_cli(["no_u.png", "no_v.png", "no_out.tif"], env)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.splitlines()) == 1 and r.stdout == ""


def test_the_command_line_test_fills_a_visible_part(oracle):
    """The oracle's final left map of the 96 x 64 synthetic census pair (no refinement, 8 directions, both runs, the left-right test at tau 1),
    the speckle model at 100 / 1, then the fills the GPU command-line test runs: without these conditions that test could pass on
    maps the step never touched."""
    from multiscale_model import leftright
    from speckle_model import speckle
    p = PAIR
    u, v, _ = synth.stereo_pair(p["nx"], p["ny"], p["dmin"], p["dmax"])
    maps = []
    for a, b, lo, hi in ((u, v, p["dmin"], p["dmax"]), (v, u, -p["dmax"], -p["dmin"])):
        Cv = oracle.costvolume(a, b, lo, hi, "none", "census")
        S, out, outc = oracle.mgm(Cv, lo, p["P1"], p["P2"], p["NDIR"], p["TSGM"])
        maps.append(out)  # (CLI_ARGS: -s none)
    lr = leftright(maps[0], maps[1], 1.0)
    final = speckle(lr, CLI_SPECKLE, 1.0)[0]
    hole = ~np.isfinite(final)
    r = rays(final)
    base, fbase = fill(final, "median", 8, 0, r=r)
    near, fnear = fill(final, "median", 8, 3, r=r)
    left = hole & (fnear == 0)
    differ = {name: int((fill(final, mode, dirs, 0, r=r)[0].view(np.uint32) != base.view(np.uint32)).sum())
              for name, mode, dirs in (("min", "min", 8), ("max", "max", 8), ("dirs=2", "median", 2))}
    print("holes after the left-right test: %d of %d; after the speckle filter: %d (%.2f %%); unfilled at maxdist 3: %d (%.2f %%); "
          "differ from median / 8 / 0: %s" % ((~np.isfinite(lr)).sum(), hole.size, hole.sum(), 100.0 * hole.mean(), left.sum(),
                                             100.0 * left.sum() / hole.size, differ))
    assert CLI_RUNS == (("median", 8, 0), ("min", 2, 0), ("median", 8, 3)) and "-s none" in CLI_ARGS and "-t census" in CLI_ARGS
    assert 0.02 <= hole.mean() <= 0.40
    assert (fbase[hole] == 1).all() and np.isfinite(base).all()
    assert 0 < left.sum() < hole.sum()
    assert all(n >= 50 for n in differ.values()), differ
