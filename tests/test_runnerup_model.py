"""The numpy model of the runner-up search and the uniqueness filter (tests/runnerup_model.py) against a plain
restatement of the definition, its invariants, what the binding, the header and --help expose, the command line's refusals, and
-- on the oracle's S of the pair the GPU command-line test uses -- the ratio that test filters with."""
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
from helpers import ndiff
from mgm_amd import synth
from runnerup_model import CLI_RADIUS, CLI_RATIO, PAIR, confidence, runnerup, uniqueness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
f32 = np.float32


def same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


def loops(S, dmin, radius):
    """The definition, pixel by pixel and label by label."""
    ny, nx, L = S.shape
    out2, out1 = np.full((ny, nx), np.nan, np.float32), np.full((ny, nx), np.nan, np.float32)
    cost2, cost1 = np.full((ny, nx), np.inf, np.float32), np.full((ny, nx), np.inf, np.float32)
    for y in range(ny):
        for x in range(nx):
            best, o1 = f32(np.inf), None
            for o in range(L):
                if np.isfinite(S[y, x, o]) and best > S[y, x, o]:
                    best, o1 = S[y, x, o], o
            if o1 is None:
                continue
            out1[y, x], cost1[y, x] = f32(o1 + dmin), best
            best, o2 = f32(np.inf), None
            for o in range(L):
                if abs(o - o1) > radius and np.isfinite(S[y, x, o]) and best > S[y, x, o]:
                    best, o2 = S[y, x, o], o
            if o2 is not None:
                out2[y, x], cost2[y, x] = f32(o2 + dmin), best
    return out2, cost2, out1, cost1


def volumes():
    rng = np.random.default_rng(23)
    cases = []
    for nx, ny, L, dmin in [(9, 3, 7, -3), (9, 3, 7, 2), (4, 2, 7, -9), (5, 1, 1, 0), (5, 2, 2, -1), (6, 2, 3, -1), (8, 2, 4, 5), (7, 2, 6, -2)]:
        S = (rng.integers(0, 4, (ny, nx, L)) - 1).astype(np.float32)   # few values, some negative: ties everywhere
        S[rng.random(S.shape) < 0.15] = np.inf
        S[rng.random(S.shape) < 0.05] = np.nan
        S[rng.random(S.shape) < 0.05] = -np.inf
        S[0, 0] = np.inf                                               # an all-INF pixel
        S[0, 1] = np.inf
        S[0, 1, L // 2] = 3.0                                          # a pixel with a single finite entry
        cases.append((S, dmin))
        cases.append(((rng.random((ny, nx, L)) * 50 - 5).astype(np.float32), dmin))
    return cases


@pytest.mark.parametrize("radius", [0, 1, 2, "L", "L+3"])
def test_model_equals_the_definition(radius):
    none = single = tie = False
    for S, dmin in volumes():
        L = S.shape[2]
        r = {"L": L, "L+3": L + 3}.get(radius, radius)
        got, want = runnerup(S, dmin, r), loops(S, dmin, r)
        for g, w in zip(got, want):
            assert same(g, w)
        o2, c2, o1, c1 = want
        none |= bool(np.isnan(o1).any())
        single |= bool((~np.isnan(o1) & np.isnan(o2)).any())
        m = np.where(np.isfinite(S), S, np.inf)
        tie |= bool(((m == m.min(axis=2, keepdims=True)) & np.isfinite(m)).sum(axis=2).max() > 1)
        if r >= L:
            assert np.isnan(o2).all() and np.isposinf(c2).all()
        # no winner: NaN / +INF four times
        nw = np.isnan(o1)
        assert np.isposinf(c1[nw]).all() and np.isnan(o2[nw]).all() and np.isposinf(c2[nw]).all()
    assert none and single and tie


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_properties(radius):
    for S, dmin in volumes():
        o2, c2, o1, c1 = runnerup(S, dmin, radius)
        has2 = ~np.isnan(o2)
        assert (c2[has2] >= c1[has2]).all() and np.isfinite(c2[has2]).all()
        assert (np.abs(o2[has2] - o1[has2]) > radius).all()
        conf = confidence(c1, c2)
        dom = (c1 >= 0) & np.isfinite(c2) & (c2 > 0)
        assert ((conf[dom] >= 0) & (conf[dom] <= 1)).all()
        assert (conf[~np.isnan(o1) & np.isnan(o2)] == 1).all()     # no runner-up: 1
        assert np.isnan(conf[np.isnan(o1)]).all()                   # no winner: INF / INF
        if radius == 0:  # the second entry of a stable sort of the finite entries
            for y, x in np.ndindex(S.shape[:2]):
                fin = np.flatnonzero(np.isfinite(S[y, x]))
                order = fin[np.argsort(S[y, x, fin], kind="stable")]
                if len(order) >= 1:
                    assert o1[y, x] == order[0] + dmin
                if len(order) >= 2:
                    assert o2[y, x] == order[1] + dmin and c2[y, x] == S[y, x, order[1]]
                else:
                    assert np.isnan(o2[y, x])


def test_uniqueness_on_crafted_values():
    nan, inf = f32(np.nan), f32(np.inf)
    #              plain  conf==ratio  just below  0/0   INF/INF  no r.-up  negative costs   cost2 = 0    NaN d
    c1 = np.array([[1.0,  3.0,         3.0001,     0.0,  inf,     2.0,      -4.0,   -1.0,    -1.0,        1.0]], np.float32)
    c2 = np.array([[2.0,  4.0,         4.0,        0.0,  inf,     inf,      -2.0,   3.0,     0.0,         8.0]], np.float32)
    d = np.array([[5.0,   6.0,         7.0,        8.0,  nan,     9.0,      10.0,   11.0,    12.0,        nan]], np.float32)
    out, conf = uniqueness(d, c1, c2, 0.25)
    assert conf[0, 0] == 0.5 and conf[0, 1] == 0.25 and conf[0, 2] < 0.25 and np.isnan(conf[0, 3]) and np.isnan(conf[0, 4])
    assert conf[0, 5] == 1 and conf[0, 6] == -1 and conf[0, 7] > 1 and conf[0, 8] == inf
    keep = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1, 1], bool)
    assert np.array_equal(np.isnan(out[0]), ~keep | np.isnan(d[0]))
    assert np.array_equal(out[0][keep & ~np.isnan(d[0])], d[0][keep & ~np.isnan(d[0])])
    out0, _ = uniqueness(d, c1, c2, 0.0)     # ratio 0 rejects negative confidences only
    assert np.array_equal(np.isnan(out0[0]), np.isnan(d[0]) | (conf[0] < 0))


def test_binding_and_header_list_the_entry_points():
    for name in ("mgm_wta_runnerup_dev", "mgm_uniqueness_dev"):
        assert name in mgm_amd.ABI_SYMBOLS
        assert name + "(" in open(os.path.join(ROOT, "include", "mgm_hip.h")).read()
    assert callable(getattr(mgm_amd.Context, "wta_runnerup_dev", None)) and callable(getattr(mgm_amd.Context, "uniqueness_dev", None))
    lib = mgm_amd.load_library()
    assert hasattr(lib, "mgm_wta_runnerup_dev") and hasattr(lib, "mgm_uniqueness_dev")


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


def test_help_states_the_mode():
    r = run_cli(["--help"], {})
    assert r.returncode == 0
    for word in ("-c FILE", "MGM_UNIQUENESS=0", "MGM_UNIQUENESS_RADIUS=1", "only the left map is filtered"):
        assert word in r.stdout, word


@pytest.mark.parametrize("how", [["-c", "conf.tif"], "env"])
@pytest.mark.parametrize("args,env", [(["-S", "2"], {}), ([], {"TSGM_ITER": "2"}), ([], {"MGM_DEVICES": "0,1"}), (["-m", "lo.tif", "-M", "hi.tif"], {})])
def test_cli_refuses_what_the_mode_does_not_combine_with(args, env, how):
    """Exit code 2 and one line on stderr, before any device or input file is touched."""
    opts, env = (how, env) if how != "env" else ([], dict(env, MGM_UNIQUENESS="0.25"))
    r = run_cli(opts + args + ["no_u.png", "no_v.png", "no_out.tif"], env)
    assert r.returncode == 2 and "-c / MGM_UNIQUENESS does not combine with" in r.stderr and len(r.stderr.splitlines()) == 1


@pytest.mark.parametrize("env,word", [({"MGM_UNIQUENESS": "1.5"}, "MGM_UNIQUENESS must"), ({"MGM_UNIQUENESS": "-0.1"}, "MGM_UNIQUENESS must"),
                                      ({"MGM_UNIQUENESS": "nan"}, "MGM_UNIQUENESS must"),
                                      ({"MGM_UNIQUENESS": "0.5", "MGM_UNIQUENESS_RADIUS": "-1"}, "MGM_UNIQUENESS_RADIUS must")])
def test_cli_refuses_bad_parameters_before_any_work(env, word):
    """Exit code 1 and one line on stderr when the command line is parsed: no device, no input file."""
    r = run_cli(["no_u.png", "no_v.png", "no_out.tif"], env)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.splitlines()) == 1 and r.stdout == ""


def test_the_ratio_of_the_command_line_test_rejects_a_visible_part(oracle):
    """The oracle's S of the 96 x 40 synthetic census pair, the model's search at radius 1 and the filter at CLI_RATIO = 0.25: the
    filter must reject between 1 % and 50 % of the pixels that have a winner, or the command-line comparison on the GPU would
    compare maps the filter never touched (or emptied).  Measured: every pixel has a winner, 82 of the 3840 have no runner-up
    (conf = 1), and 0.0839 of them (322 pixels) fall below 0.25 and are rejected; at 0.125 it would be 0.043, at 0.3 0.107."""
    p = PAIR
    u, v, _ = synth.stereo_pair(p["nx"], p["ny"], p["dmin"], p["dmax"])
    C = oracle.costvolume(u, v, p["dmin"], p["dmax"], "none", "census")
    S, _, _ = oracle.mgm(C, p["dmin"], p["P1"], p["P2"], p["NDIR"], p["TSGM"])
    o2, c2, o1, c1 = runnerup(S, p["dmin"], CLI_RADIUS)
    out, conf = uniqueness(o1, c1, c2, CLI_RATIO)
    has = ~np.isnan(o1)
    frac = float(np.mean(np.isnan(out[has])))
    print("pixels with a winner: %d of %d; without a runner-up: %d; rejected at ratio %.3f: %.4f (%d)"
          % (has.sum(), has.size, (has & np.isnan(o2)).sum(), CLI_RATIO, frac, np.isnan(out[has]).sum()))
    assert has.sum() > has.size // 2
    assert 0.01 <= frac <= 0.50
