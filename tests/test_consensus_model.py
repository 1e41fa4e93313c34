"""The numpy model of the consensus votes (tests/consensus_model.py) against a scalar restatement of the definition
on random and crafted volumes, its invariants, a list of subtly wrong searches that the crafted inputs -- the very ones the GPU
tests write over the device's pass volumes (tests/consensus_crafted.py) -- tell from it, what the header, the binding and the
README name, the command line's early answers, and -- on the oracle's per-pass Lr of the pair the GPU command-line test uses --
the share of pixels that test's filter rejects."""
import os
import subprocess

import numpy as np
import pytest

import consensus_crafted as K
import mgm_amd
from consensus_model import CLI_MIN, CLI_TOL, consensus, consensus_filter, pass_winners
from helpers import ndiff
from mgm_amd import synth
from runnerup_model import PAIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
f32 = np.float32


def same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


def loops(lr, dmin, NDIR, d, tol, lo=None, hi=None, wrong=None):
    """The definition, pixel by pixel, pass by pass and label by label.  `wrong`: one of WRONG, a search that is subtly not it."""
    n, ny, nx, L = lr.shape
    votes = np.zeros((ny, nx), np.float32)
    winners = np.full((NDIR, ny, nx), np.nan, np.float32)
    tol = f32(tol)
    npass = NDIR + 1 if wrong == "a pass beyond NDIR" and n > NDIR else NDIR
    for y in range(ny):
        for x in range(nx):
            a, b = (0, L - 1) if lo is None else (max(0, int(lo[y, x])), min(L - 1, int(hi[y, x])))
            if wrong == "zone one lower":
                a = max(0, a - 1)
            if wrong == "zone one higher":
                b = min(L - 1, b + 1)
            if wrong == "padding and unowned slots":
                a, b = 0, L - 1
            dv = f32(d[y, x])
            if wrong == "d truncated" and np.isfinite(dv):
                dv = f32(np.trunc(dv))
            for p in range(npass):
                best, w = f32(np.inf), None
                for o in range(a, b + 1):
                    v = lr[p, y, x, o]
                    cand = np.isfinite(v) if wrong != "non-finite candidates" else not np.isnan(v)
                    if cand and (best > v or (wrong == "ties to the last" and best >= v) or (wrong == "non-finite candidates" and w is None)):
                        best, w = v, o
                if w is None:
                    if wrong == "a pass without a winner counted":
                        votes[y, x] += 1
                    continue
                if p < NDIR:
                    winners[p, y, x] = f32(w + dmin)
                with np.errstate(invalid="ignore", over="ignore"):
                    diff = np.abs(f32(f32(w + dmin) - dv))
                if (diff < tol) if wrong == "< for <=" else (diff <= tol):
                    votes[y, x] += 1
    return votes, winners


WRONG = ("ties to the last", "< for <=", "non-finite candidates", "a pass without a winner counted", "zone one lower", "zone one higher",
         "padding and unowned slots", "a pass beyond NDIR", "d truncated")


def random_volumes():
    rng = np.random.default_rng(31)
    cases = []
    for nx, ny, L, dmin, NDIR in [(9, 3, 7, -3, 4), (9, 3, 7, 2, 8), (4, 2, 7, -9, 1), (5, 1, 1, 0, 3), (5, 2, 2, -1, 2), (6, 2, 3, -1, 5), (8, 2, 13, 5, 8)]:
        lr = (rng.integers(0, 4, (NDIR, ny, nx, L)) - 1).astype(np.float32)  # few values, some negative: ties everywhere
        lr[rng.random(lr.shape) < 0.15] = np.inf
        lr[rng.random(lr.shape) < 0.05] = np.nan
        lr[rng.random(lr.shape) < 0.05] = -np.inf
        lr[:, 0, 0] = np.inf          # a pixel without a winner in any pass
        lr[0, 0, 1] = np.nan          # ... in one pass
        d = (rng.integers(dmin - 1, dmin + L + 1, (ny, nx)) + rng.choice([0, 0.25, 0.5], (ny, nx))).astype(np.float32)
        d[rng.random(d.shape) < 0.1] = np.nan
        d[0, -1] = np.inf
        lo = rng.integers(-1, L, (ny, nx))
        hi = lo + rng.integers(0, L + 1, (ny, nx))
        cases.append((lr, dmin, NDIR, d, None, None))
        cases.append((lr, dmin, NDIR, d, lo, hi))
    return cases


def crafted_cases():
    """(what, the volume as a kernel sees it, dmin, NDIR, d, tol, lo, hi) over the classes, strides, zones, maps and tolerances of
    tests/consensus_crafted.py -- small shapes of what tests/test_gpu_wta_consensus_crafted.py runs"""
    out = []
    j = 0
    for L, Lk, LPL, NDIR, ny, nx, dmin, ragged in [(64, 64, 1, 4, 3, 7, -20, False), (100, 128, 2, 8, 2, 9, -50, False), (37, 37, 1, 3, 3, 5, 3, False),
                                                   (70, 128, 2, 5, 3, 9, -9, True), (128, 128, 2, 8, 2, 7, -100, True)]:
        for name, fn in K.classes(LPL).items():
            lo = hi = None
            if ragged:
                lo, hi = K.windows(40 + j, ny, nx, L)
                lr = K.lay_in_windows(fn, 100 + j, NDIR, ny, nx, L, lo, hi)
            else:
                lr = fn(100 + j, NDIR, ny, nx, L)
            vol = K.full(lr, Lk, lo, hi)
            zlo, zhi = (lo, hi) if ragged else (np.zeros((ny, nx), int), np.full((ny, nx), L - 1))
            _, win = consensus(vol, dmin, NDIR, None, 0.0, zlo, zhi)
            base = K.base_labels(ny, nx, L, LPL) if not ragged else (np.ravel(lo) + K.base_labels(ny, nx, 3, 1))
            for dname, d in K.d_maps(win[0], base, dmin).items():
                out.append(((name, L, Lk, NDIR, ragged, dname), vol, dmin, NDIR, d, K.TOLS[j % 4], zlo, zhi))
                j += 1
    return out


def test_model_equals_the_definition_on_random_volumes():
    none = tie = False
    for lr, dmin, NDIR, d, lo, hi in random_volumes():
        for tol in K.TOLS:
            got, want = consensus(lr, dmin, NDIR, d, tol, lo, hi), loops(lr, dmin, NDIR, d, tol, lo, hi)
            assert same(got[0], want[0]) and same(got[1], want[1])
        none |= bool(np.isnan(want[1]).any())
        m = np.where(np.isfinite(lr), lr, np.inf)
        tie |= bool(((m == m.min(axis=-1, keepdims=True)) & np.isfinite(m)).sum(axis=-1).max() > 1)
    assert none and tie


def test_model_equals_the_definition_on_the_crafted_volumes():
    for what, vol, dmin, NDIR, d, tol, lo, hi in crafted_cases():
        got, want = consensus(vol, dmin, NDIR, d, tol, lo, hi), loops(vol, dmin, NDIR, d, tol, lo, hi)
        assert same(got[0], want[0]) and same(got[1], want[1]), what


def test_the_crafted_volumes_tell_every_wrong_search_from_the_model():
    told = {w: 0 for w in WRONG}
    for what, vol, dmin, NDIR, d, tol, lo, hi in crafted_cases():
        votes, winners = consensus(vol, dmin, NDIR, d, tol, lo, hi)
        for w in WRONG:
            bad = loops(vol, dmin, NDIR, d, tol, lo, hi, wrong=w)
            told[w] += int(not (same(bad[0], votes) and same(bad[1], winners)))
    print(told)
    assert all(n >= 3 for n in told.values()), told


def test_invariants():
    for lr, dmin, NDIR, d, lo, hi in random_volumes() + [(vol, dmin, NDIR, d, lo, hi) for _, vol, dmin, NDIR, d, _, lo, hi in crafted_cases()[::7]]:
        L = lr.shape[-1]
        prev = None
        _, has = pass_winners(lr, NDIR, lo, hi)
        for tol in K.TOLS + (float(L + abs(dmin) + 2),):
            votes, winners = consensus(lr, dmin, NDIR, d, tol, lo, hi)
            assert ((votes >= 0) & (votes <= NDIR)).all() and (votes == np.round(votes)).all()
            assert prev is None or (votes >= prev).all()   # votes do not fall as tol rises
            prev = votes
            assert (votes[~np.isfinite(d)] == 0).all()       # a NaN or infinite d gets no vote
            assert np.array_equal(np.isnan(winners), ~has)
        inside = np.isfinite(d) & (d >= dmin) & (d <= dmin + L - 1)
        assert (prev[inside] == has.sum(axis=0)[inside]).all()  # tol >= L, d inside the range: the passes that have a winner
        if lr.shape[0] > NDIR:                                   # passes >= NDIR have no influence
            other = lr.copy()
            other[NDIR:] = 7
            a, b = consensus(lr, dmin, NDIR, d, 1.0, lo, hi), consensus(other, dmin, NDIR, d, 1.0, lo, hi)
            assert same(a[0], b[0]) and same(a[1], b[1])


def test_filter():
    nan = f32(np.nan)
    d = np.array([[1.5, nan, 3.0, np.inf, -2.0, 0.0]], np.float32)
    v = np.array([[8.0, 8.0, 5.0, 6.0, 0.0, nan]], np.float32)
    out = consensus_filter(d, v, 6)
    assert same(out, np.array([[1.5, nan, nan, np.inf, nan, 0.0]], np.float32))  # (a NaN vote count keeps d)
    assert same(consensus_filter(d, v, 0), d)
    with pytest.raises(ValueError):
        consensus_filter(d, v, -1)
    with pytest.raises(ValueError):
        consensus(np.zeros((1, 1, 1, 2), np.float32), 0, 1, d[:, :1], -1.0)


def test_header_binding_and_readme_name_the_mode():
    hdr = open(os.path.join(ROOT, "include", "mgm_hip.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in ("mgm_wta_consensus_dev", "mgm_consensus_filter_dev"):
        assert name in mgm_amd.ABI_SYMBOLS and name + "(" in hdr and name in readme
        assert hasattr(mgm_amd.load_library(), name)
    assert callable(getattr(mgm_amd.Context, "wta_consensus_dev", None)) and callable(getattr(mgm_amd.Context, "consensus_filter_dev", None))
    for word in ("-C FILE", "MGM_CONSENSUS", "MGM_CONSENSUS_TOL", "MGM_HIP_WTA_CONSENSUS_ANY"):
        assert word in readme, word
    for word in ("-C FILE", "MGM_CONSENSUS=k", "MGM_CONSENSUS_TOL", "--help"):
        assert word in hdr, word


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


@pytest.mark.parametrize("env,word", [({"MGM_CONSENSUS": "-1"}, "MGM_CONSENSUS must"), ({"MGM_CONSENSUS": "2.5"}, "MGM_CONSENSUS must"),
                                      ({"MGM_CONSENSUS": "six"}, "MGM_CONSENSUS must"), ({"MGM_CONSENSUS": "nan"}, "MGM_CONSENSUS must"),
                                      ({"MGM_CONSENSUS_TOL": "-0.5"}, "MGM_CONSENSUS_TOL must"), ({"MGM_CONSENSUS_TOL": "inf"}, "MGM_CONSENSUS_TOL must"),
                                      ({"MGM_CONSENSUS_TOL": "nan"}, "MGM_CONSENSUS_TOL must"), ({"MGM_CONSENSUS_TOL": "one"}, "MGM_CONSENSUS_TOL must"),
                                      ({"MGM_CONSENSUS": "6", "MGM_CONSENSUS_TOL": "1e39"}, "MGM_CONSENSUS_TOL must")])
def test_cli_refuses_bad_values_before_any_work(env, word):
    """Exit code 1 and one line on stderr when the command line is parsed: no device, no input file."""
    r = run_cli(["no_u.png", "no_v.png", "no_out.tif"], env)
    assert r.returncode == 1 and word in r.stderr and len(r.stderr.splitlines()) == 1 and r.stdout == ""


@pytest.mark.parametrize("args,env", [(["-C", "votes.tif"], {}), ([], {"MGM_CONSENSUS": "6"})])
def test_cli_refuses_several_devices(args, env):
    """Exit code 2 and one line on stderr, before any device or input file is touched."""
    r = run_cli(args + ["no_u.png", "no_v.png", "no_out.tif"], dict(env, MGM_DEVICES="0,1"))
    assert r.returncode == 2 and r.stderr == "mgm: -C / MGM_CONSENSUS does not combine with several MGM_DEVICES\n"


def test_the_filter_of_the_command_line_test_rejects_a_visible_part(oracle):
    """The oracle's per-pass Lr of the 96 x 40 synthetic census pair, the model's votes for the unrefined winner at tol = 1: fewer
    than CLI_MIN = 6 votes must reject between 10 % and 40 % of the pixels, and all 8 passes must agree on more than half, or the
    command-line comparison on the GPU would compare maps the filter never touched (or emptied).  Measured: 867 of 3840 rejected,
    2211 unanimous, histogram of 0..8 votes [0 20 100 107 379 261 358 404 2211]."""
    p = PAIR
    u, v, _ = synth.stereo_pair(p["nx"], p["ny"], p["dmin"], p["dmax"])
    C = oracle.costvolume(u, v, p["dmin"], p["dmax"], "none", "census")
    S, out, _, lr = oracle.mgm(C, p["dmin"], p["P1"], p["P2"], p["NDIR"], p["TSGM"], dump_lr=True)
    votes, winners = consensus(lr, p["dmin"], p["NDIR"], out, CLI_TOL)
    hist = np.bincount(votes.astype(int).ravel(), minlength=p["NDIR"] + 1)
    print("votes 0..%d: %s; fewer than %d: %d of %d" % (p["NDIR"], hist, CLI_MIN, (votes < CLI_MIN).sum(), votes.size))
    assert 0.10 <= float(np.mean(votes < CLI_MIN)) <= 0.40
    assert float(np.mean(votes == p["NDIR"])) > 0.5
    kept = consensus_filter(out, votes, CLI_MIN)
    assert np.array_equal(np.isnan(kept), (votes < CLI_MIN) | np.isnan(out))
