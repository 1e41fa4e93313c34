"""The command line's side of the solution energy:

  TSGM_DEBUG=1   stdout -- every `costvolume:` line, the weights line, the energy line of every iteration and run, the
                 `refinement:` line -- and every output file equal the REFERENCE BINARY's (oracle/_ref/mgm), byte for byte
  MGM_ENERGY     the `[mgm energy]` lines on stderr and MGM_ENERGY_MAP's file against the numpy model on the CPU oracle's volume and
                 unrefined labels
  refusals       exit code 2 through the exclusion table, exit code 1 for bad values; TSGM_DEBUG stays ignored where the reference
                 has no stdout to equal"""
import math
import os
import subprocess

import numpy as np
import pytest

import energy_model as em
import energy_runs as er
from helpers import ndiff
from mgm_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
F = np.float32

DEBUG_CASES = [  # (name, nch, args, env): cases of tests/test_gpu_cli.py
    ("cfg1-style ad O4 TSGM2", 3, "-r -20 -R 12 -t ad -O 4", dict(TSGM="2")),
    ("Makefile test: census FH vfit median", 3, "-P2 20000 -P1 2 -r -20 -R 12 -t census -s vfit -O 8",
     dict(MEDIAN="1", CENSUS_NCC_WIN="3", USE_TRUNCATED_LINEAR_POTENTIALS="1", TSGM="3")),
    ("no LR test, -l, weights", 3, "-r -20 -R 12 -t ad -O 8 -aP2 4 -aThresh 12 -l {tmp}/nolr.npy", dict(TESTLRRL="0", TSGM="3")),
    ("unknown names fall back silently", 1, "-r -8 -R 8 -t nope -p sobel_x -s bogus -O 4", dict(TSGM="2")),
    ("sobelx prefilter, cubic refinement", 1, "-r -10 -R 10 -p sobelx -t ad -s cubic -O 4", dict(TSGM="2")),
    ("gblur prefilter, parabola, median radius 2", 3, "-r -12 -R 9 -p gblur -t sd -s parabola -O 8", dict(TSGM="3", MEDIAN="2")),
    ("TSGM_ITER=2: ranges narrowed around the first solution", 1, "-r -16 -R 8 -t census -s vfit -O 8",
     dict(TSGM="3", TSGM_ITER="2", CENSUS_NCC_WIN="5")),
    ("TSGM_ITER=2, 3 channels, weights, median, no LR", 3, "-r -20 -R 12 -t ad -O 8 -aP2 4 -aThresh 12 -s parabola",
     dict(TSGM="4", TSGM_ITER="2", MEDIAN="1", TESTLRRL="0")),
    ("ragged ranges from -m/-M files, census vfit", 1, "-r -16 -R 8 -t census -s vfit -O 8 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="3", CENSUS_NCC_WIN="5")),
    ("ragged ranges, FH, TSGM=2 with weights, TSGM_ITER=2", 3, "-P1 2 -P2 9 -r -16 -R 8 -t ad -O 4 -aP2 4 -aThresh 12 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="2", TSGM_ITER="2", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    ("TSGM_ITER=0: no call of mgm() at all", 1, "-r -16 -R 8 -t census -s vfit -O 8", dict(TSGM="3", TSGM_ITER="0", MEDIAN="1")),
]


def write_pair(tmp_path, nch):
    u, v, gt = synth.stereo_pair(112, 72, -16, 8, seed=42, nch=nch)
    er.save_pair(str(tmp_path), u, v)
    lo, hi = er.cli_ranges(gt, 72, 112)
    np.save(tmp_path / "lo.npy", lo)
    np.save(tmp_path / "hi.npy", hi)
    return u, v, lo, hi


@pytest.mark.skipif(not os.path.exists(er.REF), reason="reference CLI (oracle/_ref/mgm) was not built")
@pytest.mark.parametrize("case", DEBUG_CASES, ids=lambda c: c[0])
def test_debug_stdout_is_the_reference_s(case, tmp_path):
    name, nch, args, env = case
    write_pair(tmp_path, nch)
    outs = {tag: er.run_cli(exe, args, env, str(tmp_path), str(tmp_path / tag), dict(TSGM_DEBUG="1")) for tag, exe in (("ref", er.REF), ("ours", OURS))}
    print(outs["ref"][0])
    assert outs["ref"][0] == outs["ours"][0], "stdout differs"
    n = len(er.debug_figures(outs["ref"][0]))
    assert n == int(env.get("TSGM_ITER", 1)) * (1 if env.get("TESTLRRL") == "0" else 2) and "costvolume: selecting distance" in outs["ref"][0]
    assert outs["ref"][2].keys() == outs["ours"][2].keys()
    for f in outs["ref"][2]:
        assert ndiff(outs["ref"][2][f], outs["ours"][2][f]) == 0, (name, f)
    # ... and TSGM_DEBUG=0 / unset is the program as it was: the bare newline
    plain = er.run_cli(OURS, args, env, str(tmp_path), str(tmp_path / "plain"), dict(TSGM_DEBUG="0"))
    assert "ENERGY" not in plain[0] and "costvolume" not in plain[0] and "refinement" not in plain[0]
    for f in plain[2]:
        assert ndiff(plain[2][f], outs["ours"][2][f]) == 0, (name, f)


ENERGY_CASES = [
    ("census, O8, TSGM=3, vfit, 8 neighbours", 1, "-r -16 -R 8 -t census -s vfit -O 8", dict(TSGM="3", CENSUS_NCC_WIN="5"), 8),
    ("ad, 3 channels, weights, FH, TSGM_ITER=2, 4 neighbours", 3, "-P1 2 -P2 9 -r -16 -R 8 -t ad -O 4 -aP2 4 -aThresh 12",
     dict(TSGM="2", TSGM_ITER="2", USE_TRUNCATED_LINEAR_POTENTIALS="1"), 4),
    ("-m/-M range images, weights, parabola, 8 neighbours, no LR", 1,
     "-r -16 -R 8 -t census -O 8 -aP2 4 -aThresh 12 -s parabola -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="4", CENSUS_NCC_WIN="5", TESTLRRL="0"), 8),
]


@pytest.mark.parametrize("case", ENERGY_CASES, ids=lambda c: c[0])
def test_model_energy_lines_and_map(case, oracle, tmp_path):
    name, nch, args, env, conn = case
    u, v, lo, hi = write_pair(tmp_path, nch)
    mapf = str(tmp_path / "energy.npy")
    stdout, stderr, files = er.run_cli(OURS, args, env, str(tmp_path), str(tmp_path / "ours"), dict(MGM_ENERGY=str(conn), MGM_ENERGY_MAP=mapf))
    plain = er.run_cli(OURS, args, env, str(tmp_path), str(tmp_path / "plain"))
    assert stdout == plain[0] and all(ndiff(files[f], plain[2][f]) == 0 for f in files)  # stdout and the outputs are left alone
    got = [er.MODEL_RE.match(ln).groups() for ln in stderr.splitlines() if ln.startswith("[mgm energy]")]
    prm, dmin, dmax = er.params_of(args, env, nch)
    ranged = "{ranges}" in args
    runs = er.both_runs(oracle, u, v, dmin, dmax, prm, lo if ranged else None, hi if ranged else None)
    want = []
    for key in ("L", "R"):
        if key in runs:
            r = runs[key]
            for it, d in enumerate(r["maps"]):
                want.append((key, it) + em.energy(r["C"], r["hmin"], d, 3, prm["P1"], prm["P2"], conn, prm["FH"], r["w8"], r["lo"], r["hi"]))
    assert [(g[0], int(g[1])) for g in got] == [(w[0], w[1]) for w in want], stderr
    for g, (key, it, E, t) in zip(got, want):
        assert (int(g[5]), int(g[6])) == (t["finite"], t["pixels"])
        for k, s in (("total", g[2]), ("data", g[3]), ("smooth", g[4])):
            x = float(s)
            print(name, key, it, k, x, t[k])
            assert x == t[k] or (math.isfinite(t[k]) and abs(x - t[k]) <= t["finite"] * 2.0 ** -52 * abs(t[k])), (name, key, it, k, x, t[k])
    lastL = [w for w in want if w[0] == "L"][-1][2]
    written = np.load(mapf).reshape(lastL.shape).astype(F)
    assert ndiff(written, lastL) == 0


def run_plain(args, env, tmp_path):
    cmd = [OURS] + args.split() + [str(tmp_path / "u.npy"), str(tmp_path / "v.npy"), str(tmp_path / "out.npy")]
    e = {k: v for k, v in os.environ.items() if k not in ("TSGM_DEBUG", "MGM_ENERGY", "MGM_ENERGY_MAP")}
    return subprocess.run(cmd, env=dict(e, **env), capture_output=True, text=True, timeout=600)


def test_refusals_and_bad_values(tmp_path):
    write_pair(tmp_path, 1)
    for args, env, blocker in er.ENERGY_REFUSALS:
        r = run_plain("-r -8 -R 8 " + args, dict(env, MGM_ENERGY="4"), tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (2, "-8 8\n", "mgm: MGM_ENERGY does not combine with %s\n" % blocker), (args, env, r)
    for env, msg in er.ENERGY_BAD_VALUES:
        r = run_plain("-r -8 -R 8", env, tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), (env, r)


@pytest.mark.parametrize("mode", er.DEBUG_IGNORED, ids=lambda m: m[0])
def test_debug_stays_ignored_where_the_reference_has_no_stdout(mode, tmp_path):
    name, args, env = mode
    write_pair(tmp_path, 1)
    base = "-r -16 -R 8 -t census -O 4 " + args
    a = run_plain(base, dict(env, TSGM="2"), tmp_path)
    b = run_plain(base, dict(env, TSGM="2", TSGM_DEBUG="1"), tmp_path)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert a.stdout == b.stdout and "ENERGY" not in b.stdout and "costvolume" not in b.stdout
