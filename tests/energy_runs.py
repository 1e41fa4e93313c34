"""main()'s two loops (mgm.cc:372-418) on the CPU oracle, keeping what the energy of an iteration is computed from: the cost
volume built before the loop, the run's integer ranges and weights, and the UNREFINED map of every iteration (mgm()'s own
outoff, mgm.cc:381-383).  TEST INFRASTRUCTURE ONLY: tests/test_energy_model_ref.py pins the reference binary's TSGM_DEBUG figures
on it, tests/test_gpu_energy_cli.py the command line's MGM_ENERGY lines."""
import os
import re
import subprocess

import numpy as np

import multiscale_model as msm
from oracle import oracle as orc_mod

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "mgm")
REFINING = ("vfit", "parabola", "cubic", "parabolaOCV")

ENERGY_RE = re.compile(r" ENERGY L1trunc: (\S+)\tL1: (\S+)\tL2: (\S+)$")
MODEL_RE = re.compile(r"^\[mgm energy\] run=([LR]) iter=(\d+) total=(\S+) data=(\S+) smooth=(\S+) finite=(\d+)/(\d+)$")


def repaired_ranges(lo, hi, dmin, dmax):
    """the -m/-M images as main() repairs them (mgm.cc:342-353)"""
    lo, hi = np.array(lo, F, copy=True), np.array(hi, F, copy=True)
    lo[~np.isfinite(lo)] = dmin
    hi[~np.isfinite(hi)] = dmax
    bad = hi < (lo + F(1)).astype(F)
    hi[bad] = np.ceil((lo + F(1)).astype(F))[bad]
    return lo, hi


def one_run(oracle, U, V, lo, hi, prm):
    """U, V: (nch, ny, nx); lo, hi: float range images; prm: P1, P2 (already times nch), NDIR, TSGM, FH, FIX, aP2, aThresh,
    prefilter, distance, truncDist, census_win, refine, iterations.  dict(C, hmin, lo, hi, w8, maps, out)"""
    ilo, ihi = orc_mod.int_ranges(lo, hi)
    hmin, hmax = int(ilo.min()), int(ihi.max())
    C = oracle.costvolume_ranged(U, V, ilo, ihi, hmin, hmax, prm["prefilter"], prm["distance"], prm["truncDist"], prm["census_win"])
    w8 = oracle.weights(U, prm["aP2"], prm["aThresh"]) if prm["aP2"] != 1.0 else None
    args = (prm["P1"], prm["P2"], prm["NDIR"], prm["TSGM"], prm["FH"], prm["FIX"], w8)
    refining = prm["refine"] in REFINING
    maps, wl, wh, out = [], lo, hi, None
    for it in range(prm["iterations"]):
        if it == 0:
            S, out, cost = oracle.mgm_ranged(C, hmin, ilo, ihi, *args)
            slo, shi, shmin = ilo, ihi, hmin
        else:
            wl, wh = msm.update_dmin_dmax(out, wl, wh, 3, 2)
            slo, shi = orc_mod.int_ranges(wl, wh)
            shmin, shmax = int(slo.min()), int(shi.max())
            S, out, cost = oracle.mgm_ranged(C, hmin, ilo, ihi, *args, srange=(slo, shi, shmin, shmax))
        maps.append(np.array(out, F, copy=True))
        if refining:
            out, cost = oracle.refine_ranged(S, shmin, slo, shi, prm["refine"], out, cost)
    return dict(C=C, hmin=hmin, lo=ilo, hi=ihi, w8=w8, maps=maps, out=out)


DEFAULTS = dict(P1=8.0, P2=32.0, NDIR=4, TSGM=4, FH=0, FIX=1, aP2=1.0, aThresh=5.0, prefilter="none", distance="ad", truncDist=np.inf,
                census_win=3, refine="none", iterations=1, both=True)


def params_of(args, env, nch):
    """the parameters of a command line given as its option string and environment (the options these tests use)"""
    a = args.split()
    opt = lambda name, dflt: a[a.index(name) + 1] if name in a else dflt
    p = dict(DEFAULTS)
    p.update(P1=float(F(float(opt("-P1", 8))) * F(nch)), P2=float(F(float(opt("-P2", 32))) * F(nch)), NDIR=int(opt("-O", 4)), aP2=float(opt("-aP2", 1)),
             aThresh=float(opt("-aThresh", 5)), prefilter=opt("-p", "none"), distance=opt("-t", "ad"), truncDist=float(opt("-truncDist", "inf")),
             refine=opt("-s", "none"), TSGM=int(env.get("TSGM", 4)), FH=int(env.get("USE_TRUNCATED_LINEAR_POTENTIALS", 0)),
             FIX=int(env.get("TSGM_FIX_OVERCOUNT", 1)), census_win=int(env.get("CENSUS_NCC_WIN", 3)), iterations=int(env.get("TSGM_ITER", 1)),
             both=env.get("TESTLRRL", "1") != "0")
    return p, int(opt("-r", -30)), int(opt("-R", 30))


def both_runs(oracle, u, v, dmin, dmax, prm, lo=None, hi=None):
    """{'L': one_run(...), 'R': ...} ('R' only with prm['both'])"""
    u, v = np.asarray(u, F), np.asarray(v, F)
    _, ny, nx = u.shape
    _, vny, vnx = v.shape
    if lo is None:
        lo, hi = np.full((ny, nx), dmin, F), np.full((ny, nx), dmax, F)
    else:
        lo, hi = repaired_ranges(np.asarray(lo, F).reshape(ny, nx), np.asarray(hi, F).reshape(ny, nx), dmin, dmax)
    runs = {"L": one_run(oracle, u, v, lo, hi, prm)}
    if prm["both"]:
        runs["R"] = one_run(oracle, v, u, np.full((vny, vnx), -dmax, F), np.full((vny, vnx), -dmin, F), prm)
    return runs


def save_pair(tmp, u, v):
    nch = u.shape[0]
    np.save(os.path.join(tmp, "u.npy"), np.ascontiguousarray(u.transpose(1, 2, 0)) if nch > 1 else u[0])
    np.save(os.path.join(tmp, "v.npy"), np.ascontiguousarray(v.transpose(1, 2, 0)) if nch > 1 else v[0])


def cli_ranges(gt, ny, nx):
    """the range images of tests/test_gpu_cli.py: around the true disparity, some empty, some non-finite"""
    rng = np.random.default_rng(8)
    gt2 = np.asarray(gt, F).reshape(ny, nx)
    lo = np.floor(gt2 - rng.integers(1, 7, size=gt2.shape)).astype(F) + rng.random(gt2.shape).astype(F)
    hi = lo + rng.integers(0, 14, size=gt2.shape).astype(F)
    lo[rng.random(gt2.shape) < 0.02] = np.nan
    hi[rng.random(gt2.shape) < 0.02] = np.inf
    return lo, hi


def run_cli(exe, args, env, tmp, outdir, extra_env=None):
    """one command line on tmp/u.npy, tmp/v.npy: (stdout, stderr, {file: array})"""
    os.makedirs(outdir, exist_ok=True)
    cmd = [exe] + args.format(tmp=outdir, ranges=tmp).split() + [os.path.join(tmp, "u.npy"), os.path.join(tmp, "v.npy")] + [
        os.path.join(outdir, f) for f in ("disp.npy", "cost.npy", "back.npy")]
    e = dict(os.environ, OMP_NUM_THREADS="4")
    e.update(env)
    e.update(extra_env or {})
    r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (cmd, r.stderr)
    return r.stdout, r.stderr, {f: np.load(os.path.join(outdir, f)) for f in sorted(os.listdir(outdir)) if f.endswith(".npy")}


def debug_figures(stdout):
    """the three figures of every energy line of a TSGM_DEBUG=1 stdout, in order, as float32 triples"""
    out = []
    for ln in stdout.splitlines():
        m = ENERGY_RE.search(ln)
        if m:
            out.append(tuple(F(float(x)) for x in m.groups()))
    return out


# ---- the command line's rules (src/mgm_jobplan.h): what MGM_ENERGY does not combine with, its bad values, where TSGM_DEBUG stays ignored
ENERGY_REFUSALS = [  # (options, environment, the blocker's name in the exclusion table)
    ("-S 2", {}, "-S > 1"),
    ("", dict(MGM_RIGHT_FROM_LEFT="1"), "MGM_RIGHT_FROM_LEFT=1"),
    ("", dict(MGM_DEVICES="0,0"), "several MGM_DEVICES"),
    ("", dict(MGM_SUBPIX="2"), "MGM_SUBPIX"),
]
ENERGY_BAD_VALUES = [  # (environment, stderr): exit code 1 before anything is printed
    (dict(MGM_ENERGY="3"), "mgm: MGM_ENERGY must be 4 or 8 (neighbours; 0: off)\n"),
    (dict(MGM_ENERGY="eight"), "mgm: MGM_ENERGY must be 4 or 8 (neighbours; 0: off)\n"),
    (dict(MGM_ENERGY="8x"), "mgm: MGM_ENERGY must be 4 or 8 (neighbours; 0: off)\n"),
    (dict(MGM_ENERGY_MAP="e.npy"), "mgm: MGM_ENERGY_MAP needs MGM_ENERGY=4 or 8\n"),
    (dict(MGM_ENERGY="0", MGM_ENERGY_MAP="e.npy"), "mgm: MGM_ENERGY_MAP needs MGM_ENERGY=4 or 8\n"),
]
DEBUG_IGNORED = [  # (name, options, environment)
    ("-S 2", "-S 2", {}),
    ("MGM_SUBPIX=2", "", dict(MGM_SUBPIX="2")),
    ("MGM_RIGHT_FROM_LEFT=1", "", dict(MGM_RIGHT_FROM_LEFT="1")),
    ("MGM_DEVICES=0,0", "", dict(MGM_DEVICES="0,0", MGM_MULTI_LOOPBACK="1")),
]
