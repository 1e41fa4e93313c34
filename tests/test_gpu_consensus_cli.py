"""-C FILE, MGM_CONSENSUS and MGM_CONSENSUS_TOL of the command line, and the consensus step of mgm_multiscale_pair_dev,
against the model composed over the oracle: search, vfit, votes, filter, left-right test -- on the 96 x 40 synthetic census pair of
tests/runnerup_model.py, at the filter tests/test_consensus_model.py chose on the oracle (fewer than 6 of 8 votes at tol = 1 rejects
867 of its 3840 pixels), plain, with -m/-M range images and with -S 2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
import multiscale_model as msm
from consensus_model import CLI_MIN, CLI_TOL, consensus, consensus_filter
from helpers import ndiff
from mgm_amd import synth
from oracle import oracle as orc_mod
from runnerup_model import PAIR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
CONV = os.path.join(ROOT, "mgm_amd", "bin", "imgconv")
ARGS = "-r -16 -R 0 -t census -s vfit -O 8".split()
ENV = dict(MGM_CONSENSUS=str(CLI_MIN), MGM_CONSENSUS_TOL=repr(CLI_TOL))


def same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def read_tif(path):
    npy = path + ".npy"
    subprocess.run([CONV, path, npy], check=True, timeout=60)
    return np.load(npy).astype(np.float32).squeeze()


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    p = PAIR
    u, v, gt = synth.stereo_pair(p["nx"], p["ny"], p["dmin"], p["dmax"])
    d = tmp_path_factory.mktemp("consensuscli")
    fu, fv = str(d / "u.npy"), str(d / "v.npy")
    np.save(fu, u[0]), np.save(fv, v[0])
    return dict(u=u, v=v, gt=gt, fu=fu, fv=fv, dir=d)


def ranged_run(oracle, U, V, lo, hi, p, minvotes, tol):
    """one run of the path on float range images (lo, hi): search, vfit, votes of the refined map, filter.  Returns (the
    unfiltered refined map, the votes, the filtered map)."""
    ilo, ihi = orc_mod.int_ranges(lo, hi)
    hmin, hmax = int(ilo.min()), int(ihi.max())
    Cv = oracle.costvolume_ranged(U, V, ilo, ihi, hmin, hmax, "none", "census", np.inf, 3)
    S, out, cost, lr = oracle.mgm_ranged(Cv, hmin, ilo, ihi, p["P1"], p["P2"], p["NDIR"], p["TSGM"], 0, 1, None, dump_lr=True)
    out, cost = oracle.refine_ranged(S, hmin, ilo, ihi, "vfit", out, cost)
    votes, _ = consensus(lr, hmin, p["NDIR"], out, tol, ilo - hmin, ihi - hmin)
    return out, votes, consensus_filter(out, votes, minvotes)


def uniform(shape, a, b):
    return np.full(shape, a, np.float32), np.full(shape, b, np.float32)


def model_pair(oracle, u, v, p, minvotes, tol, loL=None, hiL=None):
    """the command line's pair: the left run (on -m/-M images if given), the right run on the negated -r/-R, each filtered, then the
    left-right test both ways.  dict(votes, nolr, out, plain_nolr)"""
    shapeL, shapeR = u.shape[1:], v.shape[1:]
    if loL is None:
        loL, hiL = uniform(shapeL, p["dmin"], p["dmax"])
    L = ranged_run(oracle, u, v, loL, hiL, p, minvotes, tol)
    R = ranged_run(oracle, v, u, *uniform(shapeR, -p["dmax"], -p["dmin"]), p, minvotes, tol)
    return dict(votes=L[1], nolr=L[2], out=msm.leftright(L[2], R[2], 1.0), plain_nolr=L[0], plain=msm.leftright(L[0], R[0], 1.0))


def test_command_line_against_the_model(oracle, pair):
    p, u, v, fu, fv = PAIR, pair["u"], pair["v"], pair["fu"], pair["fv"]
    f = {k: str(pair["dir"] / (k + ".tif")) for k in ("plain", "out", "votes", "nolr", "c0", "votes0", "nolr0", "rfl", "rflnolr", "rflvotes")}
    r0 = run_cli(ARGS + [fu, fv, f["plain"]], {})
    r1 = run_cli(ARGS + ["-C", f["votes"], "-l", f["nolr"], fu, fv, f["out"]], ENV)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert r1.stdout == r0.stdout and r0.stdout.splitlines() == ["-16 0", "01234567", "01234567"]
    want = model_pair(oracle, u, v, p, CLI_MIN, CLI_TOL)
    votes, nolr, out = read_tif(f["votes"]), read_tif(f["nolr"]), read_tif(f["out"])
    assert same(votes, want["votes"]), ndiff(votes, want["votes"])
    assert same(nolr, want["nolr"]) and same(out, want["out"])
    rejected = np.isnan(nolr) & ~np.isnan(want["plain_nolr"])
    print("the filter rejected %.4f of the left run's pixels" % rejected.mean())
    assert 0.10 <= rejected.mean() <= 0.40 and not same(read_tif(f["plain"]), out) and same(read_tif(f["plain"]), want["plain"])
    # -C alone, with MGM_CONSENSUS=0: the same votes, every other output that of a run without it
    r2 = run_cli(ARGS + ["-C", f["votes0"], "-l", f["nolr0"], fu, fv, f["c0"]], dict(MGM_CONSENSUS="0"))
    assert r2.returncode == 0 and r2.stdout == r0.stdout
    assert same(read_tif(f["votes0"]), want["votes"]) and same(read_tif(f["c0"]), read_tif(f["plain"])) and same(read_tif(f["nolr0"]), want["plain_nolr"])
    # right from left: only the left map is filtered
    r3 = run_cli(ARGS + ["-C", f["rflvotes"], "-l", f["rflnolr"], fu, fv, f["rfl"]], dict(ENV, MGM_RIGHT_FROM_LEFT="1"))
    assert r3.returncode == 0 and r3.stdout.splitlines() == ["-16 0", "01234567", "right from left"]
    assert same(read_tif(f["rflvotes"]), want["votes"]) and same(read_tif(f["rflnolr"]), want["nolr"])
    # several devices: exit code 2, whatever else is asked for
    r = run_cli(ARGS + ["-C", f["votes"], fu, fv, f["out"]], dict(ENV, MGM_DEVICES="0,1"))
    assert r.returncode == 2 and r.stderr == "mgm: -C / MGM_CONSENSUS does not combine with several MGM_DEVICES\n"


def test_command_line_with_range_images(oracle, pair):
    """-m/-M: the left run's volume is ragged (windows of 4 to 9 labels around the true disparity), whichever layout it is aggregated
    on; the right run keeps -r/-R"""
    p, u, v, gt, fu, fv = PAIR, pair["u"], pair["v"], pair["gt"], pair["fu"], pair["fv"]
    rng = np.random.default_rng(3)
    lo = np.clip(np.round(gt) - rng.integers(2, 5, gt.shape), p["dmin"], p["dmax"] - 1).astype(np.float32)
    hi = np.clip(lo + rng.integers(3, 9, gt.shape), lo + 1, p["dmax"]).astype(np.float32)
    flo, fhi = str(pair["dir"] / "lo.npy"), str(pair["dir"] / "hi.npy")
    np.save(flo, lo), np.save(fhi, hi)
    f = {k: str(pair["dir"] / ("r_" + k + ".tif")) for k in ("plain", "out", "votes", "nolr")}
    extra = ["-m", flo, "-M", fhi]
    r0 = run_cli(ARGS + extra + [fu, fv, f["plain"]], {})
    r1 = run_cli(ARGS + extra + ["-C", f["votes"], "-l", f["nolr"], fu, fv, f["out"]], ENV)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stderr + r1.stderr
    assert r1.stdout == r0.stdout
    want = model_pair(oracle, u, v, p, CLI_MIN, CLI_TOL, lo, hi)
    assert same(read_tif(f["votes"]), want["votes"]) and same(read_tif(f["nolr"]), want["nolr"]) and same(read_tif(f["out"]), want["out"])
    assert same(read_tif(f["plain"]), want["plain"]) and (want["votes"] < CLI_MIN).any() and (want["votes"] == p["NDIR"]).any()


def finest_level_again(oracle, u, v, res, p, minvotes, tol):
    """the finest level of tests/multiscale_model.py once more, from the ranges it ran on, with the passes dumped: the votes of each
    run's refined map, the filter, the left-right test (TSGM_ITER = 1, MEDIAN = 0)"""
    (loL, hiL), (loR, hiR) = res["levels"][0]["ranges"]
    L = ranged_run(oracle, u, v, loL, hiL, p, minvotes, tol)
    R = ranged_run(oracle, v, u, loR, hiR, p, minvotes, tol)
    assert same(L[0], res["nolr"])  # (the helper is the model's own level when nothing is filtered)
    return dict(votes=L[1], nolr=L[2], outL=msm.leftright(L[2], R[2], 1.0), outR=msm.leftright(R[2], L[2], 1.0))


def test_two_scales(oracle, pair):
    p, u, v, fu, fv = PAIR, pair["u"], pair["v"], pair["fu"], pair["fv"]
    kw = dict(P1=p["P1"], P2=p["P2"], NDIR=p["NDIR"], TSGM=p["TSGM"], distance="census", census_win=3, refine="vfit")
    res = msm.multiscale_pair(oracle, u, v, p["dmin"], p["dmax"], 2, **kw)
    assert len(res["levels"]) == 2
    want = finest_level_again(oracle, u, v, res, p, CLI_MIN, CLI_TOL)
    assert (want["votes"] < CLI_MIN).any() and not same(want["outL"], res["outL"])
    # the command line
    f = {k: str(pair["dir"] / ("s_" + k + ".tif")) for k in ("out", "votes", "nolr")}
    r = run_cli(ARGS + ["-S", "2", "-C", f["votes"], "-l", f["nolr"], fu, fv, f["out"]], dict(ENV, TSGM_ITER="1", MEDIAN="0"))
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ["-16 0"] + ["01234567"] * 4
    assert same(read_tif(f["votes"]), want["votes"]) and same(read_tif(f["nolr"]), want["nolr"]) and same(read_tif(f["out"]), want["outL"])
    # the library
    with mgm_amd.Context(0) as ctx:
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        got = ctx.multiscale_pair(du, dv, p["dmin"], p["dmax"], 2, consensus_min=CLI_MIN, consensus_tol=CLI_TOL, want_votes=True, **kw)
        assert same(got["votesL"].download()[0], want["votes"]) and same(got["nolr"].download()[0], want["nolr"])
        assert same(got["outL"].download()[0], want["outL"]) and same(got["outR"].download()[0], want["outR"])
        only = ctx.multiscale_pair(du, dv, p["dmin"], p["dmax"], 2, want_votes=True, **kw)  # the votes alone: nothing is filtered
        assert same(only["votesL"].download()[0], want["votes"]) and same(only["outL"].download()[0], res["outL"])
        # an older caller: the struct as it has grown, its consensus fields set, but struct_size that of the old struct -- nothing new happens
        outL, costL, outR, costR, votes = (ctx.new_image(p["nx"], p["ny"]) for _ in range(5))
        votes.update(np.full((p["ny"], p["nx"]), -7, np.float32))
        n, lv = C.c_int(0), (mgm_amd.MsLevel * 8)()
        big = mgm_amd.MsParamsConsensus(C.sizeof(mgm_amd.MsParams), 2, 3, 2, p["dmin"], p["dmax"], None, None, p["P1"], p["P2"], p["NDIR"], p["TSGM"], 0, 1, 1.0, 5.0,
                                        b"none", b"census", float("inf"), 3, b"vfit", 1, 0, 1, 1.0, C.pointer(n), lv, None, CLI_TOL, CLI_MIN, votes.h)
        assert C.sizeof(big) > C.sizeof(mgm_amd.MsParams) and mgm_amd.MsParamsConsensus.consensus_tol.offset >= C.sizeof(mgm_amd.MsParams) - 8
        rc = ctx.lib.mgm_multiscale_pair_dev(ctx.h, du.h, dv.h, C.cast(C.pointer(big), C.POINTER(mgm_amd.MsParams)), outL.h, costL.h, outR.h, costR.h, None)
        assert rc == 0 and same(outL.download()[0], res["outL"]) and (votes.download() == -7).all()
        # bad values: a negative count, a tolerance that is no tolerance, votes of another size
        for kwbad in (dict(consensus_min=-1), dict(consensus_min=3, consensus_tol=-1.0), dict(consensus_min=3, consensus_tol=float("nan"))):
            with pytest.raises(mgm_amd.MgmError) as e:
                ctx.multiscale_pair(du, dv, p["dmin"], p["dmax"], 2, **dict(kw, **kwbad))
            assert e.value.code == mgm_amd.MGM_ERR_INVALID
        assert same(ctx.multiscale_pair(du, dv, p["dmin"], p["dmax"], 2, **kw)["outL"].download()[0], res["outL"])
