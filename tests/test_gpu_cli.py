"""The `mgm` host program (src/mgm_main.cc over libmgm_hip.so) against the REFERENCE'S OWN
command line (oracle/_ref/mgm, compiled from /root/reference; it travels to the GPU box as a
built binary): same arguments, same environment, .npy in / .npy out; stdout and every
output file must be identical (NaN == NaN)."""
import os
import subprocess

import numpy as np
import pytest

from helpers import ndiff
from mgm_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OURS = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
REF = os.path.join(ROOT, "oracle", "_ref", "mgm")

CASES = [
    # (name, nch, args, env)
    ("cfg1-style ad O4 TSGM2", 3, "-r -20 -R 12 -t ad -O 4", dict(TSGM="2")),
    ("defaults (TSGM=4)", 1, "-r -10 -R 10", {}),
    ("Makefile test: census FH vfit median", 3, "-P2 20000 -P1 2 -r -20 -R 12 -t census -s vfit -O 8",
     dict(MEDIAN="1", CENSUS_NCC_WIN="3", USE_TRUNCATED_LINEAR_POTENTIALS="1", TSGM="3")),
    ("README: census5 vfit O8 TSGM3", 1, "-r -22 -R 19 -s vfit -t census -O 8", dict(MEDIAN="1", CENSUS_NCC_WIN="5", TSGM="3")),
    ("no LR test, -l, weights", 3, "-r -20 -R 12 -t ad -O 8 -aP2 4 -aThresh 12 -l {tmp}/nolr.npy",
     dict(TESTLRRL="0", TSGM="3")),
    ("sd trunc, no overcount fix, tau", 1, "-r -9 -R 14 -t sd -truncDist 300 -O 2",
     dict(TSGM="1", TSGM_FIX_OVERCOUNT="0", TESTLRRL_TAU="2.5")),
    ("unknown names fall back silently", 1, "-r -8 -R 8 -t nope -p sobel_x -s bogus -O 4", dict(TSGM="2")),
    ("sobelx prefilter, cubic refinement", 1, "-r -10 -R 10 -p sobelx -t ad -s cubic -O 4", dict(TSGM="2")),
    ("gblur prefilter, parabola, median radius 2", 3, "-r -12 -R 9 -p gblur -t sd -s parabola -O 8",
     dict(TSGM="3", MEDIAN="2")),
    ("ncc cost, window 5", 1, "-r -10 -R 10 -t ncc -O 4", dict(TSGM="2", CENSUS_NCC_WIN="5")),
    ("btsd cost, 3 channels", 3, "-r -12 -R 9 -t btsd -truncDist 500 -O 8", dict(TSGM="3")),
    ("TSGM_ITER=2: ranges narrowed around the first solution", 1, "-r -16 -R 8 -t census -s vfit -O 8",
     dict(TSGM="3", TSGM_ITER="2", CENSUS_NCC_WIN="5")),
    ("TSGM_ITER=3, no over-count fix (window labels outside the volume compete), cubic", 1, "-r -10 -R 10 -t ad -s cubic -O 4",
     dict(TSGM="2", TSGM_ITER="3", TSGM_FIX_OVERCOUNT="0")),
    ("TSGM_ITER=2, 3 channels, weights, median, no LR", 3, "-r -20 -R 12 -t ad -O 8 -aP2 4 -aThresh 12 -s parabola",
     dict(TSGM="4", TSGM_ITER="2", MEDIAN="1", TESTLRRL="0")),
    ("ragged ranges from -m/-M files (NaNs, empty ranges repaired), census vfit", 1,
     "-r -16 -R 8 -t census -s vfit -O 8 -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="3", CENSUS_NCC_WIN="5")),
    ("ragged ranges, TSGM_ITER=2, no over-count fix, weights, 3 channels", 3,
     "-r -16 -R 8 -t ad -O 8 -aP2 4 -aThresh 12 -s parabola -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="4", TSGM_ITER="2", TSGM_FIX_OVERCOUNT="0")),
    ("ragged ranges, TSGM=2, cubic, median, no LR", 1, "-r -16 -R 8 -t sd -s cubic -O 4 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="2", MEDIAN="1", TESTLRRL="0")),
    ("ragged ranges with FH potentials (min-convolution over the receiving pixel's range), TSGM=3", 1,
     "-P1 2 -P2 20000 -r -16 -R 8 -t census -s vfit -O 8 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="3", CENSUS_NCC_WIN="5", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    ("ragged ranges, FH, TSGM=2 with weights, TSGM_ITER=2", 3,
     "-P1 2 -P2 9 -r -16 -R 8 -t ad -O 4 -aP2 4 -aThresh 12 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="2", TSGM_ITER="2", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    ("ragged ranges, FH, TSGM=4, non-integer costs", 1, "-P1 1.5 -P2 700 -r -16 -R 8 -t sd -O 8 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="4", USE_TRUNCATED_LINEAR_POTENTIALS="1", TESTLRRL="0")),
    ("ragged ranges, FH, TSGM=2 WITHOUT weights (update_cost2_trunclinear and its boundary fix-up)", 1,
     "-P1 2 -P2 9 -r -16 -R 8 -t census -O 8 -s vfit -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="2", USE_TRUNCATED_LINEAR_POTENTIALS="1", CENSUS_NCC_WIN="5")),
    ("ragged ranges, FH, TSGM=2 without weights, 3 channels, TSGM_ITER=2", 3,
     "-P1 1.5 -P2 40 -r -16 -R 8 -t ad -O 4 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="2", TSGM_ITER="2", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    # round 5: ragged volumes of byte costs with windows of at most 62 labels run on their range-proportional copies
    # (mgm_pass_rel.hip, k_wta_rel): every update function, weight, refinement and TSGM_ITER combination that path takes
    ("ragged ranges (range-proportional kernels): census, weights, TSGM=4, cubic", 1,
     "-r -16 -R 8 -t census -O 8 -aP2 4 -aThresh 12 -s cubic -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="4", CENSUS_NCC_WIN="5")),
    ("ragged ranges (range-proportional kernels): census, FH, weights, TSGM=3, TSGM_ITER=2, parabola", 1,
     "-P1 2 -P2 9 -r -16 -R 8 -t census -O 8 -aP2 4 -aThresh 12 -s parabola -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="3", TSGM_ITER="2", CENSUS_NCC_WIN="5", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    ("the same command line on the dense hull (MGM_HIP_REL=0): FH + weights on a ragged volume keeps the consumer-side kernels", 1,
     "-P1 2 -P2 9 -r -16 -R 8 -t census -O 8 -aP2 4 -aThresh 12 -s parabola -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="3", TSGM_ITER="2", CENSUS_NCC_WIN="5", USE_TRUNCATED_LINEAR_POTENTIALS="1", MGM_HIP_REL="0")),
    ("ragged ranges (range-proportional kernels): census, TSGM=1, O 2, no over-count fix, TSGM_ITER=3, parabolaOCV", 1,
     "-r -16 -R 8 -t census -O 2 -s parabolaOCV -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="1", TSGM_ITER="3", TSGM_FIX_OVERCOUNT="0", CENSUS_NCC_WIN="3")),
    ("ragged ranges (range-proportional kernels): grey ad (byte costs), FH TSGM=4, median, O 4", 1,
     "-P1 2 -P2 30 -r -16 -R 8 -t ad -truncDist 100 -O 4 -s vfit -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="4", MEDIAN="1", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    ("ragged ranges (range-proportional kernels): census 3x3 colour, Hirschmueller TSGM=3, TSGM_ITER=2", 3,
     "-r -16 -R 8 -t census -O 8 -s vfit -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="3", TSGM_ITER="2", CENSUS_NCC_WIN="3")),
    # mgm_naive_parallelism (mgm_core.cc:632-831): with one thread the reference accumulates S in pass order
    ("WITH_MGM2=1 (direction-parallel driver), census FH vfit, reference on one thread", 1, "-P1 2 -P2 20000 -r -16 -R 8 -t census -s vfit -O 8",
     dict(TSGM="3", WITH_MGM2="1", OMP_NUM_THREADS="1", CENSUS_NCC_WIN="5", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    ("WITH_MGM2=1, 3 channels, weights, TSGM=4, ad", 3, "-r -20 -R 12 -t ad -O 8 -aP2 4 -aThresh 12",
     dict(TSGM="4", WITH_MGM2="1", OMP_NUM_THREADS="1")),
    # what the reference's `a < b ? a : b` minima make of NaNs: the operand-order-faithful pass kernel (mgm_pass_exact.hip)
    ("ragged ranges with P2 = inf (all-INF slabs, then INF - INF = NaN), Hirschmueller TSGM=3", 1,
     "-P1 8 -P2 inf -r -16 -R 8 -t census -s vfit -O 8 -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="3", CENSUS_NCC_WIN="5", TESTLRRL="0")),
    ("ragged ranges with P2 = inf, TSGM=2, ad, 3 channels, TSGM_ITER=2", 3,
     "-P1 8 -P2 inf -r -16 -R 8 -t ad -O 4 -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="2", TSGM_ITER="2", TESTLRRL="0")),
    ("ragged ranges with P2 = inf, FH TSGM=2 (boundary fix-up) and weights TSGM=4", 1,
     "-P1 2 -P2 inf -r -16 -R 8 -t sd -O 8 -s cubic -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="2", USE_TRUNCATED_LINEAR_POTENTIALS="1", TESTLRRL="0")),
    ("ragged ranges with P2 = inf, weights, TSGM=4", 3,
     "-P1 8 -P2 inf -r -16 -R 8 -t ad -O 8 -aP2 4 -aThresh 12 -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="4", TESTLRRL="0")),
    ("-p census -t ad, 7x7 window: 48-bit descriptors differenced as float WORDS (NaN costs)", 1,
     "-r -16 -R 8 -p census -t ad -s vfit -O 8", dict(TSGM="3", CENSUS_NCC_WIN="7", TESTLRRL="0")),
    ("-p census -t sd, 5x5 window, 3 channels (72 bits), FH, TSGM=2", 3,
     "-P1 2 -P2 9 -r -12 -R 9 -p census -t sd -O 4", dict(TSGM="2", CENSUS_NCC_WIN="5", USE_TRUNCATED_LINEAR_POTENTIALS="1", TESTLRRL="0")),
    ("median radius 9 (beyond the pairwise-counting kernel: radix selection)", 1, "-r -16 -R 8 -t census -s vfit -O 4",
     dict(TSGM="2", MEDIAN="9", CENSUS_NCC_WIN="5")),
    ("2500 labels (beyond every fast kernel: the generic pass and WTA kernels), census, TSGM_ITER=2", 1,
     "-r -1250 -R 1249 -t census -O 4 -s vfit", dict(TSGM="2", TSGM_ITER="2", CENSUS_NCC_WIN="5")),
    ("2100 labels, FH, weights, TSGM=3", 3, "-P1 2 -P2 9 -r -1050 -R 1049 -t ad -O 8 -aP2 4 -aThresh 12 -s cubic",
     dict(TSGM="3", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    # main()'s iteration loops compare an int with the DOUBLE TSGM_ITER (mgm.cc:377, 406): none at all for 0 (the maps stay
    # the zero images they were allocated as), two for 1.5
    ("TSGM_ITER=0: no call of mgm() at all", 1, "-r -16 -R 8 -t census -s vfit -O 8", dict(TSGM="3", TSGM_ITER="0", MEDIAN="1")),
    ("TSGM_ITER=1.5: two iterations", 3, "-r -20 -R 12 -t ad -O 4 -s parabola", dict(TSGM="2", TSGM_ITER="1.5")),
    ("601 labels (the reference's Dvec has no label limit), ad, 3 channels", 3, "-r -300 -R 300 -t ad -O 4 -s vfit", dict(TSGM="2")),
    ("parabolaOCV, census, median radius 3, tight tau", 1, "-r -16 -R 8 -t census -s parabolaOCV -O 8",
     dict(TSGM="3", MEDIAN="3", TESTLRRL_TAU="0.5", CENSUS_NCC_WIN="5")),
]


def compare_outputs(outs, nx, ny, nch, what):
    """stdout and every output file of the two programs, bit for bit -- except where the reference itself is undefined
    (see the comments below)."""
    assert outs["ref"][0] == outs["ours"][0], ("stdout differs", what)
    assert outs["ref"][1].keys() == outs["ours"][1].keys(), what
    for f in outs["ref"][1]:
        a, b = outs["ref"][1][f], outs["ours"][1][f]
        assert a.shape == b.shape, (f, what)
        if f == "cost.npy":
            # A pixel without any finite S keeps the reference's UNINITIALISED label (mgm_core.cc:594 `float minP;`) and
            # cost +INF; what the refinement then makes of that label is undefined (NaN or +INF, seen 2x in 3500 random
            # command lines).  Here such a pixel gets a NaN label and keeps +INF: same pixels, no value to compare.
            fa, fb = np.isfinite(a), np.isfinite(b)
            assert np.array_equal(fa, fb), (f, what)
            a, b = np.where(fa, a, 0), np.where(fb, b, 0)
        else:
            # ... and the LABEL of such a pixel is the uninitialised `float minP` itself (seen as -111 in one of 4000 random
            # command lines): not compared where both sides report no finite cost
            nofin = ~(np.isfinite(outs["ref"][1]["cost.npy"]) | np.isfinite(outs["ours"][1]["cost.npy"])).reshape(ny, nx)
            m = np.broadcast_to(nofin[:, :, None], a.reshape(ny, nx, -1).shape).reshape(a.shape)
            a, b = np.where(m, 0, a), np.where(m, 0, b)
        if f == "back.npy":
            # The reference indexes v with a FLOAT expression, x + d + y*nx + c*npix (mgm.cc:437): in the last row of the
            # last channel a sub-pixel disparity just below the image border rounds up to npix*nch, one element past the end
            # of its vector -- it copies whatever the heap holds there (seen once in 2500 random command lines); the
            # library reads the last element instead.  Same pixels from the same formula; not compared.
            d32 = outs["ref"][1]["disp.npy"].reshape(ny, nx).astype(np.float32)
            with np.errstate(invalid="ignore"):
                k = (np.arange(nx, dtype=np.float32)[None, :] + d32) + (np.arange(ny, dtype=np.float32)[:, None] * np.float32(nx))
                past = np.stack([(k + np.float32(c * nx * ny)) >= np.float32(nx * ny * nch) for c in range(nch)], axis=-1)
            a = np.where(past.reshape(a.shape), 0, a)
            b = np.where(past.reshape(b.shape), 0, b)
        assert ndiff(a, b) == 0, (f, what)


@pytest.mark.skipif(not os.path.exists(REF), reason="reference CLI (oracle/_ref/mgm) was not built")
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_cli_matches_reference(case, tmp_path):
    name, nch, args, env = case
    u, v, gt = synth.stereo_pair(112, 72, -16, 8, seed=42, nch=nch)
    np.save(tmp_path / "u.npy", np.ascontiguousarray(u.transpose(1, 2, 0)) if nch > 1 else u[0])
    np.save(tmp_path / "v.npy", np.ascontiguousarray(v.transpose(1, 2, 0)) if nch > 1 else v[0])
    if "{ranges}" in args:  # per-pixel range images around the true disparity, as a coarse-to-fine caller would pass
        rng = np.random.default_rng(8)
        gt2 = np.asarray(gt, np.float32).reshape(72, 112)
        lo = np.floor(gt2 - rng.integers(1, 7, size=gt2.shape)).astype(np.float32) + rng.random(gt2.shape).astype(np.float32)
        hi = lo + rng.integers(0, 14, size=gt2.shape).astype(np.float32)      # some ranges empty: main() repairs them
        lo[rng.random(gt2.shape) < 0.02] = np.nan                             # ... and replaces non-finite bounds
        hi[rng.random(gt2.shape) < 0.02] = np.inf
        np.save(tmp_path / "lo.npy", lo)
        np.save(tmp_path / "hi.npy", hi)
    outs = {}
    for tag, exe in (("ref", REF), ("ours", OURS)):
        d = tmp_path / tag
        d.mkdir()
        a = args.format(tmp=d, ranges=tmp_path).split()
        cmd = [exe] + a + [str(tmp_path / "u.npy"), str(tmp_path / "v.npy"), str(d / "disp.npy"), str(d / "cost.npy"),
                           str(d / "back.npy")]
        e = dict(os.environ, **dict(dict(OMP_NUM_THREADS="4", MGM_HIP_KERNELS="1"), **env))
        r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (tag, r.stderr)
        outs[tag] = (r.stdout, {f: np.load(d / f) for f in sorted(os.listdir(d))})
        if tag == "ours":  # which pass kernel did the command line take? (the ragged cases must say so)
            kernels = [ln for ln in r.stderr.splitlines() if ln.startswith("[mgm kernels]")]
            assert kernels, r.stderr
            ran = set(" ".join(kernels).split()[2:])
            if "(range-proportional kernels)" in name:
                assert "k_pass_rel" in ran, (name, sorted(ran))
            if env.get("MGM_HIP_REL") == "0" or "P2 = inf" in name:
                assert "k_pass_rel" not in ran, (name, sorted(ran))
            if "P2 = inf" in name or name.startswith("-p census"):
                assert "k_pass_exact" in ran, (name, sorted(ran))
    # NaN costs: pixels without a finite S exist, whose label is the reference's uninitialised `float minP` (these cases run
    # with TESTLRRL=0: the left-right check would carry that garbage into its neighbours' verdicts)
    if "P2 = inf" in name or name.startswith("-p census"):
        return compare_outputs(outs, 112, 72, nch, name)
    assert outs["ref"][0] == outs["ours"][0], "stdout differs"
    assert outs["ref"][1].keys() == outs["ours"][1].keys()
    for f in outs["ref"][1]:
        a, b = outs["ref"][1][f], outs["ours"][1][f]
        assert a.shape == b.shape, f
        assert ndiff(a, b) == 0, (name, f)


@pytest.mark.skipif(not os.path.exists(REF), reason="reference CLI (oracle/_ref/mgm) was not built")
@pytest.mark.parametrize("devices", ["0,0", "0,0,0,0,0"])
def test_cli_on_several_devices_matches_reference(devices, tmp_path):
    """MGM_DEVICES: both mgm() runs of the pair with their passes sharded over several "devices" (loopback ranks on the
    one GPU of the box: mgm_multi_aggregate) -- stdout and outputs must still be the reference's."""
    u, v, _ = synth.stereo_pair(112, 72, -16, 8, seed=42, nch=3)
    np.save(tmp_path / "u.npy", np.ascontiguousarray(u.transpose(1, 2, 0)))
    np.save(tmp_path / "v.npy", np.ascontiguousarray(v.transpose(1, 2, 0)))
    args = "-P2 20000 -P1 2 -r -20 -R 12 -t census -s vfit -O 8 -aP2 4 -aThresh 12".split()
    env = dict(MEDIAN="1", CENSUS_NCC_WIN="3", USE_TRUNCATED_LINEAR_POTENTIALS="1", TSGM="3")
    outs = {}
    for tag, exe, extra in (("ref", REF, {}), ("ours", OURS, dict(MGM_DEVICES=devices, MGM_MULTI_LOOPBACK="1"))):
        d = tmp_path / tag
        d.mkdir()
        cmd = [exe] + args + [str(tmp_path / "u.npy"), str(tmp_path / "v.npy"), str(d / "disp.npy"), str(d / "cost.npy")]
        r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="4", **env, **extra), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (tag, r.stderr)
        outs[tag] = (r.stdout, {f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert outs["ref"][0] == outs["ours"][0], "stdout differs"
    for f in outs["ref"][1]:
        assert ndiff(outs["ref"][1][f], outs["ours"][1][f]) == 0, f


def test_cli_runs_what_round_2_refused(tmp_path):
    u, v, _ = synth.stereo_pair(32, 16, -4, 4)
    np.save(tmp_path / "u.npy", u[0])
    np.save(tmp_path / "v.npy", v[0])
    base = [OURS, str(tmp_path / "u.npy"), str(tmp_path / "v.npy"), str(tmp_path / "d.npy")]
    lo = np.zeros((16, 32), np.float32) - 4
    lo[3, 3] = -2
    np.save(tmp_path / "lo.npy", lo)
    np.save(tmp_path / "hi.npy", lo + 6)
    ragged = ["-m", str(tmp_path / "lo.npy"), "-M", str(tmp_path / "hi.npy")]
    # what round 2 still refused now runs (on the operand-order-faithful pass kernel): a ragged volume with P2 = +INF, and
    # -p census with another distance from descriptors of more than 24 bits (words differenced as floats: NaN costs)
    for extra, env in ((ragged + ["-P2", "inf"], {}), (["-p", "census", "-t", "ad"], dict(CENSUS_NCC_WIN="7"))):
        r = subprocess.run(base[:1] + extra + base[1:], env=dict(os.environ, **env), capture_output=True, text=True)
        assert r.returncode == 0, (extra, env, r.stderr)


REF_IMG = os.path.join(ROOT, "oracle", "_ref", "mgm_img")  # the reference CLI with iio's PNG/TIFF support
CONV = os.path.join(ROOT, "mgm_amd", "bin", "imgconv")

MAKEFILE_TESTS = [  # the two command lines of the reference's `make test` (Makefile:16-18), on PNG files, TIFF outputs
    ("-P2 20000 -P1 2 -r -20 -R 12 -t census -s vfit -O 8", dict(MEDIAN="1", CENSUS_NCC_WIN="3", USE_TRUNCATED_LINEAR_POTENTIALS="1", TSGM="3")),
    ("-P2 20000 -P1 4 -r -20 -R 12 -p sobel_x -truncDist 63 -s vfit -O 8", dict(MEDIAN="1", USE_TRUNCATED_LINEAR_POTENTIALS="1", TSGM="3")),
]


@pytest.mark.skipif(not os.path.exists(REF_IMG), reason="oracle/_ref/mgm_img was not built (needs libpng/libtiff headers)")
@pytest.mark.parametrize("case", MAKEFILE_TESTS, ids=["census", "sobel_x"])
def test_cli_png_in_tiff_out_matches_reference(case, tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    args, env = case
    u, v, _ = synth.stereo_pair(112, 72, -16, 8, seed=43, nch=3)
    for n, a in (("u", u), ("v", v)):
        PIL.fromarray(np.clip(np.round(a.transpose(1, 2, 0)), 0, 255).astype(np.uint8)).save(tmp_path / (n + ".png"))
    outs = {}
    for tag, exe in (("ref", REF_IMG), ("ours", OURS)):
        d = tmp_path / tag
        d.mkdir()
        cmd = [exe] + args.split() + [str(tmp_path / "u.png"), str(tmp_path / "v.png"), str(d / "disp.tif"), str(d / "cost.tif"), str(d / "back.tif")]
        r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="4", **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (tag, r.stderr)
        files = {}
        for f in ("disp", "cost", "back"):
            c = subprocess.run([CONV, str(d / (f + ".tif")), str(d / (f + ".npy"))], capture_output=True, text=True)
            assert c.returncode == 0, (tag, f, c.stderr)
            files[f] = np.load(d / (f + ".npy"))
        outs[tag] = (r.stdout, files)
    assert outs["ref"][0] == outs["ours"][0], "stdout differs"
    for f in outs["ref"][1]:
        a, b = outs["ref"][1][f], outs["ours"][1][f]
        assert a.shape == b.shape and np.isfinite(a).any(), f
        assert ndiff(a, b) == 0, f


FUZZ_N = int(os.environ.get("MGM_FUZZ_N", "0"))
FUZZ_BASE = int(os.environ.get("MGM_FUZZ_BASE", "0"))


@pytest.mark.skipif(not os.path.exists(REF), reason="reference CLI (oracle/_ref/mgm) was not built")
@pytest.mark.parametrize("seed", range(FUZZ_BASE, FUZZ_BASE + (FUZZ_N or 24)))
def test_cli_random_options_match_reference(seed, tmp_path):
    """Random command lines (every option and environment parameter of the reference's main(), small images):
    the paths only the whole program exercises -- TSGM_ITER windows, ragged ranges, post-processing."""
    rng = np.random.default_rng(77000 + seed)
    nch = int(rng.choice([1, 3]))
    nx, ny = int(rng.integers(8, 90)), int(rng.integers(6, 60))
    dmin = int(rng.integers(-20, 1))
    dmax = dmin + int(rng.integers(2, 40))
    if rng.random() < 0.15:  # label counts across the kernel-selection thresholds (64, 128, 192, 256 ...)
        dmin = int(rng.integers(-200, 1))
        dmax = dmin + int(rng.choice([62, 63, 64, 100, 126, 127, 128, 150, 191, 192, 255, 256, 300]))
    u, v, gt = synth.stereo_pair(nx, ny, max(dmin, -16), min(dmax, 8) if min(dmax, 8) > max(dmin, -16) else max(dmin, -16) + 1,
                                 seed=int(rng.integers(0, 1000)), nch=nch)
    np.save(tmp_path / "u.npy", np.ascontiguousarray(u.transpose(1, 2, 0)) if nch > 1 else u[0])
    np.save(tmp_path / "v.npy", np.ascontiguousarray(v.transpose(1, 2, 0)) if nch > 1 else v[0])
    fh = int(rng.integers(0, 2))
    P1, P2 = [(8, 32), (2, 9), (1.5, 700), (4, 20000), (0.5, 3.25)][int(rng.integers(0, 5))]
    args = ["-r", str(dmin), "-R", str(dmax), "-O", str(int(rng.choice([1, 2, 3, 4, 5, 6, 7, 8, 4, 8]))),
            "-P1", str(P1), "-P2", str(P2),
            "-t", str(rng.choice(["ad", "sd", "census", "ncc", "btad", "btsd"])),
            "-p", str(rng.choice(["none", "none", "census", "sobelx", "gblur"])),
            "-s", str(rng.choice(["none", "vfit", "parabola", "cubic", "parabolaOCV"]))]
    if rng.random() < 0.3:
        args += ["-aP2", str(rng.choice([4, 0.3])), "-aThresh", str(rng.choice([5, 12]))]
    if rng.random() < 0.3:
        args += ["-truncDist", str(rng.choice([63, 300, 20]))]
    env = dict(TSGM=str(int(rng.integers(1, 5))), TSGM_ITER=str(int(rng.choice([1, 1, 2, 3]))),
               TSGM_FIX_OVERCOUNT=str(int(rng.integers(0, 2))), USE_TRUNCATED_LINEAR_POTENTIALS=str(fh),
               MEDIAN=str(int(rng.choice([0, 0, 1, 2]))), TESTLRRL=str(int(rng.integers(0, 2))),
               TESTLRRL_TAU=str(rng.choice([1.0, 0.5, 2.5])), CENSUS_NCC_WIN=str(int(rng.choice([3, 5, 7]))))
    if rng.random() < 0.3:  # per-pixel range images, some empty or non-finite: main() repairs them
        lo = np.floor(rng.integers(dmin - 3, dmax, size=(ny, nx))).astype(np.float32) + rng.random((ny, nx)).astype(np.float32)
        hi = lo + rng.integers(0, 14, size=(ny, nx)).astype(np.float32)
        lo[rng.random((ny, nx)) < 0.02] = np.nan
        hi[rng.random((ny, nx)) < 0.02] = np.inf
        np.save(tmp_path / "lo.npy", lo)
        np.save(tmp_path / "hi.npy", hi)
        args += ["-m", str(tmp_path / "lo.npy"), "-M", str(tmp_path / "hi.npy")]
    # `-p census` with another distance differences the descriptor words as floats: NaN costs beyond 24 bits, pixels without a
    # finite S and with them the reference's uninitialised label, which its left-right check and its median filter would
    # spread into the neighbours, and update_dmin_dmax (TSGM_ITER > 1) into the next iteration's windows: none of the three
    # there (seen in 18 + 11 of 1200 + 1500 random command lines with them on)
    win = int(env["CENSUS_NCC_WIN"])
    if args[args.index("-p") + 1] == "census" and args[args.index("-t") + 1] != "census" and nch * (win * win - 1) > 24:
        env["TESTLRRL"], env["MEDIAN"], env["TSGM_ITER"] = "0", "0", "1"
    outs = {}
    for tag, exe in (("ref", REF), ("ours", OURS)):
        d = tmp_path / tag
        d.mkdir()
        cmd = [exe] + args + ["-l", str(d / "nolr.npy"), str(tmp_path / "u.npy"), str(tmp_path / "v.npy"), str(d / "disp.npy"),
                              str(d / "cost.npy"), str(d / "back.npy")]
        r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS="2", **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (tag, " ".join(args), env, r.stderr)
        outs[tag] = (r.stdout, {f: np.load(d / f) for f in sorted(os.listdir(d))})
    compare_outputs(outs, nx, ny, nch, (" ".join(args), env, nx, ny, nch))
    if FUZZ_N:  # long campaigns: do not let thousands of test directories pile up on the box
        import shutil
        shutil.rmtree(tmp_path, ignore_errors=True)


@pytest.mark.skipif(not os.path.exists(REF), reason="reference CLI (oracle/_ref/mgm) was not built")
def test_resident_batch_mode_matches_reference_pair_by_pair(tmp_path):
    """`mgm --batch FILE`: several command lines in ONE process on one device context (round 4).  Per pair, stdout and every
    output file must be what the reference binary gives for that command line run on its own -- different sizes, costs,
    potentials and weights in turn, so that the context's workspace, task tables and hand-off slots are reused across
    geometries."""
    env = dict(MEDIAN="1", CENSUS_NCC_WIN="3", USE_TRUNCATED_LINEAR_POTENTIALS="1", TSGM="3")
    jobs = [("a", 112, 72, 1, "-P2 20000 -P1 2 -r -20 -R 12 -t census -s vfit -O 8"),
            ("b", 96, 80, 3, "-r -16 -R 8 -t ad -O 4 -s parabola"),
            ("c", 112, 72, 1, "-P2 20000 -P1 2 -r -20 -R 12 -t census -s vfit -O 8 -aP2 4 -aThresh 12"),
            ("d", 64, 48, 1, "-r -12 -R 9 -t ncc -O 8 -s cubic"),
            ("e", 112, 72, 1, "-P2 20000 -P1 2 -r -20 -R 12 -t census -s vfit -O 8")]
    lines, ref_stdout = [], ""
    for tag, nx, ny, nch, args in jobs:
        u, v, _ = synth.stereo_pair(nx, ny, -16, 8, seed=50 + len(lines), nch=nch)
        np.save(tmp_path / (tag + "_u.npy"), np.ascontiguousarray(u.transpose(1, 2, 0)) if nch > 1 else u[0])
        np.save(tmp_path / (tag + "_v.npy"), np.ascontiguousarray(v.transpose(1, 2, 0)) if nch > 1 else v[0])
        files = lambda who: [str(tmp_path / (tag + "_u.npy")), str(tmp_path / (tag + "_v.npy"))] + [str(tmp_path / ("%s_%s_%s.npy" % (who, tag, k))) for k in ("disp", "cost", "back")]
        r = subprocess.run([REF] + args.split() + files("ref"), env=dict(os.environ, OMP_NUM_THREADS="4", **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        ref_stdout += r.stdout
        lines.append(" ".join(args.split() + files("ours")) + ("   # pair %s" % tag))
    (tmp_path / "list.txt").write_text("# five pairs, one process\n\n" + "\n".join(lines) + "\n")
    r = subprocess.run([OURS, "--batch", str(tmp_path / "list.txt")], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ref_stdout, "stdout differs"
    for tag, nx, ny, nch, args in jobs:
        for k in ("disp", "cost", "back"):
            a, b = np.load(tmp_path / ("ref_%s_%s.npy" % (tag, k))), np.load(tmp_path / ("ours_%s_%s.npy" % (tag, k)))
            assert a.shape == b.shape and ndiff(a, b) == 0, (tag, k)
    # a line that fails (missing file) does not stop the others, and the exit code says so
    (tmp_path / "list2.txt").write_text(lines[0] + "\n-r -4 -R 4 /nonexistent/u.npy /nonexistent/v.npy " + str(tmp_path / "x.npy") + "\n" + lines[4] + "\n")
    r = subprocess.run([OURS, "--batch", str(tmp_path / "list2.txt")], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "line 2 failed" in r.stderr
    assert ndiff(np.load(tmp_path / "ours_e_disp.npy"), np.load(tmp_path / "ref_e_disp.npy")) == 0


@pytest.mark.skipif(not os.path.exists(REF), reason="reference CLI (oracle/_ref/mgm) was not built")
def test_resident_batch_lines_may_consume_earlier_outputs(tmp_path):
    """in `mgm --batch` the decoder works ahead of the device stage -- a line whose -m/-M files are an EARLIER line's
    outputs (a coarse-to-fine chain) must see them complete: per line, the same files as the reference binary run line by line."""
    u, v, _ = synth.stereo_pair(112, 72, -16, 8, seed=61)
    np.save(tmp_path / "u.npy", u[0])
    np.save(tmp_path / "v.npy", v[0])
    env = dict(TSGM="3", CENSUS_NCC_WIN="5", TESTLRRL="0")
    # line 1 writes a disparity map and a cost map; lines 2 and 3 use those two FILES as their range images (any float image
    # will do for the purpose: main() repairs empty ranges and non-finite bounds, mgm.cc:342-353)
    def lines_for(who):
        d1, c1 = str(tmp_path / (who + "_d1.npy")), str(tmp_path / (who + "_c1.npy"))
        base = [str(tmp_path / "u.npy"), str(tmp_path / "v.npy")]
        return [["-r", "-16", "-R", "8", "-t", "census", "-O", "4"] + base + [d1, c1],
                ["-r", "-16", "-R", "8", "-t", "census", "-O", "8", "-s", "vfit", "-m", d1, "-M", c1] + base + [str(tmp_path / (who + "_d2.npy"))],
                ["-r", "-16", "-R", "8", "-t", "census", "-O", "4", "-P1", "2", "-P2", "30", "-m", d1, "-M", c1] + base + [str(tmp_path / (who + "_d3.npy"))]]
    ref_stdout = ""
    for a in lines_for("ref"):
        r = subprocess.run([REF] + a, env=dict(os.environ, OMP_NUM_THREADS="4", **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        ref_stdout += r.stdout
    (tmp_path / "chain.txt").write_text("\n".join(" ".join(a) for a in lines_for("ours")) + "\n")
    for _ in range(3):  # (a race shows up some of the time: run it a few times)
        r = subprocess.run([OURS, "--batch", str(tmp_path / "chain.txt")], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert r.stdout == ref_stdout
        for k in ("d1", "c1", "d2", "d3"):
            a, b = np.load(tmp_path / ("ref_%s.npy" % k)), np.load(tmp_path / ("ours_%s.npy" % k))
            assert a.shape == b.shape and ndiff(a, b) == 0, k
        for k in ("d1", "c1", "d2", "d3"):
            os.remove(tmp_path / ("ours_%s.npy" % k))


@pytest.mark.skipif(not os.path.exists(REF), reason="reference CLI (oracle/_ref/mgm) was not built")
@pytest.mark.parametrize("half", [24, 50], ids=["windows_of_49", "windows_of_101"])
def test_full_size_ragged_command_line_matches_reference(half, tmp_path):
    """tools/ragged_cli.sh as a test: the whole command line on a 1920x1080 pair with -m/-M range images (per-pixel
    windows inside a 256-label hull; FH, TSGM 3, 8 directions, vfit, median, left-right check) against the reference binary on
    the same files -- and the left-to-right run must have taken the range-proportional kernels (64 / 128 slots per pixel)."""
    u, v, gt = synth.stereo_pair(1920, 1080, -191, 0, seed=20150907)
    np.save(tmp_path / "u.npy", u[0])
    np.save(tmp_path / "v.npy", v[0])
    np.save(tmp_path / "lo.npy", np.clip(gt - half, -255, 0).astype(np.float32))
    np.save(tmp_path / "hi.npy", np.clip(gt + half, -255, 0).astype(np.float32))
    args = "-r -255 -R 0 -t census -s vfit -O 8 -P1 2 -P2 20000 -m {t}/lo.npy -M {t}/hi.npy".format(t=tmp_path).split()
    env = dict(CENSUS_NCC_WIN="5", TSGM="3", USE_TRUNCATED_LINEAR_POTENTIALS="1", MEDIAN="1", MGM_HIP_KERNELS="1")
    outs = {}
    for tag, exe in (("ref", REF), ("ours", OURS)):
        d = tmp_path / tag
        d.mkdir()
        cmd = [exe] + args + [str(tmp_path / "u.npy"), str(tmp_path / "v.npy"), str(d / "disp.npy"), str(d / "cost.npy")]
        r = subprocess.run(cmd, env=dict(os.environ, OMP_NUM_THREADS=str(min(32, len(os.sched_getaffinity(0)))), **env),
                           capture_output=True, text=True, timeout=1200)
        assert r.returncode == 0, (tag, r.stderr[-2000:])
        outs[tag] = (r.stdout, {f: np.load(d / f) for f in sorted(os.listdir(d))}, r.stderr)
    assert outs["ref"][0] == outs["ours"][0], "stdout differs"
    kernels = " ".join(ln for ln in outs["ours"][2].splitlines() if ln.startswith("[mgm kernels]")).split()
    assert "k_pass_rel" in kernels, kernels
    for f in ("disp.npy", "cost.npy"):
        assert ndiff(outs["ref"][1][f], outs["ours"][1][f]) == 0, f


def test_resident_batch_lines_with_the_last_filters_match_their_one_shot_runs(tmp_path):
    """The end of a job -- speckle filter, classified hole filling, the downloads, the back-projected image -- is one function for the
    single-scale and the coarse-to-fine driver, and in `mgm --batch` the device objects of a pair are kept for the next one: four lines
    under MGM_SPECKLE, MGM_FILL_HOLES, MGM_FILL_HOLES_OCC and MEDIAN, a -S 2 line and another geometry between two equal lines.  Per
    line, stdout and every output file are, byte for byte, what the same binary writes for that line run on its own; the first and
    the last line give the same bytes (the kept objects were refilled, not stale)."""
    env = dict(os.environ, MGM_SPECKLE="8", MGM_FILL_HOLES="median", MGM_FILL_HOLES_OCC="sechigh", MEDIAN="1")
    for tag, nx, ny, nch, d in (("a", 64, 48, 1, 8), ("b", 48, 40, 3, 6)):
        u, v, _ = synth.stereo_pair(nx, ny, -d, d, seed=70 + nch, nch=nch)
        np.save(tmp_path / (tag + "_u.npy"), np.ascontiguousarray(u.transpose(1, 2, 0)) if nch > 1 else u[0])
        np.save(tmp_path / (tag + "_v.npy"), np.ascontiguousarray(v.transpose(1, 2, 0)) if nch > 1 else v[0])
    jobs = [("a", "-r -8 -R 8"), ("a", "-r -8 -R 8 -S 2"), ("b", "-r -6 -R 6"), ("a", "-r -8 -R 8")]
    OUT = ("nolr", "disp", "cost", "back")

    def line(who, k):
        tag, args = jobs[k]
        d = tmp_path / ("%s%d" % (who, k))
        d.mkdir()
        return ("-t census -O 4 " + args).split() + ["-l", str(d / "nolr.npy"), str(tmp_path / (tag + "_u.npy")), str(tmp_path / (tag + "_v.npy"))] + \
            [str(d / (f + ".npy")) for f in OUT[1:]]

    stdout = ""
    for k in range(len(jobs)):
        r = subprocess.run([OURS] + line("one", k), env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (k, r.stderr)
        stdout += r.stdout
    (tmp_path / "list.txt").write_text("".join(" ".join(line("batch", k)) + "\n" for k in range(len(jobs))))
    r = subprocess.run([OURS, "--batch", str(tmp_path / "list.txt")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout == stdout and stdout.count("\n") > 3 * len(jobs)
    files = lambda who, k: [(tmp_path / ("%s%d" % (who, k)) / (f + ".npy")).read_bytes() for f in OUT]
    for k in range(len(jobs)):
        assert files("batch", k) == files("one", k), k
    assert files("batch", 0) == files("batch", 3)
    disp, nolr = (np.load(tmp_path / "batch0" / (f + ".npy")) for f in ("disp", "nolr"))
    assert ndiff(disp, nolr) > 0  # (the filters and the fill had something to do)
