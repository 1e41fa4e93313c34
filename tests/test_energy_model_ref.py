"""The numpy model of the solution energy (tests/energy_model.py):

  kinds 0-2 on the REFERENCE BINARY: oracle/_ref/mgm with TSGM_DEBUG=1 prints evaluate_energy_4connected's three figures per
            iteration and run (%.9e names an fp32 value uniquely); the model, fed with the CPU oracle's cost volume and unrefined
            labels, must give the same bits, and the file the reference writes must equal the model's L1 map
  kind 3    against a scalar restatement in plain loops
  the copy  plan_energy_copy / plan_energy_launch (mgm_amd/csrc/mgm_energyplan.h) on the host

The reference's label is uninitialised where a pixel has no finite cost (mgm_core.cc:594), so every case asserts that the oracle's
label maps are all finite: only such inputs pin anything."""
import ctypes as C
import io
import os
import struct
import subprocess
import time

import numpy as np
import pytest

import energy_model as em
import energy_runs as er
from mgm_amd import synth
from oracle.oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgm_amd", "csrc")
F = np.float32

REF_CASES = [
    # (name, (nx, ny, seed, gt range), nch, args, env)
    ("census 3x3, O8, TSGM=3", (40, 24, 1, (-8, 4)), 1, "-r -8 -R 4 -t census -O 8", dict(TSGM="3")),
    ("ad, 3 channels (P1 * nch), O2, TSGM=2", (112, 72, 42, (-16, 8)), 3, "-r -16 -R 8 -t ad -O 2 -P1 3 -P2 11", dict(TSGM="2")),
    ("sd, truncated, 1 channel, no LR run", (40, 24, 1, (-8, 4)), 1, "-r -9 -R 6 -t sd -truncDist 300 -O 4", dict(TSGM="1", TESTLRRL="0")),
    ("weights, 3 channels, O8", (40, 24, 3, (-8, 4)), 3, "-r -8 -R 4 -t ad -O 8 -aP2 4 -aThresh 12", dict(TSGM="3")),
    ("FH potentials, census 5x5, vfit", (112, 72, 42, (-16, 8)), 1, "-P1 2 -P2 9 -r -16 -R 8 -t census -s vfit -O 8",
     dict(TSGM="3", CENSUS_NCC_WIN="5", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
    ("TSGM_ITER=2, vfit", (112, 72, 42, (-16, 8)), 1, "-r -16 -R 8 -t census -s vfit -O 8", dict(TSGM="3", TSGM_ITER="2", CENSUS_NCC_WIN="5")),
    ("TSGM_ITER=2, no refinement, 3 channels, no LR run", (40, 24, 2, (-8, 4)), 3, "-r -8 -R 4 -t ad -O 4", dict(TSGM="2", TSGM_ITER="2", TESTLRRL="0")),
    ("-m/-M range images, census vfit", (112, 72, 42, (-16, 8)), 1, "-r -16 -R 8 -t census -s vfit -O 8 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="3", CENSUS_NCC_WIN="5")),
    ("-m/-M range images, ad, weights, TSGM_ITER=2, parabola", (112, 72, 42, (-16, 8)), 3,
     "-r -16 -R 8 -t ad -O 8 -aP2 4 -aThresh 12 -s parabola -m {ranges}/lo.npy -M {ranges}/hi.npy", dict(TSGM="4", TSGM_ITER="2")),
]


@pytest.fixture(scope="module")
def oracle():
    return Oracle(threads=4)


def read_float_tiff(path):
    """an uncompressed one-strip float TIFF by its IFD: (ny, nx) float32 (a reference built without libtiff writes the array in
    .npy form under the same name)"""
    b = open(path, "rb").read()
    if b[:6] == b"\x93NUMPY":
        a = np.load(io.BytesIO(b))
        return np.asarray(a, F).reshape(a.shape[0], a.shape[1])
    e = {b"II": "<", b"MM": ">"}[b[:2]]
    assert struct.unpack(e + "H", b[2:4])[0] == 42
    off = struct.unpack(e + "I", b[4:8])[0]
    tags = {}
    for k in range(struct.unpack(e + "H", b[off:off + 2])[0]):
        tag, typ, cnt = struct.unpack(e + "HHI", b[off + 2 + 12 * k:off + 10 + 12 * k])
        raw = b[off + 10 + 12 * k:off + 14 + 12 * k]
        tags[tag] = (struct.unpack(e + "H", raw[:2])[0] if typ == 3 else struct.unpack(e + "I", raw)[0], cnt)
    nx, ny = tags[256][0], tags[257][0]
    assert tags[259][0] == 1 and tags[258][0] == 32 and tags[273][1] == 1 and tags.get(277, (1, 1))[0] == 1
    return np.frombuffer(b, e + "f4", nx * ny, tags[273][0]).reshape(ny, nx).astype(F)


def model_figures(runs, prm):
    """[(L1trunc, L1, L2)] of every iteration of every run, in the order main() prints them, and the L1 maps"""
    figs, l1 = [], []
    for key in ("L", "R"):
        if key not in runs:
            continue
        r = runs[key]
        for d in r["maps"]:
            assert np.isfinite(d).all(), "a label map with a pixel that has no finite cost pins nothing"
            maps = [em.energy_map(r["C"], r["hmin"], d, kind, prm["P1"], prm["P2"], lo=r["lo"], hi=r["hi"])[0] for kind in (0, 1, 2)]
            figs.append(tuple(em.serial_sum(m) for m in maps))
            l1.append(maps[1])
    return figs, l1


@pytest.mark.skipif(not os.path.exists(er.REF), reason="reference CLI (oracle/_ref/mgm) was not built")
@pytest.mark.parametrize("case", REF_CASES, ids=lambda c: c[0])
def test_reference_figures(case, oracle, tmp_path):
    name, (nx, ny, seed, (gmin, gmax)), nch, args, env = case
    u, v, gt = synth.stereo_pair(nx, ny, gmin, gmax, seed=seed, nch=nch)
    tmp = str(tmp_path)
    er.save_pair(tmp, u, v)
    lo = hi = None
    if "{ranges}" in args:
        lo, hi = er.cli_ranges(gt, ny, nx)
        np.save(tmp_path / "lo.npy", lo)
        np.save(tmp_path / "hi.npy", hi)
    prm, dmin, dmax = er.params_of(args, env, nch)
    tif = "/tmp/ENERGY_L1trunc.tif"  # (the reference's fixed path)
    t0 = time.time()
    stdout, _, _ = er.run_cli(er.REF, args, env, tmp, str(tmp_path / "ref"), dict(TSGM_DEBUG="1"))
    written = read_float_tiff(tif) if os.path.exists(tif) and os.path.getmtime(tif) >= t0 - 2 else None  # (this run's, not an older one's)
    got = er.debug_figures(stdout)
    runs = er.both_runs(oracle, u, v, dmin, dmax, prm, lo, hi)
    want, l1 = model_figures(runs, prm)
    assert len(got) == prm["iterations"] * (2 if prm["both"] else 1) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        print(name, k, g, w)
        assert [F(x).tobytes() for x in g] == [F(x).tobytes() for x in w], (name, k, g, w)
    if not prm["both"] and prm["iterations"] == 1:
        # the file: written once per call of print_solution_energy, under the truncated kind's name, with the L1 map in it
        assert written is not None and written.shape == l1[0].shape
        assert written.tobytes() == l1[0].tobytes(), name
    # the whole stdout of the debug mode, line by line
    lines = stdout.splitlines()
    assert lines[0] == "%d %d" % (dmin, dmax) and lines[1].startswith("costvolume: ")
    assert sum(ln.startswith("refinement: using ") for ln in lines) == (len(got) if prm["refine"] in er.REFINING else 0)


# ---- kind 3 against the scalar restatement ---------------------------------------------------------------------------------
def crafted(ny, nx, L, seed):
    rng = np.random.default_rng(seed)
    C = (rng.random((ny, nx, L)) * 40).astype(F)
    C[rng.random(C.shape) < 0.05] = np.inf
    d = rng.integers(-3, L + 3, (ny, nx)).astype(F) - 2
    frac = rng.random((ny, nx)) < 0.3
    d[frac] += rng.choice([0.25, 0.5, 0.75, 1.5], frac.sum()).astype(F)
    for val in (np.nan, np.inf, -np.inf, 2.0 ** 24, -2.0 ** 24):
        d[rng.integers(ny), rng.integers(nx)] = val
    w8 = (rng.random((8, ny, nx)) * 3).astype(F)
    lo = rng.integers(-2, 3, (ny, nx)).astype(np.int32)
    hi = lo + rng.integers(0, L, (ny, nx)).astype(np.int32)
    return C, d, w8, lo, hi


@pytest.mark.parametrize("shape", [(1, 7), (7, 1), (2, 2), (3, 3), (5, 9)])
def test_model_energy_against_scalar_restatement(shape):
    ny, nx = shape
    C, d, w8, lo, hi = crafted(ny, nx, 6, 11 * ny + nx)
    for conn in (4, 8):
        for fh in (0, 1):
            for P2 in (5.5, np.inf):
                for w in (None, w8):
                    for rng_ in ((None, None), (lo, hi)):
                        E, _, _ = em.energy_map(C, -2, d, 3, 1.5, P2, conn, fh, w, *rng_)
                        S = em.scalar_model_energy(C, -2, d, 1.5, P2, conn, fh, w, *rng_)
                        assert E.tobytes() == S.tobytes() or np.array_equal(E, S, equal_nan=True), (shape, conn, fh, P2)
                        assert np.array_equal(np.isnan(E), ~np.isfinite(d) | np.isnan(S))


def test_borders_have_no_edge_term_in_kinds_0_to_2():
    """a one-pixel-wide or one-row map: both r and q must lie inside, so every edge term is skipped and E is the data term"""
    for ny, nx in ((1, 7), (7, 1), (1, 1)):
        C, d, _, _, _ = crafted(ny, nx, 6, 5)
        d = np.clip(np.nan_to_num(d, nan=0, posinf=0, neginf=0), -2, 3).astype(F)
        for kind in (0, 1, 2):
            E, data, smooth = em.energy_map(C, -2, d, kind, 2.0, 7.0)
            assert E.tobytes() == (F(0) + data).tobytes() and not smooth.any()


def test_totals_of_the_model():
    C, d, w8, _, _ = crafted(6, 11, 6, 3)
    C = np.where(np.isfinite(C), C, F(50))
    d = np.clip(np.nan_to_num(d, nan=0, posinf=0, neginf=0), -2, 3).astype(F)
    E, t = em.energy(C, -2, d, 3, 1.5, 6.0, 8, 0, w8)
    assert t["finite"] == t["pixels"] == 66 and abs(t["total"] - (t["data"] + t["smooth"])) <= 1e-3
    s = F(0)
    for x in E.ravel():
        s = F(s + x)
    assert t["serial"].tobytes() == s.tobytes()


# ---- the planner of the copy and of the launch ------------------------------------------------------------------------------
REQ = ("f32_state", "has_f32", "rel_only", "rel_state", "has_rel", "rel_slots", "rel_cb", "p8_state", "has_p8", "p8_L", "p8_cb", "c8_state", "has_c8",
       "cbytes", "L", "unfilled")
NONE, F32, REL, PADDED, COMPACT = range(5)
INVALID, NOSTATE, WRITTEN, VALID = -1, 0, 1, 2


@pytest.fixture(scope="module")
def planlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("energyplan") / "libenergy_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "energy_plan_harness.cc"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    assert lib.energy_request_ints() == len(REQ) and lib.energy_threads() == 256
    return lib


def ask(lib, **kw):
    q = dict(f32_state=0, has_f32=0, rel_only=0, rel_state=NOSTATE, has_rel=0, rel_slots=64, rel_cb=1, p8_state=NOSTATE, has_p8=0, p8_L=0, p8_cb=1,
             c8_state=NOSTATE, has_c8=0, cbytes=1, L=151, unfilled=0)
    for k, v in kw.items():
        assert k in q, k
        q[k] = v
    req = np.array([q[f] for f in REQ], np.int32)
    out = np.zeros(3, np.int32)
    lib.energy_copy_plan(req.ctypes.data_as(C.c_void_p), 1, out.ctypes.data_as(C.c_void_p))
    return tuple(out.tolist())


def test_the_copy_that_is_read(planlib):
    L = 151
    # the fp32 array whenever it is current, whatever else exists
    assert ask(planlib, f32_state=1, has_f32=1) == (F32, 4, L)
    assert ask(planlib, f32_state=1, has_f32=1, c8_state=VALID, has_c8=1, rel_state=VALID, has_rel=1, p8_state=VALID, has_p8=1, p8_L=192) == (F32, 4, L)
    # a stale fp32 array is never read
    assert ask(planlib, f32_state=0, has_f32=1) == (NONE, 0, 0)
    assert ask(planlib, f32_state=0, has_f32=1, c8_state=VALID, has_c8=1, L=128) == (COMPACT, 1, 128)
    assert ask(planlib, c8_state=WRITTEN, has_c8=1, cbytes=2, L=256) == (COMPACT, 2, 256)
    assert ask(planlib, c8_state=INVALID, has_c8=1, L=256) == (NONE, 0, 0)
    assert ask(planlib, c8_state=VALID, has_c8=0, L=256) == (NONE, 0, 0)
    # the padded compact copy: the stride is the padded label count
    assert ask(planlib, p8_state=VALID, has_p8=1, p8_L=192, p8_cb=1) == (PADDED, 1, 192)
    assert ask(planlib, p8_state=VALID, has_p8=1, p8_L=192, p8_cb=2) == (PADDED, 2, 192)
    assert ask(planlib, p8_state=VALID, has_p8=1, p8_L=128) == (NONE, 0, 0)  # (narrower than the labels: not this volume's)
    # the range-proportional copy only where it is the volume's only copy
    for slots, cb in ((64, 1), (128, 1), (64, 2), (128, 4)):
        assert ask(planlib, rel_only=1, rel_state=VALID, has_rel=1, rel_slots=slots, rel_cb=cb) == (REL, cb, slots)
    assert ask(planlib, rel_only=0, rel_state=VALID, has_rel=1) == (NONE, 0, 0)
    assert ask(planlib, rel_only=1, rel_state=WRITTEN, has_rel=1) == (NONE, 0, 0)
    assert ask(planlib, rel_only=1, rel_state=VALID, has_rel=1, f32_state=1, has_f32=1) == (F32, 4, L)  # (expanded since)
    # refusals
    assert ask(planlib, f32_state=1, has_f32=1, unfilled=1) == (NONE, 0, 0)
    assert ask(planlib, f32_state=1, has_f32=0) == (NONE, 0, 0)
    assert ask(planlib, f32_state=1, has_f32=1, L=0) == (NONE, 0, 0)


def test_the_launch_is_a_function_of_the_size(planlib):
    out = np.zeros(2, np.int64)
    for nx, ny in ((1, 7), (7, 1), (16, 16), (257, 1), (65, 5), (1920, 1080), (46340, 46340)):
        planlib.energy_launch_plan(nx, ny, out.ctypes.data_as(C.c_void_p))
        assert out[0] == -(-nx * ny // 256) and out[1] == out[0] * 32, (nx, ny, out)
    for nx, ny in ((0, 5), (5, 0), (-1, 3), (65536, 32768)):
        planlib.energy_launch_plan(nx, ny, out.ctypes.data_as(C.c_void_p))
        assert tuple(out) == (0, 0), (nx, ny)
