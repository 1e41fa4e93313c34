"""The plain winner search, the windowed and right-view searches and every refinement (mgm_wta.hip) on CRAFTED Lr volumes
(tests/wta_crafted.py): engineered ties, winners on the labels around the refinement gate, sums whose value depends on the
pass order, overflow, negative, non-finite, denormal and signed-zero values, flat pixels and pixels without a finite label.

No such value goes through a pass kernel.  The search is reached by two routes of the ABI:
  A. mgm_wta_rows_dev reads its Lr volumes from a buffer of the caller's (a torch tensor) beside any uploaded C;
  B. after an ordinary aggregation of tame costs the context's pass volumes (mgm_lr_device_ptr) are overwritten in place, and
     mgm_wta_windowed_dev / mgm_wta_right_dev read exactly those;
  C. mgm_refine takes an uploaded S and labels of the test's choice.
Everything is compared bit for bit (NaN = NaN) with the numpy restatement and the oracle's refinements, both pinned on the
CPU by tests/test_wta_crafted_ref.py.  The context is the file's own: an overwritten volume never sits in the shared one."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mgm_amd
import test_wta_plan as TP
import wta_crafted as W
import wta_plan_model as PM
from helpers import ndiff
from mgm_amd import dist as mdist
from mgm_amd import synth
from wta_right_model import wta_right

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = list(W.LR_CLASSES)
NDIRS = (1, 3, 4, 5, 8)
DMIN = -5
REACHED = {}  # choice (family, LPL, PPW, EXACT, MAXD, SUB) -> a case that reached it

P, K, Q, A = PM.PLAIN, PM.PACKED, PM.QUAD, PM.ANY
# every choice plan_wta returns for a search outside the last run under the default switches, at the label counts of this file
DECLARED = [
    (K, 4, 4, 1, 4, 4), (K, 4, 2, 1, 8, 4), (K, 4, 4, 1, 4, 2), (K, 4, 2, 1, 8, 2),                 # packed: 64, 128 labels
    (Q, 3, 0, 0, 4, 0), (Q, 3, 0, 0, 8, 0), (Q, 6, 0, 0, 4, 0), (Q, 6, 0, 0, 8, 0),                 # quad: 192, 384
    (P, 1, 4, 1, 8, 1), (P, 2, 4, 1, 8, 1), (P, 3, 2, 1, 8, 1), (P, 4, 3, 1, 8, 1), (P, 6, 1, 1, 8, 1), (P, 8, 1, 1, 8, 1),
    (P, 12, 1, 1, 8, 1), (P, 16, 1, 1, 8, 1),                                                      # plain exact, 64..1024
    (P, 1, 8, 1, 4, 1), (P, 2, 8, 1, 4, 1), (P, 3, 4, 1, 4, 1), (P, 4, 6, 1, 4, 1), (P, 6, 2, 1, 4, 1), (P, 8, 2, 1, 4, 1),  # doubled
    (P, 1, 1, 0, 8, 1), (P, 2, 1, 0, 8, 1), (P, 3, 1, 0, 8, 1), (P, 4, 1, 0, 8, 1), (P, 6, 1, 0, 8, 1), (P, 8, 1, 0, 8, 1),
    (P, 12, 1, 0, 8, 1), (P, 16, 1, 0, 8, 1), (P, 24, 1, 0, 8, 1), (P, 32, 1, 0, 8, 1),            # guarded
    (A, 0, 0, 0, 0, 0),
]
EXACT_WIDTHS = (64, 128, 192, 256, 384, 512, 768, 1024)
GUARDED_WIDTHS = (1, 2, 3, 4, 37, 100, 151, 300, 1100, 1536, 2048)
FEW_PIXELS = (200, 500, 700, 1000, 2048, 2049)  # 1 and 9 pixels only: the guarded instances of 4, 8, 12 and 16 labels per lane, and the widest
WIDTHS = EXACT_WIDTHS + GUARDED_WIDTHS + (200, 500, 700, 1000, 2049)


@pytest.fixture(scope="module")
def own():
    try:
        c = mgm_amd.Context(0)
    except mgm_amd.MgmError as e:
        if e.code == mgm_amd.MGM_ERR_HIP:
            pytest.skip("no MI355X in this box (mgm_ctx_create: MGM_ERR_HIP)")
        raise
    yield c
    c.close()


@pytest.fixture(scope="module")
def planlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("wtacrafted") / "libwta_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", TP.CSRC, os.path.join(ROOT, "tests", "wta_plan_harness.cc"), "-o", so], check=True)
    return C.CDLL(so)


def choice_of(planlib, npix, L, NDIR, refine, window=0, ragged=0, compact=0, cbytes=1, **sw):
    """what plan_wta answers to the request run_wta builds for a search of rows outside the last run (slot < 0): the fused
    kernel takes refinement none and vfit without a window, every other call is a search that writes S, then k_refine"""
    ridx = W.REFINEMENTS.index(refine)
    fused = ridx <= 1 and not window and not ragged
    q = TP.wta_request(npix=npix, L=L, Lreal=L, NDIR=NDIR, cbytes=cbytes, compact=compact, refine=ridx if fused else 0,
                       want_S=0 if (fused or ridx == 0) else 1, window=1 if (window or ragged) else 0, ragged=ragged, in_last_run=0,
                       last_min=0, lr_is_last=0, pix0_zero=0, padded=0, nvol_mod32=(npix * L) % 32, **sw)
    return TP.ask(planlib, "wta", [q])[0][:6]


def group_of(planlib, L, NDIR):
    """pixels a wave takes per turn at this width"""
    fam, LPL, PPW, EXACT, MAXD, SUB = choice_of(planlib, 768, L, NDIR, None)
    return {K: SUB * PPW, Q: 768 // max(L, 1), P: PPW, A: 1}[fam]


def shape_of(n):
    return {65: (5, 13), 130: (10, 13)}.get(n, (1, n))


def counts_of(planlib, L, NDIR):
    if L in FEW_PIXELS:
        return [1, 9]
    g = group_of(planlib, L, NDIR)
    return sorted({n for n in (1, g - 1, g, g + 1) if n >= 1} | {130 if L <= 256 else 65})


def expectation(oracle, lr, Cv, NDIR, fix, refine, dmin):
    S, idx, cost = W.sum_fix_wta(lr, Cv, NDIR, fix)
    lab = (idx + np.float32(dmin)).astype(np.float32)  # NaN where no S is finite: the kernels write NaN and +INF there
    if refine:
        lab, cost = oracle.refine(S, dmin, refine, lab, cost)
    return lab, cost


def run_rows(own, cv, lr, row0, NDIR, fix, refine):
    _, ny, nx, L = lr.shape
    t = torch.from_numpy(np.ascontiguousarray(lr)).cuda()
    out = torch.full((ny, nx), 12345.0, dtype=torch.float32, device="cuda")
    outc = torch.full((ny, nx), 54321.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    own.wta_rows_dev(cv, row0, ny, t.data_ptr(), NDIR, fix, refine, out.data_ptr(), outc.data_ptr())
    own.synchronize()
    return out.cpu().numpy(), outc.cpu().numpy()


def rows_case(own, oracle, planlib, name, cname, L, n, NDIR, fix, refine, seed=0, check_floors=True):
    """one call of mgm_wta_rows_dev over rows [1, 1 + ny) of a volume two rows taller, against the restatement"""
    ny, nx = shape_of(n)
    lr = W.LR_CLASSES[name](100 + seed, NDIR, ny, nx, L)
    pad = W.C_CLASSES[cname](300 + seed, 2, nx, L)  # (the rows of the call keep the pixel numbers of the class: what it plants stays aligned)
    Cv = np.concatenate([pad[:1], W.C_CLASSES[cname](200 + seed, ny, nx, L), pad[1:]])
    if check_floors and (fix == 0 or cname in W.TAME_C):
        W.floors(name, lr, Cv[1:1 + ny], NDIR, fix, L)
    want_o, want_c = expectation(oracle, lr, Cv[1:1 + ny], NDIR, fix, refine, DMIN)
    cv = own.upload_volume(Cv, DMIN)
    got_o, got_c = run_rows(own, cv, lr, 1, NDIR, fix, refine)
    cv.free()
    what = (name, cname, L, n, NDIR, fix, refine)
    ch = choice_of(planlib, n, L, NDIR, refine)
    REACHED.setdefault(ch, what)
    assert ndiff(got_c, want_c) == 0, what + (ch,)
    assert ndiff(got_o, want_o) == 0, what + (ch,)
    return ch


def combo(k, j):
    """(NDIR, fix, refinement, C class) of class k at its j-th pixel count: every class meets every pass count, both settings of
    the fix and all five refinements as j runs"""
    NDIR = NDIRS[(k + j) % 5]
    fix = (k + j // 5 + j) % 2
    cname = ("ints", "frac", "negative", "huge", "nan")[(k + 2 * j) % 5]
    if NDIR == 1 and fix == 1 and j % 2 == 0:
        cname = "inf1"
    return NDIR, fix, W.REFINEMENTS[(2 * k + j) % 5], cname


@pytest.mark.parametrize("L", WIDTHS)
def test_every_class_at_every_width(own, oracle, planlib, L):
    """A: every Lr class at every width, at 1 pixel, one short of a wave's group, one group, one over, and 65 / 130 pixels"""
    for k, name in enumerate(CLASSES):
        j = 0
        for NDIR0 in (8, 4):  # (the group depends on the pass count: both instance sets)
            for n in counts_of(planlib, L, NDIR0):
                NDIR, fix, refine, cname = combo(k, j)
                NDIR = NDIR if (NDIR <= 4) == (NDIR0 <= 4) else NDIR0
                rows_case(own, oracle, planlib, name, cname, L, n, NDIR, fix, refine, seed=j)
                j += 1


@pytest.mark.parametrize("NDIR", NDIRS)
@pytest.mark.parametrize("L", [64, 192, 256, 100])
def test_full_cross(own, oracle, planlib, L, NDIR):
    """A: pass counts x fix x the five refinements, at a pixel count the packed / quad instances take (128) and one they do not
    (65 or 130); the classes in turn, so that every class meets every refinement at every one of these widths"""
    k = 0
    for fix in (0, 1):
        for r, refine in enumerate(W.REFINEMENTS):
            for n in (128, 130 if L <= 256 and L != 192 else 65):
                for name in (CLASSES[(k + NDIR) % 10], CLASSES[(k + NDIR + 5) % 10]):
                    cname = "inf1" if (NDIR == 1 and fix == 1 and k % 3 == 0) else ("ints", "negative", "nan", "frac", "huge")[k % 5]
                    rows_case(own, oracle, planlib, name, cname, L, n, NDIR, fix, refine, seed=k)
                k += 1


@pytest.mark.parametrize("L", [64, 128, 192, 256, 384, 512])
def test_compact_costs(own, oracle, planlib, L):
    """A: the compact forms of C -- one byte per cost (single-word census) and two (absolute differences of a colour pair), built
    on the device; the expectation reads the volume back"""
    nx, ny, dmax = 26, 9, DMIN + L - 1
    for cb, (dist_, nch) in ((1, ("census", 1)), (2, ("ad", 3))):
        u, v, _ = synth.stereo_pair(nx, ny, -4, 6, seed=3, nch=nch)
        du, dv = own.upload_image(u), own.upload_image(v)
        cv = own.costvolume_dev(du, dv, DMIN, dmax, "none", dist_, float("inf"), 5)
        Cv = cv.download()
        assert np.isfinite(Cv).any()
        for k, name in enumerate(CLASSES):
            for rows, j in (((2, 7), 0), ((1, 9), 1)):  # 130 pixels, and 208 (a multiple of 4)
                NDIR, fix, refine = NDIRS[(k + j) % 5], 1, W.REFINEMENTS[(k + j + cb) % 5]
                lr = W.LR_CLASSES[name](300 + k, NDIR, rows[1] - rows[0], nx, L)
                want_o, want_c = expectation(oracle, lr, Cv[rows[0]:rows[1]], NDIR, fix, refine, DMIN)
                got_o, got_c = run_rows(own, cv, lr, rows[0], NDIR, fix, refine)
                what = (name, dist_, L, rows, NDIR, refine)
                REACHED.setdefault(choice_of(planlib, (rows[1] - rows[0]) * nx, L, NDIR, refine, compact=1, cbytes=cb), what)
                assert ndiff(got_c, want_c) == 0 and ndiff(got_o, want_o) == 0, what
        for h in (cv, du, dv):
            h.free()


@pytest.mark.parametrize("hull", [64, 100])
def test_ragged_volume_with_its_own_ranges(own, oracle, planlib, hull):
    """A: a volume built from range images: the window is the volume's own ranges, and labels a pixel does not own read
    0 - (NDIR-1) * INF"""
    nx, ny = 26, 10
    rng = np.random.default_rng(4)
    u, v, _ = synth.stereo_pair(nx, ny, -4, 6, seed=5)
    lo_i = rng.integers(DMIN, DMIN + hull - 8, (ny, nx))
    hi_i = np.minimum(lo_i + rng.integers(0, 12, (ny, nx)), DMIN + hull - 1)
    lo_i[0, 0], hi_i[0, 0], lo_i[0, 1], hi_i[0, 1] = DMIN, DMIN + hull - 1, DMIN, DMIN + hull - 1  # the hull is the whole label range
    dminI, dmaxI = lo_i.astype(np.float32) + np.float32(0.4), hi_i.astype(np.float32) + np.float32(0.7)
    dminI[lo_i < 0] -= np.float32(0.8)  # (int) truncates towards zero on both sides
    dmaxI[hi_i < 0] -= np.float32(1.4)
    lo, hi = W.int_window(dminI, dmaxI)
    assert (lo == lo_i).all() and (hi == hi_i).all()
    cv = own.costvolume(u, v, dminI, dmaxI, "none", "ad", float("inf"), 3)
    assert cv.dims[2:] == (DMIN, DMIN + hull - 1)
    Cv = cv.download()
    for k, name in enumerate(CLASSES):
        for j, rows in enumerate(((1, 9), (2, 7))):
            NDIR, fix, refine = NDIRS[(k + j) % 5], (k + j) % 2, W.REFINEMENTS[(k + 2 * j) % 5]
            sl = slice(rows[0], rows[1])
            lr = W.LR_CLASSES[name](400 + k, NDIR, rows[1] - rows[0], nx, hull)
            S = W.sum_fix(lr, Cv[sl], NDIR, fix)
            own_lab = (np.arange(DMIN, DMIN + hull) >= lo[sl][..., None]) & (np.arange(DMIN, DMIN + hull) <= hi[sl][..., None])
            S = np.where(own_lab, S, W.vout_of(NDIR, fix)).astype(np.float32)
            want_o, want_c, Sh, hmin, wl, wh = W.windowed(S, DMIN, dminI[sl], dmaxI[sl], NDIR, fix)
            if refine:
                want_o, want_c = oracle.refine_ranged(Sh, hmin, wl, wh, refine, want_o, want_c)
            got_o, got_c = run_rows(own, cv, lr, rows[0], NDIR, fix, refine)
            what = (name, hull, rows, NDIR, fix, refine)
            REACHED.setdefault(choice_of(planlib, (rows[1] - rows[0]) * nx, hull, NDIR, refine, ragged=1), what)
            assert ndiff(got_c, want_c) == 0 and ndiff(got_o, want_o) == 0, what
    cv.free()


# ---- the development switches: read once per process, so each runs in a child of its own ------------------------------------
def words(a):
    """Bytes to digest: NaN is NaN whatever its sign and payload (as helpers.ndiff has it), every other float its own bits."""
    a = np.array(a, np.float32, copy=True)
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a).tobytes()


SWITCH_CASES = {  # switch -> the widths it changes the choice at; the pass counts and pixel counts it does so for
    "wta_packed": ((64, 128), (8, 3), 128),
    "wta_wide4": ((256, 512), (4, 3), 65),
    "wta_quad": ((192, 384), (8, 3), 128),
}
CHILD = r"""
import hashlib, sys
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import torch
import mgm_amd
import wta_crafted as W
from test_gpu_wta_crafted import run_rows, shape_of, words, DMIN
own = mgm_amd.Context(0)
for spec in sys.argv[1:]:
    name, L, n, NDIR, fix, refine = spec.split(",")
    L, n, NDIR, fix, refine = int(L), int(n), int(NDIR), int(fix), (None if refine == "None" else refine)
    ny, nx = shape_of(n)
    lr = W.LR_CLASSES[name](100, NDIR, ny, nx, L)
    cv = own.upload_volume(W.c_ints(200, ny + 2, nx, L), DMIN)
    o, c = run_rows(own, cv, lr, 1, NDIR, fix, refine)
    print("RAN", spec, hashlib.sha256(words(o) + words(c)).hexdigest())
own.close()
""" % (ROOT, os.path.join(ROOT, "tests"))


@pytest.mark.parametrize("switch", list(SWITCH_CASES))
def test_development_switch(oracle, planlib, switch):
    """A: MGM_HIP_TUNE=<switch>=0 sends the same calls to other instances; the maps stay those of the restatement"""
    widths, ndirs, n = SWITCH_CASES[switch]
    specs, want = [], {}
    for L in widths:
        for NDIR in ndirs:
            for name in ("ties", "nonfinite"):
                for refine in (None, "vfit"):
                    on, off = choice_of(planlib, n, L, NDIR, refine), choice_of(planlib, n, L, NDIR, refine, **{"sw_" + switch[4:]: 0})
                    if NDIR == ndirs[0]:
                        assert on != off, (switch, L, NDIR, on)
                    ny, nx = shape_of(n)
                    spec = "%s,%d,%d,%d,1,%s" % (name, L, n, NDIR, refine)
                    lr = W.LR_CLASSES[name](100, NDIR, ny, nx, L)
                    o, c = expectation(oracle, lr, W.c_ints(200, ny + 2, nx, L)[1:1 + ny], NDIR, 1, refine, DMIN)
                    want[spec] = hashlib.sha256(words(o) + words(c)).hexdigest()
                    specs.append(spec)
    env = dict(os.environ, MGM_HIP_TUNE=switch + "=0")
    r = subprocess.run([sys.executable, "-c", CHILD] + specs, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("RAN "))
    assert sorted(got) == sorted(want), r.stdout[-2000:]
    bad = [s for s in specs if got[s] != want[s]]
    assert not bad, bad


# ---- B: the context's own pass volumes, overwritten ----------------------------------------------------------------------------
def windows(ny, nx, dmin, L):
    """per pixel in turn: inside the volume, straddling its lower end, its upper end, wholly below, wholly above, a single label,
    empty; the bounds off by +0.4 / +0.7 or by -0.4 / -0.7 in turn ((int) truncates towards zero on both sides)"""
    i = np.arange(ny * nx)
    kind, rng = i % 7, np.random.default_rng(6)
    a = rng.integers(dmin + 1, dmin + L - 8, ny * nx)
    lo = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [a, dmin - 3, dmin + L - 4, dmin - 6, dmin + L + 1, a], a + 3)
    hi = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5], [a + 6, dmin + 3, dmin + L + 2, dmin - 2, dmin + L + 4, a], a + 1)
    up = (i // 7) % 2 == 0
    # (int) gives b for b + 0.4 / b + 0.7 when b >= 0 and for b - 0.4 / b - 0.7 when b <= 0; a bound of the other sign takes the
    # same offset from its neighbour away from zero
    flo = np.where(up, np.where(lo >= 0, lo + 0.4, lo - 1 + 0.4), np.where(lo <= 0, lo - 0.4, lo + 1 - 0.4))
    fhi = np.where(up, np.where(hi >= 0, hi + 0.7, hi - 1 + 0.7), np.where(hi <= 0, hi - 0.7, hi + 1 - 0.7))
    flo, fhi = flo.astype(np.float32).reshape(ny, nx), fhi.astype(np.float32).reshape(ny, nx)
    wl, wh = W.int_window(flo, fhi)
    assert (wl.ravel() == lo).all() and (wh.ravel() == hi).all() and (flo != np.trunc(flo)).all()
    return flo, fhi


def overwrite(own, lr):
    NDIR, ny, nx, L = lr.shape
    for p in range(NDIR):
        ptr = own.lr_device_ptr(p)
        assert ptr, "mgm_lr_device_ptr(%d) is null" % p
        mdist.device_view(ptr, (ny, nx, L)).copy_(torch.from_numpy(np.ascontiguousarray(lr[p])).cuda())
    torch.cuda.synchronize()


@pytest.mark.parametrize("NDIR", [8, 4])
@pytest.mark.parametrize("L", [64, 192, 256, 512])
def test_windowed_and_right_search_on_overwritten_volumes(own, oracle, L, NDIR):
    nx, ny, dmin = 23, 7, -(L // 2)
    Cv = synth.raw_volume(nx, ny, L, seed=9, inf_frac=0.02)  # non-negative costs, P 8 / 32, no weights: inside every premise
    cv = own.upload_volume(Cv, dmin)
    flo, fhi = windows(ny, nx, dmin, L)
    dlo, dhi = own.upload_image(flo), own.upload_image(fhi)
    own.timing_reset()
    try:
        for k, name in enumerate(CLASSES):
            own.timing(k == 0)  # (the first class runs with the timing table on: it names the kernels that ran)
            _, o, c = own.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
            own.synchronize()
            o.free(), c.free()
            lr = W.LR_CLASSES[name](500 + k, NDIR, ny, nx, L)
            overwrite(own, lr)
            for fix in (0, 1):
                S = W.sum_fix(lr, Cv, NDIR, fix)
                wo, wc, Sh, hmin, wl, wh = W.windowed(S, dmin, flo, fhi, NDIR, fix)
                for refine in W.REFINEMENTS:
                    want_o, want_c = oracle.refine_ranged(Sh, hmin, wl, wh, refine, wo, wc) if refine else (wo, wc)
                    o, c = own.wta_windowed_dev(cv, NDIR, fix, refine, dlo, dhi)
                    got_o, got_c = o.download()[0], c.download()[0]
                    o.free(), c.free()
                    assert ndiff(got_c, want_c) == 0 and ndiff(got_o, want_o) == 0, ("windowed", name, L, NDIR, fix, refine)
                for vnx in (nx, nx - 6, nx + 9):
                    for refine in ((None, "vfit") if (k + vnx) % 2 else ("vfit", None)):
                        want_o, want_c = wta_right(S, dmin, vnx, refine)
                        for walk in ("0", "1"):
                            os.environ["MGM_HIP_WTA_RIGHT_ANY"] = walk
                            o, c = own.wta_right_dev(cv, NDIR, fix, refine, vnx)
                            got_o, got_c = o.download()[0], c.download()[0]
                            o.free(), c.free()
                            assert ndiff(got_c, want_c) == 0 and ndiff(got_o, want_o) == 0, ("right", name, L, NDIR, fix, refine, vnx, walk)
        ran = {n for n, _ in own.timings()}
        assert {"k_wta", "k_refine", "k_wta_right"} <= ran, ran
    finally:
        own.timing(False)
        os.environ.pop("MGM_HIP_WTA_RIGHT_ANY", None)
        own.trim()  # nothing later reads the overwritten volumes
        for h in (cv, dlo, dhi):
            h.free()


@pytest.mark.parametrize("NDIR", [8, 4])
@pytest.mark.parametrize("L,nx,ny", [(128, 23, 7), (384, 23, 7), (768, 23, 7), (1024, 23, 7), (64, 150, 2), (128, 140, 2)])
def test_right_search_on_the_other_instances_and_on_split_rows(own, planlib, L, nx, ny, NDIR):
    """B: k_wta_right at 2, 6, 12 and 16 labels per lane (the test above runs 1, 3, 4 and 8), and rows wider than the
    max(64, L) right pixels of a segment (plan_wta_right): crafted values cross a segment boundary and wrap the LDS ring"""
    dmin, split = -(L // 2), nx > 23
    Cv = synth.raw_volume(nx, ny, L, seed=9, inf_frac=0.02)
    cv = own.upload_volume(Cv, dmin)
    vnxs = (nx, nx - 9, nx + 9)
    for vnx in vnxs:
        ch = dict(zip(PM.RIGHT_OUT, TP.ask(planlib, "right", [TP.right_request(L=L, nx=nx, ny=ny, vnx=vnx, dmin=dmin)])[0]))
        assert (ch["family"], ch["LPL"]) == (PM.RIGHT_STREAM, L // 64), ch
        segments = -(-vnx // ch["seg"])
        assert (segments > 1) == split, (vnx, ch)
    own.timing_reset()
    try:
        for k, name in enumerate(("ties", "edges", "nonfinite", "nolabel")):
            own.timing(k == 0)
            _, o, c = own.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
            own.synchronize()
            o.free(), c.free()
            lr = W.LR_CLASSES[name](600 + k, NDIR, ny, nx, L)
            overwrite(own, lr)
            for fix in (0, 1):
                S = W.sum_fix(lr, Cv, NDIR, fix)
                for vnx in vnxs:
                    for refine in (None, "vfit"):
                        want_o, want_c = wta_right(S, dmin, vnx, refine)
                        for walk in ("0", "1"):
                            os.environ["MGM_HIP_WTA_RIGHT_ANY"] = walk
                            o, c = own.wta_right_dev(cv, NDIR, fix, refine, vnx)
                            got_o, got_c = o.download()[0], c.download()[0]
                            o.free(), c.free()
                            assert ndiff(got_c, want_c) == 0 and ndiff(got_o, want_o) == 0, ("right", name, L, nx, NDIR, fix, refine, vnx, walk)
        assert "k_wta_right" in {n for n, _ in own.timings()}
    finally:
        own.timing(False)
        os.environ.pop("MGM_HIP_WTA_RIGHT_ANY", None)
        own.trim()  # nothing later reads the overwritten volumes
        cv.free()


# ---- C: the stand-alone refinement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLASSES)
def test_refine_alone_on_labels_the_test_chooses(own, oracle, name):
    for L, (ny, nx) in ((12, (7, 19)), (256, (12, 47))):
        S = W.LR_CLASSES[name](31, 1, ny, nx, L)[0]
        lab = W.refine_labels(32, ny, nx, DMIN, L)
        cost = np.random.default_rng(33).uniform(-3, 3, (ny, nx)).astype(np.float32)
        nan = np.isnan(lab)
        vol = own.upload_volume(S, DMIN)
        for m in W.REFINEMENTS[1:]:
            want_o, want_c = oracle.refine(S, DMIN, m, lab, cost)
            got_o, got_c = own.refine(vol, m, lab, cost)
            assert ndiff(got_o, want_o) == 0 and ndiff(got_c, want_c) == 0, (name, L, m)
            assert np.isnan(got_o[nan]).all() and ndiff(got_c[nan], cost[nan]) == 0, "a NaN label: the pixel stays as it is"
        vol.free()


def test_every_declared_choice_was_reached():
    """(the last test of the file: the cases above asked plan_wta which instance each call runs on)"""
    for ch in sorted(REACHED):
        print(PM.instance("wta", ch + (0,)), "<-", REACHED[ch])
    missing = [PM.instance("wta", ch + (0,)) for ch in DECLARED if ch not in REACHED]
    assert not missing, missing
