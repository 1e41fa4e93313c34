"""The runner-up search (k_wta_runnerup<LPL, PPW, MAXD> in its 14 instances and k_wta_runnerup_any) on CRAFTED Lr
volumes: the classes of tests/runnerup_crafted.py -- winners whose exclusion zone ends on a lane boundary, clips at label 0 or
L-1, holds every finite label, has two equal candidates beside it -- and those of tests/wta_crafted.py (ties, pass-order-dependent
sums, overflow, NaN / +-INF, denormals, signed zeros, flat pixels, pixels without a label).

No such value goes through a pass kernel: a tame volume (one of the C classes; P 8 / 32, TSGM 3, no weights) is aggregated, every
pass volume of the context is fetched with the test aid mgm_debug_lr_device_ptr and overwritten in place (padding slots of a
padded label stride included), and mgm_wta_runnerup_dev searches exactly those.  All four maps are compared bit for bit
(NaN = NaN) with runnerup_model.runnerup() on wta_crafted.sum_fix() of the crafted passes -- the model is fed the Lr volumes,
not a downloaded S.  tests/test_runnerup_crafted_ref.py pins the model on a scalar restatement and shows that these inputs tell
it from eight subtly wrong searches.  The context is the file's own: an overwritten volume never sits in the shared one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import mgm_amd
import runnerup_crafted as R
import test_runnerup_plan as RP
import wta_crafted as W
from mgm_amd import dist as mdist
from mgm_amd import synth
from runnerup_model import runnerup
from test_gpu_wta_runnerup import NAMES, same, search

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_L = (64, 128, 192, 256, 384, 512, 768, 1024)
WIDE4_L = STREAM_L[:6]  # the widths with an instance of at most 4 passes (twice the pixels per wave)
OLD = list(W.LR_CLASSES)
REACHED = {}  # instance -> a case that reached it
PADDING_SEEN = set()  # {"padded", "unpadded"}: what the runs of odd widths did
PAD_FILL = np.float32(-1e30)


@pytest.fixture(scope="module")
def own():
    try:
        c = mgm_amd.Context(0)
    except mgm_amd.MgmError as e:
        if e.code == mgm_amd.MGM_ERR_HIP:
            pytest.skip("no MI355X in this box (mgm_ctx_create: MGM_ERR_HIP)")
        raise
    yield c
    c.trim()  # nothing later reads the overwritten volumes
    c.close()


@pytest.fixture(scope="module")
def rlib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("runnerupcrafted") / "librunnerup_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", RP.CSRC, os.path.join(ROOT, "tests", "runnerup_plan_harness.cc"), "-o", so], check=True)
    return C.CDLL(so)


def radii(L):
    return (0, 1, 2, 5, L)


def shape_of(n):
    return {65: (5, 13), 130: (10, 13)}.get(n, (1, n))


def plan(rlib, npix, L, Lk, NDIR, force=0, wg=0):
    return RP.ask(rlib, [RP.request(npix=npix, L=L, Lk=Lk, NDIR=NDIR, sw_any=force, sw_wg_per_cu=wg)])[0]


def counts_of(rlib, L, NDIR):
    """1 pixel, one short of a wave's group, one group, one over, one workgroup and a pixel, and 130 (65 from 384 labels on)"""
    ppw = plan(rlib, 1000, L, L, NDIR)["PPW"]
    return sorted({n for n in (1, ppw - 1, ppw, ppw + 1, 4 * ppw + 1, 130 if L < 384 else 65) if n >= 1})


def c_class(NDIR, j):
    """`ints` and `frac` in turn; `inf1` (0 * INF = NaN under the fix) on every other case of one pass"""
    return "inf1" if (NDIR == 1 and j % 2 == 1) else ("ints", "frac")[(j // 2) % 2]


def aggregate(own, Cvs, dmin, NDIR, passes_only=False):
    """upload and aggregate the tame volumes Cvs in one launch; returns their handles.  passes_only: mgm_aggregate_passes_dev,
    which never pads the label stride."""
    cvs = [own.upload_volume(Cv, dmin) for Cv in Cvs]
    if passes_only:
        assert len(cvs) == 1
        own.aggregate_passes_dev(cvs[0], 8.0, 32.0, 3, 0, 0, NDIR)
    elif len(cvs) == 1:
        _, o, c = own.aggregate_dev(cvs[0], 8.0, 32.0, NDIR, 3, 0, 1, None, None)
        o.free(), c.free()
    else:
        _, outs, costs = own.aggregate_batch_dev(cvs, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
        for h in outs + costs:
            h.free()
    own.synchronize()
    return cvs


def stride_of(own, volume=0):
    got = own.debug_lr_ptr(volume, 0)
    assert got, "mgm_debug_lr_device_ptr(%d, 0) is null" % volume
    return got[1]


def overwrite(own, lr, volume=0, pad=PAD_FILL):
    """the crafted passes lr [n][ny][nx][L] over passes 0..n-1 of `volume` as the aid hands them out; the padding slots L..Lk-1
    of a padded stride take `pad`.  Returns Lk."""
    n, ny, nx, L = lr.shape
    Lk = None
    for p in range(n):
        got = own.debug_lr_ptr(volume, p)
        assert got, "mgm_debug_lr_device_ptr(%d, %d) is null" % (volume, p)
        ptr, Lk, stride = got
        assert Lk >= L and stride >= ny * nx * Lk
        full = np.full((ny, nx, Lk), pad, np.float32)
        full[:, :, :L] = lr[p]
        mdist.device_view(ptr, (ny, nx, Lk)).copy_(torch.from_numpy(full).cuda())
    torch.cuda.synchronize()
    return Lk


def check(own, rlib, cv, lr, Cv, dmin, NDIR, Lk, rs, fixes, what, force=0, wg=0, want_first=True):
    """search at every radius of rs and every fix of fixes; all maps against the model on the crafted passes.  The first search
    runs with the timing table on: it names the family the planner chose."""
    _, ny, nx, L = lr.shape
    ch = plan(rlib, ny * nx, L, Lk, NDIR, force, wg)
    inst = RP.instance(ch)
    assert inst is not None, what
    first = True
    for fix in fixes:
        S = W.sum_fix(lr, Cv, NDIR, fix)
        for r in rs:
            if first:
                own.timing(True)
                own.timing_reset()
            got = search(own, cv, NDIR, fix, r, want_first=want_first)
            if first:
                names = {n for n, _ in own.timings()}
                own.timing(False)
                fam = "k_wta_runnerup_any" if inst == "k_wta_runnerup_any" else "k_wta_runnerup_stream"
                assert "k_wta_runnerup" in names and {n for n in names if n.startswith("k_wta_runnerup_")} == {fam}, (what, inst, names)
                first = False
            want = runnerup(S, dmin, r)
            for name, g, w in zip(NAMES, got, want):
                if g is None:
                    assert not want_first and name in ("out1", "cost1")
                    continue
                assert same(g, w), "%s on %s: radius %d fix %d %s: %d of %d differ" % (what, inst, r, fix, name, int(np.sum(~((g == w) | (np.isnan(g) & np.isnan(w))))), w.size)
    REACHED.setdefault(inst, what)
    return inst


def crafted_round(own, rlib, cv, Cv, dmin, NDIR, ny, nx, L, j, force=0, pad=PAD_FILL, olds=None):
    """on the volume just aggregated: the three classes of runnerup_crafted at radius radii(L)[j % 5] (searched at that radius,
    fix off and on), then class k % 10 of wta_crafted for every k of olds (default: j) at every radius (fix k % 2) and at radius
    1 with the other fix"""
    r = radii(L)[j % 5]
    Lk = stride_of(own)
    LPL = 1 if force else R.lpl_of(Lk)
    for name, fn in R.classes(r, LPL).items():
        lr = fn(1000 + j, NDIR, ny, nx, L)
        overwrite(own, lr, pad=pad)
        check(own, rlib, cv, lr, Cv, dmin, NDIR, Lk, (r,), (0, 1), (name, L, Lk, ny, nx, NDIR, r), force)
    for k in olds or (j,):
        name = OLD[k % len(OLD)]
        lr = W.LR_CLASSES[name](2000 + k, NDIR, ny, nx, L)
        overwrite(own, lr, pad=pad)
        inst = check(own, rlib, cv, lr, Cv, dmin, NDIR, Lk, radii(L), (k % 2,), (name, L, Lk, ny, nx, NDIR), force)
        check(own, rlib, cv, lr, Cv, dmin, NDIR, Lk, (1,), (1 - k % 2,), (name, L, Lk, ny, nx, NDIR), force)
    return inst, Lk


# ---- the aid itself ----------------------------------------------------------------------------------------------------------
def test_the_aid_serves_the_last_dense_run_and_nothing_else(own):
    nx, ny, L, dmin, NDIR = 13, 5, 64, -20, 4
    own.trim()
    assert own.debug_lr_ptr(0, 0) is None  # (trimmed: no run)
    Cs = [synth.raw_volume(nx, ny, L, seed=s, inf_frac=0.02) for s in (1, 2)]
    cvs = aggregate(own, Cs[:1], dmin, NDIR)
    got = [own.debug_lr_ptr(0, p) for p in range(NDIR)]
    assert all(got) and all(g[1] == L and g[2] == got[0][2] >= nx * ny * L for g in got)
    assert [g[0] for g in got] == [own.lr_device_ptr(p) for p in range(NDIR)]  # an unpadded run, volume 0: mgm_lr_device_ptr's
    assert [g[0] - got[0][0] for g in got] == [4 * p * got[0][2] for p in range(NDIR)]
    for volume, p in ((0, NDIR), (0, -1), (1, 0), (-1, 0), (0, 8)):
        assert own.debug_lr_ptr(volume, p) is None, (volume, p)
    # it launches nothing and changes no record: the same search gives the same maps before and after, and the pointers stay
    before = search(own, cvs[0], NDIR, 1, 1)
    assert [own.debug_lr_ptr(0, p) for p in range(NDIR)] == got
    after = search(own, cvs[0], NDIR, 1, 1)
    assert all(same(a, b) for a, b in zip(before, after)) and np.isfinite(before[1]).any()
    cvs[0].free()
    # a batch of two: both volumes, slot 1 behind slot 0's passes
    cvs = aggregate(own, Cs, dmin, NDIR)
    a, b = own.debug_lr_ptr(0, 0), own.debug_lr_ptr(1, 0)
    assert a and b and b[0] - a[0] == 4 * NDIR * a[2] and own.debug_lr_ptr(2, 0) is None and own.debug_lr_ptr(1, NDIR) is None
    # a padded stride: mgm_lr_device_ptr refuses, the aid names the stride
    for h in cvs:
        h.free()
    cvs = aggregate(own, [synth.raw_volume(nx, ny, 100, seed=3, inf_frac=0.02)], dmin, NDIR)
    got = own.debug_lr_ptr(0, 0)
    assert got and got[1] in (100, 128)
    assert (own.lr_device_ptr(0) is None or own.lr_device_ptr(0) == 0) == (got[1] == 128)
    cvs[0].free()
    own.trim()
    assert own.debug_lr_ptr(0, 0) is None


# ---- every instance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", STREAM_L)
def test_every_class_on_every_instance(own, rlib, L):
    """both instances of a width (at most 4 passes: twice the pixels per wave; up to 8) at 1 pixel, one short of a wave's group,
    one group, one over, one workgroup and a pixel, and 65 / 130 pixels; the classes, the radii, the fix and the costs in turn"""
    j, met, seen = 0, set(), set()
    for NDIR in ((1, 3, 4, 5, 8) if L <= 512 else (4, 8)):
        for n in counts_of(rlib, L, NDIR):
            ny, nx = shape_of(n)
            dmin = (-5, 3, -(L // 2))[j % 3]
            Cv = W.C_CLASSES[c_class(NDIR, j)](200 + j, ny, nx, L)
            cv, = aggregate(own, [Cv], dmin, NDIR)
            olds = (j,) if L <= 512 else (j, j + 8)  # (two instances fewer, eight cases: two classes of wta_crafted each)
            inst, Lk = crafted_round(own, rlib, cv, Cv, dmin, NDIR, ny, nx, L, j, olds=olds)
            assert Lk == L and inst.startswith("k_wta_runnerup<%d," % (L // 64)), (inst, Lk)
            seen.add(inst)
            met |= {OLD[k % len(OLD)] for k in olds}
            cv.free()
            j += 1
    assert met == set(OLD) and j >= 5, "every class of wta_crafted at this width, every radius for the classes of runnerup_crafted"
    assert len(seen) == (2 if L <= 512 else 1), seen


@pytest.mark.parametrize("NDIR", [1, 3])
@pytest.mark.parametrize("L", WIDE4_L)
def test_pass_guard(own, rlib, L, NDIR):
    """the instances of at most 4 passes read `p < NDIR` passes and no more: the volumes of a batch lie behind one another at the
    pass stride, so what a read of pass NDIR.. of slot 0 would meet are the passes of slots 1.. -- filled with a finite -1e30.
    The expectation sums the NDIR passes of slot 0 alone."""
    nb = -(-8 // NDIR)
    ppw = plan(rlib, 1000, L, L, NDIR)["PPW"]
    ny, nx = shape_of(4 * ppw + 1)
    dmin = -7
    Cvs = [W.c_ints(300 + v, ny, nx, L) for v in range(nb)]
    cvs = aggregate(own, Cvs, dmin, NDIR)
    base = own.debug_lr_ptr(0, 0)
    for v in range(1, nb):
        for p in range(NDIR):  # (slot v's pass p is "pass v * NDIR + p" of slot 0)
            got = own.debug_lr_ptr(v, p)
            assert got and got[0] - base[0] == 4 * (v * NDIR + p) * base[2], (v, p)
        overwrite(own, np.full((NDIR, ny, nx, L), PAD_FILL, np.float32), volume=v)
    Lk = stride_of(own)
    for k, (r, name) in enumerate(((1, "zone"), (2, "two_sided"), (0, "ties"), (5, "nonfinite"))):
        lr = R.all_classes(r, R.lpl_of(Lk))[name](3000 + k, NDIR, ny, nx, L)
        assert R.pass_guard(lr).shape[0] == 8 and (R.pass_guard(lr)[NDIR:] == PAD_FILL).all()  # (what the slots behind hold)
        overwrite(own, lr)
        inst = check(own, rlib, cvs[0], lr, Cvs[0], dmin, NDIR, Lk, (r,), (0, 1), ("pass_guard", name, L, NDIR))
        assert inst.endswith(",4>"), inst
    for h in cvs:
        h.free()


# ---- padded strides ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [63, 100, 151, 300])
def test_padding_slots_are_never_candidates(own, rlib, L):
    """an odd width whose run padded the label stride (Lk read from the aid): slots L..Lk-1 of every pass hold a finite -1e30,
    then NaN -- neither is ever a candidate.  The same width through mgm_aggregate_passes_dev, which never pads, lands on the
    generic kernel."""
    for j, (NDIR, n) in enumerate(((8, 130), (4, 37), (3, 9))):
        ny, nx = shape_of(n)
        dmin = -(L // 2)
        Cv = W.C_CLASSES[("ints", "frac")[j % 2]](400 + j, ny, nx, L)
        for passes_only in (False, True):
            cv, = aggregate(own, [Cv], dmin, NDIR, passes_only=passes_only)
            for rnd, pad in enumerate((PAD_FILL, np.float32(np.nan))):
                inst, Lk = crafted_round(own, rlib, cv, Cv, dmin, NDIR, ny, nx, L, 5 * j + rnd + L, pad=pad)
                if Lk > L:
                    assert not passes_only and Lk % 64 == 0 and inst.startswith("k_wta_runnerup<%d," % (Lk // 64)), (inst, Lk)
                    PADDING_SEEN.add("padded")
                else:
                    assert inst == "k_wta_runnerup_any", (inst, Lk)
                    PADDING_SEEN.add("unpadded")
                if Lk == L:
                    break  # (no padding slot to fill another way)
            cv.free()


# ---- the generic kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3, 4, 37, 64, 300, 1100])
def test_the_generic_kernel(own, rlib, L, monkeypatch):
    """MGM_HIP_WTA_RUNNERUP_ANY=1: every class on the kernel that strides the labels over the lanes, L <= 2 * radius + 1 included"""
    monkeypatch.setenv("MGM_HIP_WTA_RUNNERUP_ANY", "1")
    j = 0
    for NDIR, n in ((8, 65), (4, 130), (1, 9), (5, 1), (3, 65)):
        ny, nx = shape_of(n if L <= 300 else min(n, 65))
        dmin = (-5, 3, -(L // 2))[j % 3]
        Cv = W.C_CLASSES[c_class(NDIR, j)](500 + j, ny, nx, L)
        cv, = aggregate(own, [Cv], dmin, NDIR)
        for k in range(2):
            inst, _ = crafted_round(own, rlib, cv, Cv, dmin, NDIR, ny, nx, L, 2 * j + k, force=1)
            assert inst == "k_wta_runnerup_any"
        cv.free()
        j += 1
    assert 2 * j >= len(OLD)


# ---- several turns of the grid-stride loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,nx,ny,NDIR", [(256, 130, 40, 8), (64, 257, 45, 4)])
def test_several_turns(own, rlib, L, nx, ny, NDIR, monkeypatch):
    """MGM_HIP_WTA_RUNNERUP_WG=1: one workgroup per CU, fewer waves than groups of pixels (tests/test_runnerup_plan.py holds the
    planner to that on any device up to 304 CUs)"""
    monkeypatch.setenv("MGM_HIP_WTA_RUNNERUP_WG", "1")
    dmin, r = -(L // 2), 2
    Cv = W.c_ints(600, ny, nx, L)
    cv, = aggregate(own, [Cv], dmin, NDIR)
    Lk = stride_of(own)
    for cu in (1, 256, 304):
        g = RP.ask(rlib, [RP.request(npix=nx * ny, L=L, Lk=Lk, NDIR=NDIR, num_cu=cu, sw_wg_per_cu=1)])[0]
        assert nx * ny > g["grid"] * 4 * g["PPW"], g
    lr = R.lr_zone(601, NDIR, ny, nx, L, r, R.lpl_of(Lk))
    overwrite(own, lr)
    check(own, rlib, cv, lr, Cv, dmin, NDIR, Lk, (r,), (0, 1), ("turns", L, nx, ny, NDIR), wg=1)
    cv.free()


# ---- a batch, only the runner-up, compact costs --------------------------------------------------------------------------------
def test_slot_1_of_a_batch_of_two(own, rlib):
    nx, ny, L, dmin, NDIR, r = 13, 10, 128, -100, 8, 1
    Cvs = [W.c_ints(700 + v, ny, nx, L) for v in range(2)]
    cvs = aggregate(own, Cvs, dmin, NDIR)
    Lk = stride_of(own, 1)
    lrs = [R.lr_zone(710, NDIR, ny, nx, L, r, R.lpl_of(Lk)), R.lr_two_sided(711, NDIR, ny, nx, L, r, R.lpl_of(Lk))]
    for v in (0, 1):
        overwrite(own, lrs[v], volume=v)
    for v in (1, 0):
        check(own, rlib, cvs[v], lrs[v], Cvs[v], dmin, NDIR, Lk, (r, 0), (1, 0), ("slot %d" % v,))
    lrs = [W.lr_nonfinite(712, NDIR, ny, nx, L), W.lr_ties(713, NDIR, ny, nx, L)]
    for v in (0, 1):
        overwrite(own, lrs[v], volume=v)
    for v in (1, 0):
        check(own, rlib, cvs[v], lrs[v], Cvs[v], dmin, NDIR, Lk, (r, 5), (1, 0), ("slot %d" % v,))
    for h in cvs:
        h.free()


@pytest.mark.parametrize("L,NDIR", [(64, 4), (256, 8), (100, 8)])
def test_only_the_runner_up(own, rlib, L, NDIR):
    """out1 / cost1 NULL on `only_zone` (no runner-up anywhere) and `two_sided`: the same two maps"""
    nx, ny, dmin = 13, 10, -30
    Cv = W.c_frac(800, ny, nx, L)
    cv, = aggregate(own, [Cv], dmin, NDIR)
    Lk = stride_of(own)
    for r in (0, 2):
        for name in ("only_zone", "two_sided"):
            lr = R.classes(r, R.lpl_of(Lk))[name](810 + r, NDIR, ny, nx, L)
            overwrite(own, lr)
            check(own, rlib, cv, lr, Cv, dmin, NDIR, Lk, (r,), (0, 1), (name, "runner-up only", L), want_first=False)
    cv.free()


@pytest.mark.parametrize("L", [64, 192, 256])
def test_compact_cost_codes(own, rlib, L):
    """one byte per cost (single-word census) and two (absolute differences of a colour pair), built on the device and read
    under the over-count fix; the expectation reads the volume back"""
    nx, ny, dmin, NDIR = 26, 5, -(L - 8), 8
    for dist_, nch in (("census", 1), ("ad", 3)):
        u, v, _ = synth.stereo_pair(nx, ny, -4, 6, seed=3, nch=nch)
        du, dv = own.upload_image(u), own.upload_image(v)
        cv = own.costvolume_dev(du, dv, dmin, dmin + L - 1, "none", dist_, float("inf"), 5)
        Cv = cv.download()
        assert np.isfinite(Cv).any() and (dist_ == "census" or Cv[np.isfinite(Cv)].max() > 255)
        _, o, c = own.aggregate_dev(cv, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
        own.synchronize()
        Lk = stride_of(own)
        for r in (1, 5):
            for name in ("zone", "nonfinite"):
                lr = R.all_classes(r, R.lpl_of(Lk))[name](900 + r, NDIR, ny, nx, L)
                overwrite(own, lr)
                check(own, rlib, cv, lr, Cv, dmin, NDIR, Lk, (r,), (1,), (name, dist_, L))
        for h in (o, c, cv, du, dv):
            h.free()


def test_every_instance_was_reached(own):
    """(the last test of the file: every case above asked plan_wta_runnerup which instance its call runs on, and the timing
    table named the family the plan said)"""
    for inst in sorted(REACHED):
        print(inst, "<-", REACHED[inst])
    table = RP.launch_table()
    assert len(table) == 15 and set(REACHED) == table, sorted(set(REACHED) ^ table)
    assert PADDING_SEEN == {"padded", "unpadded"}, PADDING_SEEN
    own.trim()
