"""The consensus votes (k_wta_consensus<LPL, PPW, MAXD> in its 14 instances, k_wta_consensus_any, k_wta_consensus_rel<4 / 8>; DESIGN.md
7h) on CRAFTED Lr volumes: the classes of tests/consensus_crafted.py -- per-pass winners on label 0, label L-1 and both sides of a
lane boundary, spread over both edges of every tolerance zone, ties inside a lane, across lanes and half the range apart -- and
those of tests/wta_crafted.py, each pass taken alone (NaN, +-INF, -0 / +0, negative, denormal and overflowing values, flat pixels,
passes without a finite entry), with poison in the padding slots and on the labels a pixel does not own.

No such value goes through a pass kernel: a tame volume is aggregated, every pass volume of the context is fetched with the test
aids mgm_debug_lr_device_ptr / mgm_debug_rel_lr_device_ptr and overwritten in place, and mgm_wta_consensus_dev reads exactly
those.  Votes and winners are compared bit for bit (NaN = NaN) with consensus_model.consensus() on the crafted passes;
tests/test_consensus_model.py pins the model on a scalar restatement and shows that these inputs tell it from nine subtly wrong
searches.  Every case asks plan_wta_consensus which instance its call runs on, and the timing table names the family the plan
said.  The context is the file's own and is trimmed after use: an overwritten volume never sits in the shared one."""
import os

import numpy as np
import pytest
import torch

import consensus_crafted as K
import mgm_amd
import runnerup_crafted as RC
import test_consensus_plan as CP
import wta_crafted as W
import wta_rel_crafted as R
from consensus_model import consensus
from helpers import ndiff
from mgm_amd import dist as mdist
from test_gpu_wta_rel_crafted import Prepared

pytestmark = pytest.mark.gpu

STREAM_L = (64, 128, 192, 256, 384, 512, 768, 1024)
REACHED = {}  # instance -> a case that reached it
MET = set()   # the classes that ran
POISONS = (np.float32(-1e30), np.float32(np.nan), np.float32(-np.inf), np.float32(0.0))


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
def plib(tmp_path_factory):
    return CP.build(str(tmp_path_factory.mktemp("consensuscrafted")))


def same(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and ndiff(got, want) == 0 and np.array_equal(np.isnan(got), np.isnan(want))


def shape_of(n):
    return {65: (5, 13), 130: (10, 13)}.get(n, (1, n))


def aggregate(own, Cv, dmin, NDIR, passes_only=False, batch=1):
    """upload and aggregate `batch` copies of the tame volume Cv in one launch; returns their handles.  passes_only:
    mgm_aggregate_passes_dev, which never pads the label stride."""
    cvs = [own.upload_volume(Cv, dmin) for _ in range(batch)]
    if passes_only:
        own.aggregate_passes_dev(cvs[0], 8.0, 32.0, 3, 0, 0, NDIR)
    elif batch == 1:
        _, o, c = own.aggregate_dev(cvs[0], 8.0, 32.0, NDIR, 3, 0, 1, None, None)
        o.free(), c.free()
    else:
        _, outs, costs = own.aggregate_batch_dev(cvs, 8.0, 32.0, NDIR, 3, 0, 1, None, None)
        for h in outs + costs:
            h.free()
    own.synchronize()
    return cvs


def overwrite(own, lr, volume=0, pad=POISONS[0], lo=None, hi=None):
    """the crafted passes lr [n][ny][nx][L] over passes 0..n-1 of `volume` as the aid hands them out; the padding slots L..Lk-1 of a
    padded stride, and the labels outside [lo, hi] (label indices) of a ragged hull, take `pad`.  Returns Lk."""
    n, ny, nx, L = lr.shape
    Lk = None
    for p in range(n):
        got = own.debug_lr_ptr(volume, p)
        assert got, "mgm_debug_lr_device_ptr(%d, %d) is null" % (volume, p)
        ptr, Lk, stride = got
        assert Lk >= L and stride >= ny * nx * Lk
        full = K.full(lr[p:p + 1], Lk, lo, hi, poison=pad, guard=False)[0]
        mdist.device_view(ptr, (ny, nx, Lk)).copy_(torch.from_numpy(np.ascontiguousarray(full)).cuda())
    torch.cuda.synchronize()
    return Lk


def votes_of(own, cv, NDIR, d, tol):
    dd = own.upload_image(d)
    v, w = own.wta_consensus_dev(cv, NDIR, dd, tol, want_winners=True)
    res = v.download()[0], w.download()
    for h in (dd, v, w):
        h.free()
    return res


def check(own, plib, cv, lr, dmin, NDIR, Lk, base, what, lo=None, hi=None, force=0, wg=0, slots=0, tols=K.TOLS):
    """both maps of consensus_crafted.d_maps at the tolerances `tols` against the model on the crafted passes; the first call
    runs with the timing table on: it names the family the planner chose"""
    _, ny, nx, L = lr.shape
    ch = CP.ask(plib, [CP.request(npix=ny * nx, L=slots or L, Lk=slots or Lk, NDIR=NDIR, slots=slots, sw_any=force, sw_wg_per_cu=wg, hull=int(lo is not None and not slots))])[0]
    inst = CP.instance(ch)
    assert inst is not None, what
    _, win = consensus(lr, dmin, NDIR, None, 0.0, lo, hi)
    first = True
    for dname, d in K.d_maps(win[0], base, dmin).items():
        for tol in tols:
            if first:
                own.timing(True)
                own.timing_reset()
            gv, gw = votes_of(own, cv, NDIR, d, tol)
            if first:
                names = {n for n, _ in own.timings()}
                own.timing(False)
                assert "k_wta_consensus" in names and {n for n in names if n.startswith("k_wta_consensus_")} == {CP.family_name(ch)}, (what, inst, names)
                first = False
            wv, ww = consensus(lr, dmin, NDIR, d, tol, lo, hi)
            assert same(gv, wv), "%s on %s: %s tol %g votes: %d of %d differ" % (what, inst, dname, tol, ndiff(gv, wv), wv.size)
            assert same(gw, ww), "%s on %s: %s tol %g winners: %d of %d differ" % (what, inst, dname, tol, ndiff(gw, ww), ww.size)
    REACHED.setdefault(inst, what)
    return inst


def crafted_round(own, plib, cv, dmin, NDIR, ny, nx, L, j, force=0, pad=POISONS[0], nold=2):
    """on the volume just aggregated: `votes` at every tolerance, then `nold` classes of wta_crafted in turn at two tolerances"""
    Lk = own.debug_lr_ptr(0, 0)[1]
    LPL = 1 if force else RC.lpl_of(Lk)
    base = K.base_labels(ny, nx, L, LPL)
    lr = K.lr_votes(1000 + j, NDIR, ny, nx, L, LPL)
    overwrite(own, lr, pad=pad)
    inst = check(own, plib, cv, lr, dmin, NDIR, Lk, base, ("votes", L, Lk, ny, nx, NDIR), force=force)
    MET.add("votes")
    olds = list(W.LR_CLASSES)
    for k in range(nold):
        name = olds[(nold * j + k) % len(olds)]
        lr = W.LR_CLASSES[name](2000 + j + k, NDIR, ny, nx, L)
        overwrite(own, lr, pad=POISONS[(j + k) % 4])
        check(own, plib, cv, lr, dmin, NDIR, Lk, base, (name, L, Lk, ny, nx, NDIR), force=force, tols=(K.TOLS[(j + k) % 4], 1.0))
        MET.add(name)
    return inst, Lk


# ---- every streaming instance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", STREAM_L)
def test_every_streaming_instance(own, plib, L):
    """both instances of a width (at most 4 passes: twice the pixels per wave; up to 8) at one workgroup and a pixel, 4 * PPW + 1,
    and at 65 / 130 pixels"""
    j, seen = L // 64, set()
    for NDIR in ((3, 4, 8) if L <= 512 else (4, 8)):
        ppw = CP.ask(plib, [CP.request(npix=1000, L=L, NDIR=NDIR)])[0]["PPW"]
        for n in sorted({4 * ppw + 1, 130 if L < 384 else 65}):
            ny, nx = shape_of(n)
            dmin = (-5, 3, -(L // 2))[j % 3]
            cv, = aggregate(own, W.c_ints(200 + j, ny, nx, L), dmin, NDIR)
            inst, Lk = crafted_round(own, plib, cv, dmin, NDIR, ny, nx, L, j)
            assert Lk == L and inst.startswith("k_wta_consensus<%d," % (L // 64)), (inst, Lk)
            seen.add(inst)
            cv.free()
            j += 1
    assert len(seen) == (2 if L <= 512 else 1), seen


@pytest.mark.parametrize("L,NDIR", [(64, 3), (256, 1), (512, 3)])
def test_pass_guard(own, plib, L, NDIR):
    """the instances of at most 4 passes read `p < NDIR` passes and no more: the volumes of a batch lie behind one another at the pass
    stride, so what a read of pass NDIR.. of slot 0 would meet are the passes of slots 1.. -- filled with a finite -1e30"""
    nb = -(-8 // NDIR)
    ppw = CP.ask(plib, [CP.request(npix=1000, L=L, NDIR=NDIR)])[0]["PPW"]
    ny, nx = shape_of(4 * ppw + 1)
    dmin = -7
    cvs = aggregate(own, W.c_ints(300, ny, nx, L), dmin, NDIR, batch=nb)
    base0 = own.debug_lr_ptr(0, 0)
    for v in range(1, nb):
        for p in range(NDIR):  # (slot v's pass p is "pass v * NDIR + p" of slot 0)
            got = own.debug_lr_ptr(v, p)
            assert got and got[0] - base0[0] == 4 * (v * NDIR + p) * base0[2], (v, p)
        overwrite(own, np.full((NDIR, ny, nx, L), POISONS[0], np.float32), volume=v)
    Lk = base0[1]
    LPL = RC.lpl_of(Lk)
    lr = K.lr_votes(3000, NDIR, ny, nx, L, LPL)
    assert RC.pass_guard(lr).shape[0] == 8
    overwrite(own, lr)
    inst = check(own, plib, cvs[0], lr, dmin, NDIR, Lk, K.base_labels(ny, nx, L, LPL), ("pass_guard", L, NDIR))
    assert inst.endswith(",4>"), inst
    for h in cvs:
        h.free()


# ---- padded strides, the generic kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [100, 151])
def test_padding_slots_are_never_candidates(own, plib, L):
    """an odd width whose run padded the label stride (Lk read from the aid): slots L..Lk-1 of every pass hold -1e30, NaN, -INF or 0
    in turn.  The same width through mgm_aggregate_passes_dev, which never pads, lands on the generic kernel."""
    seen = set()
    for j, (NDIR, n) in enumerate(((8, 130), (4, 37))):
        ny, nx = shape_of(n)
        dmin = -(L // 2)
        Cv = W.c_ints(400 + j, ny, nx, L)
        for passes_only in (False, True):
            cv, = aggregate(own, Cv, dmin, NDIR, passes_only=passes_only)
            inst, Lk = crafted_round(own, plib, cv, dmin, NDIR, ny, nx, L, 5 * j + L, pad=POISONS[j % 4], nold=3)
            if Lk > L:
                assert not passes_only and Lk % 64 == 0 and inst.startswith("k_wta_consensus<%d," % (Lk // 64)), (inst, Lk)
                seen.add("padded")
            else:
                assert inst == "k_wta_consensus_any", (inst, Lk)
                seen.add("unpadded")
            cv.free()
    assert seen == {"padded", "unpadded"}, seen


@pytest.mark.parametrize("L", [1, 2, 37, 64, 300, 1100])
def test_the_generic_kernel_when_forced(own, plib, L, monkeypatch):
    """MGM_HIP_WTA_CONSENSUS_ANY=1: every class on the kernel that strides the labels over the lanes"""
    monkeypatch.setenv("MGM_HIP_WTA_CONSENSUS_ANY", "1")
    for j, (NDIR, n) in enumerate(((8, 65), (4, 130), (1, 9))):
        ny, nx = shape_of(n if L <= 300 else min(n, 65))
        dmin = (-5, 3, -(L // 2))[j % 3]
        cv, = aggregate(own, W.c_ints(500 + j, ny, nx, L), dmin, NDIR)
        inst, _ = crafted_round(own, plib, cv, dmin, NDIR, ny, nx, L, 4 * j + L % 7, force=1, nold=4)
        assert inst == "k_wta_consensus_any"
        cv.free()


# ---- several turns of the grid-stride loop -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,nx,ny,NDIR", [(256, 130, 40, 8), (64, 257, 45, 4)])
def test_several_turns(own, plib, L, nx, ny, NDIR, monkeypatch):
    """MGM_HIP_WTA_CONSENSUS_WG=1: one workgroup per CU, fewer waves than groups of pixels (tests/test_consensus_plan.py holds the
    planner to that on any device up to 304 CUs)"""
    monkeypatch.setenv("MGM_HIP_WTA_CONSENSUS_WG", "1")
    dmin = -(L // 2)
    cv, = aggregate(own, W.c_ints(600, ny, nx, L), dmin, NDIR)
    Lk = own.debug_lr_ptr(0, 0)[1]
    for cu in (1, 256, 304):
        g = CP.ask(plib, [CP.request(npix=nx * ny, L=L, Lk=Lk, NDIR=NDIR, num_cu=cu, sw_wg_per_cu=1)])[0]
        assert nx * ny > g["grid"] * 4 * g["per_wave"], g
    LPL = RC.lpl_of(Lk)
    lr = K.lr_votes(601, NDIR, ny, nx, L, LPL)
    overwrite(own, lr)
    check(own, plib, cv, lr, dmin, NDIR, Lk, K.base_labels(ny, nx, L, LPL), ("turns", L, nx, ny, NDIR), wg=1, tols=(0.5, 1.0))
    cv.free()


# ---- ragged volumes: the hull and the range-proportional copy --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["s64_c1", "s128_c2", "tiny"])
def test_ragged_both_routes_whatever_the_unowned_slots_hold(own, oracle, plib, name, monkeypatch):
    """the formats of tests/wta_rel_crafted.py (64 and 128 slots): the classes laid at every pixel's own range, the unowned slots of
    the range-proportional copy and the unowned labels and padding slots of the dense hull poisoned four ways.  Both routes equal
    the model, and therefore each other; the generic kernel reads the range-proportional layout too."""
    k = R.case(name)
    ny, nx, NDIR, dmin, L = k["ny"], k["nx"], k["NDIR"], k["dmin"], k["L"]
    zlo, zhi = k["lo"] - dmin, k["hi"] - dmin
    base = np.ravel(zlo) + K.base_labels(ny, nx, 3, 1) % np.ravel(zhi - zlo + 1)
    classes = ["votes"] + [c for n, c in enumerate(W.LR_CLASSES) if n % 3 == len(name) % 3]
    crafted = {}
    for j, cls in enumerate(classes):
        fn = K.classes(1)[cls]
        crafted[cls] = K.lay_in_windows(fn, R.SEED.get(cls, 690), NDIR, ny, nx, L, zlo, zhi)
    # the range-proportional copy
    p = Prepared(own, oracle, name)
    try:
        for j, cls in enumerate(classes):
            p.overwrite(crafted[cls], POISONS[j % 4])
            inst = check(own, plib, p.cv, crafted[cls], dmin, NDIR, k["slots"], base, (name, "rel", cls), lo=zlo, hi=zhi, slots=k["slots"], tols=(K.TOLS[j % 4], 1.0))
            assert inst == "k_wta_consensus_rel<%d>" % (k["slots"] // 16)
            MET.add(cls)
        monkeypatch.setenv("MGM_HIP_WTA_CONSENSUS_ANY", "1")
        p.overwrite(crafted["votes"], POISONS[1])
        assert check(own, plib, p.cv, crafted["votes"], dmin, NDIR, k["slots"], base, (name, "rel forced"), lo=zlo, hi=zhi, slots=k["slots"], force=1, tols=(0.5,)) == "k_wta_consensus_any"
        monkeypatch.delenv("MGM_HIP_WTA_CONSENSUS_ANY")
    finally:
        p.close()
    # the dense hull of the same volume
    os.environ["MGM_HIP_REL"] = "0"
    try:
        cv = own.costvolume(k["u"], k["v"], k["flo"], k["fhi"], "none", k["dist"], float("inf"), k["win"])
        own.timing(True)
        own.timing_reset()
        _, o, c = own.aggregate_dev(cv, k["P1"], k["P2"], NDIR, k["MGM"], k["FH"], 1, None, None)
        own.synchronize()
        names = [n for n, _ in own.timings()]
        own.timing(False)
    finally:
        os.environ.pop("MGM_HIP_REL", None)
    o.free(), c.free()
    assert "k_pass_rel" not in names, names
    for j, cls in enumerate(classes):
        Lk = overwrite(own, crafted[cls], pad=POISONS[(j + 1) % 4], lo=zlo, hi=zhi)
        inst = check(own, plib, cv, crafted[cls], dmin, NDIR, Lk, base, (name, "hull", cls), lo=zlo, hi=zhi, tols=(K.TOLS[j % 4], 1.0))
        assert inst != "k_wta_consensus_rel<%d>" % (k["slots"] // 16)
    own.trim()
    cv.free()


def test_every_instance_was_reached(own):
    """(the last test of the file)"""
    for inst in sorted(REACHED):
        print(inst, "<-", REACHED[inst])
    table = CP.launch_table()
    assert len(table) == 17 and set(REACHED) == table, sorted(set(REACHED) ^ table)
    assert MET == {"votes"} | set(W.LR_CLASSES), sorted(({"votes"} | set(W.LR_CLASSES)) ^ MET)
    own.trim()
