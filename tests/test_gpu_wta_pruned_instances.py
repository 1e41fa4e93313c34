"""Every instance of the pruned winner search (k_wta_pruned<PPW, MAXD, ALLD>: NDIR 1..8, one and two pixels per wave, fix_overcount
0 and 1) and the chunk minima k_pass2 writes for it, on inputs in which the chunks compete (wta_prune_model.INSTANCE_CASES; what
they are worth is measured on the CPU in tests/test_wta_bound.py).  Per case: the maps against the oracle and against the same call
under MGM_HIP_WTA_PRUNE=0 with the Lr volumes unchanged, the minima (mgm_debug_download_lmin) against the Lr volumes of the device
and of the oracle, and the two counters against the numpy emulation's count EXACTLY -- kernel and model take the same four steps on
the same floats.  The instances a switch selects (MGM_HIP_TUNE is read once per process) run in child processes, one at a time,
each compared with the oracle's digest."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import mgm_amd
import wta_prune_model as M
from helpers import ndiff

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgm_amd", "csrc")
NUM_CU, XCC_MASK = 256, 0xff  # an MI355X in SPX mode: what the planner harness is asked about
LINES2 = 15                   # pass2_lines(256, compact): lines per band of the 256-label compact kernels

DENSE_FIELDS = ("nx ny L nb first count layout_ndir MGM fh wmode use_c8 cb first_build ragged lines2 lpl ns devtools num_cu xcc_mask "
                "subv deep wg_per_cu strips xcdq xcdq_k one_queue w2 oneb").split()
DENSE_SCAL = ("err subv ngroups Lk R2 R w2 wk tags NS LPk wg_per_cu deep oneb xcdq nq QK one_queue any_strips maxLL ntasks hand_vstride "
              "h_npass h_groups h_slot_floats h_slots h_R").split()


class Planner:
    """plan_dense / plan_wta_prune (mgm_planner.h) on the host, through the harnesses of tests/test_planner.py and
    tests/test_wta_prune_planner.py: what a launch of `nb` 256-label one-byte volumes decides under the given tune values."""

    def __init__(self, tmp):
        libs = []
        for name in ("planner_harness", "prune_harness"):
            so = str(tmp / ("lib%s.so" % name))
            subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", CSRC, os.path.join(ROOT, "tests", name + ".cc"), "-o", so], check=True)
            libs.append(C.CDLL(so))
        self.plan_lib, self.prune_lib = libs
        assert self.prune_lib.dense_request_fields() == len(DENSE_FIELDS)

    def request(self, nx, ny, nb, NDIR, MGM, FH, **tune):
        q = dict(nx=nx, ny=ny, L=256, nb=nb, first=0, count=NDIR, layout_ndir=NDIR, MGM=MGM, fh=FH, wmode=0, use_c8=1, cb=1, first_build=0, ragged=0,
                 lines2=LINES2, lpl=4, ns=1, devtools=0, num_cu=NUM_CU, xcc_mask=XCC_MASK, subv=1, deep=-1, wg_per_cu=0, strips=-1, xcdq=-1, xcdq_k=-1,
                 one_queue=-1, w2=1, oneb=1)
        for k, v in tune.items():
            assert k in q, k
            q[k] = v
        return (C.c_int * len(DENSE_FIELDS))(*[q[f] for f in DENSE_FIELDS])

    def pruned(self, nx, ny, nb, NDIR, MGM, FH, refine, **tune):
        """Does the launch write minima and the search behind it prune?  (the Lr stride is a multiple of 32 floats: 256 per pixel
        plus a pad of 64-float blocks)"""
        call = (C.c_int * 8)(1, 1, 0, 1 if refine else 0, 0, NDIR, 256, 0)
        r = self.prune_lib.prune_for_launch(self.request(nx, ny, nb, NDIR, MGM, FH, **tune), call)
        assert r >= 0, "the plan failed"
        return bool(r)

    def plan(self, nx, ny, nb, NDIR, MGM, FH, **tune):
        cap = 1 << 14
        scal = np.zeros(len(DENSE_SCAL), np.int64)
        geom, base = np.zeros((8, 10), np.int32), np.zeros(8, np.int64)
        order, table = np.zeros((cap, 2), np.int32), np.zeros((cap + 8, 2), np.int32)
        ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        n = self.plan_lib.planner_dense(self.request(nx, ny, nb, NDIR, MGM, FH, **tune), ptr(scal, C.c_longlong), ptr(geom, C.c_int), ptr(base, C.c_longlong),
                                        ptr(order, C.c_int), ptr(table, C.c_int), cap)
        assert n >= 0
        p = dict(zip(DENSE_SCAL, (int(v) for v in scal)))
        assert p["err"] == 0
        return p


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    return Planner(tmp_path_factory.mktemp("prune_instances"))


# ---- one aggregation call on the device ------------------------------------------------------------------------------------------
class prune_env:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("MGM_HIP_WTA_PRUNE")
        os.environ["MGM_HIP_WTA_PRUNE"] = "1" if self.on else "0"

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["MGM_HIP_WTA_PRUNE"]
        else:
            os.environ["MGM_HIP_WTA_PRUNE"] = self.old


def run(ctx, cvs, P1, P2, NDIR, MGM, FH, fix, refine, prune):
    """Under MGM_HIP_WTA_PRUNE=prune: the maps per volume, every Lr volume of volume 0, the minima [slot][pass] (None: the launch
    wrote none), the counters, the kernels that ran."""
    with prune_env(prune):
        ctx.timing(True)
        ctx.timing_reset()
        if len(cvs) == 1:
            _, o, c = ctx.aggregate_dev(cvs[0], P1, P2, NDIR, MGM, FH, fix, None, refine)
            outs, outcs = [o], [c]
        else:
            _, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, FH, fix, None, refine)
        stats = ctx.wta_stats()
        names = [n for n, _ in ctx.timings()]
        ctx.timing(False)
        lr = [ctx.debug_lr(cvs[0], p) for p in range(NDIR)]
        try:
            lmin = [[ctx.debug_lmin(cvs[b], b, p) for p in range(NDIR)] for b in range(len(cvs))]
        except mgm_amd.MgmError as e:
            assert e.code == mgm_amd.MGM_ERR_INVALID
            lmin = None
        maps = [(o.download()[0], c.download()[0]) for o, c in zip(outs, outcs)]
        for h in outs + outcs:
            h.free()
    return maps, lr, lmin, stats, names


def expected_maps(r, refine):
    return (r["vout"], r["voutc"]) if refine == "vfit" else (r["out"], r["outc"])


def check(ctx, ref, cvs, P1, P2, NDIR, MGM, FH, fix, refine, pruned, what):
    """`ref`: per volume a dict as wta_prune_model.case_reference makes them."""
    maps1, lr1, lmin1, (px, ch), names1 = run(ctx, cvs, P1, P2, NDIR, MGM, FH, fix, refine, True)
    maps0, lr0, lmin0, stats0, names0 = run(ctx, cvs, P1, P2, NDIR, MGM, FH, fix, refine, False)
    ny, nx, L = ref[0]["C"].shape
    npix, emu = nx * ny * len(cvs), sum(r["chunks"] for r in ref)
    print("%s: %d pixels, %d chunks loaded, emulation %d (%s)" % (what, px, ch, emu, "pruned" if pruned else "plain search expected"))
    assert "k_wta" in names1 and "k_wta" in names0
    for b, r in enumerate(ref):
        eo, ec = expected_maps(r, refine)
        assert ndiff(maps1[b][0], eo) == 0 and ndiff(maps1[b][1], ec) == 0, "%s: volume %d differs from the oracle" % (what, b)
        assert ndiff(maps1[b][0], maps0[b][0]) == 0 and ndiff(maps1[b][1], maps0[b][1]) == 0, "%s: volume %d differs from the plain search" % (what, b)
    for p in range(NDIR):
        assert ndiff(lr1[p], lr0[p]) == 0, "%s: Lr of pass %d changed" % (what, p)
    assert stats0 == (0, 0) and lmin0 is None, "MGM_HIP_WTA_PRUNE=0 must take the plain search and leave no minima"
    if not pruned:
        assert (px, ch) == (0, 0) and lmin1 is None, "%s: this launch must fall back to the plain search" % what
        return
    assert "k_pass2" in names1
    assert lmin1 is not None, "%s: the launch wrote no minima" % what
    own = M.chunk_minima(np.stack(lr1))
    for b, r in enumerate(ref):
        want = M.chunk_minima(r["lr"])
        for p in range(NDIR):
            assert ndiff(lmin1[b][p], want[p]) == 0, "%s: minima of volume %d, pass %d are not the oracle's Lr reduced" % (what, b, p)
            if b == 0:
                assert ndiff(lmin1[0][p], own[p]) == 0, "%s: minima of pass %d are not the device's Lr reduced" % (what, p)
    assert (px, ch) == (npix, emu), "%s: counters (%d, %d), emulation (%d, %d)" % (what, px, ch, npix, emu)


def upload_case(ctx, spec, ref):
    """(handles to free, cost volumes): ramp volumes are uploaded (k_compact makes the bytes), pairs are built on the device."""
    inp = spec[0]
    if inp[0] == "ramp":
        cvs = [ctx.upload_volume(r["C"], M.RAMP_DMIN) for r in ref]
        return list(cvs), cvs
    u, v = M.wide_pair(M.PAIR_SEED)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    cv = ctx.costvolume_dev(du, dv, -255, 0, "none", inp[1], float(inp[2]), 5)
    return [du, dv, cv], [cv]


@pytest.mark.parametrize("name", sorted(M.INSTANCE_CASES))
def test_instance_case(ctx, oracle, planner, name):
    spec = M.INSTANCE_CASES[name]
    inp, NDIR, MGM, FH, P1, P2, fix, refine, floor = spec
    ref = M.case_reference(oracle, name)
    ny, nx, L = ref[0]["C"].shape
    pruned = planner.pruned(nx, ny, len(ref), NDIR, MGM, FH, refine)  # (17x1, 1x17, 5x3 included: the planner says, the test does not guess)
    handles, cvs = upload_case(ctx, spec, ref)
    try:
        check(ctx, ref, cvs, P1, P2, NDIR, MGM, FH, fix, refine, pruned, name)
    finally:
        for h in handles:
            h.free()


def test_pass_count_changes_between_launches_on_one_context(ctx, oracle, planner):
    """8 passes, then 3, then two volumes of 5, then 8 again, without anything freed in between: last_ndir, last_stride and the
    slots' places in the minima follow the launch."""
    seq = ["r97_fh8_vfit", "r97_fh3_t4_frac_vfit", "r61_hi5_t4_x2_vfit", "r97_hi1_vfit", "r97_hi8_none"]
    handles = []
    try:
        for name in seq:
            spec = M.INSTANCE_CASES[name]
            ref = M.case_reference(oracle, name)
            h, cvs = upload_case(ctx, spec, ref)
            handles += h
            check(ctx, ref, cvs, spec[4], spec[5], spec[1], spec[2], spec[3], spec[6], spec[7], True, "sequence/" + name)
    finally:
        for h in handles:
            h.free()


def test_refilled_volume_other_settings_other_ndir(ctx, oracle):
    """One volume: census costs searched with 8 FH passes, then filled again with truncated AD costs and searched with 5
    Hirschmueller passes without the over-count fix.  Between the refill and the second launch the minima of the first are refused.
    (A volume made by mgm_cv_upload cannot be filled again through the ABI, so the refilled volume is the pair's.)"""
    first, again = "p330_census_fh8_vfit", ("pair", "ad", 30.0)
    spec = M.INSTANCE_CASES[first]
    ref = M.case_reference(oracle, first)
    u, v = M.wide_pair(M.PAIR_SEED)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    cv = ctx.costvolume_dev(du, dv, -255, 0, "none", "census", float("inf"), 5)
    try:
        check(ctx, ref, [cv], spec[4], spec[5], spec[1], spec[2], spec[3], spec[6], spec[7], True, first)
        with prune_env(True):
            ctx.timing(True)
            _, o, c = ctx.aggregate_dev(cv, spec[4], spec[5], spec[1], spec[2], spec[3], spec[6], None, spec[7])
            ctx.timing(False)
            o.free(), c.free()
            assert ctx.debug_lmin(cv, 0, 7).shape == (18, 330, 8)
            for slot, p in ((1, 0), (-1, 0), (0, 8), (0, -1)):
                with pytest.raises(mgm_amd.MgmError):
                    ctx.debug_lmin(cv, slot, p)
            ctx.costvolume_dev(du, dv, -255, 0, "none", "ad", 30.0, 5, into=cv)
            with pytest.raises(mgm_amd.MgmError) as e:
                ctx.debug_lmin(cv, 0, 0)
            assert e.value.code == mgm_amd.MGM_ERR_INVALID
        C2 = oracle.costvolume(u, v, -255, 0, "none", "ad", 30.0, 5)
        S, out, outc, lr = oracle.mgm(C2, -255, 8.0, 32.0, 5, 3, 0, 0, dump_lr=True)
        vout, voutc = oracle.refine(S, -255, "vfit", out, outc)
        label, cost, chunks, Sm, LB, load = M.pruned_search(C2, lr, -255, 0)
        r2 = dict(C=C2, lr=lr, out=out, outc=outc, vout=vout, voutc=voutc, chunks=chunks)
        check(ctx, [r2], [cv], 8.0, 32.0, 5, 3, 0, 0, "vfit", True, "refilled")
    finally:
        for h in (du, dv, cv):
            h.free()


def test_one_pixel_without_a_finite_label(ctx, oracle):
    """One pixel +INF on all labels.  The oracle decides what comes out; the library may search it pruned or refuse (k_nanscan,
    k_pass_exact): either way the maps are the oracle's and the plain search's, and the counters say which path it took.  Behind
    the dead pixel Lr is INF - INF = NaN along every scan line (109 pixels without a label), the minima of those chunks are NaN,
    and the kernel's fminf drops a NaN bound: such a pixel loads nothing, as in the emulation (wta_prune_model.pruned_search, step
    (a)).  The count is held to the emulation fed with the DEVICE's Lr volumes and minima, and the minima to the device's Lr
    wherever that is NaN-free (the pass kernels are built NaN-free: what their minimum makes of a NaN is theirs to choose)."""
    C1 = M.dead_pixel_volume()
    ny, nx, L = C1.shape
    S, out, outc, lr = oracle.mgm(C1, M.RAMP_DMIN, 8.0, 32.0, 8, 1, 0, 1, dump_lr=True)
    vout, voutc = oracle.refine(S, M.RAMP_DMIN, "vfit", out, outc)
    cv = ctx.upload_volume(C1, M.RAMP_DMIN)
    try:
        maps1, lr1, lmin1, (px, ch), names1 = run(ctx, [cv], 8.0, 32.0, 8, 1, 0, 1, "vfit", True)
        maps0, lr0, lmin0, stats0, names0 = run(ctx, [cv], 8.0, 32.0, 8, 1, 0, 1, "vfit", False)
        assert ndiff(maps1[0][0], vout) == 0 and ndiff(maps1[0][1], voutc) == 0
        assert ndiff(maps1[0][0], maps0[0][0]) == 0 and ndiff(maps1[0][1], maps0[0][1]) == 0
        assert stats0 == (0, 0) and lmin0 is None
        if lmin1 is not None:  # searched pruned
            dev_lr, dev_min = np.stack(lr1), np.stack(lmin1[0])
            with np.errstate(invalid="ignore"):
                own = M.chunk_minima(dev_lr)
            clean = ~np.isnan(own)
            emu = M.pruned_search(C1, dev_lr, M.RAMP_DMIN, 1, minima=dev_min)[2]
            print("dead pixel: counters (%d, %d), emulation on the device's Lr and minima %d, on the oracle's %d; %d words of Lr differ from the "
                  "oracle's, %d are NaN, %d minima are NaN; %d pixels without a label"
                  % (px, ch, emu, M.pruned_search(C1, lr, M.RAMP_DMIN, 1)[2], ndiff(dev_lr, lr), int(np.isnan(dev_lr).sum()), int(np.isnan(dev_min).sum()),
                     int(np.isnan(out).sum())))
            assert "k_pass2" in names1
            assert ndiff(dev_min[clean], own[clean]) == 0
            assert (px, ch) == (nx * ny, emu)
        else:                  # the refusal of the pruned path
            print("dead pixel: plain search, kernels %s" % sorted(set(names1)))
            assert (px, ch) == (0, 0)
    finally:
        cv.free()


# ---- the instances a switch selects: one fresh process per setting ------------------------------------------------------------
CHILD_CASES = [  # name, NDIR, TSGM, FH, P1, P2, fix
    ("fh8", 8, 3, 1, 2.0, 20000.0, 1),
    ("hi4", 4, 3, 0, 8.0, 32.0, 1),
    ("hi5_nofix", 5, 3, 0, 8.0, 32.0, 0),
]
CHILD_MODES = [("vfit", "vfit", (7,)), ("none", None, (7,)), ("x2", "vfit", (7, 8))]  # refinement, seeds of the batch

SCRIPT = r"""
import sys, hashlib, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import mgm_amd
import wta_prune_model as M
nx, ny = int(sys.argv[1]), int(sys.argv[2])
CASES, MODES = %r, %r
def words(a):  # bytes to digest: NaN is NaN whatever its sign and payload, every other float its own bits
    a = np.array(a, np.float32, copy=True)
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a).tobytes()
ctx = mgm_amd.Context(0)
ctx.timing(True)
vols = {s: M.ramp_volume(nx, ny, 256, s) for s in (7, 8)}
for name, NDIR, MGM, FH, P1, P2, fix in CASES:
    for mode, refine, seeds in MODES:
        cvs = [ctx.upload_volume(vols[s], M.RAMP_DMIN) for s in seeds]
        ctx.timing_reset()
        if len(cvs) == 1:
            _, o, c = ctx.aggregate_dev(cvs[0], P1, P2, NDIR, MGM, FH, fix, None, refine)
            outs, outcs = [o], [c]
        else:
            _, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, FH, fix, None, refine)
        px, ch = ctx.wta_stats()
        ran = [n for n, _ in ctx.timings()]
        if (px, ch) == (0, 0):
            print("FALLBACK", name, mode)
        else:
            assert "k_wta" in ran and "k_pass2" in ran, ran
            h = hashlib.sha256()
            for b in range(len(cvs)):
                h.update(words(outs[b].download()[0]))
                h.update(words(outcs[b].download()[0]))
                for p in range(NDIR):
                    h.update(words(ctx.debug_lmin(cvs[b], b, p)))
            print("RAN", name, mode, px, ch, h.hexdigest())
        for x in outs + outcs + cvs:
            x.free()
ctx.close()
""" % (ROOT, os.path.join(ROOT, "tests"), CHILD_CASES, CHILD_MODES)

# MGM_HIP_TUNE (keys: dev() in mgm_ctx.hip, launch_wta in mgm_wta.hip) -> the same values as plan_dense takes them
SETTINGS = {
    "default": ("", {}),
    "ppw1": ("wta_prune_ppw=1", {}),          # k_wta_pruned<1, 8, true> / <1, 4, true> for NDIR 8 / 4
    "wg1": ("wta_prune_wg=1", {}),            # the grid capped at num_cu workgroups: 3201 pixels take several turns of the grid-stride loop
    "deep0": ("deep=0", dict(deep=0)),
    "xcdq0": ("xcdq=0", dict(xcdq=0)),
    "xcdq1_k1": ("xcdq=1,xcdq_k=1", dict(xcdq=1, xcdq_k=1)),
    "strips1": ("strips=1", dict(strips=1)),
    "strips0": ("strips=0", dict(strips=0)),
}
# 97x33 everywhere but for the strips: a line is walked in two strips from 8 x 15 = 120 pixels on (plan_dense), so at 97x33 neither
# setting changes a launch; 121x33 is the smallest odd width at which strips=1 and strips=0 select different instances (asserted below)
STRIP_SIZE = (121, 33)
_expect = {}


def words(a):
    """Bytes to digest: NaN is NaN whatever its sign and payload (as helpers.ndiff has it), every other float its own bits."""
    a = np.array(a, np.float32, copy=True)
    a[np.isnan(a)] = np.nan
    return np.ascontiguousarray(a).tobytes()


def child_expectation(oracle, nx, ny):
    """{(case, mode): (pixels, chunks, digest)} from the oracle and the emulation alone."""
    if (nx, ny) not in _expect:
        exp = {}
        for name, NDIR, MGM, FH, P1, P2, fix in CHILD_CASES:
            per_seed = {}
            for s in (7, 8):
                Cs = M.ramp_volume(nx, ny, 256, s)
                S, out, outc, lr = oracle.mgm(Cs, M.RAMP_DMIN, P1, P2, NDIR, MGM, FH, fix, dump_lr=True)
                vout, voutc = oracle.refine(S, M.RAMP_DMIN, "vfit", out, outc)
                assert not np.isnan(out).any()
                per_seed[s] = (out, outc, vout, voutc, M.chunk_minima(lr), M.pruned_search(Cs, lr, M.RAMP_DMIN, fix)[2])
            for mode, refine, seeds in CHILD_MODES:
                h, chunks = hashlib.sha256(), 0
                for s in seeds:
                    out, outc, vout, voutc, mins, emu = per_seed[s]
                    h.update(words(vout if refine else out))
                    h.update(words(voutc if refine else outc))
                    for p in range(NDIR):
                        h.update(words(mins[p]))
                    chunks += emu
                exp[(name, mode)] = (nx * ny * len(seeds), chunks, h.hexdigest())
        _expect[(nx, ny)] = exp
    return _expect[(nx, ny)]


def test_switches_select_other_pass_kernels(planner):
    """What each setting changes, by the planner: the ring depth, the queues, their block, the strips -- and nothing of the decision
    to prune."""
    plan = lambda nx, ny, nb, nd, fh, **kw: planner.plan(nx, ny, nb, nd, 3, fh, **kw)
    base = plan(97, 33, 1, 8, 1)
    assert (base["deep"], base["xcdq"], base["any_strips"]) == (1, 1, 0)
    assert plan(97, 33, 1, 8, 1, deep=0)["deep"] == 0
    assert plan(97, 33, 1, 8, 1, xcdq=0)["xcdq"] == 0
    k1 = plan(97, 33, 1, 8, 1, xcdq=1, xcdq_k=1)
    assert k1["xcdq"] == 1 and k1["QK"] == 1 and base["QK"] != 1
    assert plan(97, 33, 2, 5, 0)["xcdq"] == 1 and plan(97, 33, 1, 5, 0)["xcdq"] == 0  # (the batch of two brings NDIR 5 to the queues)
    for nd, fh in ((8, 1), (5, 0)):
        assert plan(97, 33, 1, nd, fh, strips=1)["any_strips"] == 0, "97x33 has no line long enough for strips"
        assert plan(119, 33, 1, nd, fh, strips=1)["any_strips"] == 0
        assert plan(*STRIP_SIZE, 1, nd, fh, strips=1)["any_strips"] == 1 and plan(*STRIP_SIZE, 1, nd, fh, strips=0)["any_strips"] == 0
    for key, (tune, kw) in SETTINGS.items():
        for name, NDIR, MGM, FH, P1, P2, fix in CHILD_CASES:
            for nb in (1, 2):
                for size in ((97, 33), STRIP_SIZE):
                    assert planner.pruned(*size, nb, NDIR, MGM, FH, "vfit", **kw), (key, name, nb, size)


@pytest.mark.parametrize("key", list(SETTINGS))
def test_switch_setting(oracle, planner, key):
    tune, kw = SETTINGS[key]
    nx, ny = STRIP_SIZE if key.startswith("strips") else (97, 33)
    exp = child_expectation(oracle, nx, ny)
    env = dict(os.environ, MGM_HIP_TUNE=tune, MGM_HIP_WTA_PRUNE="1")
    r = subprocess.run([sys.executable, "-c", SCRIPT, str(nx), str(ny)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w and w[0] == "RAN":
            got[(w[1], w[2])] = (int(w[3]), int(w[4]), w[5])
        elif w and w[0] == "FALLBACK":
            got[(w[1], w[2])] = None
    assert sorted(got) == sorted(exp), r.stdout[-2000:]
    for (name, mode), want in sorted(exp.items()):
        NDIR, MGM, FH = [(c[1], c[2], c[3]) for c in CHILD_CASES if c[0] == name][0]
        nb = len([m for m in CHILD_MODES if m[0] == mode][0][2])
        pruned = planner.pruned(nx, ny, nb, NDIR, MGM, FH, mode != "none", **kw)
        print("%s %s/%s: %s, expected %s" % (key, name, mode, got[(name, mode)], want if pruned else "the plain search"))
        if not pruned:
            assert got[(name, mode)] is None, "%s %s/%s: the planner refuses the pruned search here, the launch ran it" % (key, name, mode)
            continue
        assert got[(name, mode)] is not None, "%s %s/%s fell back to the plain search" % (key, name, mode)
        assert got[(name, mode)][:2] == want[:2], "%s %s/%s: counters %s, emulation %s" % (key, name, mode, got[(name, mode)][:2], want[:2])
        assert got[(name, mode)][2] == want[2], "%s %s/%s: maps or minima differ from the oracle's" % (key, name, mode)
