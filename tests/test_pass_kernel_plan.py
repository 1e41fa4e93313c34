"""Which instance of a pass kernel a launch runs (PassKernelChoice, mgm_amd/csrc/mgm_planner.h) on the host: plan_dense and
plan_rel choose what the three launch cascades chose before the choice moved into the plan (tests/pass_kernel_model.py: the
cascades restated, applied to the parameters run_passes / run_rel build from the plan), every field equal, refusals included;
every declared instance is chosen somewhere and every choice is declared; no request plan_dense_kernels or plan_agg_route can
produce is refused; the flags the cascades ignored silently cannot come out of plan_dense in those combinations at all; and the
harness, as a stand-alone program under the address and undefined-behaviour sanitizers, answers the sweep's corners alike."""
import ctypes as C
import itertools
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import pass_kernel_model as M
import route_plan_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgm_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "pass_kernel_harness.cc")

DENSE_FIELDS = ("nx ny L nb first count layout_ndir MGM fh wmode use_c8 cb first_build ragged lines2 lpl ns devtools num_cu xcc_mask "
                "subv deep wg_per_cu strips xcdq xcdq_k one_queue w2 oneb").split()
REL_FIELDS = ("nx ny NDIR nb MGM fh pube fh2 slots cb R HS diag_fits num_cu rel_wg rel_prio rel_lag rel_lagd rel_slots rel_slope1 rel_swap "
              "rel_diag rel_strips rel_multi").split()
DENSE_PLAN = "err R2 R subv deep xcdq one_queue oneb w2 wk wg_per_cu".split()
REL_PLAN = "err rel_wg diag_any".split()
NC = len(M.CHOICE)
NO_KERNEL = 4  # kPlanNoKernel
SWITCHES = dict(subv=1, deep=-1, wg_per_cu=0, strips=-1, xcdq=-1, xcdq_k=-1, one_queue=-1, w2=1, oneb=1)  # the defaults (DevSwitches, MGM_HIP_TUNE)
SIZES = ((5, 3), (150, 110), (1920, 1080))
ALL_LABELS = tuple(range(64, 2049, 64)) + (100, 151)  # every multiple of 64 (the first build takes each); 100 and 151 as the first build sees them
SECOND_LABELS = (64, 128, 192, 256, 384, 512, 768, 1024)  # what the second build takes: 100 / 151 run padded to 128 / 192
C8_FORMS = ((0, 1), (1, 1), (1, 2))  # (use_c8, cb)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("passkernel") / "libpass_kernel_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, HARNESS, "-o", so], check=True)
    lib = C.CDLL(so)
    assert (lib.pass_dense_request_ints(), lib.pass_rel_request_ints(), lib.pass_choice_ints()) == (len(DENSE_FIELDS), len(REL_FIELDS), NC)
    return lib


def call(fn, rows, nout, *extra):
    a = np.ascontiguousarray(rows, dtype=np.int32)
    out = np.zeros((len(a), nout) if nout > 1 else len(a), dtype=np.int32)
    fn(a.ctypes.data_as(C.c_void_p), C.c_int(len(a)), *extra, out.ctypes.data_as(C.c_void_p))
    return out


def call_threads(fn, rows, nout, threads=8):
    """call() over interleaved eighths of the rows at once (the planner is a pure function, and ctypes drops the interpreter lock)."""
    out = np.zeros((len(rows), nout), dtype=np.int32)
    with ThreadPoolExecutor(threads) as ex:
        for k, part in enumerate(ex.map(lambda k: call(fn, rows[k::threads], nout), range(threads))):
            out[k::threads] = part
    return out


def cross(**axes):
    """The cross product of the axes as columns (dict of flat arrays); an axis of tuples fills the fields its key names ("a,b")."""
    names, values = list(axes), [np.atleast_2d(np.array(v, dtype=np.int64).T).T for v in axes.values()]
    idx = np.meshgrid(*[np.arange(len(v)) for v in values], indexing="ij")
    cols = {}
    for name, v, i in zip(names, values, idx):
        for k, f in enumerate(name.split(",")):
            cols[f] = v[i.ravel(), k]
    return cols


LPL_OF = np.array([0] + [M.pass_lpl(L) for L in range(1, 2049)])
LINES2 = np.array([[M.pass2_lines(L, c8) for L in range(2049)] for c8 in (0, 1)])


def dense_requests(lib, cols, **fixed):
    """Requests as run_passes fills them: lpl, ns and lines2 as the kernels report them, the hand-off region laid out for the launch's passes."""
    n = len(next(iter(cols.values())))
    q = dict(first=0, count=8, ragged=0, devtools=0, num_cu=256, xcc_mask=0xff, **SWITCHES)
    q.update(fixed)
    q.update(cols)
    q = {k: np.broadcast_to(np.asarray(v, dtype=np.int64), (n,)) for k, v in q.items()}
    q["layout_ndir"] = q["first"] + q["count"]
    q["lpl"] = LPL_OF[q["L"]]
    q["ns"] = np.where((q["wmode"] != 0) & (q["fh"] == 0), 2, 1)
    q["lines2"] = np.zeros(n, dtype=np.int64)
    rows = np.stack([q[f] for f in DENSE_FIELDS], axis=1).astype(np.int32)
    subv = call(lib.pass_dense_subv, rows, 1)
    rows[:, DENSE_FIELDS.index("lines2")] = LINES2[(q["use_c8"] != 0).astype(int), np.minimum(q["L"] * subv, 2048)]
    return rows


BASE = dict(MGM=(1, 2, 3, 4), fh=(0, 1), wmode=(0, 1, 2), first_build=(0, 1), devtools=(0, 1))
BASE["use_c8,cb"] = C8_FORMS
# every development switch at each of its values, the other request fields one at a time
VARIANTS = [dict([kv]) for kv in (("subv", 0), ("subv", 2), ("deep", 0), ("deep", 1), ("wg_per_cu", 1), ("wg_per_cu", 2), ("strips", 0), ("strips", 1), ("xcdq", 0),
                                  ("xcdq", 1), ("xcdq", 2), ("xcdq_k", 0), ("xcdq_k", 2), ("one_queue", 0), ("one_queue", 1), ("w2", 0), ("oneb", 0), ("ragged", 1),
                                  ("xcc_mask", 0x0f), ("xcc_mask", 0), ("num_cu", 32))]
VARIANTS += [dict(first=f, count=c) for f, c in ((0, 4), (0, 2), (2, 1), (4, 4))] + [dict(deep=0, subv=2), dict(wg_per_cu=2, oneb=0), dict(xcdq=1, wg_per_cu=2)]


def dense_sweep(lib):
    """The plan's cost grows with the square of the volume count, so the whole cross of the kernel-relevant fields runs at 5x3 and at
    150x110 for the label counts whose volumes share waves (and 256); the other label counts, the switches (at 40x20: launches on
    both sides of the 32 work items the queues need) and 1920x1080 run at fewer volume counts."""
    blocks = [dense_requests(lib, cross(L=ALL_LABELS, nb=range(1, 17), **BASE), nx=5, ny=3)]
    blocks.append(dense_requests(lib, cross(L=(64, 128, 256), nb=range(1, 17), **BASE), nx=150, ny=110))
    blocks.append(dense_requests(lib, cross(L=(100, 151, 192, 320, 384, 512, 768, 1024, 1536, 2048), nb=(1, 2, 3, 4, 8), **BASE), nx=150, ny=110))
    for v in VARIANTS:
        blocks.append(dense_requests(lib, cross(L=SECOND_LABELS, nb=(1, 2, 3, 8), **BASE), nx=40, ny=20, **v))
        blocks.append(dense_requests(lib, cross(L=(64, 256, 512), nb=(1, 4), **BASE), nx=150, ny=110, **v))
    hd = dict(BASE, first_build=(0,), devtools=(0,))
    blocks.append(dense_requests(lib, cross(L=(64, 128, 256, 512, 1024), nb=(1, 2, 3, 12), **hd), nx=1920, ny=1080))
    for v in (dict(num_cu=32), dict(xcc_mask=0x0f), dict(xcc_mask=0), dict(wg_per_cu=2)):
        blocks.append(dense_requests(lib, cross(L=(64, 128, 256, 512, 1024), nb=(1, 2, 3), **hd), nx=1920, ny=1080, **v))
    blocks.append(dense_requests(lib, cross(L=(256, 2048), nb=(1, 3), **dict(BASE, first_build=(1,))), nx=1920, ny=1080))
    return np.concatenate(blocks)


def parent_dense(q, plan):
    """The parent's launch of stage 6 of run_passes on the parameters of stage 5: q, plan as dicts."""
    if plan["R2"]:
        p = dict(L=q["L"], subv=plan["subv"], C8=q["use_c8"], cbytes=q["cb"] if q["use_c8"] else 1, deep=plan["deep"],
                 xcdq=(2 if plan["one_queue"] else 1) if plan["xcdq"] else 0, oneb=plan["oneb"], wsel=plan["w2"], MGM=q["MGM"], wg_per_cu=plan["wg_per_cu"])
        return M.launch_pass2(p, bool(q["fh"]), 2 if plan["w2"] else (1 if plan["wk"] else 0), bool(q["devtools"]))
    return M.launch_pass(dict(L=q["L"]), plan["R"], bool(q["fh"]), 1 if q["wmode"] else 0)


@pytest.fixture(scope="module")
def swept(lib):
    """(requests, plans) of the dense sweep and of the range-proportional one; what they reached."""
    d = dense_sweep(lib)
    r = rel_sweep()
    return dict(dense=(d, call_threads(lib.pass_kernel_dense, d, len(DENSE_PLAN) + NC)), rel=(r, call(lib.pass_kernel_rel, r, len(REL_PLAN) + NC)))


def test_dense_sweep_chooses_what_the_cascades_launched(swept):
    rows, out = swept["dense"]
    assert len(rows) > 450000
    # what the parent's launch read: the request's share and the plan's; one answer per distinct combination
    at = [DENSE_FIELDS.index(f) for f in "L MGM fh wmode use_c8 cb devtools".split()]
    both = np.unique(np.concatenate([rows[:, at], out], axis=1), axis=0)
    for r in both.tolist():
        q, plan, got = dict(zip("L MGM fh wmode use_c8 cb devtools".split(), r)), dict(zip(DENSE_PLAN, r[7:])), tuple(r[7 + len(DENSE_PLAN):])
        if plan["err"] not in (0, NO_KERNEL):  # (no launch: the plan was refused for its geometry or lost its queues)
            assert got == M.choice(M.REFUSE), (q, plan, got)
            continue
        want = parent_dense(q, plan)
        assert (plan["err"] == NO_KERNEL) == (want is None), (q, plan, got, want)
        assert got == (want or M.choice(M.REFUSE)), (q, plan, dict(zip(M.CHOICE, got)), want and dict(zip(M.CHOICE, want)))
    assert {e for e in np.unique(out[:, 0]).tolist()} >= {0, NO_KERNEL}


def test_flags_the_cascades_ignored_cannot_come_out_of_plan_dense(swept):
    """launch2_one fell through to a kernel without queues for xcdq without deep rings, ignored oneb without xcdq, and deep / xcdq on
    the weighted, the TSGM-2 FH and the fp32-cost kernels; it refused queues with several volumes per wave.  plan_dense produces none
    of these: the queues need deep rings and one volume per wave, the deep rings tags and compact costs, oneb the queues."""
    rows, out = swept["dense"]
    p = {f: out[:, k] for k, f in enumerate(DENSE_PLAN)}
    q = {f: rows[:, k] for k, f in enumerate(DENSE_FIELDS)}
    ok = p["err"] == 0
    slabs_of_E = (p["wk"] == 0) & ~((q["fh"] != 0) & (q["MGM"] == 2))
    for what, bad in (("xcdq without deep", (p["xcdq"] != 0) & (p["deep"] == 0)), ("oneb without xcdq", (p["oneb"] != 0) & (p["xcdq"] == 0)),
                      ("xcdq with several volumes per wave", (p["xcdq"] != 0) & (p["subv"] > 1)), ("deep on fp32 costs", (p["deep"] != 0) & (q["use_c8"] == 0)),
                      ("deep without slabs of E", (p["deep"] != 0) & ~slabs_of_E & (p["w2"] == 0)), ("deep on the first build", (p["deep"] != 0) & (p["R2"] == 0))):
        assert not np.any(ok & bad), what
    assert np.any(ok & (p["xcdq"] != 0)) and np.any(ok & (p["deep"] != 0) & (p["xcdq"] == 0)) and np.any(ok & (p["oneb"] != 0)) and np.any(ok & (p["subv"] > 1))


# ---- the range-proportional kernels ------------------------------------------------------------------------------------------
def rel_hand_floats(one_slab, slots, fh2):
    return (3 * slots + 2 * (slots // 16) if fh2 else (slots + 2 * (slots // 16) if one_slab else 2 * slots)) + 4


def rel_lds_bytes(one_slab, slots, cb, fh2, diag):
    HS = rel_hand_floats(one_slab, slots, fh2)
    return 4 * (16 * 4 * HS + (2 if diag else 1) * 8 * HS + 2 * 8 * 16 * 4) + 8 * 16 * slots * cb + 4 * (8 + 4) + 16 + 4 * 16 * 24


def rel_request(nx=150, ny=110, NDIR=8, nb=1, MGM=3, fh=1, weighted=0, slots=64, cb=1, rel_wg=0, rel_multi=1, rel_diag=1, num_cu=256):
    """A request as run_rel fills it."""
    pube, fh2 = int(not fh and not weighted), int(bool(fh) and MGM == 2 and not weighted)
    q = dict(nx=nx, ny=ny, NDIR=NDIR, nb=nb, MGM=MGM, fh=fh, pube=pube, fh2=fh2, slots=slots, cb=cb, R=16, HS=rel_hand_floats(fh or pube, slots, fh2),
             diag_fits=int(rel_lds_bytes(fh or pube, slots, cb, fh2, True) <= 160 * 1024), num_cu=num_cu, rel_wg=rel_wg, rel_prio=5 if nb <= 1 else 0, rel_lag=0,
             rel_lagd=0, rel_slots=100, rel_slope1=1, rel_swap=1, rel_diag=rel_diag, rel_strips=1, rel_multi=rel_multi)
    return [q[f] for f in REL_FIELDS]


def rel_sweep():
    rows = [rel_request(nx, ny, nb=nb, MGM=MGM, fh=fh, weighted=w, slots=slots, cb=cb, rel_wg=wg, rel_multi=multi, rel_diag=diag)
            for (nx, ny), nb, MGM, fh, w, slots, cb, wg, multi, diag in itertools.product(((5, 3), (150, 110)), (1, 2), (1, 2, 3, 4), (0, 1), (0, 1), (64, 128), (1, 2, 4),
                                                                                        range(0, 7), (0, 1), (0, 1))]
    return np.array(rows, dtype=np.int32)


def test_rel_sweep_chooses_what_the_cascade_launched(swept):
    rows, out = swept["rel"]
    assert len(rows) > 10000
    at = [REL_FIELDS.index(f) for f in "slots cb rel_multi fh2 MGM fh pube".split()]
    for r in np.unique(np.concatenate([rows[:, at], out], axis=1), axis=0).tolist():
        q, plan, got = dict(zip("slots cb fh_multi fh2 MGM fh pube".split(), r)), dict(zip(REL_PLAN, r[7:])), tuple(r[7 + len(REL_PLAN):])
        assert plan["err"] in (0, NO_KERNEL)
        want = M.launch_pass_rel(dict(q, diag_any=plan["diag_any"]), bool(q["fh"]), bool(q["pube"]), plan["rel_wg"])  # (the LDS bytes are part of it)
        assert (plan["err"] == NO_KERNEL) == (want is None), (q, plan, got, want)
        assert got == (want or M.choice(M.REFUSE)), (q, plan, dict(zip(M.CHOICE, got)), want and dict(zip(M.CHOICE, want)))
    # the one refusal: update_cost2_trunclinear on 128 slots of fp32 costs
    refused = rows[out[:, 0] == NO_KERNEL]
    assert len(refused) and all(dict(zip(REL_FIELDS, r))["fh2"] and (r[REL_FIELDS.index("slots")], r[REL_FIELDS.index("cb")]) == (128, 4) for r in refused.tolist())


# ---- declared and reached -----------------------------------------------------------------------------------------------------
def declared(lib, dev):
    """Every instance the shared statement admits, as choices without their launch numbers."""
    tf = (0, 1)
    cand = [M.choice(M.FIRST, LPL=l, FH=f, WEIGHTED=w, R=r) for l, f, w, r in itertools.product(range(0, 34), tf, tf, (4, 8, 16))]
    cand += [M.choice(M.SECOND, LPL=l, FH=f, WEIGHTED=w, MGM=m, C8=c, SUBV=s, DEEP=d, XCDQ=x, ONEB=o, W2=w2)
             for l, f, w, m, c, s, d, x, o, w2 in itertools.product(range(0, 18), tf, tf, range(0, 6), range(0, 4), range(0, 6), tf, tf, tf, tf)]
    cand += [M.choice(M.REL, FH=f, PUBE=p, NK=k, SPL=s, CB=c, FH2=f2) for f, p, k, s, c, f2 in itertools.product(tf, tf, range(0, 6), (2, 4, 8, 16), range(0, 6), tf)]
    cand.append(M.choice(M.REFUSE))
    yes = call(lib.pass_kernel_exists, cand, 1, C.c_int(dev))
    return {c for c, y in zip(cand, yes.tolist()) if y}


def bare(choices):
    z = [M.CHOICE.index("lds"), M.CHOICE.index("block")]
    c = np.array(choices, dtype=np.int64).reshape(-1, NC)
    c[:, z] = 0
    return {tuple(r) for r in c.tolist()}


def test_every_declared_instance_is_chosen_and_every_choice_is_declared(lib, swept):
    full, dev = declared(lib, 0), declared(lib, 1)
    per = lambda s, fam: sum(1 for c in s if c[0] == fam)
    # the kernels of the code objects: 40 k_pass; 82 / 82 / 82 / 110 / 74 / 74 / 37 / 37 k_pass2 at 1, 2, 3, 4, 6, 8, 12, 16 labels per lane; 42 k_pass_rel
    assert (per(full, M.FIRST), per(full, M.SECOND), per(full, M.REL)) == (40, 82 * 3 + 110 + 74 * 2 + 37 * 2, 42)
    assert dev < full and all(c[M.CHOICE.index("XCDQ")] or c[M.CHOICE.index("W2")] for c in full - dev)  # a development build: no queue, no W2 instances
    rows, out = swept["dense"]
    isdev = rows[:, DENSE_FIELDS.index("devtools")] != 0
    chosen, chosen_dev = bare(out[~isdev, len(DENSE_PLAN):]), bare(out[isdev, len(DENSE_PLAN):])
    chosen |= bare(swept["rel"][1][:, len(REL_PLAN):])
    assert chosen - {M.choice(M.REFUSE)} <= full and chosen_dev - {M.choice(M.REFUSE)} <= dev
    # every instance is some swept request's choice: no list of exceptions is needed -- what the parent's refusal arms guarded
    # (queues with several volumes per wave, two-byte costs without deep rings, weights beyond 512 labels) were never instances
    missing = full - chosen
    assert not missing, sorted(M.name(c) for c in missing)[:20]
    missing = {c for c in dev if c[0] != M.REL} - chosen_dev  # (the development build is the dense kernels')
    assert not missing, sorted(M.name(c) for c in missing)[:20]
    print("dense requests swept: %d, range-proportional: %d; instances reached: %d of %d" % (len(rows), len(swept["rel"][0]), len(full & chosen), len(full)))


def test_names(lib):
    buf = C.create_string_buffer(128)
    named = [(M.choice(M.SECOND, LPL=4, FH=1, WEIGHTED=0, MGM=2, C8=1, SUBV=1, DEEP=1, XCDQ=1, ONEB=1, W2=0), "k_pass2<4, true, false, 2, 1, 1, true, true, true, false>"),
             (M.choice(M.FIRST, LPL=16, FH=0, WEIGHTED=1, R=4), "k_pass<16, false, true, 4>"),
             (M.choice(M.REL, FH=1, PUBE=0, NK=3, SPL=4, CB=1, FH2=0), "k_pass_rel<true, false, 3, 4, 1, false>"), (M.choice(M.REFUSE), "refused")]
    for c, want in named:
        n = lib.pass_kernel_name_of((C.c_int * NC)(*c), buf, len(buf))
        assert (buf.value.decode(), n) == (want, len(want)) and M.name(c) == want


# ---- what the route can ask for is never refused ----------------------------------------------------------------------------------
def test_no_request_of_plan_dense_kernels_is_refused(lib):
    """The rows of tests/test_route_plan.py's dense table, through plan_dense_kernels (its model: that test holds the two equal) to the
    request run_passes fills from the decision, to the kernel choice -- at three sizes, both build kinds, with and without queues."""
    import test_route_plan as TR
    seen = set()
    ns = (1, 2, 4, 16)  # (one volume, the fewest that share a wave at 128 and at 64 labels, the most)
    for (q, words, facts, pad), _, _ in itertools.chain(TR.dense_sweep(TR.DENSE_VARIANTS, ns=ns), TR.dense_sweep(TR.DENSE_PER_VOLUME, ns=ns, labels=TR.PER_VOLUME_LABELS)):
        d = dict(zip(RM.DENSE_OUT, RM.dense_kernels(q, words, facts, pad)[0]))
        if d["err"] or d["exact"]:
            continue
        wmode = (2 if d["w2cand"] else 1) if d["weighted"] else 0
        seen.add((d["L"], q["nb"], q["MGM"], q["fh"], wmode, d["use_c8"], d["cb"], d["first_build"], d["ragged"], q["sw_deep"]))
    assert len(seen) > 1000
    cols = {f: [s[k] for s in seen] for k, f in enumerate("L nb MGM fh wmode use_c8 cb first_build ragged deep".split())}
    for (nx, ny), dev, xcc in itertools.product(SIZES[:2], (0, 1), (0xff, 0)):
        out = call_threads(lib.pass_kernel_dense, dense_requests(lib, cols, nx=nx, ny=ny, devtools=dev, xcc_mask=xcc), len(DENSE_PLAN) + NC)
        assert not np.any(out[:, 0]) and np.all(out[:, len(DENSE_PLAN)] != M.REFUSE)


def test_no_request_plan_agg_route_sends_to_the_range_proportional_kernels_is_refused(lib):
    """The (128 slots, 4 bytes, FH2) promise of plan_agg_route, which the launcher's refusal arm relied on."""
    import test_route_plan as TR
    seen = set()
    for q, weights, vols in TR.route_sweep():
        (route, rel_weighted), _ = RM.agg_route(q, weights, vols)
        if route == RM.REL:
            seen.add((q["fh"], q["MGM"], rel_weighted, vols[0][1], vols[0][2], min(q["n"], 2)))
    assert {(s[3], s[4]) for s in seen} == {(64, 1), (64, 2), (64, 4), (128, 1), (128, 2), (128, 4)} and any(s[0] and s[1] == 2 and not s[2] for s in seen)
    rows = [rel_request(fh=fh, MGM=MGM, weighted=w, slots=slots, cb=cb, nb=nb, rel_multi=multi) for fh, MGM, w, slots, cb, nb in seen for multi in (0, 1)]
    out = call(lib.pass_kernel_rel, rows, len(REL_PLAN) + NC)
    assert not np.any(out[:, 0]) and np.all(out[:, len(REL_PLAN)] == M.REL)


# ---- the sanitizer run -----------------------------------------------------------------------------------------------------------
def test_the_harness_alone_under_the_sanitizers(lib, swept, tmp_path):
    """tests/pass_kernel_harness.cc with its own main, built with -fsanitize=address,undefined, over the corner requests of the sweeps:
    clean, and the same answers as the library gave."""
    exe = str(tmp_path / "pass_kernel_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DPASS_KERNEL_MAIN", "-Wall", "-Werror", "-I", CSRC,
                    HARNESS, "-o", exe], check=True)
    (d, od), (r, orl) = swept["dense"], swept["rel"]
    # corners: the first and last request of the sweep, every refusal kind, the largest launches, and one request per distinct choice
    pick = lambda out, skip: sorted({0, len(out) - 1} | set(np.unique(out[:, skip:], axis=0, return_index=True)[1].tolist()) | set(np.unique(out[:, 0], return_index=True)[1].tolist()))
    di, ri = pick(od, len(DENSE_PLAN)), pick(orl, len(REL_PLAN))
    di = sorted(set(di) | {int(k) for k in np.flatnonzero((d[:, 0] == 1920) & (d[:, DENSE_FIELDS.index("nb")] == 12))[:8]})
    req = tmp_path / "requests.bin"
    with open(req, "wb") as f:
        f.write(np.array([len(di), len(ri)], dtype=np.int32).tobytes() + d[di].tobytes() + r[ri].tobytes())
    run = subprocess.run([exe, str(req)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(di) + len(ri)
    for line, want in zip(lines, od[di].tolist() + orl[ri].tolist()):
        ints, nm = line.split(" ", len(want))[:len(want)], line.split(" ", len(want))[-1]
        assert [int(x) for x in ints] == want and nm == M.name(tuple(want[-NC:])), (line, want)
