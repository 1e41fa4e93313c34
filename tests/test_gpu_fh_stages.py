"""Every stage of the FH min-convolution (fh_scan: the log-step guess, fh_careful, fh_repair, the plain sweeps;
mgm_pass_common.h) on the device, in every pass kernel family that runs it: cost volumes crafted so that the slabs a run
convolves end in a chosen stage (tests/fh_stage_model.py: the classes, the case tables and the floors; tests/test_fh_stages.py
measures them on the CPU), held to the oracle bit for bit -- the Lr of every pass, S, the cost map, the labels, and the vfit
maps -- twice on one context (the hand-off tags alternate), with the instance read back and asserted.

Every input is valid for the reference and inside the hand-off's premise: costs >= +0, finite or +INF, a finite cost in every
pixel, no NaN, finite penalties > 0 with P2 >= P1 (or +INF), weights > 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fh_stage_model as fm
import mgm_amd
from helpers import labels_equal, ndiff
from oracle.oracle import int_ranges, usable_cpus

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DMIN = fm.DMIN
BAND = 15  # lines per band of k_pass2 up to 256 labels
# (family, labels per lane, label ranges per wave) the cases are named for: every case asserts the instance it ran on against its
# own entry, so this set is reached whenever the file's tests pass, in whatever selection or order they run.  "k_pass2 fh2_ragged":
# k_pass2 on a ragged volume kept on its dense hull with TSGM 2 and no weights, where combine_fh2_ragged runs (mgm_pass2.hip:789-790)
DECLARED = ({("k_pass2", lpl, 1) for lpl in (1, 2, 3, 4, 6, 8, 12, 16)} | {("k_pass2", 4, 2), ("k_pass2", 4, 4)}
            | {("k_pass", lpl, 1) for lpl in (4, 12, 24, 32)} | {("k_pass_rel", 4, 4), ("k_pass_rel", 8, 4)}
            | {("k_pass2 fh2_ragged", 1, 1), ("k_pass2 fh2_ragged", 4, 1)})


def named_for(c):
    return (c["family"] + (" fh2_ragged" if c.get("rel") == "0" else ""), c["lpl"], c["groups"])


def parse_instance(s):
    """'k_pass2<4, true, ...>' -> (family, labels per lane, label ranges per wave, FH or None where it is a run-time value)"""
    family = s.split("<")[0]
    a = [x.strip() for x in s[s.index("<") + 1:s.rindex(">")].split(",")]
    if family == "k_pass2":
        return family, int(a[0]), int(a[5]), a[1] == "true"
    if family == "k_pass":
        return family, int(a[0]), 1, None
    if family == "k_pass_rel":
        return family, int(a[3]), 4, a[0] == "true"
    return family, None, None, None


def many_threads(oracle):
    oracle.set_threads(min(16, usable_cpus()))


def check_dense(ctx, oracle, c):
    """One dense case on `ctx` -> its instance.  Floors first (on the oracle's Lr), then two identical calls and one with vfit."""
    volumes, w8h = fm.case_volumes(c), fm.case_weights(c)
    P1, P2, NDIR, MGM = c["P1"], c["P1"] * c["P2f"], c["NDIR"], c["MGM"]
    many_threads(oracle)
    try:
        refs = [oracle.mgm(C, DMIN, P1, P2, NDIR, MGM, 1, 1, w8h, dump_lr=True) for C in volumes]
        by_stage, long_ = fm.dense_counts_from_lr(c, [r[3] for r in refs], w8h)
        print(c["name"], "fwd", by_stage[0], "bwd", by_stage[1], "long", long_)
        assert not fm.floors_met(c, by_stage, long_), c["name"]
        fits = [oracle.refine(S, DMIN, "vfit", np.where(np.isfinite(oc), o, DMIN), oc) for S, o, oc, _ in refs]
    finally:
        oracle.set_threads(1)
    if c["row"] is not None:  # several bands per pass whichever way its lines run, the stragglers' row inside a band's middle
        assert min(c["nx"], c["ny"]) > 2 * BAND and c["L"] <= 256 and c["row"] % BAND not in (0, BAND - 1), c["name"]
    cvs = [ctx.upload_volume(C, DMIN) for C in volumes]
    w8 = ctx.upload_image(w8h) if w8h is not None else None
    w8s = [w8] * len(cvs) if w8 is not None else None
    instance = None
    for turn in (0, 1):
        Ss, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, 1, 1, w8s, None, want_S=True)
        instance = ctx.last_pass_kernel()
        for p in range(NDIR):  # (of the call's FIRST volume: mgm_debug_download_lr reads no other; the others through S)
            assert ndiff(ctx.debug_lr(cvs[0], p), refs[0][3][p]) == 0, (c["name"], turn, "Lr of pass %d" % p)
        for k, (S, o, oc, _) in enumerate(refs):
            go, gc = outs[k].download()[0], outcs[k].download()[0]
            assert ndiff(Ss[k].download(), S) == 0, (c["name"], turn, k, "S")
            assert ndiff(gc, oc) == 0 and labels_equal(go, o, oc), (c["name"], turn, k, "maps")
        for h in Ss + outs + outcs:
            h.free()
    _, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, 1, 1, w8s, "vfit")
    for k, (ro, rc) in enumerate(fits):
        go, gc = outs[k].download()[0], outcs[k].download()[0]
        fin = np.isfinite(refs[k][2])
        assert ndiff(gc, rc) == 0 and ndiff(go[fin], ro[fin]) == 0, (c["name"], k, "vfit")
    for h in cvs + outs + outcs + ([w8] if w8 is not None else []):
        h.free()
    print(c["name"], instance)
    family, lpl, groups, fh = parse_instance(instance)
    assert (family, lpl, groups) == (c["family"], c["lpl"], c["groups"]) and fh in (None, True), (c["name"], instance)
    args = [x.strip() for x in instance[instance.index("<") + 1:-1].split(",")]
    assert all(args[i] == v for i, v in c["flags"]), (c["name"], instance, c["flags"])  # (k_pass2<LPL, FH, WEIGHTED, MGM, C8, SUBV, DEEP, XCDQ, ONEB, W2>)
    return instance


IN_PROCESS = [c for c in fm.DENSE_CASES if not c["env"]]
IN_CHILD = [c for c in fm.DENSE_CASES if c["env"]]


@pytest.mark.parametrize("c", IN_PROCESS, ids=lambda c: c["name"])
def test_dense_case(ctx, oracle, c):
    if c["fresh"]:  # a default context of its own (the first build's cases)
        with mgm_amd.Context(0) as own:
            instance = check_dense(own, oracle, c)
    else:
        instance = check_dense(ctx, oracle, c)
    assert parse_instance(instance)[:3] == named_for(c)


CHILD = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import mgm_amd
import fh_stage_model as fm
from oracle.oracle import Oracle
from test_gpu_fh_stages import check_dense
oracle = Oracle(threads=1)
with mgm_amd.Context(0) as own:
    for c in fm.DENSE_CASES:
        if c["name"] in sys.argv[1:]:
            print("RAN", c["name"], check_dense(own, oracle, c).replace(" ", ""))
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_first_build_by_switch_in_a_child_process():
    """MGM_HIP_PASS_BUILD=1 (the first build, k_pass, at a label count the second build would take) set for a fresh child only."""
    names = [c["name"] for c in IN_CHILD]
    envs = {tuple(sorted(c["env"].items())) for c in IN_CHILD}
    assert len(envs) == 1
    r = subprocess.run([sys.executable, "-c", CHILD] + names, env=dict(os.environ, **dict(envs.pop())), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    ran = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("RAN "))
    assert sorted(ran) == sorted(names), r.stdout[-2000:]
    for c in IN_CHILD:
        assert parse_instance(ran[c["name"]])[:3] == named_for(c), (c["name"], ran[c["name"]])


# ---- k_pass_rel: ragged ranges ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fm.REL_CASES, ids=lambda c: c["name"])
def test_ragged_case(ctx, oracle, c):
    u, v, lo, hi = fm.rel_case_inputs(c)
    ilo, ihi = int_ranges(lo, hi)
    dmin, dmax = c["hull"]
    L = dmax - dmin + 1
    P1, P2, NDIR, MGM = c["P1"], c["P1"] * c["P2f"], c["NDIR"], c["MGM"]
    w8h = fm.case_weights(c)
    d = dmin + np.arange(L)[None, None, :]
    own = (d >= ilo[..., None]) & (d <= ihi[..., None])
    many_threads(oracle)
    try:
        C = oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, "none", "ad", np.inf, 5)
        S, o, oc, lr = oracle.mgm_ranged(C, dmin, ilo, ihi, P1, P2, NDIR, MGM, 1, 1, w8h, dump_lr=True)
        ro, rc = oracle.refine_ranged(S, dmin, ilo, ihi, "vfit", o, oc)
        by_stage, long_, mixed = fm.rel_case_counts(c, lr, ilo, ihi, w8h)
    finally:
        oracle.set_threads(1)
    print(c["name"], "fwd", by_stage[0], "bwd", by_stage[1], "long", long_, "mixed pixels", mixed)
    assert not fm.rel_floors_met(c, by_stage, long_, mixed), c["name"]
    before = os.environ.get("MGM_HIP_REL")
    os.environ["MGM_HIP_REL"] = c["rel"]  # ("2": the range-proportional kernels whatever the image size; "0": the dense hull)
    try:
        cv = ctx.costvolume(u, v, lo, hi, "none", "ad", float("inf"), 5)
        assert cv.dims == (c["nx"], c["ny"], dmin, dmax)
        w8 = ctx.upload_image(w8h) if w8h is not None else None
        for turn in (0, 1):
            Sg, go, gc = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, 1, 1, w8, None, want_S=True)
            instance = ctx.last_pass_kernel()
            for p in range(NDIR):
                n = int(np.sum((ctx.debug_lr(cv, p).view(np.uint32) != lr[p].view(np.uint32)) & own))
                assert n == 0, (c["name"], turn, "Lr of pass %d" % p, n)
            n = int(np.sum((Sg.download().view(np.uint32) != S.view(np.uint32)) & own))
            assert n == 0, (c["name"], turn, "S", n)
            assert ndiff(gc.download()[0], oc) == 0 and labels_equal(go.download()[0], o, oc), (c["name"], turn, "maps")
            for h in (Sg, go, gc):
                h.free()
        _, go, gc = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, 1, 1, w8, "vfit")
        fin = np.isfinite(oc)
        assert ndiff(gc.download()[0], rc) == 0 and ndiff(go.download()[0][fin], ro[fin]) == 0, (c["name"], "vfit")
        for h in (cv, go, gc) + ((w8,) if w8 is not None else ()):
            h.free()
    finally:
        if before is None:
            os.environ.pop("MGM_HIP_REL", None)
        else:
            os.environ["MGM_HIP_REL"] = before
    print(c["name"], instance)
    family, lpl, groups, fh = parse_instance(instance)
    assert (family, lpl, groups, fh) == (c["family"], c["lpl"], c["groups"], True), (c["name"], instance)
    a = [x.strip() for x in instance[instance.index("<") + 1:-1].split(",")]
    if c["rel"] == "2":
        assert int(a[2]) == MGM and (a[5] == "true") == (MGM == 2 and w8h is None), (c["name"], instance)  # side by side; FH2
    else:  # the dense hull: FH on a ragged volume borrows the weighted kernels with planes of ones; TSGM 2 there is combine_fh2_ragged
        assert a[2] == "true" and int(a[3]) == MGM == 2 and w8h is None, (c["name"], instance)


def test_the_declared_instances_are_those_the_cases_are_named_for():
    """Every case above asserts the instance it ran on against named_for(case); this is the list a reader can rely on."""
    assert {named_for(c) for c in fm.DENSE_CASES + fm.REL_CASES} == DECLARED
