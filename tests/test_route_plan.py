"""plan_agg_route, plan_subbatch / shrink_after_nomem and plan_dense_kernels (mgm_amd/csrc/mgm_planner.h) on the host: which kernels
take an aggregation call, and in which sub-batches, is what aggregate_batch_now and resolve_dense_operands decided before the
planners existed (tests/route_plan_model.py: their control flow at commit 5fa7fa3, with the device probes as logging callbacks) --
the same decision AND the same probes in the same order; the cases the comments name come out literally; the chunks cover a batch
exactly once; a decision is a function of the request's bytes alone; every `need` and every refusal is reached."""
import ctypes as C
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

import route_plan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgm_amd", "csrc")
KB = 16       # kMaxBatch
MAXLOG = 24   # route_plan_harness.cc
NS = (1, 2, 3, 4, 5, 16)
LABELS = (63, 64, 100, 151, 256, 257, 512, 513, 768, 1024, 2048, 2049)
# the weights' kinds: (given, (some value != 1, some not positive and finite, the values != 1 are one value)) per volume
WEIGHTS = dict(none=(0, (0, 0, 0)), ones=(1, (0, 0, 0)), two=(1, (1, 0, 1)), general=(1, (1, 0, 0)), odd=(1, (1, 1, 0)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("routeplan") / "libroute_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "route_plan_harness.cc"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    assert lib.route_request_bytes() == 4 * (len(M.ROUTE_FIELDS) + 3 * KB)
    assert lib.dense_kernels_request_bytes() == 4 * len(dense_flat(*dense_case(1, 64))[0])
    assert lib.subbatch_request_bytes() == 8 * 3 + 4 * 8
    return lib


def pad16(xs, fill):
    return list(xs) + [fill] * (KB - len(xs))


def drive(lib, fn, nout, reqs, facts):
    """[(decision, probes)] of the harness's ask-loop over requests whose device facts are -1 and the tables that hold them."""
    a, f = np.ascontiguousarray(reqs, dtype=np.int32), np.ascontiguousarray(facts, dtype=np.int32)
    out = np.zeros((len(a), nout + 1 + 2 * MAXLOG), dtype=np.int32)
    fn(a.ctypes.data_as(C.c_void_p), f.ctypes.data_as(C.c_void_p), C.c_int(len(a)), out.ctypes.data_as(C.c_void_p))
    res = []
    for r in out.tolist():
        assert 0 <= r[nout] <= MAXLOG, r
        res.append((tuple(r[:nout]), [(r[nout + 1 + 2 * k], r[nout + 2 + 2 * k]) for k in range(r[nout])]))
    return res


# ---- rel against dense --------------------------------------------------------------------------------------------------------
def route_case(n, fh=0, MGM=3, wkind="none", p1neg=0, p2neg=0, p2inf=0, want_S=0, only_rel=0, rel=None, wvol=None, **sw):
    """(q, weights, rel) for the model: a call of n volumes whose range-proportional copies are usable in the 64-slot one-byte form."""
    q = dict(n=n, MGM=MGM, fh=fh, want_S=want_S, weights_given=WEIGHTS[wkind][0], p1_nonneg=1 - p1neg, p2_nonneg=1 - p2neg, p2_finite=1 - p2inf,
             only_rel=only_rel, rel_enabled=1, sw_rel=1, sw_rel_tie=1, sw_rel_S=1, sw_rel_fh2=1)
    for k, v in sw.items():
        assert k in q, k
        q[k] = v
    words = [WEIGHTS[wkind][1]] * n
    if wvol:  # (volume, kind): that volume's weights are of another kind
        words = list(words)
        words[min(wvol[0], n - 1)] = WEIGHTS[wvol[1]][1]
    weights = (int(any(w[1] for w in words)), int(any(w[0] for w in words)))
    vols = [(1, 64, 1)] * n
    for v, fact in (rel or {}).items():  # volume ("first" / "mid" / "last" / "all") -> (usable, slots, cb)
        for k in {"first": [0], "mid": [n // 2], "last": [n - 1], "all": range(n)}[v]:
            vols = list(vols)
            vols[k] = fact
    return q, weights, vols


def route_flat(q, weights, vols):
    head = [q[f] for f in M.ROUTE_FIELDS[:-2]]
    cols = [pad16([v[k] for v in vols], -1) for k in range(3)]
    return head + [-1, -1] + [-1] * (3 * KB), head + list(weights) + cols[0] + cols[1] + cols[2]


ROUTE_VARIANTS = [dict()] + [dict([kv]) for kv in (("rel_enabled", 0), ("sw_rel", 0), ("sw_rel", 2), ("sw_rel_tie", 0), ("sw_rel_S", 0), ("sw_rel_fh2", 0))]
ROUTE_VARIANTS += [dict(rel={"all": f}) for f in ((1, 128, 4), (1, 128, 1), (1, 64, 2), (1, 128, 2), (1, 64, 4), (0, 64, 1))]
ROUTE_VARIANTS += [dict(rel={"all": (1, 128, 4), p: f}) for p in ("first", "mid", "last") for f in ((0, 128, 4), (1, 64, 4), (1, 128, 2))]
ROUTE_VARIANTS += [dict(wvol=(p, k)) for p in (0, 7, 15) for k in ("ones", "odd")]


P2_STATES = ((0, 0), (1, 0), (0, 1))  # (P2 < 0, P2 = +INF): positive and finite, negative, +INF


def route_sweep():
    cross = list(itertools.product(NS, (0, 1), (1, 2, 3, 4), WEIGHTS, (0, 1), P2_STATES, (0, 1), (0, 1)))
    for var in ROUTE_VARIANTS:
        for n, fh, MGM, wk, p1neg, (p2neg, p2inf), want_S, only_rel in cross:
            if "wvol" in var and wk == "none":
                continue
            yield route_case(n, fh, MGM, wk, p1neg, p2neg, p2inf, want_S, only_rel, **var)


def check_route(lib, cases, reached=None):
    flat = [route_flat(*c) for c in cases]
    got = drive(lib, lib.route_drive, 2, [a for a, _ in flat], [b for _, b in flat])
    for c, g in zip(cases, got):
        want = M.agg_route(*c)
        assert g == want, (c, g, want)
        if reached is not None:
            reached["need"] |= {n for n, _ in g[1]}
            reached["route"].add(g[0][0])
    return got


@pytest.fixture(scope="module")
def reached():
    return dict(need=set(), route=set(), err=set())


def test_route_sweep_decides_and_probes_as_the_parent(lib, reached):
    cases = list(route_sweep())
    assert len(cases) > 150000
    check_route(lib, cases, reached)


def test_route_named_cases(lib):
    W, R = M.NEED_WEIGHTS, M.NEED_REL
    named = [
        ("FH on usable copies", route_case(1, fh=1), (M.REL, 0), [(R, 0)]),
        ("a batch: every volume is asked for, in order", route_case(3), (M.REL, 0), [(R, 0), (R, 1), (R, 2)]),
        ("... up to the first that is not usable", route_case(4, rel={"mid": (0, 64, 1)}), (M.DENSE, 0), [(R, 0), (R, 1), (R, 2)]),
        ("... or has another format", route_case(4, rel={"first": (1, 128, 1)}), (M.DENSE, 0), [(R, 0), (R, 1)]),
        ("weights are scanned before any copy is resolved", route_case(2, wkind="two"), (M.REL, 1), [(W, 0), (R, 0), (R, 1)]),
        ("odd weights: the dense kernels, no copy resolved", route_case(2, wkind="odd"), (M.DENSE, 0), [(W, 0)]),
        ("negative P1: no candidate, nothing is probed", route_case(2, wkind="two", p1neg=1), (M.DENSE, 0), []),
        ("P2 = +INF: no candidate", route_case(1, fh=1, p2inf=1), (M.DENSE, 0), []),
        ("MGM_HIP_REL=0", route_case(1, fh=1, rel_enabled=0), (M.DENSE, 0), []),
        ("S wanted is served from the copies", route_case(1, fh=1, want_S=1), (M.REL, 0), [(R, 0)]),
        ("... not with rel_S=0", route_case(1, fh=1, want_S=1, sw_rel_S=0), (M.DENSE, 0), []),
        ("one unit-weight Hirschmueller volume with rel_tie=0 keeps the hull", route_case(1, sw_rel_tie=0), (M.DENSE, 0), []),
        ("... unless its only copy is the range-proportional one", route_case(1, sw_rel_tie=0, only_rel=1), (M.REL, 0), [(R, 0)]),
        ("TSGM 2 with planes of ones runs UNWEIGHTED on rel", route_case(1, MGM=2, wkind="ones"), (M.REL, 0), [(W, 0), (R, 0)]),
        ("TSGM 3 with planes of ones runs weighted", route_case(1, MGM=3, wkind="ones"), (M.REL, 1), [(W, 0), (R, 0)]),
        ("TSGM 2 FH without weights: k_pass_rel FH2", route_case(1, fh=1, MGM=2), (M.REL, 0), [(R, 0)]),
        ("... not with rel_fh2=0", route_case(1, fh=1, MGM=2, sw_rel_fh2=0), (M.DENSE, 0), []),
        ("the 128-slot fp32 FH2 exception: the hull, after the copy was resolved", route_case(1, fh=1, MGM=2, rel={"all": (1, 128, 4)}), (M.DENSE, 0), [(R, 0)]),
        ("... with planes of ones as well", route_case(1, fh=1, MGM=2, wkind="ones", rel={"all": (1, 128, 4)}), (M.DENSE, 0), [(W, 0), (R, 0)]),
        ("... but not with real weights", route_case(1, fh=1, MGM=2, wkind="two", rel={"all": (1, 128, 4)}), (M.REL, 1), [(W, 0), (R, 0)]),
        ("... nor with two-byte costs", route_case(1, fh=1, MGM=2, rel={"all": (1, 128, 2)}), (M.REL, 0), [(R, 0)]),
    ]
    got = check_route(lib, [c for _, c, _, _ in named])
    for (what, _, dec, log), g in zip(named, got):
        assert g == (dec, log), (what, g)


# ---- sub-batches --------------------------------------------------------------------------------------------------------------
def sub_flat(route, n, npix, L, rel_slots, NDIR, ws_limit, lr_pad, want_S, ridx, prune):
    return (npix, ws_limit, lr_pad, route, n, NDIR, L, rel_slots, want_S, ridx, prune)


def ask_sub(lib, rows):
    t = np.dtype([(f, "<i8" if f in ("npix", "ws_limit", "lr_pad") else "<i4") for f in M.SUB_FIELDS])
    req = np.zeros(len(rows), dtype=t)
    a = np.array([sub_flat(*r) for r in rows], dtype=np.int64)
    for k, f in enumerate(M.SUB_FIELDS):
        req[f] = a[:, k]
    out = np.zeros(len(rows), dtype=np.int32)
    lib.subbatch_plan(req.ctypes.data_as(C.c_void_p), C.c_int(len(rows)), out.ctypes.data_as(C.c_void_p))
    return out.tolist()


def test_subbatches(lib):
    npix, NDIR, lr_pad = 150 * 110, 8, 67 * 64
    rows = []
    for route, (L, slots) in itertools.product((M.DENSE, M.REL), ((256, 64), (128, 128), (151, 64), (2049, 128))):
        vol = 4 * npix * (slots if route == M.REL else (M.padded_labels(L) or L)) * NDIR  # one volume's Lr bytes, without the allowances
        for n, quarter in itertools.product(range(1, 17), range(0, 17 * 4 + 1)):
            for want_S, ridx, prune in ((0, 1, 1), (0, 1, 0), (1, 1, 1), (0, 2, 1)):  # the minima term on, and off three ways
                rows.append((route, n, npix, L, slots, NDIR, vol * quarter // 4, lr_pad, want_S, ridx, prune))
    got = ask_sub(lib, rows)
    seen = set()
    for r, g in zip(rows, got):
        assert g == M.subbatch(*r), (r, g)
        assert 1 <= g <= r[1], (r, g)
        if r[6]:  # (under a workspace limit)
            seen.add((r[0], g))
        # the launches of the batch if every size above one volume came back MGM_ERR_NOMEM once: [0, n) exactly once, never an empty chunk
        route, n = r[0], r[1]
        chunk, v0, failed, covered = g, 0, set(), []
        while v0 < n:
            m = min(chunk, n - v0)
            assert m >= 1
            if m > 1 and m not in failed:
                failed.add(m)
                chunk = lib.subbatch_shrink(route, m)
                assert 1 <= chunk < m
                continue
            covered += range(v0, v0 + m)
            v0 += m
        assert covered == list(range(n)), (r, covered)
    assert {g for rt, g in seen if rt == M.REL} == set(range(1, 15))              # rel: no rounding (17 volumes' worth / 1.16 hold 14)
    assert {g for rt, g in seen if rt == M.DENSE} == {1, 2, 4, 8, 12}              # dense (17 / 1.07: 15): multiples of four, else two (3 -> 2, also where three would fit)
    for route, m in itertools.product((M.DENSE, M.REL), range(1, 17)):
        assert lib.subbatch_shrink(route, m) == M.shrink(route, m), (route, m)
    assert [lib.subbatch_shrink(M.DENSE, m) for m in (16, 12, 10, 6, 5, 4, 3, 2)] == [8, 6, 4, 2, 2, 2, 1, 1]  # dense halves stay even above four
    assert [lib.subbatch_shrink(M.REL, m) for m in (16, 12, 10, 6, 5, 4, 3, 2)] == [8, 6, 5, 3, 2, 2, 1, 1]    # rel: plain halves
    # the minima term: 256 labels, a limit between 1.07 and 1.07 + 1/32 volumes' worth per volume
    vol = 4 * (npix * 256 + lr_pad) * NDIR
    on, off = ask_sub(lib, [(M.DENSE, 2, npix, 256, 64, NDIR, int(vol * 2 * 1.09), lr_pad, 0, 1, p) for p in (1, 0)])
    assert (on, off) == (1, 2)


# ---- the dense kernels --------------------------------------------------------------------------------------------------------
def dense_case(nb, Lreal, fh=0, MGM=3, wkind="none", p1neg=0, p2neg=0, p2inf=0, ragged=0, wvol=None, c8=None, p8=None, pad_fits=(0, 1), **kw):
    """(q, weight words, c8 facts, pad facts) for the model: nb volumes with usable one-byte compact copies and no padded copy of their
    own, whose padded copies would fit two-byte costs but not one-byte costs."""
    LP = M.padded_labels(Lreal)
    given = WEIGHTS[wkind][0]
    q = dict(nb=nb, MGM=MGM, fh=fh, allow_pad=1, Lreal=Lreal, p1_nonneg=1 - p1neg, p2_nonneg=1 - p2neg, p2_finite=1 - p2inf, force_build=0,
             lines_real=M.pass2_lines_f32(Lreal), lines_pad=M.pass2_lines_f32(LP) if LP else 0, lpl_real=M.pass_lpl(Lreal), lpl_pad=M.pass_lpl(LP) if LP else 0,
             sw_pad=1, sw_c8=1, sw_deep=-1, weights_given=given, w_given=[given] * nb, ragged=ragged, nan_words=0, same_hull=1,
             p8_valid=[0] * nb, p8_L=[0] * nb, p8_cb=[1] * nb, pad_hint=1)
    for k, v in kw.items():
        assert k in q, k
        q[k] = v
    where = lambda p: {"first": [0], "mid": [nb // 2], "last": [nb - 1], "all": range(nb)}[p]
    words = [WEIGHTS[wkind][1]] * nb
    if wvol:  # (where, kind): that volume's weights are of another kind ("none": it has no weight image)
        for k in where(wvol[0]):
            words[k] = WEIGHTS[wvol[1]][1]
            q["w_given"][k] = WEIGHTS[wvol[1]][0]
        q["weights_given"] = q["w_given"][0]
    facts = [(1, 1, 0)] * nb
    for p, f in (c8 or {}).items():  # where -> (use, cbytes, NaN found)
        for k in where(p):
            facts[k] = f
    for p, f in (p8 or {}).items():  # where -> (valid, label slots or None: the launch's, bytes)
        for k in where(p):
            q["p8_valid"][k], q["p8_L"][k], q["p8_cb"][k] = f[0], (LP if f[1] is None else f[1]), f[2]
    return q, words, facts, {1: pad_fits[0], 2: pad_fits[1]}


def dense_flat(q, words, facts, pad):
    req, tab = [], []
    for f in M.DENSE_FIELDS:
        if f == "pad_fits[3]":
            req += [-1, -1, -1]
            tab += [-1, pad[1], pad[2]]
        elif not f.endswith("[]"):
            req.append(q[f]), tab.append(q[f])
        elif f[:-2] in q:
            req += pad16(q[f[:-2]], 0)
            tab += pad16(q[f[:-2]], 0)
        else:
            src, k = {"w_not_one": (words, 0), "w_odd": (words, 1), "w_one_other": (words, 2), "c8_use": (facts, 0), "c8_bytes": (facts, 1), "nan_found": (facts, 2)}[f[:-2]]
            req += [-1] * KB
            tab += pad16([x[k] for x in src], -1)
    return req, tab


# every switch and every fact that holds for all volumes, flipped one at a time against the whole cross ...
DENSE_VARIANTS = [dict()] + [dict([kv]) for kv in (("allow_pad", 0), ("force_build", 1), ("sw_pad", 0), ("sw_c8", 0), ("sw_deep", 0), ("nan_words", 1), ("same_hull", 0),
                                                   ("pad_hint", 0), ("pad_hint", 2))]
DENSE_VARIANTS += [dict(pad_fits=f) for f in ((1, 1), (0, 0))] + [dict(pad_hint=2, pad_fits=f) for f in ((1, 0), (0, 0))]
DENSE_VARIANTS += [dict(c8={"all": (1, 2, 0)}), dict(c8={"all": (0, 1, 0)}), dict(p8={"all": (1, None, 1)}), dict(p8={"all": (1, None, 2)})]
# ... and the per-volume facts at the first, a middle and the last volume, against the cross at four label counts (one the second
# build takes, two that run padded -- below and above 512 --, one beyond the fast kernels)
DENSE_PER_VOLUME = [dict(c8={p: f}) for p in ("first", "mid", "last") for f in ((0, 1, 0), (1, 2, 0), (1, 1, 1))]
DENSE_PER_VOLUME += [dict(p8={"all": (1, None, 2), p: f}) for p in ("first", "mid", "last") for f in ((0, None, 2), (1, 64, 2), (1, None, 1))]
DENSE_PER_VOLUME += [dict(wvol=(p, k)) for p in ("first", "mid", "last") for k in ("ones", "odd", "none")]
PER_VOLUME_LABELS = (64, 151, 513, 2049)
AT = {f: k for k, f in enumerate(("nb MGM fh allow_pad Lreal p1_nonneg p2_nonneg p2_finite").split())}
AT["ragged"] = 17 + KB  # (behind the 17 scalars in front of w_given[] and that array)


def dense_sweep(variants, ns=NS, labels=LABELS):
    """(case, flat request, flat table) per row.  The volumes' side of a row is built once per (variant, n, weights, labels); the cross
    of the call's flags over it changes scalars only."""
    flags = list(itertools.product((0, 1), (1, 2, 3, 4), (0, 1), P2_STATES, (0, 1)))
    for var in variants:
        for n, L, wk in itertools.product(ns, labels, WEIGHTS):
            if "wvol" in var and wk == "none":
                continue
            q, words, facts, pad = dense_case(n, L, wkind=wk, **var)
            req0, tab0 = dense_flat(q, words, facts, pad)
            for fh, MGM, p1neg, (p2neg, p2inf), ragged in flags:
                upd = dict(fh=fh, MGM=MGM, p1_nonneg=1 - p1neg, p2_nonneg=1 - p2neg, p2_finite=1 - p2inf, ragged=ragged)
                req, tab = req0[:], tab0[:]
                for k, v in upd.items():
                    req[AT[k]] = tab[AT[k]] = v
                yield (dict(q, **upd), words, facts, pad), req, tab


def check_dense(lib, rows, reached=None):
    got = drive(lib, lib.dense_kernels_drive, len(M.DENSE_OUT), [a for _, a, _ in rows], [b for _, _, b in rows])
    for (c, _, _), g in zip(rows, got):
        want = M.dense_kernels(*c)
        assert g == want, (c, dict(zip(M.DENSE_OUT, g[0])), g[1], dict(zip(M.DENSE_OUT, want[0])), want[1])
        if reached is not None:
            reached["need"] |= {n for n, _ in g[1]}
            reached["err"].add(g[0][0])
    return got


@pytest.mark.parametrize("part", range(4))
def test_dense_sweep_decides_and_probes_as_the_parent(lib, reached, part):
    """The whole cross at every batch size against every switch (a quarter of the variants per case); the per-volume facts likewise."""
    rows = list(dense_sweep(DENSE_VARIANTS[part::4])) + list(dense_sweep(DENSE_PER_VOLUME[part::4], labels=PER_VOLUME_LABELS))
    assert len(rows) > 150000
    check_dense(lib, rows, reached)


def test_dense_named_cases(lib):
    W, K, P = M.NEED_WEIGHTS, M.NEED_C8, M.NEED_PAD
    out = lambda **kw: tuple(dict(dict(zip(M.DENSE_OUT, (0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, -1))), **kw)[k] for k in M.DENSE_OUT)
    named = [
        ("64 labels: the second build on the volume's compact copy", dense_case(1, 64), out(L=64), [(K, 0)]),
        ("100 labels: padded, one byte fits at the first try", dense_case(1, 100, pad_fits=(1, 1)), out(L=128, padded=1, pad_hint=1), [(K, 0), (P, 1)]),
        ("151 labels: two bytes are tried after one byte failed", dense_case(1, 151), out(L=192, padded=1, cb=2, pad_hint=2), [(K, 0), (P, 1), (P, 2)]),
        ("... and first where they fitted last time", dense_case(1, 151, pad_hint=2), out(L=192, padded=1, cb=2, pad_hint=2), [(K, 0), (P, 2)]),
        ("... neither fits: fp32 padded copies, and no try next time", dense_case(1, 151, pad_fits=(0, 0)), out(L=192, padded=1, use_c8=0, need_pad_f32=1, pad_hint=0),
         [(K, 0), (P, 1), (P, 2)]),
        ("... no try after that", dense_case(1, 151, pad_hint=0), out(L=192, padded=1, use_c8=0, need_pad_f32=1, pad_hint=0), [(K, 0)]),
        ("the cost kernel's own padded two-byte copies: nothing to pad", dense_case(2, 151, p8={"all": (1, None, 2)}), out(L=192, padded=1, own_padded=1, cb=2),
         [(K, 0), (K, 1)]),
        ("two-byte costs with weights fall back to fp32 and drop own_padded", dense_case(1, 151, wkind="two", p8={"all": (1, None, 2)}),
         out(L=192, padded=1, use_c8=0, cb=2, weighted=1, weighted_given=1, w2cand=1, need_pad_f32=1), [(W, 0), (K, 0)]),
        ("... unpadded: the fp32 volume", dense_case(1, 128, wkind="general", c8={"all": (1, 2, 0)}), out(L=128, use_c8=0, cb=2, weighted=1, weighted_given=1),
         [(W, 0), (K, 0)]),
        ("more than 512 labels with weights take no padding", dense_case(1, 513, wkind="two"), out(L=513, use_c8=0, weighted=1, weighted_given=1, w2cand=1),
         [(W, 0), (K, 0)]),
        ("... without weights they do", dense_case(1, 513, pad_fits=(1, 1)), out(L=768, padded=1, pad_hint=1), [(K, 0), (P, 1)]),
        ("negative P1: the first build, no padding, no compact costs", dense_case(1, 100, p1neg=1), out(first_build=1, L=100, use_c8=0), [(K, 0)]),
        ("ragged FH with P1 < 0 is exact, and never reaches c8_resolve", dense_case(1, 100, fh=1, ragged=1, p1neg=1), out(exact=1, first_build=1, L=100, ragged=1), []),
        ("ragged with P2 = +INF is exact", dense_case(1, 64, ragged=1, p2inf=1), out(exact=1, L=64, ragged=1), []),
        ("ragged FH with an odd weight is exact", dense_case(1, 64, fh=1, ragged=1, wkind="odd"), out(exact=1, L=64, ragged=1, weighted_given=1), [(W, 0)]),
        ("more than 2048 labels are exact", dense_case(1, 2049), out(exact=1, L=2049), []),
        ("a NaN cost, found by the scan of the last volume", dense_case(3, 64, c8={"last": (1, 1, 1)}), out(exact=1, L=64), [(K, 0), (K, 1), (K, 2)]),
        ("ragged FH without weights borrows the weighted kernels", dense_case(1, 64, fh=1, ragged=1), out(L=64, ragged=1, weighted=1, borrow_ones=1), [(K, 0)]),
        ("... TSGM 2: update_cost2_trunclinear of the second build", dense_case(1, 64, fh=1, MGM=2, ragged=1), out(L=64, ragged=1, weighted=1, borrow_ones=1, fh2_ragged=1),
         [(K, 0)]),
        ("refusal: weighted beside unweighted under TSGM 2, after the scan and before any c8_resolve", dense_case(2, 64, MGM=2, wkind="two", wvol=("last", "ones")),
         out(err=M.MIXED_WEIGHTS), [(W, 0)]),
        ("... TSGM 3 runs planes of ones weighted", dense_case(2, 64, wkind="two", wvol=("last", "ones")), out(L=64, weighted=1, weighted_given=1, w2cand=1),
         [(W, 0), (K, 0), (K, 1)]),
        ("refusal: ragged FH volumes with different hulls", dense_case(2, 64, fh=1, ragged=1, same_hull=0), out(err=M.RAGGED_HULLS), []),
        ("refusal: ragged FH TSGM 2 without weights on the first build", dense_case(1, 64, fh=1, MGM=2, ragged=1, force_build=1), out(err=M.FH2_NEEDS_SECOND_BUILD), []),
        ("... or at a label count the second build does not take", dense_case(1, 1025, fh=1, MGM=2, ragged=1), out(err=M.FH2_NEEDS_SECOND_BUILD), []),
    ]
    got = check_dense(lib, [(c,) + dense_flat(*c) for _, c, _, _ in named])
    for (what, _, dec, log), g in zip(named, got):
        assert g == (dec, log), (what, dict(zip(M.DENSE_OUT, g[0])), g[1])


# ---- purity, reachability -----------------------------------------------------------------------------------------------------
def test_a_decision_is_a_function_of_the_request_alone(lib):
    dense = [(a, b) for _, a, b in dense_sweep(DENSE_VARIANTS[:1] + DENSE_PER_VOLUME[-3:], ns=(1, 3, 16), labels=(64, 151, 513))]
    route = [route_flat(*c) for c in itertools.islice(route_sweep(), 0, None, 29)]
    for fn, nout, rows in ((lib.dense_kernels_drive, len(M.DENSE_OUT), dense), (lib.route_drive, 2, route)):
        key = lambda r: (tuple(r[0]), tuple(r[1]))
        first = dict(zip(map(key, rows), drive(lib, fn, nout, [a for a, _ in rows], [b for _, b in rows])))
        shuffled = rows[:]
        random.Random(7).shuffle(shuffled)
        again = drive(lib, fn, nout, [a for a, _ in shuffled], [b for _, b in shuffled])  # the same bytes in another order, behind other requests
        assert all(first[key(r)] == g for r, g in zip(shuffled, again))
        for r in shuffled[:64]:                                                            # ... and one at a time
            assert drive(lib, fn, nout, [r[0]], [r[1]]) == [first[key(r)]]


def test_every_need_and_every_refusal_is_reached(lib, reached):
    """The distinct probes, routes and refusals of the sweeps above (run here if this test was selected alone)."""
    if not (reached["route"] and reached["err"]):
        check_route(lib, list(itertools.islice(route_sweep(), 0, None, 7)), reached)
        check_dense(lib, list(dense_sweep(DENSE_VARIANTS[:1] + DENSE_PER_VOLUME[-9:], ns=(1, 3))), reached)
    assert reached["need"] == {M.NEED_WEIGHTS, M.NEED_REL, M.NEED_C8, M.NEED_PAD}
    assert reached["route"] == {M.DENSE, M.REL}
    assert reached["err"] == {M.OK, M.MIXED_WEIGHTS, M.RAGGED_HULLS, M.FH2_NEEDS_SECOND_BUILD}
