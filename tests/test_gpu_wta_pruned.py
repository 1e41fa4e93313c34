"""The pruned winner search on the device (k_wta_pruned, fed by the chunk minima k_pass2 writes): 256 labels at 96x34 -- three
bands of row lines, seven of column lines -- against the oracle, against the same call under MGM_HIP_WTA_PRUNE=0, with the Lr
volumes unchanged, and with the chunks-loaded counter held to the CPU emulation's count (wta_prune_model.py; the inputs and
seeds are those of tests/test_wta_bound.py, where the emulation is checked to read at most 40 % of the chunks)."""
import os

import numpy as np
import pytest

import wta_prune_model as M
from helpers import ndiff

pytestmark = pytest.mark.gpu

SEED_A, SEED_B, SEED_C = M.SEEDS
FH_P, HI_P = (2.0, 20000.0), (8.0, 32.0)
# name: (dmin, dmax, NDIR, TSGM, FH, refine, seeds of the batch, pruned search expected)
CASES = {
    "fh3_8dir_vfit": (-255, 0, 8, 3, 1, "vfit", (SEED_A,), True),
    "fh3_8dir_none_x3": (-255, 0, 8, 3, 1, None, (SEED_A, SEED_B, SEED_C), True),
    "hirsch3_8dir_vfit_x3": (-255, 0, 8, 3, 0, "vfit", (SEED_A, SEED_B, SEED_C), True),
    "hirsch2_4dir_none": (-255, 0, 4, 2, 0, None, (SEED_A,), True),
    "fh1_4dir_vfit": (-128, 127, 4, 1, 1, "vfit", (SEED_B,), True),
    "hirsch1_8dir_vfit": (-128, 127, 8, 1, 0, "vfit", (SEED_B,), True),
    "fh3_both_sides_none": (-128, 127, 8, 3, 1, None, (SEED_B,), True),
    "fh2_falls_back": (-255, 0, 8, 2, 1, "vfit", (SEED_A,), False),       # slabs travel with their minimum: no chunk minima
    "padded_200_falls_back": (-199, 0, 8, 3, 1, "vfit", (SEED_A,), False),  # runs padded to 256 label slots
    "constant_pair": (-255, 0, 8, 3, 1, "vfit", ("constant",), True),
}


def pairs_of(spec):
    return [M.constant_pair() if s == "constant" else M.textured_pair(spec[0], spec[1], s) for s in spec[6]]


_ref = {}


def reference(oracle, case, spec):
    """Per volume of the batch: the oracle's (label map, cost map) after the case's refinement and the emulation's chunk count."""
    if case not in _ref:
        dmin, dmax, NDIR, MGM, FH, refine, _, _ = spec
        P1, P2 = FH_P if FH else HI_P
        res = []
        for u, v in pairs_of(spec):
            C = oracle.costvolume(u, v, dmin, dmax, "none", "census", np.inf, 5)
            S, out, outc, lr = oracle.mgm(C, dmin, P1, P2, NDIR, MGM, FH, 1, dump_lr=True)
            if refine:
                out, outc = oracle.refine(S, dmin, refine, out, outc)
            chunks = M.pruned_search(C, lr, dmin, 1)[2] if (dmax - dmin + 1) % M.CHUNK == 0 else 0
            res.append((out, outc, chunks))
        _ref[case] = res
    return _ref[case]


def run(ctx, cvs, spec, prune):
    """One aggregation call under MGM_HIP_WTA_PRUNE=prune: maps, every Lr volume of volume 0, the counters, kernels that ran."""
    dmin, dmax, NDIR, MGM, FH, refine, _, _ = spec
    P1, P2 = FH_P if FH else HI_P
    old = os.environ.get("MGM_HIP_WTA_PRUNE")
    os.environ["MGM_HIP_WTA_PRUNE"] = "1" if prune else "0"
    try:
        ctx.timing(True)
        ctx.timing_reset()
        if len(cvs) == 1:
            _, o, c = ctx.aggregate_dev(cvs[0], P1, P2, NDIR, MGM, FH, 1, None, refine)
            outs, outcs = [o], [c]
        else:
            _, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, FH, 1, None, refine)
        stats = ctx.wta_stats()
        names = [n for n, _ in ctx.timings()]
        ctx.timing(False)
        lr = [ctx.debug_lr(cvs[0], p) for p in range(NDIR)]
        maps = [(o.download()[0], c.download()[0]) for o, c in zip(outs, outcs)]
        for h in outs + outcs:
            h.free()
    finally:
        if old is None:
            del os.environ["MGM_HIP_WTA_PRUNE"]
        else:
            os.environ["MGM_HIP_WTA_PRUNE"] = old
    return maps, lr, stats, names


def check(ctx, oracle, case, spec, cvs):
    dmin, dmax, NDIR, MGM, FH, refine, seeds, pruned = spec
    ref = reference(oracle, case, spec)
    maps1, lr1, (px, ch), names1 = run(ctx, cvs, spec, True)
    maps0, lr0, stats0, names0 = run(ctx, cvs, spec, False)
    assert "k_wta" in names1 and "k_wta" in names0 and "k_pass2" in names1
    for b in range(len(cvs)):
        assert ndiff(maps1[b][0], ref[b][0]) == 0 and ndiff(maps1[b][1], ref[b][1]) == 0, "volume %d differs from the oracle" % b
        assert ndiff(maps1[b][0], maps0[b][0]) == 0 and ndiff(maps1[b][1], maps0[b][1]) == 0, "volume %d differs from the plain search" % b
    for p in range(NDIR):
        assert ndiff(lr1[p], lr0[p]) == 0, "Lr of pass %d changed" % p
    assert stats0 == (0, 0), "MGM_HIP_WTA_PRUNE=0 must take the plain search"
    npix = M.NX * M.NY * len(cvs)
    emu = sum(r[2] for r in ref)
    print("%s: %d pixels, %d chunks loaded, emulation %d" % (case, px, ch, emu))
    if not pruned:
        assert (px, ch) == (0, 0), "this case must fall back to the plain search"
        return
    assert px == npix
    if seeds[0] != "constant":
        assert npix <= ch <= 1.25 * emu
    else:
        assert ch >= npix


@pytest.mark.parametrize("case", sorted(CASES))
def test_pruned_search(ctx, oracle, case):
    spec = CASES[case]
    imgs, cvs = [], []
    try:
        for u, v in pairs_of(spec):
            du, dv = ctx.upload_image(u), ctx.upload_image(v)
            imgs += [du, dv]
            cvs.append(ctx.costvolume_dev(du, dv, spec[0], spec[1], "none", "census", float("inf"), 5))
        check(ctx, oracle, case, spec, cvs)
    finally:
        for h in imgs + cvs:
            h.free()


def test_refill_on_the_same_context(ctx, oracle):
    """The same volume filled again with other images, searched with other settings: nothing of the first filling's minima may
    outlive it."""
    first = CASES["fh3_8dir_vfit"]
    again = (-255, 0, 8, 3, 0, "vfit", (SEED_B,), True)
    (u, v), = pairs_of(first)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    cv = ctx.costvolume_dev(du, dv, first[0], first[1], "none", "census", float("inf"), 5)
    try:
        check(ctx, oracle, "fh3_8dir_vfit", first, [cv])
        (u2, v2), = pairs_of(again)
        du.update(u2)
        dv.update(v2)
        ctx.costvolume_dev(du, dv, again[0], again[1], "none", "census", float("inf"), 5, into=cv)
        check(ctx, oracle, "refill", again, [cv])
    finally:
        for h in (du, dv, cv):
            h.free()


def test_planted_winners(ctx, oracle):
    """Winners at labels 31 / 32 (both sides of a chunk edge: vfit reads the neighbour chunk) and at 0 / L-1."""
    L, dmin = 256, -100
    C, where = M.planted_volume(L)
    S, out, outc, lr = oracle.mgm(C, dmin, 8.0, 32.0, 8, 3, 0, 1, dump_lr=True)
    ro, rc = oracle.refine(S, dmin, "vfit", out, outc)
    emu = M.pruned_search(C, lr, dmin, 1)[2]
    cv = ctx.upload_volume(C, dmin)
    try:
        ctx.timing(True)
        _, o, c = ctx.aggregate_dev(cv, 8.0, 32.0, 8, 3, 0, 1, None, "vfit")
        px, ch = ctx.wta_stats()
        ctx.timing(False)
        assert ndiff(o.download()[0], ro) == 0 and ndiff(c.download()[0], rc) == 0
        assert px == M.NX * M.NY and px <= ch <= 1.25 * emu
        o.free()
        c.free()
    finally:
        cv.free()
