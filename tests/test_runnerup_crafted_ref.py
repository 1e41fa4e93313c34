"""What tests/test_gpu_wta_runnerup_crafted.py holds the runner-up kernels to, pinned on the CPU: the vectorised model
(tests/runnerup_model.py) against a scalar restatement of its five defining lines on every crafted class, the floors of the
classes of tests/runnerup_crafted.py, and -- without running a kernel -- that the crafted inputs tell the model from eight
subtly wrong searches (mutants) at every (L, radius) of the device grid at which such a search can differ at all."""
import math

import numpy as np
import pytest

import runnerup_crafted as R
import wta_crafted as W
from helpers import ndiff
from runnerup_model import runnerup

f32 = np.float32
# the device grid (tests/test_gpu_wta_runnerup_crafted.py): the strides of the 14 streaming instances, the odd widths a run may
# pad, the widths of the generic kernel
STREAM_L = (64, 128, 192, 256, 384, 512, 768, 1024)
PADDED_L = (63, 100, 151, 300)
ANY_L = (1, 2, 3, 4, 37, 64, 300, 1100)
GRID_L = STREAM_L + PADDED_L + tuple(L for L in ANY_L if L not in STREAM_L + PADDED_L)
NDIRS = (1, 3, 4, 5, 8)
NY, NX = 2, 7  # 14 pixels: two rounds of the seven winner positions
DMIN = -5


def radii(L):
    return (0, 1, 2, 5, L)


def c_name(NDIR, fix, k):
    return "inf1" if (NDIR == 1 and fix == 1) else ("ints", "frac")[k % 2]


# ---- the scalar restatement (and its mutants) -----------------------------------------------------------------------------------
def scalar(S, dmin, radius, L=None, ge=False, shrink=False, last=False, nonfinite=False):
    """runnerup_model.py's head, label by label:
        o1 = first strict minimum among the finite entries by rising o; out1 = (float)(o1 + dmin), cost1 = S(o1); NaN, +INF without
        o2 = the same among the finite entries with |o - o1| > radius; NaN, +INF without a winner or without such an entry
    over the first L entries of every pixel (the rest is padding).  The flags turn it into the mutants below."""
    S = np.asarray(S, np.float32)
    ny, nx, Lk = S.shape
    L = Lk if L is None else L
    maps = [np.full((ny, nx), np.nan, np.float32), np.full((ny, nx), np.inf, np.float32),
            np.full((ny, nx), np.nan, np.float32), np.full((ny, nx), np.inf, np.float32)]
    for y in range(ny):
        for x in range(nx):
            row = S[y, x].tolist()  # (every float32 is a double: the comparisons below are float32's)
            o1, v1 = None, math.inf
            for o in range(L):
                v = row[o]
                if (nonfinite or math.isfinite(v)) and (v <= v1 if last else v < v1):
                    o1, v1 = o, v
            if o1 is None:
                continue
            maps[2][y, x], maps[3][y, x] = f32(o1 + dmin), f32(v1)
            o2, v2 = None, math.inf
            for o in range(L):
                if shrink:
                    far = o < o1 - radius or o > o1 + radius - 1
                elif ge:
                    far = abs(o - o1) >= radius
                else:
                    far = abs(o - o1) > radius
                v = row[o]
                if far and (nonfinite or math.isfinite(v)) and (v <= v2 if last else v < v2):
                    o2, v2 = o, v
            if o2 is not None:
                maps[0][y, x], maps[1][y, x] = f32(o2 + dmin), f32(v2)
    return tuple(maps)


def differ(a, b):
    return any(ndiff(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("L", GRID_L)
def test_the_model_is_the_scalar_restatement(L):
    """every (L, radius, NDIR, fix) of the device grid, two classes each in turn: every class of runnerup_crafted and of
    wta_crafted.LR_CLASSES meets every (L, radius); costs `ints` and `frac` in turn, `inf1` at one pass with the fix"""
    LPL = R.lpl_of(L)
    for radius in radii(L):
        cls = R.all_classes(radius, LPL)
        names = list(cls)
        met, j = set(), 0
        for NDIR in NDIRS:
            for fix in (0, 1):
                for name in (names[(2 * j) % len(names)], names[(2 * j + 1) % len(names)]):
                    lr = cls[name](40 + j, NDIR, NY, NX, L)
                    assert lr.dtype == np.float32 and lr.shape == (NDIR, NY, NX, L)
                    Cv = W.C_CLASSES[c_name(NDIR, fix, j)](50 + j, NY, NX, L)
                    S = W.sum_fix(lr, Cv, NDIR, fix)
                    assert not differ(runnerup(S, DMIN, radius), scalar(S, DMIN, radius)), (name, L, radius, NDIR, fix)
                    met.add(name)
                j += 1
        assert met == set(names)


@pytest.mark.parametrize("L", GRID_L)
def test_floors(L):
    """the exact counts of tests/runnerup_crafted.py on the model's maps: at 14 and 130 pixels, every radius, the instance's labels
    per lane and the generic kernel's, every pass count, without the fix and with it under `ints` and `frac`"""
    for radius in radii(L):
        for LPL in sorted({1, R.lpl_of(L)}):
            cls = R.classes(radius, LPL)
            for ny, nx in ((NY, NX), (10, 13)):
                for k, NDIR in enumerate(NDIRS):
                    for name in cls:
                        lr = cls[name](60 + k, NDIR, ny, nx, L)
                        for fix, cname in ((0, "ints"), (1, "ints"), (1, "frac")):
                            S = W.sum_fix(lr, W.C_CLASSES[cname](70 + k, ny, nx, L), NDIR, fix)
                            R.floors(name, runnerup(S, 0, radius), ny, nx, L, radius, LPL, fix)


def test_the_seven_positions():
    """at the strides of the instances every position is a label of its own kind"""
    for L in STREAM_L:
        LPL = L // 64
        for radius in (0, 1, 2, 5):
            w = [R.position(k, L, radius, LPL) for k in range(R.NPOS)]
            assert None not in w
            assert w[0] == 0 and w[1] == radius and w[2] == L - 1 and w[3] == L - 1 - radius
            assert w[4] % LPL == 0 and w[4] - radius - 1 >= 0 and (w[4] - radius - 1) // LPL < w[4] // LPL
            assert (w[5] + 1) % LPL == 0 and (w[5] + radius + 1) // LPL > w[5] // LPL
            assert (w[6] + radius + 1) % LPL == 0 and w[6] >= 0
    for L in (1, 2, 3):  # too small for most positions: every pixel still gets a winner
        for radius in radii(L):
            assert all(0 <= R.winner_of(i, L, radius, 1)[1] < L for i in range(20))


# ---- mutants ----------------------------------------------------------------------------------------------------------------------
# name -> can it differ from the model at (L, radius) at all?  By arithmetic:
#   ge, shrink   admit a label at distance exactly `radius` from the winner (the winner itself at radius 0): one exists iff radius <= L - 1
#   last         needs two labels
#   nonfinite    a -INF entry is below every finite one: always (one label is enough)
#   padding      needs a padding slot: the stride is the next multiple of 64, so iff L % 64 != 0
#   reverse, beyond, ndir    mutate the sum at 5 passes with the fix: always (out1 / cost1 differ whatever the radius)
SEARCH_MUTANTS = {
    "ge": (dict(ge=True), lambda L, r: r <= L - 1),
    "shrink": (dict(shrink=True), lambda L, r: r <= L - 1),
    "last": (dict(last=True), lambda L, r: L >= 2),
    "nonfinite": (dict(nonfinite=True), lambda L, r: True),
}
PAD = f32(-1e30)
M_NDIR = 5


def padded(S, L):
    Lk = -(-L // 64) * 64
    return np.concatenate([S, np.full(S.shape[:2] + (Lk - L,), PAD, np.float32)], axis=2)


def caught_by(L, radius, mutant):
    """the first class on which the mutant's maps differ from the model's, or None"""
    cls = R.all_classes(radius, R.lpl_of(L))
    for k, name in enumerate(cls):
        lr = cls[name](80 + k, M_NDIR, NY, NX, L)
        Cv = W.c_ints(90 + k, NY, NX, L)
        want = runnerup(W.sum_fix(lr, Cv, M_NDIR, 1), DMIN, radius)
        if mutant in SEARCH_MUTANTS:
            got = scalar(W.sum_fix(lr, Cv, M_NDIR, 1), DMIN, radius, **SEARCH_MUTANTS[mutant][0])
        elif mutant == "padding":
            got = scalar(padded(W.sum_fix(lr, Cv, M_NDIR, 1), L), DMIN, radius)  # (all Lk slots scanned)
        elif mutant == "reverse":
            got = runnerup(W.sum_fix(lr[::-1], Cv, M_NDIR, 1), DMIN, radius)
        elif mutant == "ndir":
            with np.errstate(all="ignore"):
                got = runnerup(W.sum_fix(lr, Cv, M_NDIR, 0) - f32(M_NDIR) * Cv, DMIN, radius)
        elif mutant == "beyond":
            got = runnerup(_sum_beyond(lr, Cv), DMIN, radius)
        else:
            raise KeyError(mutant)
        if differ(got, want):
            return name
    return None


def _sum_beyond(lr, Cv):
    """the sum over all 8 passes of pass_guard(lr), then the over-count term of the M_NDIR passes there are"""
    with np.errstate(all="ignore"):
        return (W.sum_fix(R.pass_guard(lr), Cv, 8, 0) - f32(M_NDIR - 1) * Cv).astype(np.float32)


MUTANTS = list(SEARCH_MUTANTS) + ["padding", "reverse", "ndir", "beyond"]


@pytest.mark.parametrize("L", GRID_L)
def test_every_mutant_is_caught(L):
    for radius in radii(L):
        for mutant in MUTANTS:
            can = SEARCH_MUTANTS[mutant][1](L, radius) if mutant in SEARCH_MUTANTS else (L % 64 != 0 if mutant == "padding" else True)
            name = caught_by(L, radius, mutant)
            if can:
                assert name is not None, "mutant %s survives every class at L %d radius %d" % (mutant, L, radius)
            else:
                assert name is None, "mutant %s cannot differ at L %d radius %d, yet %s says it does" % (mutant, L, radius, name)


def test_the_padding_mutant_reads_what_the_device_test_writes():
    """a stride-Lk array whose padding holds -1e30: the model on the first L labels ignores it, a scan of all Lk does not"""
    L, radius = 100, 2
    S = W.sum_fix(R.lr_zone(1, 3, NY, NX, L, radius, 1), W.c_ints(2, NY, NX, L), 3, 0)
    P = padded(S, L)
    assert P.shape[2] == 128 and (P[:, :, L:] == PAD).all()
    assert not differ(scalar(P, DMIN, radius, L=L), runnerup(S, DMIN, radius))
    assert (scalar(P, DMIN, radius)[3] == PAD).all()
