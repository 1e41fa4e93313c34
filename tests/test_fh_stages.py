"""The FH min-convolution's four stages (fh_scan: guess, fh_careful, fh_repair, plain sweeps; mgm_pass_common.h) on the CPU:
the numpy restatement (tests/fh_stage_model.py) pinned on the oracle, the oracle on the compiled reference, the stages on the
sequential recurrences for every instance shape, and the floors that the device cases' inputs meet
(tests/test_gpu_fh_stages.py asserts the same floors before each call).  No GPU."""
import numpy as np
import pytest

import fh_stage_model as fm
from helpers import labels_equal, ndiff
from oracle.oracle import int_ranges, usable_cpus

f32 = np.float32
CLASSES = ("infgap", "frac", "spike", "end0", "big")  # the issue's five; `byte` and `lanecol` are this suite's additions
NX, NY = 23, 11


def three_weights(rng, ny=NY, nx=NX):
    return rng.choice(np.array(fm.WEIGHTS3, f32), size=(8, ny, nx), p=(0.6, 0.25, 0.15)).astype(f32)


@pytest.fixture(scope="module")
def fast_oracle(oracle):
    oracle.set_threads(min(16, usable_cpus()))
    yield oracle
    oracle.set_threads(1)


# ---- the model pinned on the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES + ("byte", "lanecol"))
def test_model_minconv_reproduces_the_oracles_lr(fast_oracle, cls):
    """oracle.mgm(FH=1, dump_lr=True): the model's sequential minconv applied to the dumped neighbours gives the dumped Lr."""
    rng = np.random.default_rng(2)
    for L in (40, 64, 256):
        C = fm.volume(cls, 3, NY, NX, L)
        for P1 in fm.PENALTIES:
            for NDIR in (1, 8):
                for MGM in (1, 2, 3, 4):
                    w8 = three_weights(rng) if (MGM + NDIR) % 3 == 0 else None
                    P2 = np.inf if MGM == 4 else 8 * P1
                    lr = fast_oracle.mgm(C, -3, P1, P2, NDIR, MGM, 1, 1, w8, dump_lr=True)[3]
                    assert ndiff(fm.lr_from_neighbours(C, lr, P1, P2, MGM, w8), lr) == 0, (cls, L, P1, NDIR, MGM, w8 is not None)


def test_model_device_form_equals_the_sequential_form():
    """The model's fh_minconv (stages, padding reset, cap) against its own sequential minconv: padded and full label counts."""
    for cls in CLASSES:
        for L, LPL, G in ((100, 2, 1), (151, 3, 1), (256, 4, 1), (600, 12, 1), (128, 4, 2), (64, 4, 4), (50, 4, 4)):
            S = fm.volume(cls, 5, 6, 20, L).reshape(-1, L)
            for P1 in (2.0, 0.1, 2.5):
                m = S.min(1)
                assert ndiff(fm.device_minconv(S, P1, 30 * P1, m, LPL, G, L), fm.minconv(S, P1, 30 * P1, m)) == 0, (cls, L, P1)


# ---- the oracle pinned on the compiled reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES + ("byte", "lanecol"))
def test_oracle_vs_reference(fast_oracle, reference, cls):
    """The oracle needed no change: 0 differing words in S and the cost map, equal labels, weighted and unweighted."""
    rng = np.random.default_rng(4)
    for L in (40, 256):
        C = fm.volume(cls, 3, NY, NX, L)
        for P1 in fm.PENALTIES:
            for (NDIR, MGM) in ((8, 3), (8, 2), (1, 1), (8, 4)) if L == 40 else ((8, 3),):
                for w8 in (None, three_weights(rng)):
                    P2 = np.inf if MGM == 4 else 8 * P1
                    a = fast_oracle.mgm(C, -3, P1, P2, NDIR, MGM, 1, 1, w8)
                    b = reference.mgm(C, -3, P1, P2, NDIR, MGM, 1, 1, w8)
                    tag = (cls, L, P1, NDIR, MGM, w8 is not None)
                    assert ndiff(a[0], b[0]) == 0 and ndiff(a[2], b[2]) == 0 and labels_equal(a[1], b[1], a[2]), tag


# ---- the stage implementations pinned on themselves --------------------------------------------------------------------------------
@pytest.mark.parametrize("LPL", fm.LPLS)
def test_stage_carries_and_loop_bound(LPL):
    """For GROUPS 1, 2, 4 and both directions, on 500 slabs per class (the issue's five, `byte`, `lanecol`) and penalty: the carries of the stage the model says is
    accepted are the sequential carries, and the loop takes <= 67 iterations (64 lanes + the three boosted turns; the cap is
    70).  Classes are interleaved, so the lane groups of a wave (GROUPS > 1) hold different classes and vote together."""
    for G in (1, 2, 4):
        GL = 64 // G
        for L in (GL * LPL, GL * LPL - LPL - 1) if LPL in (2, 3, 12) and G == 1 else (GL * LPL,):  # (padded: as 100, 151, 600 labels)
            reach = np.zeros((2, 4), int)
            worst = 0
            for P1 in fm.PENALTIES:
                S = np.stack([fm.volume(c, 3, 20, 25, L).reshape(-1, L) for c in CLASSES + ("byte", "lanecol")], 1).reshape(-1, L)
                st, its, car = fm.stages(S, f32(P1), LPL, G, L, want_carries=True)
                for d in (0, 1):
                    acc, seq, _ = car[d]
                    assert np.array_equal(acc.view(np.uint32), seq.view(np.uint32)), (LPL, G, L, P1, d)
                    reach[d] += np.bincount(st[:, d], minlength=4)
                worst = max(worst, int(its.max()))
                assert its.max() <= 67, (LPL, G, L, P1, int(its.max()))
            print("LPL", LPL, "GROUPS", G, "L", L, "fwd", reach[0], "bwd", reach[1], "most iterations", worst)
            # every shape reaches every stage in one direction at least -- LPL 1 with GROUPS 4 (16 labels) too: a hop of up to 15
            # lanes from a value far below P1 crosses four binades
            assert (reach.sum(0) > 0).all(), (LPL, G, L, reach.tolist())
            assert worst >= GL, (LPL, G, L, worst)  # ... and the long tail: plain sweeps over the whole range


# ---- the floors of the device cases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fm.DENSE_CASES, ids=lambda c: c["name"])
def test_floors_of_the_dense_device_cases(fast_oracle, c):
    by_stage, long_ = fm.dense_case_counts(c, fast_oracle)
    print(c["name"], c["cls"] if not c["classes"] else c["classes"], "P1", c["P1"], "fwd", by_stage[0], "bwd", by_stage[1], "long", long_)
    assert not fm.floors_met(c, by_stage, long_)


def rel_oracle_run(oracle, c, dump_lr):
    u, v, lo, hi = fm.rel_case_inputs(c)
    ilo, ihi = int_ranges(lo, hi)
    dmin, dmax = c["hull"]
    C = oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, "none", "ad", np.inf, 5)
    w8 = fm.case_weights(c)
    res = oracle.mgm_ranged(C, dmin, ilo, ihi, c["P1"], c["P1"] * c["P2f"], c["NDIR"], c["MGM"], 1, 1, w8, dump_lr=dump_lr)
    return (u, v, lo, hi, ilo, ihi, C, w8), res


@pytest.mark.parametrize("c", fm.REL_CASES, ids=lambda c: c["name"])
def test_floors_of_the_ragged_device_cases(fast_oracle, c):
    (u, v, lo, hi, ilo, ihi, C, w8), res = rel_oracle_run(fast_oracle, c, True)
    fin = np.isfinite(C)
    assert fin.any(2).all() and set(np.unique(C[fin])) <= {0.0, 1.0, 2.0, 250.0}  # the one-byte class, a finite cost in every pixel
    by_stage, long_, mixed = fm.rel_case_counts(c, res[3], ilo, ihi, w8)
    print(c["name"], "P1", c["P1"], "fwd", by_stage[0], "bwd", by_stage[1], "long", long_, "mixed pixels", mixed)
    assert not fm.rel_floors_met(c, by_stage, long_, mixed)
