"""The expectation of tests/test_gpu_exact_crafted.py, without a device: for every case of tests/exact_crafted.py the CPU oracle
against the compiled reference -- S, the cost map, the labels where the cost is finite -- and the floors that keep a case from
passing by being NaN everywhere or nowhere, on the oracle's dumped Lr volumes."""
import numpy as np
import pytest

import exact_crafted as X
from helpers import labels_equal, ndiff

IDS = [c.name for c in X.CASES]


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_oracle_equals_the_reference(oracle, reference, case):
    if case.kind == "ragged" and not reference.has_ranged():
        pytest.skip("oracle/_ref/libmgm_ref.so predates the ranged entry points")
    built = X.build(case, oracle)
    exp = X.expected(case, built, oracle)
    for k in range(len(built.Cs)):
        S, out, cost = X.aggregate_on(reference, case, built, k, dump_lr=False)
        assert ndiff(exp.S[k], S) == 0, (case.name, k)
        assert ndiff(exp.cost[k], cost) == 0, (case.name, k)
        assert labels_equal(exp.out[k], out, exp.cost[k]), (case.name, k)


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_floors(oracle, case):
    built = X.build(case, oracle)
    assert X.must_take_exact(case, built) in ("nan", "labels", "ragged")
    fig = X.check_floors(case, built, oracle)
    print(case.name, fig)
    exp = X.expected(case, built, oracle)
    # the sum alone would not do: of the cases with whole-NaN pixels most have an S that is NaN almost everywhere
    assert all(lr.shape[0] == case.NDIR for lr in exp.lr)


def test_the_matrix_is_complete():
    """all four update functions x NDIR 1, 3, 4, 8; every class at 70 and 131 labels on every function; every penalty pair, weight
    set and label count at least once; lane-chunks of 1, 2, 3 and 5 labels"""
    uni = [c for c in X.CASES if c.kind == "uniform"]
    assert {(X.mode_of(c), c.NDIR) for c in uni} >= {(m, n) for m in range(4) for n in X.NDIRS}
    mat = [c for c in uni if c.name.startswith("m")]
    assert {(c.cls, X.mode_of(c), c.L) for c in mat} == {(k, m, L) for k in X.CLASSES for m in range(4) for L in (70, 131)}
    same = lambda a, b: a == b or (a != a and b != b)
    for P in X.PENALTIES:
        for FH in (0, 1):
            assert any(same(c.P1, P[0]) and same(c.P2, P[1]) and c.FH == FH for c in uni), (P, FH)
    assert {c.wkind for c in uni} >= {None, "w2", "w3", "wodd"}
    assert {c.L for c in uni} >= {1, 2, 24, 64, 65, 70, 128, 131, 300, 2049, 8193}
    assert {X.lane_chunk(c.L) for c in uni if c.L <= 300} == {1, 2, 3, 5}
    assert {(c.nx, c.ny) for c in uni} >= {(24, 16), (1, 1), (1, 9), (7, 1), (2, 2), (3, 3), (40, 3), (13, 11)}
    assert {X.mode_of(c) for c in uni if c.L == 8193} == {2, 3}  # (both FH functions on the global-scratch arrays)
    assert sum(c.kind == "batch" for c in X.CASES) == 1 and sum(c.kind == "ragged" for c in X.CASES) == 10


def test_must_take_exact_refuses_what_could_reach_a_fast_kernel(oracle):
    """the gate of the device file: a NaN-free uniform volume, a batch whose NaN-free volume is not tame, a ragged volume inside
    the fast kernels' premise"""
    case = next(c for c in X.CASES if c.name == "m1_huge_L70")
    built = X.build(case)
    clean = built._replace(Cs=[np.nan_to_num(built.Cs[0], nan=1.0)])
    with pytest.raises(AssertionError):
        X.must_take_exact(case, clean)
    batch = next(c for c in X.CASES if c.kind == "batch")
    b = X.build(batch)
    assert X.must_take_exact(batch, b) == "nan"
    for odd in (np.float32(-1.0), np.float32(0.5), np.float32(np.inf), np.float32(-0.0)):
        C0 = b.Cs[0].copy()
        C0[3, 3, 3] = odd
        with pytest.raises(AssertionError):
            X.must_take_exact(batch, b._replace(Cs=[C0] + b.Cs[1:]))
    with pytest.raises(AssertionError):
        X.must_take_exact(batch._replace(P1=-2.0), b)
    with pytest.raises(AssertionError):
        X.must_take_exact(batch, b._replace(w8s=[X.weights("wodd", batch.ny, batch.nx, 1)] + b.w8s[1:]))
    rag = next(c for c in X.CASES if c.name == "ragged_negp1_fh_t3")
    rb = X.build(rag, oracle)
    assert X.must_take_exact(rag, rb) == "ragged"
    for tame in (rag._replace(P1=2.0), rag._replace(FH=0)):
        with pytest.raises(AssertionError):
            X.must_take_exact(tame, rb)
    big = next(c for c in X.CASES if c.L == 2049)
    assert X.must_take_exact(big, X.build(big)) == "labels"
