"""The stateful campaign's generator on the CPU (tests/stateful_model.py; the campaign itself is tests/test_gpu_stateful.py):
deterministic, as wide as the campaign claims, and never a call the ABI leaves undefined."""
import stateful_model as sm

SEEDS = range(sm.DEFAULT_BLOCKS)


def test_generation_is_deterministic():
    for seed in SEEDS:
        a, b = sm.generate(seed).ops, sm.generate(seed).ops
        assert [sm.fmt_op(x) for x in a] == [sm.fmt_op(x) for x in b], seed


def test_default_seeds_reach_the_claimed_coverage():
    s = sm.summary([sm.generate(seed) for seed in SEEDS])
    # adjacent launches of one shape and batch size that differ in exactly ONE planner input
    assert s["total"] >= 30, s
    assert all(n >= 1 for n in s["collisions"].values()), s["collisions"]
    # a volume refilled out of and into every format, and ragged -> uniform -> ragged on one handle
    assert set(sm.FORMATS) <= s["from_fmt"] and set(sm.FORMATS) <= s["to_fmt"], s
    assert s["ru_r"] >= 1, s
    # every kind of operation occurs, windowed searches with every expected outcome
    ops = [op for seed in SEEDS for op in sm.generate(seed).ops]
    kinds = {op["op"] for op in ops}
    assert kinds >= {"fill", "upload", "free", "weights", "agg", "wta", "lr", "limit", "trim", "pipeline", "tries", "sync"}, kinds
    assert {op["expect"] for op in ops if op["op"] == "wta"} == {"exact", "refuse", "exact_or_refuse"}
    fills = [op for op in ops if op["op"] == "fill"]
    assert {op["kind"] for op in fills} == {"uniform", "ragged"} and any(op["into"] for op in fills)
    truncs = {sm.fmt_op(dict(t=op["trunc"])) for op in fills}
    assert {"t=inf", "t=0.0", "t=-0.0", "t=nan", "t=-2.0", "t=7.5"} <= truncs, truncs
    assert {op["rel"] for op in ops if op["op"] == "agg"} == {None, "0", "1", "2"}


def test_generated_calls_are_defined():
    """No freed handle is touched, no Lr download but straight after an aggregation, weights only where they exist (the campaign may
    make calls the header says are refused -- a windowed search outside the last aggregation -- but none whose worst case is a fault)."""
    for seed in list(SEEDS) + [100, 101, 102]:
        assert sm.check_legal(sm.generate(seed).ops), seed
