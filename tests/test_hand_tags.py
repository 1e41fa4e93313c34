"""HandTags (mgm_amd/csrc/mgm_planner.h) on the host: the tags of the self-validating hand-off slots are what run_passes / run_rel
handed out inline before the state machine existed (tests/hand_tags_model.py: both versions at commit 098beb7) -- the same clears
and the same tags on every sequence of launches, watchdog errors and trims, but for ONE deliberate difference: a watchdog error
forgets the range-proportional region too.  The protocol's invariant -- no launch hands a pass a tag that a slot of that pass may
still carry -- holds for the new code on every sequence, and the parent's range-proportional version breaks it after a time-out."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import hand_tags_model as M
from hand_tags_model import DENSE, LAUNCH, REL, TAG, TRIM, WATCHDOG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgm_amd", "csrc")
# nx, ny, npass, groups, slot floats, slots, R, bands of the last pass: A; A with one band more; A laid out for four passes (a
# prefix of A's); A for two volume groups; another image; two of the range-proportional kind (slots > 0)
LAYOUTS = [(160, 130, 8, 1, 256, 0, 8, 3), (160, 130, 8, 1, 256, 0, 8, 4), (160, 130, 4, 1, 256, 0, 8, 3), (160, 130, 8, 2, 256, 0, 8, 3),
           (150, 110, 8, 1, 256, 0, 8, 3), (150, 110, 8, 1, 72, 64, 4, 3), (150, 110, 4, 1, 72, 64, 4, 3)]
A, B = 0, 1
OK, FAILS = 0, 1


def launch(region, layout, first=0, count=None, moved=0, fails=OK):
    return (LAUNCH, region, layout, first, LAYOUTS[layout][2] - first if count is None else count, moved, fails)


WD, TR = (WATCHDOG, 0, 0, 0, 0, 0, 0), (TRIM, 0, 0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("handtags") / "libhand_tags_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "hand_tags_harness.cc"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    lib.hand_tag_bit.restype = C.c_uint
    assert lib.hand_max_dirs() == M.NPASS and lib.hand_tag_bit() == TAG
    assert lib.hand_clear_byte() == 0xFF and (0xFFFFFFFF & TAG) == M.CLEARED  # cleared words have the tag bit set
    return lib


def physical(events):
    """The events as a context can meet them: the first launch of a region, and the first after a trim, finds no buffer -- it moved."""
    fresh, out = [True, True], []
    for e in events:
        if e[0] == TRIM:
            fresh = [True, True]
        elif e[0] == LAUNCH and fresh[e[1]]:
            e, fresh[e[1]] = e[:5] + (1,) + e[6:], False
        out.append(e)
    return out


def run_new(lib, events):
    """What the harness's regions do on the events: per event None, or (clear, {pass: tag}) like the model."""
    lay = np.ascontiguousarray(LAYOUTS, dtype=np.int32)
    ev = np.ascontiguousarray(events, dtype=np.int32)
    out = np.full((len(events), 1 + M.NPASS), 0xDEAD, dtype=np.uint32)
    lib.hand_run(lay.ctypes.data_as(C.c_void_p), C.c_int(len(lay)), ev.ctypes.data_as(C.c_void_p), C.c_int(len(ev)), out.ctypes.data_as(C.c_void_p))
    steps = []
    for e, o in zip(events, out.tolist()):
        if e[0] != LAUNCH:
            steps.append(None)
            continue
        assert all(o[1 + k] == 0 for k in range(M.NPASS) if not e[3] <= k < e[3] + e[4]), (e, o)  # passes not launched: no tag
        steps.append((bool(o[0]), {k: o[1 + k] for k in range(e[3], e[3] + e[4])}))
    return steps


def random_events(rng, n, watchdog=True):
    """Launches on both regions (the range-proportional one always runs all its passes), one launch in six fails before its enqueue,
    one in five finds its buffer moved; a watchdog error or a trim now and then."""
    ev = []
    for _ in range(n):
        kind = rng.choice([LAUNCH] * 10 + [WATCHDOG] * (2 if watchdog else 0) + [TRIM])
        if kind != LAUNCH:
            ev.append(WD if kind == WATCHDOG else TR)
            continue
        region = rng.choice((DENSE, REL))
        layout = rng.choice((0, 0, 0, 1, 2, 3, 4) if region == DENSE else (5, 5, 6))
        npass = LAYOUTS[layout][2]
        first = 0 if region == REL else rng.randrange(npass)
        count = npass if region == REL else rng.choice((1, 1, npass - first, rng.randrange(1, npass - first + 1)))
        ev.append(launch(region, layout, first, count, int(rng.random() < 0.2), int(rng.random() < 1 / 6)))
    return physical(ev)


def of_region(events, steps, region):
    return [s for e, s in zip(events, steps) if e[0] == LAUNCH and e[1] == region]


FIXED = {
    "one by one, some more often, then all eight": [launch(DENSE, A, k, 1) for k in (0, 1, 2, 3, 4, 5, 6, 7, 2, 5, 2, 7)] + [launch(DENSE, A)] * 2,
    "an error between begin and commit, then the same layout": [launch(DENSE, A), launch(DENSE, A, fails=FAILS), launch(DENSE, A)]
    + [launch(REL, 5), launch(REL, 5, fails=FAILS), launch(REL, 5)],
    "layouts A, B, A": [launch(DENSE, A), launch(DENSE, B), launch(DENSE, A), launch(REL, 5), launch(REL, 6), launch(REL, 5)],
    "a trim between two equal launches": [launch(DENSE, A), launch(REL, 5), TR, launch(DENSE, A), launch(REL, 5)],
    "a prefix of the passes is another layout": [launch(DENSE, A), launch(DENSE, 2), launch(DENSE, A, 0, 4)],
    "a watchdog error": [launch(DENSE, A), launch(DENSE, A), WD, launch(DENSE, A), launch(DENSE, A, 3, 1), WD, launch(DENSE, A, 3, 1)],
}
REL_TIMEOUT = [launch(REL, 5), launch(REL, 5), WD, launch(REL, 5)]


def sequences(watchdog):
    rng = random.Random(20261019)
    return [physical(s) for s in FIXED.values()] + [random_events(rng, rng.randrange(2, 40), watchdog) for _ in range(3000)]


def test_clears_and_tags_equal_the_parents(lib):
    """Dense: on every sequence.  Range-proportional: on every sequence without a watchdog error (the deliberate difference)."""
    launches = 0
    for watchdog in (True, False):
        for ev in sequences(watchdog):
            new, old = run_new(lib, ev), M.Parent().run(ev)
            assert of_region(ev, new, DENSE) == of_region(ev, old, DENSE), ev
            if not watchdog:
                assert of_region(ev, new, REL) == of_region(ev, old, REL), ev
            launches += sum(e[0] == LAUNCH for e in ev)
    assert launches > 50000


def test_no_launch_hands_out_a_tag_its_slots_may_carry(lib):
    seen = dict(clears=0, keeps=0, watchdogs=0)
    for ev in sequences(True) + [physical(REL_TIMEOUT)]:
        steps = run_new(lib, ev)
        assert M.violations(ev, steps) == [], ev
        for e, s in zip(ev, steps):  # the range-proportional kernel takes ONE tag: its passes' tags are in lockstep
            assert e[0] != LAUNCH or e[1] != REL or len(set(s[1].values())) == 1, (ev, s)
        seen["clears"] += sum(bool(s and s[0]) for s in steps)
        seen["keeps"] += sum(bool(s and not s[0]) for s in steps)
        seen["watchdogs"] += sum(e[0] == WATCHDOG for e in ev)
    assert min(seen.values()) > 1000, seen  # (a region that was always cleared would satisfy the invariant too)


def test_the_parents_range_proportional_region_breaks_the_invariant_after_a_time_out(lib):
    """The recorded reason for the difference: the parent's watchdog error left hand_rel_key alone, so the launch after a timed-out one
    hands out the tag of the launch before it -- which the slots that the timed-out launch did not reach still carry."""
    ev = physical(REL_TIMEOUT)
    old, new = M.Parent().run(ev), run_new(lib, ev)
    assert old[3] == (False, {k: 0 for k in range(8)})
    assert [(i, t) for i, _, t in M.violations(ev, old)] == [(3, 0)] * 8
    assert new[3] == (True, {k: 0 for k in range(8)}) and new[:3] == old[:3]
    dense = physical([launch(DENSE, A), launch(DENSE, A), WD, launch(DENSE, A)])  # (the dense region was forgotten already)
    assert M.violations(dense, M.Parent().run(dense)) == []


def test_fixed_sequences(lib):
    got = {name: run_new(lib, physical(ev)) for name, ev in FIXED.items()}
    steps = got["one by one, some more often, then all eight"]
    assert [s[0] for s in steps] == [True] + [False] * 13                      # cleared once: nobody makes it be cleared again
    assert steps[12][1] == {k: (0 if k in (5, 7) else TAG) for k in range(8)}  # 5 and 7 had been launched twice, 2 three times, the rest once
    assert len(set(steps[12][1].values())) == 2                                # tags of different passes differ
    assert steps[13][1] == {k: t ^ TAG for k, t in steps[12][1].items()}
    assert [s[0] for s in got["an error between begin and commit, then the same layout"]] == [True, False, True] * 2
    assert [s[0] for s in got["layouts A, B, A"]] == [True] * 6
    assert [s[0] for s in got["a trim between two equal launches"] if s] == [True] * 4
    assert [s[0] for s in got["a prefix of the passes is another layout"]] == [True] * 3
    assert [s[0] for s in got["a watchdog error"] if s] == [True, False, True, False, True]
    for steps in got.values():  # a cleared region starts every pass again with tag 0
        assert all(set(s[1].values()) == {0} for s in steps if s and s[0])
