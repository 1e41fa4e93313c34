"""plan_wta_consensus (mgm_amd/csrc/mgm_planner.h) on the host: every instance of the launch tables of mgm_consensus.hip is
reachable and nothing else is chosen, strides outside the table and the forcing switch go to the generic kernel, the
range-proportional layout to its own two instances, bad requests are refused, the grid is never more waves than the pixels need
and never beyond its cap, and a choice is a function of the request's bytes alone."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgm_amd", "csrc")

FIELDS = ("npix", "L", "Lk", "NDIR", "num_cu", "slots", "sw_any", "sw_wg_per_cu", "hull")  # ConsensusRequest, in memory order
REQ_T = np.dtype([(f, "<i8" if f == "npix" else "<i4") for f in FIELDS])
OUT = ("family", "LPL", "PPW", "MAXD", "SPL", "per_wave", "grid")
REFUSE, STREAM, ANY, REL = 0, 1, 2, 3
FULL_HD = 1920 * 1080


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build(str(tmp_path_factory.mktemp("consensusplan")))


def build(where):
    so = os.path.join(where, "libconsensus_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "consensus_plan_harness.cc"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    lib.consensus_wg_per_cu.restype = C.c_longlong
    lib.consensus_rel_wg_per_cu.restype = C.c_longlong
    assert lib.consensus_request_bytes() == REQ_T.itemsize == 40 and lib.consensus_choice_bytes() == 8 + 6 * 4
    return lib


def request(**kw):
    q = dict(npix=FULL_HD, L=256, Lk=None, NDIR=8, num_cu=256, slots=0, sw_any=0, sw_wg_per_cu=0, hull=0)
    for k, v in kw.items():
        assert k in q, k
        q[k] = v
    if q["Lk"] is None:
        q["Lk"] = q["L"]
    return tuple(q[f] for f in FIELDS)


def ask(lib, rows):
    a = np.array(rows, dtype=np.int64)
    req = np.zeros(len(rows), dtype=REQ_T)
    for k, f in enumerate(FIELDS):
        req[f] = a[:, k]
    out = np.zeros((len(rows), len(OUT)), dtype=np.int64)
    lib.consensus_plan(req.ctypes.data_as(C.c_void_p), C.c_int(len(rows)), out.ctypes.data_as(C.c_void_p))
    return [dict(zip(OUT, r)) for r in out.tolist()]


def instance(c):
    if c["family"] == STREAM:
        return "k_wta_consensus<%d,%d,%d>" % (c["LPL"], c["PPW"], c["MAXD"])
    if c["family"] == REL:
        return "k_wta_consensus_rel<%d>" % c["SPL"]
    return {ANY: "k_wta_consensus_any", REFUSE: None}[c["family"]]


def family_name(c):
    return {STREAM: "k_wta_consensus_stream", ANY: "k_wta_consensus_any", REL: "k_wta_consensus_rel"}[c["family"]]


def launch_table():
    src = open(os.path.join(CSRC, "mgm_consensus.hip")).read()
    assert "hipLaunchKernelGGL(k_wta_consensus_any," in src
    return ({"k_wta_consensus<%s,%s,%s>" % a for a in re.findall(r"\bCONSENSUS\((\d+), (\d+), (\d+)\)", src)} |
            {"k_wta_consensus_rel<%s>" % a for a in re.findall(r"\bCONSENSUS_REL\((\d+)\)", src)} | {"k_wta_consensus_any"})


def runnerup_table():
    src = open(os.path.join(CSRC, "mgm_wta.hip")).read()
    return set(re.findall(r"\bRUNNERUP\((\d+), (\d+), (\d+)\)", src))


def test_every_instance_of_the_tables_is_reachable_and_nothing_else(lib):
    rows = [request(L=L, Lk=Lk, NDIR=n, npix=npix, hull=h) for Lk in [64 * k for k in range(1, 20)] + [63, 65, 100, 200, 1100, 2049]
            for L in {Lk, max(1, Lk - 13), 1} for n in range(1, 9) for npix in (1, 5, 3201, FULL_HD) for h in (0, 1)]
    rows += [request(slots=s, NDIR=n, npix=npix, L=L) for s in (64, 128) for n in (1, 4, 8) for npix in (1, 17, FULL_HD) for L in (0, 70)]
    reached = {instance(c) for c in ask(lib, rows)}
    table = launch_table()
    assert len(table) == 17
    assert reached == table, sorted(reached ^ table)
    # the streaming instances are the runner-up search's 14
    src = open(os.path.join(CSRC, "mgm_consensus.hip")).read()
    assert set(re.findall(r"\bCONSENSUS\((\d+), (\d+), (\d+)\)", src)) == runnerup_table() and len(runnerup_table()) == 14


NAMED = [
    ("256 labels, 8 passes", dict(), "k_wta_consensus<4,3,8>"), ("256 labels, 4 passes: twice the slabs", dict(NDIR=4), "k_wta_consensus<4,6,4>"),
    ("64 labels", dict(L=64), "k_wta_consensus<1,4,8>"), ("... 3 passes", dict(L=64, NDIR=3), "k_wta_consensus<1,8,4>"),
    ("128 labels", dict(L=128), "k_wta_consensus<2,4,8>"), ("... 1 pass", dict(L=128, NDIR=1), "k_wta_consensus<2,8,4>"),
    ("192 labels", dict(L=192), "k_wta_consensus<3,2,8>"), ("... 4 passes", dict(L=192, NDIR=4), "k_wta_consensus<3,4,4>"),
    ("151 labels padded to 192", dict(L=151, Lk=192), "k_wta_consensus<3,2,8>"), ("a ragged hull of 70 labels padded to 128", dict(L=70, Lk=128, hull=1), "k_wta_consensus<2,4,8>"),
    ("384 labels", dict(L=384), "k_wta_consensus<6,1,8>"), ("... 4 passes", dict(L=384, NDIR=4), "k_wta_consensus<6,2,4>"),
    ("512 labels", dict(L=512), "k_wta_consensus<8,1,8>"), ("... 4 passes", dict(L=512, NDIR=4), "k_wta_consensus<8,2,4>"),
    ("768 labels", dict(L=768), "k_wta_consensus<12,1,8>"), ("... 4 passes: no wider instance", dict(L=768, NDIR=4), "k_wta_consensus<12,1,8>"),
    ("1024 labels", dict(L=1024), "k_wta_consensus<16,1,8>"), ("a stride of 100", dict(L=100), "k_wta_consensus_any"),
    ("a stride of 320: no instance", dict(L=320), "k_wta_consensus_any"), ("1100 labels padded to 1152", dict(L=1100, Lk=1152), "k_wta_consensus_any"),
    ("MGM_HIP_WTA_CONSENSUS_ANY=1", dict(sw_any=1), "k_wta_consensus_any"), ("... on the range-proportional layout", dict(slots=64, sw_any=1), "k_wta_consensus_any"),
    ("64 slots", dict(slots=64), "k_wta_consensus_rel<4>"), ("128 slots, whatever L says", dict(slots=128, L=0, Lk=0), "k_wta_consensus_rel<8>"),
    ("no label", dict(L=0, Lk=64), None), ("a stride below the labels", dict(L=256, Lk=192), None), ("no pixel", dict(npix=0), None),
    ("a negative pixel count", dict(npix=-4), None), ("no pass", dict(NDIR=0), None), ("nine passes", dict(NDIR=9), None),
    ("refused even when forced", dict(L=0, Lk=64, sw_any=1), None), ("a negative cap", dict(sw_wg_per_cu=-1), None),
    ("32 slots: no such format", dict(slots=32), None), ("96 slots", dict(slots=96), None), ("no pass on the range-proportional layout", dict(slots=64, NDIR=0), None),
]


def test_the_named_choices(lib):
    got = ask(lib, [request(**kw) for _, kw, _ in NAMED])
    for (what, kw, want), g in zip(NAMED, got):
        assert instance(g) == want, (what, kw, g)
        if want is None:
            assert g == dict(family=0, LPL=0, PPW=0, MAXD=0, SPL=0, per_wave=0, grid=0), (what, g)
        elif want == "k_wta_consensus_any":
            assert (g["LPL"], g["PPW"], g["MAXD"], g["SPL"], g["per_wave"]) == (0, 0, 0, 0, 1)
        elif g["family"] == REL:
            assert (g["LPL"], g["PPW"], g["MAXD"], g["per_wave"]) == (0, 0, 0, 4)
        else:
            assert g["SPL"] == 0 and g["per_wave"] == g["PPW"]


def test_the_grid_is_never_more_waves_than_the_pixels_need(lib):
    """exactly the waves the pixels need (a wave takes per_wave pixels per turn), four per workgroup, at most the cap: 768
    workgroups per CU (the runner-up search's figure), 64 on the range-proportional layout (k_wta_rel's), or what
    MGM_HIP_WTA_CONSENSUS_WG says"""
    assert lib.consensus_wg_per_cu() == 768 and lib.consensus_rel_wg_per_cu() == 64
    rows, caps = [], []
    for npix, cu, (L, n, slots), any_, wg in itertools.product((1, 3, 4, 5, 33, 3201, FULL_HD, 1 << 33), (0, 1, 256, 304),
                                                               ((1, 8, 0), (64, 8, 0), (64, 4, 0), (100, 8, 0), (256, 8, 0), (256, 3, 0), (1024, 8, 0), (1100, 8, 0),
                                                                (64, 8, 64), (128, 4, 128)), (0, 1), (0, 1, 5)):
        rows.append(request(npix=npix, num_cu=cu, L=L, NDIR=n, slots=slots, sw_any=any_, sw_wg_per_cu=wg))
        caps.append((cu if cu > 0 else 256) * (wg if wg > 0 else (64 if slots and not any_ else 768)))
    turns = set()
    for q, cap, g in zip(rows, caps, ask(lib, rows)):
        npix = q[0]
        assert g["family"] != REFUSE and g["per_wave"] >= 1
        waves = -(-npix // g["per_wave"])
        assert 1 <= g["grid"] <= cap and g["grid"] == min(-(-waves // 4), cap), (q, g)
        assert (g["grid"] - 1) * 4 * g["per_wave"] < npix  # every workgroup has a pixel
        turns.add(min(3, -(-npix // (g["grid"] * 4 * g["per_wave"]))))
    assert turns == {1, 2, 3}  # one turn of the grid-stride loop, two, more
    # the capped volumes of tests/test_gpu_wta_consensus_crafted.py take several turns on any device up to 304 CUs
    for kw in (dict(npix=130 * 40, L=256, NDIR=8), dict(npix=257 * 45, L=64, NDIR=4), dict(npix=130 * 40, L=100, NDIR=8), dict(npix=130 * 40, slots=64, NDIR=8)):
        for cu in (1, 256, 304):
            g = ask(lib, [request(num_cu=cu, sw_wg_per_cu=1, **kw)])[0]
            assert kw["npix"] > g["grid"] * 4 * g["per_wave"], (kw, cu, g)


def test_a_choice_is_a_function_of_the_request_alone(lib):
    rows = list(dict.fromkeys(request(L=L, Lk=Lk, NDIR=n, npix=npix, sw_any=a, num_cu=cu, slots=s)
                              for Lk in (63, 64, 128, 192, 256, 320, 384, 512, 768, 1024, 1100) for L in (Lk, max(1, Lk - 1))
                              for n, npix, a, cu, s in itertools.product((1, 4, 5, 8), (3, 3201, FULL_HD), (0, 1), (0, 256), (0, 64, 128))))
    key = lambda g: tuple(g[k] for k in OUT)
    first = dict(zip(rows, map(key, ask(lib, rows))))
    assert dict(zip(rows, map(key, ask(lib, rows)))) == first            # the same bytes, asked again
    shuffled = rows[:]
    random.Random(7).shuffle(shuffled)
    assert dict(zip(shuffled, map(key, ask(lib, shuffled)))) == first    # ... in another order, behind other requests
    for q in shuffled[:64]:                                              # ... and one at a time
        assert key(ask(lib, [q])[0]) == first[q]
    # the hull flag changes no choice today
    assert [key(g) for g in ask(lib, [request(L=70, Lk=128, hull=h) for h in (0, 1)])] == [key(ask(lib, [request(L=70, Lk=128)])[0])] * 2


def test_the_planner_reads_nothing_but_its_argument():
    """no getenv, no global, no device: the function's text in the header names only its request, its constants and the standard library"""
    src = open(os.path.join(CSRC, "mgm_planner.h")).read()
    body = src[src.index("inline ConsensusChoice plan_wta_consensus"):]
    body = body[:body.index("\n}\n") + 3]
    assert "getenv" not in body and "static " not in body and "hip" not in body.lower().replace("hipcc", "")
    idents = set(re.findall(r"\b[A-Za-z_]\w*\b", re.sub(r"//[^\n]*", "", body)))
    allowed = {"inline", "ConsensusChoice", "plan_wta_consensus", "const", "ConsensusRequest", "q", "c", "if", "return", "else", "long", "int", "switch", "case",
               "break", "default", "std", "min", "cus", "cap", "lpl", "ppw", "waves", "kMaxDirs", "kConsensusWgPerCu", "kConsensusRelWgPerCu",
               "kConsensusAny", "kConsensusRel", "kConsensusStream", "npix", "NDIR", "sw_wg_per_cu", "slots", "L", "Lk", "num_cu", "sw_any",
               "family", "per_wave", "SPL", "LPL", "PPW", "MAXD", "grid"}
    assert idents <= allowed, sorted(idents - allowed)
