"""plan_wta_runnerup (mgm_amd/csrc/mgm_planner.h) on the host: every instance of the launch table of mgm_wta.hip is reachable
and nothing else is chosen, strides outside the table and the forcing switch go to the generic kernel, bad requests are
refused, the grid stays between 1 and its cap, and a choice is a function of the request's bytes alone."""
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

FIELDS = ("npix", "L", "Lk", "NDIR", "num_cu", "sw_any", "sw_wg_per_cu")  # RunnerupRequest, in memory order
REQ_T = np.dtype([(f, "<i8" if f == "npix" else "<i4") for f in FIELDS])
OUT = ("family", "LPL", "PPW", "MAXD", "grid")
REFUSE, STREAM, ANY = 0, 1, 2
FULL_HD = 1920 * 1080
STREAM_LPL = (1, 2, 3, 4, 6, 8, 12, 16)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("runnerupplan") / "librunnerup_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "runnerup_plan_harness.cc"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    lib.runnerup_wg_per_cu.restype = C.c_longlong
    assert lib.runnerup_request_bytes() == REQ_T.itemsize and lib.runnerup_choice_bytes() == 8 + 4 * 4
    return lib


def request(**kw):
    q = dict(npix=FULL_HD, L=256, Lk=None, NDIR=8, num_cu=256, sw_any=0, sw_wg_per_cu=0)
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
    lib.runnerup_plan(req.ctypes.data_as(C.c_void_p), C.c_int(len(rows)), out.ctypes.data_as(C.c_void_p))
    return [dict(zip(OUT, r)) for r in out.tolist()]


def instance(c):
    if c["family"] == STREAM:
        return "k_wta_runnerup<%d,%d,%d>" % (c["LPL"], c["PPW"], c["MAXD"])
    return {ANY: "k_wta_runnerup_any", REFUSE: None}[c["family"]]


def launch_table():
    src = open(os.path.join(CSRC, "mgm_wta.hip")).read()
    assert "hipLaunchKernelGGL(k_wta_runnerup_any," in src
    return {"k_wta_runnerup<%s,%s,%s>" % a for a in re.findall(r"\bRUNNERUP\((\d+), (\d+), (\d+)\)", src)} | {"k_wta_runnerup_any"}


def test_every_instance_of_the_table_is_reachable_and_nothing_else(lib):
    rows = [request(L=L, Lk=Lk, NDIR=n, npix=npix) for Lk in [64 * k for k in range(1, 20)] + [63, 65, 100, 200, 1100, 2049]
            for L in {Lk, max(1, Lk - 13), 1} for n in range(1, 9) for npix in (1, 5, 3201, FULL_HD)]
    reached = {instance(c) for c in ask(lib, rows)}
    table = launch_table()
    assert len(table) == 15
    assert reached == table, sorted(reached ^ table)


# (what, the request, the instance): the pixels per wave are those of the k_wta instances without a padding lane
NAMED = [
    ("256 labels, 8 passes", dict(), "k_wta_runnerup<4,3,8>"), ("256 labels, 4 passes: twice the slabs", dict(NDIR=4), "k_wta_runnerup<4,6,4>"),
    ("64 labels", dict(L=64), "k_wta_runnerup<1,4,8>"), ("... 3 passes", dict(L=64, NDIR=3), "k_wta_runnerup<1,8,4>"),
    ("128 labels", dict(L=128), "k_wta_runnerup<2,4,8>"), ("... 1 pass", dict(L=128, NDIR=1), "k_wta_runnerup<2,8,4>"),
    ("192 labels", dict(L=192), "k_wta_runnerup<3,2,8>"), ("... 4 passes", dict(L=192, NDIR=4), "k_wta_runnerup<3,4,4>"),
    ("151 labels padded to 192", dict(L=151, Lk=192), "k_wta_runnerup<3,2,8>"), ("65 labels padded to 128", dict(L=65, Lk=128, NDIR=4), "k_wta_runnerup<2,8,4>"),
    ("384 labels", dict(L=384), "k_wta_runnerup<6,1,8>"), ("... 4 passes", dict(L=384, NDIR=4), "k_wta_runnerup<6,2,4>"),
    ("512 labels", dict(L=512), "k_wta_runnerup<8,1,8>"), ("... 4 passes", dict(L=512, NDIR=4), "k_wta_runnerup<8,2,4>"),
    ("768 labels", dict(L=768), "k_wta_runnerup<12,1,8>"), ("... 4 passes: no wider instance", dict(L=768, NDIR=4), "k_wta_runnerup<12,1,8>"),
    ("1024 labels", dict(L=1024), "k_wta_runnerup<16,1,8>"), ("... 4 passes", dict(L=1024, NDIR=4), "k_wta_runnerup<16,1,8>"),
    ("a stride of 63", dict(L=63), "k_wta_runnerup_any"), ("a stride of 65", dict(L=65), "k_wta_runnerup_any"),
    ("a stride of 320: no instance", dict(L=320), "k_wta_runnerup_any"), ("1100 labels", dict(L=1100), "k_wta_runnerup_any"),
    ("1100 labels padded to 1152", dict(L=1100, Lk=1152), "k_wta_runnerup_any"), ("2048 labels", dict(L=2048), "k_wta_runnerup_any"),
    ("MGM_HIP_WTA_RUNNERUP_ANY=1", dict(sw_any=1), "k_wta_runnerup_any"), ("... at 64 labels, 4 passes", dict(L=64, NDIR=4, sw_any=1), "k_wta_runnerup_any"),
    ("no label", dict(L=0, Lk=64), None), ("a stride below the labels", dict(L=256, Lk=192), None), ("no pixel", dict(npix=0), None),
    ("a negative pixel count", dict(npix=-4), None), ("no pass", dict(NDIR=0), None), ("nine passes", dict(NDIR=9), None),
    ("refused even when forced", dict(L=0, Lk=64, sw_any=1), None), ("a negative cap", dict(sw_wg_per_cu=-1), None),
]


def test_the_named_choices(lib):
    got = ask(lib, [request(**kw) for _, kw, _ in NAMED])
    for (what, kw, want), g in zip(NAMED, got):
        assert instance(g) == want, (what, kw, g)
        if want is None:
            assert g == dict(family=0, LPL=0, PPW=0, MAXD=0, grid=0), (what, g)
        if want == "k_wta_runnerup_any":
            assert (g["LPL"], g["PPW"], g["MAXD"]) == (0, 0, 0)
    assert {w for _, _, w in NAMED} - {None} == launch_table()


def test_the_grid_is_at_least_one_and_at_most_the_cap(lib):
    """exactly the waves the pixels need (a wave takes PPW pixels per turn, the generic kernel one), four per workgroup, at
    most the cap: 768 workgroups per CU (plan_wta's figure for one pixel per slab) or what MGM_HIP_WTA_RUNNERUP_WG says"""
    per_cu = lib.runnerup_wg_per_cu()
    assert per_cu == 768
    rows, caps = [], []
    for npix, cu, (L, n), any_, wg in itertools.product((1, 3, 4, 5, 33, 3201, FULL_HD, 1 << 33), (0, 1, 256, 304),
                                                        ((1, 8), (64, 8), (64, 4), (100, 8), (256, 8), (256, 3), (1024, 8), (1100, 8)), (0, 1), (0, 1, 5)):
        rows.append(request(npix=npix, num_cu=cu, L=L, NDIR=n, sw_any=any_, sw_wg_per_cu=wg))
        caps.append((cu if cu > 0 else 256) * (wg if wg > 0 else per_cu))
    turns = set()
    for q, cap, g in zip(rows, caps, ask(lib, rows)):
        npix = q[0]
        assert g["family"] != REFUSE
        per_wave = g["PPW"] if g["family"] == STREAM else 1
        waves = -(-npix // per_wave)
        assert 1 <= g["grid"] <= cap and g["grid"] == min(-(-waves // 4), cap), (q, g)
        turns.add(min(3, -(-npix // (g["grid"] * 4 * per_wave))))
    assert turns == {1, 2, 3}  # one turn of the grid-stride loop, two, more
    # the two capped volumes of tests/test_gpu_wta_runnerup.py take several turns on any device up to 304 CUs
    for kw in (dict(npix=130 * 40, L=256, NDIR=8), dict(npix=257 * 45, L=64, NDIR=4), dict(npix=130 * 40, L=300, NDIR=8)):
        for cu in (1, 256, 304):
            g = ask(lib, [request(num_cu=cu, sw_wg_per_cu=1, **kw)])[0]
            assert kw["npix"] > g["grid"] * 4 * max(1, g["PPW"]), (kw, cu, g)


def test_a_choice_is_a_function_of_the_request_alone(lib):
    rows = list(dict.fromkeys(request(L=L, Lk=Lk, NDIR=n, npix=npix, sw_any=a, num_cu=cu)
                              for Lk in (63, 64, 128, 192, 256, 320, 384, 512, 768, 1024, 1100) for L in (Lk, max(1, Lk - 1))
                              for n, npix, a, cu in itertools.product((1, 4, 5, 8), (3, 3201, FULL_HD), (0, 1), (0, 256))))
    key = lambda g: tuple(g[k] for k in OUT)
    first = dict(zip(rows, map(key, ask(lib, rows))))
    assert dict(zip(rows, map(key, ask(lib, rows)))) == first            # the same bytes, asked again
    shuffled = rows[:]
    random.Random(7).shuffle(shuffled)
    assert dict(zip(shuffled, map(key, ask(lib, shuffled)))) == first    # ... in another order, behind other requests
    for q in shuffled[:64]:                                              # ... and one at a time
        assert key(ask(lib, [q])[0]) == first[q]
