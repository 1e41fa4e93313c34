"""plan_wta_prune (mgm_amd/csrc/mgm_planner.h) on the host: the launch writes chunk minima and the pruned winner search runs
for exactly the launches the 256-label compact unweighted kernels take and the searches that can use them, and for nothing else."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgm_amd", "csrc")

DENSE_FIELDS = ("nx ny L nb first count layout_ndir MGM fh wmode use_c8 cb first_build ragged lines2 lpl ns devtools num_cu xcc_mask "
                "subv deep wg_per_cu strips xcdq xcdq_k one_queue w2 oneb").split()
CALL_FIELDS = "enabled search_follows want_S refine slot0 nslots Lreal stride_mod32".split()
PRUNE_FIELDS = ("enabled search_follows want_S refine first count slot0 nslots L Lreal ragged R2 subv tags w2 wk lpl use_c8 cb "
                "stride_mod32").split()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("prune") / "libprune_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "prune_harness.cc"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    assert lib.prune_request_fields() == len(PRUNE_FIELDS) and lib.dense_request_fields() == len(DENSE_FIELDS)
    return lib


def ints(v):
    return (C.c_int * len(v))(*v)


def launch(lib, **kw):
    """The decision for a cfg3-like launch (1920x1080x256, 8 directions, TSGM 3, FH, one-byte costs) with `kw` changed."""
    d = dict(nx=1920, ny=1080, L=256, nb=12, first=0, count=8, layout_ndir=8, MGM=3, fh=1, wmode=0, use_c8=1, cb=1, first_build=0, ragged=0,
             lines2=15, lpl=4, ns=1, devtools=0, num_cu=256, xcc_mask=255, subv=1, deep=-1, wg_per_cu=0, strips=-1, xcdq=-1, xcdq_k=-1,
             one_queue=-1, w2=1, oneb=1)
    c = dict(enabled=1, search_follows=1, want_S=0, refine=1, slot0=0, nslots=None, Lreal=None, stride_mod32=0)
    for k, v in kw.items():
        assert k in d or k in c, k
        (d if k in d else c)[k] = v
    if c["nslots"] is None:
        c["nslots"] = c["slot0"] + d["count"]
    if c["Lreal"] is None:
        c["Lreal"] = d["L"]
    r = lib.prune_for_launch(ints([d[f] for f in DENSE_FIELDS]), ints([c[f] for f in CALL_FIELDS]))
    assert r >= 0, "the plan failed"
    return bool(r)


def test_opts_in_for_what_cfg3_and_cfg3h_run(lib):
    for nb in (1, 2, 3, 12, 16):          # any batch size: shallow and deep rings, with and without queues, one or two bands per CU
        for fh in (0, 1):
            for mgm in (1, 3, 4):
                assert launch(lib, nb=nb, fh=fh, MGM=mgm)
    assert launch(lib, fh=0, MGM=2)         # Hirschmueller with TSGM 2 publishes E too
    assert launch(lib, count=4, layout_ndir=4)
    assert launch(lib, refine=0)
    for sw in (dict(deep=0), dict(deep=1), dict(xcdq=0), dict(xcdq=1), dict(oneb=0), dict(wg_per_cu=1), dict(wg_per_cu=2), dict(strips=1), dict(xcc_mask=15)):
        assert launch(lib, nb=1, **sw), sw
    assert launch(lib, nx=96, ny=34, nb=1) and launch(lib, nx=96, ny=34, nb=3, fh=0)


def test_opts_out(lib):
    assert not launch(lib, enabled=0)                         # MGM_HIP_WTA_PRUNE=0
    assert not launch(lib, fh=1, MGM=2)                       # FH with TSGM 2: slabs of T, not E
    assert not launch(lib, wmode=1, ns=2) and not launch(lib, wmode=2, ns=2)   # two-valued weights, general weights
    assert not launch(lib, use_c8=0) and not launch(lib, cb=2)  # fp32 costs, two-byte costs
    assert not launch(lib, first_build=1, lines2=0)           # the first build (k_pass)
    assert not launch(lib, Lreal=200)                         # a padded label count
    assert not launch(lib, ragged=1)
    for L, lpl, nb in ((128, 2, 1), (128, 2, 16), (64, 1, 16), (192, 3, 1), (384, 6, 1), (512, 8, 1)):   # other label counts, volumes sharing waves
        assert not launch(lib, L=L, lpl=lpl, nb=nb), L
    assert not launch(lib, want_S=1)
    for refine in (2, 3, 4):                                  # parabola, cubic, parabolaOCV: a second kernel on S
        assert not launch(lib, refine=refine)
    assert not launch(lib, search_follows=0)                  # direction-sharded / multi-device building blocks
    assert not launch(lib, first=2, count=2) and not launch(lib, first=0, count=4, slot0=2, nslots=8)   # a subset of the passes; other slots
    assert not launch(lib, stride_mod32=16)


def test_is_a_function_of_the_request_alone(lib):
    """Every field takes part by value: the same request gives the same answer, and flipping any single gate of an opted-in
    request opts out."""
    base = dict(enabled=1, search_follows=1, want_S=0, refine=1, first=0, count=8, slot0=0, nslots=8, L=256, Lreal=256, ragged=0, R2=15, subv=1,
                tags=1, w2=0, wk=0, lpl=4, use_c8=1, cb=1, stride_mod32=0)
    ask = lambda q: bool(lib.prune_decision(ints([q[f] for f in PRUNE_FIELDS])))
    assert ask(base) and ask(dict(base))
    flips = dict(enabled=0, search_follows=0, want_S=1, refine=2, first=1, slot0=1, nslots=9, L=128, Lreal=255, ragged=1, R2=0, subv=2, tags=0, w2=1,
                 wk=1, lpl=2, use_c8=0, cb=2, stride_mod32=1)
    for k, v in flips.items():
        assert not ask(dict(base, **{k: v})), k
