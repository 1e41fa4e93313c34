"""plan_wta, plan_wta_right and plan_wta_rel (mgm_amd/csrc/mgm_planner.h) on the host: the instance and the grid every winner
search runs on are what the launchers chose before the planner existed (tests/wta_plan_model.py), the choices DESIGN.md and
the launchers' comments name come out literally, every instance of the launch tables is reachable, and a choice is a function
of the request's bytes alone."""
import ctypes as C
import itertools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import wta_plan_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mgm_amd", "csrc")

FULL_HD = 1920 * 1080
STRIDES = (1, 63, 64, 65, 100, 128, 192, 256, 384, 512, 513, 768, 1000, 1024, 1025, 2048, 2049)
NPIX = (1, 3, 4, 15, 17, 3201, FULL_HD)  # not divisible by 2, by 4, by 768/L; one workgroup, several, more than any cap
SWITCHES = dict(sw_prune=1, sw_prune_ppw=2, sw_prune_wg=0, sw_wg_per_cu=0, sw_packed=1, sw_wide4=1, sw_quad=1)  # the defaults


def dtype_of(fields, wide):
    return np.dtype([(f, "<i8" if f in wide else "<i4") for f in fields])


WTA_T = dtype_of(M.WTA_FIELDS, ("npix",))
RIGHT_T = dtype_of(M.RIGHT_FIELDS, ())
REL_T = dtype_of(M.REL_FIELDS, ("npix", "num_cu"))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("wtaplan") / "libwta_plan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "wta_plan_harness.cc"), "-o", so],
                   check=True)
    lib = C.CDLL(so)
    assert (lib.wta_request_bytes(), lib.wta_right_request_bytes(), lib.wta_rel_request_bytes()) == (WTA_T.itemsize, RIGHT_T.itemsize, REL_T.itemsize)
    return lib


def ask(lib, kind, rows):
    """The planner's choices for `rows` (tuples in field order), as tuples in the order of the model's."""
    fn, t, nout = {"wta": (lib.wta_plan, WTA_T, len(M.WTA_OUT)), "right": (lib.wta_right_plan, RIGHT_T, len(M.RIGHT_OUT)),
                   "rel": (lib.wta_rel_plan, REL_T, len(M.REL_OUT))}[kind]
    a = np.array(rows, dtype=np.int64)
    req = np.zeros(len(rows), dtype=t)
    for k, f in enumerate(t.names):
        req[f] = a[:, k]
    out = np.zeros((len(rows), nout), dtype=np.int64)
    fn(req.ctypes.data_as(C.c_void_p), C.c_int(len(rows)), out.ctypes.data_as(C.c_void_p))
    return [tuple(r) for r in out.tolist()]


def wta_request(**kw):
    """A cfg3-like search (1920x1080, 256 labels, 8 passes, one-byte compact costs, vfit) right behind its launch, which wrote
    no minima unless `last_min` says so; `kw` changes it.  lpl and padded follow from L and Lreal unless given."""
    q = dict(npix=FULL_HD, L=256, Lreal=None, NDIR=8, lpl=None, cbytes=1, compact=1, refine=1, want_S=0, window=0, ragged=0, in_last_run=1, last_min=0,
             lr_is_last=1, pix0_zero=1, padded=None, nvol_mod32=0, num_cu=256, **SWITCHES)
    for k, v in kw.items():
        assert k in q, k
        q[k] = v
    if q["Lreal"] is None:
        q["Lreal"] = q["L"]
    if q["lpl"] is None:
        q["lpl"] = M.pass_lpl(q["L"])
    if q["padded"] is None:
        q["padded"] = int(q["Lreal"] < q["L"])
    return tuple(q[f] for f in M.WTA_FIELDS)


def right_request(**kw):
    q = dict(L=256, Lk=None, nx=1920, ny=1080, vnx=1920, dmin=-255, dmax=None, num_cu=256, sw_right_seg=0, sw_right_any=0)
    for k, v in kw.items():
        assert k in q, k
        q[k] = v
    if q["Lk"] is None:
        q["Lk"] = q["L"]
    if q["dmax"] is None:
        q["dmax"] = q["dmin"] + q["L"] - 1
    return tuple(q[f] for f in M.RIGHT_FIELDS)


def wta_sweep():
    """The cross the three launchers are held to, one request per row.  The whole cross of shapes runs behind a launch that
    wrote minima and behind one that did not; every switch, every flag of "what the last launch left" and the device sizes are
    then flipped one at a time against the same cross at four of the seven pixel counts."""
    at = {f: k for k, f in enumerate(M.WTA_FIELDS)}
    shape = [at[f] for f in "npix NDIR compact cbytes window ragged want_S refine".split()]
    cross = lambda npix: np.array([(n, d) + c + r for n, d, c, r in itertools.product(npix, range(1, 9), ((1, 1), (1, 2), (0, 1)),
                                                                                     itertools.product((0, 1), (0, 1), (0, 1), (0, 1, 2)))], dtype=np.int64)
    whole, part = cross(NPIX), cross((3, 4, 3201, FULL_HD))
    variants = [(dict(last_min=1), whole), (dict(last_min=0), whole), (dict(last_min=1, padded=0), part), (dict(last_min=1, padded=1), part)]
    variants += [(dict(last_min=1, **{k: v}), part) for k, v in (("num_cu", 0), ("num_cu", 1), ("num_cu", 304), ("sw_prune", 0), ("sw_prune_ppw", 1),
                                                                ("sw_prune_wg", 7), ("sw_wg_per_cu", 5), ("sw_packed", 0), ("sw_wide4", 0), ("sw_quad", 0),
                                                                ("in_last_run", 0), ("lr_is_last", 0), ("pix0_zero", 0), ("nvol_mod32", 16))]
    blocks = []
    for v, x in variants:
        for L in STRIDES:
            for Lreal in {L, max(1, L - 1), 151 if L == 192 else L}:
                rows = np.tile(np.array(wta_request(L=L, Lreal=Lreal, **v), dtype=np.int64), (len(x), 1))
                rows[:, shape] = x
                blocks.append(rows)
    return np.concatenate(blocks)


def test_the_sweep_selects_what_the_launchers_selected(lib, reached):
    rows = wta_sweep()
    got = ask(lib, "wta", rows)
    for q, g in zip(rows.tolist(), got):
        want = M.wta(q)
        assert g == want, (dict(zip(M.WTA_FIELDS, q)), dict(zip(M.WTA_OUT, g)), dict(zip(M.WTA_OUT, want)))
    reached["wta"] |= {M.instance("wta", g) for g in set(got)}

    rows = []
    for L, pad in itertools.product((1, 63, 64, 100, 128, 151, 192, 256, 384, 512, 513, 768, 1024, 1025, 2049), (0, 1)):
        Lk = {151: 192}.get(L, (L + 63) // 64 * 64) if pad else L
        for (nx, ny, vnx), cu, seg, force in itertools.product(((1, 1, 1), (17, 3, 23), (96, 34, 90), (1920, 1080, 1920), (1920, 1080, 2000), (40000, 60000, 40000)),
                                                               (0, 1, 256, 304), (0, 1, 100), (0, 1)):
            rows.append(right_request(L=L, Lk=Lk, nx=nx, ny=ny, vnx=vnx, num_cu=cu, sw_right_seg=seg, sw_right_any=force))
    rows += [right_request(L=0), right_request(L=256, Lk=192), right_request(nx=0), right_request(ny=0), right_request(vnx=0), right_request(dmax=7)]
    got = ask(lib, "right", rows)
    for q, g in zip(rows, got):
        want = M.wta_right(q)
        assert g == want, (dict(zip(M.RIGHT_FIELDS, q)), dict(zip(M.RIGHT_OUT, g)), dict(zip(M.RIGHT_OUT, want)))
    reached["right"] |= {M.instance("right", g) for g in got}

    rows = list(itertools.product((1, 15, 16, 17, 3201, FULL_HD, 1 << 32), (0, 1, 256, 304), (64, 128), (1, 2, 4)))
    got = ask(lib, "rel", rows)
    for q, g in zip(rows, got):
        assert g == M.wta_rel(q), (q, g)
    reached["rel"] |= {M.instance("rel", g) for g in got}


# (what, the request, the instance) -- from DESIGN.md and the comments of the launch tables
NAMED = [
    ("cfg3: 256 labels, 8 passes, unpruned", dict(), "k_wta<4,3,true,8,1>"),
    ("cfg3, its launch wrote the chunk minima", dict(last_min=1), "k_wta_pruned<2,8,true>"),
    ("... MGM_HIP_WTA_PRUNE=0", dict(last_min=1, sw_prune=0), "k_wta<4,3,true,8,1>"),
    ("... wta_prune_ppw=1", dict(last_min=1, sw_prune_ppw=1), "k_wta_pruned<1,8,true>"),
    ("pruned, 4 passes", dict(last_min=1, NDIR=4), "k_wta_pruned<2,4,true>"),
    ("... wta_prune_ppw=1", dict(last_min=1, NDIR=4, sw_prune_ppw=1), "k_wta_pruned<1,4,true>"),
    ("pruned, 2 passes: the guarded 4-direction instance", dict(last_min=1, NDIR=2), "k_wta_pruned<1,4,false>"),
    ("pruned, 6 passes: the guarded 8-direction instance", dict(last_min=1, NDIR=6), "k_wta_pruned<1,8,false>"),
    ("a window is never pruned", dict(last_min=1, window=1), "k_wta<4,3,true,8,1>"),
    ("nor a search that writes S", dict(last_min=1, want_S=1), "k_wta<4,3,true,8,1>"),
    ("nor rows of a volume (mgm_wta_rows_dev)", dict(last_min=1, in_last_run=0), "k_wta<4,3,true,8,1>"),
    ("minima at an Lr stride that is no multiple of 32: refused", dict(last_min=1, nvol_mod32=16), None),
    ("256 labels, 4 passes: twice the slabs", dict(NDIR=4), "k_wta<4,6,true,4,1>"),
    ("... wta_wide4=0", dict(NDIR=4, sw_wide4=0), "k_wta<4,3,true,8,1>"),
    ("200 labels on a stride of 200", dict(L=200), "k_wta<4,1,false,8,1>"),
    ("128 labels, even pixel count: two pixels per slab", dict(L=128), "k_wta<4,2,true,8,2>"),
    ("... 4 passes", dict(L=128, NDIR=4), "k_wta<4,4,true,4,2>"),
    ("128 labels, odd pixel count: one pixel per slab", dict(L=128, npix=3201), "k_wta<2,4,true,8,1>"),
    ("... 4 passes", dict(L=128, npix=3201, NDIR=4), "k_wta<2,8,true,4,1>"),
    ("128 labels, wta_packed=0", dict(L=128, sw_packed=0), "k_wta<2,4,true,8,1>"),
    ("100 labels on a stride of 100", dict(L=100), "k_wta<2,1,false,8,1>"),
    ("64 labels: four pixels per slab", dict(L=64), "k_wta<4,2,true,8,4>"),
    ("... 4 passes", dict(L=64, NDIR=4), "k_wta<4,4,true,4,4>"),
    ("64 labels, a pixel count that is no multiple of 4", dict(L=64, npix=FULL_HD + 2), "k_wta<1,4,true,8,1>"),
    ("... 4 passes", dict(L=64, npix=FULL_HD + 2, NDIR=4), "k_wta<1,8,true,4,1>"),
    ("63 labels", dict(L=63), "k_wta<1,1,false,8,1>"),
    ("192 labels: four pixels per three slabs", dict(L=192), "k_wta_q<192,8>"),
    ("... 4 passes", dict(L=192, NDIR=4), "k_wta_q<192,4>"),
    ("192 labels with a window leaves k_wta_q", dict(L=192, window=1), "k_wta<3,2,true,8,1>"),
    ("... 4 passes", dict(L=192, window=1, NDIR=4), "k_wta<3,4,true,4,1>"),
    ("192 labels, wta_quad=0", dict(L=192, sw_quad=0), "k_wta<3,2,true,8,1>"),
    ("192 labels, a pixel count that is no multiple of 4", dict(L=192, npix=3201), "k_wta<3,2,true,8,1>"),
    ("151 labels padded to 192: the exact instance of the stride", dict(L=192, Lreal=151), "k_wta<3,2,true,8,1>"),
    ("151 labels on their own stride", dict(L=151), "k_wta<3,1,false,8,1>"),
    ("384 labels: two pixels per three slabs", dict(L=384), "k_wta_q<384,8>"),
    ("... 4 passes", dict(L=384, NDIR=4), "k_wta_q<384,4>"),
    ("384 labels, ragged", dict(L=384, ragged=1), "k_wta<6,1,true,8,1>"),
    ("... 4 passes", dict(L=384, ragged=1, NDIR=4), "k_wta<6,2,true,4,1>"),
    ("320 labels: the next width built", dict(L=320), "k_wta<6,1,false,8,1>"),
    ("512 labels", dict(L=512), "k_wta<8,1,true,8,1>"),
    ("... 4 passes", dict(L=512, NDIR=4), "k_wta<8,2,true,4,1>"),
    ("448 labels", dict(L=448), "k_wta<8,1,false,8,1>"),
    ("768 labels", dict(L=768), "k_wta<12,1,true,8,1>"),
    ("... 4 passes: no wider instance beyond 512 labels", dict(L=768, NDIR=4), "k_wta<12,1,true,8,1>"),
    ("513 labels", dict(L=513), "k_wta<12,1,false,8,1>"),
    ("1024 labels", dict(L=1024), "k_wta<16,1,true,8,1>"),
    ("1000 labels", dict(L=1000), "k_wta<16,1,false,8,1>"),
    ("1025 labels", dict(L=1025), "k_wta<24,1,false,8,1>"),
    ("1536 labels: guarded all the same", dict(L=1536), "k_wta<24,1,false,8,1>"),
    ("2048 labels", dict(L=2048), "k_wta<32,1,false,8,1>"),
    ("above 2048 labels", dict(L=2049), "k_wta_any"),
]
NAMED_RIGHT = [
    ("64 labels", dict(L=64), "k_wta_right<1,2>"), ("128 labels", dict(L=128), "k_wta_right<2,2>"), ("192 labels", dict(L=192), "k_wta_right<3,2>"),
    ("151 labels padded to 192", dict(L=151, Lk=192), "k_wta_right<3,2>"), ("256 labels", dict(L=256), "k_wta_right<4,2>"),
    ("384 labels", dict(L=384), "k_wta_right<6,1>"), ("512 labels", dict(L=512), "k_wta_right<8,1>"), ("768 labels", dict(L=768), "k_wta_right<12,1>"),
    ("1024 labels", dict(L=1024), "k_wta_right<16,1>"),
    ("a stride of 100: the diagonal walk", dict(L=100), "k_wta_right_any"), ("a stride of 320", dict(L=320), "k_wta_right_any"),
    ("MGM_HIP_WTA_RIGHT_ANY=1", dict(sw_right_any=1), "k_wta_right_any"),
    ("a label range that is not the volume's: refused", dict(dmax=7), None),
]
NAMED_REL = [((FULL_HD, 256, slots, cb), "k_wta_rel<%d,%d>" % (slots // 16, cb)) for slots in (64, 128) for cb in (1, 2, 4)]


@pytest.fixture(scope="module")
def reached():
    return dict(wta=set(), right=set(), rel=set())


def test_the_named_choices(lib, reached):
    got = ask(lib, "wta", [wta_request(**kw) for _, kw, _ in NAMED])
    for (what, kw, want), g in zip(NAMED, got):
        assert M.instance("wta", g) == want, (what, kw, dict(zip(M.WTA_OUT, g)))
    named = {"wta": {w for _, _, w in NAMED}}
    # the grids of the headline: 8 pixels per workgroup and iteration against 64 workgroups per CU; 4 against 768
    assert got[1][M.WTA_OUT.index("grid")] == 256 * 64 and got[1][M.WTA_OUT.index("prune")] == 1
    assert got[0][M.WTA_OUT.index("grid")] == 256 * 768 and got[0][M.WTA_OUT.index("prune")] == 0
    got = ask(lib, "right", [right_request(**kw) for _, kw, _ in NAMED_RIGHT])
    for (what, kw, want), g in zip(NAMED_RIGHT, got):
        assert M.instance("right", g) == want, (what, kw, dict(zip(M.RIGHT_OUT, g)))
    named["right"] = {w for _, _, w in NAMED_RIGHT}
    got = ask(lib, "rel", [q for q, _ in NAMED_REL])
    for (q, want), g in zip(NAMED_REL, got):
        assert M.instance("rel", g) == want, (q, g)
    named["rel"] = {w for _, w in NAMED_REL}

    # every instance of the launch tables is named at least once, and nothing is named that the tables do not hold
    tables = launch_tables()
    assert {k: len(v) for k, v in tables.items()} == dict(wta=39, right=9, rel=6)
    for kind in tables:
        assert named[kind] - {None} == tables[kind], (kind, sorted(tables[kind] ^ (named[kind] - {None})))
        reached[kind] |= named[kind]


def launch_tables():
    """The instantiations of the three launch tables of mgm_wta.hip, as instance() spells them."""
    src = open(os.path.join(CSRC, "mgm_wta.hip")).read()
    b = lambda v: "true" if int(v) else "false"
    t = dict(wta={"k_wta_any"}, right={"k_wta_right_any"}, rel=set())
    assert "hipLaunchKernelGGL(k_wta_any," in src and "hipLaunchKernelGGL(k_wta_right_any," in src
    for name, args in re.findall(r"\bWTA(|_Q|_PRUNED|_RIGHT|_REL)\((\d+(?:, \d+)*)\)", src):
        a = args.split(", ")
        if name == "":
            t["wta"].add("k_wta<%s,%s,%s,%s,%s>" % (a[0], a[1], b(a[2]), a[3], a[4]))
        elif name == "_Q":
            t["wta"].add("k_wta_q<%d,%s>" % (64 * int(a[0]), a[1]))
        elif name == "_PRUNED":
            t["wta"].add("k_wta_pruned<%s,%s,%s>" % (a[0], a[1], b(a[2])))
        elif name == "_RIGHT":
            t["right"].add("k_wta_right<%s,%s>" % (a[0], a[1]))
        else:
            t["rel"].add("k_wta_rel<%s,%s>" % (a[0], a[1]))
    return t


def test_sweep_and_table_reach_the_launch_tables_and_nothing_else(lib, reached):
    """The distinct choices of the two tests above (run here if this test was selected alone) against the instantiations."""
    if not (reached["wta"] and reached["right"] and reached["rel"]):
        test_the_sweep_selects_what_the_launchers_selected(lib, reached)
        test_the_named_choices(lib, reached)
    tables = launch_tables()
    for kind in tables:
        assert reached[kind] - {None} == tables[kind], (kind, sorted(tables[kind] ^ (reached[kind] - {None})))


def test_the_pruned_instances_of_the_gpu_test(lib):
    """tests/test_gpu_wta_pruned_instances.py reaches the six instances through NDIR and wta_prune_ppw alone."""
    cases = {(8, 2): "k_wta_pruned<2,8,true>", (8, 1): "k_wta_pruned<1,8,true>", (4, 2): "k_wta_pruned<2,4,true>", (4, 1): "k_wta_pruned<1,4,true>",
             (2, 2): "k_wta_pruned<1,4,false>", (6, 2): "k_wta_pruned<1,8,false>"}
    got = ask(lib, "wta", [wta_request(last_min=1, NDIR=n, sw_prune_ppw=p, npix=96 * 34, num_cu=256) for n, p in cases])
    assert [M.instance("wta", g) for g in got] == list(cases.values())


def test_a_choice_is_a_function_of_the_request_alone(lib):
    rows = list(dict.fromkeys(wta_request(L=L, Lreal=Lr, NDIR=n, npix=npix, last_min=m, window=w)
                              for L, n, npix, m, w in itertools.product(STRIDES, (1, 4, 8), (3, 3201, FULL_HD), (0, 1), (0, 1)) for Lr in (L, max(1, L - 1))))
    first = dict(zip(rows, ask(lib, "wta", rows)))
    assert dict(zip(rows, ask(lib, "wta", rows))) == first                 # the same bytes, asked again
    shuffled = rows[:]
    random.Random(7).shuffle(shuffled)
    assert dict(zip(shuffled, ask(lib, "wta", shuffled))) == first         # ... in another order, behind other requests
    for q in shuffled[:64]:                                                # ... and one at a time
        assert ask(lib, "wta", [q]) == [first[q]]
