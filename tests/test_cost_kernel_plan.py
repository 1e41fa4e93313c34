"""plan_cost_kernel and cost_request (mgm_amd/csrc/mgm_fillplan.h) on the host: no device.

tests/cost_kernel_harness.cc is compiled with plain g++ and no ROCm include path.
  1. Over the cross product below the planner's choice -- family, template arguments, grids, LDS bytes, truncation byte, name --
     is what the launchers' former cascade chose (tests/cost_kernel_model.py), field by field.
  2. The boundary at 2^31 - 1 pixels: k_cost_census8x below it and k_cost_census8 from there on; no k_cost_diffx from there on.
  3. Every choice is in the instance list, and every instance is chosen (k_cost_census8 only at 2^31 - 1 pixels and more).
  4. The link to the fill plan: no attempt of any walk of tests/test_fillplan.py's sweeps is refused, a padded attempt is always
     taken by k_cost_diffx or a k_cost_census8* kernel, and a direct attempt is never planned."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import cost_kernel_model as M
import test_fillplan as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = [4, 63, 64, 100, 128, 150, 151, 152, 192, 256, 300, 384, 512, 600, 768, 1024, 1028, 1500]
NCHS = [1, 2, 3, 4, 5, 8]
WIDTHS, HEIGHTS = [1, 3, 4, 5, 44, 45, 1920], [1, 3, 1080]
TRUNCS = tf.TRUNCS
BIG = [(2147483646, 1), (2147483647, 1), (65536, 32768)]  # 2^31 - 2, 2^31 - 1 and 2^31 pixels


def build_harness(tmp):
    so = os.path.join(str(tmp), "libcost_kernel_harness.so")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mgm_amd", "csrc"),
           os.path.join(ROOT, "tests", "cost_kernel_harness.cc"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib = C.CDLL(so)
    lim = (C.c_int * 5)()
    lib.cost_kernel_limits(lim)
    assert list(lim)[:4] == [len(M.FIELDS), len(M.OUT), M.NAME_BYTES, len(tf.FIELDS)], "a request or the choice gained or lost a field: extend the harness and the model"
    lib.maxatt = lim[4]
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("costkernel"))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def plan(lib, req, trunc):
    req, trunc = np.ascontiguousarray(req, np.int32), np.ascontiguousarray(trunc, np.float32)
    out, names = np.zeros((len(req), len(M.OUT)), np.int64), np.zeros(len(req), "S%d" % M.NAME_BYTES)
    lib.cost_kernel_plan(len(req), ptr(req), ptr(trunc), ptr(out), ptr(names))
    return out, names


def walks(lib, req, trunc, script):
    """-> attempts made [n], (form, family) of each [n][maxatt][2], names [n][maxatt]"""
    req, trunc, flags = np.ascontiguousarray(req, np.int32), np.ascontiguousarray(trunc, np.float32), np.asarray(script, np.uint32)
    w, names = np.zeros((len(req), 1 + 2 * lib.maxatt), np.int64), np.zeros((len(req), lib.maxatt), "S%d" % M.NAME_BYTES)
    lib.cost_kernel_walks(len(req), ptr(req), ptr(trunc), len(flags), ptr(flags), ptr(w), ptr(names))
    return w[:, 0], w[:, 1:].reshape(len(req), lib.maxatt, 2), names


def instances(lib):
    out, names = np.zeros((64, 8), np.int64), np.zeros(64, "S%d" % M.NAME_BYTES)
    n = lib.cost_kernel_instances(64, ptr(out), ptr(names))
    assert 0 < n <= 64
    return [tuple(r) for r in out[:n].tolist()], names[:n]


def request(**kw):
    """A grey AD volume of 64 labels on a 44 x 20 pair, compact copy alone; `kw` changes it."""
    q = dict(costfn=0, nch=1, nx=44, ny=20, vnx=None, vny=None, L=64, Lreal=None, cbytes=1, hwin=1, f32=0, compact=1, ragged=0, scratch=0)
    q.update(kw)
    q["vnx"], q["vny"] = q["vnx"] or q["nx"], q["vny"] or q["ny"]
    q["Lreal"] = q["Lreal"] or q["L"]
    return [q[f] for f in M.FIELDS]


def inner_block():
    """The part of the cross product that does not depend on (costfn, nch, Lreal): rows of request columns and truncations."""
    rows = np.array(list(itertools.product(LABELS, (0, 1, 2), (0, 1), (0, 1), (0, 1), (0, 1), range(6), WIDTHS, HEIGHTS, range(len(TRUNCS)))), np.int32)
    req = np.zeros((len(rows), len(M.FIELDS)), np.int32)
    col = {f: k for k, f in enumerate(M.FIELDS)}
    for name, k in (("L", 0), ("cbytes", 1), ("f32", 2), ("compact", 3), ("ragged", 4), ("scratch", 5), ("hwin", 6), ("nx", 7), ("ny", 8)):
        req[:, col[name]] = rows[:, k]
    req[:, col["vnx"]] = (req[:, col["nx"]] * 7 + 7) // 8  # (a narrower right image: its grids are its own)
    req[:, col["vny"]] = req[:, col["ny"]]
    return req, np.array(TRUNCS, np.float32)[rows[:, 9]], col


def key_of(out):
    """The instance of a choice (its first eight fields) as one integer."""
    k = np.zeros(len(out), np.int64)
    for c, base in zip(range(8), (16, 8, 2, 4, 2, 4, 2048, 4)):
        assert out[:, c].min() >= 0 and out[:, c].max() < base
        k = k * base + out[:, c]
    return k


def unkey(k):
    f = []
    for base in (4, 2048, 4, 2, 4, 2, 8, 16):
        f.append(int(k % base))
        k //= base
    return tuple(reversed(f))


def compare(got, gnames, want, wnames, req, trunc):
    if np.array_equal(got, want) and np.array_equal(gnames, wnames):
        return
    i = int(np.argmax(np.any(got != want, axis=1) | (gnames != wnames)))
    raise AssertionError((dict(zip(M.FIELDS, req[i].tolist())), float(trunc[i]), dict(zip(M.OUT, got[i].tolist())), gnames[i], dict(zip(M.OUT, want[i].tolist())), wnames[i]))


@pytest.fixture(scope="module")
def swept(lib):
    """1. The sweep against the model -> (requests, per-family counts, the distinct instances chosen)."""
    req, trunc, col = inner_block()
    counts, keys, total = np.zeros(len(M.FAMILIES), np.int64), set(), 0
    for costfn, nch, below in itertools.product(range(6), NCHS, (0, 1)):
        req[:, col["costfn"]], req[:, col["nch"]] = costfn, nch
        L = req[:, col["L"]]
        req[:, col["Lreal"]] = np.where(L == 192, 151, np.maximum(L - 1, 1)) if below else L
        got, gnames = plan(lib, req, trunc)
        want, wnames = M.choose(req, trunc)
        compare(got, gnames, want, wnames, req, trunc)
        counts += np.bincount(got[:, 0], minlength=len(counts))
        keys |= set(np.unique(key_of(got)).tolist())
        total += len(req)
    return total, counts, {unkey(k) for k in keys}


def test_the_sweep_chooses_what_the_launchers_chose(swept):
    total, counts, _ = swept
    assert total == 6 * len(NCHS) * len(LABELS) * 2 * 3 * 4 * 2 * 2 * 6 * len(WIDTHS) * len(HEIGHTS) * len(TRUNCS)
    assert counts.sum() == total and counts[M.REFUSED] > 0 and counts[M.GENERAL] > 0


def boundary(lib):
    """2. -> the instances chosen"""
    fam = lambda **kw: int(plan(lib, [request(**kw)], [np.inf])[0][0, 0])
    reqs, truncs = [], []
    for (nx, ny), L, Lreal, costfn, cb, nch, t in itertools.product(BIG, M.COMPACT_LABELS, (0, 1), (0, 1, 2), (1, 2), (1, 3, 4), (np.inf, 20.0)):
        reqs.append(request(nx=nx, ny=ny, L=L, Lreal=L - 5 * Lreal, costfn=costfn, cbytes=cb, nch=nch))
        truncs.append(t)
    got, gnames = plan(lib, reqs, truncs)
    want, wnames = M.choose(reqs, truncs)
    compare(got, gnames, want, wnames, np.array(reqs), np.array(truncs))
    for (nx, ny), beyond in zip(BIG, (False, True, True)):
        for L in M.COMPACT_LABELS:
            assert fam(nx=nx, ny=ny, L=L, costfn=2) == (M.CENSUS8 if beyond else M.CENSUS8X), (nx, ny, L)
            assert fam(nx=nx, ny=ny, L=L, Lreal=L - 5, costfn=2) == (M.CENSUS8 if beyond else M.CENSUS8X), (nx, ny, L, "padded")
            for costfn, cb in itertools.product((0, 1), (1, 2)):
                if L * cb <= 1024:
                    assert fam(nx=nx, ny=ny, L=L, costfn=costfn, cbytes=cb) == (M.GENERAL if beyond else M.DIFFX), (nx, ny, L, costfn, cb)
                    assert fam(nx=nx, ny=ny, L=L, Lreal=L - 5, costfn=costfn, cbytes=cb) == (M.REFUSED if beyond else M.DIFFX), (nx, ny, L, costfn, cb, "padded")
    return {unkey(k) for k in np.unique(key_of(got)).tolist()}


def test_the_pixel_count_boundary(lib):
    assert boundary(lib)


def test_every_choice_has_an_instance_and_every_instance_is_chosen(lib, swept):
    """3."""
    _, counts, chosen = swept
    inst, names = instances(lib)
    assert len(inst) == len(set(inst)) == 50 and set(inst) == set(M.INSTANCES), sorted(set(inst) ^ set(M.INSTANCES))
    assert {i[6] for i in inst if i[0] == M.CENSUS8X} == {L for L in range(1, 1100) if lib.cost_kernel_c8_supported(L)} == {64 * i[6] for i in inst if i[0] == M.CENSUS8}
    for what, n in zip(M.FAMILIES, counts.tolist()):
        print("%-20s %9d requests" % (what, n))
    assert chosen - {(M.REFUSED,) + (0,) * 7} <= set(inst), sorted(chosen - set(inst))
    assert set(inst) - chosen == {i for i in inst if i[0] == M.CENSUS8}, "every instance but k_cost_census8's below 2^31 - 1 pixels"
    big = boundary(lib)
    assert big - {(M.REFUSED,) + (0,) * 7} <= set(inst) and {i for i in inst if i[0] == M.CENSUS8} <= big
    # the name of an instance is a function of the instance: the one the planner returns with it
    by_name = dict(zip(inst, names.tolist()))
    got, gnames = plan(lib, [request(costfn=2, L=L, nx=nx) for L in M.COMPACT_LABELS for nx in (44, 45)], [np.inf] * 16)
    assert [by_name[tuple(r)] for r in got[:, :8].tolist()] == gnames.tolist()


def test_the_launch_table_holds_the_instance_list(lib):
    """launch_cost (mgm_cost_fast.hip) has one `return launch_*<...>` per template argument list of kCostInstances, no other,
    and no `default:` arm but the one that refuses."""
    import re
    src = open(os.path.join(ROOT, "mgm_amd", "csrc", "mgm_cost_fast.hip")).read()
    table = src[src.index("hipError_t launch_cost("):]
    helpers = src[src.index("// ---- launch_cost:"):src.index("hipError_t launch_cost(")]
    assert "default:" not in table and re.findall(r"default: *([^\n]*)", helpers) == ["return hipErrorInvalidValue;"]
    blocks = re.findall(r"X\((\d+)\)", open(os.path.join(ROOT, "mgm_amd", "csrc", "mgm_fillplan.h")).read().split("#define MGM_LABEL_BLOCKS(X)")[1].split("\n")[0])
    got = set()
    for fn, args in re.findall(r"return launch_(\w+)<([^>]*)>\(p, k, s\);", table):
        got |= {(fn, args.replace("n", b)) for b in blocks} if "n" in args else {(fn, args)}
    nch = set(re.findall(r"case (\d): hipLaunchKernelGGL\(\(k_cost_diffx<CB, \1, SD>\)", helpers))
    inst, _ = instances(lib)
    want = set()
    for fam, FN, W4, CB, SD, NCH, LN, HW in inst:
        want |= {M.NCC: {("ncc", str(HW))}, M.BTX_BT: {("btx", str(FN))}, M.BTX_DIFF: {("btx", str(FN))}, M.BTX_CENSUS: {("btx", str(FN))},
                 M.DIFFX: {("diffx", "%d, %s" % (CB, "true" if SD else "false"))}, M.CENSUS8X: {("census8x", "64 * %d" % (LN // 64))},
                 M.CENSUS8: {("census8", str(LN))}, M.GENERAL: set()}[fam]
    assert got == want, sorted(got ^ want)
    assert nch == {str(i[5]) for i in inst if i[0] == M.DIFFX} and "return launch_cost_general(p, k.grid, s);" in table


def test_no_planned_attempt_is_refused(lib):
    """4. Every request of test_fillplan.py's sweeps, every attempt of every scripted walk."""
    seen, total = set(), 0
    for what, req, trunc in tf.all_sweeps():
        for script in tf.SCRIPTS:
            natt, att, _ = walks(lib, req, trunc, script)
            made = np.arange(lib.maxatt)[None, :] < natt[:, None]
            form, family = att[:, :, 0], att[:, :, 1]
            direct = made & (form == tf.REL)
            assert np.all(family[direct] == -1) and np.all(family[made & ~direct] >= 0), (what, script, "a direct attempt is k_cost_census_rel's, every other one is planned")
            bad = made & ~direct & (family == M.REFUSED)
            if bad.any():
                i, k = (int(x[0]) for x in np.nonzero(bad))
                raise AssertionError(("refused", what, script, dict(zip(tf.FIELDS, req[i].tolist())), float(trunc[i]), "attempt", k, att[i, :natt[i]].tolist()))
            pad = made & (form == tf.PAD)
            ok = np.isin(family[pad], (M.DIFFX, M.CENSUS8X, M.CENSUS8))
            if not ok.all():
                i = int(np.nonzero(pad)[0][np.argmin(ok)])
                raise AssertionError(("a padded attempt no restructured kernel takes", what, script, dict(zip(tf.FIELDS, req[i].tolist())), float(trunc[i]), att[i, :natt[i]].tolist()))
            seen |= set(np.unique(family[made]).tolist())
            total += int(made.sum())
    assert total > 3000000
    assert seen == {-1, M.NCC, M.BTX_BT, M.BTX_DIFF, M.BTX_CENSUS, M.DIFFX, M.CENSUS8X, M.GENERAL}, seen


def test_the_named_choices(lib):
    """The kernels DESIGN.md's table names, from requests spelled out."""
    name = lambda t=np.inf, **kw: plan(lib, [request(**kw)], [t])[1][0].decode()
    assert name() == "k_cost_diffx_1b" and name(nch=3, cbytes=2) == "k_cost_diffx_2b" and name(nch=2, cbytes=2) == "k_cost_diffx_2b_anych"
    assert name(L=768, nch=2) == "k_cost_diffx_1b_anych" and name(L=768, cbytes=2) == "k_cost_general" and name(t=-2.0) == "k_cost_general"
    assert name(L=192, Lreal=151) == "k_cost_diffx_1b" and name(L=192, Lreal=151, t=np.nan) == "k_cost_general"
    assert name(costfn=2) == "k_cost_census8x_w4" and name(costfn=2, nx=45) == "k_cost_census8x" and name(costfn=2, nch=2) == "k_cost_general"
    f32 = dict(f32=1, compact=0, cbytes=0)
    assert name(costfn=2, nch=2, **f32) == "k_cost_btx_census_w4" and name(costfn=1, nx=45, **f32) == "k_cost_btx_diff" and name(costfn=0, L=151, **f32) == "k_cost_general"
    assert name(costfn=3, scratch=1, **f32) == "k_cost_ncc" and name(costfn=3, scratch=1, hwin=4, **f32) == "k_cost_general" and name(costfn=3, **f32) == "k_cost_general"
    assert name(costfn=3, scratch=1, L=1028, **f32) == "k_cost_general" and name(costfn=3, scratch=1, nch=5, **f32) == "k_cost_general"
    assert name(costfn=4, scratch=1, **f32) == "k_cost_btx_bt_w4" and name(costfn=5, scratch=1, nx=45, **f32) == "k_cost_btx_bt" and name(costfn=5, scratch=1, L=150, **f32) == "k_cost_general"
    assert name(costfn=4, **f32) == "k_cost_general" and name(ragged=1, f32=1) == "k_cost_general"
    out = plan(lib, [request(costfn=3, scratch=1, nch=3, hwin=2, L=100, nx=100, ny=7, vnx=90, **f32)], [np.inf])[0][0]
    assert dict(zip(M.OUT, out.tolist())) == dict(family=M.NCC, FN=0, W4=0, CB=0, SD=0, NCH=0, LN=0, HW=2, pre=M.PRE_NCC_STATS, pre_grid_u=3, pre_grid_v=3, grid=28,
                                                  lds=4 * 3 * 5 * (36 + 135), tb=0)
