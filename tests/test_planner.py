"""The launch planner on the host (mgm_amd/csrc/mgm_planner.h): no device, the real shapes.

tests/planner_harness.cc is compiled with plain g++ -- no ROCm include path: that it compiles IS the test that the planner is
HIP-free -- and called through ctypes.  For every request of the sweeps below:
  (a) the global ticket order holds every (volume group, pass, band, strip) of the launch exactly once, band b of a pass behind
      band b - 1 of both strips;
  (b) every queue of the dealt table is a subsequence of the global order, the header's (first, count) pairs are contiguous and
      sum to the number of tasks, queues beyond the device's are empty;
  (c) dense: bit 24 (plain hand-off) exactly where the successor band exists and lies in the same queue block, never under one queue;
  (d) range-proportional: bit 24 (issue priority) only with more than one workgroup per CU, exactly on the chains within
      rel_prio % of the longest;
  (e) the passes' hand-off ranges are disjoint and inside the per-group stride; more bands than kMaxBands is refused;
  (f) planning twice gives identical bytes;
  (g) the two pairs of requests the context's table cache once conflated are unequal requests with different ticket orders."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1 << 18  # tasks of the largest launch below: 16 volumes x 8 passes of 4096x4096 in bands of 7 lines, two strips on four

DENSE_FIELDS = ("nx ny L nb first count layout_ndir MGM fh wmode use_c8 cb first_build ragged lines2 lpl ns devtools num_cu xcc_mask "
                "subv deep wg_per_cu strips xcdq xcdq_k one_queue w2 oneb").split()
REL_FIELDS = ("nx ny NDIR nb MGM fh pube fh2 slots cb R HS diag_fits num_cu rel_wg rel_prio rel_lag rel_lagd rel_slots rel_slope1 rel_swap "
              "rel_diag rel_strips rel_multi").split()
DENSE_SCAL = ("err subv ngroups Lk R2 R w2 wk tags NS LPk wg_per_cu deep oneb xcdq nq QK one_queue any_strips maxLL ntasks hand_vstride "
              "h_npass h_groups h_slot_floats h_slots h_R").split()
REL_SCAL = "err rel_wg diag_any swapmask maxLL ntasks hand_vstride h_npass h_groups h_slot_floats h_slots h_R".split()
GEOM = "NL LL form nbands slope nstrips split swap diag wmax".split()
ERR_TOO_MANY_BANDS = 2
MAX_BANDS = 4096


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("planner") / "libplanner_harness.so")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mgm_amd", "csrc"),
           os.path.join(ROOT, "tests", "planner_harness.cc"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib = C.CDLL(so)
    lib.planner_rel_chains.restype = None
    lim = (C.c_int * 3)()
    lib.planner_limits(lim)
    assert (lim[0], lim[1]) == (len(DENSE_FIELDS), len(REL_FIELDS)), "a request gained or lost a field: extend the harness and this file"
    assert lim[2] == MAX_BANDS
    return lib


def ints(values):
    return (C.c_int * len(values))(*[int(v) for v in values])


# ---- what the kernels report (mgm_pass.hip, mgm_pass2_dispatch.hip, mgm_pass_rel.hip): the caller's part of a request ----
def pass_lpl(L):
    lpl = (L + 63) // 64
    if lpl in (5, 7):
        return lpl + 1
    return lpl if lpl <= 8 else (12 if lpl <= 12 else 16 if lpl <= 16 else 24 if lpl <= 24 else 32)


def pass2_lines(L, c8):
    if L % 64:
        return 0
    lpl = L // 64
    if c8 and L in (64, 128, 192, 256, 384, 512, 768, 1024):
        return 15 if lpl <= 4 else 7
    return 14 if lpl in (1, 2, 3, 4) else 7 if lpl in (6, 8, 12, 16) else 0


def dense_request(lib, nx, ny, L, nb=1, first=0, count=8, layout_ndir=None, MGM=3, fh=0, wmode=0, use_c8=1, cb=1, first_build=0, ragged=0,
                  devtools=0, num_cu=256, xcc_mask=0xff, subv=1, deep=-1, wg_per_cu=0, strips=-1, xcdq=-1, xcdq_k=-1, one_queue=-1, w2=1, oneb=1):
    q = dict(nx=nx, ny=ny, L=L, nb=nb, first=first, count=count, layout_ndir=max(layout_ndir or 0, first + count), MGM=MGM, fh=fh, wmode=wmode,
             use_c8=use_c8, cb=cb, first_build=first_build, ragged=ragged, lines2=0, lpl=pass_lpl(L), ns=2 if (wmode and not fh) else 1,
             devtools=devtools, num_cu=num_cu, xcc_mask=xcc_mask, subv=subv, deep=deep, wg_per_cu=wg_per_cu, strips=strips, xcdq=xcdq,
             xcdq_k=xcdq_k, one_queue=one_queue, w2=w2, oneb=oneb)
    q["lines2"] = pass2_lines(L * lib.planner_dense_subv(ints([q[f] for f in DENSE_FIELDS])), use_c8)
    return q


def rel_request(nx, ny, NDIR=8, nb=1, MGM=3, fh=1, weighted=0, slots=64, cb=1, diag_fits=1, num_cu=256, rel_wg=0, rel_prio=None, rel_lag=0,
                rel_lagd=0, rel_slots=100, rel_slope1=1, rel_swap=1, rel_diag=1, rel_strips=1, rel_multi=1):
    pube = int(not fh and not weighted)
    fh2 = int(bool(fh) and MGM == 2 and not weighted)
    one_slab = bool(fh or pube)
    HS = (3 * slots + 2 * (slots // 16) if fh2 else (slots + 2 * (slots // 16) if one_slab else 2 * slots)) + 4
    return dict(nx=nx, ny=ny, NDIR=NDIR, nb=nb, MGM=MGM, fh=fh, pube=pube, fh2=fh2, slots=slots, cb=cb, R=16, HS=HS, diag_fits=diag_fits,
                num_cu=num_cu, rel_wg=rel_wg, rel_prio=(5 if nb <= 1 else 0) if rel_prio is None else rel_prio, rel_lag=rel_lag, rel_lagd=rel_lagd,
                rel_slots=rel_slots, rel_slope1=rel_slope1, rel_swap=rel_swap, rel_diag=rel_diag, rel_strips=rel_strips, rel_multi=rel_multi)


class Plan:
    pass


def run_plan(lib, q, dense):
    fields, names = (DENSE_FIELDS, DENSE_SCAL) if dense else (REL_FIELDS, REL_SCAL)
    scal = np.zeros(len(names), np.int64)
    geom = np.zeros((8, len(GEOM)), np.int32)
    base = np.zeros(8, np.int64)
    order = np.zeros((CAP, 2), np.int32)
    table = np.zeros((CAP + 8, 2), np.int32)
    ptr = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    n = (lib.planner_dense if dense else lib.planner_rel)(ints([q[f] for f in fields]), ptr(scal, C.c_longlong), ptr(geom, C.c_int), ptr(base, C.c_longlong),
                                                           ptr(order, C.c_int), ptr(table, C.c_int), CAP)
    assert n >= 0, "CAP too small for %r" % (q,)
    p = Plan()
    for k, v in zip(names, scal):
        setattr(p, k, int(v))
    p.g = [dict(zip(GEOM, (int(x) for x in row)), hand_base=int(b)) for row, b in zip(geom, base)]
    p.order = order[:p.ntasks].copy()
    p.table = table[:n].copy()
    return p


def same_plans(a, b):
    return (all(v == b.__dict__[k] for k, v in a.__dict__.items() if k not in ("order", "table")) and np.array_equal(a.order, b.order)
            and np.array_equal(a.table, b.table))


def check_order(p, ngroups, first, count):
    """(a) for a global order; returns the position of every item by its key."""
    x, y = p.order[:, 0].astype(np.int64), p.order[:, 1].astype(np.int64)
    assert not np.any(y >> 24), "the global order carries no marks"
    key = (x << 17) | ((y & 0xffff) << 1) | (y >> 16)
    want = [((v * 8 + k) << 17) | (b << 1) | st for v in range(ngroups) for k in range(first, first + count)
            for b in range(p.g[k]["nbands"]) for st in range(p.g[k]["nstrips"])]
    srt = np.argsort(key, kind="stable")
    assert np.array_equal(key[srt], np.array(sorted(want), np.int64)), "every (group, pass, band, strip) exactly once"
    skey = key[srt]
    where = lambda ks: srt[np.searchsorted(skey, ks)]  # position in the order of the items with these keys
    later = (y & 0xffff) > 0
    me = np.nonzero(later)[0]
    two = np.array([p.g[int(k) % 8]["nstrips"] == 2 for k in x[me]], bool)
    assert np.all(where(key[me] - 2) < me), "band b comes after band b - 1"
    assert np.all(where((key[me][two] ^ 1) - 2) < me[two]), "... of both strips"
    return skey, srt


def check_dense(p, q):
    first, count = q["first"], q["count"]
    assert p.err == 0
    assert p.ngroups * p.subv == q["nb"]
    skey, srt = check_order(p, p.ngroups, first, count)
    head, items = p.table[:8].astype(np.int64), p.table[8:].astype(np.int64)
    assert len(items) == p.ntasks
    if not p.xcdq:
        assert not head.any() and np.array_equal(items, p.order) and not p.one_queue
    else:
        # (b)
        assert np.array_equal(head[:, 0], np.concatenate([[0], np.cumsum(head[:-1, 1])])) and head[:, 1].sum() == p.ntasks
        assert not head[p.nq:, 1].any() and (not p.one_queue or not head[1:, 1].any())
        x, y = items[:, 0], items[:, 1]
        assert not np.any(y >> 25)
        key = (x << 17) | ((y & 0xffff) << 1) | ((y >> 16) & 0xff)
        at = srt[np.searchsorted(skey, key)]
        assert np.array_equal(np.sort(at), np.arange(p.ntasks)), "every item is dealt to exactly one queue"
        band, grp, k = y & 0xffff, x // 8, x % 8
        for n in range(8):
            a = at[head[n, 0]:head[n, 0] + head[n, 1]]
            assert np.all(np.diff(a) > 0), "a queue keeps the global order"
            if not p.one_queue:
                sl = slice(head[n, 0], head[n, 0] + head[n, 1])
                assert np.all((band[sl] // p.QK + grp[sl] * count + (k[sl] - first)) % p.nq == n)
        # (c)
        nbands = np.array([g["nbands"] for g in p.g])[k]
        plain = (band + 1 < nbands) & ((band + 1) // p.QK == band // p.QK) & (not p.one_queue)
        assert np.array_equal((y >> 24) & 1, plain.astype(np.int64))
    # (e)
    if p.tags:
        end = 0
        for n in range(q["layout_ndir"]):
            g = p.g[n]
            assert g["hand_base"] == end
            end += g["nbands"] * g["LL"]
        assert end == p.hand_vstride and (p.h_npass, p.h_groups, p.h_slot_floats, p.h_R) == (q["layout_ndir"], p.ngroups, p.LPk, p.R)
    assert max(g["nbands"] for g in p.g) <= MAX_BANDS


def check_rel(lib, p, q):
    assert p.err == 0
    skey, srt = check_order(p, q["nb"], 0, q["NDIR"])
    t = p.table.astype(np.int64)
    assert len(t) == p.ntasks and np.array_equal(t[:, 0], p.order[:, 0]) and np.array_equal(t[:, 1] & 0xffffff, p.order[:, 1]) and not np.any(t[:, 1] >> 25)
    # (d)
    rem = np.zeros(16 * 8 * 2)
    lib.planner_rel_chains(ints([q[f] for f in REL_FIELDS]), rem.ctypes.data_as(C.POINTER(C.c_double)))
    mine = rem[t[:, 0] * 2 + ((t[:, 1] >> 16) & 0xff)]
    assert np.all(mine > 0)
    pct = float(q["rel_prio"])
    want = (mine >= rem.max() * (1.0 - pct / 100.0)) if (p.rel_wg > 1 and pct > 0) else np.zeros(len(t), bool)
    assert np.array_equal((t[:, 1] >> 24) & 1, want.astype(np.int64))
    if p.rel_wg <= 1:
        assert not np.any(t[:, 1] >> 24)
    # (e)
    end = 0
    for n in range(q["NDIR"]):
        g = p.g[n]
        assert g["hand_base"] == end
        end += g["nbands"] * (2 * g["wmax"] if g["diag"] else g["LL"])
    assert end == p.hand_vstride and (p.h_npass, p.h_groups, p.h_slot_floats, p.h_slots) == (q["NDIR"], q["nb"], q["HS"], q["slots"])


SHAPES = [(1920, 1080, 256), (1080, 1920, 256), (700, 500, 192), (4096, 4096, 192), (150, 60, 64), (140, 96, 128), (40, 36, 64)]
PASSES = [(0, 8, 8), (0, 4, 4), (0, 1, 8), (2, 1, 8), (5, 1, 8), (7, 1, 8)]  # first, count, layout_ndir


def dense_sweep(lib):
    seen = set()

    def emit(**kw):
        q = dense_request(lib, **kw)
        key = tuple(q[f] for f in DENSE_FIELDS)
        if key not in seen:
            seen.add(key)
            yield q

    for (nx, ny, L), nb in itertools.product(SHAPES, (1, 2, 4, 12, 16)):
        big = nx * ny > 4e6
        for (first, count, lay), MGM, fh in itertools.product(PASSES, (1, 2, 3, 4), (0, 1)):
            # (the largest shape: every batch size, but only all eight passes and one single pass of each form, TSGM 2 and 4)
            if big and ((first, count) not in ((0, 8), (5, 1)) or MGM in (1, 3) or (nb in (2, 4) and fh)):
                continue
            yield from emit(nx=nx, ny=ny, L=L, nb=nb, first=first, count=count, layout_ndir=lay, MGM=MGM, fh=fh, subv=1)
    # the weight modes (two-valued: the W2 kernels on the queues; general: progress words), compact and fp32 costs
    for (nx, ny, L), nb, wmode, use_c8, fh in itertools.product(SHAPES[:3] + SHAPES[4:], (1, 4), (1, 2), (1, 0), (0, 1)):
        yield from emit(nx=nx, ny=ny, L=L, nb=nb, wmode=wmode, use_c8=use_c8, fh=fh)
    # the device: all XCDs, a partition, no census; the queue block; workgroups per CU; strips; one queue forced
    for (nx, ny, L), nb, mask, k, wg, strips in itertools.product(SHAPES[:2] + SHAPES[5:6], (1, 4), (0xff, 0x0f, 0), (-1, 0, 2), (0, 1, 2), (0, 1)):
        yield from emit(nx=nx, ny=ny, L=L, nb=nb, xcc_mask=mask, xcdq_k=k, wg_per_cu=wg, strips=strips, fh=nb == 1)
    for (nx, ny, L), one in itertools.product(SHAPES[:2], (0, 1)):
        yield from emit(nx=nx, ny=ny, L=L, one_queue=one)
    # wave sharing at 64 / 128 labels, by the heuristic and forced; two-byte costs; the first build; more than 512 labels
    for (nx, ny), L, nb, subv in itertools.product(((1920, 1080), (140, 96), (40, 36)), (64, 128), (2, 4, 16), (0, 1, 2)):
        yield from emit(nx=nx, ny=ny, L=L, nb=nb, subv=subv)
    for nx, ny, L in SHAPES[:3]:
        yield from emit(nx=nx, ny=ny, L=L, cb=2)
        yield from emit(nx=nx, ny=ny, L=L, first_build=1, use_c8=0)
        yield from emit(nx=nx, ny=ny, L=1024, nb=2)
        yield from emit(nx=nx, ny=ny, L=1100, use_c8=0)


def test_dense_plans(planner):
    n = 0
    for q in dense_sweep(planner):
        p = run_plan(planner, q, True)
        try:
            check_dense(p, q)
            assert same_plans(p, run_plan(planner, q, True)), "(f) planning twice gives the same plan"
        except AssertionError as e:
            raise AssertionError("%s\nrequest %r" % (e, q)) from e
        n += 1
    assert n > 1000


def rel_sweep():
    for (nx, ny, _), nb, MGM, fh in itertools.product(SHAPES[:3] + SHAPES[4:], (1, 2, 4, 16), (1, 2, 3, 4), (0, 1)):
        if nx * ny > 1e6 and (MGM in (1, 4) and nb in (2, 4)):
            continue
        yield rel_request(nx, ny, nb=nb, MGM=MGM, fh=fh, NDIR=8 if nb != 2 else 4)
    for (nx, ny, _), slots, cb, fits, swap, wg in itertools.product((SHAPES[0], SHAPES[1], SHAPES[4], SHAPES[6]), (64, 128), (1, 2, 4), (1, 0), (0, 1, 2), (0, 1, 2, 3)):
        yield rel_request(nx, ny, slots=slots, cb=cb, diag_fits=fits, rel_swap=swap, rel_wg=wg, fh=wg != 2, weighted=cb == 4, rel_prio=None if wg else 20)
    yield rel_request(4096, 4096, nb=1)
    yield rel_request(4096, 4096, nb=4, fh=0)
    for kw in (dict(rel_diag=0), dict(rel_strips=0, rel_diag=0), dict(rel_slope1=0), dict(rel_lag=3, rel_lagd=2), dict(rel_slots=50), dict(rel_prio=100), dict(rel_prio=0)):
        yield rel_request(1920, 1080, **kw)
        yield rel_request(150, 60, nb=2, **kw)


def test_rel_plans(planner):
    n = 0
    for q in rel_sweep():
        p = run_plan(planner, q, False)
        try:
            check_rel(planner, p, q)
            assert same_plans(p, run_plan(planner, q, False)), "(f) planning twice gives the same plan"
        except AssertionError as e:
            raise AssertionError("%s\nrequest %r" % (e, q)) from e
        n += 1
    assert n > 400


def test_too_many_bands_are_refused(planner):
    """(e) A side of more than kMaxBands bands is refused, as run_passes / run_rel always did; the largest that fits is planned."""
    fits = dense_request(planner, MAX_BANDS * 15, 16, 64, count=4)
    assert run_plan(planner, fits, True).err == 0
    for q in (dense_request(planner, MAX_BANDS * 15 + 1, 16, 64, count=4), dense_request(planner, 16, 70000, 64)):
        assert run_plan(planner, q, True).err == ERR_TOO_MANY_BANDS
    assert run_plan(planner, rel_request(70000, 16), False).err == ERR_TOO_MANY_BANDS
    assert run_plan(planner, rel_request(16, MAX_BANDS * 16 + 1, rel_swap=0, rel_diag=0), False).err == ERR_TOO_MANY_BANDS


def test_requests_the_table_cache_once_conflated(planner):
    """(g) TSGM 3 and 4 (slope 1 or 2 on the form-0 passes), and no weights against general weights without queues (the hand-off lag
    of the model): same shape, batch and occupancy, other schedules -- so other requests."""
    a = dense_request(planner, 1920, 1080, 256, MGM=3)
    b = dense_request(planner, 1920, 1080, 256, MGM=4)
    c = dense_request(planner, 1920, 1080, 256, xcdq=0)
    d = dense_request(planner, 1920, 1080, 256, xcdq=0, wmode=2)
    a0, b0 = dense_request(planner, 1920, 1080, 256, MGM=3, strips=0), dense_request(planner, 1920, 1080, 256, MGM=4, strips=0)
    for q, r, same_old_key in ((a, b, False), (a0, b0, True), (c, d, True)):
        assert not planner.dense_requests_equal(ints([q[f] for f in DENSE_FIELDS]), ints([r[f] for f in DENSE_FIELDS]))
        assert planner.dense_requests_equal(ints([q[f] for f in DENSE_FIELDS]), ints([q[f] for f in DENSE_FIELDS]))
        p, s = run_plan(planner, q, True), run_plan(planner, r, True)
        if same_old_key:  # (shape, passes, volumes, wave sharing, strips, queues, two bands per CU, band height: all alike)
            assert (p.wg_per_cu, p.xcdq, p.subv, p.any_strips, p.R) == (s.wg_per_cu, s.xcdq, s.subv, s.any_strips, s.R)
            assert p.ntasks == s.ntasks
        assert not np.array_equal(p.order, s.order)
    x, y = rel_request(1920, 1080, MGM=3), rel_request(1920, 1080, MGM=4)
    assert not planner.rel_requests_equal(ints([x[f] for f in REL_FIELDS]), ints([y[f] for f in REL_FIELDS]))
