"""How a cost volume gets filled, on the host (mgm_amd/csrc/mgm_fillplan.h): no device.

tests/fillplan_harness.cc is compiled with plain g++ -- no ROCm include path: that it compiles IS the test that the policy is
HIP-free -- and called through ctypes: plan_fill, and a WALK (a request and a scripted list of flag words -> the attempts made,
the attempt that stands, the memory the volume keeps).  Over all six distances x four prefilters, 1..4 channels, census windows
3..11, twelve label counts, dense and ragged, nine truncations, every memory state and each switch off in turn:
  1. refusals exactly where nch * (w * w - 1) is not a positive multiple of 8 or exceeds 8 words;
  2. every walk ends, in at most five attempts, in an attempt that cannot fail; none is repeated and widths only grow;
  3. the compact-only, padded and direct forms are attempted only where their switches and the request allow;
  4. the refill memory;
  5. agreement with the stateful campaign's model (tests/stateful_model.py)."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import stateful_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM_ERR_INVALID, MGM_ERR_UNSUPPORTED = 1, 2  # include/mgm_hip.h
REL, PAD, COMPACT, GENERAL = range(4)  # FillForm
FIELDS = "nx ny vnx vny nch L dist pre win ragged diff_fails diff_wide hint c8 pad lazy_f32 rel rel_direct".split()
SWITCHES = FIELDS[13:]
DIST = ["ad", "sd", "census", "ncc", "btad", "btsd"]
PRE = ["none", "census", "sobelx", "gblur"]
LABELS = [64, 100, 128, 151, 192, 256, 300, 512, 600, 768, 1024, 1500]
COMPACT_LABELS = [64, 128, 192, 256, 384, 512, 768, 1024]
WINS = [3, 5, 7, 9, 11]
TRUNCS = [math.inf, 20.0, 254.0, 255.0, 7.5, 0.0, -0.0, -2.0, math.nan]
MEMORIES = [(f, w, h) for f in (0, 1, 2) for w in (0, 1) for h in (64, 128)]
SCRIPTS = [[0], [1], [9], [1, 0], [1, 9], [3, 3, 0]]  # flag words of the attempts: fits / two bytes would do / no compact form / ...


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fillplan") / "libfillplan_harness.so")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mgm_amd", "csrc"),
           os.path.join(ROOT, "tests", "fillplan_harness.cc"), "-o", so]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lib = C.CDLL(so)
    lib.fillplan_message.restype = C.c_char_p
    lib.fillplan_message.argtypes = [C.c_void_p, C.c_float]
    lib.fillplan_is_byte_code.argtypes = [C.c_float]
    lim = (C.c_int * 4)()
    lib.fillplan_limits(lim)
    assert lim[0] == len(FIELDS), "the request gained or lost a field: extend the harness and this file"
    lib.nplan, lib.nwalk, lib.maxatt = lim[1], lim[2], lim[3]
    return lib


def request(**kw):
    q = dict(nx=44, ny=20, vnx=44, vny=20, nch=1, L=64, dist=0, pre=0, win=3, ragged=0, diff_fails=0, diff_wide=0, hint=64, c8=1, pad=1,
             lazy_f32=1, rel=1, rel_direct=1, trunc=math.inf)
    q.update(kw)
    return q


class Batch:
    """Plans and walks of n requests (columns of ints `req`, truncations `trunc`) under one script of flag words."""

    def __init__(self, lib, req, trunc, script):
        req, trunc = np.ascontiguousarray(req, np.int32), np.ascontiguousarray(trunc, np.float32)
        n = len(req)
        flags = np.asarray(script, np.uint32)
        plans, walks = np.zeros((n, lib.nplan), np.int64), np.zeros((n, lib.nwalk), np.int64)
        lib.fillplan_batch(n, req.ctypes.data_as(C.c_void_p), trunc.ctypes.data_as(C.c_void_p), len(flags), flags.ctypes.data_as(C.c_void_p),
                           plans.ctypes.data_as(C.c_void_p), walks.ctypes.data_as(C.c_void_p))
        self.req, self.trunc, self.n = req, trunc, n
        for k, name in enumerate(FIELDS):
            setattr(self, name, req[:, k])
        self.err, self.costfn, self.pre_fixed, self.words, self.nan_words, self.pnch = (plans[:, k] for k in range(6))
        self.inputs, self.bytes_u, self.bytes_v, self.bytes_tmp = (plans[:, k] for k in range(7, 11))
        self.ptrunc = plans[:, 6].astype(np.uint32).view(np.float32)
        self.first, self.general, self.gather_cb = plans[:, 11:15], plans[:, 15:19], plans[:, 19]
        self.natt, self.mem = walks[:, 0], walks[:, 1:4]
        self.att = walks[:, 5:].reshape(n, lib.maxatt, 4)  # (form, slots, cbytes, readback) of attempt k
        k = np.clip(self.natt - 1, 0, None)
        self.last = self.att[np.arange(n), k]


def walk(lib, script, **kw):
    q = request(**kw)
    return Batch(lib, [[q[f] for f in FIELDS]], [q["trunc"]], script)


def sweep(nchs=(1, 2, 3, 4), memories=((0, 0, 64),), off=None):
    """The requests of the cross product as (int columns, truncations)."""
    rows = np.array(list(itertools.product(nchs, LABELS, range(6), range(4), WINS, (0, 1), range(len(TRUNCS)), range(len(memories)))), np.int32)
    n = len(rows)
    req = np.zeros((n, len(FIELDS)), np.int32)
    col = {f: k for k, f in enumerate(FIELDS)}
    req[:, :4] = (44, 20, 44, 20)
    for name, k in (("nch", 0), ("L", 1), ("dist", 2), ("pre", 3), ("win", 4), ("ragged", 5)):
        req[:, col[name]] = rows[:, k]
    mem = np.array(memories, np.int32)[rows[:, 7]]
    req[:, col["diff_fails"]:col["hint"] + 1] = mem
    req[:, col["c8"]:] = 1
    if off:
        req[:, col[off]] = 0
    return req, np.array(TRUNCS, np.float32)[rows[:, 6]]


def all_sweeps():
    """(what, requests, truncations): every memory state with every switch on; each switch off in turn."""
    yield ("default", *sweep())
    yield ("memories", *sweep(nchs=(1, 3), memories=MEMORIES))
    for s in SWITCHES:
        yield ("%s off" % s, *sweep(nchs=(1, 3), off=s))


def census_bits(b):
    pre1 = (b.dist == 2) | (b.pre == 1)
    side = 2 * (b.win // 2) + 1
    return pre1, b.nch * (side * side - 1)


def byte_code(t):
    t = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isposinf(t) | ((t >= 0) & ~np.signbit(t) & (t <= 254) & (t == np.rint(t)))


def test_refusals(lib):
    """1. Exactly where nch * (w * w - 1) is not a positive multiple of 8 (invalid) or exceeds 8 words (unsupported) -- whatever
    else the request holds --, with the messages the filling always gave."""
    total = 0
    for what, req, trunc in all_sweeps():
        b = Batch(lib, req, trunc, [0])
        pre1, nbits = census_bits(b)
        invalid = pre1 & (nbits % 8 != 0)
        unsupported = pre1 & ~invalid & ((nbits // 8 + 3) // 4 > 8)
        want = np.where(invalid, MGM_ERR_INVALID, np.where(unsupported, MGM_ERR_UNSUPPORTED, 0))
        assert np.array_equal(b.err, want), what
        assert unsupported.any() and (want == 0).any()  # (4 w (w + 1) is a multiple of 8 for every window >= 3: the invalid ones are below)
        total += b.n
    assert total > 900000
    q = request(dist=2, win=3, nch=3, L=151, ragged=1, diff_fails=2, c8=0)
    for win, nch, msg in ((3, 3, b""), (3, 1, b""), (1, 1, b"census: nch*(win*win-1) must be a positive multiple of 8"), (0, 4, b"census: nch*(win*win-1) must be a positive multiple of 8"),
                          (-3, 1, b"census: nch*(win*win-1) must be a positive multiple of 8"), (5, 3, b""), (11, 3, b"census descriptor longer than 256 bits"),
                          (9, 4, b"census descriptor longer than 256 bits"), (9, 3, b"")):
        q.update(win=win, nch=nch)
        assert lib.fillplan_message((C.c_int * len(FIELDS))(*[q[f] for f in FIELDS]), q["trunc"]) == msg, (win, nch)
    q.update(dist=0, pre=0, win=0)
    assert lib.fillplan_message((C.c_int * len(FIELDS))(*[q[f] for f in FIELDS]), q["trunc"]) == b"", "no census prefilter: the window is not looked at"


def test_plan_outputs(lib):
    """The distance / prefilter pair after the consistency fix, descriptor words, nan_words, the scaled truncation, the scratch."""
    req, trunc = sweep()
    b = Batch(lib, req, trunc, [0])
    ok = b.err == 0
    pre1, nbits = census_bits(b)
    assert np.array_equal(b.costfn[ok], b.dist[ok]) and np.array_equal(b.pre_fixed[ok], np.where(pre1, 1, b.pre)[ok])
    words = np.where(pre1, (nbits // 8 + 3) // 4, 0)
    assert np.array_equal(b.words[ok], words[ok])
    assert np.array_equal(b.nan_words[ok], (pre1 & (b.dist != 2) & (nbits > 24))[ok])
    pnch = np.where(pre1, words, b.nch)
    assert np.array_equal(b.pnch[ok], pnch[ok])
    want = (b.trunc * pnch.astype(np.float32)).astype(np.float32)
    assert np.array_equal(b.ptrunc[ok].view(np.uint32), want[ok].view(np.uint32)), "truncDist * nch, to the bit (-0 and NaN included)"
    npix = 44 * 20
    plain = ~pre1 & (b.pre == 0)
    per = np.where(pre1, 4 * words, np.where((b.pre == 2) | (b.pre == 3), 4 * b.nch,
                   np.where(plain & (b.dist == 3) & (b.ragged == 0), 4 * (2 * b.nch + 1), np.where(plain & (b.dist >= 4) & (b.ragged == 0), 8 * b.nch, 0))))
    assert np.array_equal(b.bytes_u[ok], (npix * per)[ok]) and np.array_equal(b.bytes_v[ok], (npix * per)[ok])
    assert np.array_equal(b.bytes_tmp[ok], np.where(~pre1 & (b.pre == 3), npix * 4 * b.nch, 0)[ok]), "the blur's temporary"
    w = walk(lib, [0], nx=100, ny=60, vnx=120, vny=50, nch=3, pre=3)
    assert (w.bytes_u[0], w.bytes_v[0], w.bytes_tmp[0]) == (72000, 72000, 72000)


def check_walks(b, script, what):
    ok = b.err == 0
    n, att, natt = b.n, b.att, b.natt
    # 2. termination
    assert np.all(natt[ok] >= 1) and np.all(natt[ok] <= 5), what
    last = b.last
    fitted = np.array(script)[np.minimum(natt - 1, len(script) - 1)] == 0  # (the flag word the last attempt came back with)
    assert np.all((last[ok, 0] == GENERAL) | (last[ok, 3] == 0) | fitted[ok]), (what, "ends in a fit or in an attempt that cannot fail")
    if all(script):
        assert np.all((last[ok, 0] == GENERAL) | (last[ok, 3] == 0)), (what, "nothing fits: ends in an attempt that cannot fail")
    for k in range(1, 5):
        live = ok & (natt > k)
        p, c = att[live, k - 1], att[live, k]
        same = p[:, 0] == c[:, 0]
        assert np.all(c[~same, 0] == GENERAL), (what, "a form is only left for the general fill")
        assert np.all(p[:, 0] != GENERAL), (what, "nothing follows the general fill")
        grow = (c[same, 1] >= p[same, 1]) & (c[same, 2] >= p[same, 2]) & ((c[same, 1] > p[same, 1]) | (c[same, 2] > p[same, 2]))
        assert np.all(grow), (what, "widths only grow, no attempt is repeated")
    # 3. where the narrow forms are attempted
    made = np.arange(att.shape[1])[None, :] < natt[:, None]
    for form in (REL, PAD, COMPACT):
        tried = ok & np.any(made & (att[:, :, 0] == form), axis=1)
        assert np.all((b.c8[tried] == 1) | (form == REL)) and np.all(b.lazy_f32[tried] == 1), (what, form)
        if form == PAD:
            assert np.all((b.ragged[tried] == 0) & ~np.isin(b.L[tried], COMPACT_LABELS) & (b.pad[tried] == 1) & (b.L[tried] <= 1024)), what
            slots = att[tried, 0, 1]
            assert np.all((slots >= b.L[tried]) & np.isin(slots, COMPACT_LABELS)), what
        if form == COMPACT:
            assert np.all((b.ragged[tried] == 0) & np.isin(b.L[tried], COMPACT_LABELS)), what
        if form == REL:
            assert np.all((b.ragged[tried] == 1) & (b.costfn[tried] == 2) & (b.words[tried] == 1) & byte_code(b.trunc[tried]) & (b.rel[tried] == 1)
                          & (b.rel_direct[tried] == 1)), what
    two = ok & np.any(made & (att[:, :, 0] != GENERAL) & (att[:, :, 0] != REL) & (att[:, :, 2] == 2), axis=1)
    assert np.all(np.where(att[two, 0, 0] == PAD, att[two, 0, 1], b.L[two]) <= 512), (what, "two bytes per cost up to 512 label slots")
    return int(ok.sum())


def test_walks_end_and_narrow_forms_stay_behind_their_switches(lib):
    total, seen = 0, set()
    for what, req, trunc in all_sweeps():
        for script in SCRIPTS:
            b = Batch(lib, req, trunc, script)
            total += check_walks(b, script, (what, script))
            ok = b.err == 0
            seen |= set(map(tuple, b.att[ok][:, :3, 0][np.arange(ok.sum())[:, None], np.zeros((ok.sum(), 1), int)].tolist()))
            seen |= {("n", int(x)) for x in np.unique(b.natt[ok])}
            if what == "lazy_f32 off":
                assert np.all(b.att[ok, 0, 0] == GENERAL), (what, "nothing but the general fill")
            if what == "c8 off":
                assert np.all(np.isin(b.att[ok, 0, 0], (GENERAL, REL))) and not np.any(b.att[ok][:, :, 2][b.att[ok][:, :, 0] == GENERAL]), (what, "no compact copy, no twin")
            if what == "pad off":
                assert not np.any(b.att[ok, 0, 0] == PAD)
            if what in ("rel off", "rel_direct off"):
                assert not np.any(b.att[ok, 0, 0] == REL)
            if what == "rel off":
                assert not np.any(b.gather_cb[ok])
    assert total > 3000000
    assert {(REL,), (PAD,), (COMPACT,), (GENERAL,), ("n", 1), ("n", 2), ("n", 3)} <= seen, seen


def test_first_attempts(lib):
    """The first attempt of the families the filling knows, spelled out."""
    f = lambda **kw: tuple(int(x) for x in walk(lib, [0], **kw).first[0])
    assert f() == (COMPACT, 64, 1, 1)  # grey AD
    assert f(nch=3) == (COMPACT, 64, 2, 1) and f(dist=1) == (COMPACT, 64, 2, 1)  # colour AD, grey SD
    assert f(L=768) == (COMPACT, 768, 1, 1) and f(L=768, nch=3) == (COMPACT, 768, 1, 1)  # (two bytes stop at 512 labels)
    assert f(pre=2) == (COMPACT, 64, 1, 1) and f(pre=3) == (GENERAL, 0, 0, 0)
    assert f(diff_wide=1) == (COMPACT, 64, 2, 1) and f(diff_fails=2) == (GENERAL, 0, 0, 0)
    assert f(trunc=-2.0) == (COMPACT, 64, 1, 1), "(the kernel decides: a negative truncation is no reason for the plan)"
    assert f(L=151) == (PAD, 192, 1, 1) and f(L=151, dist=1) == (PAD, 192, 2, 1) and f(L=600, dist=1) == (PAD, 768, 1, 1)
    assert f(L=151, trunc=-2.0) == (GENERAL, 0, 0, 0) and f(L=151, trunc=-0.0) == (GENERAL, 0, 0, 0) and f(L=151, trunc=0.0) == (PAD, 192, 1, 1)
    assert f(L=151, nx=65536, ny=32768) == (GENERAL, 0, 0, 0) and f(L=1500) == (GENERAL, 0, 0, 0)
    assert f(dist=2, win=5) == (COMPACT, 64, 1, 0) and f(dist=2, win=5, trunc=254.0) == (COMPACT, 64, 1, 0)
    assert f(dist=2, win=5, trunc=255.0) == (GENERAL, 0, 1, 0) and f(dist=2, win=5, trunc=7.5) == (GENERAL, 0, 1, 0)
    assert f(dist=2, win=5, L=151) == (PAD, 192, 1, 0) and f(dist=2, win=5, L=151, diff_fails=2) == (GENERAL, 0, 0, 0)
    assert f(dist=2, win=7) == (GENERAL, 0, 0, 0) and f(dist=3) == (GENERAL, 0, 0, 0) and f(dist=4) == (GENERAL, 0, 0, 0)
    assert f(dist=0, pre=1, win=5) == (GENERAL, 0, 0, 0)  # descriptor words read as floats
    assert f(dist=2, win=5, ragged=1) == (REL, 64, 1, 1) and f(dist=2, win=5, ragged=1, hint=128) == (REL, 128, 1, 1)
    assert f(dist=2, win=5, ragged=1, trunc=7.5) == (GENERAL, 0, 1, 0) and f(ragged=1) == (GENERAL, 0, 1, 0) and f(ragged=1, L=100) == (GENERAL, 0, 0, 0)
    g = lambda **kw: int(walk(lib, [0], ragged=1, **kw).gather_cb[0])
    assert (g(), g(nch=3), g(dist=1), g(pre=2), g(dist=2, win=5, trunc=7.5), g(dist=2, win=7), g(dist=3), g(pre=3), g(rel=0)) == (1, 2, 2, 2, 1, 4, 4, 4, 0)
    assert int(walk(lib, [0]).gather_cb[0]) == 0


def test_refill_memory(lib):
    """4."""
    mem = lambda w: dict(diff_fails=int(w.mem[0, 0]), diff_wide=int(w.mem[0, 1]), hint=int(w.mem[0, 2]))
    forms = lambda w: [tuple(int(x) for x in a[:3]) for a in w.att[0, :w.natt[0]]]
    for L, form, slots in ((64, COMPACT, 64), (151, PAD, 192)):
        # two misfit walks in a row, and the third request makes no compact attempt; a fit in between resets the count
        a = walk(lib, [9], L=L)
        assert forms(a) == [(form, slots, 1), (GENERAL, 0, 0)] and mem(a)["diff_fails"] == 1
        b = walk(lib, [9], L=L, **mem(a))
        assert forms(b) == forms(a) and mem(b)["diff_fails"] == 2
        c = walk(lib, [0], L=L, **mem(b))
        assert forms(c) == [(GENERAL, 0, 0)] and mem(c)["diff_fails"] == 2, "and an 8-bit pair after it stays there"
        d = walk(lib, [0], L=L, **mem(a))
        assert forms(d) == [(form, slots, 1)] and mem(d)["diff_fails"] == 0
        # a flag of exactly 1 on a one-byte attempt leads to the two-byte attempt, and the next request starts there
        e = walk(lib, [1, 0], L=L)
        assert forms(e) == [(form, slots, 1), (form, slots, 2)] and mem(e) == dict(diff_fails=0, diff_wide=1, hint=64)
        assert forms(walk(lib, [0], L=L, **mem(e))) == [(form, slots, 2)]
        g = walk(lib, [1, 1], L=L)  # (two bytes do not fit either)
        assert forms(g) == [(form, slots, 1), (form, slots, 2), (GENERAL, 0, 0)] and mem(g) == dict(diff_fails=1, diff_wide=1, hint=64)
        assert forms(walk(lib, [3], L=L)) == [(form, slots, 1), (GENERAL, 0, 0)], "only a flag of exactly 1 widens"
    # ... up to 512 labels
    assert forms(walk(lib, [1, 0], L=512)) == [(COMPACT, 512, 1), (COMPACT, 512, 2)]
    assert forms(walk(lib, [1, 0], L=768)) == [(COMPACT, 768, 1), (GENERAL, 0, 0)] and forms(walk(lib, [1, 0], L=600)) == [(PAD, 768, 1), (GENERAL, 0, 0)]
    assert forms(walk(lib, [1, 0], L=500)) == [(PAD, 512, 1), (PAD, 512, 2)]
    # census: by construction, and the count is a matter of the differences
    h = walk(lib, [9], dist=2, win=5, diff_fails=1)
    assert forms(h) == [(COMPACT, 64, 1)] and mem(h)["diff_fails"] == 1
    # a direct fill that needed 128 slots starts there next time
    r = walk(lib, [1, 0], dist=2, win=5, ragged=1)
    assert forms(r) == [(REL, 64, 1), (REL, 128, 1)] and mem(r)["hint"] == 128
    assert forms(walk(lib, [0], dist=2, win=5, ragged=1, **mem(r))) == [(REL, 128, 1)]
    s = walk(lib, [1, 1], dist=2, win=5, ragged=1)
    assert forms(s) == [(REL, 64, 1), (REL, 128, 1), (GENERAL, 0, 1)] and mem(s)["hint"] == 64, "too wide for both: the hint stays"
    t = walk(lib, [0], dist=2, win=5, ragged=1, hint=128)
    assert forms(t) == [(REL, 128, 1)] and mem(t)["hint"] == 128


def rel_ladder(lib, slots, cb, width, integer, hull=True):
    """The gathered copy's ladder with the flag words a window of `width` labels and integer / fractional costs give."""
    s, b = C.c_int(slots), C.c_int(cb)
    for _ in range(4):
        flag = (1 if width > s.value - 2 else 0) | (2 if (not integer and b.value < 4) else 0)
        if flag == 0:
            return s.value, b.value
        if not lib.fillplan_rel_next_format(flag, int(hull), C.byref(s), C.byref(b)):
            return None
    return None


def test_rel_next_format(lib):
    assert rel_ladder(lib, 64, 1, 21, True) == (64, 1) and rel_ladder(lib, 64, 1, 101, True) == (128, 1)
    assert rel_ladder(lib, 64, 1, 127, True) is None and rel_ladder(lib, 64, 1, 101, True, hull=False) is None
    assert rel_ladder(lib, 64, 1, 21, False) == (64, 4) and rel_ladder(lib, 64, 2, 101, False) == (128, 4)
    s, b = C.c_int(64), C.c_int(4)
    assert not lib.fillplan_rel_next_format(2, 1, C.byref(s), C.byref(b)) and (s.value, b.value) == (64, 4)


def test_helpers(lib):
    for L in range(1, 1100):
        lp = lib.fillplan_padded_labels(L)
        assert lp == min([x for x in COMPACT_LABELS if x >= L], default=0)
        assert bool(lib.fillplan_c8_supported(L)) == (L in COMPACT_LABELS)
    assert not lib.fillplan_c8_supported(0) and lib.fillplan_padded_labels(1025) == 0
    for t, want in zip(TRUNCS, (1, 1, 1, 0, 0, 1, 0, 0, 0)):
        assert lib.fillplan_is_byte_code(t) == want, t


def test_agreement_with_the_stateful_model(lib):
    """5. The cost specs of the stateful campaign: the flags its pair kinds imply (8-bit pairs under a whole-number truncation fit,
    half-integer pairs do not; a window wider than the slots take asks for more), and the walk's final form in the class fill_format names, with the bytes
    per cost cost_bytes names."""
    labels = sorted({L for _, _, Ls in sm.SHAPES for L in Ls})
    n = 0
    for (cost, (pre, dist, win, kind)), trunc, L, ragged, half in itertools.product(sm.COSTS.items(), sm.TRUNCS, labels, (0, 1), (5, 27, 40, 59, 70)):
        if not ragged and half != 5:
            continue
        width = 2 * half + 1 + 4  # (the campaign's windows: half on either side, moved by up to two labels at either end)
        # (a truncation that is no whole number >= +0 shows in the costs themselves, whatever the pixels are)
        integer = kind != "h" and (trunc == math.inf or (trunc >= 0 and math.copysign(1, trunc) > 0 and float(trunc).is_integer()))
        nch = 3 if kind == "c" else 1
        script = [(1 if width > 62 else 0), (1 if width > 126 else 0)] if ragged else [0 if integer else 9]
        w = walk(lib, script, nch=nch, L=L, dist=DIST.index(dist), pre=PRE.index(pre), win=win, ragged=ragged, trunc=trunc)
        assert w.err[0] == 0
        form, slots, cb, _ = (int(x) for x in w.last[0])
        want_fmt = sm.fill_format(dict(cost=cost, trunc=trunc, kind="ragged" if ragged else "uniform", half=half), L)
        want_cb = sm.cost_bytes(cost, trunc, bool(ragged))
        if ragged:
            if form == GENERAL:  # the gathered copy: the integer costs of the model's clean specs keep their code, the others widen
                clean = want_cb != 4
                got = rel_ladder(lib, 64, int(w.gather_cb[0]), width, clean)
                fmt, cb = ("f32", 4) if got is None else ("r%d" % got[0], got[1])
            else:
                assert form == REL
                fmt = "r%d" % slots
            assert fmt == want_fmt, (cost, trunc, L, half, fmt, want_fmt)
            if fmt != "f32":
                assert cb == want_cb, (cost, trunc, L, half, cb, want_cb)
        else:
            fmt = {PAD: "pad", GENERAL: "f32"}.get(form) or ("c8" if w.costfn[0] == 2 else "d%d" % cb)
            assert fmt == want_fmt, (cost, trunc, L, fmt, want_fmt)
            assert (4 if form == GENERAL else cb) == want_cb, (cost, trunc, L, cb, want_cb)
        n += 1
    assert n > 2000
