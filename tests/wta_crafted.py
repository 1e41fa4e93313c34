"""Crafted Lr volumes, cost volumes and a numpy restatement for the plain winner search and the refinements (mgm_wta.hip).

The restatement is mgm_core.cc:582-609 and nothing else:

    S(d)   = ((0 + L0(d)) + L1(d)) + ...          float32, in pass order
    S(d)  -= float32(NDIR - 1) * C(d)             with the over-count fix
    winner = the first strict minimum among the finite S(d), by rising d

tests/test_wta_crafted_ref.py pins it on the oracle (and the oracle's refinements on the compiled reference) for the inputs
built here; tests/test_gpu_wta_crafted.py holds the kernels to it.  An Lr class is a function of (seed, NDIR, ny, nx, L)
returning float32 [NDIR][ny][nx][L], a C class a function of (seed, ny, nx, L) returning float32 [ny][nx][L].  Pixels are
numbered i = y * nx + x.

Planted pixels: on the pixels PLANTED(i) every C class holds ONE finite value on all labels, so that what an Lr class plants
there (two equal minima, a strict winner on an edge label) survives the over-count term whatever the class of C.
"""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
DENORM = np.array([1], np.uint32).view(np.float32)[0]  # 1e-45, the smallest denormal
GATE_LABELS = lambda L: (0, 1, L - 3, L - 2, L - 1)    # the five labels around the gate of mgm_refine.h:58
REFINEMENTS = (None, "vfit", "parabola", "cubic", "parabolaOCV")


def PLANTED(i):
    """ties plants on i % 4 == 0, edges on i % 16 < 5"""
    return (i % 4 == 0) | (i % 16 < 5)


def _pix(ny, nx):
    return np.arange(ny * nx).reshape(ny, nx)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def sum_fix(lr, C, NDIR, fix):
    """S [ny][nx][L] of the NDIR pass volumes lr[p] and the costs C"""
    lr = np.asarray(lr, np.float32)
    S = np.zeros(lr.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for p in range(NDIR):
            S = S + lr[p]
        if fix:
            S = S - f32(NDIR - 1) * np.asarray(C, np.float32)
    return S


def first_min(S):
    """(label index as float32, NaN where no S is finite; cost, +INF there)"""
    fin = np.isfinite(S)
    masked = np.where(fin, S, INF)
    arg = np.argmin(masked, axis=-1)  # the first of equal minima = the first strict minimum (and -0 == +0)
    has = fin.any(axis=-1)
    cost = np.where(has, np.take_along_axis(S, arg[..., None], -1)[..., 0], INF).astype(np.float32)
    return np.where(has, arg, np.nan).astype(np.float32), cost


def sum_fix_wta(lr, C, NDIR, fix):
    """(S, label_index, cost)"""
    S = sum_fix(lr, C, NDIR, fix)
    return (S,) + first_min(S)


def vout_of(NDIR, fix):
    """what a label outside the volume holds in the reference's S: never incremented, then the over-count term with C = +INF"""
    with np.errstate(invalid="ignore"):
        return f32(0) - f32(NDIR - 1) * INF if fix else f32(0)


def int_window(lo, hi):
    """(int) of the range images: truncation towards zero on both sides"""
    return np.trunc(np.asarray(lo, np.float64)).astype(np.int64), np.trunc(np.asarray(hi, np.float64)).astype(np.int64)


def windowed(S, dmin, lo, hi, NDIR, fix):
    """First strict minimum of the corrected S over the window [(int)lo, (int)hi] of every pixel; window labels outside the
    volume hold vout.  Returns (out, cost, Sh, hmin, wl, wh): the two maps (NaN / +INF where the window holds nothing
    finite), S on the hull [hmin, hmin + Sh.shape[2]) of the volume and all windows, and the integer windows."""
    S = np.asarray(S, np.float32)
    ny, nx, L = S.shape
    wl, wh = int_window(lo, hi)
    some = wl <= wh
    hmin = int(min(dmin, wl[some].min())) if some.any() else dmin
    hmax = int(max(dmin + L - 1, wh[some].max())) if some.any() else dmin + L - 1
    Sh = np.full((ny, nx, hmax - hmin + 1), vout_of(NDIR, fix), np.float32)
    Sh[:, :, dmin - hmin:dmin - hmin + L] = S
    d = np.arange(hmin, hmax + 1)
    inwin = (d >= wl[..., None]) & (d <= wh[..., None])
    idx, cost = first_min(np.where(inwin, Sh, INF))
    return (idx + f32(hmin)).astype(np.float32), cost, Sh, hmin, wl, wh


def numpy_windowed_wta(S, dmin, lo, hi, NDIR, fix):
    """(out, cost) of windowed()"""
    return windowed(S, dmin, lo, hi, NDIR, fix)[:2]


def gate_open(idx, L):
    """mgm_refine.h:58 on label indices"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(idx) & (idx - 1 >= 0) & (idx + 2 <= L - 1)


# ---- Lr classes -------------------------------------------------------------------------------------------------------------
def _nonfinite(rng, shape):
    return np.array([np.inf, -np.inf, np.nan], np.float32)[rng.integers(0, 3, shape)]


def tie_labels(kind, L):
    """the two labels of a planted tie: 0 far apart (two lanes of every instance), 1 neighbours at a multiple of 48 (one lane of
    every instance with two labels per lane or more, one chunk of k_wta_q), 2 as 0 with the next pixel planted too (pixels of a
    shared slab), 3 labels 256 apart (two of the three chunks of one k_wta_q lane at 384 labels)"""
    if L < 2:
        return 0, 0
    if kind == 1:
        a = 48 if L > 49 else 0
        return a, a + 1
    if kind == 3 and L > 21 + 258:
        return 21, 21 + 256 + 2
    return (1, L - 2) if L > 3 else (0, L - 1)


def lr_ties(seed, NDIR, ny, nx, L):
    """integers 0..3; on every fourth pixel two labels hold -1 in pass 0 and 0 in the others: two equal strict minima"""
    rng = np.random.default_rng(seed)
    lr = rng.integers(0, 4, (NDIR, ny, nx, L)).astype(np.float32)
    flat = lr.reshape(NDIR, ny * nx, L)
    for i in range(0, ny * nx, 4):
        kind = (i // 4) % 4
        a, b = tie_labels(kind, L)
        for j in ((i, i + 1) if kind == 2 and i + 1 < ny * nx else (i,)):
            flat[:, j, a] = flat[:, j, b] = 0
            flat[0, j, a] = flat[0, j, b] = -1
    return lr


def lr_edges(seed, NDIR, ny, nx, L):
    """random fractions of [0, 1); pixel i with i % 16 < 5 holds -1 in every pass at label (0, 1, L-3, L-2, L-1)[i % 16]"""
    rng = np.random.default_rng(seed)
    lr = rng.random((NDIR, ny, nx, L), dtype=np.float32)
    flat = lr.reshape(NDIR, ny * nx, L)
    for i in range(ny * nx):
        if i % 16 < 5:
            flat[:, i, min(L - 1, max(0, GATE_LABELS(L)[i % 16]))] = -1
    return lr


def lr_order(seed, NDIR, ny, nx, L):
    """per cell one pass holds 2^24 and the others 1 or 2, in an order of the cell's own: 2^24 + 1 rounds back to 2^24, so the
    sum depends on where the large term stands"""
    rng = np.random.default_rng(seed)
    lr = rng.choice(np.array([1, 2], np.float32), (NDIR, ny, nx, L))
    big = rng.integers(0, NDIR, (ny, nx, L))
    cells = rng.random((ny, nx, L)) < (0.3 if NDIR == 1 else 1.0)  # (one pass: a volume of 2^24 alone would be flat)
    np.put_along_axis(lr, big[None], np.where(cells, f32(2 ** 24), np.take_along_axis(lr, big[None], 0)[0])[None], 0)
    return lr


def lr_overflow(seed, NDIR, ny, nx, L):
    """+-1e38..3e38: the running sum reaches +-INF, and INF - INF, or stays finite, depending on the order"""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(1e38, 3e38, (NDIR, ny, nx, L)).astype(np.float32)
    return np.where(rng.random((NDIR, ny, nx, L)) < 0.5, mag, -mag).astype(np.float32)


def lr_negative(seed, NDIR, ny, nx, L):
    rng = np.random.default_rng(seed)
    return rng.uniform(-20, 20, (NDIR, ny, nx, L)).astype(np.float32)


def lr_nonfinite(seed, NDIR, ny, nx, L):
    """fractions of [-20, 20]; 15 % of the cells (pixel, label) hold +INF, -INF or NaN (a third each) in one pass, a third of
    those another such value in a second pass -- so that 15 % of S is not finite, at every pass count"""
    rng = np.random.default_rng(seed)
    lr = rng.uniform(-20, 20, (NDIR, ny, nx, L)).astype(np.float32)
    cell = rng.random((ny, nx, L)) < 0.15
    p0 = rng.integers(0, NDIR, (ny, nx, L))
    v0 = np.where(cell, _nonfinite(rng, (ny, nx, L)), np.take_along_axis(lr, p0[None], 0)[0])
    np.put_along_axis(lr, p0[None], v0[None], 0)
    two = cell & (rng.random((ny, nx, L)) < 1 / 3)
    p1 = rng.integers(0, NDIR, (ny, nx, L))
    v1 = np.where(two, _nonfinite(rng, (ny, nx, L)), np.take_along_axis(lr, p1[None], 0)[0])
    np.put_along_axis(lr, p1[None], v1[None], 0)
    return lr


def lr_denormal(seed, NDIR, ny, nx, L):
    """integer multiples of 1e-45, both signs"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-1000, 1001, (NDIR, ny, nx, L)).astype(np.float64) * float(DENORM)).astype(np.float32)


def lr_zeros(seed, NDIR, ny, nx, L):
    """+0 and -0; 15 % of the cells not finite in one pass"""
    rng = np.random.default_rng(seed)
    lr = np.where(rng.random((NDIR, ny, nx, L)) < 0.5, f32(0.0), f32(-0.0)).astype(np.float32)
    cell = rng.random((ny, nx, L)) < 0.15
    p0 = rng.integers(0, NDIR, (ny, nx, L))
    v0 = np.where(cell, _nonfinite(rng, (ny, nx, L)), np.take_along_axis(lr, p0[None], 0)[0])
    np.put_along_axis(lr, p0[None], v0[None], 0)
    return lr


def lr_flat(seed, NDIR, ny, nx, L):
    """one value per pixel on every label of every pass; on the odd pixels label 0 is +INF in pass 0"""
    rng = np.random.default_rng(seed)
    lr = np.broadcast_to(rng.uniform(-5, 5, (1, ny, nx, 1)).astype(np.float32), (NDIR, ny, nx, L)).copy()
    lr[0, :, :, 0][_pix(ny, nx) % 2 == 1] = np.inf
    return lr


def lr_nolabel(seed, NDIR, ny, nx, L):
    """fractions of [0, 8); every third pixel (i % 3 == 1) holds +INF, -INF or NaN on all labels of one pass: no finite S"""
    rng = np.random.default_rng(seed)
    lr = rng.uniform(0, 8, (NDIR, ny, nx, L)).astype(np.float32)
    flat = lr.reshape(NDIR, ny * nx, L)
    for i in range(1, ny * nx, 3):
        flat[(i // 3) % NDIR, i, :] = (np.inf, -np.inf, np.nan)[(i // 3) % 3]
    return lr


def nolabel_pixels(ny, nx):
    return _pix(ny, nx) % 3 == 1


LR_CLASSES = dict(ties=lr_ties, edges=lr_edges, order=lr_order, overflow=lr_overflow, negative=lr_negative, nonfinite=lr_nonfinite,
                  denormal=lr_denormal, zeros=lr_zeros, flat=lr_flat, nolabel=lr_nolabel)


# ---- C classes --------------------------------------------------------------------------------------------------------------
def _planted_const(C, const):
    ny, nx, _ = C.shape
    m = PLANTED(_pix(ny, nx))
    C[m] = const[m][:, None]
    return C


def c_ints(seed, ny, nx, L):
    """0..254 and (3 %) +INF"""
    rng = np.random.default_rng(seed)
    C = rng.integers(0, 255, (ny, nx, L)).astype(np.float32)
    C[rng.random((ny, nx, L)) < 0.03] = np.inf
    return _planted_const(C, rng.integers(0, 255, (ny, nx)).astype(np.float32))


def c_frac(seed, ny, nx, L):
    rng = np.random.default_rng(seed)
    return _planted_const(rng.uniform(0, 30, (ny, nx, L)).astype(np.float32), rng.uniform(0, 30, (ny, nx)).astype(np.float32))


def c_negative(seed, ny, nx, L):
    rng = np.random.default_rng(seed)
    return _planted_const(rng.uniform(-30, 30, (ny, nx, L)).astype(np.float32), rng.uniform(-30, 30, (ny, nx)).astype(np.float32))


def c_huge(seed, ny, nx, L):
    """+-1e38..3e38: f * C overflows from two passes on (the planted pixels: an ordinary fraction)"""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(1e38, 3e38, (ny, nx, L)).astype(np.float32)
    C = np.where(rng.random((ny, nx, L)) < 0.5, mag, -mag).astype(np.float32)
    return _planted_const(C, rng.uniform(0, 30, (ny, nx)).astype(np.float32))


def c_nan(seed, ny, nx, L):
    """fractions with 5 % NaN"""
    rng = np.random.default_rng(seed)
    C = rng.uniform(0, 30, (ny, nx, L)).astype(np.float32)
    C[rng.random((ny, nx, L)) < 0.05] = np.nan
    return _planted_const(C, rng.uniform(0, 30, (ny, nx)).astype(np.float32))


def c_inf1(seed, ny, nx, L):
    """for NDIR 1 with the fix: 0 * INF = NaN on every +INF cost (10 %), the planted pixels included"""
    rng = np.random.default_rng(seed)
    C = rng.integers(0, 255, (ny, nx, L)).astype(np.float32)
    C[rng.random((ny, nx, L)) < 0.10] = np.inf
    return C


C_CLASSES = dict(ints=c_ints, frac=c_frac, negative=c_negative, huge=c_huge, nan=c_nan, inf1=c_inf1)


# ---- the floors -------------------------------------------------------------------------------------------------------------
# The floors are those of an Lr class under costs that leave its S alone: without the over-count fix, or with it and a C
# class of TAME_C.  With `huge`, `nan` or `inf1` costs f * C is +-INF or NaN on most cells of the unplanted pixels (9 of 16), so
# no share of winners can be promised there; those combinations are run and compared, not counted.
# Exemptions, by arithmetic:
#   finite winner on 3/4 of the pixels: `nolabel` (a third of the pixels has none by construction), `flat` and `zeros` are
#     named by the floor itself; `overflow` at 5 passes or more and fewer than 16 labels: a cell stays finite with p = 0.11 at 8
#     passes (0.28 at 5), so a pixel keeps a finite label with 1 - 0.89^L, which is below 3/4 up to 11 labels.
#   gate and dx: `flat` (label 0 or 1 wins: closed), `zeros` (the first zero wins: label 0 on 85 % of the pixels, and equal
#     neighbours); L < 8 as stated.
#   order: NDIR <= 2 (one term, or a + b = b + a).
#   nonfinite's 20 fits with a non-finite neighbour: from 130 pixels on (65 pixels x 15 % x 3 neighbours expect 25: no margin).
#   edges: from 32 pixels on, as stated (two rounds of the 16-pixel pattern).
#   shapes of 1..9 pixels and L < 4: no share is asserted, only that the restatement runs.
TAME_C = ("ints", "frac", "negative")
GATE_EXEMPT = ("flat", "zeros")
WINNER_EXEMPT = ("nolabel", "flat", "zeros")


def floors(name, lr, C, NDIR, fix, L, verbose=False):
    """Assert the floors of class `name` on the restatement of (lr, C, NDIR, fix); returns the shares reached."""
    S, idx, cost = sum_fix_wta(lr, C, NDIR, fix)
    ny, nx, _ = S.shape
    npix = ny * nx
    got = {}
    has = np.isfinite(cost)
    got["winner"] = has.mean()
    gate = gate_open(idx, L)
    got["gate"] = gate.mean()
    if gate.any():
        from wta_right_model import vfit
        ys, xs = np.nonzero(gate)
        o = idx[ys, xs].astype(int)
        dx = np.array([vfit(S[y, x, k - 1], S[y, x, k], S[y, x, k + 1])[1] for y, x, k in zip(ys, xs, o)])
        got["dx"] = float(np.mean(~(dx == 0)))  # (NaN counts: it is not 0)
        nb = np.stack([S[ys, xs, o - 1], S[ys, xs, o + 1], S[ys, xs, o + 2]])
        got["nonfinite_neighbours"] = int((~np.isfinite(nb)).any(axis=0).sum())
    with np.errstate(invalid="ignore"):
        got["tie"] = float(np.mean((np.isfinite(S) & (S == cost[..., None])).sum(axis=2) > 1))
    for k, lab in enumerate(GATE_LABELS(L)):
        got["edge%d" % k] = int((has & (idx == lab)).sum())
    if name == "order":
        got["order"] = float(np.mean(sum_fix(lr[::-1], C, NDIR, fix).view(np.uint32) != S.view(np.uint32)))
    if verbose:
        print("floors %-9s NDIR %d fix %d %dx%dx%d: %s" % (name, NDIR, fix, nx, ny, L, " ".join("%s=%.3g" % kv for kv in got.items())))
    if npix < 10 or L < 4:
        return got
    if name == "overflow" and NDIR >= 5 and L < 16:
        assert has.any(), got
    elif name not in WINNER_EXEMPT:
        assert got["winner"] >= 0.75, (name, got)
    if name == "nolabel":
        assert not has[nolabel_pixels(ny, nx)].any() and has[~nolabel_pixels(ny, nx)].all(), got
    if L >= 8 and name not in GATE_EXEMPT:
        assert got["gate"] >= 0.25, (name, got)
        assert got["dx"] >= 0.25, (name, got)
    if name == "ties":
        assert got["tie"] >= 0.25, got
    if name == "edges" and npix >= 32:
        assert all(got["edge%d" % k] >= 2 for k in range(5)), got
    if name == "order" and NDIR > 2:
        assert got["order"] >= 0.25, got
    if name == "nonfinite" and L >= 8 and npix >= 130:
        assert got["nonfinite_neighbours"] >= 20, got
    return got


# ---- labels for the stand-alone refinement ----------------------------------------------------------------------------------
def refine_labels(seed, ny, nx, dmin, L):
    """Labels the TEST chooses, pixel by pixel in turn: every integer of [dmin - 2, dmax + 2], then the same with a fraction
    added that (int) drops towards zero (3.7 -> 3, -2.5 -> -2, and -0.5 -> 0 beside +0.5 -> 0), and NaN on every 11th pixel
    (undefined in the reference: the kernels and the oracle leave such a pixel alone).  |label| stays far below 2^24."""
    rng = np.random.default_rng(seed)
    ints = np.arange(dmin - 2, dmin + L + 2)
    i = np.arange(ny * nx)
    base = ints[i % len(ints)].astype(np.float64)
    frac = rng.choice(np.array([0.0, 0.4, 0.5, 0.7]), ny * nx) * ((i // len(ints)) % 2)  # first round: integers alone
    lab = np.where(base < 0, base - frac, base + frac)
    lab = np.where((base == 0) & (i % 2 == 1), -frac, lab)  # -0.5 -> 0
    lab = lab.astype(np.float32)
    lab[i % 11 == 10] = np.nan
    return lab.reshape(ny, nx)
