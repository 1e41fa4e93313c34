"""Inputs for the NaN-faithful pass kernel (k_pass_exact, mgm_pass_exact.hip): cost volumes that hold NaNs and still stay mostly
finite, the floors that say so, and the host-side proof that a case can only take that kernel.

The kernel exists to give the reference's words where the operand order of `a < b ? a : b` decides what a NaN does.  A volume
with a whole-NaN pixel and little else floods: the sum over eight passes is NaN almost everywhere and a comparison is NaN against
NaN.  So the cases here are compared pass by pass (the Lr volumes), their NaNs are scattered thinly -- the recipe below -- and
every case is held to floors measured on the CPU oracle's Lr volumes alone: it may be NaN neither everywhere nor nowhere, and it
must hold words that an operand-swapped minimum would change.

k_pass_exact is the one pass kernel without a loop that waits for another wave.  Every other one hands slabs over through polled
tags, on a premise (finite, non-negative values) these inputs leave on purpose -- so must_take_exact() proves on the host, before
anything is uploaded, that the planner (plan_dense_kernels, mgm_planner.h) can only choose k_pass_exact for the case.

tests/test_exact_crafted_ref.py pins the expectation (the oracle) on the compiled reference and asserts the floors;
tests/test_gpu_exact_crafted.py runs the cases on the device."""
from collections import namedtuple

import numpy as np

from helpers import ndiff
from mgm_amd import synth
from oracle.oracle import int_ranges

INF, NAN = np.float32(np.inf), np.float32(np.nan)
FAST_LABELS = 2048  # kFastKernelLabels: beyond it only k_pass_exact exists

# ---- cost classes, [ny][nx][L] ------------------------------------------------------------------------------------------------
CLASSES = ("ints", "zeros", "negfrac", "huge", "denormal", "infs")


def cost_class(name, ny, nx, L, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 25, (ny, nx, L))
    if name == "ints":  # what every NaN case had so far
        C = k.astype(np.float32)
    elif name == "zeros":  # +0 / -0 at random, 30 % ones: "the first of several equal minima is kept"
        C = np.where(rng.random((ny, nx, L)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        C[rng.random((ny, nx, L)) < 0.3] = 1.0
    elif name == "negfrac":  # negative thirds
        C = ((k - 12).astype(np.float32) * np.float32(1.0 / 3.0)).astype(np.float32)
    elif name == "huge":  # sums overflow, INF - INF arises
        C = (k.astype(np.float32) * np.float32(1e37)).astype(np.float32)
    elif name == "denormal":
        C = (k.astype(np.float64) * 1e-45).astype(np.float32)
    elif name == "infs":  # 5 % +INF, -INF on two cells only (a -INF minimum turns everything downstream of it into NaN)
        C = k.astype(np.float32)
        C[rng.random((ny, nx, L)) < 0.05] = INF
        for dx in (-2, 2):  # (on the centre line, like the whole-NaN pixels of the recipe below)
            C[ny // 2, min(max(nx // 2 + dx, 0), nx - 1), rng.integers(L)] = -INF
    elif name == "zsign":  # label 0 is +0, the others -0 (94 %), +0 (4 %) or 1: see the tie-rule cases below
        r = rng.random((ny, nx, L))
        C = np.where(r < 0.94, np.float32(-0.0), np.where(r < 0.98, np.float32(0.0), np.float32(1.0))).astype(np.float32)
        C[:, :, 0] = 0.0
    else:
        raise KeyError(name)
    return np.ascontiguousarray(C, np.float32)


# ---- the NaN recipe -------------------------------------------------------------------------------------------------------------
Recipe = namedtuple("Recipe", "pixels cells bands")
SCATTER = Recipe(pixels=2, cells=12, bands=3)  # measured at 24x16: each pass volume 0.2-0.6 NaN (0.04-0.08 at TSGM 1)


def lane_chunk(L):
    """labels per lane of the kernel's slab-minimum scan (uniform volume)"""
    return max(1, (L + 63) // 64)


def scatter(C, seed, recipe=SCATTER):
    """NaNs on top of a class: `pixels` whole-NaN interior pixels, `cells` random cells, `bands` runs of 8 consecutive labels; and,
    deterministically, a NaN on labels 0 and L-1 (the at() edges), on both sides of a lane-chunk boundary k*chunk-1 | k*chunk,
    and on a frame pixel (never updated: Lr = C)."""
    C = C.copy()
    ny, nx, L = C.shape
    rng = np.random.default_rng(seed)
    if ny >= 5 and nx >= 5:  # (next to the centre line: no pass has much more than half of the image downstream of them)
        for i in range(recipe.pixels):
            C[ny // 2 + (-1, 1)[i % 2], nx // 2 + int(rng.integers(-3, 4)), :] = NAN
    for q in rng.choice(ny * nx, size=recipe.cells, replace=recipe.cells > ny * nx):  # (distinct pixels where there is room)
        C[q // nx, q % nx, rng.integers(L)] = NAN
    for _ in range(recipe.bands):
        o = int(rng.integers(0, max(1, L - 7)))
        C[rng.integers(ny), rng.integers(nx), o:o + 8] = NAN
    y, x = ny // 2, nx // 2
    C[y, x, 0] = NAN
    C[y, min(x + 1, nx - 1), L - 1] = NAN
    b = 3 * lane_chunk(L)
    if b < L:
        C[y, max(x - 1, 0), b - 1:b + 1] = NAN
    C[0, 0, min(1, L - 1)] = NAN  # (a corner: on the frame of every pass)
    return C


# ---- weights, [8][ny][nx] -------------------------------------------------------------------------------------------------------
def weights(kind, ny, nx, seed):
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    values, p = {"w2": ([1.0, 0.3], [0.5, 0.5]),
                 "w3": ([1.0, 2.5, 4.0], [0.6, 0.25, 0.15]),
                 "wodd": ([1.0, 2.5, 0.0, -1.0, np.inf, np.nan], [0.7, 0.1, 0.05, 0.05, 0.05, 0.05]),
                 "wzero": ([1.0, 0.0], [0.9, 0.1]),
                 "wneg": ([1.0, -1.0], [0.9, 0.1])}[kind]
    return np.ascontiguousarray(rng.choice(np.array(values, np.float32), size=(8, ny, nx), p=p), np.float32)


def weights_tame(w8):
    return w8 is None or bool((np.isfinite(w8) & (w8 > 0)).all())


# ---- the cases ------------------------------------------------------------------------------------------------------------------
# kind: "uniform" (one uploaded volume), "batch" (three uploaded volumes, one call), "ragged" (built on the device from an image
# pair and range images).  recipe: the scatter of the case (None: SCATTER); seed: of the class and the scatter.
Case = namedtuple("Case", "name kind nx ny L dmin cls seed P1 P2 NDIR MGM FH wkind recipe")
NX, NY = 24, 16
PENALTIES = [(8.0, 32.0), (2.0, np.inf), (-2.0, 32.0), (0.0, 0.0), (3.0, 1.0), (np.inf, np.inf), (np.nan, 32.0), (8.0, np.nan),
             (8.0, -np.inf)]
FH_DEFAULT = (2.0, 9.0)  # (the matrix's FH cases; the nine pairs above all run in the penalty sweep)
NDIRS = (1, 3, 4, 8)
# Other recipes, where the standard one misses a floor (measured on the oracle; the floors stay):
#   * FH potentials with a truncation (P2 < +INF): min(M[o], m + P2) heals a NaN of the neighbour's slab, so a NaN cell of C stays
#     one NaN word of Lr -- the standard recipe leaves 10-36 finite words beside a NaN per pass, the boundary floor asks 50:
#     THICK.  (Without the truncation -- P2 = +INF or NaN -- the NaNs spread as under Hirschmueller's potentials: SCATTER.)
#   * 1 and 2 labels: a NaN cell is all of a pixel or half of it, and a pixel without a finite label poisons everything
#     downstream of it: the deterministic NaNs alone (BARE), under FH at 2 labels some cells (they heal).
#   * 40x3 has no room for whole-NaN pixels: more cells.
#   * P2 = -INF: every updated slab is -INF and the next one -INF - -INF = NaN whatever the costs hold: only a shape with most
#     pixels on the frame keeps the share down (the penalty sweep runs that pair at 40x3).
#   * `infs`: a -INF cell poisons what lies downstream of it like a whole-NaN pixel does: one whole-NaN pixel beside the two cells.
THICK = Recipe(pixels=2, cells=150, bands=10)
BARE = Recipe(pixels=0, cells=0, bands=0)
CELLS = Recipe(pixels=0, cells=40, bands=3)
CELLS2 = Recipe(pixels=0, cells=120, bands=0)
ONE_PIXEL = Recipe(pixels=1, cells=12, bands=3)
BAND_FH = Recipe(pixels=0, cells=150, bands=15)  # (40x3 under FH: the NaNs heal, 3 % of the cells keep the share above its floor)


def mode_of(case):
    """which of the reference's four update functions the call runs (run_passes_exact)"""
    if case.wkind is not None:
        return 3 if case.FH else 1
    return (2 if case.MGM == 2 else 3) if case.FH else (0 if case.MGM == 2 else 1)


def _cases():
    out, seed = [], [1000]

    def add(name, kind="uniform", nx=NX, ny=NY, L=70, cls="ints", P=None, NDIR=8, MGM=3, FH=0, wkind=None, recipe=None, dmin=-5):
        seed[0] += 1
        P1, P2 = P if P is not None else (FH_DEFAULT if FH else PENALTIES[0])
        if recipe is None and FH and P2 < np.inf and kind == "uniform":
            recipe = THICK
        if recipe is None and cls == "infs":
            recipe = ONE_PIXEL
        out.append(Case(name, kind, nx, ny, L, dmin, cls, seed[0], float(P1), float(P2), NDIR, MGM, FH, wkind, recipe))

    # the matrix: classes x the four update functions at 70 and 131 labels; NDIR, TSGM and the weights cycle so that every update
    # function meets every NDIR
    for ci, cls in enumerate(CLASSES):
        for mode in range(4):
            for li, L in enumerate((70, 131)):
                FH = mode >= 2
                MGM = 2 if mode in (0, 2) else (1, 3, 4)[(ci + li) % 3]
                wkind = (None, "w2", None, "w3")[(ci + 2 * li) % 4] if mode in (1, 3) else None
                add("m%d_%s_L%d" % (mode, cls, L), L=L, cls=cls, NDIR=NDIRS[(ci + 2 * li + mode) % 4], MGM=MGM, FH=int(FH), wkind=wkind)
    # label counts: one lane-chunk, its edges, several (chunk 1, 2, 3, 5)
    for i, L in enumerate((1, 2, 24, 64, 65, 128, 300)):
        add("labels_h_L%d" % L, L=L, NDIR=8, MGM=(2, 3)[i % 2], recipe=BARE if L <= 2 else None)
        add("labels_fh_L%d" % L, L=L, NDIR=4, MGM=(1, 2)[i % 2] if L <= 2 else (3, 2)[i % 2], FH=1, recipe={1: BARE, 2: CELLS2}.get(L))
    # geometry: no interior at all, one line, one column, the smallest image with an updated pixel, a band
    for nx, ny in ((1, 1), (1, 9), (7, 1), (2, 2), (3, 3), (40, 3)):
        add("geom_h_%dx%d" % (nx, ny), nx=nx, ny=ny, NDIR=8, MGM=3, recipe=CELLS if (nx, ny) == (40, 3) else None)
        add("geom_fh_%dx%d" % (nx, ny), nx=nx, ny=ny, NDIR=4, MGM=2, FH=1, recipe=BAND_FH if (nx, ny) == (40, 3) else SCATTER)
    # beyond the fast kernels, and beyond the LDS (FH's arrays in global scratch)
    add("big_h2_L2049", nx=13, ny=11, L=2049, NDIR=4, MGM=2, dmin=-700)
    add("big_hw_L2049", nx=13, ny=11, L=2049, NDIR=8, MGM=4, wkind="w2", dmin=-700)
    add("big_fh2_L8193", nx=13, ny=11, L=8193, NDIR=3, MGM=2, FH=1, dmin=-3000)
    add("big_fh_L8193", nx=13, ny=11, L=8193, NDIR=8, MGM=3, FH=1, dmin=-3000)
    # the penalties
    for i, P in enumerate(PENALTIES):
        shape = dict(nx=40, ny=3, recipe=BARE) if P[1] == -np.inf else {}  # (see the recipes above)
        tag = "p%s_%s" % (P[0], P[1])
        if i:  # (the first pair is the matrix's under Hirschmueller's potentials)
            add("pen_h_" + tag, P=P, NDIR=NDIRS[i % 4], MGM=(2, 3, 1, 4)[i % 4], **shape)
        add("pen_fh_" + tag, P=P, NDIR=NDIRS[(i + 2) % 4], MGM=(3, 2, 4, 2)[i % 4], FH=1, **shape)
    # the weights (two-valued and three-valued ones ran in the matrix too): TSGM 2 with weights is the weighted function
    for i, wkind in enumerate(("w2", "w3", "wodd")):
        add("w_h_%s" % wkind, L=131, NDIR=8, MGM=(2, 4, 3)[i], wkind=wkind, cls=("ints", "negfrac", "ints")[i])
        add("w_fh_%s" % wkind, L=131, NDIR=(4, 8, 3)[i], MGM=(4, 2, 1)[i], FH=1, wkind=wkind)
    # a batch: exact_mins and the weights per volume
    add("batch3_hw", kind="batch", NDIR=8, MGM=3, wkind="w2")
    # ragged volumes: 40x24, windows of 21 labels in [-60, 0]
    rg = dict(kind="ragged", nx=40, ny=24, L=61, dmin=-60, cls="census")
    add("ragged_p2inf_h_t1", P=(8.0, np.inf), NDIR=8, MGM=1, **rg)
    add("ragged_p2inf_h_t2", P=(8.0, np.inf), NDIR=4, MGM=2, **rg)
    add("ragged_p2inf_h_t3", P=(8.0, np.inf), NDIR=8, MGM=3, **rg)
    add("ragged_p2inf_h_t4_w3", P=(8.0, np.inf), NDIR=4, MGM=4, wkind="w3", **rg)
    add("ragged_p2inf_fh_t2", P=(2.0, np.inf), NDIR=8, MGM=2, FH=1, **rg)
    add("ragged_p2inf_fh_t3", P=(2.0, np.inf), NDIR=4, MGM=3, FH=1, **rg)
    add("ragged_negp1_fh_t2", P=(-1.0, 30.0), NDIR=8, MGM=2, FH=1, **rg)
    add("ragged_negp1_fh_t3", P=(-1.0, 30.0), NDIR=4, MGM=3, FH=1, **rg)
    add("ragged_w0_fh_t3", P=(2.0, 30.0), NDIR=8, MGM=3, FH=1, wkind="wzero", **rg)
    add("ragged_wneg_fh_t3", P=(2.0, 30.0), NDIR=4, MGM=3, FH=1, wkind="wneg", **rg)
    # Which of several equal minima a slab keeps -- the FIRST of +0 / -0 -- shows only where a zero's sign survives to Lr.  Under
    # Hirschmueller's potentials it never does (e = +0 + ...).  Under FH a word is -0 iff C, every M[o] and no m is: `zsign` puts +0
    # first and mostly -0 behind it, so every slab minimum is +0 by the rule and -0 by any rule that lets a later label win, and
    # the -0 words of one pixel make the next slab two-signed again, along the whole line.  (`zeros`, half and half, leaves two-signed
    # slabs on the frame only: an emulation of `<=` in the lane combine on the CPU oracle changes 2-70 words of a whole case, here
    # 100-11000 per pass.)  40x24: the two-signed slabs of the first generation are the frame's, and 24x16 has some 54 of them.
    add("zsign_fh_t1_L70", nx=40, ny=24, L=70, cls="zsign", P=(0.0, 32.0), NDIR=4, MGM=1, FH=1)
    add("zsign_fh_t2_L131", nx=40, ny=24, L=131, cls="zsign", P=(0.0, 32.0), NDIR=8, MGM=2, FH=1)
    add("zsign_fh_t3_L70", nx=40, ny=24, L=70, cls="zsign", NDIR=4, MGM=3, FH=1)
    add("zsign_fh_t4_L131", nx=40, ny=24, L=131, cls="zsign", P=(0.0, 32.0), NDIR=3, MGM=4, FH=1)
    return out


CASES = _cases()
RAGGED_WIDTH = 21


# ---- the inputs of a case ---------------------------------------------------------------------------------------------------------
Built = namedtuple("Built", "Cs w8s ranges images")  # volumes; weights per volume (or None); (lo, hi, ilo, ihi) / None; (u, v) / None


def build(case, oracle=None):
    """the host arrays of a case; a ragged one needs the oracle for its cost volume (nothing needs a device)"""
    if case.kind == "uniform":
        C = scatter(cost_class(case.cls, case.ny, case.nx, case.L, case.seed), case.seed, case.recipe or SCATTER)
        return Built([C], [weights(case.wkind, case.ny, case.nx, case.seed)] if case.wkind else None, None, None)
    if case.kind == "batch":  # volume 0 tame and NaN-free; 1 and 2 `ints` and `zeros` with different NaN placements
        Cs = [cost_class("ints", case.ny, case.nx, case.L, case.seed),
              scatter(cost_class("ints", case.ny, case.nx, case.L, case.seed + 100), case.seed + 1),
              scatter(cost_class("zeros", case.ny, case.nx, case.L, case.seed + 200), case.seed + 2)]
        return Built(Cs, [weights(case.wkind, case.ny, case.nx, case.seed + k) for k in range(3)], None, None)
    # ragged: the form of tests/test_gpu_route.py's `ragged` -- windows of exactly RAGGED_WIDTH labels jittered +-2 around the true
    # disparity in a hull of [dmin, dmax] that two pixels attain
    width, dmin, dmax = RAGGED_WIDTH, case.dmin, case.dmin + case.L - 1
    u, v, gt = synth.stereo_pair(case.nx, case.ny, dmin * 3 // 4, 0, seed=300 + width)
    rng = np.random.default_rng(40)
    lo = np.clip(gt - width // 2 + rng.integers(-2, 3, size=gt.shape), dmin, dmax - width + 1).astype(np.float32)
    hi = (lo + width - 1).astype(np.float32)
    lo[0, 0], hi[0, 0] = dmin, dmin + width - 1
    lo[0, 1], hi[0, 1] = dmax - width + 1, dmax
    ilo, ihi = int_ranges(lo, hi)
    C = oracle.costvolume_ranged(u, v, ilo, ihi, dmin, dmax, "none", "census", np.inf, 5)
    return Built([C], [weights(case.wkind, case.ny, case.nx, case.seed)] if case.wkind else None, (lo, hi, ilo, ihi), (u, v))


def must_take_exact(case, built):
    """Raises unless plan_dense_kernels can only choose k_pass_exact for this call (mgm_planner.h: `d.exact`), whatever else the
    volumes, penalties and weights hold.  Decided on host arrays, before anything is uploaded."""
    p2_finite, p1_nonneg = case.P2 < np.inf, case.P1 >= 0
    if case.kind == "ragged":
        wodd = built.w8s is not None and not weights_tame(built.w8s[0])
        ok = (not p2_finite) or (case.FH and ((not p1_nonneg) or wodd))
        if not ok:
            raise AssertionError("%s: a ragged volume inside the fast kernels' premise" % case.name)
        return "ragged"
    if case.L > FAST_LABELS:
        return "labels"
    # an uploaded uniform volume: k_compact / k_nanscan read every word, so a NaN anywhere forces the route
    nan = [bool(np.isnan(C).any()) for C in built.Cs]
    if not any(nan):
        raise AssertionError("%s: no volume holds a NaN -- an odd value here would reach a kernel with a polled hand-off" % case.name)
    for k, C in enumerate(built.Cs):
        if nan[k]:
            continue
        # a NaN-free volume of a batch rides along; it must be tame in case it ever runs alone
        tame = bool((np.isfinite(C) & (C >= 0) & (C <= 24) & (C == np.rint(C))).all() and not np.signbit(C).any())
        pen = np.isfinite(case.P1) and np.isfinite(case.P2) and case.P1 >= 0 and case.P2 >= 0
        if not (tame and pen and weights_tame(built.w8s[k] if built.w8s else None)):
            raise AssertionError("%s: volume %d is NaN-free and not tame" % (case.name, k))
    return "nan"


# ---- the expectation (computed once per case and process, never modified) -------------------------------------------------------
Expected = namedtuple("Expected", "S out cost lr")  # per volume: lists
_EXPECTED = {}


def aggregate_on(engine, case, built, k, C=None, dump_lr=True):
    """volume k of the case on the oracle (or, dump_lr=False, on the compiled reference)"""
    C = built.Cs[k] if C is None else C
    w8 = built.w8s[k] if built.w8s else None
    if case.kind == "ragged":
        lo, hi, ilo, ihi = built.ranges
        if dump_lr:
            return engine.mgm_ranged(C, case.dmin, ilo, ihi, case.P1, case.P2, case.NDIR, case.MGM, case.FH, 1, w8, dump_lr=True)
        return engine.mgm_ranged(C, case.dmin, lo, hi, case.P1, case.P2, case.NDIR, case.MGM, case.FH, 1, w8)
    if dump_lr:
        return engine.mgm(C, case.dmin, case.P1, case.P2, case.NDIR, case.MGM, case.FH, 1, w8, dump_lr=True)
    return engine.mgm(C, case.dmin, case.P1, case.P2, case.NDIR, case.MGM, case.FH, 1, w8)


def expected(case, built, oracle):
    if case.name not in _EXPECTED:
        res = [aggregate_on(oracle, case, built, k) for k in range(len(built.Cs))]
        for r in res:
            for a in r:
                a.setflags(write=False)
        _EXPECTED[case.name] = Expected(*[[r[i] for r in res] for i in range(4)])
    return _EXPECTED[case.name]


# ---- the floors -------------------------------------------------------------------------------------------------------------------
NAN_SHARE = (0.02, 0.7)
ORDER_WORDS = 50
FH_BOUNDARY_WORDS = 50
RAGGED_OWN_SHARE = (0.1, 0.6)
FIXUP_PIXELS = 50
TIE_MINIMA = 50  # slabs per pass whose kept minimum changes sign with the tie rule (`zsign`)
ODD_WORDS = 50   # words per pass that the odd penalty or weight of a NaN-free ragged case decides
MIN_UPDATED = 100  # updated pixels below which the order and boundary floors cannot be asked (see updated_pixels)


def updated_pixels(case):
    """pixels that have all four neighbours of some pass inside the image: at most (nx - 1) * (ny - 1).  A frame pixel's Lr is
    its cost slab whatever a minimum does, and the geometry cases have 0 (one line, one column) to 78 (40x3) others: the floors
    that count what an UPDATE leaves are asked from MIN_UPDATED such pixels on."""
    return max(0, case.nx - 1) * max(0, case.ny - 1)


def nan_shares(lr):
    return [float(np.isnan(p).mean()) for p in lr]


def order_sensitive_words(case, built, oracle, k=0):
    """per pass: the words that change when the volume is aggregated with its label axis reversed and flipped back -- the words
    an operand-swapped minimum would change (Hirschmueller potentials; FH is symmetric under the flip)"""
    straight = expected(case, built, oracle).lr[k]
    flipped = aggregate_on(oracle, case, built, k, C=np.ascontiguousarray(built.Cs[k][:, :, ::-1]))[3]
    return [ndiff(straight[p], flipped[p][:, :, ::-1]) for p in range(case.NDIR)]


def fh_boundary_words(lr):
    """per pass: finite words with a NaN on label +-1 of the same pixel -- where a healed NaN and a spread NaN differ"""
    out = []
    for p in lr:
        nan = np.isnan(p)
        near = np.zeros_like(nan)
        near[:, :, 1:] |= nan[:, :, :-1]
        near[:, :, :-1] |= nan[:, :, 1:]
        out.append(int((np.isfinite(p) & near).sum()))
    return out


def own_labels(case, built):
    """[ny][nx][L]: the labels each pixel owns (all of them in a uniform volume)"""
    if built.ranges is None:
        return np.ones(built.Cs[0].shape, bool)
    _, _, ilo, ihi = built.ranges
    d = case.dmin + np.arange(case.L)[None, None, :]
    return (d >= ilo[..., None]) & (d <= ihi[..., None])


def own_nan_shares(case, built, lr):
    """ragged: per pass, the NaN share of the labels the pixels own"""
    own = own_labels(case, built)
    return [float((np.isnan(p) & own).sum() / own.sum()) for p in lr]


def fixup_pixels(case, built):
    """ragged: (pixels whose left neighbour's range reaches below theirs, pixels whose left neighbour's reaches above) -- where the
    two branches of FixBounrady_for_minConvTruncatedLinear have work.  Every pass has a horizontal or diagonal neighbour and the
    windows are jittered independently per pixel: the left neighbour stands for them."""
    _, _, ilo, ihi = built.ranges
    return int((ilo[:, :-1] < ilo[:, 1:]).sum()), int((ihi[:, :-1] > ihi[:, 1:]).sum())


def tie_sensitive_minima(lr):
    """per pass: the slabs whose minimum is a zero and whose FIRST zero (the one Dvec::get_minvalue keeps, strict `<` in label order)
    differs in sign from the first zero of the last lane-chunk that holds one (the one a lane combine with `<=` would keep)"""
    out = []
    for vol in lr:
        ny, nx, L = vol.shape
        chunk, n = lane_chunk(L), 0
        for slab in vol.reshape(ny * nx, L):
            z = np.flatnonzero(slab == 0)
            if z.size == 0 or np.nanmin(slab) < 0:
                continue
            last = z[z // chunk == z[-1] // chunk][0]
            n += bool(np.signbit(slab[z[0]]) != np.signbit(slab[last]))
        out.append(n)
    return out


def tame_twin(case):
    """the ragged FH cases whose odd value is a penalty or a weight: the same call inside the fast kernels' premise"""
    return case._replace(P1=abs(case.P1), wkind=None)


def order_floor_asked(case):
    """Hirschmueller cases of `ints` and `negfrac` in which the term min(L[o-1], L[o+1]) + P1 -- the one minimum whose operand
    order matters to a NaN -- can win fmin3 at all: P1 finite (NaN: `m > b` is false; +INF: never below L[o]) and below P2
    (P2 <= P1 on costs that are whole multiples: m + P2 <= min(..) + P1 always, and fmin3 tests P2's term last with a strict
    `>`); and three labels or more: with two, one operand of that minimum is always the +INF beyond the slab and its result never
    beats L[o].  Measured on the oracle: 0 order-sensitive words in every pass for (0, 0), (3, 1), (+INF, +INF), (NaN, 32), (8, -INF)."""
    return (not case.FH and case.cls in ("ints", "negfrac") and case.kind == "uniform" and case.L >= 3
            and updated_pixels(case) >= MIN_UPDATED and bool(np.isfinite(case.P1)) and not case.P2 <= case.P1)


def check_floors(case, built, oracle):
    """-> the figures of the case (a dict); raises where a floor is missed"""
    exp = expected(case, built, oracle)
    fig = {}
    if case.kind == "ragged":
        shares = own_nan_shares(case, built, exp.lr[0])
        fig["own_nan_share"] = shares
        if case.FH and case.MGM == 2 and case.wkind is None:  # (update_cost2_trunclinear: the one function with the fix-up)
            fig["fixup_pixels"] = fixup_pixels(case, built)
            assert min(fig["fixup_pixels"]) >= FIXUP_PIXELS, (case.name, fig)
        # (update_cost2_trunclinear's fix-up carries the neighbour's values beyond the range into it: no slab is all +INF and no
        # NaN arises -- 0.0 in every pass -- so that case is held to the fix-up's floor above alone)
        if not case.P2 < np.inf and not (case.FH and case.MGM == 2 and case.wkind is None):
            assert any(RAGGED_OWN_SHARE[0] <= s <= RAGGED_OWN_SHARE[1] for s in shares), (case.name, shares)
        if case.P2 < np.inf:
            # a negative slope, a weight of 0 or -1: no NaN arises (0.0 in every pass), so what keeps such a case from passing as an
            # ordinary volume is that its odd value decides words: every pass differs from the tame twin's in ODD_WORDS words
            twin = tame_twin(case)
            tb = built._replace(w8s=None)
            tame = aggregate_on(oracle, twin, tb, 0)[3]
            fig["words_unlike_tame_twin"] = [ndiff(exp.lr[0][p], tame[p]) for p in range(case.NDIR)]
            assert min(fig["words_unlike_tame_twin"]) >= ODD_WORDS, (case.name, fig)
        return fig
    for k, C in enumerate(built.Cs):
        if not np.isnan(C).any():
            continue  # (the tame volume of the batch)
        shares = nan_shares(exp.lr[k])
        fig.setdefault("nan_share", []).append(shares)
        assert all(NAN_SHARE[0] <= s <= NAN_SHARE[1] for s in shares), (case.name, k, shares)
        if case.FH and case.L >= 2 and updated_pixels(case) >= MIN_UPDATED:
            words = fh_boundary_words(exp.lr[k])
            fig.setdefault("fh_boundary_words", []).append(words)
            assert min(words) >= FH_BOUNDARY_WORDS, (case.name, k, words)
        if case.cls == "zsign":
            fig["tie_sensitive_minima"] = tie_sensitive_minima(exp.lr[k])
            assert min(fig["tie_sensitive_minima"]) >= TIE_MINIMA, (case.name, fig)
        if order_floor_asked(case):
            words = order_sensitive_words(case, built, oracle, k)
            fig.setdefault("order_words", []).append(words)
            assert max(words) >= ORDER_WORDS, (case.name, k, words)
    return fig
