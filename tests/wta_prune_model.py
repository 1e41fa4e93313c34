"""The pruned winner search (mgm_amd/csrc/mgm_wta.hip, k_wta_pruned) in numpy, float32 throughout: chunk minima of the
per-pass Lr volumes, the lower bound they give on S, and steps (a)-(d) of the search, vfit included.  tests/test_wta_bound.py checks it
against the oracle on the CPU; tests/test_gpu_wta_pruned.py and tests/test_gpu_wta_pruned_instances.py take its chunk count as the
figure the kernel's counter is held to.  Shared inputs and the instance case table of these files live here too."""
import numpy as np

from mgm_amd import synth

CHUNK = 32  # labels per chunk minimum: 128 bytes of an Lr slab
SEEDS = (41, 42, 43)  # of the textured pairs both test files run: the emulation reads at most 40 % of their chunks (test_wta_bound.py)


def sum_fix(terms, C, fix):
    """S = ((0 + t0) + t1) + ... in pass order, then S - (NDIR-1) * C (mgm_core.cc:582-599): the kernels' operations and order."""
    S = np.zeros(C.shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in terms:
            S = S + t
        if fix:
            S = S - np.float32(len(terms) - 1) * C
    assert S.dtype == np.float32
    return S


def chunk_minima(lr):
    """min over every chunk of 32 consecutive labels, per pass and pixel: (NDIR, ny, nx, L/32), float32; +INF enters as +INF."""
    nd, ny, nx, L = lr.shape
    assert L % CHUNK == 0 and lr.dtype == np.float32
    return lr.reshape(nd, ny, nx, L // CHUNK, CHUNK).min(axis=4)


def lower_bound(C, lr, fix, minima=None):
    m = chunk_minima(lr) if minima is None else minima
    return sum_fix([np.repeat(m[p], CHUNK, axis=2) for p in range(lr.shape[0])], C, fix)


def pruned_search(C, lr, dmin, fix=1, minima=None):
    """Steps (a)-(d); `minima`: the chunk minima to bound with, (NDIR, ny, nx, L/32), instead of chunk_minima(lr).  Returns (label map, cost map, chunks loaded, S, LB, load): labels as floats (dmin + index, NaN where no
    S is finite), costs (+INF there), the number of (pixel, chunk) pairs whose Lr values the search reads and which they are."""
    ny, nx, L = C.shape
    nch = L // CHUNK
    S = sum_fix(list(lr), C, fix)
    LB = lower_bound(C, lr, fix, minima)
    # (a) a label with C = +INF is out, and so is a label whose bound is NaN: the kernel folds the bounds with fminf, which returns
    # its other operand.  A NaN bound means a NaN minimum (costs are >= 0: no INF - INF in the chain), i.e. a chunk of Lr that is NaN
    # on every label in that pass, so S is NaN on the label too and cannot win
    lb = np.where((C < np.inf) & ~np.isnan(LB), LB, np.inf).astype(np.float32)
    clb = lb.reshape(ny, nx, nch, CHUNK).min(axis=3)
    gmin = clb.min(axis=2)
    some = gmin < np.inf
    seed = np.argmax(clb == gmin[..., None], axis=2)  # the lowest chunk holding the smallest bound
    # (b) the seed chunk's exact S
    Sc = S.reshape(ny, nx, nch, CHUNK)
    fin = np.isfinite(Sc)
    cmin = np.where(fin, Sc, np.inf).min(axis=3)  # per chunk: smallest finite S
    best0 = np.take_along_axis(cmin, seed[..., None], axis=2)[..., 0]
    # (c) every other chunk with some LB <= best0
    is_seed = np.arange(nch)[None, None, :] == seed[..., None]
    load = (is_seed | (clb <= best0[..., None])) & some[..., None]
    # (d) first strict minimum among the finite S of what was loaded
    cand = np.where(fin & load[..., None], Sc, np.inf).reshape(ny, nx, L)
    idx = np.argmin(cand, axis=2)
    cost = np.take_along_axis(cand, idx[..., None], axis=2)[..., 0].astype(np.float32)
    found = cost < np.inf
    label = np.where(found, (idx + dmin).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    return label, cost, int(load.sum()), S, LB, load


def vfit_step(S, load, dmin, label, cost):
    """The vfit step of (d) on pruned_search's maps (refine.h:70-92 behind the gate of mgm_refine.h:58), float32 throughout.  The
    kernel reads S at the winner's neighbours from the staged chunks or, where a neighbour lies in a chunk that stayed out,
    recomputes it from memory by sum_fix's operations -- the same float either way, so S serves for both.  Returns (label map,
    cost map, winners with a neighbour in a chunk that stayed out)."""
    ny, nx, L = S.shape
    found = ~np.isnan(label)
    bi = np.where(found, label - np.float32(dmin), 0).astype(np.int64)
    gate = found & (bi - 1 >= 0) & (bi + 2 <= L - 1)
    b = np.where(gate, bi, 1)
    at = lambda o: np.take_along_axis(S, o[..., None], axis=2)[..., 0]
    v0, v1, v2 = at(b - 1), at(b), at(b + 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        slope = np.where((v2 - v1) < (v0 - v1), v0 - v1, v2 - v1).astype(np.float32)
        x = ((v0 - v2) / (np.float32(2.0) * slope)).astype(np.float32)
        vmin = (v2 + (x - np.float32(1.0)) * slope).astype(np.float32)
        peak = (v1 > v0) & (v1 > v2)
        x = np.where(peak, np.float32(0.0), x)
        vmin = np.where(peak, v1, vmin)
        out = np.where(gate, (b + dmin).astype(np.float32) + x, label).astype(np.float32)
    outc = np.where(gate, vmin, cost).astype(np.float32)
    ld = lambda o: np.take_along_axis(load, (o // CHUNK)[..., None], axis=2)[..., 0]
    return out, outc, int((gate & ~(ld(b - 1) & ld(b + 1))).sum())


# ---- shared inputs ----------------------------------------------------------------------------------------------------------
NX, NY = 96, 34  # three bands of row lines, seven of column lines in the 256-label pass kernels


def textured_pair(dmin, dmax, seed):
    gt_lo = max(dmin, -(NX // 2))
    u, v, _ = synth.stereo_pair(NX, NY, gt_lo, min(dmax, 0), seed=seed)
    return u, v


def constant_pair():
    u = np.full((1, NY, NX), 100.0, np.float32)
    return u, u.copy()


def constant_volume(L):
    return np.full((NY, NX, L), 7.0, np.float32)


def planted_volume(L, seed=5):
    """Integer costs (the compact path) whose smallest entry per pixel is PLANTED, by image quarter, at labels 31, 32, 0 and
    L-1: winners on both sides of a chunk edge and at both ends of the range.  (A pair of 96-pixel-wide images cannot put a
    winner at label L-1 of 256: that disparity leaves the right image at every pixel, so this case is a cost volume.)"""
    rng = np.random.default_rng(seed)
    C = rng.integers(40, 90, (NY, NX, L)).astype(np.float32)
    where = np.zeros((NY, NX), np.int64)
    where[: NY // 2, : NX // 2] = 31
    where[: NY // 2, NX // 2:] = 32
    where[NY // 2:, : NX // 2] = 0
    where[NY // 2:, NX // 2:] = L - 1
    np.put_along_axis(C, where[..., None], 0.0, axis=2)
    return C, where


def ramp_volume(nx, ny, L=256, seed=7):
    """Integer costs (the compact path) in which the chunks COMPETE: every label finite before a few +INF are planted, two noisy
    valleys half the label range apart whose position sweeps all L labels along each row.  2 % of the cells and nx*ny/10 whole
    (pixel, chunk) pairs are +INF; no pixel is +INF on all its labels."""
    rng = np.random.default_rng(seed)
    y, x, d = np.arange(ny)[:, None, None], np.arange(nx)[None, :, None], np.arange(L)[None, None, :]
    gt = ((x * (L - 1)) // max(nx - 1, 1) + 5 * (y % 3)) % L
    C = np.minimum(np.abs(d - gt) * 3, 120) + rng.integers(0, 13, (ny, nx, L))
    C = np.minimum(C, np.minimum(np.abs(d - (gt + L // 2) % L) * 3, 120) + rng.integers(0, 13, (ny, nx, L)) + 2).astype(np.float32)
    keep = C[np.arange(ny)[:, None], np.arange(nx)[None, :], gt[..., 0]].copy()
    C[rng.random((ny, nx, L)) < 0.02] = np.inf
    n = nx * ny // 10
    py, px, pc = rng.integers(0, ny, n), rng.integers(0, nx, n), rng.integers(0, L // CHUNK, n)
    for a, b, c in zip(py, px, pc):
        C[a, b, c * CHUNK:(c + 1) * CHUNK] = np.inf
    dead = ~np.isfinite(C).any(axis=2)
    C[dead, gt[..., 0][dead]] = keep[dead]
    return C


def wide_pair(seed):
    """330 pixels wide for 256 labels: every label of most pixels stays inside the right image."""
    u, v, _ = synth.stereo_pair(330, 18, -255, 0, seed=seed)
    return u, v


# ---- the instance cases: tests/test_wta_bound.py (CPU) and tests/test_gpu_wta_pruned_instances.py (device) --------------------
RAMP_DMIN = -100
PAIR_SEED = 41
# name: (input, NDIR, TSGM, FH, P1, P2, fix, refinement of the device run, floor)
#   input: ("ramp", nx, ny, seeds of the batch) -> ramp_volume, uploaded as a volume (k_compact makes the bytes);
#          ("pair", distance, truncDist) -> wide_pair(PAIR_SEED), census window 5, built on the device;
#   floor (what tests/test_wta_bound.py asks of the reference side before anything is compared):
#     "compete": at most 0.80 of the chunks loaded, at least 0.30 of the winners outside the seed chunk, each of the eight chunks the
#                winner of at least 20 pixels, no pixel without a label -- every ramp case with fix = 1 and NDIR >= 3;
#     "tight":   fix = 0 or NDIR <= 2, about one chunk per pixel: at least 0.125 of the chunks loaded, no pixel without a label;
#     "pair":    as "tight" (a pair's winners sit where its disparity planes are, not in every chunk);
#     "launch":  17, 17 and 15 pixels -- a launch shape, not a population: eight chunks cannot each win 20 pixels; as "tight".
INSTANCE_CASES = {
    "r97_fh8_vfit": (("ramp", 97, 33, (7,)), 8, 3, 1, 2.0, 20000.0, 1, "vfit", "compete"),
    "r97_hi8_none": (("ramp", 97, 33, (7,)), 8, 3, 0, 8.0, 32.0, 1, None, "compete"),
    "r97_hi5_nofix_vfit": (("ramp", 97, 33, (7,)), 5, 3, 0, 8.0, 32.0, 0, "vfit", "tight"),
    "r97_fh3_t4_frac_vfit": (("ramp", 97, 33, (7,)), 3, 4, 1, 0.3, 1.7, 1, "vfit", "compete"),
    "r97_hi7_t1_frac_none": (("ramp", 97, 33, (7,)), 7, 1, 0, 8.1, 32.3, 1, None, "compete"),
    "r97_fh6_none": (("ramp", 97, 33, (7,)), 6, 3, 1, 2.0, 9.0, 1, None, "compete"),
    "r97_hi4_vfit": (("ramp", 97, 33, (7,)), 4, 3, 0, 8.0, 32.0, 1, "vfit", "compete"),
    "r97_hi1_vfit": (("ramp", 97, 33, (7,)), 1, 3, 0, 8.0, 32.0, 1, "vfit", "tight"),
    "r97_fh2_t1_none": (("ramp", 97, 33, (7,)), 2, 1, 1, 2.0, 20000.0, 1, None, "tight"),
    "r97_fh8_nofix_none": (("ramp", 97, 33, (7,)), 8, 3, 1, 2.0, 20000.0, 0, None, "tight"),
    "r61_hi5_t4_x2_vfit": (("ramp", 61, 19, (7, 8)), 5, 4, 0, 8.0, 32.0, 1, "vfit", "compete"),
    "r61_hi4_x3_none": (("ramp", 61, 19, (7, 8, 9)), 4, 3, 0, 8.0, 32.0, 1, None, "compete"),
    "r33_fh8_vfit": (("ramp", 33, 17, (7,)), 8, 3, 1, 2.0, 20000.0, 1, "vfit", "compete"),
    "r33_hi7_t1_frac_vfit": (("ramp", 33, 17, (7,)), 7, 1, 0, 8.1, 32.3, 1, "vfit", "compete"),
    "r33_fh3_t4_none": (("ramp", 33, 17, (7,)), 3, 4, 1, 0.3, 1.7, 1, None, "compete"),
    "p330_census_fh8_vfit": (("pair", "census", np.inf), 8, 3, 1, 2.0, 20000.0, 1, "vfit", "pair"),
    "p330_census_hi6_none": (("pair", "census", np.inf), 6, 3, 0, 8.0, 32.0, 1, None, "pair"),
    "p330_ad_fh8_none": (("pair", "ad", np.inf), 8, 3, 1, 2.0, 20000.0, 1, None, "pair"),
    "p330_ad_hi8_nofix_none": (("pair", "ad", np.inf), 8, 3, 0, 8.0, 32.0, 0, None, "pair"),
    "p330_adt30_hi8_vfit": (("pair", "ad", 30.0), 8, 3, 0, 8.0, 32.0, 1, "vfit", "pair"),
    "p330_adt30_fh5_t4_vfit": (("pair", "ad", 30.0), 5, 4, 1, 2.0, 20000.0, 1, "vfit", "pair"),
    "t17x1_fh8_none": (("ramp", 17, 1, (7,)), 8, 3, 1, 2.0, 20000.0, 1, None, "launch"),
    "t1x17_hi4_none": (("ramp", 1, 17, (7,)), 4, 3, 0, 8.0, 32.0, 1, None, "launch"),
    "t5x3_fh3_t4_none": (("ramp", 5, 3, (7,)), 3, 4, 1, 0.3, 1.7, 1, None, "launch"),
}


def case_dmin(spec):
    return RAMP_DMIN if spec[0][0] == "ramp" else -255


def case_costs(oracle, spec):
    """The cost volumes of a case's batch, as the oracle has them."""
    inp = spec[0]
    if inp[0] == "ramp":
        return [ramp_volume(inp[1], inp[2], 256, s) for s in inp[3]]
    u, v = wide_pair(PAIR_SEED)
    return [oracle.costvolume(u, v, -255, 0, "none", inp[1], inp[2], 5)]


_case_ref = {}


def case_reference(oracle, name):
    """Per volume of the batch, computed once and left read-only: a dict of the costs C, the oracle's lr, S, maps without
    refinement (out, outc) and after vfit (vout, voutc), the emulation's results (label, cost, chunks, load, its vfit maps vlabel /
    vcost, nout = winners with a vfit neighbour in a chunk that stayed out) and LB."""
    if name not in _case_ref:
        spec = INSTANCE_CASES[name]
        _, NDIR, MGM, FH, P1, P2, fix, _, _ = spec
        dmin = case_dmin(spec)
        res = []
        for C in case_costs(oracle, spec):
            S, out, outc, lr = oracle.mgm(C, dmin, P1, P2, NDIR, MGM, FH, fix, dump_lr=True)
            vout, voutc = oracle.refine(S, dmin, "vfit", out, outc)
            label, cost, chunks, Sm, LB, load = pruned_search(C, lr, dmin, fix)
            vlabel, vcost, nout = vfit_step(Sm, load, dmin, label, cost)
            r = dict(C=C, lr=lr, S=S, out=out, outc=outc, vout=vout, voutc=voutc, label=label, cost=cost, chunks=chunks, Sm=Sm, LB=LB, load=load,
                     vlabel=vlabel, vcost=vcost, nout=nout)
            for a in r.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            res.append(r)
        _case_ref[name] = res
    return _case_ref[name]


def seed_chunks(C, LB):
    """The seed chunk of every pixel (step (a)): the lowest chunk holding the smallest bound."""
    ny, nx, L = C.shape
    lb = np.where((C < np.inf) & ~np.isnan(LB), LB, np.inf).reshape(ny, nx, L // CHUNK, CHUNK).min(axis=3)
    return np.argmax(lb == lb.min(axis=2)[..., None], axis=2)


def dead_pixel_volume(nx=61, ny=19, seed=7):
    """ramp_volume with ONE pixel +INF on all its labels (the single non-finite case the pruned path is asked about)."""
    C = ramp_volume(nx, ny, 256, seed)
    C[ny // 2, nx // 3, :] = np.inf
    return C
