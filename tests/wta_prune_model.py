"""The pruned winner search (mgm_amd/csrc/mgm_wta.hip, k_wta_pruned) in numpy, float32 throughout: chunk minima of the
per-pass Lr volumes, the lower bound they give on S, and steps (a)-(d) of the search.  tests/test_wta_bound.py checks it
against the oracle on the CPU; tests/test_gpu_wta_pruned.py takes its chunk count as the figure the kernel's counter is held to.
Shared inputs of the two files live here too."""
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


def lower_bound(C, lr, fix):
    m = chunk_minima(lr)
    return sum_fix([np.repeat(m[p], CHUNK, axis=2) for p in range(lr.shape[0])], C, fix)


def pruned_search(C, lr, dmin, fix=1):
    """Steps (a)-(d).  Returns (label map, cost map, chunks loaded, S, LB, load): labels as floats (dmin + index, NaN where no
    S is finite), costs (+INF there), the number of (pixel, chunk) pairs whose Lr values the search reads and which they are."""
    ny, nx, L = C.shape
    nch = L // CHUNK
    S = sum_fix(list(lr), C, fix)
    LB = lower_bound(C, lr, fix)
    # (a) a label with C = +INF is out; a NaN bound bounds nothing (-INF)
    lb = np.where(C < np.inf, np.where(np.isnan(LB), -np.inf, LB), np.inf).astype(np.float32)
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
