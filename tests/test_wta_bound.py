"""The bound behind the pruned winner search, on the CPU: with the minimum of every 32-label chunk of Lr in the place of the Lr
values, the sum-and-fix chain of the search gives LB <= S in float32 on every finite cell (no epsilon: IEEE addition and
s - f*c are monotone), and the search that only reads the chunks whose bound can still beat the seed chunk's best (the numpy
emulation of steps a-d in wta_prune_model.py) returns the oracle's label and cost maps bit for bit."""
import numpy as np
import pytest

import wta_prune_model as M
from helpers import ndiff

SEED_A, SEED_B, SEED_C = M.SEEDS  # (tests/test_gpu_wta_pruned.py runs the same inputs on the device)

# name: (dmin, dmax, NDIR, TSGM, FH, P1, P2, pair)
CASES = {
    "fh_256": (-255, 0, 8, 3, 1, 2.0, 20000.0, ("textured", SEED_A)),
    "hirsch_256": (-255, 0, 8, 3, 0, 8.0, 32.0, ("textured", SEED_A)),
    "fh_256_b": (-255, 0, 8, 3, 1, 2.0, 20000.0, ("textured", SEED_B)),
    "hirsch_256_c": (-255, 0, 8, 3, 0, 8.0, 32.0, ("textured", SEED_C)),
    "fh_128_4dir": (-127, 0, 4, 3, 1, 2.0, 20000.0, ("textured", SEED_B)),
    "both_sides": (-128, 127, 8, 3, 1, 2.0, 20000.0, ("textured", SEED_B)),  # the windows leave the right image on both sides
    "constant": (-255, 0, 8, 3, 1, 2.0, 20000.0, ("constant", 0)),
}
_cache = {}


def run_case(oracle, name):
    """(C, lr, oracle label map, oracle cost map, model results), computed once per case."""
    if name not in _cache:
        dmin, dmax, NDIR, MGM, FH, P1, P2, (kind, seed) = CASES[name]
        u, v = M.constant_pair() if kind == "constant" else M.textured_pair(dmin, dmax, seed)
        C = oracle.costvolume(u, v, dmin, dmax, "none", "census", np.inf, 5)
        S, out, outc, lr = oracle.mgm(C, dmin, P1, P2, NDIR, MGM, FH, 1, dump_lr=True)
        _cache[name] = (C, lr, S, out, outc, M.pruned_search(C, lr, dmin, 1))
        for a in (C, lr, S, out, outc):
            a.setflags(write=False)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_bound_holds_on_every_finite_cell(oracle, name):
    C, lr, S, out, outc, (label, cost, chunks, Sm, LB, load) = run_case(oracle, name)
    assert ndiff(Sm, S) == 0, "the model's sum-and-fix chain is not the oracle's"
    fin = np.isfinite(S)
    assert fin.any()
    assert not np.isnan(LB[fin]).any()
    assert int(np.sum(LB[fin] > S[fin])) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_pruned_search_returns_the_oracle_maps(oracle, name):
    C, lr, S, out, outc, (label, cost, chunks, Sm, LB, load) = run_case(oracle, name)
    assert ndiff(label, out) == 0
    assert ndiff(cost, outc) == 0
    npix, nch = C.shape[0] * C.shape[1], C.shape[2] // M.CHUNK
    assert chunks >= npix  # every pixel reads its seed chunk
    print("%s: %d chunks for %d pixels (%.2f of %d per pixel)" % (name, chunks, npix, chunks / npix, nch))
    if CASES[name][7][0] == "textured":
        assert chunks <= 0.4 * npix * nch, "pick another seed: the GPU test expects the emulation to read at most 40 % of the chunks"


def test_constant_pair_reads_every_tied_chunk_and_takes_the_lowest_label(oracle):
    """A constant pair.  Not every label ties here: the labels whose window leaves the right image cost +INF, and next to them S
    rises, so most pixels have their ties inside one chunk (test_constant_volume_every_label_ties has the all-ties case).
    Where labels of several chunks do tie with the winner, every such chunk must be read (`<=`, not `<`), and the winner is
    the lowest tying label."""
    C, lr, S, out, outc, (label, cost, chunks, Sm, LB, load) = run_case(oracle, "constant")
    dmin = CASES["constant"][0]
    ties = (S == outc[..., None]).reshape(S.shape[0], S.shape[1], -1, M.CHUNK).any(axis=3)
    assert int((ties.sum(axis=2) >= 2).sum()) > 0, "no ties across chunks: the case tests nothing"
    assert not (ties & ~load).any()
    lowest = np.argmax(S == outc[..., None], axis=2) + dmin
    assert np.array_equal(label, lowest.astype(np.float32))


def test_constant_volume_every_label_ties(oracle):
    """One cost for every label of every pixel: every S ties, so every chunk must be read and the lowest label wins."""
    L, dmin = 256, -255
    C = M.constant_volume(L)
    S, out, outc, lr = oracle.mgm(C, dmin, 2.0, 20000.0, 8, 3, 1, 1, dump_lr=True)
    label, cost, chunks, Sm, LB, load = M.pruned_search(C, lr, dmin, 1)
    assert ndiff(label, out) == 0 and ndiff(cost, outc) == 0
    assert load.all() and chunks == M.NX * M.NY * (L // M.CHUNK)
    assert np.array_equal(out, np.full(out.shape, dmin, np.float32))


def test_planted_winners_at_chunk_edges_and_range_ends(oracle):
    L, dmin = 256, -100
    C, where = M.planted_volume(L)
    S, out, outc, lr = oracle.mgm(C, dmin, 8.0, 32.0, 8, 3, 0, 1, dump_lr=True)
    label, cost, chunks, Sm, LB, load = M.pruned_search(C, lr, dmin, 1)
    assert ndiff(label, out) == 0 and ndiff(cost, outc) == 0
    assert int(np.sum(LB > S)) == 0
    inner = np.zeros(where.shape, bool)
    inner[3:-3, 3:-3] = True
    inner[M.NY // 2 - 3: M.NY // 2 + 3, :] = False
    inner[:, M.NX // 2 - 3: M.NX // 2 + 3] = False
    assert np.array_equal(out[inner], (where[inner] + dmin).astype(np.float32)), "the planted labels do not win: the case tests nothing"
