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


# ---- the instance cases (wta_prune_model.INSTANCE_CASES; tests/test_gpu_wta_pruned_instances.py runs them on the device) -----
INSTANCES = sorted(M.INSTANCE_CASES)


def shares(r, dmin):
    """(chunks loaded / all, winners outside the seed chunk / labelled pixels, winners per chunk, pixels without a label) -- of the
    ORACLE's maps, the model's bound and its load set."""
    ny, nx, L = r["C"].shape
    nch = L // M.CHUNK
    lab = ~np.isnan(r["out"])
    win = (r["out"][lab] - dmin).astype(np.int64) // M.CHUNK
    outside = float((win != M.seed_chunks(r["C"], r["LB"])[lab]).mean()) if lab.any() else 0.0
    return r["chunks"] / (nx * ny * nch), outside, np.bincount(win, minlength=nch), int((~lab).sum())


@pytest.mark.parametrize("name", INSTANCES)
def test_instance_case_is_not_empty(oracle, name):
    """The floors of a case, met by the reference side alone (seeds are picked for them; they are not measurements).

    Measured with this file's generator (ramp_volume seed 7, dmin -100; chunks loaded / all, winners outside the seed chunk, vfit
    neighbours in a chunk that stayed out):
      97x33  NDIR 8 TSGM 3 FH  P 2/20000   fix 1: 0.46 0.52 34     NDIR 8 TSGM 3 Hi P 8/32     fix 1: 0.69 0.64 12
             NDIR 5 TSGM 3 Hi  P 8/32      fix 0: 0.13 0.04 206    NDIR 3 TSGM 4 FH P 0.3/1.7  fix 1: 0.62 0.73 3
             NDIR 7 TSGM 1 Hi  P 8.1/32.3  fix 1: 0.66 0.59 10     NDIR 6 TSGM 3 FH P 2/9      fix 1: 0.70 0.91 6
             NDIR 4 TSGM 3 Hi  P 8/32      fix 1: 0.60 0.44 7      NDIR 1 TSGM 3 Hi P 8/32     fix 1: 0.125 0.00 206
             NDIR 2 TSGM 1 FH  P 2/20000   fix 1: 0.28 0.08 26     NDIR 8 TSGM 3 FH P 2/20000  fix 0: 0.125 0.00 225
             every chunk the winner of at least 27 pixels in the fix = 1, NDIR >= 3 rows (304..380 in all but the first)
      61x19 and 33x17: the same shares within 0.03 (Hirschmueller 8-dir: +0.13 / +0.23 of winners outside), 1..82 and 1..53 neighbours
      wide_pair(41), 8 directions, TSGM 3: census 0.29 / 0.12 (FH and Hirschmueller; 180 and 1879 neighbours); AD 0.58 / 0.48 (FH),
             0.66 / 0.60 (Hirschmueller), 0 neighbours; AD with truncDist 30 0.30 / 0.09 (FH, 95), 0.38 / 0.11 (Hirschmueller, 1237)
    In all of them the model's S is the oracle's, LB <= S on every finite cell, and the emulation returns the oracle's maps, with
    and without vfit, bit for bit."""
    spec = M.INSTANCE_CASES[name]
    inp, NDIR, MGM, FH, P1, P2, fix, refine, floor = spec
    dmin = M.case_dmin(spec)
    assert (floor == "compete") == (inp[0] == "ramp" and inp[1] * inp[2] >= 160 and fix == 1 and NDIR >= 3), "the floor is decided by the case, not chosen"
    for b, r in enumerate(M.case_reference(oracle, name)):
        load, outside, per_chunk, unlabelled = shares(r, dmin)
        print("%s[%d]: %.3f of the chunks loaded, %.3f of the winners outside the seed chunk, winners per chunk %s, %d vfit neighbours out"
              % (name, b, load, outside, per_chunk.tolist(), r["nout"]))
        assert unlabelled == 0
        assert load >= 0.125
        if floor == "compete":
            assert load <= 0.80 and outside >= 0.30 and per_chunk.min() >= 20
        if inp[0] == "pair":   # one byte per cost on the device: no finite cost above 254, whole numbers only
            fin = r["C"][np.isfinite(r["C"])]
            assert fin.max() <= 254 and np.array_equal(fin, np.rint(fin))
        if refine == "vfit":
            assert r["nout"] >= 1, "vfit never recomputes a neighbour here: run the case without it or pick another seed"


def test_some_vfit_case_recomputes_many_neighbours(oracle):
    most = max(r["nout"] for n in INSTANCES if M.INSTANCE_CASES[n][7] == "vfit" for r in M.case_reference(oracle, n))
    assert most >= 40


def test_instance_cases_cover_every_setting():
    s = list(M.INSTANCE_CASES.values())
    assert {c[1] for c in s} == set(range(1, 9))                       # NDIR
    assert {c[6] for c in s} == {0, 1} and {c[2] for c in s} == {1, 3, 4} and {c[3] for c in s} == {0, 1}
    assert any(c[4] != int(c[4]) for c in s)                           # fractional penalties
    assert {c[0][1:] for c in s if c[0][0] == "pair"} == {("census", np.inf), ("ad", np.inf), ("ad", 30.0)}
    assert any(c[6] == 0 and c[7] == "vfit" for c in s)


@pytest.mark.parametrize("name", INSTANCES)
def test_instance_case_bound_and_maps(oracle, name):
    spec = M.INSTANCE_CASES[name]
    for r in M.case_reference(oracle, name):
        assert ndiff(r["Sm"], r["S"]) == 0, "the model's sum-and-fix chain is not the oracle's"
        fin = np.isfinite(r["S"])
        assert fin.any() and not np.isnan(r["LB"][fin]).any()
        assert int(np.sum(r["LB"][fin] > r["S"][fin])) == 0
        assert ndiff(r["label"], r["out"]) == 0 and ndiff(r["cost"], r["outc"]) == 0
        assert ndiff(r["vlabel"], r["vout"]) == 0 and ndiff(r["vcost"], r["voutc"]) == 0, "the model's vfit step is not oracle.refine"


def test_one_dead_pixel_is_the_oracle_s_to_decide(oracle):
    """One pixel +INF on all labels: behind it the oracle's Lr is INF - INF = NaN along every scan line, the minima of those chunks
    are NaN and so are their bounds.  The kernel's fminf drops a NaN bound, so such a pixel loads nothing -- and has nothing to
    find: S is NaN on all its labels.  The emulation does the same and still returns the oracle's maps, with and without vfit."""
    C = M.dead_pixel_volume()
    y, x = C.shape[0] // 2, C.shape[1] // 3
    S, out, outc, lr = oracle.mgm(C, M.RAMP_DMIN, 8.0, 32.0, 8, 1, 0, 1, dump_lr=True)
    assert np.isnan(out[y, x]) and not np.isfinite(outc[y, x])
    assert 1 < int(np.isnan(out).sum()) < out.size // 4, "the dead pixel's NaN must reach its scan lines and must not take the image"
    with np.errstate(invalid="ignore"):
        label, cost, chunks, Sm, LB, load = M.pruned_search(C, lr, M.RAMP_DMIN, 1)
        nanbound = np.isnan(LB) & (C < np.inf)
    assert nanbound.any() and not np.isfinite(S[nanbound]).any()
    assert not load[np.isnan(out)].any()
    assert ndiff(label, out) == 0 and ndiff(cost, outc) == 0
    vout, voutc = oracle.refine(S, M.RAMP_DMIN, "vfit", out, outc)
    vl, vc, _ = M.vfit_step(Sm, load, M.RAMP_DMIN, label, cost)
    assert ndiff(vl, vout) == 0 and ndiff(vc, voutc) == 0
