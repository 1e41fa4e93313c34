"""plan_holes (mgm_amd/csrc/mgm_planner.h) on the host: a choice is a function of the request alone, the bands cover the rows
exactly, every grid is at least one workgroup and large enough for its work, bad requests are refused, and the scratch is the
planes the kernels index."""
import numpy as np
import pytest

from holes_model import plan, plan_lib

REFUSE, LINES = 0, 1
INT_MAX = 2 ** 31 - 1
SHAPES = [(1, 1), (1, 9), (7, 1), (3, 4), (63, 63), (64, 64), (65, 65), (129, 129), (200, 200), (1920, 1080), (1080, 1920), (4096, 4097),
          (5000, 4096), (INT_MAX, 1), (1, INT_MAX), (46340, 46340), (65536, 32767)]
DIRS = (2, 4, 8)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = plan_lib(tmp_path_factory.mktemp("holesplan"))
    assert lib.holes_request_bytes() == 4 * 4 and lib.holes_choice_bytes() == 6 * 8 + 6 * 4
    return lib


def test_bands_cover_the_rows_exactly_and_the_grids_hold_the_work(lib):
    threads = lib.holes_threads()
    rows = [(nx, ny, dirs, 256) for nx, ny in SHAPES for dirs in DIRS]
    for (nx, ny, dirs, _), c in zip(rows, plan(lib, rows)):
        assert c["family"] == LINES, (nx, ny, dirs)
        chunk, band, nbands = c["chunk"], c["band"], c["nbands"]
        assert chunk == 64 and threads % chunk == 0                       # one pixel per lane of a wave, whole waves per workgroup
        assert band >= 1 and (nbands - 1) * band < ny <= nbands * band     # no empty band, no row outside one
        assert nbands <= band                                              # the look-back over carry-outs costs no more than a band's walk
        assert c["walk_dirs"] == dirs - 2 and c["planes"] == dirs
        assert c["nlines"] == nx + ny - 1                                  # the diagonals of one orientation; the columns are nx of them
        waves = 2 * ny                                                     # k_holes_rows: one wave per (row, direction 0 / 1)
        per = threads // chunk
        assert c["grid_rows"] >= 1 and (c["grid_rows"] - 1) * per < waves <= c["grid_rows"] * per
        assert c["grid_walk"] >= 1 and (c["grid_walk"] - 1) * threads < c["nlines"] <= c["grid_walk"] * threads   # one lane per line
        assert c["grid_apply"] >= 1 and (c["grid_apply"] - 1) * threads < nx * ny <= c["grid_apply"] * threads    # one thread per pixel
        assert all(1 <= c[g] <= INT_MAX for g in ("grid_rows", "grid_walk", "grid_apply")) and nbands <= 65535    # (grid.y)
        assert c["carry_words"] == c["walk_dirs"] * nbands * c["nlines"]
        assert c["scratch_bytes"] == 4 * (dirs * nx * ny + 2 * c["carry_words"])


def test_bands_at_the_headline_size(lib):
    c = plan(lib, [(1920, 1080, 8, 256)])[0]
    assert c["nbands"] > 1 and c["band"] * c["band"] >= 1080


def test_refusals(lib):
    bad = [(0, 5), (5, 0), (-1, 5), (5, -1), (0, 0), (INT_MAX, 2), (2, INT_MAX), (46341, 46341), (65536, 32768), (INT_MAX, INT_MAX)]
    for (nx, ny), c in zip(bad, plan(lib, [(nx, ny, 8, 256) for nx, ny in bad])):
        assert c["family"] == REFUSE and c["scratch_bytes"] == 0 and c["grid_rows"] == 0 and c["grid_apply"] == 0, (nx, ny)
    ok = [(INT_MAX, 1), (1, INT_MAX), (46340, 46340), (65536, 32767)]   # the largest maps: at most 2^31 - 1 pixels
    assert all(c["family"] == LINES for c in plan(lib, [(nx, ny, 8, 256) for nx, ny in ok]))
    for dirs in (-1, 0, 1, 3, 5, 6, 7, 9, 16):                          # only the three direction sets exist
        assert plan(lib, [(40, 30, dirs, 256)])[0]["family"] == REFUSE


def test_a_choice_is_a_function_of_the_request_alone(lib):
    rows = [(nx, ny, dirs, cu) for nx, ny in SHAPES for dirs in DIRS for cu in (0, 1, 104, 256, 304)]
    first = plan(lib, rows)
    again = plan(lib, rows[::-1])[::-1]        # another order, other neighbours in the batch
    assert first == again
    one_by_one = [plan(lib, [r])[0] for r in rows]
    assert first == one_by_one
    rng = np.random.default_rng(5)
    rnd = [(int(rng.integers(1, 5000)), int(rng.integers(1, 5000)), int(rng.choice(DIRS)), int(rng.integers(0, 400))) for _ in range(300)]
    assert plan(lib, rnd) == plan(lib, list(rnd))


def test_chunk_and_band_depend_on_the_shape_alone(lib):
    """The GPU tests place their seams by the chunk and the band they read here, for dirs = 8: the other direction sets and device
    widths must not move them."""
    for nx, ny in SHAPES:
        cs = plan(lib, [(nx, ny, dirs, cu) for dirs in DIRS for cu in (0, 64, 256)])
        assert len({(c["chunk"], c["band"], c["nbands"]) for c in cs}) == 1
