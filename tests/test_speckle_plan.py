"""plan_speckle (mgm_amd/csrc/mgm_planner.h) on the host: a choice is a function of the request alone, the tiles cover the image
exactly, every grid is at least one workgroup and large enough for its work, bad requests are refused, and the scratch is the
planes the kernels index."""
import numpy as np
import pytest

from speckle_model import plan, plan_lib

REFUSE, TILES = 0, 1
INT_MAX = 2 ** 31 - 1
SHAPES = [(1, 1), (1, 9), (7, 1), (3, 4), (63, 15), (64, 16), (65, 17), (129, 33), (200, 200), (1920, 1080), (4096, 4096),
          (INT_MAX, 1), (1, INT_MAX), (46340, 46340), (65536, 32767)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = plan_lib(tmp_path_factory.mktemp("speckleplan"))
    assert lib.speckle_request_bytes() == 3 * 4 and lib.speckle_choice_bytes() == 5 * 8 + 6 * 4
    return lib


def test_tiles_cover_the_image_exactly_and_the_grids_hold_the_work(lib):
    threads = lib.speckle_threads()
    for (nx, ny), c in zip(SHAPES, plan(lib, [(nx, ny, 256) for nx, ny in SHAPES])):
        assert c["family"] == TILES, (nx, ny)
        tw, th, ntx, nty = c["tw"], c["th"], c["ntx"], c["nty"]
        assert tw >= 1 and th >= 1 and (tw * th) % threads == 0      # whole pixels per thread of k_speckle_local
        assert (ntx - 1) * tw < nx <= ntx * tw and (nty - 1) * th < ny <= nty * th  # no empty tile, no pixel outside one
        assert c["grid_local"] == ntx * nty
        pairs = (ntx - 1) * ny + (nty - 1) * nx                      # one thread per pixel pair across a seam
        assert c["grid_seams"] >= 1 and (c["grid_seams"] - 1) * threads < max(pairs, 1) <= c["grid_seams"] * threads
        for g in ("grid_count", "grid_apply"):                       # one thread per pixel
            assert c[g] >= 1 and (c[g] - 1) * threads < nx * ny <= c[g] * threads
        assert all(1 <= c[g] <= INT_MAX for g in ("grid_local", "grid_seams", "grid_count", "grid_apply"))
        assert c["planes"] in (2, 3) and c["scratch_bytes"] == c["planes"] * nx * ny * 4


def test_refusals(lib):
    bad = [(0, 5), (5, 0), (-1, 5), (5, -1), (0, 0), (INT_MAX, 2), (2, INT_MAX), (46341, 46341), (65536, 32768), (INT_MAX, INT_MAX)]
    for (nx, ny), c in zip(bad, plan(lib, [(nx, ny, 256) for nx, ny in bad])):
        assert c["family"] == REFUSE and c["scratch_bytes"] == 0 and c["grid_local"] == 0, (nx, ny)
    ok = [(INT_MAX, 1), (1, INT_MAX), (46340, 46340), (65536, 32767)]   # the largest maps: at most 2^31 - 1 pixels
    assert all(c["family"] == TILES for c in plan(lib, [(nx, ny, 256) for nx, ny in ok]))


def test_a_choice_is_a_function_of_the_request_alone(lib):
    rows = [(nx, ny, cu) for nx, ny in SHAPES for cu in (0, 1, 104, 256, 304)]
    first = plan(lib, rows)
    again = plan(lib, rows[::-1])[::-1]        # another order, other neighbours in the batch
    assert first == again
    one_by_one = [plan(lib, [r])[0] for r in rows]
    assert first == one_by_one
    rng = np.random.default_rng(5)
    rnd = [(int(rng.integers(1, 5000)), int(rng.integers(1, 5000)), int(rng.integers(0, 400))) for _ in range(300)]
    assert plan(lib, rnd) == plan(lib, list(rnd))


def test_the_tile_is_one_shape_today(lib):
    """The GPU tests place their seams by the tile they read here; the kernels have one instance, which the launcher checks."""
    tiles = {(c["tw"], c["th"]) for c in plan(lib, [(nx, ny, cu) for nx, ny in SHAPES for cu in (0, 64, 256)])}
    assert len(tiles) == 1
