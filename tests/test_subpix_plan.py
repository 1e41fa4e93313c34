"""plan_subpix (mgm_amd/csrc/mgm_planner.h) on the host: a choice is a function of the request alone, the workgroups cover every
(pixel, label) exactly once, the costs of a workgroup index in 32 bits, the fp32 spans start 16-byte aligned, and bad requests are
refused."""
import numpy as np
import pytest

from subpix_model import plan, plan_lib

REFUSE, CODES, FLOATS = 0, 1, 2
INT_MAX = 2 ** 31 - 1
NPIX = [1, 3, 4, 5, 15, 64, 201, 390, 1920 * 1080, 2 ** 31 - 1, 2 ** 32]


def padded(L):
    return next(lp for lp in (64, 128, 192, 256, 384, 512, 768, 1024) if lp >= L)


def codes_row(npix, L, s, cu=256):
    lab = s * (L - 1) + 1
    return (npix, lab, padded(lab), padded(L), s, 1, cu)


def floats_row(npix, L, s, cu=256):
    lab = s * (L - 1) + 1
    return (npix, lab, lab, L, s, 4, cu)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = plan_lib(tmp_path_factory.mktemp("subpixplan"))
    assert lib.subpix_request_bytes() == 8 + 6 * 4 and lib.subpix_choice_bytes() == 8 + 4 * 4
    assert lib.subpix_max_labels() == 1 << 22
    return lib


def test_the_grid_covers_every_pixel_and_label_once(lib):
    threads, span = lib.subpix_threads(), lib.subpix_span_bytes()
    assert threads == 256 and span % (16 * threads) == 0
    rows = [codes_row(n, L, s) for n in NPIX for L in (1, 2, 3, 33, 64, 65, 129, 256) for s in (2, 4)]
    rows += [floats_row(n, L, s) for n in NPIX for L in (1, 2, 3, 33, 64, 65, 257, 1000, 5000) for s in (2, 4)]
    for q, c in zip(rows, plan(lib, rows)):
        npix, lab, slots, in_slots, s, cb, _ = q
        assert c["family"] == (CODES if cb == 1 else FLOATS), q
        pix, grid, vec = c["pix"], c["grid"], c["vec"]
        assert vec * cb == 16                                              # every chunk is one 16-byte store
        assert pix >= 1 and 1 <= grid <= INT_MAX
        assert (grid - 1) * pix < npix <= grid * pix                       # no empty workgroup, no pixel outside one
        assert pix * slots * cb >= span                                    # a full workgroup writes at least the span
        assert pix * slots < 2 ** 31                                       # the costs of a workgroup index in 32 bits
        assert c["chunks"] == -(-pix * slots // vec)
        if cb == 1:
            assert slots % vec == 0                                        # whole chunks per row: a chunk never leaves its pixel
            assert (slots - 1) // s < in_slots                             # the last chunk's loads stay inside the phase's row
        else:
            assert pix % 4 == 0                                            # workgroup b starts at float b * pix * labels: 16-byte aligned
            assert (lab - 1) // s == in_slots - 1                          # the last label is phase 0's last


def test_one_label(lib):
    """L' = 1 (dmin = dmax): one label per pixel, only phase 0 contributes."""
    for npix in NPIX:
        c = plan(lib, [floats_row(npix, 1, 4)])[0]
        assert c["family"] == FLOATS and c["pix"] == 4096 and c["grid"] == -(-npix // 4096)
        c = plan(lib, [codes_row(npix, 1, 2)])[0]
        assert c["family"] == CODES and c["pix"] == 256 and c["grid"] == -(-npix // 256)   # 64 slots per pixel, all but one padding


def test_the_largest_label_count(lib):
    """mgm_cv_create admits 2^22 labels: L' = s * (L - 1) + 1 just below it is planned, one label more is refused."""
    big = {2: (1 << 21), 4: (1 << 20)}                                      # the largest L with s * (L - 1) + 1 <= 2^22
    for s, L in big.items():
        lab = s * (L - 1) + 1
        assert lab <= 1 << 22 < s * L + 1
        c = plan(lib, [floats_row(7, L, s)])[0]
        assert c["family"] == FLOATS and c["pix"] == 4 and c["grid"] == 2 and c["pix"] * lab < 2 ** 31
        assert plan(lib, [floats_row(7, L + 1, s)])[0]["family"] == REFUSE
    c = plan(lib, [(5, (1 << 22) - 3, 1 << 22, 1 << 20, 4, 1, 0)])[0]          # codes at that size: one pixel per workgroup
    assert c["family"] == CODES and c["pix"] == 1 and c["grid"] == 5


def test_refusals(lib):
    ok = floats_row(100, 33, 2)
    assert plan(lib, [ok])[0]["family"] == FLOATS
    bad = [
        (0, 65, 65, 33, 2, 4, 0), (-1, 65, 65, 33, 2, 4, 0),               # no pixels
        (100, 0, 0, 1, 2, 4, 0), (100, -3, -3, 1, 2, 4, 0),                # no labels
        (100, 65, 65, 33, 1, 4, 0), (100, 65, 65, 33, 3, 4, 0), (100, 65, 65, 17, 8, 4, 0),   # s outside {2, 4}
        (100, 66, 66, 33, 2, 4, 0), (100, 67, 67, 17, 4, 4, 0),            # labels that are not s * (L - 1) + 1
        (100, 65, 65, 33, 2, 2, 0), (100, 65, 65, 33, 2, 0, 0),            # a form that is neither codes nor fp32
        (100, 65, 66, 33, 2, 4, 0), (100, 65, 65, 34, 2, 4, 0),            # fp32 rows are exactly the labels
        (100, 65, 65, 64, 2, 1, 0), (100, 65, 100, 64, 2, 1, 0),           # code rows are multiples of 64 ...
        (100, 65, 128, 33, 2, 1, 0), (100, 129, 192, 0, 2, 1, 0),          # ... of both volumes, and hold the labels
        (100, 129, 64, 128, 2, 1, 0),
        (2 ** 31 * 4096, 1, 1, 1, 2, 4, 0),                                # more workgroups than a grid has
    ]
    for q, c in zip(bad, plan(lib, bad)):
        assert c == dict(family=REFUSE, grid=0, pix=0, vec=0, chunks=0), q


def test_a_choice_is_a_function_of_the_request_alone(lib):
    rows = [f(n, L, s, cu) for n in NPIX for L in (1, 2, 33, 64, 65, 256) for s in (2, 4) for cu in (0, 104, 256) for f in (codes_row, floats_row)]
    first = plan(lib, rows)
    assert first == plan(lib, rows[::-1])[::-1]
    assert first == [plan(lib, [r])[0] for r in rows]
    rng = np.random.default_rng(11)
    rnd = [floats_row(int(rng.integers(1, 10 ** 7)), int(rng.integers(1, 3000)), int(rng.choice((2, 4))), int(rng.integers(0, 400))) for _ in range(300)]
    assert plan(lib, rnd) == plan(lib, list(rnd))
    # the device's width does not move a choice today
    for n in NPIX:
        assert len({tuple(c.values()) for c in plan(lib, [codes_row(n, 256, 2, cu) for cu in (0, 64, 256, 304)])}) == 1
