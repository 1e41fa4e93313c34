"""The kernel the host plans for a filling is the kernel the device ran: for every case below the volume is built with timing
on, the names the timing table lists next to "k_cost" -- one per attempt, in order -- are the names plan_cost_kernel
(mgm_fillplan.h, through tests/cost_kernel_harness.cc) gives for the attempts of the same request's walk, and the downloaded
volume is the oracle's bit for bit.

The shapes are the smallest at which a launch can go wrong: left images 5 (one partial group of four pixels), 44 and 45 wide (the
_w4 instances and the guarded ones), 1 and 3 rows, and a right image of 37 against 45.  The pairs hold whole numbers below 100
(8-bit images; no sum of squared differences leaves two bytes), so which attempts a walk makes follows from the request: a
truncation that is no whole number after its scaling by the channels leaves no compact form (the flag word of the first attempt is
not 0 and not 1: the fp32 fill follows), and one planted difference of 255 asks for two bytes (a flag word of exactly 1)."""
import math

import numpy as np
import pytest

import test_fillplan as tf
from helpers import ndiff
from test_cost_kernel_plan import build_harness, walks

pytestmark = pytest.mark.gpu

INF = float("inf")
W5, W44, W45, W45N = (5, 3, 5), (44, 1, 44), (45, 3, 45), (45, 1, 37)  # (nx, ny, vnx)
W44H, W5L = (44, 3, 44), (5, 1, 5)

# (distance, census / NCC window, channels, labels, truncDist, shape)
CASES = [
    ("ad", 3, 1, 64, INF, W44), ("ad", 3, 2, 64, 20.0, W45), ("ad", 3, 3, 64, 2.5, W5),
    ("sd", 3, 1, 64, 2.5, W45N), ("sd", 3, 2, 64, INF, W5L), ("sd", 3, 3, 64, 20.0, W44H),
    ("ad", 3, 1, 151, 20.0, W45N), ("ad", 3, 2, 151, 2.5, W44H), ("ad", 3, 3, 151, INF, W5),
    ("sd", 3, 1, 151, INF, W5L), ("sd", 3, 2, 151, 20.0, W44), ("sd", 3, 3, 151, 2.5, W45),
    ("ad", 3, 1, 152, 2.5, W44H), ("ad", 3, 2, 152, INF, W5), ("ad", 3, 3, 152, 2.5, W45N),
    ("sd", 3, 1, 152, 2.5, W5L), ("sd", 3, 2, 152, 20.0, W45), ("sd", 3, 3, 152, INF, W44),
    ("census", 3, 1, 64, INF, W44H), ("census", 5, 1, 64, 20.0, W45N), ("census", 5, 1, 151, INF, W5), ("census", 3, 1, 64, 2.5, W44),
    ("census", 7, 1, 64, INF, W44), ("census", 7, 1, 64, 20.0, W45),
    ("ncc", 3, 1, 64, INF, W45N), ("ncc", 3, 4, 64, 20.0, W5), ("ncc", 5, 1, 64, 2.5, W44H), ("ncc", 5, 4, 64, INF, W45),
    ("ncc", 7, 1, 64, 20.0, W5L), ("ncc", 7, 4, 64, 2.5, W44), ("ncc", 9, 1, 64, INF, W45),
    ("btad", 3, 1, 64, INF, W44H), ("btsd", 3, 3, 64, 20.0, W45N), ("btad", 3, 2, 150, 2.5, W5), ("btsd", 3, 1, 150, INF, W44),
    ("ad", 3, 2, 768, 20.0, W5),
]
ids = lambda c: "%s-w%d-%dch-%dl-%s-%dx%d-%d" % (c[:5] + c[5]) if isinstance(c, tuple) else str(c)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("costchoice"))


def pair(nch, shape, seed):
    nx, ny, vnx = shape
    rng = np.random.default_rng(seed)
    return rng.integers(0, 100, (nch, ny, nx)).astype(np.float32), rng.integers(0, 100, (nch, ny, vnx)).astype(np.float32)


def planned_names(lib, u, v, dist, win, L, td, script):
    """The kernel of each attempt of the walk the request makes under `script` (no filling before it, every switch on)."""
    q = tf.request(nx=u.shape[2], ny=u.shape[1], vnx=v.shape[2], vny=v.shape[1], nch=u.shape[0], L=L, dist=tf.DIST.index(dist), win=win, trunc=td)
    natt, att, names = walks(lib, [[q[f] for f in tf.FIELDS]], [td], script)
    assert natt[0] >= 1 and not np.any(att[0, :natt[0], 0] == tf.REL)
    return [n.decode() for n in names[0, :natt[0]]]


def check(ctx, oracle, lib, u, v, dist, win, L, td, script, tag):
    dmin = -(L // 2)
    want = planned_names(lib, u, v, dist, win, L, td, script)
    a = oracle.costvolume(u, v, dmin, dmin + L - 1, "none", dist, td, win)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        cv = ctx.costvolume_dev(du, dv, dmin, dmin + L - 1, "none", dist, td, win)
        ran = [n for n, _ in ctx.timings() if n.startswith("k_cost_")]
    finally:
        ctx.timing(False)
        ctx.timing_reset()
    got = cv.download()
    for h in (cv, du, dv):
        h.free()
    print(tag, ran)
    assert ran == want, (tag, ran, want)
    assert ndiff(a, got) == 0, (tag, ndiff(a, got), ran)
    return ran


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_the_planned_kernel_ran(ctx, oracle, lib, case):
    dist, win, nch, L, td, shape = case
    u, v = pair(nch, shape, 8800 + CASES.index(case))
    # differences under a truncation that is no whole number (after its scaling by the channels): the compact attempt misfits
    fits = dist not in ("ad", "sd") or td == INF or float(np.float32(td) * np.float32(nch)).is_integer()
    ran = check(ctx, oracle, lib, u, v, dist, win, L, td, [0] if fits else [9], case)
    assert len(ran) == (1 if fits else 2), (case, ran)


def test_a_difference_of_255_walks_from_one_byte_to_two(ctx, oracle, lib):
    u, v = pair(1, W44H, 8899)
    u[0, 1, 20], v[0, 1, 15] = 255.0, 0.0  # (disparity -5: inside the labels)
    assert check(ctx, oracle, lib, u, v, "ad", 3, 64, INF, [1, 0], "grey AD, 255") == ["k_cost_diffx_1b", "k_cost_diffx_2b"]


def test_the_cases_reach_every_family_the_tests_can(lib):
    """(host only) The walks of the cases above plan every kernel name but k_cost_census8's, which needs 2^31 - 1 pixels."""
    seen = set()
    for dist, win, nch, L, td, shape in CASES:
        u, v = pair(nch, shape, 0)
        fits = dist not in ("ad", "sd") or td == INF or math.isinf(td) or float(np.float32(td) * np.float32(nch)).is_integer()
        seen |= set(planned_names(lib, u, v, dist, win, L, td, [0] if fits else [9]))
    assert seen == {"k_cost_diffx_1b", "k_cost_diffx_1b_anych", "k_cost_diffx_2b", "k_cost_diffx_2b_anych", "k_cost_btx_diff", "k_cost_btx_diff_w4",
                    "k_cost_btx_census", "k_cost_btx_census_w4", "k_cost_btx_bt", "k_cost_btx_bt_w4", "k_cost_ncc", "k_cost_census8x", "k_cost_census8x_w4",
                    "k_cost_general"}, seen
