"""The HIP kernels that read PIXELS -- census, prefilters, weights, zoom-out, every cost kernel -- and what runs downstream of
them, on the pixel domains of tests/pixel_domains.py: 16-bit and float-valued samples, denormals, signed zeros, flat regions,
NaN nodata and +-Inf.  Everything goes through the C ABI and is compared with the CPU oracle bit for bit (NaN == NaN); the
oracle itself is pinned on the compiled reference for the same domains by tests/test_pixel_domains_ref.py, and where the
compiled reference travelled (oracle/_ref) it is compared here too.

Each cost-volume case is DESIGNED for one kernel of launch_cost_fast / the general kernel and asserts from the timing table
that this kernel ran (the table lists the kernel launch_cost chose next to "k_cost"): a case that silently lands in the general
kernel does not test the fast one.  The last test of the file prints the table kernel x pixel class -> cases.

Every case that is not `degenerate_ok` satisfies the non-degeneracy condition (at most half of the pixels all-zero, at most
half of the cells +INF) on the oracle's volume before anything is compared.
"""
import collections
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
import multiscale_model as msm
import pixel_domains as pd
from helpers import labels_equal, ndiff
from oracle import oracle as orc_mod

pytestmark = pytest.mark.gpu

INF = float("inf")
F = np.float32
SEEN = collections.Counter()  # (kernel name, pixel class) -> cases that entered it
PRODUCED = collections.Counter()  # (cost kernel, pixel class) -> cases whose COMPARED volume that kernel wrote (the last fill)


class Trace:
    """The names of the timing table for the calls made inside the block."""

    def __init__(self, ctx, cls):
        self.ctx, self.cls, self.names = ctx, cls, []

    def __enter__(self):
        self.ctx.timing(True)
        self.ctx.timing_reset()
        return self

    def __exit__(self, *exc):
        self.names = [n for n, _ in self.ctx.timings()]
        self.ctx.timing(False)
        self.ctx.timing_reset()
        for n in set(self.names):
            SEEN[(n, self.cls)] += 1
        fills = [n for n in self.names if n.startswith("k_cost_")]
        self.final = fills[-1] if fills else None  # (a fill whose flag says "no compact form" is done again: the last one stays)


def condition_volume(ref, a, u, v, dmin, dmax, pre, dist, td, win):
    """The volume the non-degeneracy condition is asserted on: the compiled reference's where it travelled and can compute
    the case (it reads its window once per process), else the oracle's `a`."""
    if ref is not None and win == ref.census_win():
        return ref.costvolume(u, v, dmin, dmax, pre, dist, td)
    return a


def check_condition(C, cls, dist, tag):
    if pd.degenerate_ok(cls, pd.effective_distance(dist)):
        return
    zero, inf = pd.degeneracy(C)
    assert zero <= 0.5 and inf <= 0.5, ("degenerate volume", tag, zero, inf)


@pytest.fixture(scope="module")
def ref_or_none():
    return orc_mod.Reference() if orc_mod.Reference.available() else None


@pytest.fixture(scope="module")
def big_oracle():
    return orc_mod.Oracle(threads=orc_mod.usable_cpus(16))


def free(*hs):
    for h in hs:
        if h is not None:
            h.free()


# ---- a. primitives ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", pd.CLASSES)
def test_census_and_prefilters(ctx, oracle, ref_or_none, cls):
    """k_census and k_filter2d are not exported on their own: reached through the fp32 AD volume of the prefiltered images
    (census AD costs are the distances of the descriptor words read as floats).  Odd sizes, 1 and 3 channels; census windows
    3, 5 and 7 (one, one and two descriptor words per channel group)."""
    for nch, (ny, nx), vshape in ((1, (75, 91), None), (3, (61, 105), (59, 101))):  # (gblur spreads every NaN over 7x7 pixels)
        u, v = pd.pair(cls, 3100 + pd.CLASSES.index(cls) + nch, nch, ny, nx, vshape)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        for pre, win, kernel in (("census", 3, "k_census"), ("census", 5, "k_census"), ("census", 7, "k_census"),
                                 ("sobelx", 3, "k_filter2d"), ("gblur", 3, "k_filter2d")):
            dmin, dmax = -9, 6
            a = oracle.costvolume(u, v, dmin, dmax, pre, "ad", INF, win)
            check_condition(condition_volume(ref_or_none, a, u, v, dmin, dmax, pre, "ad", INF, win), cls, "ad", (cls, nch, pre, win))
            with Trace(ctx, cls) as t:
                cv = ctx.costvolume_dev(du, dv, dmin, dmax, pre, "ad", INF, win)
            assert kernel in t.names, (pre, t.names)
            assert ndiff(a, cv.download()) == 0, (cls, nch, pre, win)
            if ref_or_none is not None and win == ref_or_none.census_win():
                assert ndiff(ref_or_none.costvolume(u, v, dmin, dmax, pre, "ad", INF), cv.download()) == 0, (cls, nch, pre, "ref")
            cv.free()
        free(du, dv)


@pytest.mark.parametrize("cls", pd.CLASSES)
def test_weights(ctx, oracle, ref_or_none, cls):
    for nch, (ny, nx) in ((1, (37, 45)), (3, (29, 52))):
        u, _ = pd.pair(cls, 3200 + pd.CLASSES.index(cls) + nch, nch, ny, nx)
        du = ctx.upload_image(u)
        for aThresh in (5.0, 12.0, 1e30):
            for aP in (4.0, 0.3):
                with Trace(ctx, cls) as t:
                    w = ctx.weights_dev(du, aP, aThresh)
                assert "k_weights" in t.names
                got = w.download()
                assert ndiff(oracle.weights(u, aP, aThresh), got) == 0, (cls, nch, aP, aThresh)
                if ref_or_none is not None:
                    assert ndiff(ref_or_none.weights(u, aP, aThresh), got) == 0, (cls, nch, aP, aThresh, "ref")
                w.free()
        du.free()


@pytest.mark.parametrize("cls", pd.CLASSES)
def test_zoom_out(ctx, cls):
    for nch, (ny, nx) in ((1, (37, 45)), (3, (48, 64)), (1, (1, 7)), (2, (9, 1))):
        u, _ = pd.pair(cls, 3300 + pd.CLASSES.index(cls) + nch, nch, max(ny, 8), max(nx, 8))
        u = np.ascontiguousarray(u[:, :ny, :nx])
        du = ctx.upload_image(u)
        with Trace(ctx, cls) as t:
            z = ctx.zoom_out_dev(du)
        assert "k_zoom_out" in t.names
        with np.errstate(all="ignore"):
            want = msm.zoom_out(u)
        assert ndiff(z.download(), want) == 0, (cls, nch, ny, nx)
        free(du, z)


# ---- b. the cost-volume matrix ----------------------------------------------------------------------------------------------
# nx, ny, right image (vny, vnx) or the same size, dmin, label count.  Widths that are multiples of four and not; label counts with
# a compact form (64 .. 384), padded (151 -> 192 slots), a multiple of four without a compact form (152), beyond kNccMaxL; right
# images narrower and shorter than the left; every dmin lets the windows cross both borders of the right image.
SHAPES = {
    "A": (96, 40, None, -40, 64),
    "B": (149, 40, (37, 141), -70, 128),
    "C": (160, 24, None, -100, 192),
    "D": (201, 24, (24, 190), -130, 256),
    "E": (240, 16, None, -190, 384),
    "F": (150, 24, None, -80, 151),
    "G": (152, 40, (38, 152), -80, 152),
    "H": (48, 16, None, -515, 1030),
    "I": (256, 72, None, -100, 192),  # (for gblur, which spreads every NaN over 7x7 pixels: room for the nodata class)
    "J": (100, 8, None, -384, 768),   # (beyond 512 labels the compact form is one byte per cost whatever the channel count)
}
NAN = float("nan")
# (shape, prefilter, distance, window, channels, truncDist, the kernel the case is designed for)
PLAN = [
    ("A", "none", "ad", 3, 1, INF, "k_cost_diffx_1b"),
    ("B", "none", "ad", 3, 3, 20.0, "k_cost_diffx_2b"),
    ("D", "none", "ad", 3, 2, 2.5, "k_cost_diffx_2b_anych"),
    ("F", "none", "ad", 3, 1, INF, "k_cost_diffx_1b"),            # the padded layout: 151 labels in 192 slots
    ("C", "none", "sd", 3, 1, INF, "k_cost_diffx_2b"),
    ("E", "none", "sd", 3, 4, 20.0, "k_cost_diffx_2b_anych"),
    ("G", "none", "ad", 3, 3, 2.5, "k_cost_btx_diff_w4"),         # no compact form of 152 labels, a fractional truncDist: fp32
    ("A", "none", "census", 5, 1, INF, "k_cost_census8x_w4"),
    ("B", "none", "census", 3, 3, 20.0, "k_cost_census8x"),
    ("D", "none", "census", 5, 1, 2.5, "k_cost_general"),         # a fractional truncDist: no compact form
    ("F", "none", "census", 5, 1, INF, "k_cost_census8x"),        # padded
    ("E", "none", "census", 7, 1, INF, "k_cost_btx_census_w4"),   # two descriptor words: halves of bit counts
    ("B", "none", "census", 7, 1, INF, "k_cost_btx_census"),      # ... on a width that is not a multiple of four
    ("F", "none", "census", 7, 1, 20.0, "k_cost_general"),        # ... at a label count that is not a multiple of four
    ("J", "none", "ad", 3, 2, 20.0, "k_cost_diffx_1b_anych"),     # 768 labels, two channels: one byte per cost, any channel count
    ("A", "census", "ad", 3, 1, INF, "k_cost_btx_diff_w4"),
    ("B", "sobelx", "ad", 3, 1, 20.0, "k_cost_diffx_1b"),
    ("I", "gblur", "sd", 3, 3, INF, "k_cost_btx_diff_w4"),
    ("B", "gblur", "ad", 3, 1, 2.5, "k_cost_btx_diff"),
    ("A", "none", "ncc", 3, 1, INF, "k_cost_ncc"),
    ("B", "none", "ncc", 5, 3, 2.5, "k_cost_ncc"),
    ("G", "none", "ncc", 7, 4, 20.0, "k_cost_ncc"),
    ("H", "none", "ncc", 3, 1, 20.0, "k_cost_general"),           # beyond kNccMaxL
    ("B", "gblur", "ncc", 3, 1, INF, "k_cost_general"),           # NCC of prefiltered images
    ("A", "none", "btad", 3, 1, INF, "k_cost_btx_bt_w4"),
    ("D", "none", "btsd", 3, 3, 20.0, "k_cost_btx_bt"),
    ("G", "none", "btad", 3, 2, 2.5, "k_cost_btx_bt_w4"),
    ("F", "none", "btsd", 3, 1, INF, "k_cost_general"),           # a label count that is not a multiple of four
    ("A", "sobelx", "btsd", 3, 1, 20.0, "k_cost_general"),        # Birchfield-Tomasi on prefiltered images
    # a NaN truncDist: every comparison with it is false, so every cost IS truncDist (mgm_costvolume.h:401-412) and the pixel
    # rule then zeroes the volume -- the selection `c < t ? c : t` is not a minimum
    ("A", "none", "btad", 3, 1, NAN, "k_cost_btx_bt_w4"),
    ("A", "none", "ad", 3, 1, NAN, "k_cost_general"),
]
MATRIX = [(cls, k) for cls in pd.CLASSES for k in range(len(PLAN))]


def matrix_case(cls, k):
    shape, pre, dist, win, nch, td, kernel = PLAN[k]
    nx, ny, vshape, dmin, L = SHAPES[shape]
    u, v = pd.pair(cls, 7000 + 50 * k + pd.CLASSES.index(cls), nch, ny, nx, vshape)
    return u, v, dmin, dmin + L - 1, pre, dist, win, td, kernel


@pytest.mark.parametrize("cls,k", MATRIX, ids=lambda x: x if isinstance(x, str) else "%02d-%s" % (x, "-".join(str(p) for p in PLAN[x][:6])))
def test_costvolume_matrix(ctx, oracle, ref_or_none, cls, k):
    u, v, dmin, dmax, pre, dist, win, td, kernel = matrix_case(cls, k)
    tag = (cls,) + PLAN[k]
    a = oracle.costvolume(u, v, dmin, dmax, pre, dist, td, win)
    if td == td:
        check_condition(condition_volume(ref_or_none, a, u, v, dmin, dmax, pre, dist, td, win), cls, dist, tag)
    else:
        assert not a.any(), tag  # (the oracle agrees with the reading above)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    with Trace(ctx, cls) as t:
        cv = ctx.costvolume_dev(du, dv, dmin, dmax, pre, dist, td, win)
    got = cv.download()
    assert kernel in t.names, (tag, t.names)
    PRODUCED[(t.final, cls)] += 1
    assert ndiff(a, got) == 0, (tag, ndiff(a, got), t.names)
    if ref_or_none is not None and win == ref_or_none.census_win():
        assert ndiff(ref_or_none.costvolume(u, v, dmin, dmax, pre, dist, td), got) == 0, (tag, "ref")
    free(cv, du, dv)


# ---- c. downstream of the fill ----------------------------------------------------------------------------------------------
CONFIGS = [(8, 3, 0, 8.0, 32.0), (8, 4, 1, 2.0, 9.0), (4, 2, 0, 8.0, 32.0)]  # (NDIR, TSGM, FH, P1, P2)
# (nch, nx, ny, vshape, dmin, dmax, prefilter, distance, window): one-byte costs (grey AD, census), two-byte (colour AD), and
# whatever the class makes of them: 16-bit and float samples leave the compact forms (the refill in fp32 after the flag)
DOWN_VOLUMES = [(1, 96, 40, None, -40, 23, "none", "ad", 3), (3, 149, 32, (30, 141), -70, 57, "none", "ad", 3),
                (1, 100, 36, None, -40, 23, "none", "census", 5), (1, 90, 30, None, -30, 13, "none", "ncc", 3)]


def compare_aggregation(ctx, oracle, cv, C, dmin, cfg, w8=None, w8dev=None, tag=None):
    NDIR, MGM, FH, P1, P2 = cfg
    Sa, oa, ca = oracle.mgm(C, dmin, P1, P2, NDIR, MGM, FH, 1, w8)
    S, o, c = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, FH, 1, w8dev, None, want_S=True)
    assert ndiff(Sa, S.download()) == 0, (tag, "S")
    assert ndiff(ca, c.download()[0]) == 0, (tag, "costs")
    assert labels_equal(oa, o.download()[0], ca), (tag, "labels")
    fin = np.isfinite(ca)
    ra, rca = oracle.refine(Sa, dmin, "vfit", np.where(fin, oa, dmin), ca)
    _, fo, fc = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, FH, 1, w8dev, "vfit")
    assert ndiff(ra[fin], fo.download()[0][fin]) == 0 and ndiff(rca, fc.download()[0]) == 0, (tag, "vfit")
    free(S, o, c, fo, fc)


@pytest.mark.parametrize("vol", range(len(DOWN_VOLUMES)), ids=lambda i: "%dch-%s-L%d" % (DOWN_VOLUMES[i][0], DOWN_VOLUMES[i][7], DOWN_VOLUMES[i][5] - DOWN_VOLUMES[i][4] + 1))
@pytest.mark.parametrize("cls", ["u16", "unit", "nodata", "inf", "mixed", "flat"])
def test_aggregation_of_device_built_volumes(ctx, oracle, cls, vol):
    """S, costs, labels (where the cost is finite) and one refinement of the volume the device built, for three
    configurations; then the same volume UPLOADED, which makes the library derive its compact copy and NaN flag from the floats
    (k_compact / k_nanscan) instead of from the cost kernel."""
    nch, nx, ny, vshape, dmin, dmax, pre, dist, win = DOWN_VOLUMES[vol]
    u, v = pd.pair(cls, 8100 + 10 * vol + pd.CLASSES.index(cls), nch, ny, nx, vshape)
    C = oracle.costvolume(u, v, dmin, dmax, pre, dist, INF, win)
    check_condition(C, cls, dist, (cls, vol))
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    with Trace(ctx, cls):
        cv = ctx.costvolume_dev(du, dv, dmin, dmax, pre, dist, INF, win)
        for cfg in CONFIGS:
            compare_aggregation(ctx, oracle, cv, C, dmin, cfg, tag=(cls, vol, cfg))
    assert ndiff(C, cv.download()) == 0
    with Trace(ctx, cls):
        up = ctx.upload_volume(C, dmin)
        compare_aggregation(ctx, oracle, up, C, dmin, CONFIGS[1], tag=(cls, vol, "uploaded"))
    free(cv, up, du, dv)


def test_aggregation_of_an_uploaded_volume_without_compact_form(ctx, oracle):
    """44 labels: no compact copy, the NaN scan alone (k_nanscan) reads the floats the cost kernel wrote."""
    for cls in ("u16", "nodata", "inf"):
        u, v = pd.pair(cls, 8300 + pd.CLASSES.index(cls), 1, 30, 70)
        C = oracle.costvolume(u, v, -30, 13, "none", "ad", INF, 3)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        cv = ctx.costvolume_dev(du, dv, -30, 13, "none", "ad", INF, 3)
        got = cv.download()
        assert ndiff(C, got) == 0
        with Trace(ctx, cls) as t:
            up = ctx.upload_volume(got, -30)
            compare_aggregation(ctx, oracle, up, C, -30, CONFIGS[0], tag=(cls, "uploaded L44"))
        assert "k_nanscan" in t.names, t.names
        free(cv, up, du, dv)


def test_batch_of_four_classes_in_one_launch(ctx, oracle):
    """aggregate_batch_dev over four volumes of one geometry built from four pixel classes (so: different storage forms)."""
    nx, ny, dmin, dmax = 96, 40, -40, 23
    NDIR, MGM, FH, P1, P2 = CONFIGS[1]
    classes = ["u16", "nodata", "inf", "flat"]
    pairs = [pd.pair(cls, 8400 + i, 1, ny, nx) for i, cls in enumerate(classes)]
    imgs = [(ctx.upload_image(u), ctx.upload_image(v)) for u, v in pairs]
    cvs = [ctx.costvolume_dev(du, dv, dmin, dmax, "none", "ad", INF, 3) for du, dv in imgs]
    S, outs, outcs = ctx.aggregate_batch_dev(cvs, P1, P2, NDIR, MGM, FH, 1, None, None, want_S=True)
    for i, (cls, (u, v)) in enumerate(zip(classes, pairs)):
        C = oracle.costvolume(u, v, dmin, dmax, "none", "ad", INF, 3)
        Sa, oa, ca = oracle.mgm(C, dmin, P1, P2, NDIR, MGM, FH, 1)
        assert ndiff(C, cvs[i].download()) == 0, cls
        assert ndiff(Sa, S[i].download()) == 0, cls
        assert ndiff(ca, outcs[i].download()[0]) == 0 and labels_equal(oa, outs[i].download()[0], ca), cls
    free(*(S + outs + outcs + cvs + [h for p in imgs for h in p]))


@pytest.mark.parametrize("cfg", CONFIGS[:2], ids=["hirsch", "fh"])
def test_weights_from_a_nodata_image(ctx, oracle, cfg):
    """k_weights planes of an image with NaN pixels (every comparison with a NaN difference fails: weight 1) into the
    aggregation of that pair's volume."""
    nx, ny, dmin, dmax = 96, 40, -40, 23
    u, v = pd.pair("nodata", 8500, 3, ny, nx)
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    w8dev = ctx.weights_dev(du, 4.0 if not cfg[2] else 0.3, 12.0)
    w8 = oracle.weights(u, 4.0 if not cfg[2] else 0.3, 12.0)
    assert ndiff(w8, w8dev.download()) == 0 and np.any(w8 != 1.0)
    C = oracle.costvolume(u, v, dmin, dmax, "none", "ad", INF, 3)
    cv = ctx.costvolume_dev(du, dv, dmin, dmax, "none", "ad", INF, 3)
    compare_aggregation(ctx, oracle, cv, C, dmin, cfg, w8=w8, w8dev=w8dev, tag=("weights", cfg))
    free(cv, w8dev, du, dv)


# ---- d. ranged volumes ------------------------------------------------------------------------------------------------------
def windows_around(shift, ny, nx, half, hmin, hmax, seed):
    """Float range images of at most 2 * half + 1 labels around the pair's true disparity (a constant), jittered per pixel."""
    rng = np.random.default_rng(seed)
    j = rng.integers(-2, 3, size=(ny, nx))
    lo = np.clip(shift - half + 2 + j, hmin, hmax)
    hi = np.clip(shift + half - 2 + rng.integers(-2, 3, size=(ny, nx)), hmin, hmax)
    hi = np.maximum(hi, lo)
    lo[0, 0], hi[0, 0] = shift - half, shift + half  # the widest window is attained
    return lo.astype(F) + F(0.25) * (lo >= 0), hi.astype(F)


RANGED = [("u16", "census", 5), ("nodata", "census", 5), ("inf", "census", 5), ("u16", "ad", 3), ("unit", "ad", 3), ("nodata", "ad", 3),
          ("inf", "ad", 3)]


@pytest.mark.parametrize("half", [24, 50], ids=["w49", "w101"])
@pytest.mark.parametrize("cls,dist,win", RANGED, ids=lambda x: str(x))
def test_ranged_volumes(ctx, oracle, cls, dist, win, half):
    """costvolume_ranged_dev (census: the direct k_cost_census_rel fill; AD: the hull by the general kernel, then gathered -- one
    byte per cost with +INF codes for 8-bit nodata images, the fp32 cost itself for float images) and its aggregation through
    k_pass_rel, against the ragged oracle: the hull volume, S, costs, labels, vfit."""
    nx, ny, shift = 160, 48, 3
    u, v = pd.pair(cls, 8600 + pd.CLASSES.index(cls) + half, 1, ny, nx, None, shift)
    dminI, dmaxI = windows_around(shift, ny, nx, half, -60, 60, 77 + half)
    lo, hi = orc_mod.int_ranges(dminI, dmaxI)
    hmin, hmax = int(lo.min()), int(hi.max())
    assert int((hi - lo + 1).max()) == 2 * half + 1
    C = oracle.costvolume_ranged(u, v, lo, hi, hmin, hmax, "none", dist, INF, win)
    own = (np.arange(hmin, hmax + 1)[None, None, :] >= lo[..., None]) & (np.arange(hmin, hmax + 1)[None, None, :] <= hi[..., None])
    zero = float(np.mean(np.all((C == 0) | ~own, axis=2)))
    assert zero <= 0.5 and float(np.mean(np.isposinf(C[own]))) <= 0.5, (cls, dist, zero)
    du, dv, dl, dh = ctx.upload_image(u), ctx.upload_image(v), ctx.upload_image(dminI), ctx.upload_image(dmaxI)
    NDIR, MGM, FH, P1, P2 = 8, 3, 1, 2.0, 20000.0
    with Trace(ctx, cls) as t:
        cv = ctx.costvolume_ranged_dev(du, dv, dl, dh, hmin, hmax, "none", dist, INF, win)
        _, o, c = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, FH, 1, None, "vfit")
    assert ("k_cost_census_rel" if dist == "census" else "k_rel_gather") in t.names, t.names
    assert "k_pass_rel" in t.names, t.names
    assert ndiff(C, cv.download()) == 0, (cls, dist, half)
    Sa, oa, ca = oracle.mgm_ranged(C, hmin, lo, hi, P1, P2, NDIR, MGM, FH, 1)
    fin = np.isfinite(ca)
    ra, rca = oracle.refine_ranged(Sa, hmin, lo, hi, "vfit", np.where(fin, oa, lo).astype(F), ca)
    assert ndiff(rca, c.download()[0]) == 0 and ndiff(ra[fin], o.download()[0][fin]) == 0, (cls, dist, half)
    S, o2, c2 = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, FH, 1, None, None, want_S=True)
    # (S exists inside each pixel's own range only: the reference's Dvec holds nothing else, as in test_gpu_ragged_oracle)
    assert ndiff(np.where(own, Sa, 0), np.where(own, S.download(), 0)) == 0, (cls, dist, half)
    assert ndiff(ca, c2.download()[0]) == 0 and labels_equal(oa, o2.download()[0], ca), (cls, dist, half)
    free(cv, o, c, S, o2, c2, du, dv, dl, dh)


# ---- e. multiscale ----------------------------------------------------------------------------------------------------------
def test_multiscale_pair_with_nodata(ctx, big_oracle):
    """NaN pixels come down the pyramid exactly as the model's fp32 arithmetic says: the 256x192 crop of the fountain pair with a
    nodata border on two sides and a hole in each image, three scales, census 5x5."""
    from test_gpu_multiscale import BASE, compare, run_device
    from helpers import GOLDEN
    d = np.load(os.path.join(GOLDEN, "cfg1_fountain23.npz"))
    u = np.ascontiguousarray(d["uL"].astype(F).transpose(2, 0, 1)[:, 150:342, 300:556])
    v = np.ascontiguousarray(d["uR"].astype(F).transpose(2, 0, 1)[:, 150:342, 300:556])
    rng = np.random.default_rng(91)
    u[:, pd.nodata_mask(rng, 192, 256, 0)] = np.nan
    v[:, pd.nodata_mask(rng, 192, 256, 1)] = np.nan
    u[:, 60:83, 100:131] = np.nan  # a hole that survives two halvings
    want = msm.multiscale_pair(big_oracle, u, v, -120, 30, 3, **BASE)
    with Trace(ctx, "nodata"):
        got = run_device(ctx, u, v, -120, 30, 3, **BASE)
    compare(got, want, "nodata crop S=3")
    assert len(got["levels"]) == 3 and np.isfinite(want["outL"]).mean() > 0.2


# ---- f. command line --------------------------------------------------------------------------------------------------------
CLI_LINES = [
    ("census vfit", 1, "-r -20 -R 12 -t census -s vfit -O 8", dict(TSGM="3", CENSUS_NCC_WIN="5")),
    ("ad weights", 3, "-r -20 -R 12 -t ad -O 8 -aP2 4 -aThresh 12", dict(TSGM="3")),
    ("ncc window 5", 1, "-r -12 -R 10 -t ncc -O 4", dict(TSGM="2", CENSUS_NCC_WIN="5")),
    ("btad", 3, "-r -12 -R 9 -t btad -O 8", dict(TSGM="3")),
    ("sobelx sd truncDist", 1, "-r -12 -R 9 -p sobelx -t sd -truncDist 300 -O 4 -s cubic", dict(TSGM="2")),
    ("range images", 1, "-r -16 -R 8 -t census -s vfit -O 8 -m {ranges}/lo.npy -M {ranges}/hi.npy",
     dict(TSGM="3", CENSUS_NCC_WIN="5", USE_TRUNCATED_LINEAR_POTENTIALS="1")),
]
CLI_CLASSES = ["u16", "unit", "nodata", "mixed"]


def save_pair(tmp_path, u, v):
    nch = u.shape[0]
    np.save(tmp_path / "u.npy", np.ascontiguousarray(u.transpose(1, 2, 0)) if nch > 1 else u[0])
    np.save(tmp_path / "v.npy", np.ascontiguousarray(v.transpose(1, 2, 0)) if nch > 1 else v[0])


@pytest.mark.parametrize("cls", CLI_CLASSES)
@pytest.mark.parametrize("line", CLI_LINES, ids=lambda c: c[0].replace(" ", "-"))
def test_cli_on_float_npy_pairs(line, cls, tmp_path):
    """mgm_amd/bin/mgm and the reference's own program on float32 .npy pairs of the non-8-bit classes: stdout and every output
    file, with the comparison rules of test_gpu_cli.compare_outputs (the reference's uninitialised label where no cost is finite).
    Both programs replace non-finite samples by 0 as they read the images (mgm.cc:335-336): through the command line a nodata
    pixel reaches the kernels as a zero next to 16-bit values, not as a NaN."""
    from test_gpu_cli import OURS, REF, compare_outputs
    if not os.path.exists(REF):
        pytest.skip("reference CLI (oracle/_ref/mgm) was not built")
    name, nch, args, env = line
    nx, ny = 112, 72
    u, v = pd.pair(cls, 8700 + CLI_LINES.index(line) * 10 + CLI_CLASSES.index(cls), nch, ny, nx, None, 3)
    save_pair(tmp_path, u, v)
    if "{ranges}" in args:
        rng = np.random.default_rng(18)
        lo = (3 - rng.integers(1, 9, size=(ny, nx))).astype(F) + rng.random((ny, nx)).astype(F) * F(0.5)
        hi = np.floor(lo) + rng.integers(1, 14, size=(ny, nx)).astype(F)
        np.save(tmp_path / "lo.npy", lo.astype(F))
        np.save(tmp_path / "hi.npy", hi.astype(F))
    outs = {}
    for tag, exe in (("ref", REF), ("ours", OURS)):
        d = tmp_path / tag
        d.mkdir()
        cmd = [exe] + args.format(ranges=tmp_path).split() + [str(tmp_path / "u.npy"), str(tmp_path / "v.npy"), str(d / "disp.npy"),
                                                               str(d / "cost.npy"), str(d / "back.npy")]
        e = dict(os.environ, **dict(dict(OMP_NUM_THREADS="4"), **env))
        r = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (tag, r.stderr)
        outs[tag] = (r.stdout, {f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert np.isfinite(outs["ref"][1]["cost.npy"]).mean() > 0.5, (name, cls)
    compare_outputs(outs, nx, ny, nch, (name, cls))


def test_cli_three_scales_on_a_mixed_npy_pair(big_oracle, tmp_path):
    from test_gpu_multiscale import CLI_ARGS, CLI_ENV, CLI_KW, expected_stdout
    from test_gpu_cli import OURS
    nx, ny = 256, 192
    u, v = pd.pair("mixed", 8800, 3, ny, nx, None, -20)
    save_pair(tmp_path, u, v)
    f = lambda n: str(tmp_path / n)
    cmd = [OURS] + CLI_ARGS.split() + ["-S", "3", "-l", f("nolr.npy"), f("u.npy"), f("v.npy"), f("disp.npy"), f("cost.npy")]
    r = subprocess.run(cmd, env=dict(os.environ, **CLI_ENV), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    # main() replaces non-finite samples by 0 before anything else (mgm.cc:335-336)
    want = msm.multiscale_pair(big_oracle, np.where(np.isfinite(u), u, F(0)), np.where(np.isfinite(v), v, F(0)), -120, 30, 3, **CLI_KW)
    assert r.stdout == expected_stdout(3)
    for name, key in (("disp.npy", "outL"), ("cost.npy", "costL"), ("nolr.npy", "nolr")):
        assert ndiff(np.load(f(name)).reshape(ny, nx), want[key]) == 0, name


# ---- g. at size -------------------------------------------------------------------------------------------------------------
def at_size(ctx, big_oracle, u, v, dmin, dmax, dist, win, cfg, cls, expect):
    NDIR, MGM, FH, P1, P2 = cfg
    du, dv = ctx.upload_image(u), ctx.upload_image(v)
    with Trace(ctx, cls) as t:
        cv = ctx.costvolume_dev(du, dv, dmin, dmax, "none", dist, INF, win)
        S, o, c = ctx.aggregate_dev(cv, P1, P2, NDIR, MGM, FH, 1, None, None, want_S=True)
    assert expect in t.names, t.names
    C = big_oracle.costvolume(u, v, dmin, dmax, "none", dist, INF, win)
    check_condition(C, cls, dist, ("at size", cls))
    assert ndiff(C, cv.download()) == 0, "cost volume"
    Sa, oa, ca = big_oracle.mgm(C, dmin, P1, P2, NDIR, MGM, FH, 1)
    del C
    assert ndiff(Sa, S.download()) == 0, "S"
    del Sa
    assert ndiff(ca, c.download()[0]) == 0 and labels_equal(oa, o.download()[0], ca), "costs / labels"
    free(S, o, c, cv, du, dv)


def test_at_size_headline_shape_with_nodata_frame_and_holes(big_oracle):
    """1920x1080, 256 labels, census 5x5, 8 directions TSGM 3 FH: a 40-pixel nodata frame and holes a few hundred pixels wide --
    all-zero pixels at block and band boundaries of the cost, pass and winner kernels."""
    from mgm_amd import synth
    nx, ny, dmin, dmax = 1920, 1080, -255, 0
    u, v, _ = synth.stereo_pair(nx, ny, dmin * 3 // 4, 0, seed=9100)
    rng = np.random.default_rng(9100)
    for a in (u, v):
        a[:, :40], a[:, -40:], a[:, :, :40], a[:, :, -40:] = np.nan, np.nan, np.nan, np.nan
        for _ in range(3):
            hy, hx = int(rng.integers(100, 300)), int(rng.integers(200, 400))
            y0, x0 = int(rng.integers(40, ny - hy - 40)), int(rng.integers(40, nx - hx - 40))
            a[:, y0:y0 + hy, x0:x0 + hx] = np.nan
    with mgm_amd.Context(0) as c:
        at_size(c, big_oracle, u, v, dmin, dmax, "census", 5, (8, 3, 1, 2.0, 20000.0), "nodata", "k_cost_census8x_w4")


def test_at_size_three_channel_u16_ad(big_oracle):
    """1920x1080x3 16-bit samples, AD at 128 labels: the costs overflow two bytes, the fp32 volume is used."""
    nx, ny, dmin, dmax = 1920, 1080, -100, 27
    u, v = pd.pair("u16", 9200, 3, ny, nx, None, -40)
    with mgm_amd.Context(0) as c:
        at_size(c, big_oracle, u, v, dmin, dmax, "ad", 3, (8, 3, 0, 8.0, 32.0), "u16", "k_cost_btx_diff_w4")


# ---- the table --------------------------------------------------------------------------------------------------------------
# every kernel that reads pixels, or what those kernels wrote, must have been entered with these classes
# every cost kernel plan_cost_kernel can choose for an image of fewer than 2^31 - 1 pixels (only k_cost_census8 cannot be
# reached: it takes single-word census volumes of 2^31 - 1 pixels and more, every smaller one goes to k_cost_census8x)
COST_KERNELS = ["k_cost_diffx_1b", "k_cost_diffx_1b_anych", "k_cost_diffx_2b", "k_cost_diffx_2b_anych", "k_cost_btx_diff",
                "k_cost_btx_diff_w4", "k_cost_btx_census", "k_cost_btx_census_w4", "k_cost_btx_bt", "k_cost_btx_bt_w4", "k_cost_ncc",
                "k_cost_census8x", "k_cost_census8x_w4", "k_cost_general"]
# ... and the other kernels that read pixels, or what those kernels wrote
MUST_SEE = COST_KERNELS + ["k_census", "k_filter2d", "k_weights", "k_zoom_out", "k_cost_census_rel", "k_rel_gather", "k_pass_rel",
                           "k_compact", "k_nanscan", "k_wta"]


def test_plan_is_designed_for_every_reachable_cost_kernel():
    """The coverage requirement without any state: every cost kernel is the DESIGNED kernel of some row of PLAN, every row runs
    with every pixel class (MATRIX), and test_costvolume_matrix asserts per case that the designed kernel ran."""
    designed = {row[6] for row in PLAN}
    assert designed == set(COST_KERNELS), (designed ^ set(COST_KERNELS))
    assert {cls for cls, _ in MATRIX} == set(pd.CLASSES) and len(MATRIX) == len(pd.CLASSES) * len(PLAN)
    assert {SHAPES[row[0]][0] % 4 == 0 for row in PLAN} == {True, False}  # widths that are multiples of four and not


def test_dispatch_coverage_table(request):
    """A report (it runs last, collection order): kernel x pixel class -> cases that ENTERED the kernel / cases whose compared
    volume the kernel PRODUCED (cost kernels of the matrix only).  The two differ where a compact fill raised its "does not
    fit" flag and the volume was filled again in fp32 (16-bit, float, signed, huge samples on the k_cost_diffx rows: those pin the
    flag decision and the refill, the 8-bit based classes -- u8, negzero, flat, nodata, inf -- pin the compact arithmetic)."""
    kernels = sorted({k for k, _ in SEEN})
    print("\n%-24s" % "kernel" + "".join("%11s" % c for c in pd.CLASSES))
    for k in kernels:
        cell = lambda c: ("%d/%d" % (SEEN[(k, c)], PRODUCED[(k, c)])) if k in COST_KERNELS else "%d" % SEEN[(k, c)]
        print("%-24s" % k + "".join("%11s" % cell(c) for c in pd.CLASSES))
    if not request.config.getoption("keyword") and not any("::" in a for a in request.config.args):  # (the whole file ran)
        missing = [(k, c) for k in MUST_SEE for c in ("u16", "nodata", "inf") if not SEEN[(k, c)]]
        assert not missing, missing
        # every cost kernel PRODUCED a compared volume for the nodata and inf classes (8-bit based: the compact forms hold)
        idle = [(k, c) for k in COST_KERNELS for c in ("nodata", "inf") if not PRODUCED[(k, c)]]
        assert not idle, idle
