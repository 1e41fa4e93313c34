"""The four restatements of oracle/post.py -- median, left-right check, range update, back-projection -- against the compiled
reference on every map class x shape of tests/post_domains.py (CPU only; skipped where oracle/_ref was not built).  Bit for
bit, NaN == NaN.  This is what makes them a sound yardstick for the GPU tests of the same maps (tests/test_gpu_post_edges.py).

Before anything is compared, every class that is not `trivial` must satisfy, on the REFERENCE's own result, the condition that
keeps a case from passing by being empty:

  median        changes at least a quarter of the pixels (at every radius of the sweep)
  left-right    keeps at least a quarter and drops at least a quarter (at tau = 1 against an `other` of the map's own size)
  range update  rewrites at least half of the pixels (at every (slack, radius))
  back-project  takes at least a quarter of its pixels from each image

EXEMPT lists by name the cases of which that cannot be asked; post_domains.SEEDS holds the seeds at which the reference alone meets the
conditions (found by running `python tests/test_post_ref.py` -- the search looks at the reference's results only).

One class is not compared bit for bit: the MEDIAN of `signedzero`, where the reference returns whichever zero nth_element leaves
at v[n/2] -- compared with the zero signs masked.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import pixel_domains as pxd  # noqa: E402
import post_domains as pd  # noqa: E402
from helpers import ndiff  # noqa: E402
from oracle import oracle as orc_mod  # noqa: E402
from oracle import post  # noqa: E402

# Cases of which a condition cannot be asked, by (check, class or "*", shape) with the reason:
EXEMPT = {
    # one pixel: a quarter of it is less than a pixel, and a window that holds the pixel alone returns it
    ("median", "*", (1, 1)): "one pixel is its own median",
    ("leftright", "*", (1, 1)): "one pixel is kept or dropped, not both",
    # one column: Lx has to be 0, and no half rounds to 0 (round() goes away from zero): every pixel is dropped
    ("leftright", "half", (7, 1)): "no k + 0.5 rounds to column 0",
    # one pixel whose window is the pixel: when it is not finite and the map has no finite extremum, nothing is rewritten
    ("ranges", "*", (1, 1)): "one pixel: half of it is less than a pixel where that pixel is NaN",
}
needs_refpost = pytest.mark.skipif(not orc_mod.RefPost.available(), reason="oracle/_ref/libmgm_refpost.so was not built here")
NONTRIVIAL = [c for c, t in pd.CLASSES.items() if not t]


def exempt(check, cls, shape):
    return pd.CLASSES[cls] or (check, cls, shape) in EXEMPT or (check, "*", shape) in EXEMPT


# ---- what each check does for one (class, shape): the conditions on the reference, then restatement == reference ------------
def check_median(rp, cls, shape, m, compare=True):
    """-> the smallest share of pixels the reference's median changed over the radii"""
    worst = 1.0
    for r in pd.RADII:
        want = rp.median(m, r)
        worst = min(worst, pd.share_changed(m, want))
        if compare:
            got = post.median(m, r)
            if cls == "signedzero":  # (the reference's zero sign is an artefact of nth_element)
                got, want = pd.mask_zero_signs(got), pd.mask_zero_signs(want)
            assert ndiff(got, want) == 0, ("median", cls, shape, r)
    return worst


def check_leftright(rp, cls, shape, d, compare=True):
    """-> the share the reference keeps at tau = 1 against the fractional `other` of the map's own size"""
    kept = None
    for tag, o, tau in pd.leftright_cases(cls, shape, d):
        want = rp.leftright(d, o, tau)
        if kept is None:
            kept = pd.share_kept(want)
        if compare:
            assert ndiff(post.leftright(d, o, tau), want) == 0, ("leftright", cls, shape, tag)
    return kept


def check_ranges(rp, cls, shape, d, compare=True):
    """-> the smallest share of pixels the reference rewrote over the (slack, radius) cases"""
    lo, hi = pd.ranges(pd.seed_of(cls, shape), *shape)
    worst = 1.0
    for slack, radius in pd.RANGE_CASES:
        wl, wh = rp.update_ranges(d, lo, hi, slack, radius)
        rewritten = (wl.view(np.uint32) != lo.view(np.uint32)) | (wh.view(np.uint32) != hi.view(np.uint32))
        worst = min(worst, float(np.mean(rewritten)))
        if compare:
            gl, gh = post.update_ranges(d, lo, hi, slack, radius)
            assert ndiff(gl, wl) == 0 and ndiff(gh, wh) == 0, ("ranges", cls, shape, slack, radius)
    return worst


@needs_refpost
@pytest.mark.parametrize("cls", list(pd.CLASSES))
def test_median_vs_reference(cls):
    rp = orc_mod.RefPost()
    for shape, m in pd.median_maps(cls):
        if not exempt("median", cls, shape[-2:]):
            assert check_median(rp, cls, shape, m, compare=False) >= 0.25, ("empty case", cls, shape)
        check_median(rp, cls, shape, m)


@needs_refpost
@pytest.mark.parametrize("cls", list(pd.CLASSES))
def test_leftright_vs_reference(cls):
    rp = orc_mod.RefPost()
    for shape in pd.SHAPES:
        d = pd.the_map(cls, shape)
        if not exempt("leftright", cls, shape):
            kept = check_leftright(rp, cls, shape, d, compare=False)
            assert 0.25 <= kept <= 0.75, ("empty case", cls, shape, kept)
        check_leftright(rp, cls, shape, d)


@needs_refpost
@pytest.mark.parametrize("cls", list(pd.CLASSES))
def test_update_ranges_vs_reference(cls):
    rp = orc_mod.RefPost()
    for shape in pd.SHAPES:
        d = pd.the_map(cls, shape)
        if not exempt("ranges", cls, shape):
            assert check_ranges(rp, cls, shape, d, compare=False) >= 0.5, ("empty case", cls, shape)
        check_ranges(rp, cls, shape, d)


# ---- back-projection: through the reference's own command line -----------------------------------------------------------
REF_MGM = orc_mod.REF_MGM
# (nch, vnx, TESTLRRL): the left image is 40 x 24, the right one narrower and wider; v is u moved 12 pixels to the LEFT
CLI_CASES = [(nch, vnx, lr) for nch in (1, 3) for vnx in (28, 46) for lr in (0, 1)]


def _to_file(a):
    return np.ascontiguousarray(a.transpose(1, 2, 0)) if a.shape[0] > 1 else a[0]


@pytest.mark.skipif(not os.path.exists(REF_MGM), reason="reference command line (oracle/_ref/mgm) was not built here")
@pytest.mark.parametrize("nch,vnx,lr", CLI_CASES)
def test_backproject_vs_the_reference_command_line(nch, vnx, lr, tmp_path):
    ny, nx = 24, 40
    # Without the check the matcher finds a label inside v wherever there is one; what then falls outside is the rows v does
    # not have.  (With the check v keeps u's height: leftright_test reads row y of the other map for every row of this one.)
    vny = ny if lr else 16
    u, v = pxd.pair("u8", 31 + nch, nch, ny, nx, vshape=(vny, vnx), shift=-12)
    np.save(tmp_path / "u.npy", _to_file(u))
    np.save(tmp_path / "v.npy", _to_file(v))
    cmd = [REF_MGM, "-r", "-16", "-R", "4", "-t", "ad", "-s", "vfit", "-O", "4", str(tmp_path / "u.npy"), str(tmp_path / "v.npy"),
           str(tmp_path / "disp.npy"), str(tmp_path / "cost.npy"), str(tmp_path / "back.npy")]
    r = subprocess.run(cmd, env=dict(os.environ, TESTLRRL=str(lr), TSGM="2", OMP_NUM_THREADS="2"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    disp = np.load(tmp_path / "disp.npy").astype(np.float32).reshape(ny, nx)
    back = np.load(tmp_path / "back.npy").astype(np.float32)
    back = back.transpose(2, 0, 1) if back.ndim == 3 else back[None]
    assert back.shape == u.shape
    if lr:
        assert np.isnan(disp).mean() > 0.05, "the left-right check is what puts NaN labels into the written map"
    assert np.any(disp != np.rint(disp)), "sub-pixel disparities are the point of the float index"
    inside, k = post.backproject_index(nx, ny, nch, vnx, vny, disp)
    assert 0.25 <= inside.mean() <= 0.75, ("empty case", nch, vnx, lr, inside.mean())
    past = np.broadcast_to(inside[None], k.shape) & (k >= nch * vny * vnx)  # the reference read past the end of its vector there
    got = post.backproject(u, v, disp)
    assert ndiff(np.where(past, 0, got), np.where(past, 0, back)) == 0, (nch, vnx, lr)


# ---- the generator itself -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", list(pd.CLASSES))
def test_generator_is_deterministic_per_seed(cls):
    for ny, nx in pd.SHAPES:
        a, b = pd.disparity(cls, 5, ny, nx), pd.disparity(cls, 5, ny, nx)
        assert a.shape == (ny, nx) and a.dtype == np.float32 and ndiff(a, b) == 0
    if cls not in ("allnan", "constant"):
        assert ndiff(pd.disparity(cls, 5, 11, 13), pd.disparity(cls, 6, 11, 13)) != 0


def test_generator_classes_hold_what_they_promise():
    g = lambda cls, rnc=None: pd.disparity(cls, 3, 11, 13, rnc)
    xs = np.arange(13, dtype=np.float32)[None, :]
    m = g("ties")
    fin = m[np.isfinite(m)]
    assert np.array_equal(fin, np.rint(fin)) and len(np.unique(fin)) <= 5
    s = xs + g("half")
    assert np.mean(s - np.floor(s) == 0.5) > 0.6 and np.any(s < 0) and np.any(s > 0)
    s = xs + g("border", 9)
    for t in (-0.5, 0.0, 8.0, 8.5, 9.0):
        near = np.abs(s - np.float32(t)) <= 2 * np.spacing(np.float32(max(abs(t), 1)))
        assert near.any(), t
    assert np.any(s == 9.0) and np.any(s == np.nextafter(np.float32(9), np.float32(0)))
    m = g("huge")
    assert np.all(np.isfinite(m)) and np.abs(m).min() >= 2.0 ** 24 and np.any(np.abs(m) == np.float32(2.0 ** 31))
    m = g("nonfinite")
    assert np.isnan(m).any() and np.isposinf(m).any() and np.isneginf(m).any() and np.isfinite(m).mean() > 0.3
    assert np.isnan(g("allnan")).all() and np.isfinite(g("onefinite")).sum() == 1
    m = g("denormal")
    fin = m[np.isfinite(m)]
    assert np.all(np.abs(fin) < np.finfo(np.float32).tiny) and np.all(fin != 0) and np.any(fin < 0) and np.any(fin > 0)
    m = g("signedzero")
    assert np.any(np.signbit(m) & (m == 0)) and np.any(~np.signbit(m) & (m == 0)) and np.any(m == 1) and np.any(m == -1)
    assert len(np.unique(g("constant"))) == 1
    lo, hi = pd.ranges(3, 11, 13)
    for a in (lo, hi):
        assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
    assert [c for c, t in pd.CLASSES.items() if t] == ["huge", "allnan", "onefinite", "constant"]


def test_restated_median_orders_negative_zero_below_positive_zero():
    """the project's one rule for both median kernels: rank by the total order"""
    nz, pz = np.float32(-0.0), np.float32(0.0)
    for row, want_negative in (([pz, nz, nz], True), ([nz, pz, pz], False), ([pz, nz], False), ([-1, nz, pz, pz, nz], True),
                               ([nz, nz, pz, pz, 1], False)):
        m = post.median(np.array([row], np.float32), 20)
        assert np.all(m == 0) and np.all(np.signbit(m) == want_negative), row


# ---- the seed search: `python tests/test_post_ref.py` prints a SEEDS table (for tests/post_domains.py) at which the reference meets the conditions -----
def _search():
    rp = orc_mod.RefPost()
    found = {}
    for cls in NONTRIVIAL:
        for shape in pd.SHAPES:
            for seed in range(200):
                pd.SEEDS[(cls, shape)] = seed
                d = pd.the_map(cls, shape)
                ok = exempt("median", cls, shape) or check_median(rp, cls, shape, d[None], compare=False) >= 0.25
                if ok and shape == (11, 13):
                    ok = check_median(rp, cls, (2, 11, 13), pd.two_channel(cls, seed), compare=False) >= 0.25
                ok = ok and (exempt("leftright", cls, shape) or 0.25 <= check_leftright(rp, cls, shape, d, compare=False) <= 0.75)
                ok = ok and (exempt("ranges", cls, shape) or check_ranges(rp, cls, shape, d, compare=False) >= 0.5)
                if ok:
                    break
            else:
                print("# no seed below 200 for", cls, shape)
                del pd.SEEDS[(cls, shape)]
                continue
            if seed:
                found[(cls, shape)] = seed
    print("SEEDS = %r" % (found,))


if __name__ == "__main__":
    _search()
