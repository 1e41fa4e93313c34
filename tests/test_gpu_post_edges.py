"""mgm_post.hip (k_median / k_median_big, k_leftright, k_backproject) and k_update_ranges on the EDGE maps of
tests/post_domains.py: value ties, signed zeros, x + d on exact halves and within an ulp of the other image's borders, huge and
non-finite disparities, all-NaN and one-sample maps, denormals, maps smaller than the window (1x1, 1x9, 7x1, 3x4, 11x13).

Every result is compared BIT FOR BIT (NaN == NaN) with the numpy restatements of oracle/post.py, which tests/test_post_ref.py
pins on the compiled reference on the same maps and seeds, and with the compiled reference itself where it travelled
(oracle/_ref/libmgm_refpost.so).  Two comparisons mask the sign of zero, both on the class `signedzero` only:
the median AGAINST THE REFERENCE (whose zero is whatever nth_element leaves at v[n/2]; against the restatement it is bit for
bit: one rule, the total order, for both kernels), and the range update (the reference folds zeros in operand order, the
kernel with v_min_f32 and ordered-bit atomics).

Every test asserts from the context's timing table that the kernel it names ran.  The table has ONE name, `k_median`, for
k_median and k_median_big (mgm_median_dev times the call, not the kernel): that radius 8 and the chunked cases take the radix
kernel follows from launch_median (radius > 7), not from the table; and a block that wraps many calls is satisfied by one entry.
"""
import numpy as np
import pytest

import post_domains as pd
from helpers import ndiff

pytestmark = pytest.mark.gpu
f32 = np.float32


def refpost():
    from oracle.oracle import RefPost
    return RefPost() if RefPost.available() else None


class ran:
    """with ran(ctx, "k_median"): ...  -- the timing table of the block must name the kernel (refused=True: must not)"""

    def __init__(self, ctx, name, refused=False):
        self.ctx, self.name, self.refused = ctx, name, refused

    def __enter__(self):
        self.ctx.timing(True)
        self.ctx.timing_reset()

    def __exit__(self, exc_type, exc, tb):
        names = [n for n, _ in self.ctx.timings()]
        self.ctx.timing(False)
        self.ctx.timing_reset()
        if exc_type is None:
            assert (self.name in names) != self.refused, (self.name, names)
        return False


def free(*hs):
    for h in hs:
        h.free()


# ---- median ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", list(pd.CLASSES))
def test_median_edges(ctx, cls):
    from oracle import post
    rp = refpost()
    with ran(ctx, "k_median"):
        for shape, m in pd.median_maps(cls):
            d = ctx.upload_image(m)
            for r in pd.RADII:
                got = ctx.median_dev(d, r)
                g = got.download()
                assert ndiff(g, post.median(m, r)) == 0, (cls, shape, r)
                if rp is not None:
                    want = rp.median(m, r)
                    if cls == "signedzero":
                        g, want = pd.mask_zero_signs(g), pd.mask_zero_signs(want)
                    assert ndiff(g, want) == 0, (cls, shape, r, "reference")
                got.free()
            d.free()


def whole_map_median(m):
    """post.median where the window is the whole map at every pixel: one value per channel (a pixel keeps its own only in a
    channel without any sample)"""
    from oracle import post
    out = np.array(m, f32, copy=True)
    for c in range(m.shape[0]):
        w = m[c][~np.isnan(m[c])]
        if w.size:
            out[c] = w[np.argsort(post.total_order_key(w), kind="stable")[w.size // 2]]
    return out


@pytest.mark.parametrize("nch,ny,nx,radius,launches", [(1, 30, 40, 1024, 2), (2, 30, 40, 1024, 3), (1, 100, 128, 300, 2)])
def test_median_cut_into_several_launches(ctx, nch, ny, nx, radius, launches):
    """k_median_big's work is cut into launches of `chunk` outputs (launch_median): 1024 at radius 1024, 12544 at radius 300.
    40x30 is two launches, two channels of it three with the cuts at 1024 and 2048 INSIDE the channels (they meet at 1200);
    128x100 at radius 300 is two.  Every window is the whole map."""
    from oracle import post
    chunk = int(1.5e11 / (33.0 * (2 * radius + 1) ** 2)) // 256 * 256
    assert -(-nch * ny * nx // chunk) == launches and (ny * nx) % chunk != 0
    for cls in ("signedzero", "ties", "control"):
        m = np.stack([pd.disparity(cls, 40 + c, ny, nx) for c in range(nch)])
        want = whole_map_median(m)
        if ny * nx <= 1200:
            assert ndiff(want, post.median(m, radius)) == 0
        d, out = ctx.upload_image(m), ctx.upload_image(np.full(m.shape, 777.0, f32))  # (what no launch writes stays 777)
        with ran(ctx, "k_median"):
            ctx.median_dev(d, radius, out=out)
        assert ndiff(out.download(), want) == 0, cls
        free(d, out)


@pytest.mark.parametrize("cls", ["signedzero", "ties", "denormal", "nonfinite"])
def test_median_radii_7_and_8_are_one_filter(ctx, cls):
    """launch_median sends radius 7 to k_median and radius 8 to k_median_big (the timing table cannot tell them apart); on an 8x8
    map both windows are the whole map: one expectation"""
    m = np.stack([pd.disparity(cls, 7 + c, 8, 8) for c in range(2)])
    want = whole_map_median(m)
    d = ctx.upload_image(m)
    with ran(ctx, "k_median"):
        a, b = ctx.median_dev(d, 7), ctx.median_dev(d, 8)
    assert ndiff(a.download(), want) == 0 and ndiff(b.download(), want) == 0, cls
    free(d, a, b)


# ---- left-right check -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", list(pd.CLASSES))
def test_leftright_edges(ctx, cls):
    from oracle import post
    rp = refpost()
    with ran(ctx, "k_leftright"):
        for shape in pd.SHAPES:
            d = pd.the_map(cls, shape)
            dd = ctx.upload_image(d)
            for tag, o, tau in pd.leftright_cases(cls, shape, d):
                do = ctx.upload_image(o)
                got = ctx.leftright_dev(dd, do, tau)
                g = got.download()[0]
                assert ndiff(g, post.leftright(d, o, tau)) == 0, (cls, shape, tag)
                if rp is not None:
                    assert ndiff(g, rp.leftright(d, o, tau)) == 0, (cls, shape, tag, "reference")
                free(do, got)
            dd.free()


@pytest.mark.parametrize("cls", ["control", "half", "border"])
def test_leftright_in_place_equals_out_of_place(ctx, cls):
    """`out` may be `d` (each thread reads its own pixel of d before it writes it); `other` may have more rows than d"""
    from oracle import post
    d = pd.the_map(cls, (11, 13))
    o = pd.other_map(1, d, 9, rny=14)
    dd, do = ctx.upload_image(d), ctx.upload_image(o)
    with ran(ctx, "k_leftright"):
        apart = ctx.leftright_dev(dd, do, 1.0)
        same = ctx.leftright_dev(dd, do, 1.0, out=dd)
    assert same is dd
    want = post.leftright(d, o, 1.0)
    assert 0 < np.isnan(want).sum() - np.isnan(d).sum(), "the check has to drop something for in place to matter"
    assert ndiff(apart.download()[0], want) == 0 and ndiff(dd.download()[0], want) == 0
    free(dd, do, apart)


# ---- range update ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", list(pd.CLASSES))
def test_update_ranges_edges(ctx, cls):
    from oracle import post
    rp = refpost()
    with ran(ctx, "k_update_ranges"):
        for shape in pd.SHAPES:
            d = pd.the_map(cls, shape)
            lo, hi = pd.ranges(pd.seed_of(cls, shape), *shape)
            dd = ctx.upload_image(d)
            for slack, radius in pd.RANGE_CASES:
                # (the one exemption: zeros meet zeros only with slack 0 -- v - 3 == 0 is always +0 -- DESIGN section 1)
                canon = pd.mask_zero_signs if cls == "signedzero" and slack == 0 else (lambda a: a)
                dl, dh = ctx.upload_image(lo), ctx.upload_image(hi)
                ctx.update_ranges_dev(dd, dl, dh, slack, radius)
                gl, gh = canon(dl.download()[0]), canon(dh.download()[0])
                wl, wh = post.update_ranges(d, lo, hi, slack, radius)
                assert ndiff(gl, canon(wl)) == 0 and ndiff(gh, canon(wh)) == 0, (cls, shape, slack, radius)
                if rp is not None:
                    wl, wh = rp.update_ranges(d, lo, hi, slack, radius)
                    assert ndiff(gl, canon(wl)) == 0 and ndiff(gh, canon(wh)) == 0, (cls, shape, slack, radius, "reference")
                free(dl, dh)
            dd.free()


# ---- back-projection ------------------------------------------------------------------------------------------------------
def distinct_images(nch, ny, nx, vny, vnx):
    """no two elements of u and v alike: a wrong index cannot return the right value"""
    u = (f32(1000) + np.arange(nch * ny * nx, dtype=f32)).reshape(nch, ny, nx)
    v = (f32(-1) - np.arange(nch * vny * vnx, dtype=f32)).reshape(nch, vny, vnx)
    return u, v


def v_shapes(ny, nx):
    """(name, vny, vnx): the same size, narrower, wider, shorter, taller (narrower / shorter only where u has the room)"""
    out = [("same", ny, nx), ("wider", ny, nx + 5), ("taller", ny + 3, nx)]
    if nx > 1:
        out.append(("narrower", ny, max(1, nx - 3)))
    if ny > 1:
        out.append(("shorter", max(1, ny - 2), nx))
    return out


@pytest.mark.parametrize("cls", ["control", "ties", "half", "border", "huge", "nonfinite", "signedzero", "denormal"])
def test_backproject_edges(ctx, cls):
    from oracle import post
    with ran(ctx, "k_backproject"):
        for (ny, nx) in pd.SHAPES:
            for nch in (1, 3):
                for name, vny, vnx in v_shapes(ny, nx):
                    u, v = distinct_images(nch, ny, nx, vny, vnx)
                    d = pd.disparity(cls, pd.seed_of(cls, (ny, nx)), ny, nx, vnx)
                    inside, _ = post.backproject_index(nx, ny, nch, vnx, vny, d)
                    if not pd.CLASSES[cls] and (ny, nx) == (11, 13) and name == "shorter":
                        assert 0.25 <= inside.mean() <= 0.75, ("empty case", cls, inside.mean())  # a quarter from each image
                    du, dv, dd = ctx.upload_image(u), ctx.upload_image(v), ctx.upload_image(d)
                    got = ctx.backproject_dev(du, dv, dd)
                    assert ndiff(got.download(), post.backproject(u, v, d)) == 0, (cls, ny, nx, nch, name)
                    free(du, dv, dd, got)


def test_backproject_reads_the_last_element_where_the_reference_reads_past_the_end(ctx):
    """Last pixel of the last channel, x + d just below the width: the float index rounds up to nch * npix, one past the end of
    v.  The reference copies what follows its vector; the library reads the last element."""
    from oracle import post
    nch, ny, nx = 2, 3, 5
    u, v = distinct_images(nch, ny, nx, ny, nx)
    d = np.zeros((ny, nx), f32)
    d[-1, -1] = f32(np.nextafter(f32(nx), f32(0)) - f32(nx - 1))  # 4 + d = 4.9999995 < 5: inside
    inside, k = post.backproject_index(nx, ny, nch, nx, ny, d)
    assert inside[-1, -1] and k[-1, -1, -1] == nch * ny * nx, "the case has to be the one it names"
    du, dv, dd = ctx.upload_image(u), ctx.upload_image(v), ctx.upload_image(d)
    with ran(ctx, "k_backproject"):
        got = ctx.backproject_dev(du, dv, dd)
    g = got.download()
    assert g[-1, -1, -1] == v[-1, -1, -1]
    assert ndiff(g, post.backproject(u, v, d)) == 0
    free(du, dv, dd, got)


def test_backproject_index_beyond_2_to_the_23(ctx):
    """From 2^23 on a float holds no fraction: x + d + y * vnx + c * vnpix drops the fraction of the disparity and rounds halves
    to even.  The smallest shape that gets there: the index passes 2^23 in the THIRD channel as soon as v has more than 2^22
    pixels -- v is 3 x 2049 x 2048 (50 MB); u need not be large (3 x 4 x 2048).  In the second channel (offset 2^22 + 2048)
    floats step by 0.5 and quarters are what rounds."""
    from oracle import post
    nch, ny, nx, vny, vnx = 3, 4, 2048, 2049, 2048
    rng = np.random.default_rng(23)
    u = (f32(-1) - np.arange(nch * ny * nx, dtype=f32)).reshape(nch, ny, nx)
    v = np.arange(nch * vny * vnx, dtype=f32).reshape(nch, vny, vnx)  # (below 2^24: every element names its own index)
    assert v.size < 2 ** 24
    land = rng.integers(-40, vnx + 40, (ny, nx)).astype(f32) + rng.integers(0, 4, (ny, nx)).astype(f32) * f32(0.25)
    d = land - np.arange(nx, dtype=f32)[None, :]
    inside, k = post.backproject_index(nx, ny, nch, vnx, vny, d)
    assert k.max() >= 2 ** 23 and 0.9 < inside.mean() < 1.0
    exact = np.floor(np.arange(nx)[None, :] + d.astype(np.float64)) + np.arange(ny)[:, None] * vnx  # the index without rounding
    up = (k[2].astype(np.float64) - 2 * vny * vnx > exact) & inside
    assert up.mean() > 0.2 and (inside & ~up).mean() > 0.2, "halves go to even: up at some pixels, down at others"
    du, dv, dd = ctx.upload_image(u), ctx.upload_image(v), ctx.upload_image(d)
    with ran(ctx, "k_backproject"):
        got = ctx.backproject_dev(du, dv, dd)
    assert ndiff(got.download(), post.backproject(u, v, d)) == 0
    free(du, dv, dd, got)


# ---- refusals, each with its status code ----------------------------------------------------------------------------------
def refused(ctx, kernel, call, code=None):
    import mgm_amd
    with ran(ctx, kernel, refused=True):
        with pytest.raises(mgm_amd.MgmError) as e:
            call()
    assert e.value.code == (mgm_amd.MGM_ERR_INVALID if code is None else code), e.value


def test_median_refusals(ctx):
    a, b, small, two = ctx.new_image(13, 11), ctx.new_image(13, 11), ctx.new_image(12, 11), ctx.new_image(13, 11, 2)
    refused(ctx, "k_median", lambda: ctx.median_dev(a, 1, out=a))      # in is out
    refused(ctx, "k_median", lambda: ctx.median_dev(a, 0, out=b))      # radius 0
    refused(ctx, "k_median", lambda: ctx.median_dev(a, 1025, out=b))   # radius 1025
    refused(ctx, "k_median", lambda: ctx.median_dev(a, 1, out=small))  # size mismatch
    refused(ctx, "k_median", lambda: ctx.median_dev(a, 1, out=two))    # channel mismatch
    with ran(ctx, "k_median"):
        ctx.median_dev(a, 1024, out=b)                                 # (the largest radius is accepted on a small map)
    free(a, b, small, two)


def test_leftright_refusals(ctx):
    d, o, out, low, two = ctx.new_image(13, 11), ctx.new_image(9, 11), ctx.new_image(13, 11), ctx.new_image(9, 10), ctx.new_image(13, 11, 2)
    o13 = ctx.new_image(13, 11)
    refused(ctx, "k_leftright", lambda: ctx.leftright_dev(d, o13, 1.0, out=o13))  # out is other
    refused(ctx, "k_leftright", lambda: ctx.leftright_dev(d, low, 1.0, out=out))  # other with fewer rows than d
    refused(ctx, "k_leftright", lambda: ctx.leftright_dev(two, o, 1.0, out=out))  # multi-channel d
    refused(ctx, "k_leftright", lambda: ctx.leftright_dev(d, two, 1.0, out=out))  # multi-channel other
    refused(ctx, "k_leftright", lambda: ctx.leftright_dev(d, o, 1.0, out=two))    # multi-channel out
    free(d, o, out, low, two, o13)


def test_update_ranges_refusals(ctx):
    d, lo, hi, two, small = ctx.new_image(13, 11), ctx.new_image(13, 11), ctx.new_image(13, 11), ctx.new_image(13, 11, 2), ctx.new_image(13, 10)
    refused(ctx, "k_update_ranges", lambda: ctx.update_ranges_dev(d, lo, hi, 3, 17))   # radius 17
    refused(ctx, "k_update_ranges", lambda: ctx.update_ranges_dev(d, lo, hi, 3, -1))
    refused(ctx, "k_update_ranges", lambda: ctx.update_ranges_dev(two, lo, hi, 3, 2))  # multi-channel arguments
    refused(ctx, "k_update_ranges", lambda: ctx.update_ranges_dev(d, two, hi, 3, 2))
    refused(ctx, "k_update_ranges", lambda: ctx.update_ranges_dev(d, lo, small, 3, 2))
    with ran(ctx, "k_update_ranges"):
        ctx.update_ranges_dev(d, lo, hi, 3, 16)                                        # (the largest radius is accepted)
    free(d, lo, hi, two, small)


def test_backproject_refusals(ctx):
    u, v, disp, out = ctx.new_image(13, 11, 3), ctx.new_image(9, 12, 3), ctx.new_image(13, 11), ctx.new_image(13, 11, 3)
    v1, disp2, dsmall, osmall, o1 = ctx.new_image(9, 12, 1), ctx.new_image(13, 11, 2), ctx.new_image(12, 11), ctx.new_image(13, 10, 3), ctx.new_image(13, 11, 1)
    refused(ctx, "k_backproject", lambda: ctx.backproject_dev(u, v1, disp, out=out))     # channel mismatch u / v
    refused(ctx, "k_backproject", lambda: ctx.backproject_dev(u, v, disp2, out=out))     # a disparity map of two channels
    refused(ctx, "k_backproject", lambda: ctx.backproject_dev(u, v, disp, out=o1))       # channel mismatch u / out
    refused(ctx, "k_backproject", lambda: ctx.backproject_dev(u, v, dsmall, out=out))    # size mismatch u / disp
    refused(ctx, "k_backproject", lambda: ctx.backproject_dev(u, v, disp, out=osmall))   # size mismatch u / out
    free(u, v, disp, out, v1, disp2, dsmall, osmall, o1)
