"""Seeded disparity maps and range images in named EDGE CLASSES -- test infrastructure, no GPU.

The post-processing kernels (median, left-right check, range update, back-projection) were pinned on one kind of map only,
`nan_label_map` of tests/test_oracle_vs_ref.py: random sub-pixel labels with NaN holes.  This module draws the maps on which such
kernels go wrong: value ties, signed zeros, `x + d` on exact halves and within an ulp of the other image's borders, huge and
non-finite disparities, maps that are all NaN or hold one sample, denormals, maps smaller than any window.

    d = disparity("border", seed, ny, nx, rnc)      # float32 (ny, nx); rnc = width of the OTHER image (default nx)
    o = other_map(seed, d, rnc, rny, integer)       # a right-to-left map that agrees with d at about 70 % of its targets
    lo, hi = ranges(seed, ny, nx)                   # range images with NaN and +-INF entries

`CLASSES` maps each name to its `trivial` flag: a trivial class leaves the kernels nothing to choose (every disparity outside the
other image, no sample or one sample, one value), so the non-emptiness conditions of tests/test_post_ref.py are not asked of it.
"""
import numpy as np

f32 = np.float32
FLT_MAX = f32(3.4028234663852886e38)
# name -> trivial.  `huge`, `allnan` and `constant` are trivial by construction; `onefinite` joins them by arithmetic: with one
# finite sample the left-right check can keep one pixel and the back-projection can take one pixel from the other image, never
# a quarter of them.
CLASSES = {"control": False, "ties": False, "half": False, "border": False, "huge": True, "nonfinite": False, "allnan": True,
           "onefinite": True, "denormal": False, "signedzero": False, "constant": True}
SHAPES = [(1, 1), (1, 9), (7, 1), (3, 4), (11, 13)]  # (ny, nx)
HUGE = [f32(2.0 ** 24), f32(2.0 ** 24 + 2), f32(1e9), np.nextafter(f32(2.0 ** 31), f32(0)), f32(2.0 ** 31),
        np.nextafter(f32(2.0 ** 31), f32(np.inf)), f32(3e9), f32(2.0 ** 32), f32(1e30), f32(3.4e38), FLT_MAX]


def _holes(rng, m, frac, value=np.nan):
    """`value` at isolated pixels (share `frac`) and in one patch of a third of each side (where the map has room for one)."""
    ny, nx = m.shape
    m[rng.random((ny, nx)) < frac] = value
    py, px = ny // 3, nx // 3
    if py and px:
        y0, x0 = int(rng.integers(0, ny - py + 1)), int(rng.integers(0, nx - px + 1))
        m[y0:y0 + py, x0:x0 + px] = value


def _landing(x, t):
    """A float32 d with float32(x + d) == t where one exists next to float32(t - x), else float32(t - x)."""
    x, t = f32(x), f32(t)
    d0 = f32(t - x)
    for d in (d0, np.nextafter(d0, f32(np.inf)), np.nextafter(d0, f32(-np.inf))):
        if f32(x + d) == t:
            return d
    return d0


def disparity(cls, seed, ny, nx, rnc=None):
    """A float32 (ny, nx) map of class `cls`; deterministic in all its arguments.  `rnc` is the width of the image the
    disparities point into (the classes `half` and `border` aim at its columns)."""
    if cls not in CLASSES:
        raise ValueError("unknown map class %r" % (cls,))
    rnc = nx if rnc is None else rnc
    rng = np.random.default_rng([seed, sorted(CLASSES).index(cls), ny, nx, rnc])
    amp = max(1.0, nx / 2.0)  # most of x + d stays inside an image of about this width, some of it leaves on either side
    xs = np.broadcast_to(np.arange(nx, dtype=f32)[None, :], (ny, nx))
    if cls == "control":  # what the NaN-faithful path leaves: sub-pixel labels, NaN isolated and in a patch
        m = rng.uniform(-amp, amp, (ny, nx)).astype(f32)
        _holes(rng, m, 0.15)
    elif cls == "ties":  # whole numbers in -2..2: every window holds each value several times
        m = rng.integers(-2, 3, (ny, nx)).astype(f32)
        _holes(rng, m, 0.08)
    elif cls == "half":  # x + d = k + 0.5 exactly, k + 0.5 of both signs: round() goes away from zero, rint() to even
        k = rng.integers(-3, rnc + 2, (ny, nx)).astype(f32) + f32(0.5)
        m = (k - xs).astype(f32)
        pick = rng.random((ny, nx)) < 0.3  # ... and d itself a half, so that the median ranks halves of both signs
        m[pick] = (rng.integers(-3, 3, (ny, nx)).astype(f32) + f32(0.5))[pick]
    elif cls == "border":  # x + d on, one ulp below and one ulp above each border value of the other image
        targets = [f32(-0.5), f32(0), f32(rnc - 1), f32(rnc - 0.5), f32(rnc)]
        # (on a control background: the targets name two columns of the other image, which can agree with a few pixels only)
        m = rng.uniform(-amp, amp, (ny, nx)).astype(f32)
        for y in range(ny):
            for x in range(nx):
                if rng.random() < 0.4:
                    continue
                t = targets[int(rng.integers(0, len(targets)))]
                t = (np.nextafter(t, f32(-np.inf)), t, np.nextafter(t, f32(np.inf)))[int(rng.integers(0, 3))]
                m[y, x] = _landing(x, t)
    elif cls == "huge":  # |d| from 2^24 (where x + d stops being exact) to FLT_MAX, +-2^31 and its float neighbours included
        m = np.array(HUGE, f32)[rng.integers(0, len(HUGE), (ny, nx))] * np.where(rng.random((ny, nx)) < 0.5, f32(-1), f32(1))
    elif cls == "nonfinite":  # +INF, -INF and NaN, each isolated and in a patch, on a control background
        m = rng.uniform(-amp, amp, (ny, nx)).astype(f32)
        for value in (np.nan, np.inf, -np.inf):
            _holes(rng, m, 0.08, value)
    elif cls == "allnan":
        m = np.full((ny, nx), np.nan, f32)
    elif cls == "onefinite":
        m = np.full((ny, nx), np.nan, f32)
        m[int(rng.integers(0, ny)), int(rng.integers(0, nx))] = f32(rng.integers(-1, 2))
    elif cls == "denormal":  # multiples of 1e-40 of both signs: x + d == x, but the median has to order them
        m = (rng.integers(1, 100, (ny, nx)) * np.where(rng.random((ny, nx)) < 0.5, -1, 1)).astype(f32) * f32(1e-40)
        _holes(rng, m, 0.05)
    elif cls == "signedzero":  # both zeros in every window, a few other values around them, some NaN
        vals = np.array([-0.0, 0.0, -1.0, 1.0, np.nan], f32)
        m = vals[rng.choice(5, size=(ny, nx), p=[0.3, 0.3, 0.15, 0.15, 0.1])]
    elif cls == "constant":
        m = np.full((ny, nx), 2.0, f32)
    return np.ascontiguousarray(m, f32)


def other_map(seed, d, rnc, rny=None, integer=False):
    """A map (rny, rnc) for the other side of the left-right check: random labels, then at about 70 % of the columns d points
    into (round half away from zero) the label that sends the pixel back to where it came from -- exactly, or a quarter of a
    pixel off unless `integer` -- and a few NaN and +-INF entries.  rny >= d's rows; the extra rows are never read."""
    ny, nx = d.shape
    rny = ny if rny is None else rny
    rng = np.random.default_rng([seed, 77, ny, nx, rnc, rny, int(integer)])
    amp = max(3.0, rnc / 2.0)
    o = rng.uniform(-amp, amp, (rny, rnc)).astype(f32)
    if integer:
        o = np.rint(o).astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (np.arange(nx, dtype=f32)[None, :] + d).astype(np.float64)
        r = np.sign(s) * np.floor(np.abs(s) + 0.5)
    for y in range(ny):
        for x in range(nx):
            if np.isfinite(r[y, x]) and 0 <= r[y, x] < rnc and rng.random() < 0.7:
                Lx = int(r[y, x])
                o[y, Lx] = f32(x - Lx) + (f32(0) if integer else f32(0.25))
    o[rng.random((rny, rnc)) < 0.04] = np.nan
    o[rng.random((rny, rnc)) < 0.03] = np.inf
    o[rng.random((rny, rnc)) < 0.03] = -np.inf
    return np.ascontiguousarray(o, f32)


def ranges(seed, ny, nx):
    """(lo, hi) range images around -40 / 20 with sub-pixel parts, NaN, +INF and -INF entries in both."""
    rng = np.random.default_rng([seed, 78, ny, nx])
    lo = (f32(-40) + rng.uniform(-3, 3, (ny, nx))).astype(f32)
    hi = (f32(20) + rng.uniform(-3, 3, (ny, nx))).astype(f32)
    for a in (lo, hi):
        r = rng.random((ny, nx))
        a[r < 0.1] = np.nan
        a[(r >= 0.1) & (r < 0.2)] = np.inf
        a[(r >= 0.2) & (r < 0.3)] = -np.inf
    return lo, hi


def two_channel(cls, seed, ny=11, nx=13):
    """The one multi-channel map of the median sweep: two maps of the class, different seeds."""
    return np.stack([disparity(cls, seed, ny, nx), disparity(cls, seed + 1000, ny, nx)])


def mask_zero_signs(a):
    """-0 -> +0: for the two comparisons in which the reference's zero sign is an artefact."""
    a = np.array(a, f32, copy=True)
    a[a == 0] = 0.0
    return a


# ---- the conditions that keep a case from passing by being empty ----------------------------------------------------------
def share_changed(before, after):
    """share of words that differ (NaN == NaN; the zeros by VALUE, their sign is not a change)"""
    a, b = np.asarray(before, f32).ravel(), np.asarray(after, f32).ravel()
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    return float(np.mean(~same))


def share_kept(checked):
    return float(np.mean(~np.isnan(np.asarray(checked))))


# ---- the cases both test files run: tests/test_post_ref.py on the CPU, tests/test_gpu_post_edges.py on the device ----------
RADII = (1, 2, 7, 8, 20)
TAUS = (1.0, 0.0, -1.0, np.inf, np.nan, 1e-45, 2.0 ** 24)   # the first is the one the condition is asserted at
WIDTHS = (1, 6, 9, 30)                                       # widths of `other` besides the map's own
RANGE_CASES = ((3, 2), (0, 0), (-3, 1), (5, 16), (0, 2), (2 ** 30, 1))  # (slack, radius)
# (class, shape) -> seed; 0 where not listed.  The seeds at which the REFERENCE alone meets the non-emptiness conditions of
# tests/test_post_ref.py (found by `python tests/test_post_ref.py`, which looks at the reference's results only)
SEEDS = {('ties', (7, 1)): 5, ('border', (1, 9)): 3, ('denormal', (3, 4)): 1, ('signedzero', (1, 9)): 3}


def seed_of(cls, shape):
    return SEEDS.get((cls, shape), 0)


def the_map(cls, shape):
    return disparity(cls, seed_of(cls, shape), shape[0], shape[1])


def median_maps(cls):
    for shape in SHAPES:
        yield shape, the_map(cls, shape)[None]
    yield (2, 11, 13), two_channel(cls, seed_of(cls, (11, 13)))


def leftright_cases(cls, shape, d):
    """(tag, other, tau): the map's own width at every tau, integer and fractional; the other widths at three taus; an
    `other` with more rows than d"""
    ny, nx = shape
    seed = seed_of(cls, shape)
    for integer in (False, True):
        o = other_map(seed, d, nx, integer=integer)
        for tau in TAUS:
            yield ("own", integer, tau), o, tau
    yield ("taller",), other_map(seed, d, nx, rny=ny + 3), 1.0
    for w in WIDTHS:
        o = other_map(seed, d, w)
        for tau in (1.0, 0.0, 2.0 ** 24):
            yield ("width", w, tau), o, tau
