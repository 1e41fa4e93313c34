"""Crafted Lr volumes for the runner-up search (k_wta_runnerup / k_wta_runnerup_any), on top of tests/wta_crafted.py.

The classes of wta_crafted.LR_CLASSES put ties, pass-order-dependent sums, overflow and non-finite values in front of a winner
search; none of them aims at the boundary of the exclusion zone [o1 - radius, o1 + radius], where the runner-up search differs
from it.  The classes here do.  An Lr class keeps the signature (seed, NDIR, ny, nx, L) -> float32 [NDIR][ny][nx][L] and the
pixel numbering i = y * nx + x of wta_crafted; the two parameters of this module, `radius` (of the search under test) and `LPL`
(labels per lane of the kernel instance under test, 1 for the generic kernel), are bound by classes(radius, LPL).

What a class plants sits in pass 0; at the planted labels the other passes hold 0.  On the pixels wta_crafted.PLANTED every C
class holds one finite value on all labels, so the plant survives the over-count term there whatever the class of C (f * c
stays below 2^11, the planted values are 1 apart: no two of them round together); without the fix it survives on every pixel.

Winner positions (POSITIONS; pixel i takes position (i + i // 7) % 7, the next valid one where L is too small for it):
    0  label 0                                   the zone clips at 0
    1  label radius                              the zone's lower end is label 0 exactly: the runner-up can only lie above
    2  label L-1                                 the zone clips at L-1
    3  label L-1-radius                          the zone's upper end is label L-1 exactly
    4  a multiple of LPL                         the winner the first label of its lane, the runner-up (below) in a lane before
    5  a multiple of LPL, minus 1                the winner the last label of its lane, the runner-up (above) in a lane behind
    6  (w + radius + 1) % LPL == 0               the runner-up (above) the first label of its lane, the zone ends with the lane before
The side of the runner-up alternates by pixel at positions 0..3 and is as stated at 4..6; where that side has no label, the other.
"""
import numpy as np

import wta_crafted as W

f32 = np.float32
WIN, ZONE, BESIDE = f32(-8), f32(-7), f32(-6)
NPOS = 7


def position(k, L, radius, LPL):
    """the winner's label at position k, or None where L has no room for it"""
    mid = (L // 2) // LPL * LPL
    w = {0: 0, 1: radius, 2: L - 1, 3: L - 1 - radius,
         4: max(mid, -(-(radius + 1) // LPL) * LPL),                  # >= radius + 1: the label radius + 1 below exists
         5: max(mid, LPL) - 1,
         6: max(mid, -(-(radius + 1) // LPL) * LPL) - radius - 1}[k]
    if not 0 <= w < L:
        return None
    if k == 4 and w - radius - 1 < 0 or k in (5, 6) and w + radius + 1 > L - 1:
        return None
    return w


def winner_of(i, L, radius, LPL):
    """(position, label) of pixel i: position (i + i // 7) % 7, or the next one that L has room for (position 0 always has)"""
    k0 = (i + i // NPOS) % NPOS
    for j in range(NPOS):
        k = (k0 + j) % NPOS
        w = position(k, L, radius, LPL)
        if w is not None:
            return k, w
    raise AssertionError("position 0 exists at every L >= 1")


def beside_of(i, k, w, L, radius):
    """the label radius + 1 away from the winner on this pixel's side (below: even pixels at positions 0..3, position 4), the
    other side where that one has no label, None where neither has"""
    below = (i % 2 == 0) if k < 4 else (k == 4)
    lo, hi = w - radius - 1, w + radius + 1
    first, second = (lo, hi) if below else (hi, lo)
    for b in (first, second):
        if 0 <= b < L:
            return b
    return None


def _background(rng, NDIR, npix, L):
    """integers 0..3 in every pass: S >= 0 wherever nothing is planted, and exact in any order"""
    return rng.integers(0, 4, (NDIR, npix, L)).astype(np.float32)


def _plant(flat, i, labels, values):
    flat[:, i, labels] = 0
    flat[0, i, labels] = values


def lr_zone(seed, NDIR, ny, nx, L, radius=1, LPL=1):
    """every pixel: the winner w at -8, every other label within `radius` of it at -7 (cheaper than the rest, inside the zone),
    ONE label exactly radius + 1 away at -6, everything else >= 0: the runner-up lies directly beside the zone"""
    rng = np.random.default_rng(seed)
    flat = _background(rng, NDIR, ny * nx, L)
    for i in range(ny * nx):
        k, w = winner_of(i, L, radius, LPL)
        zone = np.arange(max(0, w - radius), min(L - 1, w + radius) + 1)
        _plant(flat, i, zone, ZONE)
        _plant(flat, i, w, WIN)
        b = beside_of(i, k, w, L, radius)
        if b is not None:
            _plant(flat, i, b, BESIDE)
    return flat.reshape(NDIR, ny, nx, L)


def lr_only_zone(seed, NDIR, ny, nx, L, radius=1, LPL=1):
    """finite values only inside [w - radius, w + radius] (w at -8, the others in [-7, -6)); everywhere else +INF, -INF, NaN in
    turn by label, in pass 0: there is no runner-up.  Pixels i % 5 == 4 keep exactly one finite label, pixels i % 7 == 6 none."""
    rng = np.random.default_rng(seed)
    flat = _background(rng, NDIR, ny * nx, L)
    bad = np.array([np.inf, -np.inf, np.nan], np.float32)
    for i in range(ny * nx):
        k, w = winner_of(i, L, radius, LPL)
        row = bad[(np.arange(L) + i) % 3]
        if i % 7 != 6:
            if i % 5 != 4:
                zone = np.arange(max(0, w - radius), min(L - 1, w + radius) + 1)
                row[zone] = rng.uniform(-7, -6, len(zone)).astype(np.float32)
            row[w] = WIN
        fin = np.isfinite(row)
        flat[:, i, :] = np.where(fin, f32(0), flat[:, i, :])
        flat[0, i, :] = row
    return flat.reshape(NDIR, ny, nx, L)


def only_zone_kinds(ny, nx):
    """(pixels without a finite label, pixels with exactly one)"""
    i = np.arange(ny * nx).reshape(ny, nx)
    return i % 7 == 6, (i % 7 != 6) & (i % 5 == 4)


def far_tie_of(w, L, radius):
    """a label more than radius + 1 away from w, half the range further on (wrapping), or None"""
    f = (w + L // 2) % L
    return f if abs(f - w) > radius + 1 else None


def two_sided_tied(ny, nx):
    return np.arange(ny * nx).reshape(ny, nx) % 3 == 2


def lr_two_sided(seed, NDIR, ny, nx, L, radius=1, LPL=1):
    """as `zone`, with -6 on BOTH labels radius + 1 away from the winner (those that exist): two equal runner-up candidates, the
    lower label wins.  Pixels i % 3 == 2 also hold the winner's own -8 on a label far from it (far_tie_of): cost2 == cost1, and
    out2 is the second of the two tied labels."""
    rng = np.random.default_rng(seed)
    flat = _background(rng, NDIR, ny * nx, L)
    for i in range(ny * nx):
        k, w = winner_of(i, L, radius, LPL)
        zone = np.arange(max(0, w - radius), min(L - 1, w + radius) + 1)
        _plant(flat, i, zone, ZONE)
        _plant(flat, i, w, WIN)
        for b in (w - radius - 1, w + radius + 1):
            if 0 <= b < L:
                _plant(flat, i, b, BESIDE)
        f = far_tie_of(w, L, radius)
        if i % 3 == 2 and f is not None:
            _plant(flat, i, f, WIN)
    return flat.reshape(NDIR, ny, nx, L)


BASE = dict(zone=lr_zone, only_zone=lr_only_zone, two_sided=lr_two_sided)


def classes(radius, LPL=1):
    """{name: class of signature (seed, NDIR, ny, nx, L)} for a search of this radius on an instance of LPL labels per lane"""
    def bind(fn):
        return lambda seed, NDIR, ny, nx, L: fn(seed, NDIR, ny, nx, L, radius=radius, LPL=LPL)
    return {name: bind(fn) for name, fn in BASE.items()}


def all_classes(radius, LPL=1):
    """the classes of this module, then those of wta_crafted"""
    d = classes(radius, LPL)
    d.update(W.LR_CLASSES)
    return d


def pass_guard(lr, fill=f32(-1e30)):
    """the NDIR passes of any class, followed by 8 - NDIR passes of a finite, very small value: what a kernel that read a pass
    beyond NDIR would add.  The expectation uses the first NDIR passes alone."""
    NDIR = lr.shape[0]
    return np.concatenate([lr, np.full((8 - NDIR,) + lr.shape[1:], fill, np.float32)])


def lpl_of(L):
    """labels per lane of the streaming instance a stride of L runs on (1 for every stride the generic kernel takes)"""
    return L // 64 if L % 64 == 0 and L // 64 in (1, 2, 3, 4, 6, 8, 12, 16) else 1


# ---- the floors -------------------------------------------------------------------------------------------------------------
# Exact counts, by construction, of the model's maps (out2, cost2, out1, cost1 with dmin = 0) on S of the class.  `ok` marks the
# pixels whose plant survives: all of them without the over-count fix (or with one pass: f = 0 -- but 0 * INF = NaN under `ints`
# and `inf1`, so one pass with the fix counts as "with the fix"), the PLANTED ones with it.
#   zone       L >= 2 * radius + 4 and >= 14 pixels (at a smaller L position 1 or 3 may have no label beside the zone):
#              |o2 - o1| == radius + 1 on every ok pixel; without the fix each of the seven positions occurs at least twice.
#   only_zone  no ok pixel has a finite cost2, nor has any pixel with one finite label or none, fix or not (a non-finite S stays
#              non-finite under - f * C; on the other pixels the fix may move the winner off the zone's centre, and a label of
#              the zone then lies outside the new winner's); from 14 pixels on at least two ok pixels have a winner and at
#              least one pixel has none.
#   two_sided  on the ok pixels without the added tie whose lower candidate exists out2 < out1 (and out1 - out2 == radius + 1);
#              on the ok pixels with the added tie cost2 == cost1 and out2 > out1.
def ok_pixels(ny, nx, fix):
    i = np.arange(ny * nx).reshape(ny, nx)
    return W.PLANTED(i) if fix else np.ones((ny, nx), bool)


def floors(name, maps, ny, nx, L, radius, LPL, fix):
    o2, c2, o1, c1 = maps
    ok = ok_pixels(ny, nx, fix)
    npix = ny * nx
    if name == "zone" and L >= 2 * radius + 4 and npix >= 14:
        assert np.isfinite(c1[ok]).all() and np.isfinite(c2[ok]).all()
        assert (np.abs(o2[ok] - o1[ok]) == radius + 1).all(), (L, radius, LPL, fix)
        if not fix:
            assert (c1 == WIN).all() and (c2 == BESIDE).all()
            got = [winner_of(i, L, radius, LPL) for i in range(npix)]
            assert all(o1.ravel()[i] == w for i, (_, w) in enumerate(got))
            for k in range(NPOS):
                assert sum(1 for kk, _ in got if kk == k) >= 2, (k, L, radius, LPL)
    if name == "only_zone":
        none, one = only_zone_kinds(ny, nx)
        for m in (ok, none, one):
            assert not np.isfinite(c2[m]).any() and np.isnan(o2[m]).all()
        assert np.isnan(o1[none]).all() and np.isposinf(c1[none]).all()
        if npix >= 14:
            assert (np.isfinite(c1) & ok).sum() >= 2 and none.sum() >= 1
            assert np.isfinite(c1[ok & ~none]).all()
    if name == "two_sided" and L >= 2 * radius + 4:
        tied = two_sided_tied(ny, nx)
        for i in np.flatnonzero(ok.ravel()):
            _, w = winner_of(i, L, radius, LPL)
            a, b, ca, cb = o1.ravel()[i], o2.ravel()[i], c1.ravel()[i], c2.ravel()[i]
            if tied.ravel()[i] and far_tie_of(w, L, radius) is not None:
                assert ca == cb and b > a and {a, b} == {w, far_tie_of(w, L, radius)}, (i, w, a, b)
            elif w - radius - 1 >= 0:
                assert a == w and b == w - radius - 1 and b < a, (i, w, a, b)
            elif w + radius + 1 < L:
                assert a == w and b == w + radius + 1, (i, w, a, b)
