"""Crafted Lr volumes and maps for the consensus votes: what tests/test_consensus_model.py pins on the CPU and
tests/test_gpu_wta_consensus_crafted.py writes over the context's own pass volumes.

    votes       integers 0..3 in every pass; pixel i has a base label b_i that walks over label 0, label L-1, the two labels at the
                first lane boundary of an instance of LPL labels per lane, the two at the boundary in the middle, and two labels
                in between; pass p holds -8 at b_i + OFF[(i + p) % 8], OFF = 0 0 +1 -1 +2 -2 +3 -3 (clipped to the volume), so the
                passes' winners spread over both edges of every tolerance zone; on the pixels i % 4 == 1 a second label holds -8
                too: the next label, the label LPL further (another lane), or the label half the range away -- two equal minima,
                the smaller label wins
    the classes of tests/wta_crafted.py, each pass taken alone: ties, NaN, +-INF, -0 / +0, negative, denormal and overflowing
                values, flat pixels, and passes without a finite entry (`nolabel`)

The maps to judge (`d_maps`): pass 0's winner shifted per pixel by 0, +-0.5, +-1, 1.5, +-2.5, 3, 0.25 (a shift EQUAL to a tolerance
of 0.5, 1 or 2.5 sits on the zone's edge: <= votes, < does not; a half shift tells a comparison in float from one on a truncated
map), NaN, +INF, -INF and 1e30; and the base label itself.

`full` lays a class into what a kernel sees: the label stride Lk with `poison` in the padding slots L..Lk-1 and on the labels a
pixel does not own, and behind the NDIR passes more passes of a finite, very small value.
"""
import numpy as np

import runnerup_crafted as R
import wta_crafted as W

f32 = np.float32
TOLS = (0.0, 0.5, 1.0, 2.5)
OFF = (0, 0, 1, -1, 2, -2, 3, -3)
SHIFTS = (0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.5, -2.5, 3.0, 0.25, np.nan, np.inf, -np.inf, 1e30)
POISON = f32(-1e30)


def positions(L, LPL):
    mid = max(LPL, (L // 2 // LPL) * LPL)
    cand = (0, L - 1, LPL - 1, LPL, mid - 1, mid, L // 3, (2 * L) // 3)
    return [c for c in dict.fromkeys(cand) if 0 <= c < L]


def base_labels(ny, nx, L, LPL):
    pos = positions(L, LPL)
    i = np.arange(ny * nx)
    return np.array(pos)[(i + i // len(pos)) % len(pos)]


def lr_votes(seed, NDIR, ny, nx, L, LPL=1):
    rng = np.random.default_rng(seed)
    n = ny * nx
    lr = rng.integers(0, 4, (NDIR, n, L)).astype(np.float32)
    b = base_labels(ny, nx, L, LPL)
    for i in range(n):
        for p in range(NDIR):
            w = int(np.clip(b[i] + OFF[(i + p) % 8], 0, L - 1))
            lr[p, i, w] = -8
            if i % 4 == 1 and L > 1:
                kind = (i // 4 + p) % 3
                t = w + (1, LPL, L // 2)[kind]
                if t >= L:
                    t = w - (1, LPL, L // 2)[kind]
                if 0 <= t < L:
                    lr[p, i, t] = -8
    return lr.reshape(NDIR, ny, nx, L)


def classes(LPL=1):
    """{name: class of signature (seed, NDIR, ny, nx, L)}: `votes`, then those of wta_crafted"""
    d = {"votes": lambda seed, NDIR, ny, nx, L: lr_votes(seed, NDIR, ny, nx, L, LPL)}
    d.update(W.LR_CLASSES)
    return d


def d_maps(winner0, base, dmin):
    """{name: d [ny][nx] float32}: pass 0's winner (NaN where it has none) shifted per pixel, and the base label as it is"""
    ny, nx = winner0.shape
    i = np.arange(ny * nx)
    with np.errstate(invalid="ignore", over="ignore"):
        shifted = (winner0.ravel() + np.array(SHIFTS, np.float32)[(i + i // len(SHIFTS)) % len(SHIFTS)]).astype(np.float32)
    return {"shifted": shifted.reshape(ny, nx), "base": (np.asarray(base).reshape(ny, nx) + dmin).astype(np.float32)}


def windows(seed, ny, nx, L, wmin=3, wmax=40):
    """label-index zones (lo, hi) [ny][nx], 3..40 labels wide somewhere in the volume; pixel 0 at its low end, the last at its high end"""
    rng = np.random.default_rng(seed)
    n = ny * nx
    w = np.minimum(rng.integers(wmin, wmax + 1, n), L)
    lo = rng.integers(0, L - w + 1)
    lo[0] = 0
    lo[-1] = L - w[-1]
    return lo.reshape(ny, nx), (lo + w - 1).reshape(ny, nx)


def lay_in_windows(fn, seed, NDIR, ny, nx, L, lo, hi):
    """the class generated per pixel at the width of its own zone and laid there (what it plants lands inside the zone); elsewhere
    the class at the volume's width -- `full` poisons it"""
    dense = fn(seed + 1000, NDIR, ny, nx, L).reshape(NDIR, ny * nx, L)
    lo_, w_ = np.ravel(lo), np.ravel(hi - lo + 1)
    for w in np.unique(w_):
        gen = fn(seed, NDIR, ny, nx, int(w)).reshape(NDIR, ny * nx, int(w))
        for p in np.nonzero(w_ == w)[0]:
            dense[:, p, lo_[p]:lo_[p] + w] = gen[:, p, :]
    return dense.reshape(NDIR, ny, nx, L)


def full(lr, Lk=None, lo=None, hi=None, poison=POISON, guard=True):
    """[8 or NDIR][ny][nx][Lk] as a kernel sees the class: poison in the padding slots and on the unowned labels, R.pass_guard's
    passes behind"""
    lr = np.asarray(lr, np.float32)
    NDIR, ny, nx, L = lr.shape
    Lk = Lk or L
    out = np.full((NDIR, ny, nx, Lk), poison, np.float32)
    out[..., :L] = lr
    if lo is not None:
        o = np.arange(Lk).reshape(1, 1, 1, Lk)
        out = np.where((o >= lo[None, ..., None]) & (o <= hi[None, ..., None]), out, f32(poison)).astype(np.float32)
    return R.pass_guard(out) if guard else out
