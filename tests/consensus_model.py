"""numpy model of the consensus votes and the consensus filter, float32 throughout.

    pass winner  w_p = first strict minimum, by rising label, among the finite entries of Lr_p(y, x, .) over the labels the pixel
                 owns: all L of a dense volume, lo(y, x)..hi(y, x) (label INDICES, clipped to the volume) of a ragged one;
                 equal values (-0 / +0 included) go to the smaller label; no finite entry: no winner
    vote         w_p exists and fabsf((float)(w_p + dmin) - d) <= tol   (one float subtraction: a NaN or infinite d gets none)
    votes        = (float) number of voting passes among the first NDIR; winners[p] = (float)(w_p + dmin), NaN without a winner
    filter       out = NaN where votes < (float)minvotes, else d
"""
import numpy as np

f32 = np.float32

# the command-line test's filter on runnerup_model.PAIR (test_consensus_model.py checks on the oracle that it rejects a visible
# part of the pixels, not all of them)
CLI_MIN = 6
CLI_TOL = 1.0


def owned(shape, lo=None, hi=None):
    """bool [ny][nx][L]: the labels a pixel owns; lo / hi are label indices [ny][nx] (inclusive), None: all"""
    ny, nx, L = shape
    o = np.arange(L).reshape(1, 1, L)
    m = np.ones((ny, nx, L), bool)
    if lo is not None:
        m &= (o >= np.asarray(lo).reshape(ny, nx, 1)) & (o <= np.asarray(hi).reshape(ny, nx, 1))
    return m


def pass_winners(lr, NDIR, lo=None, hi=None):
    """lr [n >= NDIR][ny][nx][L] -> (w int64 [NDIR][ny][nx], has bool [NDIR][ny][nx]); w is arbitrary where has is False"""
    lr = np.asarray(lr, np.float32)[:NDIR]
    assert lr.shape[0] == NDIR
    cand = np.isfinite(lr) & owned(lr.shape[1:], lo, hi)[None]
    masked = np.where(cand, lr, f32(np.inf))
    return np.argmin(masked, axis=-1), cand.any(axis=-1)  # (argmin: the first of equal minima, and -0 == +0)


def consensus(lr, dmin, NDIR, d, tol, lo=None, hi=None):
    """(votes [ny][nx], winners [NDIR][ny][nx]), float32.  d None: votes is None."""
    if not (np.isfinite(tol) and tol >= 0):
        raise ValueError("consensus: tol must be finite and >= 0")
    w, has = pass_winners(lr, NDIR, lo, hi)
    lab = (w + dmin).astype(np.float32)
    winners = np.where(has, lab, f32(np.nan)).astype(np.float32)
    if d is None:
        return None, winners
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        vote = has & (np.abs((lab - d[None]).astype(np.float32)) <= f32(tol))
    return vote.sum(axis=0).astype(np.float32), winners


def consensus_filter(d, votes, minvotes):
    if minvotes < 0:
        raise ValueError("consensus filter: minvotes must be >= 0")
    with np.errstate(invalid="ignore"):
        return np.where(np.asarray(votes, np.float32) < f32(minvotes), f32(np.nan), np.asarray(d, np.float32)).astype(np.float32)
