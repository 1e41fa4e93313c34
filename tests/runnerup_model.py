"""numpy model of the runner-up search and the uniqueness filter, float32 throughout.

    winner     o1 = first strict minimum among the finite entries of S(y, x, .) by rising o (mgm_core.cc:592-609)
               out1 = (float)(o1 + dmin), cost1 = S(o1);  NaN, +INF when no entry is finite
    runner-up  o2 = first strict minimum among the finite entries with |o - o1| > radius, by rising o
               out2 = (float)(o2 + dmin), cost2 = S(o2);  NaN, +INF without a winner or without such an entry
    conf       = 1.0f - cost1 / cost2   (one division, one subtraction; whatever IEEE gives)
    out        = NaN where conf < ratio, else d   (a NaN conf keeps d)
"""
import numpy as np

f32 = np.float32

# the pair and the options of the command-line test in test_gpu_wta_runnerup.py, and the ratio it filters with
# (test_runnerup_model.py checks on the oracle that this ratio rejects a visible part of the pixels, not all of them)
PAIR = dict(nx=96, ny=40, dmin=-16, dmax=0, NDIR=8, P1=8.0, P2=32.0, TSGM=4)
CLI_RATIO = 0.25
CLI_RADIUS = 1


def _first_min(masked, has, dmin):
    """(label, value, index) of the first of the equal minima of `masked` (+INF where an entry is no candidate)."""
    arg = np.argmin(masked, axis=-1)  # the first of equal minima = the first strict minimum
    out = np.where(has, (arg + dmin).astype(np.float32), f32(np.nan)).astype(np.float32)
    cost = np.where(has, np.take_along_axis(masked, arg[..., None], -1)[..., 0], f32(np.inf)).astype(np.float32)
    return out, cost, arg


def runnerup(S, dmin, radius):
    """S [ny][nx][L] over labels dmin..dmin+L-1 -> (out2, cost2, out1, cost1), float32 [ny][nx]."""
    S = np.asarray(S, np.float32)
    if radius < 0:
        raise ValueError("runner-up: radius must be >= 0")
    L = S.shape[-1]
    fin = np.isfinite(S)
    inf = f32(np.inf)
    has1 = fin.any(axis=-1)
    out1, cost1, o1 = _first_min(np.where(fin, S, inf), has1, dmin)
    o = np.arange(L).reshape((1,) * (S.ndim - 1) + (L,))
    far = fin & (np.abs(o - o1[..., None]) > radius) & has1[..., None]
    out2, cost2, _ = _first_min(np.where(far, S, inf), far.any(axis=-1), dmin)
    return out2, cost2, out1, cost1


def confidence(cost1, cost2):
    with np.errstate(all="ignore"):
        q = (np.asarray(cost1, np.float32) / np.asarray(cost2, np.float32)).astype(np.float32)
        return (f32(1) - q).astype(np.float32)


def uniqueness(d, cost1, cost2, ratio):
    """(out, conf), float32, of the two formulas above."""
    conf = confidence(cost1, cost2)
    with np.errstate(invalid="ignore"):
        out = np.where(conf < f32(ratio), f32(np.nan), np.asarray(d, np.float32)).astype(np.float32)
    return out, conf
