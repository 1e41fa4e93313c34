"""Window statistics of the coarse-to-fine mode, from the numpy model on the CPU (no device): per level the distribution of
window widths, how windows nest along a scan line, and how full the 64-slot records of the range-proportional layout are.

    python tools/multiscale_stats.py [nscales ...]       (fountain23 of tests/golden, census 5x5, 8 directions, TSGM 4, vfit)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import multiscale_model as msm  # noqa: E402
from oracle import oracle as orc_mod  # noqa: E402


def main():
    scales = [int(a) for a in sys.argv[1:]] or [1, 2, 3, 4]
    d = np.load(os.path.join(ROOT, "tests", "golden", "cfg1_fountain23.npz"))
    u = np.ascontiguousarray(d["uL"].astype(np.float32).transpose(2, 0, 1))
    v = np.ascontiguousarray(d["uR"].astype(np.float32).transpose(2, 0, 1))
    orc = orc_mod.Oracle(threads=orc_mod.usable_cpus(16))
    kw = dict(P1=24.0, P2=96.0, NDIR=8, TSGM=4, distance="census", census_win=5, refine="vfit")
    one = None
    for S in scales:
        r = msm.multiscale_pair(orc, u, v, -120, 30, S, **kw)
        if S == 1:
            one = r["outL"]
        both = np.isfinite(r["outL"]) & np.isfinite(one) if one is not None else None
        close = float(np.mean(np.abs(r["outL"][both] - one[both]) <= 1)) if both is not None else float("nan")
        print("S=%d  valid %.3f  within 1 px of S=1 (both valid) %.3f" % (S, np.isfinite(r["outL"]).mean(), close))
        for s, lv in enumerate(r["levels"]):
            lo, hi = orc_mod.int_ranges(*lv["ranges"][0])
            w = (hi - lo + 1).astype(np.int64)
            q = np.percentile(w, [50, 90, 99])
            same = (lo[:, 1:] == lo[:, :-1]) & (hi[:, 1:] == hi[:, :-1])
            contains = (lo[:, 1:] <= lo[:, :-1]) & (hi[:, 1:] >= hi[:, :-1])
            slots = 64 if w.max() <= 62 else 128  # (one format per volume)
            print("   level %d %4dx%-4d  width mean %.1f median %d p90 %d p99 %d max %d | <=16: %.2f <=30: %.2f <=62: %.2f <=126: %.2f | "
                  "equals left neighbour's %.2f, contains it %.2f | share of the %d-slot records occupied %.2f (if 32 slots were enough for <=30: %.2f of pixels)"
                  % (s, lv["dims"][0], lv["dims"][1], w.mean(), q[0], q[1], q[2], w.max(), np.mean(w <= 16), np.mean(w <= 30), np.mean(w <= 62),
                     np.mean(w <= 126), same.mean(), contains.mean(), slots, float(w.mean()) / slots, np.mean(w <= 30)))


if __name__ == "__main__":
    main()
