"""Development aid (runs on the GPU box): hole filling on the final left map of a bench workload (default: the headline setting,
1920x1080x256, census 5x5, 8 directions, TSGM 3, FH) after the left-right test and the speckle filter, next to k_median radius 1
and k_speckle on the same map -- and on a second map, the same one with every pixel NaN except the four corners.

    python tools/holes_time.py [workload] [--runs 15] [--warmup 3] [--mode median] [--dirs 8] [--maxdist 0] [--out FILE.json]

One process, one context.  Both runs of the pair are aggregated once, the left map goes through the left-right test and the
speckle filter (maxsize 100, maxdiff 1); every round then runs k_median (radius 1), k_speckle and k_holes on that map and k_holes
on the corners-only map, timed by the library's own device events (mgm_timing_*: k_holes brackets the call, its kernels are
listed inside it).  After the warm-up rounds: the median of each, its spread, the split of k_holes over its launches on both
maps side by side (the claim "the time does not depend on the holes" is those two columns), the ratios to k_median and k_speckle
and the share of a pair's device time.  The only floor known in advance is the traffic: the map is read about 1 + dirs times,
the candidate planes are written and read at holes, out is written once."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
import mgm_amd  # noqa: E402

PAIR_DEVICE_MS = 16.6  # a pair's device time at the headline setting, two runs
PHASES = ("k_holes_rows", "k_holes_carry", "k_holes_walk", "k_holes_apply")


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a[0]), max=float(a[-1]), iqr=float(q3 - q1), n=int(a.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", default="median")
    ap.add_argument("--dirs", type=int, default=8)
    ap.add_argument("--maxdist", type=int, default=0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten runs each")
    w = bench.WORKLOADS[a.workload]
    nx, ny = w["nx"], w["ny"]
    phases = PHASES if a.dirs > 2 else (PHASES[0], PHASES[3])
    with mgm_amd.Context(0) as ctx:  # raises without a device: there is nothing to time on a CPU
        u, v, _ = bench.pair_of(w)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        maps = []
        for a_, b_, lo, hi in ((du, dv, w["dmin"], w["dmax"]), (dv, du, -w["dmax"], -w["dmin"])):
            cv = ctx.costvolume_dev(a_, b_, lo, hi, "none", w.get("cost", "census"), float("inf"), w["win"])
            _, out, outc = ctx.aggregate_dev(cv, w["P1"], w["P2"], w["NDIR"], w["MGM"], w["FH"], 1, None, "vfit")
            maps.append(out)
            outc.free(), cv.free()
        ctx.trim()  # (the Lr workspace is not needed any more)
        final = ctx.leftright_dev(maps[0], maps[1], 1.0)
        ctx.speckle_dev(final, 100, 1.0, out=final)
        d = final.download()[0]
        corners = np.full((ny, nx), np.nan, np.float32)
        for y, x in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1)):
            corners[y, x] = d[y, x] if np.isfinite(d[y, x]) else 1.0
        dcorners = ctx.upload_image(corners)
        spare, out_map, out_corners, filled = (ctx.new_image(nx, ny) for _ in range(4))
        keys = ("k_median", "k_speckle", "k_holes") + phases
        t = {k: [] for k in keys + tuple("corners:" + n for n in ("k_holes",) + phases)}
        for k in range(a.warmup + a.runs):
            row = {}
            for tag, src, dst in (("", final, out_map), ("corners:", dcorners, out_corners)):
                ctx.synchronize()
                ctx.timing(True)
                ctx.timing_reset()
                if not tag:
                    ctx.median_dev(final, 1, spare)
                    ctx.speckle_dev(final, 100, 1.0, out=spare)
                ctx.fill_holes_dev(src, a.mode, a.dirs, a.maxdist, out=dst)
                ctx.synchronize()
                tm = ctx.timings()
                ctx.timing(False)
                names = [n for n, _ in tm]
                for n in (keys if not tag else ("k_holes",) + phases):
                    assert names.count(n) == 1, names
                    row[tag + n] = dict(tm)[n]
            if k >= a.warmup:
                for n in t:
                    t[n].append(row[n])
        ctx.lib.mgm_fill_holes_dev(ctx.h, final.h, a.mode.encode(), a.dirs, a.maxdist, None, filled.h)
        f, fc = filled.download()[0], out_corners.download()[0]
    hole = ~np.isfinite(d)
    res = dict(workload=a.workload, nx=nx, ny=ny, mode=a.mode, dirs=a.dirs, maxdist=a.maxdist, warmup=a.warmup,
               holes=int(hole.sum()), hole_share=float(hole.mean()), filled=int(f.sum()), corners_map_filled=int(np.isfinite(fc).sum() - 4),
               **{n + "_ms": stats(ms) for n, ms in t.items()})
    res["ratio_to_k_median"] = res["k_holes_ms"]["median"] / res["k_median_ms"]["median"]
    res["ratio_to_k_speckle"] = res["k_holes_ms"]["median"] / res["k_speckle_ms"]["median"]
    res["share_of_pair_device_time"] = res["k_holes_ms"]["median"] / PAIR_DEVICE_MS
    res["corners_to_map"] = res["corners:k_holes_ms"]["median"] / res["k_holes_ms"]["median"]
    # the map 1 + dirs times (the columns and diagonals twice: carry and walk), out once, the planes written and read at holes
    res["traffic_floor_MB"] = nx * ny * 4 * (1 + a.dirs + max(a.dirs - 2, 0) + 1 + 2 * a.dirs * res["hole_share"]) / 1e6
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
