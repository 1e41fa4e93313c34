"""Development aid (runs on the GPU box): the speckle filter on the final left map of a bench workload (default: the headline
setting, 1920x1080x256, census 5x5, 8 directions, TSGM 3, FH), next to the other two post-processing steps on the same map.

    python tools/speckle_time.py [workload] [--runs 15] [--warmup 3] [--maxsize 100] [--maxdiff 1] [--out FILE.json]

One process, one context.  Both runs of the pair are aggregated once, the left map goes through the left-right test, and every
round then runs k_median (radius 1), k_leftright and k_speckle on that map, timed by the library's own device events
(mgm_timing_*: k_speckle brackets the call, its four kernels are listed inside it).  After the warm-up rounds: the median of
each, its spread, the split of k_speckle over its four launches, the ratio to k_median and the share of a pair's device time.
The only floor known in advance is the traffic: the map is read about three times and the two int32 planes a few times, about
100 MB at 1080p; anything above that is the latency of the finds and the atomics."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
import mgm_amd  # noqa: E402

PAIR_DEVICE_MS = 16.6  # a pair's device time at the headline setting, two runs
PHASES = ("k_speckle_local", "k_speckle_seams", "k_speckle_count", "k_speckle_apply")


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a[0]), max=float(a[-1]), iqr=float(q3 - q1), n=int(a.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maxsize", type=int, default=100)
    ap.add_argument("--maxdiff", type=float, default=1.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten runs each")
    w = bench.WORKLOADS[a.workload]
    nx, ny = w["nx"], w["ny"]
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
        spare, filtered, size_map = ctx.new_image(nx, ny), ctx.new_image(nx, ny), ctx.new_image(nx, ny)
        t = {k: [] for k in ("k_median", "k_leftright", "k_speckle") + PHASES}
        for k in range(a.warmup + a.runs):
            ctx.synchronize()
            ctx.timing(True)
            ctx.timing_reset()
            ctx.median_dev(final, 1, spare)
            ctx.leftright_dev(maps[0], maps[1], 1.0, spare)
            ctx.speckle_dev(final, a.maxsize, a.maxdiff, out=filtered)
            ctx.synchronize()
            tm = ctx.timings()
            ctx.timing(False)
            names = [n for n, _ in tm]
            assert all(names.count(n) == 1 for n in t), names
            if k >= a.warmup:
                for n in t:
                    t[n].append(dict(tm)[n])
        ctx.lib.mgm_speckle_dev(ctx.h, final.h, a.maxsize, a.maxdiff, None, size_map.h)
        d, f, s = final.download()[0], filtered.download()[0], size_map.download()[0]
    valid = np.isfinite(d)
    roots = int(np.sum(1.0 / s[valid].astype(np.float64)).round())  # every component's pixels sum to 1
    res = dict(workload=a.workload, nx=nx, ny=ny, maxsize=a.maxsize, maxdiff=a.maxdiff, warmup=a.warmup,
               valid_pixels=int(valid.sum()), components=roots, largest_component=int(s.max()),
               removed_pixels=int((valid & np.isnan(f)).sum()), **{n + "_ms": stats(ms) for n, ms in t.items()})
    res["ratio_to_k_median"] = res["k_speckle_ms"]["median"] / res["k_median_ms"]["median"]
    res["ratio_to_k_leftright"] = res["k_speckle_ms"]["median"] / res["k_leftright_ms"]["median"]
    res["share_of_pair_device_time"] = res["k_speckle_ms"]["median"] / PAIR_DEVICE_MS
    res["traffic_floor_MB"] = nx * ny * 4 * (3 + 1 + 8) / 1e6  # the map three times, out once, the planes about eight word accesses per pixel
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
