"""Development aid (runs on the GPU box): the runner-up search against the plain winner search at a bench workload (default:
the headline volume, 1920x1080x256, census 5x5, 8 directions, TSGM 3, FH).

    python tools/runnerup_time.py [workload] [--runs 15] [--warmup 3] [--radius 1] [--no-first] [--out FILE.json]

One process, one context.  Every round aggregates the volume (MGM_HIP_WTA_PRUNE=0, refinement none: the call's own search is
the plain k_wta) and then searches the same Lr volumes for the runner-up, so the two kernels alternate; both are timed by
the library's own device events (mgm_timing_*).  After the warm-up rounds: the median of each, its spread (min, max, the
interquartile range) and the ratio of the medians.  By bytes the two are equal -- the same reads, 16 against 8 bytes written
per pixel beside ~9 KB read -- so the yardstick is k_wta in the same run, not a fixed number.  --no-first: the search writes
the runner-up's two maps only (8 bytes per pixel, as k_wta does)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ["MGM_HIP_WTA_PRUNE"] = "0"  # (read by the library at every call)
import bench  # noqa: E402
import mgm_amd  # noqa: E402


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a[0]), max=float(a[-1]), iqr=float(q3 - q1), n=int(a.size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--no-first", action="store_true", help="out1 / cost1 are not asked for")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten runs each")
    w = bench.WORKLOADS[a.workload]
    L = bench.labels_of(w)
    with mgm_amd.Context(0) as ctx:  # raises without a device: there is nothing to time on a CPU
        u, v, _ = bench.pair_of(w)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        cv = ctx.costvolume_dev(du, dv, w["dmin"], w["dmax"], "none", w.get("cost", "census"), float("inf"), w["win"])
        nx, ny = w["nx"], w["ny"]
        out, outc = ctx.new_image(nx, ny), ctx.new_image(nx, ny)
        o2, c2 = ctx.new_image(nx, ny), ctx.new_image(nx, ny)
        t_wta, t_ru = [], []
        for k in range(a.warmup + a.runs):
            ctx.synchronize()
            ctx.timing(True)
            ctx.timing_reset()
            ctx.aggregate_dev(cv, w["P1"], w["P2"], w["NDIR"], w["MGM"], w["FH"], 1, None, None, out, outc)
            imgs = ctx.wta_runnerup_dev(cv, w["NDIR"], 1, a.radius, o2, c2, want_first=not a.no_first)
            ctx.synchronize()
            t = ctx.timings()
            ctx.timing(False)
            for im in imgs[2:]:
                if im is not None:
                    im.free()
            names = [n for n, _ in t]
            assert names.count("k_wta") == 1 and names.count("k_wta_runnerup") == 1 and "k_wta_pruned" not in names, names
            if k >= a.warmup:
                t_wta.append(dict(t)["k_wta"])
                t_ru.append(dict(t)["k_wta_runnerup"])
        # the two searches agree on the winner (refinement none: out is the winner's label)
        o2_, c2_, o1, c1 = ctx.wta_runnerup_dev(cv, w["NDIR"], 1, a.radius, o2, c2)
        ctx.aggregate_dev(cv, w["P1"], w["P2"], w["NDIR"], w["MGM"], w["FH"], 1, None, None, out, outc)
        same = bool(np.array_equal(out.download(), o1.download(), equal_nan=True) and np.array_equal(outc.download(), c1.download(), equal_nan=True))
    res = dict(workload=a.workload, nx=nx, ny=ny, labels=L, NDIR=w["NDIR"], radius=a.radius, warmup=a.warmup, maps_written=2 if a.no_first else 4,
               k_wta_ms=stats(t_wta), k_wta_runnerup_ms=stats(t_ru), winner_agrees=same)
    res["ratio_of_medians"] = res["k_wta_runnerup_ms"]["median"] / res["k_wta_ms"]["median"]
    gb = nx * ny * (L * (4 * w["NDIR"] + 1)) / 1e9  # Lr of every pass + one-byte costs, read once
    res["read_GB"] = gb
    res["k_wta_TBps"] = gb / res["k_wta_ms"]["median"]
    res["k_wta_runnerup_TBps"] = gb / res["k_wta_runnerup_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
