"""Development aid (runs on the GPU box): the consensus votes against the plain winner search at a bench workload
(default: the headline volume, 1920x1080x256, census 5x5, 8 directions, TSGM 3, FH -- k_wta_consensus<4,3,8> against k_wta; with
`cfg3r`, its range images of 49 labels per pixel, k_wta_consensus_rel<4> against k_wta_rel).

    python tools/consensus_time.py [workload] [--runs 15] [--warmup 3] [--processes 3] [--tol 1] [--out FILE.json]

Every process is a fresh child with one context.  Every round aggregates the volume (MGM_HIP_WTA_PRUNE=0, refinement none: the
call's own search is the plain k_wta / k_wta_rel) and then counts the votes for that call's map over the same Lr volumes, so the
two kernels alternate; both are timed by the library's own device events (mgm_timing_*).  After the warm-up rounds: the median of
each, its spread (min, max, the interquartile range) and the ratio of the medians, per process, and the median of the ratios.  The
votes kernel reads the same NDIR * Lk * 4 bytes per pixel as the search and no costs, so the yardstick is the search in the same
process, not a fixed number.  Only the instance that ran here may be called measured."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ["MGM_HIP_WTA_PRUNE"] = "0"  # (read by the library at every call)


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a[0]), max=float(a[-1]), iqr=float(q3 - q1), n=int(a.size))


def one_process(a):
    import bench
    import mgm_amd
    w = bench.WORKLOADS[a.workload]
    L = bench.labels_of(w)
    nx, ny = w["nx"], w["ny"]
    with mgm_amd.Context(0) as ctx:  # raises without a device: there is nothing to time on a CPU
        u, v, gt = bench.pair_of(w)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        if w.get("ragged"):
            g = gt.astype(np.float32)
            lo = ctx.upload_image(np.clip(g - w["ragged"], w["dmin"], w["dmax"])[None])
            hi = ctx.upload_image(np.clip(g + w["ragged"], w["dmin"], w["dmax"])[None])
            cv = ctx.costvolume_ranged_dev(du, dv, lo, hi, w["dmin"], w["dmax"], "none", w.get("cost", "census"), float("inf"), w["win"])
        else:
            cv = ctx.costvolume_dev(du, dv, w["dmin"], w["dmax"], "none", w.get("cost", "census"), float("inf"), w["win"])
        out, outc, votes = ctx.new_image(nx, ny), ctx.new_image(nx, ny), ctx.new_image(nx, ny)
        t_wta, t_cs, fam = [], [], set()
        for k in range(a.warmup + a.runs):
            ctx.synchronize()
            ctx.timing(True)
            ctx.timing_reset()
            ctx.aggregate_dev(cv, w["P1"], w["P2"], w["NDIR"], w["MGM"], w["FH"], 1, None, None, out, outc)
            ctx.wta_consensus_dev(cv, w["NDIR"], out, a.tol, votes=votes)
            ctx.synchronize()
            t = ctx.timings()
            ctx.timing(False)
            names = [n for n, _ in t]
            assert names.count("k_wta") == 1 and names.count("k_wta_consensus") == 1 and "k_wta_pruned" not in names, names
            fam |= {n for n in names if n.startswith("k_wta_consensus_")}
            if k >= a.warmup:
                t_wta.append(dict(t)["k_wta"])
                t_cs.append(dict(t)["k_wta_consensus"])
        vt = votes.download()[0]
        hist = np.bincount(vt.astype(int).ravel(), minlength=w["NDIR"] + 1).tolist()
    slots = None
    if "k_wta_consensus_rel" in fam:
        slots = 64 if 2 * w["ragged"] + 1 <= 62 else 128
    res = dict(workload=a.workload, nx=nx, ny=ny, labels=L, NDIR=w["NDIR"], tol=a.tol, warmup=a.warmup, family=sorted(fam), rel_slots=slots,
               k_wta_ms=stats(t_wta), k_wta_consensus_ms=stats(t_cs), votes_histogram=hist)
    res["ratio_of_medians"] = res["k_wta_consensus_ms"]["median"] / res["k_wta_ms"]["median"]
    gb = nx * ny * (slots or L) * 4 * w["NDIR"] / 1e9  # Lr of every pass, read once (the search reads the cost codes besides)
    res["lr_read_GB"] = gb
    res["k_wta_consensus_TBps"] = gb / res["k_wta_consensus_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--tol", type=float, default=1.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten runs each")
    if a.child:
        print(json.dumps(one_process(a)))
        return 0
    per = []
    for _ in range(a.processes):  # (fresh children, one after the other: this process never opens the device)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), a.workload, "--runs", str(a.runs), "--warmup", str(a.warmup), "--tol", repr(a.tol), "--child"],
                           stdout=subprocess.PIPE, text=True, timeout=600)
        if r.returncode:
            return r.returncode
        per.append(json.loads(r.stdout.strip().splitlines()[-1]))
    res = dict(processes=per, ratio_median_of_processes=float(np.median([p["ratio_of_medians"] for p in per])))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
