"""Development aid (runs on the GPU box): hole classification and the classified fill on the final left map of a bench workload
(default: the headline setting, 1920x1080x256, census 5x5, 8 directions, TSGM 3, FH) after the left-right test and the speckle
filter -- tools/holes_time.py's map -- next to the plain k_holes on the same map in the same process.

    python tools/occlusion_time.py [workload] [--runs 15] [--warmup 3] [--occ sechigh] [--mis median] [--dirs 8] [--out FILE.json]

One process, one context.  Both runs of the pair are aggregated once; the left map goes through the left-right test and the speckle
filter (maxsize 100, maxdiff 1), the right map stays as it entered that test.  Every round runs mgm_fill_holes_dev (the plain
k_holes), mgm_classify_holes_dev (k_holes_classify, over the workload's range at tau 1) and mgm_fill_holes_classified_dev (k_holes
with the classified apply phase), each timed by the library's own device events.  After the warm-up rounds: the median of each, its
spread, the ratios, the classes' counts."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
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
    ap.add_argument("--occ", default="sechigh")
    ap.add_argument("--mis", default="median")
    ap.add_argument("--dirs", type=int, default=8)
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
        ctx.speckle_dev(final, 100, 1.0, out=final)
        other = maps[1]
        cls, out_plain, out_cls = (ctx.new_image(nx, ny) for _ in range(3))
        t = {"k_holes": [], "k_holes_classify": [], "k_holes(classified)": [], "k_holes_apply": [], "k_holes_apply(classified)": []}

        def timed(fn):
            ctx.synchronize()
            ctx.timing(True)
            ctx.timing_reset()
            fn()
            ctx.synchronize()
            tm = dict(ctx.timings())
            ctx.timing(False)
            return tm

        for k in range(a.warmup + a.runs):
            plain = timed(lambda: ctx.fill_holes_dev(final, a.mis, a.dirs, 0, out=out_plain))
            cl = timed(lambda: ctx.classify_holes_dev(final, other, w["dmin"], w["dmax"], 1.0, cls=cls))
            fc = timed(lambda: ctx.fill_holes_classified_dev(final, cls, a.occ, a.mis, a.dirs, 0, out=out_cls))
            if k >= a.warmup:
                t["k_holes"].append(plain["k_holes"])
                t["k_holes_apply"].append(plain["k_holes_apply"])
                t["k_holes_classify"].append(cl["k_holes_classify"])
                t["k_holes(classified)"].append(fc["k_holes"])
                t["k_holes_apply(classified)"].append(fc["k_holes_apply"])
        d, c, o1, o2 = final.download()[0], cls.download()[0], out_plain.download()[0], out_cls.download()[0]
    hole = ~np.isfinite(d)
    res = dict(workload=a.workload, nx=nx, ny=ny, dmin=w["dmin"], dmax=w["dmax"], tau=1.0, occ=a.occ, mis=a.mis, dirs=a.dirs, warmup=a.warmup,
               holes=int(hole.sum()), hole_share=float(hole.mean()), occlusions=int((c == 1).sum()), mismatches=int((c == 2).sum()),
               differ_from_plain=int((o1.view(np.uint32) != o2.view(np.uint32)).sum()), **{n + "_ms": stats(ms) for n, ms in t.items()})
    res["classify_to_k_holes"] = res["k_holes_classify_ms"]["median"] / res["k_holes_ms"]["median"]
    res["classified_to_k_holes"] = res["k_holes(classified)_ms"]["median"] / res["k_holes_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
