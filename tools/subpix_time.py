"""Development aid (runs on the GPU box): what sub-pixel label spacing costs at a bench workload (default: the headline
setting, 1920x1080x256, census 5x5, 8 directions, TSGM 3, FH).

    python tools/subpix_time.py [workload] [--runs 11] [--warmup 3] [--s 2 4] [--pair-s 2] [--out FILE.json]

One process, one context, everything timed with device events on the context's stream around calls that do not synchronise; medians
after the warm-up rounds, with the spread.  Per s:
  k_cv_interleave   the library's own timing row of the gather, next to a device-to-device hipMemcpyAsync of the bytes of F in the
                    form the gather left it in (the padded one-byte codes for census), in the same process, the two alternating.  The
                    kernel reads and writes exactly those bytes, so the copy is its ceiling: ratio = kernel / copy.
  the whole build   mgm_costvolume_build_subpix_dev against s ordinary builds of the same range into s kept volumes; the excess is
                    the phase kernels plus the gather.
For --pair-s (default 2): the device time of a pair -- both builds, both runs in one batched launch with vfit, the rescale, the
left-right test -- with the fine volumes against the same pair without them, alternating."""
import argparse
import ctypes as C
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


class Hip:
    """The few runtime calls the copy and the event pairs need."""

    def __init__(self, stream):
        self.lib = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            self.chk(self.lib.hipEventCreate(C.byref(e)))

    def chk(self, r):
        if r:
            raise RuntimeError("HIP runtime error %d" % r)

    def malloc(self, n):
        p = C.c_void_p()
        self.chk(self.lib.hipMalloc(C.byref(p), C.c_size_t(n)))
        return p

    def free(self, p):
        self.chk(self.lib.hipFree(p))

    def timed(self, fn):
        """milliseconds on the device between the events around fn's enqueues"""
        self.chk(self.lib.hipEventRecord(self.a, self.stream))
        fn()
        self.chk(self.lib.hipEventRecord(self.b, self.stream))
        self.chk(self.lib.hipEventSynchronize(self.b))
        ms = C.c_float()
        self.chk(self.lib.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return float(ms.value)

    def copy(self, dst, src, n):
        self.chk(self.lib.hipMemcpyAsync(dst, src, C.c_size_t(n), 3, self.stream))  # hipMemcpyDeviceToDevice


def padded(L):
    return next((lp for lp in (64, 128, 192, 256, 384, 512, 768, 1024) if lp >= L), 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--s", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--pair-s", type=int, default=2)
    ap.add_argument("--interp", default="cubic")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten runs each")
    w = bench.WORKLOADS[a.workload]
    nx, ny, dmin, dmax = w["nx"], w["ny"], w["dmin"], w["dmax"]
    cost, win = bench.cost_of(w), w["win"]
    L = dmax - dmin + 1
    res = dict(workload=a.workload, nx=nx, ny=ny, labels=L, cost=cost, win=win, interp=a.interp, warmup=a.warmup, s={})
    with mgm_amd.Context(0) as ctx:  # raises without a device: there is nothing to time on a CPU
        hip = Hip(ctx.stream_ptr())
        u, v, _ = bench.pair_of(w)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        build = lambda s, into: ctx.costvolume_subpix_dev(du, dv, dmin, dmax, s, a.interp, "none", cost, float("inf"), win, into=into)
        plain = lambda into: ctx.costvolume_dev(du, dv, dmin, dmax, "none", cost, float("inf"), win, into=into)
        for s in a.s:
            Lf = s * (L - 1) + 1
            codes = cost == "census" and padded(Lf) != 0
            fbytes = nx * ny * (padded(Lf) if codes else 4 * Lf)
            F = build(s, None)
            kept = [plain(None) for _ in range(s)]
            src, dst = hip.malloc(fbytes), hip.malloc(fbytes)
            t = dict(k_cv_interleave=[], k_subpix_phase=[], copy=[], build=[], plain_builds=[])
            for k in range(a.warmup + a.runs):
                ctx.synchronize()
                ctx.timing(True)
                ctx.timing_reset()
                tb = hip.timed(lambda: build(s, F))
                ctx.synchronize()
                tm = ctx.timings()
                ctx.timing(False)
                tc = hip.timed(lambda: hip.copy(dst, src, fbytes))
                tp = hip.timed(lambda: [plain(c) for c in kept])
                names = [n for n, _ in tm]
                assert names.count("k_cv_interleave") == 1 and names.count("k_subpix_phase") == s - 1, names
                if k >= a.warmup:
                    t["build"].append(tb), t["copy"].append(tc), t["plain_builds"].append(tp)
                    t["k_cv_interleave"].append(dict(tm)["k_cv_interleave"])
                    t["k_subpix_phase"].append(sum(ms for n, ms in tm if n == "k_subpix_phase"))
            r = {n + "_ms": stats(ms) for n, ms in t.items()}
            r.update(fine_labels=Lf, form="codes" if codes else "fp32", F_bytes=fbytes)
            r["interleave_to_copy"] = r["k_cv_interleave_ms"]["median"] / r["copy_ms"]["median"]
            r["interleave_GBps"] = 2 * fbytes / r["k_cv_interleave_ms"]["median"] / 1e6   # read + written
            r["copy_GBps"] = 2 * fbytes / r["copy_ms"]["median"] / 1e6
            r["build_excess_ms"] = r["build_ms"]["median"] - r["plain_builds_ms"]["median"]
            res["s"][str(s)] = r
            hip.free(src), hip.free(dst)
            for c in kept + [F]:
                c.free()
            ctx.trim()
        # ---- a pair's device time with and without the mode
        s = a.pair_s
        if s > 1:
            outs = [ctx.new_image(nx, ny) for _ in range(2)]
            costs = [ctx.new_image(nx, ny) for _ in range(2)]
            chk = ctx.new_image(nx, ny)
            vols = {1: [None, None], s: [None, None]}
            runs = ((du, dv, dmin, dmax), (dv, du, -dmax, -dmin))

            def pair(sp):
                for k, (x, y, lo, hi) in enumerate(runs):
                    vols[sp][k] = ctx.costvolume_subpix_dev(x, y, lo, hi, sp, a.interp, "none", cost, float("inf"), win, into=vols[sp][k])
                ctx.aggregate_batch_dev(vols[sp], w["P1"], w["P2"], w["NDIR"], w["MGM"], w["FH"], 1, None, "vfit", outs=outs, outcosts=costs)
                for o in outs:
                    ctx.subpix_scale_dev(o, sp, out=o)
                ctx.leftright_dev(outs[0], outs[1], 1.0, out=chk)

            t = {1: [], s: []}
            agg = {1: [], s: []}
            for k in range(a.warmup + a.runs):
                for sp in (1, s):
                    ctx.synchronize()
                    ctx.timing(True)
                    ctx.timing_reset()
                    ms = hip.timed(lambda: pair(sp))
                    ctx.synchronize()
                    tm = ctx.timings()
                    ctx.timing(False)
                    if k >= a.warmup:
                        t[sp].append(ms)
                        agg[sp].append(sum(x for n, x in tm if n.startswith("k_pass") or n.startswith("k_wta")))
            res["pair"] = dict(s=s, plain_ms=stats(t[1]), subpix_ms=stats(t[s]), plain_passes_and_search_ms=stats(agg[1]),
                               subpix_passes_and_search_ms=stats(agg[s]), kernel=ctx.last_pass_kernel())
            res["pair"]["ratio"] = res["pair"]["subpix_ms"]["median"] / res["pair"]["plain_ms"]["median"]
            res["pair"]["aggregation_ratio"] = res["pair"]["subpix_passes_and_search_ms"]["median"] / res["pair"]["plain_passes_and_search_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
