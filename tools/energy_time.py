"""Development aid (runs on the GPU box): the solution energy on the unrefined left map of a bench workload
(default: the headline setting, 1920x1080x256, census 5x5, 8 directions, TSGM 3, FH), next to k_median radius 1 on the same map and
a device-to-device copy of one map.

    python tools/energy_time.py [workload] [--runs 15] [--warmup 3] [--out FILE.json]

One process, one context.  The volume is built (one-byte census codes: the copy k_energy reads) and aggregated once without a
refinement; every round then runs k_median (radius 1), k_energy of kind 0 (truncated L1) and of kind 3 (8 neighbours, the weight
image of mgm_weights_dev), both writing their map and their partials, and the copy, all on the context's stream.  The kernels are
timed by the library's own device events (mgm_timing_*), the copy by an event pair of its own.  After the warm-up rounds: the median
of each, its spread, and the ratios.  The totals' host part (two downloads, two sums) is not in these numbers: it is timed once, by
the host clock, around a call that asks for them.  The floor known in advance is the traffic: d read about once from HBM (its
neighbours come from the caches), E written, kind 3's eight weight planes read, and one 64-byte sector of the volume per pixel."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
import mgm_amd  # noqa: E402

PAIR_DEVICE_MS = 16.6  # a pair's device time at the headline setting, two runs


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    q1, q3 = np.percentile(a, [25, 75])
    return dict(median=float(np.median(a)), min=float(a[0]), max=float(a[-1]), iqr=float(q3 - q1), n=int(a.size))


class Hip:
    """The few runtime calls the copy and its event pair need."""

    def __init__(self, stream):
        self.lib = C.CDLL("libamdhip64.so")
        self.stream = C.c_void_p(stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            self.chk(self.lib.hipEventCreate(C.byref(e)))

    def chk(self, r):
        if r:
            raise RuntimeError("HIP runtime error %d" % r)

    def timed_copy(self, dst, src, n):
        self.chk(self.lib.hipEventRecord(self.a, self.stream))
        self.chk(self.lib.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(n), 3, self.stream))  # hipMemcpyDeviceToDevice
        self.chk(self.lib.hipEventRecord(self.b, self.stream))
        self.chk(self.lib.hipEventSynchronize(self.b))
        ms = C.c_float()
        self.chk(self.lib.hipEventElapsedTime(C.byref(ms), self.a, self.b))
        return float(ms.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", nargs="?", default="cfg3")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs: at least ten runs each")
    w = bench.WORKLOADS[a.workload]
    nx, ny = w["nx"], w["ny"]
    with mgm_amd.Context(0) as ctx:  # raises without a device: there is nothing to time on a CPU
        hip = Hip(ctx.stream_ptr())
        u, v, _ = bench.pair_of(w)
        du, dv = ctx.upload_image(u), ctx.upload_image(v)
        cv = ctx.costvolume_dev(du, dv, w["dmin"], w["dmax"], "none", w.get("cost", "census"), float("inf"), w["win"])
        _, d, dc = ctx.aggregate_dev(cv, w["P1"], w["P2"], w["NDIR"], w["MGM"], w["FH"], 1, None, None)
        w8 = ctx.weights_dev(du, 4.0, 12.0)
        ctx.trim()  # (the Lr workspace is not needed any more)
        spare, E0, E3 = (ctx.new_image(nx, ny) for _ in range(3))
        q0 = mgm_amd.EnergyParams(0, w["P1"], w["P2"], 4, 0, None)
        q3 = mgm_amd.EnergyParams(3, w["P1"], w["P2"], 8, w["FH"], w8.h)
        tot = mgm_amd.EnergyTotals()
        ptr = lambda im: ctx.lib.mgm_img_device_ptr(im.h)
        t = dict(k_median=[], k_energy_kind0=[], k_energy_kind3=[], copy=[])
        for k in range(a.warmup + a.runs):
            ctx.synchronize()
            ctx.timing(True)
            ctx.timing_reset()
            ctx.median_dev(d, 1, spare)
            # (with totals: the launch that also writes the partials; the call's downloads are behind the kernel's events)
            ctx._chk(ctx.lib.mgm_energy_dev(ctx.h, cv.h, d.h, C.byref(q0), E0.h, C.byref(tot)))
            ctx._chk(ctx.lib.mgm_energy_dev(ctx.h, cv.h, d.h, C.byref(q3), E3.h, C.byref(tot)))
            ctx.synchronize()
            tm = ctx.timings()
            ctx.timing(False)
            tc = hip.timed_copy(ptr(spare), ptr(d), nx * ny * 4)
            names = [n for n, _ in tm]
            assert names.count("k_energy") == 2 and names.count("k_median") == 1 and "k_expand" not in names, names
            en = [ms for n, ms in tm if n == "k_energy"]
            if k >= a.warmup:
                t["k_median"].append(dict(tm)["k_median"]), t["k_energy_kind0"].append(en[0]), t["k_energy_kind3"].append(en[1]), t["copy"].append(tc)
        host = []
        for _ in range(5):  # the whole call with totals by the host clock: launch, two downloads, the two sums
            ctx.synchronize()
            t0 = time.perf_counter()
            ctx._chk(ctx.lib.mgm_energy_dev(ctx.h, cv.h, d.h, C.byref(q3), None, C.byref(tot)))
            host.append((time.perf_counter() - t0) * 1e3)
        totals = {f: getattr(tot, f) for f, _ in mgm_amd.EnergyTotals._fields_}
    res = dict(workload=a.workload, nx=nx, ny=ny, labels=bench.labels_of(w), warmup=a.warmup, totals_kind3=totals,
               call_with_totals_host_ms=stats(host), **{n + "_ms": stats(ms) for n, ms in t.items()})
    for n in ("k_energy_kind0", "k_energy_kind3"):
        res[n + "_to_k_median"] = res[n + "_ms"]["median"] / res["k_median_ms"]["median"]
        res[n + "_to_copy"] = res[n + "_ms"]["median"] / res["copy_ms"]["median"]
        res[n + "_share_of_pair_device_time"] = res[n + "_ms"]["median"] / PAIR_DEVICE_MS
    # d once, E once, the partials; kind 3: eight weight planes; one 64-byte sector of cost codes per pixel
    res["traffic_floor_MB"] = dict(kind0=nx * ny * (4 + 4 + 64) / 1e6, kind3=nx * ny * (4 + 4 + 32 + 64) / 1e6)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f_:
            f_.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
