"""k_pass_exact (mgm_pass_exact.hip), the NaN-faithful pass kernel, on the cases of tests/exact_crafted.py: volumes that hold NaNs
and stay mostly finite -- six cost classes under one NaN recipe, the four update functions x NDIR 1, 3, 4, 8, 1 to 8193 labels
(lane-chunks of 1, 2, 3, 5 labels; FH's arrays in the LDS and in global scratch), odd penalties and weights, images without an
updated pixel, a batch of three, ragged volumes with P2 = +INF, a negative FH slope or an odd weight, and four `zsign` volumes on
which the slab minimum's tie rule (the first of +0 / -0 is kept) decides thousands of words.

Compared bit for bit (NaN = NaN) with the CPU oracle, which tests/test_exact_crafted_ref.py pins on the compiled reference for the
same cases: the Lr volume of EVERY pass (the sum over the passes is NaN almost everywhere, see exact_crafted.py), S, the cost map
and the labels where the cost is finite.  Each case runs twice on the shared context.

Every case is proved on the host to take k_pass_exact before anything is uploaded (exact_crafted.must_take_exact): the other pass
kernels wait for each other through polled tags and are not made for these values.  After each call the context must name
k_pass_exact and the timing table no other pass kernel.  Once a device call has raised, nothing more of this file runs."""
import ctypes as C

import numpy as np
import pytest

import exact_crafted as X
import mgm_amd
from helpers import labels_equal, ndiff

pytestmark = pytest.mark.gpu

RAISED = []  # the case whose device call raised: the rest of the file is not run after it


def lr_of(ctx, cv, volume, p, shape):
    """pass p of volume `volume` of the last call: volume 0 through mgm_debug_download_lr, the others from where they lie"""
    if volume == 0:
        return ctx.debug_lr(cv, p)
    got = ctx.debug_lr_ptr(volume, p)
    assert got, "mgm_debug_lr_device_ptr(%d, %d) is null" % (volume, p)
    ptr, Lk, _ = got
    ny, nx, L = shape
    # hipMemcpy looked up THROUGH the library's own handle: dlsym on it searches the library and what it was linked against, so
    # the copy goes through the very runtime instance that owns the pointer, whatever other copy of the runtime is on the path
    hip_memcpy = ctx.lib.hipMemcpy
    hip_memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip_memcpy.restype = C.c_int
    buf = np.empty((ny, nx, Lk), np.float32)
    ctx.synchronize()
    assert hip_memcpy(buf.ctypes.data, ptr, buf.nbytes, 2) == 0  # hipMemcpyDeviceToHost
    return np.ascontiguousarray(buf[:, :, :L])


def run_once(ctx, case, built, cvs, w8d):
    """one aggregation call -> per volume (S, labels, cost map), with the route asserted"""
    ctx.synchronize()
    ctx.timing(True)
    ctx.timing_reset()
    try:
        if case.kind == "batch":
            Ss, outs, outcs = ctx.aggregate_batch_dev(cvs, case.P1, case.P2, case.NDIR, case.MGM, case.FH, 1, w8d, None, want_S=True)
            ctx.synchronize()
            res = [(S, o.download()[0], c.download()[0]) for S, o, c in zip(Ss, outs, outcs)]
            for h in outs + outcs:
                h.free()
        else:
            w8 = built.w8s[0] if built.w8s else None
            res = [ctx.aggregate(cvs[0], case.P1, case.P2, case.NDIR, case.MGM, case.FH, 1, w8, None, want_S=True)]
        names = [n for n, _ in ctx.timings()]
    finally:
        ctx.timing(False)
    assert ctx.last_pass_kernel() == "k_pass_exact", (case.name, ctx.last_pass_kernel())
    ran = [n for n in names if n.startswith("k_pass")]
    assert ran and set(ran) == {"k_pass_exact"}, (case.name, names)
    return res


@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_exact_kernel_on_crafted_volumes(ctx, oracle, case):
    if RAISED:
        pytest.fail("not run: the device call of %s raised" % RAISED[0])
    built = X.build(case, oracle)
    X.must_take_exact(case, built)  # (raises: nothing is uploaded then)
    fig = X.check_floors(case, built, oracle)
    exp = X.expected(case, built, oracle)
    print(case.name, fig)
    cvs, w8d = [], None
    try:
        try:
            if case.kind == "ragged":
                lo, hi, _, _ = built.ranges
                u, v = built.images
                cvs = [ctx.costvolume(u, v, lo, hi, "none", "census", float("inf"), 5)]
                assert cvs[0].dims == (case.nx, case.ny, case.dmin, case.dmin + case.L - 1)
                assert ndiff(cvs[0].download(), built.Cs[0]) == 0  # (the volume the oracle aggregated)
            else:
                cvs = [ctx.upload_volume(C, case.dmin) for C in built.Cs]
            if case.kind == "batch":
                w8d = [ctx.upload_image(w) for w in built.w8s]
            shape = built.Cs[0].shape
            own = X.own_labels(case, built)
            for rep in range(2):
                res = run_once(ctx, case, built, cvs, w8d)
                try:
                    for k, (S, out, cost) in enumerate(res):
                        tag = (case.name, "run", rep, "volume", k)
                        for p in range(case.NDIR):
                            assert ndiff(lr_of(ctx, cvs[0], k, p, shape), exp.lr[k][p]) == 0, tag + ("Lr", p)
                        # (a ragged S exists inside each pixel's own range only: the reference's Dvec holds nothing else)
                        assert ndiff(np.where(own, S.download(), 0), np.where(own, exp.S[k], 0)) == 0, tag + ("S",)
                        assert ndiff(cost, exp.cost[k]) == 0, tag + ("cost",)
                        assert labels_equal(out, exp.out[k], exp.cost[k]), tag + ("labels",)
                finally:
                    if not RAISED:
                        for S, _, _ in res:
                            S.free()
        except mgm_amd.MgmError:
            RAISED.append(case.name)
            raise
    finally:
        if not RAISED:
            for h in cvs + (w8d or []):
                h.free()
