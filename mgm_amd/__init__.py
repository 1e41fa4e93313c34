"""mgm_amd -- Python (ctypes) binding of libmgm_hip.so, the MI355X MGM stereo core.

This module is host-side plumbing for tests and benchmarks: every compute call
goes through the C ABI declared in ``include/mgm_hip.h`` and runs as HIP
kernels on a gfx950 device.  There is no CPU path here; if the shared library
is missing or no device is usable, calls raise :class:`MgmError`.

The function names and argument meanings mirror the reference's three entry
points (``allocate_and_fill_sgm_costvolume``, ``mgm``, ``subpixel_refinement_sgm``;
mgm.cc:32-59) so tests read like calls into the reference.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MGM_HIP_LIB") or os.path.join(_HERE, "lib", "libmgm_hip.so")

# every symbol include/mgm_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "mgm_ctx_create", "mgm_ctx_destroy", "mgm_last_error", "mgm_ctx_synchronize", "mgm_ctx_stream", "mgm_version", "mgm_ctx_trim",
    "mgm_timing_enable", "mgm_timing_reset", "mgm_timing_count", "mgm_timing_get",
    "mgm_img_create", "mgm_img_upload", "mgm_img_download", "mgm_img_dims", "mgm_img_device_ptr", "mgm_img_free",
    "mgm_cv_create", "mgm_cv_upload", "mgm_cv_download", "mgm_cv_dims", "mgm_cv_device_ptr", "mgm_cv_free",
    "mgm_costvolume_build_dev", "mgm_costvolume_build", "mgm_weights_dev",
    "mgm_aggregate_dev", "mgm_aggregate", "mgm_debug_download_lr", "mgm_refine_dev", "mgm_refine",
    "mgm_selftest_div3", "mgm_aggregate_passes_dev", "mgm_lr_device_ptr", "mgm_wta_rows_dev",
    "mgm_aggregate_batch_dev", "mgm_median_dev", "mgm_leftright_dev", "mgm_backproject_dev",
    "mgm_wta_windowed_dev", "mgm_wta_right_dev", "mgm_update_ranges_dev", "mgm_costvolume_build_ranged_dev",
    "mgm_multi_create", "mgm_multi_destroy", "mgm_multi_size", "mgm_multi_ctx", "mgm_multi_last_error", "mgm_multi_plan",
    "mgm_multi_aggregate", "mgm_multi_transport", "mgm_img_device", "mgm_cv_device", "mgm_aggregate_passes_at_dev",
    "mgm_ctx_set_workspace_limit", "mgm_ctx_mem_info", "mgm_ctx_set_pipeline", "mgm_img_update", "mgm_debug_probe_workspace", "mgm_ctx_set_placement_tries",
    "mgm_debug_wta_stats", "mgm_debug_download_lmin", "mgm_debug_last_pass_kernel",
    "mgm_multiscale_levels", "mgm_zoom_out_dev", "mgm_ranges_zoom_out_dev", "mgm_ranges_from_coarse_dev", "mgm_multiscale_pair_dev",
    "mgm_wta_runnerup_dev", "mgm_uniqueness_dev", "mgm_speckle_dev", "mgm_fill_holes_dev",
    "mgm_classify_holes_dev", "mgm_fill_holes_classified_dev",
    "mgm_subpix_phase_dev", "mgm_costvolume_build_subpix_dev", "mgm_subpix_scale_dev",
    "mgm_debug_rel_lr_device_ptr", "mgm_debug_wta_rel_again_dev", "mgm_debug_lr_device_ptr",
    "mgm_wta_consensus_dev", "mgm_consensus_filter_dev", "mgm_energy_dev",
]

MGM_OK, MGM_ERR_INVALID, MGM_ERR_UNSUPPORTED, MGM_ERR_HIP, MGM_ERR_NOMEM, MGM_ERR_INTERNAL = range(6)


class MgmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mgm_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


class MsLevel(C.Structure):
    """``mgm_ms_level``: what one level of the multiscale driver ran on ([0] left->right, [1] right->left)."""
    _fields_ = [("nx", C.c_int), ("ny", C.c_int), ("vnx", C.c_int), ("vny", C.c_int), ("hull_min", C.c_int * 2),
                ("hull_max", C.c_int * 2), ("weighted", C.c_int * 2), ("batched", C.c_int)]


class MsParams(C.Structure):
    """``mgm_ms_params`` (size-prefixed: ``struct_size`` first)."""
    _fields_ = [("struct_size", C.c_uint), ("nscales", C.c_int), ("slack", C.c_int), ("radius", C.c_int), ("dmin", C.c_int),
                ("dmax", C.c_int), ("lo", C.c_void_p), ("hi", C.c_void_p), ("P1", C.c_float), ("P2", C.c_float),
                ("NDIR", C.c_int), ("TSGM", C.c_int), ("use_fh", C.c_int), ("fix_overcount", C.c_int), ("aP2", C.c_float),
                ("aThresh", C.c_float), ("prefilter", C.c_char_p), ("distance", C.c_char_p), ("truncDist", C.c_float),
                ("census_win", C.c_int), ("refine", C.c_char_p), ("iterations", C.c_int), ("median", C.c_int),
                ("testlrrl", C.c_int), ("tau", C.c_float), ("levels_run", C.POINTER(C.c_int)), ("levels", C.POINTER(MsLevel)),
                ("outR_nolr", C.c_void_p)]


class MsParamsConsensus(C.Structure):
    """``mgm_ms_params`` as it has grown at its end: ``MsParams`` (kept as the struct of an older caller) and the consensus fields."""
    _fields_ = MsParams._fields_ + [("consensus_tol", C.c_float), ("consensus_min", C.c_int), ("votesL", C.c_void_p)]


class EnergyParams(C.Structure):
    """``mgm_energy_params``."""
    _fields_ = [("kind", C.c_int), ("P1", C.c_float), ("P2", C.c_float), ("connectivity", C.c_int), ("use_fh", C.c_int), ("w8", C.c_void_p)]


class EnergyTotals(C.Structure):
    """``mgm_energy_totals``."""
    _fields_ = [("serial", C.c_float), ("total", C.c_double), ("data", C.c_double), ("smooth", C.c_double), ("finite", C.c_ulonglong),
                ("pixels", C.c_ulonglong)]


ENERGY_KINDS = {"l1trunc": 0, "l1": 1, "l2": 2, "model": 3}


def load_library():
    """dlopen libmgm_hip.so (building nothing: see mgm_amd/build.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MgmError(MGM_ERR_HIP, "%s not found: run `python -m mgm_amd.build` (hipcc, gfx950)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, fp, i, f, cp = C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_char_p
    pp = C.POINTER(C.c_void_p)
    L.mgm_version.restype = cp
    L.mgm_last_error.restype = cp
    L.mgm_last_error.argtypes = [vp]
    L.mgm_ctx_create.argtypes = [i, pp]
    L.mgm_ctx_destroy.argtypes = [vp]
    L.mgm_ctx_synchronize.argtypes = [vp]
    L.mgm_ctx_trim.argtypes = [vp]
    L.mgm_ctx_stream.argtypes = [vp]
    L.mgm_ctx_stream.restype = vp
    L.mgm_timing_enable.argtypes = [vp, i]
    L.mgm_timing_reset.argtypes = [vp]
    L.mgm_timing_count.argtypes = [vp]
    L.mgm_timing_get.argtypes = [vp, i, C.POINTER(cp), C.POINTER(f)]
    L.mgm_img_create.argtypes = [vp, i, i, i, pp]
    L.mgm_img_upload.argtypes = [vp, fp, i, i, i, pp]
    L.mgm_img_download.argtypes = [vp, vp, fp]
    L.mgm_img_update.argtypes = [vp, vp, fp]
    L.mgm_debug_probe_workspace.argtypes = [vp, i, C.POINTER(f)]
    L.mgm_ctx_set_placement_tries.argtypes = [vp, i]
    L.mgm_debug_wta_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.mgm_debug_last_pass_kernel.argtypes = [vp, cp, i]
    L.mgm_img_dims.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.mgm_img_device_ptr.argtypes = [vp]
    L.mgm_img_device_ptr.restype = vp
    L.mgm_img_free.argtypes = [vp, vp]
    L.mgm_cv_create.argtypes = [vp, i, i, i, i, pp]
    L.mgm_cv_upload.argtypes = [vp, fp, i, i, i, i, pp]
    L.mgm_cv_download.argtypes = [vp, vp, fp]
    L.mgm_cv_dims.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.mgm_cv_device_ptr.argtypes = [vp]
    L.mgm_cv_device_ptr.restype = vp
    L.mgm_cv_free.argtypes = [vp, vp]
    L.mgm_costvolume_build_dev.argtypes = [vp, vp, vp, i, i, cp, cp, f, i, pp]
    L.mgm_costvolume_build.argtypes = [vp, fp, fp, i, i, i, i, i, fp, fp, cp, cp, f, i, pp]
    L.mgm_weights_dev.argtypes = [vp, vp, f, f, pp]
    L.mgm_aggregate_dev.argtypes = [vp, vp, vp, f, f, i, i, i, i, cp, vp, vp, pp]
    L.mgm_aggregate.argtypes = [vp, vp, fp, f, f, i, i, i, i, cp, fp, fp, pp]
    L.mgm_median_dev.argtypes = [vp, vp, i, vp]
    L.mgm_costvolume_build_ranged_dev.argtypes = [vp, vp, vp, vp, vp, i, i, cp, cp, f, i, pp]
    L.mgm_wta_windowed_dev.argtypes = [vp, vp, i, i, cp, vp, vp, vp, vp]
    L.mgm_wta_right_dev.argtypes = [vp, vp, i, i, cp, vp, vp]
    L.mgm_wta_runnerup_dev.argtypes = [vp, vp, i, i, i, vp, vp, vp, vp]
    L.mgm_uniqueness_dev.argtypes = [vp, vp, vp, vp, f, vp, vp]
    L.mgm_wta_consensus_dev.argtypes = [vp, vp, i, vp, f, vp, vp]
    L.mgm_consensus_filter_dev.argtypes = [vp, vp, vp, i, vp]
    L.mgm_speckle_dev.argtypes = [vp, vp, i, f, vp, vp]
    L.mgm_energy_dev.argtypes = [vp, vp, vp, C.POINTER(EnergyParams), vp, C.POINTER(EnergyTotals)]
    L.mgm_fill_holes_dev.argtypes = [vp, vp, cp, i, i, vp, vp]
    L.mgm_classify_holes_dev.argtypes = [vp, vp, vp, i, i, f, vp]
    L.mgm_fill_holes_classified_dev.argtypes = [vp, vp, vp, cp, cp, i, i, vp, vp]
    L.mgm_subpix_phase_dev.argtypes = [vp, vp, i, i, cp, pp]
    L.mgm_costvolume_build_subpix_dev.argtypes = [vp, vp, vp, i, i, i, cp, cp, cp, f, i, pp]
    L.mgm_subpix_scale_dev.argtypes = [vp, vp, i, vp]
    L.mgm_update_ranges_dev.argtypes = [vp, vp, vp, vp, i, i]
    L.mgm_leftright_dev.argtypes = [vp, vp, vp, f, vp]
    L.mgm_backproject_dev.argtypes = [vp, vp, vp, vp, vp]
    L.mgm_aggregate_batch_dev.argtypes = [vp, i, pp, pp, f, f, i, i, i, i, cp, pp, pp, pp]
    L.mgm_debug_download_lr.argtypes = [vp, i, fp]
    L.mgm_debug_download_lmin.argtypes = [vp, i, i, fp]
    L.mgm_debug_rel_lr_device_ptr.argtypes = [vp, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_longlong), pp]
    L.mgm_debug_rel_lr_device_ptr.restype = vp
    L.mgm_debug_lr_device_ptr.argtypes = [vp, i, i, C.POINTER(i), C.POINTER(C.c_longlong)]
    L.mgm_debug_lr_device_ptr.restype = vp
    L.mgm_debug_wta_rel_again_dev.argtypes = [vp, vp, i, i, cp, vp, vp, pp]
    L.mgm_refine_dev.argtypes = [vp, vp, cp, vp, vp]
    L.mgm_refine.argtypes = [vp, vp, cp, fp, fp]
    L.mgm_selftest_div3.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.mgm_aggregate_passes_dev.argtypes = [vp, vp, vp, f, f, i, i, i, i]
    L.mgm_lr_device_ptr.argtypes = [vp, i]
    L.mgm_lr_device_ptr.restype = vp
    L.mgm_wta_rows_dev.argtypes = [vp, vp, i, i, vp, i, i, cp, vp, vp]
    ip = C.POINTER(i)
    L.mgm_multi_create.argtypes = [ip, i, pp]
    L.mgm_multi_destroy.argtypes = [vp]
    L.mgm_multi_size.argtypes = [vp]
    L.mgm_multi_ctx.argtypes = [vp, i]
    L.mgm_multi_ctx.restype = vp
    L.mgm_multi_last_error.argtypes = [vp]  # (NULL: why the last mgm_multi_create failed)
    L.mgm_multi_last_error.restype = cp
    L.mgm_multi_plan.argtypes = [i, i, i, ip, ip, ip, ip]
    L.mgm_multi_aggregate.argtypes = [vp, pp, pp, f, f, i, i, i, i, cp, vp, vp]
    L.mgm_multi_transport.argtypes = [vp]
    L.mgm_multi_transport.restype = cp
    L.mgm_img_device.argtypes = [vp]
    L.mgm_cv_device.argtypes = [vp]
    L.mgm_aggregate_passes_at_dev.argtypes = [vp, vp, vp, f, f, i, i, i, i, i, i, i]
    L.mgm_ctx_set_workspace_limit.argtypes = [vp, C.c_ulonglong]
    L.mgm_ctx_set_pipeline.argtypes = [vp, i]
    L.mgm_ctx_mem_info.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.mgm_multiscale_levels.argtypes = [i, i, i, i, i, ip]
    L.mgm_zoom_out_dev.argtypes = [vp, vp, pp]
    L.mgm_ranges_zoom_out_dev.argtypes = [vp, vp, vp, pp, pp]
    L.mgm_ranges_from_coarse_dev.argtypes = [vp, vp, vp, vp, i, i, ip, ip]
    L.mgm_multiscale_pair_dev.argtypes = [vp, vp, vp, C.POINTER(MsParams), vp, vp, vp, vp, vp]
    _lib = L
    return L


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Image:
    """Device-resident planar float image (the reference's ``struct Img``)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def shape(self):
        nx, ny, nch = C.c_int(), C.c_int(), C.c_int()
        self.ctx.lib.mgm_img_dims(self.h, nx, ny, nch)
        return (nch.value, ny.value, nx.value)

    def download(self):
        out = np.empty(self.shape, np.float32)
        self.ctx._chk(self.ctx.lib.mgm_img_download(self.ctx.h, self.h, _ptr(out)))
        return out

    def update(self, a):
        """Refill from a host array of the image's own shape (no allocation)."""
        a = np.ascontiguousarray(a, np.float32)
        if a.size != int(np.prod(self.shape)):
            raise ValueError("Image.update: %r does not match the image's shape %r" % (a.shape, self.shape))
        self.ctx._chk(self.ctx.lib.mgm_img_update(self.ctx.h, self.h, _ptr(a)))

    def free(self):
        if self.h:
            self.ctx.lib.mgm_img_free(self.ctx.h, self.h)
            self.h = None


class CostVolume:
    """Device-resident dense volume [ny][nx][L] (the reference's ``costvolume_t``)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    @property
    def dims(self):
        nx, ny, dmin, dmax = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.ctx.lib.mgm_cv_dims(self.h, nx, ny, dmin, dmax)
        return nx.value, ny.value, dmin.value, dmax.value

    def download(self):
        nx, ny, dmin, dmax = self.dims
        out = np.empty((ny, nx, dmax - dmin + 1), np.float32)
        self.ctx._chk(self.ctx.lib.mgm_cv_download(self.ctx.h, self.h, _ptr(out)))
        return out

    def free(self):
        if self.h:
            self.ctx.lib.mgm_cv_free(self.ctx.h, self.h)
            self.h = None


class Context:
    """One device + stream + workspace (``mgm_ctx``)."""

    def __init__(self, device=0, _borrowed=None):
        self.lib = load_library()
        self.owned = _borrowed is None
        if _borrowed is not None:  # a rank's context of an mgm_multi handle (destroyed with it)
            self.h = C.c_void_p(_borrowed)
            return
        h = C.c_void_p()
        r = self.lib.mgm_ctx_create(device, C.byref(h))
        if r:
            raise MgmError(r, "mgm_ctx_create(%d) failed: no usable HIP device" % device)
        self.h = h

    def close(self):
        if self.h and self.owned:
            self.lib.mgm_ctx_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, r):
        if r:
            raise MgmError(r, self.lib.mgm_last_error(self.h).decode())

    def synchronize(self):
        self._chk(self.lib.mgm_ctx_synchronize(self.h))

    def trim(self):
        """Release the grow-only workspace (mgm_ctx_trim)."""
        self._chk(self.lib.mgm_ctx_trim(self.h))

    def set_workspace_limit(self, nbytes):
        """Cap on the workspace of one pass launch; larger batches run as several launches (mgm_ctx_set_workspace_limit)."""
        self._chk(self.lib.mgm_ctx_set_workspace_limit(self.h, int(nbytes)))

    def set_pipeline(self, depth):
        """depth >= 2: aggregate calls are deferred and gathered, `depth` of them run as one batched launch (results after the
        last call of a group, synchronize() or any download); see mgm_ctx_set_pipeline in mgm_hip.h."""
        self._chk(self.lib.mgm_ctx_set_pipeline(self.h, int(depth)))

    def mem_info(self):
        """(free, total) bytes of the context's device right now."""
        f, t = C.c_ulonglong(0), C.c_ulonglong(0)
        self._chk(self.lib.mgm_ctx_mem_info(self.h, C.byref(f), C.byref(t)))
        return int(f.value), int(t.value)

    def stream_ptr(self):
        """The hipStream_t everything is enqueued on (for torch.cuda.ExternalStream)."""
        return int(self.lib.mgm_ctx_stream(self.h) or 0)

    # ---- containers ----
    def upload_image(self, a):
        a = _f32(a)
        if a.ndim == 2:
            a = a[None]
        nch, ny, nx = a.shape
        h = C.c_void_p()
        self._chk(self.lib.mgm_img_upload(self.h, _ptr(a), nx, ny, nch, C.byref(h)))
        return Image(self, h)

    def new_image(self, nx, ny, nch=1):
        h = C.c_void_p()
        self._chk(self.lib.mgm_img_create(self.h, nx, ny, nch, C.byref(h)))
        return Image(self, h)

    def upload_volume(self, dense, dmin):
        dense = _f32(dense)
        ny, nx, L = dense.shape
        h = C.c_void_p()
        self._chk(self.lib.mgm_cv_upload(self.h, _ptr(dense), nx, ny, dmin, dmin + L - 1, C.byref(h)))
        return CostVolume(self, h)

    # ---- the path ----
    def costvolume_dev(self, u, v, dmin, dmax, prefilter="none", distance="ad", truncDist=float("inf"),
                       census_win=3, into=None):
        h = C.c_void_p(into.h.value) if into is not None else C.c_void_p()
        self._chk(self.lib.mgm_costvolume_build_dev(self.h, u.h, v.h, dmin, dmax, prefilter.encode(),
                                                    distance.encode(), truncDist, census_win, C.byref(h)))
        return into if into is not None else CostVolume(self, h)

    def costvolume_ranged_dev(self, u, v, dminI, dmaxI, hull_min, hull_max, prefilter="none", distance="ad", truncDist=float("inf"),
                              census_win=3, into=None):
        """Device form with per-pixel range images (device Images): the ragged volume over [hull_min, hull_max]."""
        h = C.c_void_p(into.h.value) if into is not None else C.c_void_p()
        self._chk(self.lib.mgm_costvolume_build_ranged_dev(self.h, u.h, v.h, dminI.h, dmaxI.h, hull_min, hull_max, prefilter.encode(),
                                                           distance.encode(), truncDist, census_win, C.byref(h)))
        return into if into is not None else CostVolume(self, h)

    def costvolume(self, u, v, dminI, dmaxI, prefilter="none", distance="ad", truncDist=float("inf"), census_win=3):
        """Host-buffer form with per-pixel range images, like the reference."""
        u, v = _f32(u), _f32(v)
        if u.ndim == 2:
            u, v = u[None], v[None]
        nch, ny, nx = u.shape
        _, vny, vnx = v.shape
        dminI, dmaxI = _f32(dminI), _f32(dmaxI)
        h = C.c_void_p()
        self._chk(self.lib.mgm_costvolume_build(self.h, _ptr(u), _ptr(v), nx, ny, nch, vnx, vny, _ptr(dminI),
                                                _ptr(dmaxI), prefilter.encode(), distance.encode(), truncDist,
                                                census_win, C.byref(h)))
        return CostVolume(self, h)

    def weights_dev(self, u, aP, aThresh, into=None):
        h = C.c_void_p(into.h.value) if into is not None else C.c_void_p()
        self._chk(self.lib.mgm_weights_dev(self.h, u.h, aP, aThresh, C.byref(h)))
        return into if into is not None else Image(self, h)

    def aggregate_dev(self, Cv, P1, P2, NDIR, MGM, use_fh=0, fix_overcount=1, w8=None, refine=None, out=None,
                      outcost=None, want_S=False):
        nx, ny, _, _ = Cv.dims
        out = out or self.new_image(nx, ny)
        outcost = outcost or self.new_image(nx, ny)
        S = C.c_void_p()
        self._chk(self.lib.mgm_aggregate_dev(self.h, Cv.h, w8.h if w8 is not None else None, P1, P2, NDIR, MGM,
                                             use_fh, fix_overcount, refine.encode() if refine else None, out.h,
                                             outcost.h, C.byref(S) if want_S else None))
        return (CostVolume(self, S) if want_S else None), out, outcost

    def wta_windowed_dev(self, Cv, NDIR, fix_overcount, refine, dminI, dmaxI, out=None, outcost=None):
        nx, ny, _, _ = Cv.dims
        out = out or self.new_image(nx, ny)
        outcost = outcost or self.new_image(nx, ny)
        self._chk(self.lib.mgm_wta_windowed_dev(self.h, Cv.h, NDIR, fix_overcount, refine.encode() if refine else None,
                                                dminI.h, dmaxI.h, out.h, outcost.h))
        return out, outcost

    def wta_right_dev(self, Cv, NDIR, fix_overcount, refine, vnx, out=None, outcost=None):
        """The right view's map (vnx wide) read out of the context's last aggregation of the LEFT volume Cv: (out, outcost)
        as device images; refine None / "none" / "vfit" (mgm_wta_right_dev)."""
        _, ny, _, _ = Cv.dims
        out = out or self.new_image(vnx, ny)
        outcost = outcost or self.new_image(vnx, ny)
        self._chk(self.lib.mgm_wta_right_dev(self.h, Cv.h, NDIR, fix_overcount, refine.encode() if refine else None, out.h, outcost.h))
        return out, outcost

    def wta_runnerup_dev(self, Cv, NDIR, fix_overcount, radius=1, out2=None, cost2=None, want_first=True):
        """The runner-up search over the context's last aggregation of Cv (mgm_wta_runnerup_dev): device images
        (out2, cost2, out1, cost1) -- the best label more than `radius` away from the winner and S there, the unrefined winner
        and S there (None, None with want_first=False)."""
        nx, ny, _, _ = Cv.dims
        mine = []  # the images made here: freed if the call fails

        def new():
            mine.append(self.new_image(nx, ny))
            return mine[-1]
        try:
            out2 = out2 or new()
            cost2 = cost2 or new()
            out1 = new() if want_first else None
            cost1 = new() if want_first else None
            self._chk(self.lib.mgm_wta_runnerup_dev(self.h, Cv.h, NDIR, fix_overcount, radius, out2.h, cost2.h,
                                                    out1.h if want_first else None, cost1.h if want_first else None))
        except Exception:
            for im in mine:
                im.free()
            raise
        return out2, cost2, out1, cost1

    def uniqueness_dev(self, d, cost1, cost2, ratio, out=None, want_conf=True):
        """conf = 1 - cost1 / cost2 and out = NaN where conf < ratio, else d (mgm_uniqueness_dev): device images (out, conf).
        out: an image to write (d itself is allowed), None for a new one, False for none; conf is None with want_conf=False."""
        _, ny, nx = d.shape
        mine = []  # the images made here: freed if the call fails
        try:
            if out is None:
                out = self.new_image(nx, ny)
                mine.append(out)
            conf = None
            if want_conf:
                conf = self.new_image(nx, ny)
                mine.append(conf)
            self._chk(self.lib.mgm_uniqueness_dev(self.h, d.h, cost1.h, cost2.h, ratio, out.h if out else None, conf.h if want_conf else None))
        except Exception:
            for im in mine:
                im.free()
            raise
        return (out if out else None), conf

    def wta_consensus_dev(self, Cv, NDIR, d, tol=1.0, votes=None, want_winners=False):
        """The consensus votes over the context's last aggregation of Cv (mgm_wta_consensus_dev): device images (votes, winners)
        -- how many of the NDIR passes, each taken alone, pick a label within tol of the map d, and the passes' own winners
        (nx x ny x NDIR; None without want_winners).  votes: an image to write, None for a new one, False for none (d may then
        be None)."""
        nx, ny, _, _ = Cv.dims
        mine = []  # the images made here: freed if the call fails
        try:
            if votes is None:
                votes = self.new_image(nx, ny)
                mine.append(votes)
            winners = None
            if want_winners:
                winners = self.new_image(nx, ny, NDIR)
                mine.append(winners)
            self._chk(self.lib.mgm_wta_consensus_dev(self.h, Cv.h, NDIR, d.h if d is not None else None, tol, votes.h if votes else None,
                                                     winners.h if want_winners else None))
        except Exception:
            for im in mine:
                im.free()
            raise
        return (votes if votes else None), winners

    def consensus_filter_dev(self, d, votes, minvotes, out=None):
        """out = NaN where votes < minvotes, else d (mgm_consensus_filter_dev): the device image out -- one to write (d itself is
        allowed) or None for a new one."""
        _, ny, nx = d.shape
        mine = []  # the image made here: freed if the call fails
        try:
            if out is None:
                out = self.new_image(nx, ny)
                mine.append(out)
            self._chk(self.lib.mgm_consensus_filter_dev(self.h, d.h, votes.h, minvotes, out.h))
        except Exception:
            for im in mine:
                im.free()
            raise
        return out

    def speckle_dev(self, d, maxsize, maxdiff=1.0, out=None, want_size=False):
        """The speckle filter (mgm_speckle_dev): NaN into every 4-connected component of finite pixels, joined where
        |d(p) - d(q)| <= maxdiff, of at most maxsize pixels; device images (out, size_map).  out: an image to write (d itself is
        allowed), None for a new one, False for none; size_map (every pixel's component size, 0 on non-finite pixels) is None
        without want_size."""
        _, ny, nx = d.shape
        mine = []  # the images made here: freed if the call fails
        try:
            if out is None:
                out = self.new_image(nx, ny)
                mine.append(out)
            size_map = None
            if want_size:
                size_map = self.new_image(nx, ny)
                mine.append(size_map)
            self._chk(self.lib.mgm_speckle_dev(self.h, d.h, maxsize, maxdiff, out.h if out else None, size_map.h if want_size else None))
        except Exception:
            for im in mine:
                im.free()
            raise
        return (out if out else None), size_map

    def energy_dev(self, Cv, d, kind, P1, P2, connectivity=4, use_fh=0, w8=None, want_map=True, want_totals=True):
        """The energy of the map d on the volume Cv (mgm_energy_dev).  kind: 0 / "l1trunc", 1 / "l1", 2 / "l2" -- the reference's
        evaluate_energy_4connected -- or 3 / "model": data term plus the weighted potentials of the run's kind (use_fh) over 4 or 8
        neighbours, w8 None (ones) or an 8-channel weight image.  P1 / P2 as given (already multiplied by the channel count).
        Returns (map, totals): a new device image or None, and a dict (serial: the fp32 sum in raster order; total, data, smooth:
        fp64 sums over the finite pixels; finite, pixels) or None.  Asking for the totals synchronises."""
        _, ny, nx = d.shape
        q = EnergyParams(ENERGY_KINDS.get(kind, kind) if isinstance(kind, str) else int(kind), P1, P2, connectivity, use_fh, w8.h if w8 is not None else None)
        tot = EnergyTotals()
        mine = []  # the image made here: freed if the call fails
        try:
            E = None
            if want_map:
                E = self.new_image(nx, ny)
                mine.append(E)
            self._chk(self.lib.mgm_energy_dev(self.h, Cv.h, d.h, C.byref(q), E.h if E else None, C.byref(tot) if want_totals else None))
        except Exception:
            for im in mine:
                im.free()
            raise
        return E, ({f: getattr(tot, f) for f, _ in EnergyTotals._fields_} if want_totals else None)

    def fill_holes_dev(self, d, mode="median", dirs=8, maxdist=0, out=None, want_filled=False):
        """Hole filling (mgm_fill_holes_dev): every non-finite pixel of d takes the median / min / max of the nearest finite pixels
        along the first `dirs` (2, 4, 8) of the rays (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,+1) (+1,-1) (-1,-1), at most maxdist steps
        away (0: no limit); rays read the original map.  Device images (out, filled).  out: an image to write (d itself is allowed),
        None for a new one, False for none; filled (1 where a hole received a value, else 0) is None without want_filled."""
        _, ny, nx = d.shape
        mine = []  # the images made here: freed if the call fails
        try:
            if out is None:
                out = self.new_image(nx, ny)
                mine.append(out)
            filled = None
            if want_filled:
                filled = self.new_image(nx, ny)
                mine.append(filled)
            self._chk(self.lib.mgm_fill_holes_dev(self.h, d.h, None if mode is None else str(mode).encode(), dirs, maxdist,
                                                  out.h if out else None, filled.h if want_filled else None))
        except Exception:
            for im in mine:
                im.free()
            raise
        return (out if out else None), filled

    def classify_holes_dev(self, d, other, dmin, dmax, tau, cls=None):
        """Hole classification (mgm_classify_holes_dev): the device image cls -- 0 where d is finite, 2 (a mismatch) at a hole (x, y)
        that some column xr of [x + dmin, x + dmax] inside `other` lands on, |xr + other(xr, y) - x| <= tau in float, 1 (an occlusion)
        at every other hole.  other: the other view's map as it went INTO the left-right test, of d's height.  cls: an image of d's
        size to write, None for a new one."""
        _, ny, nx = d.shape
        mine = []  # the images made here: freed if the call fails
        try:
            if cls is None:
                cls = self.new_image(nx, ny)
                mine.append(cls)
            self._chk(self.lib.mgm_classify_holes_dev(self.h, d.h, other.h, dmin, dmax, tau, cls.h))
        except Exception:
            for im in mine:
                im.free()
            raise
        return cls

    def fill_holes_classified_dev(self, d, cls, mode_occ="sechigh", mode_mis="median", dirs=8, maxdist=0, out=None, want_filled=False):
        """The classified fill (mgm_fill_holes_classified_dev): fill_holes_dev with two rules -- a hole with cls == 1 (an occlusion)
        takes mode_occ, every other hole mode_mis; the modes are median, min, max, seclow (the second lowest candidate) and sechigh
        (the second highest).  The background is sechigh where disparities are negative (a range like -64 .. 0) and seclow where
        they are positive.  Device images (out, filled), as fill_holes_dev returns them."""
        _, ny, nx = d.shape
        mine = []  # the images made here: freed if the call fails
        try:
            if out is None:
                out = self.new_image(nx, ny)
                mine.append(out)
            filled = None
            if want_filled:
                filled = self.new_image(nx, ny)
                mine.append(filled)
            enc = lambda m: None if m is None else str(m).encode()
            self._chk(self.lib.mgm_fill_holes_classified_dev(self.h, d.h, cls.h if cls is not None else None, enc(mode_occ), enc(mode_mis), dirs,
                                                             maxdist, out.h if out else None, filled.h if want_filled else None))
        except Exception:
            for im in mine:
                im.free()
            raise
        return (out if out else None), filled

    def pair_right_from_left(self, u, v, dmin, dmax, P1=8.0, P2=32.0, NDIR=4, TSGM=4, use_fh=0, fix_overcount=1, aP2=1.0, aThresh=5.0,
                             prefilter="none", distance="ad", truncDist=float("inf"), census_win=3, refine="none", tau=1.0, median=0):
        """A stereo pair with ONE run: the left->right cost volume and aggregation, the right map read out of that run
        (wta_right_dev), the optional medians and the left-right test both ways.  u, v: device images of one height (P1 / P2 as
        given: multiply by the channel count yourself).  Returns device images (left map, right map, left cost), the maps checked."""
        _, ny, nx = u.shape
        _, vny, vnx = v.shape
        if vny != ny:
            raise ValueError("pair_right_from_left: the two images must have one height")
        refine = refine if refine and refine != "none" else None
        cv = self.costvolume_dev(u, v, dmin, dmax, prefilter, distance, truncDist, census_win)
        w8 = self.weights_dev(u, aP2, aThresh) if aP2 != 1 else None
        mine = [cv, w8]
        try:
            _, outL, costL = self.aggregate_dev(cv, P1, P2, NDIR, TSGM, use_fh, fix_overcount, w8=w8, refine=refine)
            mine += [outL, costL]
            outR, costR = self.wta_right_dev(cv, NDIR, fix_overcount, refine, vnx)
            mine += [outR, costR]
            if median:
                mL, mR = self.median_dev(outL, median), self.median_dev(outR, median)
                mine += [mL, mR]
                outL, outR = mL, mR
            chkR = self.leftright_dev(outR, outL, tau)
            mine.append(chkR)
            chkL = self.leftright_dev(outL, outR, tau)
        except Exception:
            for o in mine:
                if o is not None:
                    o.free()
            raise
        for o in mine:
            if o is not None and o is not chkR and o is not costL:
                o.free()
        return chkL, chkR, costL

    # ---- sub-pixel label spacing (mgm_subpix.hip) ----
    def subpix_phase_dev(self, v, s, k, interp="cubic", into=None):
        """The phase image v_k of v at the shift k/s along x (mgm_subpix_phase_dev): s 1, 2 or 4, k 0..s-1, interp "linear" or "cubic"
        (Keys, a = -1/2); k = 0 is a copy of v.  into: an image of v's shape to refill, None for a new one."""
        h = C.c_void_p(into.h.value) if into is not None else C.c_void_p()
        self._chk(self.lib.mgm_subpix_phase_dev(self.h, v.h, s, k, None if interp is None else str(interp).encode(), C.byref(h)))
        return into if into is not None else Image(self, h)

    def costvolume_subpix_dev(self, u, v, dmin, dmax, s, interp="cubic", prefilter="none", distance="ad", truncDist=float("inf"),
                              census_win=3, into=None):
        """The fine volume of mgm_costvolume_build_subpix_dev: labels s*dmin .. s*dmax, fine label d' = the disparity d'/s, made of
        s ordinary builds of u against the phase images of v.  Aggregations and searches of it give maps in fine units
        (subpix_scale_dev); P1, P2, the runner-up radius and the refinements act per fine label."""
        h = C.c_void_p(into.h.value) if into is not None else C.c_void_p()
        self._chk(self.lib.mgm_costvolume_build_subpix_dev(self.h, u.h, v.h, dmin, dmax, s, None if interp is None else str(interp).encode(),
                                                           prefilter.encode(), distance.encode(), truncDist, census_win, C.byref(h)))
        return into if into is not None else CostVolume(self, h)

    def subpix_scale_dev(self, img, s, out=None):
        """out = img / s (mgm_subpix_scale_dev): a map in fine labels becomes one in pixels.  out may be img itself; None: a new image."""
        nch, ny, nx = img.shape
        mine = out is None
        out = self.new_image(nx, ny, nch) if mine else out
        try:
            self._chk(self.lib.mgm_subpix_scale_dev(self.h, img.h, s, out.h))
        except Exception:
            if mine:
                out.free()
            raise
        return out

    def pair_subpix(self, u, v, dmin, dmax, s, interp="cubic", P1=8.0, P2=32.0, NDIR=4, TSGM=4, use_fh=0, fix_overcount=1, aP2=1.0,
                    aThresh=5.0, prefilter="none", distance="ad", truncDist=float("inf"), census_win=3, refine="none", tau=1.0, median=0):
        """A stereo pair at the label spacing 1/s: both runs on fine volumes (the right->left one with the images exchanged and the
        range [-dmax, -dmin]), the rescale to pixels, the optional medians and the left-right test of the left map.  u, v: device
        images of one height; P1 / P2 as given, PER FINE LABEL (a slope of one pixel takes s steps of P1).  Returns device images
        (checked left map, unchecked left map, unchecked right map, left cost map); the cost map is not rescaled."""
        _, ny, nx = u.shape
        _, vny, vnx = v.shape
        if vny != ny:
            raise ValueError("pair_subpix: the two images must have one height")
        refine = refine if refine and refine != "none" else None
        mine = []
        try:
            maps = []
            for a, b, lo, hi in ((u, v, dmin, dmax), (v, u, -dmax, -dmin)):
                cv = self.costvolume_subpix_dev(a, b, lo, hi, s, interp, prefilter, distance, truncDist, census_win)
                mine.append(cv)
                w8 = self.weights_dev(a, aP2, aThresh) if aP2 != 1 else None
                mine.append(w8)
                _, out, cost = self.aggregate_dev(cv, P1, P2, NDIR, TSGM, use_fh, fix_overcount, w8=w8, refine=refine)
                mine += [out, cost]
                self.subpix_scale_dev(out, s, out=out)
                if median:
                    m = self.median_dev(out, median)
                    mine.append(m)
                    out = m
                maps.append((out, cost))
            (outL, costL), (outR, _) = maps
            chkL = self.leftright_dev(outL, outR, tau)
        except Exception:
            for o in mine:
                if o is not None:
                    o.free()
            raise
        for o in mine:
            if o is not None and o is not outL and o is not outR and o is not costL:
                o.free()
        return chkL, outL, outR, costL

    def update_ranges_dev(self, outoff, dminI, dmaxI, slack=3, radius=2):
        self._chk(self.lib.mgm_update_ranges_dev(self.h, outoff.h, dminI.h, dmaxI.h, slack, radius))

    # ---- coarse to fine (mgm_pyramid.hip) ----
    def zoom_out_dev(self, img, out=None):
        """2x2 mean with clamped indices: ((a + b) + (c + d)) * 0.25f -> an image of ((nx+1)/2, (ny+1)/2)."""
        h = C.c_void_p(out.h.value) if out is not None else C.c_void_p()
        self._chk(self.lib.mgm_zoom_out_dev(self.h, img.h, C.byref(h)))
        return out if out is not None else Image(self, h)

    def ranges_zoom_out_dev(self, lo, hi):
        """(floorf(0.5f * min lo), ceilf(0.5f * max hi)) over each 2x2 block: the base ranges of the next coarser level."""
        a, b = C.c_void_p(), C.c_void_p()
        self._chk(self.lib.mgm_ranges_zoom_out_dev(self.h, lo.h, hi.h, C.byref(a), C.byref(b)))
        return Image(self, a), Image(self, b)

    def ranges_from_coarse_dev(self, coarse_disp, lo, hi, slack=3, radius=2, want_hull=True):
        """lo / hi (the fine level's base ranges) are updated in place from the coarser level's map; returns the integer hull
        (min (int)lo, max (int)hi) or None."""
        a, b = C.c_int(), C.c_int()
        self._chk(self.lib.mgm_ranges_from_coarse_dev(self.h, coarse_disp.h, lo.h, hi.h, slack, radius,
                                                      C.byref(a) if want_hull else None, C.byref(b) if want_hull else None))
        return (a.value, b.value) if want_hull else None

    def multiscale_pair(self, u, v, dmin, dmax, nscales, P1=8.0, P2=32.0, NDIR=4, TSGM=4, use_fh=0, fix_overcount=1, aP2=1.0,
                        aThresh=5.0, prefilter="none", distance="ad", truncDist=float("inf"), census_win=3, refine="none",
                        iterations=1, median=0, testlrrl=1, tau=1.0, slack=3, radius=2, lo=None, hi=None, want_nolr=True,
                        want_right_nolr=False, consensus_min=0, consensus_tol=1.0, want_votes=False):
        """mgm_multiscale_pair_dev on device images u, v (P1 / P2 as given: multiply by the channel count yourself).
        Returns a dict of device images outL, costL, outR, costR (None with testlrrl=0), nolr (None unless wanted), outR_nolr
        (with want_right_nolr and testlrrl: the full-size right map before its left-right test, else None), votesL (with
        want_votes: the left run's consensus votes at full size, else None) and `levels`: one dict per level that ran,
        [0] = full size.  consensus_min > 0: the finest level's maps are NaN where fewer passes vote for them (tolerance
        consensus_tol).  Without consensus_min and want_votes the call passes the struct of an older caller."""
        _, ny, nx = u.shape
        _, vny, vnx = v.shape
        res = dict(outL=self.new_image(nx, ny), costL=self.new_image(nx, ny), outR=None, costR=None, nolr=None, outR_nolr=None)
        if testlrrl:
            res["outR"], res["costR"] = self.new_image(vnx, vny), self.new_image(vnx, vny)
            if want_right_nolr:
                res["outR_nolr"] = self.new_image(vnx, vny)
        if want_nolr:
            res["nolr"] = self.new_image(nx, ny)
        res["votesL"] = self.new_image(nx, ny) if want_votes else None
        n = C.c_int(0)
        lv = (MsLevel * 8)()
        p = MsParams(C.sizeof(MsParams), nscales, slack, radius, dmin, dmax, lo.h if lo is not None else None,
                     hi.h if hi is not None else None, P1, P2, NDIR, TSGM, use_fh, fix_overcount, aP2, aThresh, prefilter.encode(),
                     distance.encode(), truncDist, census_win, (refine or "none").encode(), iterations, median, testlrrl, tau,
                     C.pointer(n), lv, res["outR_nolr"].h if res["outR_nolr"] is not None else None)
        hnd = lambda im: im.h if im is not None else None
        if consensus_min or want_votes:  # the struct as it has grown: the same leading bytes, then the consensus fields
            big = MsParamsConsensus()
            C.memmove(C.byref(big), C.byref(p), C.sizeof(p))
            big.struct_size, big.consensus_tol, big.consensus_min, big.votesL = C.sizeof(big), consensus_tol, consensus_min, hnd(res["votesL"])
            p = C.cast(C.pointer(big), C.POINTER(MsParams)).contents
        r = self.lib.mgm_multiscale_pair_dev(self.h, u.h, v.h, C.byref(p), hnd(res["outL"]), hnd(res["costL"]), hnd(res["outR"]),
                                             hnd(res["costR"]), hnd(res["nolr"]))
        if r:
            for im in res.values():
                if im is not None:
                    im.free()
            self._chk(r)
        res["levels"] = [dict(nx=l.nx, ny=l.ny, vnx=l.vnx, vny=l.vny, hull=[(l.hull_min[k], l.hull_max[k]) for k in range(2)],
                              weighted=[bool(l.weighted[k]) for k in range(2)], batched=bool(l.batched)) for l in lv[:n.value]]
        return res

    def median_dev(self, img, radius, out=None):
        nch, ny, nx = img.shape
        out = out or self.new_image(nx, ny, nch)
        self._chk(self.lib.mgm_median_dev(self.h, img.h, radius, out.h))
        return out

    def leftright_dev(self, d, other, tau, out=None):
        _, ny, nx = d.shape
        out = out or self.new_image(nx, ny)
        self._chk(self.lib.mgm_leftright_dev(self.h, d.h, other.h, tau, out.h))
        return out

    def backproject_dev(self, u, v, disp, out=None):
        nch, ny, nx = u.shape
        out = out or self.new_image(nx, ny, nch)
        self._chk(self.lib.mgm_backproject_dev(self.h, u.h, v.h, disp.h, out.h))
        return out

    def aggregate_batch_dev(self, Cvs, P1, P2, NDIR, MGM, use_fh=0, fix_overcount=1, w8s=None, refine=None, outs=None,
                            outcosts=None, want_S=False):
        """mgm() over several volumes of identical geometry in one pass launch: ([S...] or None, [out...], [outcost...])."""
        n = len(Cvs)
        nx, ny, _, _ = Cvs[0].dims
        outs = outs or [self.new_image(nx, ny) for _ in range(n)]
        outcosts = outcosts or [self.new_image(nx, ny) for _ in range(n)]
        arr = lambda hs: (C.c_void_p * n)(*hs)
        S = (C.c_void_p * n)()
        self._chk(self.lib.mgm_aggregate_batch_dev(
            self.h, n, arr([cv.h for cv in Cvs]), arr([w.h for w in w8s]) if w8s is not None else None, P1, P2, NDIR, MGM,
            use_fh, fix_overcount, refine.encode() if refine else None, arr([o.h for o in outs]),
            arr([o.h for o in outcosts]), S if want_S else None))
        return ([CostVolume(self, C.c_void_p(h)) for h in S] if want_S else None), outs, outcosts

    def aggregate(self, Cv, P1, P2, NDIR, MGM, use_fh=0, fix_overcount=1, w8=None, refine=None, want_S=True):
        """mgm(): returns (S or None, out, outcost) with host arrays for out/outcost."""
        nx, ny, _, _ = Cv.dims
        out = np.empty((ny, nx), np.float32)
        outc = np.empty((ny, nx), np.float32)
        S = C.c_void_p()
        w = _f32(w8) if w8 is not None else None
        self._chk(self.lib.mgm_aggregate(self.h, Cv.h, _ptr(w) if w is not None else None, P1, P2, NDIR, MGM, use_fh,
                                         fix_overcount, refine.encode() if refine else None, _ptr(out), _ptr(outc),
                                         C.byref(S) if want_S else None))
        return (CostVolume(self, S) if want_S else None), out, outc

    def debug_lr(self, Cv, p):
        nx, ny, dmin, dmax = Cv.dims
        out = np.empty((ny, nx, dmax - dmin + 1), np.float32)
        self._chk(self.lib.mgm_debug_download_lr(self.h, p, _ptr(out)))
        return out

    def debug_lmin(self, Cv, slot, p):
        """The chunk minima of pass p of volume `slot` of the last aggregation call: (ny, nx, L/32), as the pruned search reads them."""
        nx, ny, dmin, dmax = Cv.dims
        out = np.empty((ny, nx, (dmax - dmin + 1) // 32), np.float32)
        self._chk(self.lib.mgm_debug_download_lmin(self.h, slot, p, _ptr(out)))
        return out

    def debug_rel_lr(self, p):
        """Test aid (mgm_debug_rel_lr_device_ptr): (device pointer of pass p's Lr volume [npix][slots] of the last range-proportional
        run, slots, bytes per cost code, floats between passes, device pointer of the records [npix][4] int32), or None where
        mgm_debug_download_lr would refuse."""
        slots, cb, stride, rec = C.c_int(0), C.c_int(0), C.c_longlong(0), C.c_void_p()
        ptr = self.lib.mgm_debug_rel_lr_device_ptr(self.h, p, C.byref(slots), C.byref(cb), C.byref(stride), C.byref(rec))
        return (ptr, slots.value, cb.value, stride.value, rec.value) if ptr else None

    def debug_lr_ptr(self, volume, p):
        """Test aid (mgm_debug_lr_device_ptr): (device pointer of pass p's Lr volume [npix][Lk] of volume `volume` of the last dense
        run, the label stride Lk, floats between passes), or None where the last aggregation was no dense run or has no such
        volume or pass."""
        Lk, stride = C.c_int(0), C.c_longlong(0)
        ptr = self.lib.mgm_debug_lr_device_ptr(self.h, volume, p, C.byref(Lk), C.byref(stride))
        return (ptr, Lk.value, stride.value) if ptr else None

    def debug_wta_rel_again_dev(self, Cv, NDIR, fix_overcount, refine, out=None, outcost=None, want_S=False):
        """Test aid (mgm_debug_wta_rel_again_dev): the un-windowed search of the last range-proportional aggregation of Cv again,
        on the Lr volumes as they lie in the workspace: (S or None, out, outcost) as device handles."""
        nx, ny, _, _ = Cv.dims
        mine = []  # the images made here: freed if the call fails
        for given in (out, outcost):
            if not given:
                mine.append(self.new_image(nx, ny))
        out, outcost = out or mine[0], outcost or mine[-1]
        S = C.c_void_p()
        try:
            self._chk(self.lib.mgm_debug_wta_rel_again_dev(self.h, Cv.h, NDIR, fix_overcount, refine.encode() if refine else None,
                                                           out.h, outcost.h, C.byref(S) if want_S else None))
        except Exception:
            for im in mine:
                im.free()
            raise
        return (CostVolume(self, S) if want_S else None), out, outcost

    def refine(self, S, method, out, outcost):
        out = np.array(out, np.float32, copy=True)
        outcost = np.array(outcost, np.float32, copy=True)
        self._chk(self.lib.mgm_refine(self.h, S.h, method.encode(), _ptr(out), _ptr(outcost)))
        return out, outcost

    # ---- direction sharding (see mgm_amd/dist.py) ----
    def aggregate_passes_dev(self, Cv, P1, P2, MGM, use_fh, first_pass, n_passes, w8=None):
        self._chk(self.lib.mgm_aggregate_passes_dev(self.h, Cv.h, w8.h if w8 is not None else None, P1, P2, MGM, use_fh,
                                                    first_pass, n_passes))

    def aggregate_passes_at_dev(self, Cv, P1, P2, MGM, use_fh, first_pass, n_passes, slot0, n_slots, NDIR_total, w8=None):
        self._chk(self.lib.mgm_aggregate_passes_at_dev(self.h, Cv.h, w8.h if w8 is not None else None, P1, P2, MGM, use_fh,
                                                       first_pass, n_passes, slot0, n_slots, NDIR_total))

    def lr_device_ptr(self, slot):
        return self.lib.mgm_lr_device_ptr(self.h, slot)

    def wta_rows_dev(self, Cv, row0, nrows, lr_slabs_ptr, NDIR, fix_overcount, refine, out_ptr, outcost_ptr):
        self._chk(self.lib.mgm_wta_rows_dev(self.h, Cv.h, row0, nrows, lr_slabs_ptr, NDIR, fix_overcount,
                                            refine.encode() if refine else None, out_ptr, outcost_ptr))

    def set_placement_tries(self, tries):
        self._chk(self.lib.mgm_ctx_set_placement_tries(self.h, tries))

    def probe_workspace(self, nstreams=8):
        g = C.c_float()
        self._chk(self.lib.mgm_debug_probe_workspace(self.h, nstreams, C.byref(g)))
        return g.value

    def wta_stats(self):
        """(pixels searched, chunks of 32 labels loaded) by the pruned winner searches of the last aggregation call; counted
        only while timing is on; (0, 0) when no search of that call was a pruned one."""
        px, ch = C.c_ulonglong(0), C.c_ulonglong(0)
        self._chk(self.lib.mgm_debug_wta_stats(self.h, C.byref(px), C.byref(ch)))
        return px.value, ch.value

    def last_pass_kernel(self):
        """The pass kernel instance the context's last aggregation launched, as a kernel trace spells it."""
        buf = C.create_string_buffer(128)
        self._chk(self.lib.mgm_debug_last_pass_kernel(self.h, buf, len(buf)))
        return buf.value.decode()

    def selftest_div3(self):
        n = C.c_ulonglong(0)
        self._chk(self.lib.mgm_selftest_div3(self.h, C.byref(n)))
        return n.value

    # ---- timing ----
    def timing(self, enable=True):
        self.lib.mgm_timing_enable(self.h, 1 if enable else 0)

    def timing_reset(self):
        self.lib.mgm_timing_reset(self.h)

    def timings(self):
        n = self.lib.mgm_timing_count(self.h)
        res = []
        for k in range(n):
            name, ms = C.c_char_p(), C.c_float()
            self._chk(self.lib.mgm_timing_get(self.h, k, C.byref(name), C.byref(ms)))
            res.append((name.value.decode(), ms.value))
        return res


def multiscale_levels(nx, ny, vnx=None, vny=None, nscales=1):
    """mgm_multiscale_levels: [(nx, ny, vnx, vny)] per level that would run, full size first (no device needed)."""
    L = load_library()
    dims = (C.c_int * 32)()
    S = L.mgm_multiscale_levels(nx, ny, nx if vnx is None else vnx, ny if vny is None else vny, nscales, dims)
    if S < 0:
        raise MgmError(-S, "mgm_multiscale_levels: sizes must be >= 1 and nscales 1..8")
    return [tuple(int(dims[4 * s + k]) for k in range(4)) for s in range(S)]


def multi_plan(n, NDIR, ny):
    """mgm_multi_plan: [(first_pass, n_passes, row0, nrows)] per rank (no device needed)."""
    L = load_library()
    a = [(C.c_int * n)() for _ in range(4)]
    r = L.mgm_multi_plan(n, NDIR, ny, *a)
    if r:
        raise MgmError(r, "mgm_multi_plan: bad arguments")
    return [tuple(int(x[k]) for x in a) for k in range(n)]


class Multi:
    """n GPUs of one node behind one handle (``mgm_multi``): direction sharding of one volume with an RCCL slab exchange."""

    def __init__(self, device_ids):
        self.lib = load_library()
        ids = (C.c_int * len(device_ids))(*device_ids)
        h = C.c_void_p()
        r = self.lib.mgm_multi_create(ids, len(device_ids), C.byref(h))
        if r:
            raise MgmError(r, "mgm_multi_create(%s) failed: %s" % (list(device_ids), self.lib.mgm_multi_last_error(None).decode()))
        self.h = h
        self.n = len(device_ids)
        self.ctx = [Context(_borrowed=self.lib.mgm_multi_ctx(h, k)) for k in range(self.n)]

    def transport(self):
        """"rccl", "peer" or "loopback" (mgm_multi_transport)."""
        return self.lib.mgm_multi_transport(self.h).decode()

    def aggregate_dev(self, Cvs, P1, P2, NDIR, MGM, use_fh, fix_overcount, refine, out, outc, w8s=None):
        """mgm_multi_aggregate into images on device 0 (returns when they are complete)."""
        arr = lambda hs: (C.c_void_p * self.n)(*hs)
        r = self.lib.mgm_multi_aggregate(self.h, arr([cv.h for cv in Cvs]), arr([w.h for w in w8s]) if w8s is not None else None, P1, P2,
                                         NDIR, MGM, use_fh, fix_overcount, refine.encode() if refine else None, out.h, outc.h)
        if r:
            raise MgmError(r, self.lib.mgm_multi_last_error(self.h).decode())

    def aggregate(self, Cvs, P1, P2, NDIR, MGM, use_fh=0, fix_overcount=1, refine=None, w8s=None):
        """mgm_multi_aggregate: returns host arrays (out, outcost)."""
        nx, ny, _, _ = Cvs[0].dims
        out, outc = self.ctx[0].new_image(nx, ny), self.ctx[0].new_image(nx, ny)
        self.aggregate_dev(Cvs, P1, P2, NDIR, MGM, use_fh, fix_overcount, refine, out, outc, w8s)
        res = out.download()[0], outc.download()[0]
        out.free(), outc.free()
        return res

    def close(self):
        if self.h:
            self.lib.mgm_multi_destroy(self.h)
            self.h = None
            for c in self.ctx:
                c.h = None
