"""The RANGE-PROPORTIONAL winner search and S (k_wta_rel<SPL,CB>, k_rel_S; mgm_wta.hip) on CRAFTED Lr volumes: the classes of
tests/wta_crafted.py laid at every pixel's own range (tests/wta_rel_crafted.py) -- engineered ties, winners on lo, lo+1, hi-2, hi-1
and hi, sums whose value depends on the pass order, overflow, negative, non-finite, denormal and signed-zero values, flat pixels
and pixels without a finite label.

No such value goes through a pass kernel.  Per format (64 / 128 slots x 1 / 2 / 4 bytes per cost code) ONE tame aggregation of
natural costs runs k_pass_rel; then the workspace is overwritten through mgm_debug_rel_lr_device_ptr -- the slots a pixel does not
own with a poison value -- and searched again: mgm_debug_wta_rel_again_dev (the un-windowed search of run_rel, and k_rel_S) and
mgm_wta_windowed_dev (windows placed at each pixel's own range).  Everything is compared bit for bit (NaN = NaN) with the numpy
restatement and the oracle's refinements, pinned on the CPU by tests/test_wta_crafted_ref.py and tests/test_wta_rel_crafted_ref.py.
The context is the file's own, and trimmed after every use: an overwritten volume is never read by anything later."""
import os

import numpy as np
import pytest
import torch

import mgm_amd
import wta_crafted as W
import wta_plan_model as PM
import wta_rel_crafted as R
from helpers import ndiff
from mgm_amd import dist as mdist
from mgm_amd import synth

pytestmark = pytest.mark.gpu

FORMATS = list(R.CASES)
CLASSES = list(W.LR_CLASSES)
REACHED = {}  # instance of k_wta_rel -> the format that reached it
DECLARED = ["k_wta_rel<%d,%d>" % (spl, cb) for spl in (4, 8) for cb in (1, 2, 4)]


@pytest.fixture(scope="module")
def own():
    try:
        c = mgm_amd.Context(0)
    except mgm_amd.MgmError as e:
        if e.code == mgm_amd.MGM_ERR_HIP:
            pytest.skip("no MI355X in this box (mgm_ctx_create: MGM_ERR_HIP)")
        raise
    yield c
    c.close()


class Prepared:
    """One format: its volume built on the device, ONE tame aggregation through k_pass_rel (asserted from the timing table), the
    format asserted from the accessor, the records read back."""

    def __init__(self, own, oracle, name):
        k = self.k = R.case(name)
        self.own, self.C = own, R.costs(oracle, k)
        self.npix = k["nx"] * k["ny"]
        os.environ["MGM_HIP_REL"] = "2"
        try:
            self.cv = own.costvolume(k["u"], k["v"], k["flo"], k["fhi"], "none", k["dist"], float("inf"), k["win"])
            assert self.cv.dims == (k["nx"], k["ny"], k["dmin"], k["dmin"] + k["L"] - 1)
            own.timing(True)
            own.timing_reset()
            _, o, c = own.aggregate_dev(self.cv, k["P1"], k["P2"], k["NDIR"], k["MGM"], k["FH"], 1, None, None)
            own.synchronize()
            names = [n for n, _ in own.timings()]
            own.timing(False)
        finally:
            os.environ.pop("MGM_HIP_REL", None)
        o.free(), c.free()
        assert "k_pass_rel" in names and "k_wta" in names, names
        self.ptr = []
        for p in range(k["NDIR"]):
            got = own.debug_rel_lr(p)
            assert got, "mgm_debug_rel_lr_device_ptr(%d) is null" % p
            ptr, slots, cb, stride, rec = got
            assert (slots, cb) == (k["slots"], k["cb"]), (name, slots, cb)  # the format, from the accessor
            assert stride >= self.npix * slots and (p == 0 or ptr == self.ptr[0] + 4 * stride * p), (name, p, stride)
            self.ptr.append(ptr)
        assert own.debug_rel_lr(k["NDIR"]) is None and own.debug_rel_lr(-1) is None
        self.instance = PM.instance("rel", PM.wta_rel((self.npix, 256, slots, cb)))
        REACHED.setdefault(self.instance, name)
        # the records: slot 0 is the label below the range
        records = mdist.device_view(rec, (self.npix, 4)).view(torch.int32).cpu().numpy()
        assert np.array_equal(records, R.records(k["dmin"], k["lo"], k["hi"])), name

    def overwrite(self, lr, poison):
        k = self.k
        rel = R.to_rel(lr, k["dmin"], k["lo"], k["hi"], k["slots"], poison)
        self.own.synchronize()
        for p in range(k["NDIR"]):
            mdist.device_view(self.ptr[p], (self.npix, k["slots"])).copy_(torch.from_numpy(np.ascontiguousarray(rel[p])).cuda())
        torch.cuda.synchronize()

    def crafted(self, cls):
        k = self.k
        return R.crafted(cls, R.SEED[cls], k["NDIR"], k["dmin"], k["L"], k["lo"], k["hi"])

    def again(self, fix, refine):
        """(out, outcost, S) of the un-windowed search on the workspace as it lies"""
        S, o, c = self.own.debug_wta_rel_again_dev(self.cv, self.k["NDIR"], fix, refine, want_S=True)
        got = o.download()[0], c.download()[0], S.download()
        o.free(), c.free(), S.free()
        return got

    def windowed(self, fix, refine, dlo, dhi):
        o, c = self.own.wta_windowed_dev(self.cv, self.k["NDIR"], fix, refine, dlo, dhi)
        got = o.download()[0], c.download()[0]
        o.free(), c.free()
        return got

    def window_images(self):
        wl, wh = R.windows(self.k["lo"], self.k["hi"])
        fwl, fwh = R.off_by_fractions(wl, wh)
        return fwl, fwh, self.own.upload_image(fwl), self.own.upload_image(fwh)

    def close(self, *handles):
        self.own.trim()  # nothing later reads the overwritten volumes
        for h in handles + (self.cv,):
            h.free()


def poison_of(j):
    return list(R.POISONS.values())[j % 4]


@pytest.mark.parametrize("name", FORMATS)
def test_round_trip_through_the_download(own, oracle, name):
    """mgm_debug_download_lr gives the crafted values back on the labels a pixel owns and +INF elsewhere, whatever the other slots hold"""
    p = Prepared(own, oracle, name)
    try:
        k = p.k
        mask = R.own_mask(k["dmin"], k["L"], k["lo"], k["hi"])
        for j, cls in enumerate(CLASSES):
            lr = p.crafted(cls)
            p.overwrite(lr, poison_of(j))
            for q in range(k["NDIR"]):
                assert ndiff(own.debug_lr(p.cv, q), np.where(mask, lr[q], np.inf)) == 0, (name, cls, q)
    finally:
        p.close()


@pytest.mark.parametrize("name", FORMATS)
def test_unwindowed_search_and_S(own, oracle, name):
    """mgm_debug_wta_rel_again_dev: out, outcost and S for both settings of the fix and every refinement, every class"""
    p = Prepared(own, oracle, name)
    try:
        k = p.k
        for j, cls in enumerate(CLASSES):
            lr = p.crafted(cls)
            R.floors(cls, lr, p.C, k)
            p.overwrite(lr, poison_of(j + 1))
            for fix in (0, 1):
                S = R.masked_S(lr, p.C, k["dmin"], k["lo"], k["hi"], k["NDIR"], fix)
                want_S = R.expect_S(lr, p.C, k["dmin"], k["lo"], k["hi"], k["NDIR"], fix)
                for refine in W.REFINEMENTS:
                    want_o, want_c = R.expect_search(oracle, S, k["dmin"], k["flo"], k["fhi"], k["NDIR"], fix, refine)
                    got_o, got_c, got_S = p.again(fix, refine)
                    what = (name, p.instance, cls, fix, refine)
                    assert ndiff(got_c, want_c) == 0, what + ("cost",)
                    assert ndiff(got_o, want_o) == 0, what + ("disparity",)
                    assert ndiff(got_S, want_S) == 0, what + ("S",)
    finally:
        p.close()


@pytest.mark.parametrize("name", FORMATS)
def test_windowed_search(own, oracle, name):
    """mgm_wta_windowed_dev with the seven window kinds placed at each pixel's own range: both settings of the fix, every refinement"""
    p = Prepared(own, oracle, name)
    fwl, fwh, dlo, dhi = p.window_images()
    try:
        k = p.k
        for j, cls in enumerate(CLASSES):
            lr = p.crafted(cls)
            p.overwrite(lr, poison_of(j + 2))
            for fix in (0, 1):
                S = R.masked_S(lr, p.C, k["dmin"], k["lo"], k["hi"], k["NDIR"], fix)
                for refine in W.REFINEMENTS:
                    want_o, want_c = R.expect_search(oracle, S, k["dmin"], fwl, fwh, k["NDIR"], fix, refine)
                    got_o, got_c = p.windowed(fix, refine, dlo, dhi)
                    what = (name, p.instance, cls, fix, refine)
                    assert ndiff(got_c, want_c) == 0, what + ("cost",)
                    assert ndiff(got_o, want_o) == 0, what + ("disparity",)
    finally:
        p.close(dlo, dhi)


@pytest.mark.parametrize("name", FORMATS)
def test_poison_invariance(own, oracle, name):
    """the same calls with NaN, -INF, -1e30 and +0 in the slots a pixel does not own: every output bit-identical.  Outside its own
    [lo, hi] the search may read the record, never the slot."""
    p = Prepared(own, oracle, name)
    fwl, fwh, dlo, dhi = p.window_images()
    try:
        for cls in CLASSES:
            lr = p.crafted(cls)
            first = None
            for pname, poison in R.POISONS.items():
                p.overwrite(lr, poison)
                maps = []
                for fix in (0, 1):
                    for refine in W.REFINEMENTS:
                        maps += list(p.again(fix, refine)) + list(p.windowed(fix, refine, dlo, dhi))
                bits = [np.ascontiguousarray(m).view(np.uint32) for m in maps]
                if first is None:
                    first = bits
                else:
                    bad = [n for n, (a, b) in enumerate(zip(first, bits)) if not np.array_equal(a, b)]
                    assert not bad, (name, p.instance, cls, pname, bad)
    finally:
        p.close(dlo, dhi)


def test_the_aids_refuse_what_they_should(own, oracle):
    """the accessor answers null, and the second search MGM_ERR_INVALID, without a range-proportional run of that volume and pass count"""
    assert own.debug_rel_lr(0) is None  # (trimmed: no run)
    p = Prepared(own, oracle, "tiny")
    k = p.k
    other = None
    try:
        with pytest.raises(mgm_amd.MgmError) as e:
            own.debug_wta_rel_again_dev(p.cv, k["NDIR"] + 1, 1, None)  # another pass count than that run's
        assert e.value.code == mgm_amd.MGM_ERR_INVALID
        other = own.upload_volume(synth.raw_volume(16, 8, 32, seed=2), k["dmin"])
        with pytest.raises(mgm_amd.MgmError) as e:
            own.debug_wta_rel_again_dev(other, k["NDIR"], 1, None)  # a volume that was not part of it
        assert e.value.code == mgm_amd.MGM_ERR_INVALID
        _, o, c = own.debug_wta_rel_again_dev(p.cv, k["NDIR"], 1, None)  # (and the run is still there)
        o.free(), c.free()
        # a dense aggregation since: the range-proportional run is no longer the context's last
        _, o, c = own.aggregate_dev(other, 8.0, 32.0, k["NDIR"], 3, 0, 1, None, None)
        o.free(), c.free()
        assert own.debug_rel_lr(0) is None
        with pytest.raises(mgm_amd.MgmError) as e:
            own.debug_wta_rel_again_dev(p.cv, k["NDIR"], 1, None)
        assert e.value.code == mgm_amd.MGM_ERR_INVALID
    finally:
        p.close(*([other] if other else []))
    assert own.debug_rel_lr(0) is None


def test_every_instance_was_reached(own):
    """(the last test of the file, and like the others one for a device: every format asserted its instance from the accessor's format and plan_wta_rel's restatement)"""
    for inst in sorted(REACHED):
        print(inst, "<-", REACHED[inst])
    missing = [inst for inst in DECLARED if inst not in REACHED]
    assert not missing, missing
