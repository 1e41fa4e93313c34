"""A stateful random campaign on long-lived contexts: refills in place across formats, batches, weights, windowed searches, Lr
downloads and context operations (workspace limit, trim, pipeline, placement retries, free / recreate), every result against the
CPU oracle computed from a host-side model of what each handle holds (tests/stateful_model.py), never against a second context.

Each seed block has its own mgm_amd.Context.  On a mismatch the message names the seed, the operation, the last operations
(replayable) and whether the operation also fails on a fresh context with freshly filled handles (a state bug or a plain kernel
bug).  MGM_ERR_HIP or the watchdog error (MGM_ERR_INTERNAL) ends the campaign at once: no further GPU call in this process.
MGM_FUZZ_N / MGM_FUZZ_BASE lengthen it (blocks)."""
import math
import os

import numpy as np
import pytest

import mgm_amd
import stateful_model as sm
from helpers import labels_equal, ndiff
from mgm_amd import synth
from oracle.oracle import int_ranges, usable_cpus

pytestmark = pytest.mark.gpu

FUZZ_N = int(os.environ.get("MGM_FUZZ_N", "0"))
FUZZ_BASE = int(os.environ.get("MGM_FUZZ_BASE", "0"))
SEEDS = list(range(FUZZ_BASE, FUZZ_BASE + (FUZZ_N or sm.DEFAULT_BLOCKS)))
FATAL = (mgm_amd.MGM_ERR_HIP, mgm_amd.MGM_ERR_INTERNAL)
REACHED = set()  # kernel names over the whole run (the last test checks them)
COUNTS = {"ops": 0, "blocks": 0}


class Fatal(Exception):
    pass


class Mismatch(AssertionError):
    pass


def call(f, *a, **k):
    try:
        return f(*a, **k)
    except mgm_amd.MgmError as e:
        if e.code in FATAL:
            raise Fatal(str(e))
        raise


class World:
    """The block's images (host and device) and the oracle's view of every handle."""

    def __init__(self, seed, oracle):
        nx, ny, _ = sm.SHAPES[seed % len(sm.SHAPES)]
        self.nx, self.ny, self.oracle = nx, ny, oracle
        u, v, gt = synth.stereo_pair(nx, ny, sm.IMG_DMIN, 0, seed=900 + seed)
        uc, vc, _ = synth.stereo_pair(nx, ny, sm.IMG_DMIN, 0, seed=900 + seed, nch=3)
        self.pairs = {"g": (u, v), "c": (uc, vc), "h": (u + np.float32(0.5), v + np.float32(0.5))}
        self.gt = gt
        self.cache = {}

    def ranges(self, spec, L):
        dmin, dmax = sm.dims(L)
        rng = np.random.default_rng(spec["rseed"])
        h = spec["half"]
        lo = np.clip(self.gt - h + rng.integers(-2, 3, self.gt.shape), dmin, dmax).astype(np.float32)
        hi = np.clip(self.gt + h + rng.integers(-2, 3, self.gt.shape), dmin, dmax).astype(np.float32)
        return lo, np.maximum(hi, lo)

    def volume(self, spec):
        """(C on the hull, lo, hi) the oracle holds for a fill / upload spec."""
        key = repr(sorted((k, v) for k, v in spec.items() if k not in ("vol", "into")))
        if key in self.cache:
            return self.cache[key]
        L = spec["L"]
        dmin, dmax = sm.dims(L)
        if spec["op"] == "upload":
            C = synth.raw_volume(self.nx, self.ny, L, seed=spec["seed"], inf_frac=0.03)
            rng = np.random.default_rng(spec["seed"])
            C[rng.random(C.shape) < 0.01] = -0.0
            if spec["nan"]:
                C[rng.random(C.shape) < 0.002] = np.nan
            lo = np.full((self.ny, self.nx), dmin, np.int32)
            hi = np.full((self.ny, self.nx), dmax, np.int32)
        else:
            pre, dist, win, pk = sm.COSTS[spec["cost"]]
            u, v = self.pairs[pk]
            if spec["kind"] == "ragged":
                flo, fhi = self.ranges(spec, L)
                lo, hi = int_ranges(flo, fhi)
                C = self.oracle.costvolume_ranged(u, v, lo, hi, dmin, dmax, pre, dist, spec["trunc"], win)
            else:
                C = self.oracle.costvolume(u, v, dmin, dmax, pre, dist, spec["trunc"], win)
                lo = np.full((self.ny, self.nx), dmin, np.int32)
                hi = np.full((self.ny, self.nx), dmax, np.int32)
        self.cache[key] = (C, lo, hi)
        return self.cache[key]

    def weights(self, op):
        if op["kind"] is None:
            return None
        rng = np.random.default_rng(op["seed"])
        if op["kind"] == "w2":
            return self.oracle.weights(self.pairs["g"][0], 4.0, 12.0)
        if op["kind"] == "ones":
            return np.ones((8, self.ny, self.nx), np.float32)
        return rng.choice(np.array([1.0, 2.5, 4.0], np.float32), size=(8, self.ny, self.nx), p=[0.6, 0.25, 0.15])


def expected_agg(world, op, specs, w8h, k):
    """Oracle (S, out, outcost) of volume k of an aggregation, refined as asked."""
    spec = specs[op["vols"][k]]
    C, lo, hi = world.volume(spec)
    dmin, _ = sm.dims(spec["L"])
    o = world.oracle
    if spec.get("kind") == "ragged":
        S, out, outc = o.mgm_ranged(C, dmin, lo, hi, op["P1"], op["P2"], op["NDIR"], op["MGM"], op["FH"], op["fix"], w8h)
        if op["refine"]:
            out, outc = o.refine_ranged(S, dmin, lo, hi, op["refine"], out, outc)
    else:
        S, out, outc = o.mgm(C, dmin, op["P1"], op["P2"], op["NDIR"], op["MGM"], op["FH"], op["fix"], w8h)
        if op["refine"]:
            out, outc = o.refine(S, dmin, op["refine"], out, outc)
    return S, out, outc, lo, hi


class Runner:
    def __init__(self, seed, oracle, gen):
        self.seed, self.gen, self.oracle = seed, gen, oracle
        self.world = World(seed, oracle)
        self.ctx = mgm_amd.Context(0)
        self.dev = {}  # volume name -> CostVolume
        self.specs = {}  # volume name -> what it holds (the op that filled it)
        self.imgs = {}
        self.w = None
        self.wspec = None
        self.pending = []  # (op index, op, outputs, expectations): checked at the next synchronisation point
        self.lastsol = {}  # volume name -> the oracle's labels of its last aggregation (windows for wta)
        self.pipeline = 1
        self.limit = 0
        self.refused = set()  # aggregations refused as documented: what follows them is not checked against them
        self.aggw = {}
        self.ctx.timing(True)

    def close(self):
        os.environ.pop("MGM_HIP_REL", None)
        for h in list(self.dev.values()) + list(self.imgs.values()) + ([self.w] if self.w else []):
            try:
                h.free()
            except mgm_amd.MgmError:
                pass
        self.ctx.close()

    def img(self, pk, side):
        key = (pk, side)
        if key not in self.imgs:
            self.imgs[key] = call(self.ctx.upload_image, self.world.pairs[pk][side])
        return self.imgs[key]

    def harvest(self):
        REACHED.update(n for n, _ in self.ctx.timings())
        self.ctx.timing_reset()

    # ---- operations ----
    def fill(self, op):
        L = op["L"]
        dmin, dmax = sm.dims(L)
        pre, dist, win, pk = sm.COSTS[op["cost"]]
        into = self.dev.get(op["vol"]) if op["into"] else None
        if op["kind"] == "ragged":
            lo, hi = self.world.ranges(op, L)
            dlo, dhi = call(self.ctx.upload_image, lo[None]), call(self.ctx.upload_image, hi[None])
            cv = call(self.ctx.costvolume_ranged_dev, self.img(pk, 0), self.img(pk, 1), dlo, dhi, dmin, dmax, pre, dist, op["trunc"], win, into=into)
            dlo.free(), dhi.free()
        else:
            cv = call(self.ctx.costvolume_dev, self.img(pk, 0), self.img(pk, 1), dmin, dmax, pre, dist, op["trunc"], win, into=into)
        self.dev[op["vol"]] = cv
        self.specs[op["vol"]] = op

    def upload(self, op):
        C, _, _ = self.world.volume(op)
        self.dev[op["vol"]] = call(self.ctx.upload_volume, C, sm.dims(op["L"])[0])
        self.specs[op["vol"]] = op

    def weights(self, op):
        self.wspec = op
        if op["kind"] is None:
            return
        if op["into"] and self.w is not None:
            call(self.ctx.weights_dev, self.img("g", 0), 4.0, 12.0, into=self.w)
            return
        if self.w is not None:
            self.w.free()
        if op["kind"] == "w2":
            self.w = call(self.ctx.weights_dev, self.img("g", 0), 4.0, 12.0)
        else:
            self.w = call(self.ctx.upload_image, self.world.weights(op))

    def agg(self, i, op):
        cvs = [self.dev[k] for k in op["vols"]]
        w8 = self.w if op["w"] is not None else None
        if op["rel"] is None:
            os.environ.pop("MGM_HIP_REL", None)
        else:
            os.environ["MGM_HIP_REL"] = op["rel"]
        try:
            if len(cvs) == 1 and i % 2:
                S, o, c = call(self.ctx.aggregate_dev, cvs[0], op["P1"], op["P2"], op["NDIR"], op["MGM"], op["FH"], op["fix"], w8, op["refine"],
                               want_S=op["wantS"])
                Ss, outs, outcs = ([S] if S is not None else None), [o], [c]
            else:
                Ss, outs, outcs = call(self.ctx.aggregate_batch_dev, cvs, op["P1"], op["P2"], op["NDIR"], op["MGM"], op["FH"], op["fix"],
                                       [w8] * len(cvs) if w8 is not None else None, op["refine"], want_S=op["wantS"])
        except mgm_amd.MgmError as e:
            ragged = self.specs[op["vols"][0]].get("kind") == "ragged"
            if e.code == mgm_amd.MGM_ERR_UNSUPPORTED and ragged and op["FH"] and op["MGM"] == 2 and w8 is None:
                self.refused.add(id(op))
                return  # (update_cost2_trunclinear on a ragged volume where the second build does not take it: refused, documented)
            raise Mismatch("aggregation refused: %s" % e)
        finally:
            os.environ.pop("MGM_HIP_REL", None)
        w8h = self.world.weights(self.wspec) if w8 is not None else None
        self.aggw[id(op)] = w8h  # (the weights of THIS launch: a later weights op replaces the context's image)
        specs = {k: self.specs[k] for k in op["vols"]}
        self.pending.append((i, op, specs, w8h, Ss, outs, outcs))
        if self.pipeline <= 1:
            self.check_pending()

    def check_pending(self):
        pend, self.pending = self.pending, []
        for i, op, specs, w8h, Ss, outs, outcs in pend:
            for k, name in enumerate(op["vols"]):
                S, eo, ec, lo, hi = expected_agg(self.world, op, specs, w8h, k)
                go, gc = call(outs[k].download)[0], call(outcs[k].download)[0]
                self.lastsol[name] = (eo, ec, specs[name])
                if ndiff(gc, ec) or not labels_equal(go, eo, ec):
                    raise Mismatch("op %d volume %s: costs differ at %d pixels, labels at %d" % (i, name, ndiff(gc, ec), ndiff(go, eo)))
                if Ss is not None:
                    gS = call(Ss[k].download)
                    own = sm_own(lo, hi, sm.dims(specs[name]["L"])[0], gS.shape[2])
                    d = int(np.sum((gS.view(np.uint32) != S.view(np.uint32)) & ~(np.isnan(gS) & np.isnan(S)) & own))
                    if d:
                        raise Mismatch("op %d volume %s: S differs at %d words" % (i, name, d))
                    Ss[k].free()
                outs[k].free(), outcs[k].free()
        self.harvest()

    def wta(self, i, op):
        name = op["vol"]
        spec = self.specs[name]
        L = spec["L"]
        dmin, dmax = sm.dims(L)
        rng = np.random.default_rng(op["seed"])
        base = self.lastsol.get(name, (np.full((self.world.ny, self.world.nx), float(dmin), np.float32), None, None))[0]
        base = np.where(np.isfinite(base), base, dmin)
        wl = np.clip(np.floor(base) - rng.integers(1, 9, base.shape), dmin - 3, dmax).astype(np.float32)
        wh = np.clip(wl + rng.integers(2, 16, base.shape), wl, dmax + 3).astype(np.float32)
        dwl, dwh = call(self.ctx.upload_image, wl[None]), call(self.ctx.upload_image, wh[None])
        agg = op["agg"]
        if agg is not None and id(agg) in self.refused:
            return
        try:
            o, c = call(self.ctx.wta_windowed_dev, self.dev[name], op["NDIR"], agg["fix"] if agg else 1, op["refine"], dwl, dwh)
        except mgm_amd.MgmError as e:
            if e.code == mgm_amd.MGM_ERR_INVALID and op["expect"] in ("refuse", "exact_or_refuse"):
                return
            raise Mismatch("windowed search: %s (expected %s)" % (e, op["expect"]))
        finally:
            dwl.free(), dwh.free()
        got = (call(o.download)[0], call(c.download)[0])
        o.free(), c.free()
        if op["expect"] == "refuse":
            raise Mismatch("windowed search on a volume outside the last aggregation was not refused")
        C, lo, hi = self.world.volume(spec)
        slo, shi = int_ranges(wl, wh)
        shmin, shmax = int(slo.min()), int(shi.max())
        w8h = self.aggw[id(agg)]
        S2, oo, cc = self.oracle.mgm_ranged(C, dmin, lo, hi, agg["P1"], agg["P2"], op["NDIR"], agg["MGM"], agg["FH"], agg["fix"], w8h,
                                           (slo, shi, shmin, shmax))
        if op["refine"]:
            oo, cc = self.oracle.refine_ranged(S2, shmin, slo, shi, op["refine"], oo, cc)
        if ndiff(got[1], cc) or not labels_equal(got[0], oo, cc):
            raise Mismatch("windowed search differs: costs at %d pixels, labels at %d" % (ndiff(got[1], cc), ndiff(got[0], oo)))

    def lr(self, i, op):
        agg = op["agg"]
        if id(agg) in self.refused:
            return
        name = agg["vols"][0]
        spec = self.specs[name]
        C, lo, hi = self.world.volume(spec)
        dmin, _ = sm.dims(spec["L"])
        w8h = self.aggw[id(agg)]
        if spec.get("kind") == "ragged":
            _, _, _, lra = self.oracle.mgm_ranged(C, dmin, lo, hi, agg["P1"], agg["P2"], agg["NDIR"], agg["MGM"], agg["FH"], agg["fix"], w8h,
                                                  want_S=False, dump_lr=tuple(op["passes"]))
        else:
            lra = self.oracle.mgm(C, dmin, agg["P1"], agg["P2"], agg["NDIR"], agg["MGM"], agg["FH"], agg["fix"], w8h, dump_lr=True)[3][op["passes"]]
        own = sm_own(lo, hi, dmin, C.shape[2])
        for n, p in enumerate(op["passes"]):
            got = call(self.ctx.debug_lr, self.dev[name], p)
            d = int(np.sum((got.view(np.uint32) != lra[n].view(np.uint32)) & ~(np.isnan(got) & np.isnan(lra[n])) & own))
            if d:
                raise Mismatch("Lr of pass %d differs at %d words" % (p, d))

    def step(self, i, op):
        k = op["op"]
        if k == "fill":
            self.fill(op)
        elif k == "upload":
            self.upload(op)
        elif k == "free":
            call(self.dev.pop(op["vol"]).free)
            self.lastsol.pop(op["vol"], None)
        elif k == "weights":
            self.weights(op)
        elif k == "agg":
            self.agg(i, op)
        elif k == "wta":
            self.check_pending()
            self.wta(i, op)
        elif k == "lr":
            self.lr(i, op)
        elif k == "limit":
            nx, ny = self.world.nx, self.world.ny
            self.limit = op["units"]
            call(self.ctx.set_workspace_limit, int(op["units"] * 1.1 * 4 * 8 * nx * ny * 151))  # (room for one or two volumes' Lr volumes)
        elif k == "trim":
            call(self.ctx.trim)
        elif k == "pipeline":
            call(self.ctx.set_pipeline, op["depth"])
            self.pipeline = op["depth"]
            if op["depth"] == 1:
                self.check_pending()
        elif k == "tries":
            call(self.ctx.set_placement_tries, op["n"])
        elif k == "sync":
            call(self.ctx.synchronize)
            self.check_pending()


def sm_own(lo, hi, dmin, L):
    d = dmin + np.arange(L)[None, None, :]
    return (d >= lo[..., None]) & (d <= hi[..., None])


def replay_alone(seed, oracle, gen, i):
    """The failing operation on a fresh context whose handles are filled fresh with what the model says they hold."""
    ops = gen.ops
    op = ops[i]
    r = Runner(seed, oracle, gen)
    try:
        holds, wop = {}, None
        agg_at = next((j for j in range(i) if ops[j] is op.get("agg")), i)
        for j in range(i):
            if ops[j]["op"] in ("fill", "upload"):
                holds[ops[j]["vol"]] = ops[j]
            elif ops[j]["op"] == "free":
                holds.pop(ops[j]["vol"], None)
            elif ops[j]["op"] == "weights" and j < agg_at:  # (the weights the replayed launch had)
                wop = ops[j]
        if wop:
            r.weights(dict(wop, into=False))
        for name, f in holds.items():
            (r.upload if f["op"] == "upload" else r.fill)(dict(f, into=False))
        if op["op"] in ("wta", "lr"):
            agg = op["agg"]
            if agg is None or any(v not in holds for v in agg["vols"]):
                return "not replayable alone"
            r.agg(i, agg)
            if op["op"] == "wta" and op["expect"] == "refuse":
                return "not replayable alone (a refusal depends on the history)"
        r.step(i, op)
        r.check_pending()
        return "passes on a fresh context (a STATE bug)"
    except Fatal as e:
        return "fatal on a fresh context: %s" % e
    except (Mismatch, mgm_amd.MgmError) as e:
        return "fails on a fresh context too (a kernel bug): %s" % e
    finally:
        r.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_stateful_campaign(oracle, seed):
    gen = sm.generate(seed)
    oracle.set_threads(min(16, usable_cpus()))
    r = Runner(seed, oracle, gen)
    i = -1
    try:
        for i, op in enumerate(gen.ops):
            r.step(i, op)
        r.check_pending()
    except Fatal:
        r = None  # (no further GPU call: not even a free, nor the replay)
        raise
    except (Mismatch, mgm_amd.MgmError) as e:
        r.close()
        r = None
        alone = replay_alone(seed, oracle, gen, i)
        tail = "\n".join("  [%d] %s" % (j, sm.fmt_op(gen.ops[j])) for j in range(max(0, i - 10), i + 1))
        pytest.fail("seed %d op %d: %s\nreplayed alone: %s\nlast operations:\n%s" % (seed, i, e, alone, tail))
    finally:
        if r is not None:
            r.close()
        oracle.set_threads(1)
    COUNTS["ops"] += len(gen.ops)
    COUNTS["blocks"] += 1


def test_stateful_campaign_reached_every_kernel():
    """Runs after the campaign (collection order): the kernels it claims to exercise all ran."""
    if COUNTS["blocks"] != len(SEEDS):
        pytest.fail("the campaign did not complete (%d of %d blocks)" % (COUNTS["blocks"], len(SEEDS)))
    missing = [k for k in sm.KERNELS if k not in REACHED]
    assert not missing, (missing, sorted(REACHED))
