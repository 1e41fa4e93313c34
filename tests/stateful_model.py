"""Operation generator and handle model of the stateful campaign (tests/test_gpu_stateful.py).

Plain Python, no device: tests/test_stateful_gen.py checks on the CPU that generation is deterministic, that the default
seeds reach the coverage and collision counts the campaign claims, and that no operation touches a freed handle or makes a
call whose behaviour the ABI leaves undefined.

A block is a list of operations (dicts) over a small pool of long-lived handles of one image shape: stereo pairs ("g" grey,
"c" colour, "h" half-integer grey), volumes "V0".."V5" of a fixed geometry each, one weight image "W".  The generator keeps a
model of what every handle holds, so every operation it emits is legal and its expected outcome (an exact result or a clean
refusal) is decided by the model alone.  It seeks collisions: most aggregations keep the previous launch's shape and batch size
and change ONE planner input."""
import math

import numpy as np

# (nx, ny, label counts the volumes of this shape may have): a landscape image (the column passes walk with exchanged roles),
# a tall one (several bands per pass), a wide one (two strips per line where the anti-diagonal bands do not fit)
SHAPES = [(150, 56, (64, 128, 151)), (60, 190, (64, 128, 256)), (200, 40, (64, 128, 151))]
IMG_DMIN = -36  # disparities of the synthetic pairs: inside every volume's labels
NVOL = 8
DEFAULT_BLOCKS = 6
DEFAULT_OPS = 40

# cost functions: name -> (prefilter, distance, census window, pair kind)
COSTS = {
    "census1": ("none", "census", 5, "g"),
    "census1h": ("none", "census", 3, "h"),
    "census2": ("none", "census", 7, "g"),
    "ad": ("none", "ad", 3, "g"),
    "ad3": ("none", "ad", 3, "c"),
    "sd": ("none", "sd", 3, "g"),
    "adh": ("none", "ad", 3, "h"),
    "sobel": ("sobelx", "ad", 3, "g"),
    "ncc": ("none", "ncc", 3, "g"),
    "btad": ("none", "btad", 3, "g"),
    "census3c": ("none", "census", 3, "c"),
}
TRUNCS = [math.inf, math.inf, math.inf, 20.0, 7.5, 0.0, -0.0, -2.0, math.nan]
# planner inputs that adjacent launches are made to differ in (one at a time)
AXES = ("fh", "tsgm34", "fh2", "cb", "slots", "weights", "subv", "passes", "wantS")
# the formats a refill moves a volume between
FORMATS = ("c8", "d1", "d2", "pad", "f32", "r64", "r128")
KERNELS = ("k_pass2", "k_pass", "k_pass_exact", "k_pass_rel", "k_rel_gather", "k_rel_S", "k_pad", "k_expand")


def dims(L):
    dmin = -(3 * L // 4)
    return dmin, dmin + L - 1


def fill_format(spec, L):
    """The format class a fill leaves the volume in (for the coverage count; what the library picks may be wider)."""
    cost, trunc = spec["cost"], spec["trunc"]
    clean = trunc == math.inf or (trunc >= 0 and not math.copysign(1, trunc) < 0 and float(trunc).is_integer())
    if spec["kind"] == "ragged":
        w = spec["half"] * 2 + 1
        return "r64" if w <= 56 else ("r128" if w <= 120 else "f32")
    if not clean or cost in ("ncc", "btad", "census2", "adh"):  # (census1h: bit counts, whatever the pixels are; census3c: 24 bits, one word)
        return "f32"
    if L == 151:
        return "pad"
    if cost in ("census1", "census1h", "census3c"):
        return "c8"
    return "d2" if cost in ("ad3", "sd") else "d1"


def planner_sig(op, model):
    """What the planner sees of an aggregation (for the collision count)."""
    v0 = model["vols"][op["vols"][0]]
    return dict(shape=model["shape"], nb=len(op["vols"]), fh=op["FH"], tsgm34=op["MGM"], fh2=int(op["FH"] and op["MGM"] == 2),
                cb=v0["cb"], slots=v0["fmt"] if v0["fmt"] in ("r64", "r128") else "hull", weights=op["w"] or "none", subv=v0["L"],
                passes=op["NDIR"], wantS=op["wantS"])


def cost_bytes(cost, trunc, ragged=False):
    """Bytes per cost of the copy the pass kernels read: one (bit counts, grey differences), two (colour / squared differences; the
    gathered copy of a ragged volume of differences of filtered images), four."""
    clean = trunc == math.inf or (trunc >= 0 and math.copysign(1, trunc) > 0 and float(trunc).is_integer())
    if not clean or cost not in ("census1", "census1h", "census3c", "ad", "sobel", "ad3", "sd"):
        return 4
    return 2 if cost in ("ad3", "sd") or (ragged and cost == "sobel") else 1


def _new_vol(L, fmt="none"):
    return dict(L=L, alive=False, kind=None, fmt=fmt, gen=0, nan=False)


class Generator:
    def __init__(self, seed, nops=DEFAULT_OPS):
        self.seed, self.nops = seed, nops
        self.rng = np.random.default_rng(7919 * seed + 17)
        nx, ny, Ls = SHAPES[seed % len(SHAPES)]
        r = self.rng
        self.model = dict(shape=(nx, ny), vols={"V%d" % k: _new_vol(int(Ls[k % len(Ls)])) for k in range(NVOL)}, w=None, gen=0,
                          pipeline=1, limit=0, last=None, maybe=set(), pending_lr=False, prev_agg=None)
        self.ops = []
        self.sigs = []  # planner signatures of the aggregations, in order
        self.transitions = set()  # (from format, to format) of refills
        self.ru_r = 0  # ragged -> uniform -> ragged on one handle
        self.history = {k: [] for k in self.model["vols"]}
        del r

    # ---- helpers ----
    def choice(self, seq, p=None):
        return seq[int(self.rng.choice(len(seq), p=p))]

    def alive(self):
        return [k for k, v in self.model["vols"].items() if v["alive"]]

    def emit(self, op):
        self.ops.append(op)
        return op

    def bump(self, name):
        m = self.model
        m["gen"] += 1
        m["vols"][name]["gen"] = m["gen"]
        m["maybe"].discard(name)
        if m["last"] and name in m["last"]["vols"]:
            m["last"]["stale"].add(name)

    # ---- operations ----
    def fill(self, name, kind=None, cost=None, half=None, trunc=None):
        m, r = self.model, self.rng
        v = m["vols"][name]
        L = v["L"]
        kind = kind or self.choice(["uniform", "ragged"], p=[0.45, 0.55])
        if kind == "uniform" and r.random() < 0.08:
            return self.upload(name)
        cost = cost or self.choice(list(COSTS))
        if half is None:
            half = int(self.choice([int(r.integers(3, 20)), int(r.integers(34, 58)), int(r.integers(64, 80))], p=[0.55, 0.35, 0.10]))
        trunc = self.choice(TRUNCS) if trunc is None else trunc
        spec = dict(kind=kind, cost=cost, trunc=trunc, half=half, rseed=int(r.integers(1 << 20)))
        fmt = fill_format(spec, L)
        if v["alive"] and v["fmt"] != "none":
            self.transitions.add((v["fmt"], fmt))
        into = v["alive"]
        self.emit(dict(op="fill", vol=name, into=into, L=L, **spec))
        hist = self.history[name]
        hist.append(kind)
        if hist[-3:] == ["ragged", "uniform", "ragged"]:
            self.ru_r += 1
        v.update(alive=True, kind=kind, fmt=fmt, nan=False, cb=cost_bytes(cost, trunc, kind == "ragged"), spec=dict(kind=kind, cost=cost, half=half, trunc=trunc))
        self.bump(name)

    def upload(self, name):
        m, r = self.model, self.rng
        v = m["vols"][name]
        nan = bool(r.random() < 0.3)
        if v["alive"]:
            self.emit(dict(op="free", vol=name))
            v["alive"] = False
            self.bump(name)
        self.emit(dict(op="upload", vol=name, L=v["L"], seed=int(r.integers(1 << 20)), nan=nan))
        if v["fmt"] != "none":
            self.transitions.add((v["fmt"], "pad" if v["L"] == 151 else "f32"))
        self.history[name].append("uniform")
        v.update(alive=True, kind="uniform", fmt="pad" if v["L"] == 151 else "f32", nan=nan, cb=4, spec=None)
        self.bump(name)

    def weights(self):
        kind = self.choice(["w2", "three", "ones", None], p=[0.4, 0.3, 0.15, 0.15])
        self.emit(dict(op="weights", kind=kind, seed=int(self.rng.integers(1 << 20)), into=self.model["w"] == "w2" and kind == "w2"))
        self.model["w"] = kind

    def agg(self):
        m, r = self.model, self.rng
        prev = m["prev_agg"]
        op = None
        if prev is not None and r.random() < 0.75:
            op = self.mutate(prev)
        if op is None:
            op = self.fresh_agg()
        if op is None:
            return
        if op["w"] is not None:  # (the weight image the context holds NOW)
            op["w"] = m["w"]
        self.emit(op)
        self.sigs.append(planner_sig(op, m))
        m["prev_agg"] = op
        chunked = m["limit"] > 0 and len(op["vols"]) > 1
        piped = m["pipeline"] > 1
        m["last"] = dict(vols=list(op["vols"]), NDIR=op["NDIR"], exact=not (chunked or piped), stale=set(), op=op,
                         nan=any(m["vols"][k]["nan"] for k in op["vols"]))
        if piped or chunked:
            m["maybe"].update(op["vols"])
        else:
            m["maybe"] = set()
        m["pending_lr"] = not (chunked or piped)

    def _group(self, n, like=None):
        m = self.model
        vols = m["vols"]
        alive = self.alive()
        if like is None:
            like = alive[int(self.rng.integers(len(alive)))] if alive else None
        if like is None:
            return None
        same = [k for k in alive if vols[k]["L"] == vols[like]["L"] and vols[k]["kind"] == vols[like]["kind"] and k != like]
        self.rng.shuffle(same)
        return [like] + same[:n - 1]

    def fresh_agg(self):
        r = self.rng
        g = self._group(int(self.choice([1, 1, 2, 2, 3, 5])))
        if g is None:
            return None
        MGM = int(self.choice([1, 2, 3, 3, 4]))
        FH = int(r.random() < 0.5)
        return dict(op="agg", vols=g, FH=FH, MGM=MGM, NDIR=int(self.choice([8, 8, 4, 2, 1])), fix=int(r.random() < 0.7),
                    P1=float(self.choice([2.0, 8.0, 1.5, -0.5], p=[0.32, 0.32, 0.28, 0.08])),  # (a negative P1: the first build, k_pass)
                    P2=float(self.choice([20.0, 32.0, 9.0, 20000.0, math.inf], p=[0.3, 0.3, 0.15, 0.2, 0.05])),
                    refine=self.choice([None, "vfit", "parabola", "cubic", "parabolaOCV"]), wantS=bool(r.random() < 0.3),
                    w=self.model["w"] if r.random() < 0.4 else None, rel=self.choice([None, "0", "1", "2"], p=[0.4, 0.1, 0.3, 0.2]))

    def mutate(self, prev):
        """The previous launch with ONE planner input changed (the same volumes unless the input is their format)."""
        m, r = self.model, self.rng
        vols = m["vols"]
        if not all(vols[k]["alive"] for k in prev["vols"]):
            return None
        op = dict(prev)
        op["vols"] = list(prev["vols"])
        kind = vols[op["vols"][0]]["kind"]
        axis = self.choice([a for a in AXES if a != "slots" or kind == "ragged"])
        if axis == "fh":
            op["FH"] = 1 - prev["FH"]
            if op["MGM"] == 2:
                op["MGM"] = 3
        elif axis == "tsgm34":
            op["MGM"] = 7 - prev["MGM"] if prev["MGM"] in (3, 4) else 3
        elif axis == "fh2":
            op["FH"], op["MGM"] = (1, 2) if not (prev["FH"] and prev["MGM"] == 2) else (1, 3)
        elif axis in ("cb", "slots"):
            # refill the launch's volumes (same kind) with another cost function / other windows, then launch again
            if axis == "cb":
                cost = self.choice(["census1", "ad3", "ncc", "ad", "sd"])
                half = int(r.integers(3, 20))
            else:
                cost = "census1"
                half = int(r.integers(34, 58)) if vols[op["vols"][0]]["fmt"] == "r64" else int(r.integers(3, 20))
            for k in op["vols"]:
                self.fill(k, kind=kind, cost=cost, half=half, trunc=math.inf)
        elif axis == "weights":
            self.weights()
            op["w"] = m["w"] if prev["w"] is None else None
        elif axis == "subv":
            # the same launch on volumes of another label count (64 <-> 128 labels: volumes share a wave or not)
            # (refilled like the launch's first volume where they hold something else)
            spec = vols[op["vols"][0]].get("spec")
            L0 = vols[op["vols"][0]]["L"]
            Ls = sorted({v["L"] for v in vols.values()} - {L0})
            L1 = Ls[int(r.integers(len(Ls)))]
            g = [k for k in vols if vols[k]["L"] == L1][:len(op["vols"])]
            if spec is None or len(g) != len(op["vols"]):
                return None
            for k in g:
                if not vols[k]["alive"] or vols[k].get("spec") != spec:
                    self.fill(k, **spec)
            op["vols"] = g
        elif axis == "passes":
            op["NDIR"] = 4 if prev["NDIR"] == 8 else 8
        elif axis == "wantS":
            op["wantS"] = not prev["wantS"]
        op["axis"] = axis
        return op

    def wta(self):
        m, r = self.model, self.rng
        last = m["last"]
        alive = self.alive()
        if not alive:
            return
        if last and r.random() < 0.6:
            name = self.choice(last["vols"])
        else:
            name = self.choice(alive)
        if not m["vols"][name]["alive"] or m["vols"][name]["nan"]:
            return
        NDIR = last["NDIR"] if last and r.random() < 0.85 else int(self.choice([1, 2, 4, 8]))
        in_last = bool(last and name in last["vols"] and name not in last["stale"] and NDIR == last["NDIR"])
        if in_last and last["exact"]:
            expect = "exact"
        elif in_last or (name in m["maybe"] and last and NDIR == last["NDIR"]):
            expect = "exact_or_refuse"
        else:
            expect = "refuse"
        self.emit(dict(op="wta", vol=name, NDIR=NDIR, refine=self.choice([None, "vfit", "cubic"]), seed=int(r.integers(1 << 20)),
                       expect=expect, agg=last["op"] if last else None))

    def ctxop(self):
        m, r = self.model, self.rng
        k = self.choice(["limit", "trim", "pipeline", "tries", "free", "sync"], p=[0.2, 0.15, 0.25, 0.1, 0.2, 0.1])
        if k == "limit":
            m["limit"] = 0 if m["limit"] else int(self.choice([1, 2]))
            self.emit(dict(op="limit", units=m["limit"]))
        elif k == "trim":  # (releases the Lr volumes: the last aggregation can no longer be searched again)
            self.emit(dict(op="trim"))
            m["last"], m["maybe"], m["pending_lr"] = None, set(), False
        elif k == "pipeline":
            m["pipeline"] = 1 if m["pipeline"] > 1 else int(self.choice([2, 3, 4]))
            self.emit(dict(op="pipeline", depth=m["pipeline"]))
            m["pending_lr"] = False
        elif k == "tries":
            self.emit(dict(op="tries", n=2))
        elif k == "free":
            alive = self.alive()
            if alive:
                name = self.choice(alive)
                self.emit(dict(op="free", vol=name))
                m["vols"][name]["alive"] = False
                self.bump(name)
                self.fill(name)  # (a new handle under the old name: the allocator may hand back the same address)
        else:
            self.emit(dict(op="sync"))
            m["pending_lr"] = False

    # ---- the block ----
    def generate(self):
        m, r = self.model, self.rng
        self.weights()
        for k in m["vols"]:
            self.fill(k)
        # one handle through every format, each fill aggregated (later fills and aggregations come at random)
        tour = [k for k, v in m["vols"].items() if v["L"] != 151][self.seed % 3]
        padded = [k for k, v in m["vols"].items() if v["L"] == 151][:1]
        steps = [(tour, "uniform", "census1", 0), (tour, "uniform", "ad", 0), (tour, "uniform", "ad3", 0), (tour, "uniform", "ncc", 0),
                 (tour, "ragged", "census1", 10), (tour, "ragged", "census1", 45), (tour, "uniform", "census1", 0), (tour, "ragged", "ad", 8)]
        steps += [(k, kind, cost, 0) for k in padded for kind, cost in (("uniform", "census1"), ("uniform", "ncc"), ("uniform", "ad"))]
        for tour, kind, cost, half in steps:
            self.fill(tour, kind=kind, cost=cost, half=half, trunc=math.inf)
            op = self.fresh_agg()
            op["vols"] = [tour]
            self.emit(op)
            self.sigs.append(planner_sig(op, m))
            m["prev_agg"] = op
            m["last"] = dict(vols=[tour], NDIR=op["NDIR"], exact=True, stale=set(), op=op, nan=False)
            m["maybe"] = set()
        for step in range(self.nops):
            x = r.random()
            if m["pending_lr"] and x < 0.2:
                last = m["last"]
                if not last["nan"]:
                    self.emit(dict(op="lr", passes=sorted({0, last["NDIR"] - 1}), agg=last["op"]))
                m["pending_lr"] = False
                continue
            m["pending_lr"] = False
            if x < 0.55:
                self.agg()
            elif x < 0.68:
                alive = self.alive()
                self.fill(self.choice(alive) if alive else "V0")
            elif x < 0.74:
                self.weights()
            elif x < 0.86:
                self.wta()
            else:
                self.ctxop()
        if m["pipeline"] > 1:
            self.emit(dict(op="pipeline", depth=1))
        self.emit(dict(op="sync"))
        return self.ops


def generate(seed, nops=DEFAULT_OPS):
    g = Generator(seed, nops)
    g.generate()
    return g


def collisions(sigs):
    """Adjacent aggregations of one shape and batch size that differ in exactly one planner input: {axis: count}."""
    out = {a: 0 for a in AXES}
    for a, b in zip(sigs, sigs[1:]):
        if a["shape"] != b["shape"] or a["nb"] != b["nb"]:
            continue
        diff = [k for k in AXES if a[k] != b[k]]
        if "fh2" in diff and set(diff) <= {"fh", "tsgm34", "fh2"}:  # (FH with TSGM 2 is one input, though it moves FH or TSGM with it)
            diff = ["fh2"]
        if len(diff) == 1:
            out[diff[0]] += 1
    return out


def check_legal(ops):
    """Raises AssertionError if an operation touches a freed handle or makes a call the ABI leaves undefined."""
    alive, w = set(), None
    last_agg, since_agg = None, 99
    for i, op in enumerate(ops):
        k = op["op"]
        since_agg += 1
        if k in ("fill", "upload"):
            assert op.get("into", False) == (op["vol"] in alive) or k == "upload", (i, op)
            if k == "upload":
                assert op["vol"] not in alive, (i, "upload over a live handle leaks it", op)
            alive.add(op["vol"])
            if k == "fill":
                assert op["cost"] in COSTS and op["kind"] in ("uniform", "ragged"), (i, op)
        elif k == "free":
            assert op["vol"] in alive, (i, "double free", op)
            alive.discard(op["vol"])
        elif k == "agg":
            assert all(v in alive for v in op["vols"]), (i, "freed handle in a batch", op)
            assert len(set(op["vols"])) == len(op["vols"]) and 1 <= len(op["vols"]) <= 16, (i, op)
            assert op["w"] is None or w is not None, (i, "weights that do not exist", op)
            last_agg, since_agg = op, 0
        elif k == "weights":
            w = op["kind"]
        elif k == "wta":
            assert op["vol"] in alive, (i, "windowed search on a freed handle", op)
        elif k == "lr":
            # mgm_debug_download_lr only straight after an aggregation (the refusal after a refill is its own test)
            assert since_agg == 1 and last_agg is not None and op["agg"] is last_agg, (i, op)
        elif k == "limit":
            assert op["units"] in (0, 1, 2), (i, op)
        elif k == "pipeline":
            assert 1 <= op["depth"] <= 4, (i, op)
        elif k == "tries":
            assert op["n"] == 2
        else:
            assert k in ("trim", "sync"), (i, op)
    return True


def summary(gens):
    """Coverage of a set of generated blocks: collisions per axis, formats refilled from / into, ragged -> uniform -> ragged."""
    col = {a: 0 for a in AXES}
    trans, rur, nagg = set(), 0, 0
    for g in gens:
        for a, n in collisions(g.sigs).items():
            col[a] += n
        trans |= g.transitions
        rur += g.ru_r
        nagg += len(g.sigs)
    return dict(collisions=col, total=sum(col.values()), from_fmt={f for f, _ in trans}, to_fmt={t for _, t in trans}, ru_r=rur, aggs=nagg)


def fmt_op(op):
    """One line a reader can replay by hand."""
    d = {k: v for k, v in op.items() if k not in ("agg",)}
    return " ".join("%s=%s" % (k, v) for k, v in d.items())
