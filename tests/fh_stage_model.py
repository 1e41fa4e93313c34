"""The one numpy restatement of the truncated-linear (FH) min-convolution as the pass kernels run it (fh_scan, fh_careful,
fh_repair, fh_minconv in mgm_amd/csrc/mgm_pass_common.h), next to the reference's sequential recurrences
(minConvTruncatedLinear, mgm_core.cc:152-163), and the generators of the cost volumes the FH tests feed it.

Layout of the model: a wave of 64 lanes, lane l holding LPL consecutive label slots; GROUPS label ranges per wave, lane groups
of GL = 64/GROUPS lanes that scan independently but VOTE together (the sweep loop's ballot and the `boosted` state are the
wave's), so with GROUPS > 1 consecutive slabs of the input share a wave and a stage.  Slots >= L are padding: +INF on entry,
reset to +INF between the forward and the backward scan.  Every operation is one float32 (or, in the repair, float64)
operation of the device code, in its order; numpy rounds each one to nearest even as the device does.

Stages (what `stages` returns per slab and direction): 0 the log-step guess is accepted by the first sweep, 1 fh_careful's
guess by the second, 2 fh_repair's by the third, 3 plain sweeps settle it, one more lane per sweep."""
import numpy as np

f32 = np.float32
f64 = np.float64
INF = f32(np.inf)
CAP = 70  # fh_scan's loop bound
LPLS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32)
LANE = np.arange(64)
LI, ROW = LANE & 15, LANE >> 4


# ---- the reference -----------------------------------------------------------------------------------------------------------
def seq_scan(M, P1, fwd):
    """One sequential recurrence over the last axis: fwd M[o] = min(M[o-1] + P1, M[o]) for rising o, else the mirror image."""
    F = np.array(M, f32, copy=True)
    P1 = f32(P1)
    n = F.shape[-1]
    for o in (range(1, n) if fwd else range(n - 2, -1, -1)):
        F[..., o] = np.minimum(F[..., o], F[..., o - 1 if fwd else o + 1] + P1)
    return F


def minconv(slabs, P1, P2, m):
    """minConvTruncatedLinear of every slab [..., L] from the two sequential recurrences only; m: the slabs' minima [...]."""
    M = seq_scan(seq_scan(slabs, P1, True), P1, False)
    if f32(P2) < INF:
        M = np.minimum(M, (np.asarray(m, f32) + f32(P2))[..., None])
    return M


# ---- lane moves of a wave: [N, 64] -> [N, 64], NaN where a lane has no source lane ---------------------------------------------
def _row_shift(x, k, fwd):  # DPP row_shr:k (fwd) / row_shl:k inside rows of 16 lanes
    r = x.reshape(-1, 4, 16)
    out = np.full_like(r, np.nan)
    if fwd:
        out[:, :, k:] = r[:, :, :-k]
    else:
        out[:, :, :-k] = r[:, :, k:]
    return out.reshape(-1, 64)


def _wave_shift(x, fwd, fill):  # wave_shr:1 (fwd: lane l reads lane l-1) / wave_shl:1
    out = np.full_like(x, fill)
    if fwd:
        out[:, 1:] = x[:, :-1]
    else:
        out[:, :-1] = x[:, 1:]
    return out


def _min_shift(c, t, k, fwd):  # MGM_DPP_MIN: c = min(c, t[source lane]); lanes without a source keep c
    s = _row_shift(t, k, fwd)
    return np.where(np.isnan(s), c, np.minimum(c, s))


def _prev_row_lane15(x):  # row_bcast:15 -- rows 1..3 read lane 15 of the row before; row 0 reads 0 (its addend is +INF)
    return np.where(ROW >= 1, x[:, np.maximum(ROW * 16 - 1, 0)], x.dtype.type(0))


def _edge(fwd, G):  # the first lane of a label range in scan order: no carry enters it
    GL = 64 // G
    return (LANE % GL == 0) if fwd else (LANE % GL == GL - 1)


def _where(cond, x):  # per-lane constant: x where cond, +INF elsewhere
    return np.where(cond, x, np.inf).astype(np.asarray(x).dtype)


# ---- the stages, each on carry-outs a [N, 64] of lanes that ignore their carry-in ------------------------------------------------
def origin(X, P1, fwd):
    """fh_scan's `origin`: X [N, 64, LPL] -> the carry-out of every lane ignoring its carry-in."""
    P1 = f32(P1)
    order = range(X.shape[2]) if fwd else range(X.shape[2] - 1, -1, -1)
    a = None
    for q in order:
        a = X[:, :, q].copy() if a is None else np.minimum(X[:, :, q], a + P1)
    return a


def guess(a, P1, LPL, fwd, G=1):
    """The log-step guess of fh_scan (and of fh_scan_multi, which is the G = 4 form)."""
    R = f32(LPL) * f32(P1)
    c = a.copy()
    for k in (1, 2, 4, 8):
        c = _min_shift(c, c + f32(k) * R, k, fwd)
    if fwd:
        if G <= 2:
            offA = _where((ROW >= 1) if G == 1 else (ROW & 1) == 1, (LI + 1).astype(f32) * R)
            c = np.minimum(c, _prev_row_lane15(c) + offA)
        if G == 1:
            offB = _where(ROW >= 2, (LI + 1 + np.where(ROW == 3, 16, 0)).astype(f32) * R)
            c = np.minimum(c, c[:, [31]] + offB)
    elif G == 1:
        offA0 = _where(ROW == 0, (16 - LI).astype(f32) * R)
        offA2 = _where(ROW == 2, (16 - LI).astype(f32) * R)
        offB = _where(ROW <= 1, (32 - LANE).astype(f32) * R)
        c = np.minimum(np.minimum(c, c[:, [16]] + offA0), c[:, [48]] + offA2)
        c = np.minimum(c, c[:, [32]] + offB)
    elif G == 2:
        tp = np.where(ROW == 0, c[:, [16]], c[:, [48]])
        c = np.minimum(c, tp + _where((ROW & 1) == 0, (16 - LI).astype(f32) * R))
    return c


def careful(a, P1, LPL, fwd, G=1):
    """fh_careful: carries advanced by a whole lane in unit steps, hops cut into pieces of at most 4R, 12R, 16R."""
    P1 = f32(P1)
    R = f32(LPL) * P1
    R4, R12 = f32(4) * R, f32(12) * R
    b = a.copy()
    for _ in range(LPL):
        b = b + P1
    s = _where(~_edge(fwd, G), _wave_shift(b, fwd, INF))
    s = _min_shift(s, s + R, 1, fwd)
    s = _min_shift(s, s + f32(2) * R, 2, fwd)
    s = _min_shift(s, s + R4, 4, fwd)
    s = _min_shift(s, (s + R4) + R4, 8, fwd)
    if fwd:
        if G <= 2:
            off = (LI + 1).astype(f32) * R
            p1 = np.minimum(off, R4)
            p2 = off - p1
            on = (ROW >= 1) if G == 1 else (ROW & 1) == 1
            t = _prev_row_lane15(s) + _where(on, p1)
            t = t + np.where(on, p2, f32(0))
            s = np.minimum(s, t)
        if G == 1:
            off = (LI + 1 + np.where(ROW == 3, 16, 0)).astype(f32) * R
            p1 = np.minimum(off, R4)
            p2 = np.minimum(off - p1, R12)
            p3 = (off - p1) - p2
            on = ROW >= 2
            t = s[:, [31]] + _where(on, p1)
            t = (t + np.where(on, p2, f32(0))) + np.where(on, p3, f32(0))
            s = np.minimum(s, t)
    else:
        add16 = lambda x: (x + R4) + R12
        off = (16 - LI).astype(f32) * R
        p1 = np.minimum(off, R4)
        p2 = off - p1
        if G == 1:
            t3 = s[:, [48]]
            t2 = np.minimum(s[:, [32]], add16(t3))
            t1 = np.minimum(s[:, [16]], add16(t2))
            tp = np.where(ROW == 0, t1, np.where(ROW == 1, t2, t3))
            s = np.minimum(s, np.where(ROW <= 2, (tp + p1) + p2, INF))
        elif G == 2:
            tp = np.where(ROW == 0, s[:, [16]], s[:, [48]])
            s = np.minimum(s, np.where((ROW & 1) == 1, INF, (tp + p1) + p2))
    return np.minimum(a, s)


def repair(a, P1, LPL, fwd, G=1):
    """fh_repair: the min-plus scan of the exact sums in f64, then successive rounding to every binade's float32 grid."""
    P1 = f32(P1)
    P1d, Rd = f64(P1), f64(LPL) * f64(P1)
    dmin = lambda x, y: np.where(y < x, y, x)
    b = (a + P1).astype(f64)
    s = np.where(_edge(fwd, G), np.inf, _wave_shift(b, fwd, np.inf) + Rd)

    def moved(x, k):
        m = _row_shift(x, k, fwd)
        return np.where(np.isnan(m), np.inf, m)
    for k in (1, 2, 4, 8):
        s = dmin(s, moved(s, k) + f64(k) * Rd)
    if fwd:
        if G <= 2:  # row_mask 0xa: rows 1 and 3 only
            s = dmin(s, np.where((ROW & 1) == 1, _prev_row_lane15(s), np.inf) + (LI + 1).astype(f64) * Rd)
        if G == 1:
            s = dmin(s, np.where(ROW >= 2, s[:, [31]], np.inf) + (LI + 1 + np.where(ROW == 3, 16, 0)).astype(f64) * Rd)
    elif G == 1:
        t3 = s[:, [48]]
        t2 = dmin(s[:, [32]], t3 + 16.0 * Rd)
        t1 = dmin(s[:, [16]], t2 + 16.0 * Rd)
        tp = np.where(ROW == 0, t1, np.where(ROW == 1, t2, t3))
        s = dmin(s, np.where(ROW <= 2, tp + (16 - LI).astype(f64) * Rd, np.inf))
    elif G == 2:
        tp = np.where(ROW == 0, s[:, [16]], s[:, [48]])
        s = dmin(s, np.where((ROW & 1) == 1, np.inf, tp + (16 - LI).astype(f64) * Rd))
    s = s - P1d
    if P1 > 0:
        # (the device leaves the loop when no lane of the wave lands in [B, 2B); B only grows, so going on changes nothing)
        B = f64(np.array((np.array(P1, f32).view(np.uint32) & np.uint32(0x7f800000)) + np.uint32(0x00800000), np.uint32).view(f32))
        for _ in range(64):
            reach = (s < np.inf) & (s >= B)
            if not reach.any():
                break
            magic = B * 805306368.0
            s = np.where(reach, (s + magic) - magic, s)
            B = B + B
    return np.minimum(a, s.astype(f32))


def sweep(Xt, c, P1, fwd, G=1):
    """One sweep of fh_scan's loop: the exact in-lane recurrence given the neighbour lane's carry.  Xt [LPL, N, 64] (slot-major,
    so that every step reads contiguous memory) -> (f [LPL, N, 64], carries [N, 64])."""
    P1 = f32(P1)
    prev = _wave_shift(c, fwd, f32(0)) + _where(~_edge(fwd, G), np.full(64, P1, f32))  # carry + P1; +INF into a range's first lane
    f = np.empty_like(Xt)
    order = list(range(Xt.shape[0])) if fwd else list(range(Xt.shape[0] - 1, -1, -1))
    for q in order:
        np.minimum(Xt[q], prev if q == order[0] else prev + P1, out=f[q])
        prev = f[q]
    return f, prev


def scan(X, P1, LPL, fwd, G=1, cap=CAP):
    """fh_scan on waves X [N, 64, LPL] -> (result, stage [N], loop iterations [N], the accepted stage's carries [N, 64])."""
    N = X.shape[0]
    a = origin(X, P1, fwd)
    c = guess(a, P1, LPL, fwd, G)
    out, stage, its, acc = np.empty_like(X), np.full(N, 3), np.zeros(N, int), np.full((N, 64), np.nan, f32)
    live = np.arange(N)
    Xt = np.ascontiguousarray(X.transpose(2, 0, 1))
    with np.errstate(invalid="ignore"):
        for it in range(cap):
            f, c2 = sweep(Xt, c, P1, fwd, G)
            ok = (c2 == c).all(1)
            its[live] = it + 1
            done = live[ok] if it < cap - 1 else live  # (a slab still rejected at the bound keeps the last sweep's values, as the device would)
            out[done] = f[:, ok if it < cap - 1 else slice(None)].transpose(1, 2, 0)
            stage[live[ok]] = min(it, 3)
            acc[live[ok]] = c[ok]
            if ok.any():
                live, c, Xt = live[~ok], c2[~ok], np.ascontiguousarray(Xt[:, ~ok])
            else:
                c = c2
            if live.size == 0:
                break
            if it == 0:
                c = careful(a[live], P1, LPL, fwd, G)
            elif it == 1:
                c = repair(a[live], P1, LPL, fwd, G)
    return out, stage, its, acc


def waves(slabs, LPL, G, L):
    """slabs [N, L] -> waves [ceil(N/G), 64, LPL]: G consecutive slabs per wave (the last wave repeats the last slab), padded +INF."""
    slabs = np.asarray(slabs, f32)
    N = slabs.shape[0]
    GL = 64 // G
    assert slabs.shape[1] == L and L <= GL * LPL, (slabs.shape, L, GL, LPL)
    idx = np.minimum(np.arange(-(-N // G) * G), N - 1)
    W = np.full((idx.size, GL * LPL), INF, f32)
    W[:, :L] = slabs[idx]
    return W.reshape(-1, 64, LPL)


def stages(slabs, P1, LPL, G, L, cap=CAP, want_carries=False):
    """fh_minconv's two scans on slabs [N, L]: per slab, stage [N, 2] and loop iterations [N, 2] (column 0 forward, 1 backward).
    With want_carries also, per direction, (accepted carries, sequential carries) of the slabs' waves."""
    X = waves(slabs, LPL, G, L)
    N, GL = np.asarray(slabs).shape[0], 64 // G
    pad = (np.arange(GL * LPL) >= L).reshape(GL, LPL)
    pad = np.tile(pad, (G, 1))
    st, its, car = [], [], []
    for fwd in (True, False):
        F, s, n, acc = scan(X, P1, LPL, fwd, G, cap)
        if want_carries:
            seq = seq_scan(X.reshape(-1, G, GL * LPL), P1, fwd).reshape(-1, 64, LPL)[:, :, LPL - 1 if fwd else 0]
            car.append((acc, seq, s))
        st.append(np.repeat(s, G)[:N])
        its.append(np.repeat(n, G)[:N])
        X = np.where(pad, INF, F)
    res = (np.stack(st, 1), np.stack(its, 1))
    return res + (car,) if want_carries else res


def device_minconv(slabs, P1, P2, m, LPL, G, L):
    """The model's own fh_minconv result (what the kernel computes when the loop bound holds): [N, L]."""
    X = waves(slabs, LPL, G, L)
    GL = 64 // G
    pad = np.tile((np.arange(GL * LPL) >= L).reshape(GL, LPL), (G, 1))
    F = scan(X, P1, LPL, True, G)[0]
    B = scan(np.where(pad, INF, F), P1, LPL, False, G)[0]
    M = B.reshape(-1, GL * LPL)[:np.asarray(slabs).shape[0], :L]
    return np.minimum(M, (np.asarray(m, f32) + f32(P2))[:, None]) if f32(P2) < INF else M


# ---- the slabs a run convolves -----------------------------------------------------------------------------------------------
# mgm_core.cc:481-484 (pass table) as the oracle restates it: neighbour offsets of every pass, and the weight plane of
# neighbour k in pass p
PASS_NEIGHBOURS = [
    [(-1, 0), (0, -1), (-1, -1), (1, -1)], [(1, 0), (0, 1), (1, 1), (-1, 1)],
    [(0, 1), (-1, 0), (-1, 1), (-1, -1)], [(0, -1), (1, 0), (1, -1), (1, 1)],
    [(-1, -1), (1, -1), (0, -1), (1, 0)], [(1, -1), (1, 1), (1, 0), (0, 1)],
    [(1, 1), (-1, 1), (0, 1), (-1, 0)], [(-1, 1), (-1, -1), (-1, 0), (0, -1)]]
P2C = [[0, 1, 2, 3, 4, 5, 6, 7], [3, 2, 0, 1, 5, 6, 7, 4], [4, 6, 7, 5, 3, 1, 2, 0], [5, 7, 4, 6, 1, 2, 0, 3]]


def neighbour_terms(lr_dump, MGM, w8=None):
    """Every min-convolution of a uniform-range run, from its dumped Lr [NDIR, ny, nx, L]: a list over (pass, k < MGM) of
    (pass, k, ys, xs, slabs [n, L], P1 factor [n]) -- the neighbour-k slabs of every updated pixel (ys, xs) of the pass and the
    receiving pixel's weight (1 without weights)."""
    NDIR, ny, nx, L = lr_dump.shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    out = []
    for p in range(NDIR):
        inside = np.ones((ny, nx), bool)  # updated iff all FOUR neighbours of the pass are inside, whatever MGM is (mgm_core.cc:538-541)
        for dx, dy in PASS_NEIGHBOURS[p]:
            inside &= (xx + dx >= 0) & (xx + dx < nx) & (yy + dy >= 0) & (yy + dy < ny)
        ys, xs = yy[inside], xx[inside]
        for k in range(MGM):
            dx, dy = PASS_NEIGHBOURS[p][k]
            D = w8[P2C[k][p], ys, xs].astype(f32) if w8 is not None else np.ones(ys.size, f32)
            out.append((p, k, ys, xs, lr_dump[p, ys + dy, xs + dx], D))
    return out


def slabs_of_run(lr_dump, P1, MGM, w8=None):
    """The min-convolution inputs of a whole run grouped by the penalty they meet: {float32(P1 * w): slabs [n, L]} (the Lr
    slabs of every pixel that has a successor, once per distinct consumer penalty)."""
    groups = {}
    for p, k, ys, xs, S, D in neighbour_terms(lr_dump, MGM, w8):
        pen = f32(P1) * D
        for v in np.unique(pen):
            groups.setdefault(float(v), []).append(S[pen == v])
    return {v: np.unique(np.concatenate(s), axis=0) for v, s in groups.items()}


def lr_from_neighbours(C, lr_dump, P1, P2, MGM, w8=None, conv=minconv):
    """The Lr of every pass recomputed from the DUMPED neighbours with `conv` and the reference's update
    (update_cost2_trunclinear for MGM 2 without weights, update_costW_trunclinear otherwise; mgm_core.cc:197-281)."""
    NDIR, ny, nx, L = lr_dump.shape
    out = np.stack([np.array(C, f32)] * NDIR)  # frame pixels keep Lr = C
    terms = neighbour_terms(lr_dump, MGM, w8)
    weighted = w8 is not None and bool((w8 != 1).any())
    for p in range(NDIR):
        mine = [t for t in terms if t[0] == p]
        ys, xs = mine[0][2], mine[0][3]
        Ms, ms = [], []
        for _, k, _, _, S, D in mine:
            m = S.min(1)
            Dk = D if weighted else np.ones_like(D)
            M = np.empty_like(S)
            for v in np.unique(Dk):  # one call per distinct penalty
                sel = Dk == v
                M[sel] = conv(S[sel], f32(P1) * v, f32(P2) * v, m[sel])
            Ms.append(M)
            ms.append(m[:, None])
        with np.errstate(invalid="ignore"):
            if MGM == 2 and not weighted:
                e = (Ms[0] - ms[0] + Ms[1] - ms[1]) / f32(2)
            else:
                e = Ms[0] - ms[0]
                for k in range(1, MGM):
                    e = e + (Ms[k] - ms[k])
                e = e / f32(MGM)
            out[p, ys, xs] = np.asarray(C, f32)[ys, xs] + e
    return out


# ---- generators: cost volumes [ny][nx][L]; every pixel has a finite cost; integers where the class is integer ---------------------
def _sparse(rng, ny, nx, L, kmin, kmax, draw, fill):
    C = np.full((ny, nx, L), fill, f32)
    for y in range(ny):
        for x in range(nx):
            k = int(rng.integers(kmin, kmax + 1))
            C[y, x, rng.choice(L, size=min(k, L), replace=False)] = draw(min(k, L))
    return C


def gen_infgap(seed, ny, nx, L):  # all +INF except 1-4 values in [0, 10)
    rng = np.random.default_rng(seed)
    return _sparse(rng, ny, nx, L, 1, 4, lambda k: rng.uniform(0, 10, k).astype(f32), INF)


def gen_frac(seed, ny, nx, L):  # uniform in [0, 1e6) with 1-3 values in [0, 1)
    rng = np.random.default_rng(seed)
    C = rng.uniform(0, 1e6, (ny, nx, L)).astype(f32)
    S = _sparse(rng, ny, nx, L, 1, 3, lambda k: rng.uniform(0, 1, k).astype(f32), f32(-1))
    return np.where(S >= 0, S, C)


def gen_spike(seed, ny, nx, L):  # integers in [1000, 60000) with 1-3 values in {0, 1, 2}: a two-byte compact copy applies
    rng = np.random.default_rng(seed)
    C = rng.integers(1000, 60000, (ny, nx, L)).astype(f32)
    S = _sparse(rng, ny, nx, L, 1, 3, lambda k: rng.integers(0, 3, k).astype(f32), f32(-1))
    return np.where(S >= 0, S, C)


def gen_end0(seed, ny, nx, L):  # 1e7 everywhere except label 0 (a small integer per pixel)
    rng = np.random.default_rng(seed)
    C = np.full((ny, nx, L), 1e7, f32)
    C[:, :, 0] = rng.integers(0, 3, (ny, nx))
    return C


def gen_big(seed, ny, nx, L):  # all +INF but 1-2 integers in [2^20, 2^24)
    rng = np.random.default_rng(seed)
    return _sparse(rng, ny, nx, L, 1, 2, lambda k: rng.integers(1 << 20, 1 << 24, k).astype(f32), INF)


def gen_byte(seed, ny, nx, L):  # `spike` scaled into one byte: integers in [100, 250) with 1-3 values in {0, 1, 2}
    rng = np.random.default_rng(seed)
    C = rng.integers(100, 250, (ny, nx, L)).astype(f32)
    S = _sparse(rng, ny, nx, L, 1, 3, lambda k: rng.integers(0, 3, k).astype(f32), f32(-1))
    return np.where(S >= 0, S, C)


def gen_lanecol(seed, ny, nx, L):
    """Aimed at fh_repair: every pixel's two near-zero costs, v * 10^u with v in [0, 1) and u in [-3, 1), sit on the SAME
    two labels -- the last slot of lane 20 and the first slot of lane 40 of the label layout a full L takes (64 lanes of LPL slots).
    The neighbours' minima then sit on the pixel's own finite labels, so Lr stays far below the penalty there, and a chain that
    starts from a lane's raw carry-out (forward: its last slot, backward: its first) is what fh_careful misses and fh_repair
    gets: on single-value slabs only those two slot positions ever end in stage 2."""
    rng = np.random.default_rng(seed)
    lpl = lpl_of(L)
    lanes = -(-L // lpl)  # (lanes that hold labels: 5/16 and 5/8 of the way, lanes 20 and 40 of 64)
    labs = (lanes * 5 // 16 * lpl + lpl - 1, lanes * 5 // 8 * lpl)
    # every other label: 8 per label of distance to the nearer of the two, + 4 -- above any ramp of a penalty <= 8, so the ramps
    # still win everywhere, and of the ramps' own size, so that Lr = C + e keeps what a wrong carry does to e (behind +INF
    # costs it would vanish: the first version of this class did not notice a repair that was skipped)
    o = np.arange(L)
    far = (8 * np.minimum(abs(o - labs[0]), abs(o - labs[1])) + 4).astype(f32)
    C = np.broadcast_to(far, (ny, nx, L)).copy()
    for lab in labs:
        C[:, :, lab] = rng.uniform(0, 1, (ny, nx)) * 10.0 ** rng.uniform(-3, 1, (ny, nx))
    return C


def gen_flat(seed, ny, nx, L):  # one integer in [0, 25) on every label of a pixel: no ramp ever wins, every guess holds
    rng = np.random.default_rng(seed)
    return np.repeat(rng.integers(0, 25, (ny, nx, 1)).astype(f32), L, axis=2)


def gen_bytecol(seed, ny, nx, L):  # (L = 128 or 64: 32 or 16 lanes of 4 labels)
    rng = np.random.default_rng(seed)
    lanes = L // 4
    labs = (3, L - 4)  # the last slot of the first lane, the first slot of the last: the longest hops either way
    o = np.arange(L)
    far = np.minimum(8 * np.minimum(abs(o - labs[0]), abs(o - labs[1])) + 4, 250).astype(f32)
    C = np.broadcast_to(far, (ny, nx, L)).copy()
    for lab in labs:
        C[:, :, lab] = rng.integers(0, 3, (ny, nx))
    return C


GENERATORS = dict(bytecol=gen_bytecol, flat=gen_flat, infgap=gen_infgap, frac=gen_frac, spike=gen_spike, end0=gen_end0, big=gen_big, byte=gen_byte,
                  lanecol=gen_lanecol)
PENALTIES = (2.0, 7.0, 0.1, float(f32(1.0) / f32(3.0)), 2.5, 1000.0)


def volume(cls, seed, ny, nx, L):
    C = GENERATORS[cls](seed, ny, nx, L)
    assert np.isfinite(C).any(2).all() and not np.isnan(C).any() and (C >= 0).all() and not np.signbit(C).any()
    return C


def row_volume(cls, seed, ny, nx, L, row):
    """`cls` on ONE image row, tame integers 0..24 (the suite's usual costs) elsewhere: one line of a band straggles."""
    rng = np.random.default_rng(seed + 1000)
    C = rng.integers(0, 25, (ny, nx, L)).astype(f32)
    C[row] = volume(cls, seed, 1, nx, L)[0]
    return C


def ad_pair(seed, ny, nx, bright=250.0, zeros=3):
    """The image-pair form (k_pass_rel builds its own costs): u constant 0, v `bright` with `zeros` pixels per row at 0..2 --
    the `ad` cost |u(x) - v(x + d)| of a pixel is `bright` on every label but the few that meet a near-zero pixel: the
    one-byte `spike` class over each pixel's range."""
    rng = np.random.default_rng(seed)
    u = np.zeros((1, ny, nx), f32)
    v = np.full((1, ny, nx), bright, f32)
    for y in range(ny):
        xs = rng.choice(nx, size=zeros, replace=False)
        v[0, y, xs] = rng.integers(0, 3, zeros)
    return u, v


# ---- the device cases (tests/test_gpu_fh_stages.py) and the floors their inputs meet (tests/test_fh_stages.py) ------------------
# What a case is named for -> the (class, P1) that reaches it on the Lr of a run (the counts: DESIGN.md section 4).  `s1`: the
# guess is rejected and fh_careful accepted; `s2`: fh_repair accepted; `s3`: plain sweeps; `sweeps`: plain sweeps over
# (nearly) the whole label range.
STAGE_INPUT = dict(s1=("frac", 2.0), s2=("lanecol", 7.0), s3=("infgap", 0.1), sweeps=("big", 2.5))
STAGE_OF = dict(s1=1, s2=2, s3=3, sweeps=3)
WEIGHTS3, WEIGHTS2 = (1.0, 0.3, 2.5), (1.0, 0.3)


# P2 = 20000 * P1 (the suite's usual ratio) unless a case names another: the cap m + P2 then never cuts a ramp, however long.  (With
# P2 = 40 * P1 a ramp ends after 40 labels -- three lanes at 12 labels per lane -- and hides what a late lane's carry did wrong:
# a loop bound of 8 for 70 went unnoticed from 512 labels on.)
def case(name, family, lpl, groups, stage, L, nx=24, ny=16, P2f=20000.0, NDIR=8, MGM=3, weights=None, cls=None, P1=None, nb=1,
         classes=None, row=None, env=None, fresh=False, flags=(), flat_rows=False):
    c, p = STAGE_INPUT[stage]
    if stage == "s2" and lpl % 3 == 0:
        p = 5.0  # (with P1 = 7 no slab of `lanecol` ends in stage 2 at 3, 6, 12 or 24 labels per lane; with 5 they do)
    return dict(name=name, family=family, lpl=lpl, groups=groups, stage=stage, L=L, nx=nx, ny=ny, cls=cls or c,
                P1=float(P1 if P1 is not None else p), P2f=P2f, NDIR=NDIR, MGM=MGM, weights=weights, nb=nb, classes=classes,
                row=row, env=env, fresh=fresh, flags=flags, flat_rows=flat_rows)


def lpl_of(L):
    return min(l for l in LPLS if 64 * l >= L)


def _dense_cases():
    out = []
    for L in (64, 128, 192, 256, 384, 512, 768, 1024, 100, 151, 600):  # LPL 1..16; 100, 151, 600: padding slots to reset
        for st in ("s1", "s2", "s3", "sweeps"):
            out.append(case("p2_l%d_%s" % (L, st), "k_pass2", lpl_of(L), 1, st, L))
    for MGM in (1, 2, 4):  # (2: update_cost2_trunclinear, the build without tags)
        for st in STAGE_INPUT:
            out.append(case("p2_t%d_l256_%s" % (MGM, st), "k_pass2", 4, 1, st, 256, MGM=MGM))
    for st in STAGE_INPUT:
        out.append(case("p2_ndir3_l128_%s" % st, "k_pass2", 2, 1, st, 128, NDIR=3))
        out.append(case("p2_p2inf_l192_%s" % st, "k_pass2", 3, 1, st, 192, P2f=np.inf))
    # one-byte compact costs: integers and an integer penalty are exact, only the thirds of e / 3 in Lr make a guess fail -- 96 x 32
    out.append(case("p2_byte_l256_s1", "k_pass2", 4, 1, "s1", 256, cls="byte", P1=7.0, nx=96, ny=32))
    for L in (64, 128, 192, 256, 384, 512, 768, 1024, 100, 151, 600):  # ... at every label count: the builds with deep rings
        out.append(case("p2_byte_l%d_sweeps" % L, "k_pass2", lpl_of(L), 1, "sweeps", L, cls="byte", P1=0.1, flags=((4, "1"), (6, "true")), flat_rows=True))
    for L in (64, 256):  # ... and from 32 work items on the per-XCD queues and the one-band build (flags: template arguments 7, 8)
        out.append(case("p2_byte_l%d_queues_sweeps" % L, "k_pass2", lpl_of(L), 1, "sweeps", L, cls="byte", P1=0.1, nx=96, ny=32,
                        flags=((4, "1"), (6, "true"), (7, "true"), (8, "true")), flat_rows=True))
    out.append(case("p2_twobyte_l256_sweeps", "k_pass2", 4, 1, "sweeps", 256, cls="spike", P1=0.1, flat_rows=True, flags=((4, "2"),)))  # two-byte compact costs
    # volumes sharing a wave (one-byte compact costs only): every slot the same class, and stalled groups beside hot ones -- under
    # a penalty that is not dyadic every integer slab with a ramp in it stalls, a `flat` one (one cost on all labels) never does
    out.append(case("p2_four_of_l128_sweeps", "k_pass2", 4, 2, "sweeps", 128, nb=4, cls="byte", P1=0.1))
    out.append(case("p2_four_of_l128_mixed", "k_pass2", 4, 2, "sweeps", 128, nb=4, cls="byte", P1=0.1,
                    classes=("byte", "flat", "flat", "byte")))
    out.append(case("p2_eight_of_l64_sweeps", "k_pass2", 4, 4, "sweeps", 64, nb=8, cls="byte", P1=0.1))
    # ... and the two cheap stages there: one-byte costs reach them only through the thirds of e / 3 in Lr (`bytecol`: `lanecol` in
    # integers, the near-zero costs 0..2 on the last slot of the first lane and the first slot of the last lane OF THE VOLUME'S LANE
    # GROUP: the longest hops either way; with the two labels mid-range neither direction of four per wave reached stage 2)
    out.append(case("p2_four_of_l128_s1", "k_pass2", 4, 2, "s1", 128, nb=4, cls="bytecol", P1=7.0, nx=48, ny=32))
    out.append(case("p2_eight_of_l64_s1", "k_pass2", 4, 4, "s1", 64, nb=8, cls="bytecol", P1=7.0, nx=48, ny=32))
    out.append(case("p2_four_of_l128_s2", "k_pass2", 4, 2, "s2", 128, nb=4, cls="bytecol", P1=7.0, nx=48, ny=32))
    out.append(case("p2_eight_of_l64_s2", "k_pass2", 4, 4, "s2", 64, nb=8, cls="bytecol", P1=7.0, nx=48, ny=32))
    # weighted: the consumer's penalty P1 * w; with a dyadic P1 on integers only the weighted penalty leaves the premise
    for st in STAGE_INPUT:
        out.append(case("p2_weights3_l128_%s" % st, "k_pass2", 2, 1, st, 128, weights=WEIGHTS3))
        out.append(case("p2_weights2_l128_%s" % st, "k_pass2", 2, 1, st, 128, weights=WEIGHTS2))
    # W2 (the producer publishes both transforms, mgm_pass2.hip:874-875) wants one-byte costs, <= 256 labels and the queues
    out.append(case("p2_w2_l128_dyadic", "k_pass2", 2, 1, "s3", 128, weights=WEIGHTS2, cls="byte", P1=2.0, nx=96, ny=48, flags=((9, "true"),)))
    out.append(case("p2_w2_l256_sweeps", "k_pass2", 4, 1, "sweeps", 256, weights=WEIGHTS2, cls="byte", P1=0.1, nx=96, ny=48, flags=((9, "true"),)))
    out.append(case("p2_weights3_dyadic_l128", "k_pass2", 2, 1, "s3", 128, weights=WEIGHTS3, cls="byte", P1=2.0))
    out.append(case("p2_weights2_dyadic_l128", "k_pass2", 2, 1, "s3", 128, weights=WEIGHTS2, cls="byte", P1=2.0))
    # the first build: above 1024 labels, weighted FH above 512, and by switch in a child process
    for L in (1100, 1536, 2048):
        for st in STAGE_INPUT:  # (13 x 11 has too few slabs for the stage-1 floor: 48 x 16 there; `flat` rows give `s3` its stage-0 slabs)
            out.append(case("p1_l%d_%s" % (L, st), "k_pass", lpl_of(L), 1, st, L, nx=48 if st == "s1" else 13, ny=16 if st == "s1" else 11,
                            fresh=True, flat_rows=st == "s3"))
    for st in STAGE_INPUT:
        out.append(case("p1_weights3_l600_%s" % st, "k_pass", 12, 1, st, 600, nx=13, ny=11, weights=WEIGHTS3, fresh=True))
        out.append(case("p1_switch_l256_%s" % st, "k_pass", 4, 1, st, 256, env={"MGM_HIP_PASS_BUILD": "1"}))
    # several bands per pass, the stragglers on ONE image row
    for L in (256, 64):
        out.append(case("p2_bands_l%d_row_sweeps" % L, "k_pass2", lpl_of(L), 1, "sweeps", L, nx=96, ny=33, row=16))
    return out


DENSE_CASES = _dense_cases()


def case_volumes(c):
    """The cost volumes of a dense case: nb of them, seeds of their own."""
    out = []
    for k in range(c["nb"]):
        cls = c["classes"][k] if c["classes"] else c["cls"]
        seed = 3 + 17 * k
        if c["row"] is not None:
            out.append(row_volume(cls, seed, c["ny"], c["nx"], c["L"], c["row"]))
        else:
            out.append(volume(cls, seed, c["ny"], c["nx"], c["L"]))
        if c["flat_rows"]:  # every fourth image row `flat`: slabs no penalty stalls, in the same bands as the stalled ones
            out[-1][3::4] = volume("flat", seed, c["ny"], c["nx"], c["L"])[3::4]
    return out


def case_weights(c):
    if c["weights"] is None:
        return None
    p = (0.6, 0.25, 0.15) if len(c["weights"]) == 3 else (0.6, 0.4)
    return np.random.default_rng(5).choice(np.array(c["weights"], f32), size=(8, c["ny"], c["nx"]), p=p).astype(f32)


def stage_counts(groups, LPL, G, L, cap=None):
    """{penalty: slabs [n, L]} -> per direction: slabs ending in stage 0..3 [2, 4], and slabs needing >= GL - 8 plain sweeps
    [2] (loop iterations beyond the three boosted turns).  Every slab is judged ALONE: it fills every lane group of its own
    wave, so the count does not depend on which slabs happen to share a wave.  With `cap`, at most that many slabs per penalty
    are judged, at a fixed stride: the counts are then lower bounds of the run's.
    GL - 8 by arithmetic: a sweep settles one more lane, counted from the first lane of the range in scan order.  The backward
    scan of a padded range starts in padding lanes, +INF and right from the first guess on, so only the ceil(L / LPL) lanes
    that hold labels can need a sweep each: backward the bound is that lane count - 8."""
    GL = 64 // G
    need = (GL - 8, -(-L // LPL) - 8)
    by_stage, long_ = np.zeros((2, 4), int), np.zeros(2, int)
    for pen, S in sorted(groups.items()):
        if cap:
            S = S[::max(1, -(-len(S) // cap))]
        st, its = stages(np.repeat(S, G, axis=0), f32(pen), LPL, G, L)
        st, its = st[::G], its[::G]
        for d in (0, 1):
            by_stage[d] += np.bincount(st[:, d], minlength=4)
            long_[d] += int(((st[:, d] == 3) & (its[:, d] - 3 >= need[d])).sum())
    return by_stage, long_


def floors_met(c, by_stage, long_):
    """The floors of a case as a list of failures (empty: met).  In every direction the case is named for: >= 20 slabs ending
    in its stage; `sweeps`: >= 5 slabs needing >= GL - 8 plain sweeps.  And >= 1 slab of stage 0 in the case, BOTH directions
    taken together, so the hot path runs beside the cold one in the same bands: under a penalty that is not dyadic a padded
    range has no forward stage-0 slab at all (the forward scan's ramp runs on through the padding lanes, one rounding per
    step), and such cases meet this floor through their backward scans."""
    bad = []
    for d in (0, 1):
        if by_stage[d][STAGE_OF[c["stage"]]] < 20:
            bad.append(("stage", d, by_stage[d].tolist()))
        if c["stage"] == "sweeps" and long_[d] < 5:
            bad.append(("long", d, int(long_[d])))
    if by_stage[:, 0].sum() < 1:
        bad.append(("no stage-0 slab", by_stage.tolist()))
    return bad


def dense_counts_from_lr(c, lrs, w8=None):
    """(stage counts, long counts) of the slabs a dense case's min-convolutions read, from the dumped Lr of each of its volumes."""
    by_stage, long_ = np.zeros((2, 4), int), np.zeros(2, int)
    for lr in lrs:
        a, b = stage_counts(slabs_of_run(lr, c["P1"], c["MGM"], w8), c["lpl"], c["groups"], c["L"],
                            cap=800 if STAGE_OF[c["stage"]] == 3 and c["row"] is None else None)  # (the cheap stages, and one row's stragglers: every slab)
        by_stage += a
        long_ += b
    return by_stage, long_


DMIN = -3


def dense_case_counts(c, oracle):
    w8 = case_weights(c)
    return dense_counts_from_lr(c, [oracle.mgm(C, DMIN, c["P1"], c["P1"] * c["P2f"], c["NDIR"], c["MGM"], 1, 1, w8, dump_lr=True)[3]
                                    for C in case_volumes(c)], w8)


# ---- k_pass_rel: ragged ranges over an image pair whose `ad` costs form the one-byte class ---------------------------------------
def rel_case(name, slots, MGM, stage, P1, weights=None, nx=48, ny=32, P2f=20000.0, align=None, rel="2"):
    """rel "2": the range-proportional kernels (k_pass_rel, 16 lanes of slots / 16 slots per pixel); "0": the volume stays on its dense
    hull and k_pass2 takes it, one label range per wave -- with TSGM 2 and no weights through combine_fh2_ragged (mgm_pass2.hip:789-790;
    mgm_pass_common.h: two stand-alone scans of the neighbour's raw slab, then fh_minconv)."""
    hull, width = ((-60, 0), 21) if slots == 64 else ((-200, 10), 100)
    L = hull[1] - hull[0] + 1
    kern = dict(family="k_pass_rel", lpl=slots // 16, groups=4) if rel == "2" else dict(family="k_pass2", lpl=lpl_of(L), groups=1)
    return dict(name=name, slots=slots, hull=hull, width=width, MGM=MGM, stage=stage, P1=float(P1), P2f=P2f, NDIR=8, weights=weights,
                nx=nx, ny=ny, align=align, rel=rel, **kern)


# `s3` / `sweeps`: integers under a penalty that is not dyadic (every chain rounds at every step); `mixed`: a dyadic penalty on
# integers, exact under weight 1 and 2.5 (P1 * w = 2, 5) and not under 0.3 (0.6) -- of the pixel's convolutions side by side
# some are accepted at once and some end in the fall-back loop.  TSGM 1, 2 (FH2, the producer's two stand-alone scans) and 3.
REL_CASES = [
    rel_case("rel_t1_64_s3", 64, 1, "s3", 0.1),
    rel_case("rel_t2_64_fh2_s3", 64, 2, "s3", 0.1),
    rel_case("rel_t3_64_s3", 64, 3, "s3", 0.1),
    rel_case("rel_t3_64_sweeps", 64, 3, "sweeps", float(f32(1.0) / f32(3.0))),
    rel_case("rel_t3_64_mixed", 64, 3, "mixed", 2.0, weights=WEIGHTS3),
    rel_case("rel_t3_64_s1", 64, 3, "s1", 7.0),
    rel_case("rel_t3_128_s3", 128, 3, "s3", 0.1),
    rel_case("rel_t3_128_mixed", 128, 3, "mixed", 2.0, weights=WEIGHTS3),
    rel_case("rel_t2_128_fh2_sweeps", 128, 2, "sweeps", 0.1),
    # stage 2 on one-byte costs comes from the thirds of e / 3 alone (TSGM 1 divides by 1: integers, every addition exact, no stage
    # above 0 with an integer penalty): near-zero COLUMNS of v and windows that slide with x put the pixel's two near-zero costs on
    # the last slot of lane 0 and the first slot of lane 5 in every pixel's frame (`align`: the first's slot, the columns' distance)
    rel_case("rel_t3_64_s2", 64, 3, "s2", 13.0, nx=64, align=(3, 17)),
    # FH2 on the dense hull (combine_fh2_ragged in k_pass2): the same ragged inputs, kept off the range-proportional kernels
    rel_case("hull_t2_61_fh2_s3", 64, 2, "s3", 0.1, rel="0"),
    rel_case("hull_t2_211_fh2_s3", 128, 2, "s3", 0.1, rel="0"),
    # (only stage 3 there: e / 2 of integers is exact, so an integer penalty on these costs never leaves stage 0 -- tried P1 7: 0 of 5680)
]


def rel_case_inputs(c):
    """-> (u, v, lo, hi): the image pair and float range images of exactly `width` labels inside the hull, placed at random."""
    dmin, dmax = c["hull"]
    if c["align"]:
        s0, gap = c["align"]
        rng = np.random.default_rng(11)
        u, v = np.zeros((1, c["ny"], c["nx"]), f32), np.full((1, c["ny"], c["nx"]), 250.0, f32)
        for X in (0, gap):
            v[0, :, X] = rng.integers(0, 3, c["ny"])
        # v's column 0 meets pixel x at disparity -x: slot s0 of a window that starts at -x - s0 + 1 (clipped into the hull)
        lo = np.repeat(np.clip(-np.arange(c["nx"]) - s0 + 1, dmin, dmax - c["width"] + 1).astype(f32)[None], c["ny"], 0)
    else:
        u, v = ad_pair(11, c["ny"], c["nx"], zeros=max(3, c["nx"] // 6))
        rng = np.random.default_rng(12)
        lo = rng.integers(dmin, dmax - c["width"] + 2, (c["ny"], c["nx"])).astype(f32)
    hi = lo + f32(c["width"] - 1)
    lo[0, 0], hi[0, 0] = dmin, dmin + c["width"] - 1  # the hull is attained
    lo[0, 1], hi[0, 1] = dmax - c["width"] + 1, dmax
    return u, v, lo, hi


def rel_case_counts(c, lr_dump, ilo, ihi, w8=None):
    """Stage counts of a ragged run's min-convolutions from its dumped Lr (hull layout, +INF outside a pixel's range): the
    neighbour's slab over the RECEIVING pixel's range (mgm_core.cc:242-271), in the kernel's frame -- the range from slot 1 on,
    16 lanes of `lpl` slots.  (TSGM 2 without weights: before the boundary fix-up folds the outside into the two end labels.)
    -> (per direction slabs ending in stage 0..3 [2, 4], slabs needing >= 16 - 8 plain sweeps [2] -- backward the lanes that
    hold labels - 8, at least 1, as in stage_counts: a window of 21 labels fills 6 lanes --, pixels whose convolutions side by
    side hold both an accepted first guess and a fall-back)."""
    hmin = c["hull"][0]
    need = (8, max(1, -(-(c["width"] + 1) // c["lpl"]) - 8))
    slots, L = c["slots"], lr_dump.shape[3]
    G, first = 4, 1
    if c["rel"] == "0":  # the dense hull: label o in slot o of 64 lanes
        slots, G, first = L, 1, None
    by_stage, long_, mixed = np.zeros((2, 4), int), np.zeros(2, int), 0
    per_pixel = {}
    for p, k, ys, xs, S, D in neighbour_terms(lr_dump, c["MGM"], w8):
        a, b = ilo[ys, xs] - hmin, ihi[ys, xs] - hmin
        idx = (a[:, None] - first if first is not None else 0) + np.arange(slots)[None, :]
        own = (idx >= a[:, None]) & (idx <= b[:, None])
        M = np.where(own, np.take_along_axis(S, np.clip(idx, 0, L - 1), 1), INF).astype(f32)
        pen = f32(c["P1"]) * D
        worst = np.zeros(len(ys), int)
        for v in np.unique(pen):
            sel = np.nonzero(pen == v)[0][::4]  # (a quarter of the pixels: lower bounds)
            st, its = stages(np.repeat(M[sel], G, axis=0), v, c["lpl"], G, slots)
            st, its = st[::G], its[::G]
            for d in (0, 1):
                by_stage[d] += np.bincount(st[:, d], minlength=4)
                long_[d] += int(((st[:, d] == 3) & (its[:, d] - 3 >= need[d])).sum())
            worst[sel] = 1 + (st.max(1) > 0)  # 1: both scans accepted at once, 2: a fall-back
        per_pixel.setdefault(p, []).append(worst)
    for p, ws in per_pixel.items():
        w = np.stack(ws)
        mixed += int((((w == 1).any(0)) & ((w == 2).any(0))).sum())
    return by_stage, long_, mixed


def rel_floors_met(c, by_stage, long_, mixed):
    bad = []
    for d in (0, 1):
        if c["stage"] in STAGE_OF and by_stage[d][STAGE_OF[c["stage"]]] < 20:
            bad.append(("stage", d, by_stage[d].tolist()))
        if c["stage"] == "sweeps" and long_[d] < 5:
            bad.append(("long", d, int(long_[d])))
    if c["stage"] == "mixed" and mixed < 20:
        bad.append(("mixed", mixed))
    if by_stage[:, 0].sum() < 1:
        bad.append(("no stage-0 slab", by_stage.tolist()))
    return bad
