"""Inputs for the pruned winner search laid out as eight lanes per pixel (k_wta_pruned, mgm_amd/csrc/mgm_wta.hip): a wave works on
eight consecutive pixels at once and walks their candidate chunks in rounds, so what can go wrong is NEIGHBOURS that need very different
numbers of chunks, and chunks that no longer arrive by rising label.  Both generators give integer costs <= 133 (the compact path).
tests/test_wta_groups.py measures what they are worth on the CPU; tests/test_gpu_wta_groups.py runs them on the device."""
import numpy as np

from wta_prune_model import CHUNK, INSTANCE_CASES, RAMP_DMIN, pruned_search, ramp_volume, sum_fix, vfit_step

GROUP = 8  # consecutive pixels (row-major) a wave's lanes work on together


def mixed_volume(nx, ny, s):
    """Neighbours that need 1 chunk next to neighbours that need 7-8."""
    C = ramp_volume(nx, ny, 256, s)
    y, x = np.mgrid[:ny, :nx]
    sharp = (x + y) % 2 == 0
    flat = (x + y) % 4 == 1
    Cs = np.full((ny, nx, 256), 120.0, np.float32)
    np.put_along_axis(Cs, ((x * 37 + y * 11) % 256)[..., None], 0.0, axis=2)
    C[sharp] = Cs[sharp]
    C[flat] = 60.0
    return C


def periodic_volume(nx, ny, s):
    """Equal S in two chunks, the seed often the HIGHER one."""
    C = ramp_volume(nx, ny, 256, s)
    C = np.where(np.isfinite(C), C, 120.0).astype(np.float32)
    C[:, :, 128:] = C[:, :, :128]
    rng = np.random.default_rng(s + 200)
    C[(rng.random(C.shape) < 0.15) & (C >= 30)] += 1.0
    return C


GENERATORS = {"mixed": mixed_volume, "periodic": periodic_volume}
SEED = 7
FH, HI = (1, 2.0, 20000.0), (0, 8.0, 32.0)  # (FH, P1, P2): the potentials of the table below
MGM = 3  # TSGM
# name: (generator, nx, ny, (FH, P1, P2), NDIR, floor); fix_overcount 1, dmin RAMP_DMIN, seed SEED
#   floor "mixed":    at least 1/4 of the groups hold a pixel loading >= 7 chunks AND one loading <= 2
#   floor "periodic": at least 20 pixels whose smallest finite loaded S sits in two loaded chunks, at least 10 of them with the
#                     winner's chunk BELOW the seed
GROUP_CASES = {
    "mixed33_fh8": ("mixed", 33, 17, FH, 8, "mixed"),
    "mixed33_hi8": ("mixed", 33, 17, HI, 8, "mixed"),
    "mixed16_fh8": ("mixed", 16, 3, FH, 8, "mixed"),
    "mixed16_hi8": ("mixed", 16, 3, HI, 8, "mixed"),
    "periodic33_hi8": ("periodic", 33, 17, HI, 8, "periodic"),
    "periodic33_hi4": ("periodic", 33, 17, HI, 4, "periodic"),
    "periodic16_hi8": ("periodic", 16, 3, HI, 8, "periodic"),
}

_ref = {}


def reference(oracle, gen, nx, ny, pot, NDIR, seed=SEED, fix=1):
    """Computed once and left read-only: the costs C, the oracle's lr and maps without refinement (out, outc) and after vfit (vout,
    voutc), the emulation's maps and S (label, cost, vlabel, vcost, Sm), its chunk count, load set and bound LB."""
    key = (gen, nx, ny, pot, NDIR, seed, fix)
    if key not in _ref:
        C = GENERATORS[gen](nx, ny, seed) if gen in GENERATORS else ramp_volume(nx, ny, 256, seed)
        S, out, outc, lr = oracle.mgm(C, RAMP_DMIN, pot[1], pot[2], NDIR, MGM, pot[0], fix, dump_lr=True)
        vout, voutc = oracle.refine(S, RAMP_DMIN, "vfit", out, outc)
        label, cost, chunks, Sm, LB, load = pruned_search(C, lr, RAMP_DMIN, fix)
        vlabel, vcost, nout = vfit_step(Sm, load, RAMP_DMIN, label, cost)
        r = dict(C=C, lr=lr, S=S, out=out, outc=outc, vout=vout, voutc=voutc, label=label, cost=cost, chunks=chunks, Sm=Sm, LB=LB, load=load,
                 vlabel=vlabel, vcost=vcost, nout=nout)
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ref[key] = r
    return _ref[key]


def case_reference(oracle, name):
    gen, nx, ny, pot, NDIR, _ = GROUP_CASES[name]
    return reference(oracle, gen, nx, ny, pot, NDIR)


def groups_spread(load):
    """(groups holding a pixel that loads >= 7 chunks AND one that loads <= 2, groups): 8 consecutive pixels in row-major order,
    the last group padded with its own last pixel."""
    n = load.reshape(-1, load.shape[2]).sum(axis=1)
    pad = (-len(n)) % GROUP
    n = np.concatenate([n, np.full(pad, n[-1])]).reshape(-1, GROUP)
    return int(((n.max(axis=1) >= 7) & (n.min(axis=1) <= 2)).sum()), len(n)


def ties_across_chunks(r):
    """(pixels whose smallest finite loaded S sits in two or more loaded chunks, those of them whose winner's chunk lies below
    the seed chunk)."""
    ny, nx, L = r["C"].shape
    nch = L // CHUNK
    Sc = np.where(np.isfinite(r["Sm"]), r["Sm"], np.inf).reshape(ny, nx, nch, CHUNK)
    cmin = np.where(r["load"], Sc.min(axis=3), np.inf)
    best = cmin.min(axis=2)
    tied = ((cmin == best[..., None]) & (best[..., None] < np.inf)).sum(axis=2) >= 2
    lb = chunk_bound_fold(r["C"], r["LB"])
    seed = np.argmax(lb == lb.min(axis=2)[..., None], axis=2)
    win = np.argmax(cmin == best[..., None], axis=2)
    return int(tied.sum()), int((tied & (win < seed)).sum())


def chunk_bound_fold(C, LB):
    """Step (a) as wta_prune_model.pruned_search has it: per chunk, the smallest bound over its labels with a finite cost, a NaN bound
    dropped; +INF where nothing is left."""
    ny, nx, L = C.shape
    return np.where((C < np.inf) & ~np.isnan(LB), LB, np.inf).astype(np.float32).reshape(ny, nx, L // CHUNK, CHUNK).min(axis=3)


def chunk_bound_largest_cost(C, minima, fix):
    """Step (a) as the kernel has it: ONE evaluation of the sum-and-fix chain per chunk, on the minima and the chunk's LARGEST finite
    cost (s - f*c does not rise with c); a chunk without a finite cost gives +INF, a NaN result is dropped to +INF."""
    ny, nx, L = C.shape
    Cc = C.reshape(ny, nx, L // CHUNK, CHUNK)
    fin = Cc < np.inf
    cmax = np.where(fin, Cc, -np.inf).max(axis=3)
    some = fin.any(axis=3)
    b = sum_fix([minima[p] for p in range(minima.shape[0])], np.where(some, cmax, 0.0).astype(np.float32), fix)
    return np.where(some & ~np.isnan(b), b, np.inf).astype(np.float32)
