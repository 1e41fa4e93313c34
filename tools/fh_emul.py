"""Development aid (CPU): run the numpy restatement of fh_scan's stages (tests/fh_stage_model.py -- the one copy) on the
per-pass Lr slabs of a real census volume and report how often the first sweep rejects the guess (default), how many loop
iterations the rejected slabs take (HIST=1), and how often fh_repair alone would be wrong (REPAIR=1)."""
import os, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle.oracle import Oracle
from mgm_amd import synth
from fh_stage_model import guess, origin, repair, seq_scan, stages, waves

f32 = np.float32
LPL = 4


def run_slabs(P1):
    nx, ny, L = int(os.environ.get("NX", 384)), 40, 256
    u, v, _ = synth.stereo_pair(nx, ny, -(L - 1) * 3 // 4, 0)
    o = Oracle(threads=8)
    Cv = o.costvolume(u, v, -(L - 1), 0, "none", "census", np.inf, 5)
    _, _, _, lr = o.mgm(Cv, -(L - 1), float(P1), 20000.0, 8, 3, FH=1, FIX=1, dump_lr=True)
    return lr.reshape(-1, L)


def check(M, P1, fwd):
    """-> (lanes whose guessed carry is wrong [N, 64], guess, sequential carries)"""
    X = waves(M, LPL, 1, M.shape[1])
    c = guess(origin(X, P1, fwd), P1, LPL, fwd)
    t = seq_scan(M, P1, fwd).reshape(-1, 64, LPL)[:, :, LPL - 1 if fwd else 0]
    return c != t, c, t


def main():
    P1 = f32(2.0)
    M = run_slabs(P1)
    F = seq_scan(M, P1, True)
    badf, cf, tf = check(M, P1, True)
    badb, cb, tb = check(F, P1, False)
    print("slabs", M.shape[0], "fwd rejected %.3f%%" % (100 * badf.any(1).mean()), "bwd rejected %.3f%%" % (100 * badb.any(1).mean()))
    for name, bad, c, t, src in (("fwd", badf, cf, tf, M), ("bwd", badb, cb, tb, F)):
        for i in np.nonzero(bad.any(1))[0][:3]:
            lanes = np.nonzero(bad[i])[0]
            print(name, "slab", i, "lanes", lanes[:8], "guess", c[i, lanes[:4]], "true", t[i, lanes[:4]])
            print("   n_inf", int(np.isinf(src[i]).sum()), "min", float(src[i][np.isfinite(src[i])].min()) if np.isfinite(src[i]).any() else None,
                  "values near", src[i].reshape(64, LPL)[max(lanes[0] - 2, 0):lanes[0] + 2].ravel())


def hist():
    P1 = f32(2.0)
    M = run_slabs(P1)
    st, its = stages(M, P1, LPL, 1, M.shape[1])
    for d, name in enumerate(("fwd", "bwd")):
        print(name, "stage of the accepted carries (guess, careful, repair, plain sweeps):", np.bincount(st[:, d], minlength=4),
              "loop iterations histogram:", np.bincount(np.minimum(its[:, d], 20))[:21])


def check_repair():
    for P1 in (f32(2.0), f32(8.0), f32(3.0), f32(2.5)):
        M = run_slabs(P1)
        for fwd in (True, False):
            src = M if fwd else seq_scan(M, P1, True)
            c = repair(origin(waves(src, LPL, 1, src.shape[1]), P1, fwd), P1, LPL, fwd)
            t = seq_scan(src, P1, fwd).reshape(-1, 64, LPL)[:, :, LPL - 1 if fwd else 0]
            print("P1", P1, "fwd" if fwd else "bwd", "repair wrong on %.4f%% of slabs" % (100.0 * (c != t).any(1).mean()))


if __name__ == "__main__":
    check_repair() if os.environ.get("REPAIR") else (hist() if os.environ.get("HIST") else main())
