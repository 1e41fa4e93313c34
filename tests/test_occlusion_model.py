"""The numpy model of hole classification and the classified fill (tests/occlusion_model.py) against plain loops that
walk every xr and every ray, the properties the definition promises, a planted scene with known occlusions, plan_holes_classify on
the host, what the binding, the header and --help expose, and the command line's early refusals."""
import inspect
import os
import subprocess

import numpy as np
import pytest

import mgm_amd
from holes_model import STEPS, crafted, fill, rays, same_bits
from occlusion_model import (MODES5, RANGES, SCENE, TAUS, classify, crafted_d, crafted_other, fill_classified, plan, plan_lib,
                             planted_scene)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
f32 = np.float32
INT_MAX = 2 ** 31 - 1


# ---- the definition with loops -----------------------------------------------------------------------------------------------------
def classify_loops(d, other, dmin, dmax, tau):
    d, other = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(other, np.float32)
    (ny, nx), vnx = d.shape, other.shape[1]
    cls = np.zeros((ny, nx), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for y in range(ny):
            for x in range(nx):
                if np.isfinite(d[y, x]):
                    continue
                cls[y, x] = 1
                for xr in range(max(0, x + dmin), min(vnx - 1, x + dmax) + 1):
                    o = other[y, xr]
                    if np.isfinite(o) and np.abs(f32(f32(xr) + o) - f32(x)) <= f32(tau):
                        cls[y, x] = 2
                        break
    return cls


def march_classified(d, cls, mode_occ, mode_mis, dirs, maxdist):
    """every hole marches every ray (tests/test_holes_model.march), then picks by its class"""
    d = np.ascontiguousarray(d, np.float32)
    ny, nx = d.shape
    out, filled = d.copy(), np.zeros((ny, nx), np.float32)
    for y in range(ny):
        for x in range(nx):
            if np.isfinite(d[y, x]):
                continue
            cands = []
            for k in range(dirs):
                sx, sy = STEPS[k]
                t = 1
                while 0 <= x + t * sx < nx and 0 <= y + t * sy < ny and (maxdist == 0 or t <= maxdist):
                    q = d[y + t * sy, x + t * sx]
                    if np.isfinite(q):
                        cands.append(q)
                        break
                    t += 1
            if not cands:
                continue
            v = []  # a stable insertion sort: an element moves past strictly larger ones only
            for c in cands:
                i = len(v)
                while i > 0 and v[i - 1] > c:
                    i -= 1
                v.insert(i, c)
            n = len(v)
            mode = mode_occ if cls[y, x] == 1 else mode_mis
            out[y, x] = {"min": v[0], "max": v[-1], "median": v[n // 2], "seclow": v[min(1, n - 1)], "sechigh": v[max(n - 2, 0)]}[mode]
            filled[y, x] = 1
    return out, filled


SMALL = [(1, 1), (1, 3), (7, 1), (5, 4), (12, 9), (9, 12)]  # (nx, ny)


def odd_classes(d, seed):
    """a class map with 0, 1, 2, NaN and 7 at the holes (and anything on the valid pixels, where it is not read)"""
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 1, 1, 2, np.nan, 7], np.float32), size=d.shape).astype(np.float32)


def test_classify_matches_the_loops():
    n = 0
    for nx, ny in SMALL:
        for vnx in (nx + 7, max(1, nx - 5)):
            for dmin, dmax in RANGES + ((-2, 1), (5, 7)):
                for tau in TAUS:
                    other = crafted_other(nx, ny, vnx, dmin, dmax, tau)
                    for name, d in crafted_d(nx, ny, seg=8, lane=4):
                        got, want = classify(d, other, dmin, dmax, tau), classify_loops(d, other, dmin, dmax, tau)
                        assert same_bits(got, want), (nx, ny, vnx, dmin, dmax, tau, name)
                        assert np.array_equal(got == 0, np.isfinite(d))        # 0 exactly on the finite pixels
                        assert np.isin(got[~np.isfinite(d)], (1, 2)).all()
                        n += 1
    assert n == len(SMALL) * 2 * 7 * 4 * 4


def test_the_crafted_inputs_reach_what_they_are_there_for():
    nx, ny, vnx = 130, 3, 137
    seen = {1: 0, 2: 0}
    for dmin, dmax in RANGES:
        for tau in TAUS:
            other = crafted_other(nx, ny, vnx, dmin, dmax, tau)
            assert np.isnan(other).any() and np.isposinf(other).any() and np.isneginf(other).any() and (np.abs(other) == f32(1e30)).any()
            assert ((other == 0) & np.signbit(other)).any()
            cls = classify(np.full((ny, nx), np.nan, np.float32), other, dmin, dmax, tau)
            for k in seen:
                seen[k] += int((cls == k).sum())
            if (dmin, dmax) == (60, 66):  # wholly outside `other` for the right part of every row: occlusions
                assert (cls[:, vnx - 60:] == 1).all() and (cls[:, :vnx - 60] == 2).any()
            # exactly on tau and one ulp to either side: raising tau by one ulp, or lowering it, moves some hole
            up, down = classify(np.full((ny, nx), np.nan, np.float32), other, dmin, dmax, np.nextafter(f32(tau), f32(9))), None
            if tau > 0:
                down = classify(np.full((ny, nx), np.nan, np.float32), other, dmin, dmax, np.nextafter(f32(tau), f32(0)))
            if (dmin, dmax) in ((3, 9), (-9, -3), (-300, 300)) and tau > 0:
                assert (up != cls).any() or (down != cls).any(), (dmin, dmax, tau)
    assert seen[1] > 1000 and seen[2] > 1000
    names = [n for n, _ in crafted_d(130, 3)]
    assert names == ["all_holes", "no_holes", "boundaries", "random"]
    b = dict(crafted_d(257, 3))["boundaries"]
    assert np.isnan(b[:, [0, 63, 64, 127, 128, 255, 256]]).all() and np.isfinite(b[:, [1, 62, 65, 254]]).all()


def test_wider_ranges_and_larger_tau_only_move_holes_from_occlusion_to_mismatch():
    nx, ny, vnx = 40, 5, 47
    d = dict(crafted_d(nx, ny))["random"]
    for dmin, dmax in ((3, 9), (-9, -3), (0, 0)):
        for tau in TAUS:
            other = crafted_other(nx, ny, vnx, dmin, dmax, tau)
            base = classify(d, other, dmin, dmax, tau)
            for a, b, t in ((dmin - 1, dmax, tau), (dmin, dmax + 2, tau), (dmin - 30, dmax + 30, tau), (dmin, dmax, tau + 0.25), (dmin, dmax, tau + 3)):
                wide = classify(d, other, a, b, t)
                assert ((wide == 0) == (base == 0)).all() and (wide >= base).all(), (dmin, dmax, tau, a, b, t)
    assert (classify(d, other, -30, 30, 5.5) > classify(d, other, 0, 0, 0)).any()


def test_fill_classified_matches_the_marched_rays():
    n = 0
    for nx, ny in ((5, 4), (12, 9)):
        for name, d in crafted(nx, ny, chunk=4, band=3):
            r = rays(d)
            cls = odd_classes(d, n)
            for mo in MODES5:
                for mm in MODES5:
                    for dirs, maxdist in ((8, 0), (4, 2), (2, 0)):
                        got = fill_classified(d, cls, mo, mm, dirs, maxdist, r=r)
                        want = march_classified(d, cls, mo, mm, dirs, maxdist)
                        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (name, mo, mm, dirs, maxdist)
                        n += 1
    assert n == 2 * len(crafted(5, 4)) * 25 * 3


def test_one_rule_for_both_classes_is_the_plain_fill():
    for nx, ny in ((12, 9), (40, 23)):
        for name, d in crafted(nx, ny, chunk=8, band=4):
            r = rays(d)
            cls = odd_classes(d, 3)
            for mode in ("median", "min", "max"):
                for dirs, maxdist in ((8, 0), (4, 0), (2, 0), (8, 2)):
                    got, want = fill_classified(d, cls, mode, mode, dirs, maxdist, r=r), fill(d, mode, dirs, maxdist, r=r)
                    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (name, mode, dirs, maxdist)


def test_the_five_rules_are_ordered():
    """min <= seclow <= median <= sechigh <= max at every filled hole with n >= 3 candidates; with one candidate all five agree"""
    seen3 = seen1 = 0
    for nx, ny in ((12, 9), (40, 23)):
        for name, d in crafted(nx, ny, chunk=8, band=4):
            r = rays(d)
            ones = np.ones(d.shape, np.float32)
            for dirs, maxdist in ((8, 0), (4, 0), (8, 2), (2, 1)):
                has = (r[1][:dirs] >= 1) & ((r[1][:dirs] <= maxdist) if maxdist else True)
                n = has.sum(axis=0)
                hole = ~np.isfinite(d)
                o = {m: fill_classified(d, ones, m, m, dirs, maxdist, r=r)[0] for m in MODES5}
                m3, m1 = hole & (n >= 3), hole & (n == 1)
                for a, b in zip(("min", "seclow", "median", "sechigh"), ("seclow", "median", "sechigh", "max")):
                    assert (o[a][m3] <= o[b][m3]).all(), (name, a, b)
                for m in MODES5:
                    assert same_bits(o[m][m1], o["min"][m1])
                seen3, seen1 = seen3 + int(m3.sum()), seen1 + int(m1.sum())
    assert seen3 > 1000 and seen1 > 100


# ---- the planted scene ---------------------------------------------------------------------------------------------------------------
def test_planted_scene_classes():
    s = SCENE
    left, right, holes, occluded, strip = planted_scene()
    hole = ~np.isfinite(holes)
    planted = hole & ~occluded
    assert (s["nx"], s["ny"]) == (96, 24) and occluded.sum() == 132 and strip.sum() == 84 and planted.sum() > 150
    cls0 = classify(holes, right, s["dmin"], s["dmax"], 0.0)
    print("tau 0: %d of %d occluded holes are class 1, %d of %d planted holes class 2" % ((cls0[occluded] == 1).sum(), occluded.sum(),
                                                                                        (cls0[planted] == 2).sum(), planted.sum()))
    assert (cls0[occluded] == 1).all() and (cls0[planted] == 2).all()
    prev = cls0 == 1
    for tau in (1.0, 2.0):
        c = classify(holes, right, s["dmin"], s["dmax"], tau)
        now = c == 1
        print("tau %g: class 1 on %d holes" % (tau, now.sum()))
        assert (c[planted] == 2).all() and (now <= prev).all() and not (now & ~occluded).any()   # (the columns near the edge may flip)
        prev = now


def test_planted_scene_background_fills_the_strip():
    """sechigh for the occlusions, median for the mismatches: every filled occluded hole of the strip beside the block takes the
    background's -2, while plain `median` puts the foreground's -9 into some of them.

    Where the two rules part is a matter of which rays reach what, so the fill's distance bound matters, and it is the scene's
    geometry that sets it (SCENE["fill_dist"] = 6): the strip is 7 columns wide (33..39) beside a block 12 rows tall (6..17), with
    background 6 rows above and below the block's two middle rows.  At a bound of 6 steps a hole in column 39 of row 11 reaches the
    foreground along (+1,0) (+1,+1) (+1,-1) at one step, and background along exactly two rays, (0,-1) and (-1,-1) at six steps (row
    5); (-1,0), (0,+1) and (-1,+1) need seven.  Its candidates are [-9 -9 -9 -2 -2]: the upper median v[2] is -9, sechigh v[3] is
    -2.  Every other strip hole has at least two background candidates within six steps as well (further left the row's background
    comes into reach, further up or down the column's), so sechigh gives -2 throughout.  With a bound of 7 or none all five rays
    that do not head for the block reach background, and v[4] of [-9 -9 -9 -2 -2 -2 -2 -2] is -2 under the plain median too: an
    8-ray median cannot fail across a straight edge unless the bound hides the background, which is asserted below as well."""
    s = SCENE
    left, right, holes, occluded, strip = planted_scene()
    cls = classify(holes, right, s["dmin"], s["dmax"], 0.0)
    r = rays(holes)
    bg, fg = f32(s["bg"]), f32(s["fg"])
    out, filled = fill_classified(holes, cls, "sechigh", "median", 8, s["fill_dist"], r=r)
    plain, pfilled = fill(holes, "median", 8, s["fill_dist"], r=r)
    got = strip & (filled == 1)
    wrong = int((plain[got] == fg).sum())
    print("maxdist %d: %d of %d strip holes filled, -9 in %d of them (sechigh / median) and in %d (plain median)"
          % (s["fill_dist"], got.sum(), strip.sum(), (out[got] == fg).sum(), wrong))
    assert got.sum() == strip.sum() == 84 and np.array_equal(filled, pfilled)
    assert (out[got] == bg).all()                          # every filled occluded hole of the strip takes -2 ...
    assert wrong > 0 and (plain[got & (plain != fg)] == bg).all()   # ... while plain median puts -9 into some of them
    assert plain[11, 39] == fg and out[11, 39] == bg       # the hole of the docstring
    # without a bound (and from 7 steps on) both rules see five background candidates of eight
    for maxdist in (0, 7):
        o2, f2 = fill_classified(holes, cls, "sechigh", "median", 8, maxdist, r=r)
        p2, _ = fill(holes, "median", 8, maxdist, r=r)
        assert (f2[strip] == 1).all() and (o2[strip] == bg).all()
        if maxdist == 0:
            assert (p2[strip] == bg).all()
    # ... and the planted mismatches take their own side's value back wherever the median can tell
    planted = ~np.isfinite(holes) & ~occluded
    o0 = fill_classified(holes, cls, "sechigh", "median", r=r)[0]
    assert (o0[planted] == left[planted]).mean() > 0.95


def test_wedge_scene():
    """A wedge of background pointing into the foreground: inside it up to five or six of a hole's rays reach foreground, the plain
    median takes the foreground's -9 there, the background rule (sechigh, negative disparities) does so at fewer holes -- only where
    fewer than two rays reach background at all."""
    s = SCENE
    left, right, holes, occluded, strip = planted_scene(wedge=True)
    cls = classify(holes, right, s["dmin"], s["dmax"], 0.0)
    hole = ~np.isfinite(holes)
    assert (cls[occluded] == 1).all() and (cls[hole & ~occluded] == 2).all()
    r = rays(holes)
    out, _ = fill_classified(holes, cls, "sechigh", "median", r=r)
    plain, _ = fill(holes, "median", r=r)
    wrong_cls, wrong_plain = int((out[strip] == f32(s["fg"])).sum()), int((plain[strip] == f32(s["fg"])).sum())
    print("wedge: -9 in %d (classified) and %d (plain median) of %d strip holes" % (wrong_cls, wrong_plain, strip.sum()))
    assert 0 < wrong_plain and wrong_cls < wrong_plain
    nbg = ((r[0].view(np.float32) == f32(s["bg"])) & (r[1] >= 1)).sum(axis=0)      # rays that reach background
    assert (nbg[strip & (out == f32(s["fg"]))] < 2).all() and (out[strip & (nbg >= 2)] == f32(s["bg"])).all()
    mis = hole & ~occluded
    assert same_bits(out[mis], plain[mis])                                         # the mismatches keep the median


# ---- plan_holes_classify -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = plan_lib(tmp_path_factory.mktemp("holesclsplan"))
    assert lib.holes_classify_request_bytes() == 4 * 4 + 8 and lib.holes_classify_choice_bytes() == 2 * 8 + 4 * 4
    return lib


PLAN_SHAPES = [(1, 1), (1, 9), (7, 1), (63, 3), (64, 64), (65, 70), (257, 3), (1920, 1080), (1080, 1920), (INT_MAX, 1), (1, INT_MAX), (46340, 46340)]


def test_plan_covers_the_map_for_every_range_length(lib):
    threads, max_span = lib.holes_classify_threads(), lib.holes_classify_max_span()
    for nx, ny in PLAN_SHAPES:
        for vnx in {max(1, nx - 5), nx, min(INT_MAX, nx + 7)}:
            Ls = list(range(1, 70)) + [127, 128, 129, 255, 256, 257, 601, 1023, 1024, 1025, 4095, 4096, 2 ** 32]
            rows = [(nx, ny, vnx, L, 256) for L in Ls]
            for (_, _, _, L, _), c in zip(rows, plan(lib, rows)):
                assert c["family"] == 1 and c["seg"] == threads, (nx, ny, vnx, L)
                assert c["grid_x"] >= 1 and (c["grid_x"] - 1) * c["seg"] < nx <= c["grid_x"] * c["seg"]      # the segments cover a row
                assert 1 <= c["grid_y"] <= min(ny, 65535) and (c["grid_y"] == ny or c["grid_y"] == 65535)   # rows: strided, none left out
                assert c["span"] % 64 == 0 and 64 <= c["span"] <= max_span
                named = min(L + c["seg"] - 1, vnx)                                                            # columns a segment can name
                assert c["span"] >= min(named, max_span)          # any L: what does not fit one span is a loop over spans, never a cap
                assert c["lds_bytes"] == 4 * (c["span"] + c["seg"] + 8) <= 65536
    for L in range(1, 4097):                                                                                  # every L from 1 to 4096
        c = plan(lib, [(1920, 1080, 1920, L, 256)])[0]
        assert c["family"] == 1 and min(L + 255, 1920, max_span) <= c["span"] <= max_span


def test_plan_refusals(lib):
    bad = [(0, 5), (5, 0), (-1, 5), (5, -1), (INT_MAX, 2), (2, INT_MAX), (46341, 46341), (65536, 32768)]   # what plan_holes refuses
    for (nx, ny), c in zip(bad, plan(lib, [(nx, ny, 10, 5, 256) for nx, ny in bad])):
        assert all(v == 0 for v in c.values()), (nx, ny)
    for vnx, L in ((0, 5), (-3, 5), (10, 0), (10, -1)):
        assert plan(lib, [(10, 10, vnx, L, 256)])[0]["family"] == 0
    ok = [(INT_MAX, 1), (1, INT_MAX), (46340, 46340), (65536, 32767)]
    assert all(c["family"] == 1 for c in plan(lib, [(nx, ny, nx, 65, 256) for nx, ny in ok]))


def test_plan_is_a_function_of_the_request_alone(lib):
    rng = np.random.default_rng(5)
    rows = [(int(rng.integers(1, 5000)), int(rng.integers(1, 5000)), int(rng.integers(1, 5000)), int(rng.integers(1, 5000)), int(rng.integers(0, 400)))
            for _ in range(300)]
    first = plan(lib, rows)
    assert first == plan(lib, rows[::-1])[::-1] and first == [plan(lib, [r])[0] for r in rows]


# ---- binding, header, command line ---------------------------------------------------------------------------------------------------
def test_binding_and_header_list_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "mgm_hip.h")).read()
    for name in ("mgm_classify_holes_dev", "mgm_fill_holes_classified_dev"):
        assert name in mgm_amd.ABI_SYMBOLS and hasattr(mgm_amd.load_library(), name)
    assert "mgm_classify_holes_dev(mgm_ctx *ctx, const mgm_img *d, const mgm_img *other, int dmin, int dmax, float tau, mgm_img *cls)" in hdr
    assert "mgm_fill_holes_classified_dev(mgm_ctx *ctx, const mgm_img *d, const mgm_img *cls, const char *mode_occ, const char *mode_mis," in hdr
    assert "mgm_img *outR_nolr;" in hdr and hdr.index("mgm_img *outR_nolr;") > hdr.index("mgm_ms_level *levels;")
    assert mgm_amd.MsParams._fields_[-1][0] == "outR_nolr" and mgm_amd.MsParams._fields_[-2][0] == "levels"
    sig = lambda f: list(inspect.signature(getattr(mgm_amd.Context, f)).parameters)[1:]
    assert sig("classify_holes_dev") == ["d", "other", "dmin", "dmax", "tau", "cls"]
    assert sig("fill_holes_classified_dev") == ["d", "cls", "mode_occ", "mode_mis", "dirs", "maxdist", "out", "want_filled"]
    p = inspect.signature(mgm_amd.Context.fill_holes_classified_dev).parameters
    assert (p["mode_occ"].default, p["mode_mis"].default, p["dirs"].default, p["maxdist"].default) == ("sechigh", "median", 8, 0)
    assert inspect.signature(mgm_amd.Context.multiscale_pair).parameters["want_right_nolr"].default is False


def run_cli(args, env):
    e = dict(os.environ)
    e.update(env)
    return subprocess.run([MGM] + args, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)


def test_help_states_the_step():
    r = run_cli(["--help"], {})
    assert r.returncode == 0
    for word in ("MGM_FILL_HOLES_OCC=none", "seclow, sechigh, min, max or median", "TESTLRRL_TAU", "sechigh for a range like -r -64 -R 0",
                 "needs the right view", "exit code 2",
                 # ... and every word tests/test_holes_model.py looks for is still there
                 "MGM_FILL_HOLES=none", "MGM_FILL_HOLES_DIRS=8", "MGM_FILL_HOLES_DIST=0", "after MGM_SPECKLE", "before the back-projected image",
                 "(+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,+1) (+1,-1) (-1,-1)"):
        assert word in r.stdout, word


@pytest.mark.parametrize("env,start,word", [
    ({"MGM_FILL_HOLES": "median", "MGM_FILL_HOLES_OCC": "second"}, "mgm: MGM_FILL_HOLES_OCC must", ""),
    ({"MGM_FILL_HOLES": "median", "MGM_FILL_HOLES_OCC": "Sechigh"}, "mgm: MGM_FILL_HOLES_OCC must", ""),
    ({"MGM_FILL_HOLES": "median", "MGM_FILL_HOLES_OCC": "1"}, "mgm: MGM_FILL_HOLES_OCC must", ""),
    ({"MGM_FILL_HOLES_OCC": "mean"}, "mgm: MGM_FILL_HOLES_OCC must", ""),
    ({"MGM_FILL_HOLES_OCC": "sechigh"}, "mgm: MGM_FILL_HOLES_OCC", "needs MGM_FILL_HOLES"),
    ({"MGM_FILL_HOLES": "none", "MGM_FILL_HOLES_OCC": "seclow"}, "mgm: MGM_FILL_HOLES_OCC", "needs MGM_FILL_HOLES"),
    ({"MGM_FILL_HOLES": "", "MGM_FILL_HOLES_OCC": "median"}, "mgm: MGM_FILL_HOLES_OCC", "needs MGM_FILL_HOLES")])
def test_cli_refuses_bad_parameters_before_any_work(env, start, word):
    """Exit code 1 and one line on stderr when the command line is parsed: no device, no input file."""
    r = run_cli(["no_u.png", "no_v.png", "no_out.tif"], env)
    assert r.returncode == 1 and r.stderr.startswith(start) and word in r.stderr and len(r.stderr.splitlines()) == 1 and r.stdout == ""


def test_cli_needs_the_right_view_before_any_device_work():
    """TESTLRRL=0 leaves no right map to classify from (MGM_RIGHT_FROM_LEFT is off without TESTLRRL): exit code 2, no input file read"""
    for env in ({"TESTLRRL": "0"}, {"TESTLRRL": "0", "MGM_RIGHT_FROM_LEFT": "1"}):
        r = run_cli(["no_u.png", "no_v.png", "no_out.tif"], dict(env, MGM_FILL_HOLES="median", MGM_FILL_HOLES_OCC="sechigh"))
        assert r.returncode == 2 and "needs the right view" in r.stderr and len(r.stderr.splitlines()) == 1
