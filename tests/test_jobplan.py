"""plan_job and refuse_on_session (src/mgm_jobplan.h) on the host, against tests/golden/cli_table.json -- what the program
answered to ~2700 command lines BEFORE the planner existed (tools/record_cli_table.py): every line that ended or was refused
is planned to the same exit code, stdout and stderr, every line that ran is planned to run with the fields its options and
environment imply; a plan is a function of the request alone, whatever the process's environment holds; and the program itself
still answers a covering subset of the refused lines byte for byte.

`python tests/test_jobplan.py --rows` prints the table's requests one per block for tests/jobplan_sanitize.cc."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
with open(os.path.join(ROOT, "tests", "golden", "cli_table.json")) as _f:
    TABLE = json.load(_f)
SECTIONS = ("combos", "early", "values")
# every variable the planner knows (the list of tools/record_cli_table.py)
PLANNER_ENV = ["MGM_UNIQUENESS", "MGM_UNIQUENESS_RADIUS", "MGM_SPECKLE", "MGM_SPECKLE_DIFF", "MGM_FILL_HOLES", "MGM_FILL_HOLES_DIRS",
               "MGM_FILL_HOLES_DIST", "MGM_FILL_HOLES_OCC", "MGM_SUBPIX", "MGM_SUBPIX_INTERP", "TSGM", "USE_TRUNCATED_LINEAR_POTENTIALS",
               "TSGM_FIX_OVERCOUNT", "CENSUS_NCC_WIN", "TSGM_ITER", "TESTLRRL", "TESTLRRL_TAU", "MEDIAN", "MGM_RIGHT_FROM_LEFT", "MGM_BATCH_LR",
               "MGM_MS_SLACK", "MGM_MS_RADIUS", "MGM_DEVICE", "MGM_DEVICES", "MGM_PLACE_TRIES", "MGM_HIP_STATS", "MGM_HIP_KERNELS",
               "MGM_HIP_ORDERLY_EXIT", "WITH_MGM2"]
FILES = ["no_u.png", "no_v.png", "no_out.tif"]


def request(row):
    """(args, env) of a row: its atoms' arguments one after the other, the union of their environments."""
    args, env = [], {}
    for i in row[0]:
        args += TABLE["atoms"][i]["args"]
        env.update(TABLE["atoms"][i]["env"])
    return args, env


def rows():
    return [(s, k, r) for s in SECTIONS for k, r in enumerate(TABLE[s])]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("jobplan") / "libjobplan_harness.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-Wall", "-Werror", "-I", os.path.join(ROOT, "src"),
                    os.path.join(ROOT, "tests", "jobplan_harness.cc"), "-o", so], check=True)
    return C.CDLL(so)


def _call(fn, args, env, *more):
    tok = [b"mgm"] + [a.encode() for a in args]
    names, values = [k.encode() for k in env], [v.encode() for v in env.values()]
    buf = C.create_string_buffer(1 << 16)
    n = fn((C.c_char_p * len(tok))(*tok), len(tok), (C.c_char_p * len(names))(*names), (C.c_char_p * len(values))(*values), len(names),
           *more, buf, len(buf))
    assert 0 < n < len(buf)
    return buf.raw[:n]


def plan_bytes(lib, args, env):
    return _call(lib.jobplan_plan, args, env)


def plan(lib, args, env):
    return json.loads(plan_bytes(lib, args, env))


def refuse(lib, args, env, multi_up, u_ny, v_ny):
    return json.loads(_call(lib.jobplan_refuse, args, env, C.c_int(multi_up), C.c_int(u_ny), C.c_int(v_ny)))


@pytest.fixture(scope="module")
def plans(lib):
    """Every row's plan, made once."""
    return {(s, k): plan(lib, *request(r)) for s, k, r in rows()}


def test_the_table_is_what_the_issue_asks_for():
    assert len(TABLE["combos"]) == 32 * (1 + 13 + 66) and len(TABLE["early"]) >= 15 and len(TABLE["values"]) >= 70
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "cli_table.json")) < 100 << 10
    ran = [r for _, _, r in rows() if r[1] is None]
    assert 400 < len(ran) < 500 and all(r[3] is None for r in ran)


def test_lines_that_ended_or_were_refused(plans):
    n = {"end": 0, "refuse": 0}
    for s, k, r in rows():
        if r[1] is None:
            continue
        p, out, err = plans[s, k], TABLE["messages"][r[2]], TABLE["messages"][r[3]]
        what = (s, k, request(r))
        assert p["outcome"] in n and p["code"] == r[1] and p["err"] == err, (what, p)
        if p["outcome"] == "refuse":  # after the job's range line, which is the program's to print
            assert p["code"] == 2 and p["out"] == "" and out == "%d %d\n" % (p["dmin"], p["dmax"]), (what, p)
        else:
            assert p["out"] == out, (what, p)
        n[p["outcome"]] += 1
    assert n["end"] > 100 and n["refuse"] > 2000, n


def expected_of_combo(args, env):
    it = {None: 1, "2": 2, "0": 0, "1.5": 2}[env.get("TSGM_ITER")]
    both = env.get("TESTLRRL") != "0"
    devs = env.get("MGM_DEVICES")
    return dict(iterations=it, both=int(both), rfl=int(env.get("MGM_RIGHT_FROM_LEFT") == "1" and both), uq=int("-c" in args or "MGM_UNIQUENESS" in env),
                ranged=int("-m" in args), devices={None: [], "0,1": [0, 1], "0,": [0], "0": [0]}[devs], devices_comma=int(devs is not None and "," in devs),
                nscales=2 if "-S" in args else 1, refine=args[args.index("-s") + 1] if "-s" in args else "none", subpix=int(env.get("MGM_SUBPIX", 1)),
                conf_file="f" if "-c" in args else "",
                fill=env.get("MGM_FILL_HOLES", ""), fill_occ=env.get("MGM_FILL_HOLES_OCC", ""), min_file="a" if "-m" in args else "",
                max_file="b" if "-M" in args else "", f_u=FILES[0], f_v=FILES[1], f_out=FILES[2], f_cost="", f_back="", dmin=-30, dmax=30)


def test_lines_that_ran(plans):
    seen = set()
    for s, k, r in rows():
        if r[1] is not None:
            continue
        p = plans[s, k]
        args, env = request(r)
        assert p["outcome"] == "run" and p["code"] == 0 and p["out"] == "" and p["err"] == "", (s, k, args, env, p)
        assert TABLE["messages"][r[2]] == "%d %d\n" % (p["dmin"], p["dmax"])
        if s == "combos":
            want = expected_of_combo(args, env)
            assert {f: p[f] for f in want} == want, (k, args, env)
            assert float(p["uniq"]) == float(env.get("MGM_UNIQUENESS", 0))
            seen.add((p["iterations"], p["both"], p["rfl"], p["uq"], p["ranged"], tuple(p["devices"]), p["devices_comma"]))
    assert {x[0] for x in seen} == {0, 1, 2} and {x[1] for x in seen} == {0, 1} and {x[2] for x in seen} == {0, 1}
    assert {x[5] for x in seen} == {(), (0,), (0, 1)} and ((0,), 1) in {x[5:] for x in seen}


def test_right_from_left_is_off_without_the_left_right_test(plans):
    n = 0
    for k, r in enumerate(TABLE["combos"]):
        args, env = request(r)
        if env.get("MGM_RIGHT_FROM_LEFT") == "1" and env.get("TESTLRRL") == "0":
            assert plans["combos", k]["rfl"] == 0 and "MGM_RIGHT_FROM_LEFT=1 does not" not in plans["combos", k]["err"]
            n += 1
    assert n > 100


def test_pick_option_takes_the_next_token_whatever_it_is(lib):
    p = plan(lib, ["-r", "-R", "5"] + FILES, {})  # -r's value is "-R": atoi 0; no -R is left, and 5 is the left image
    assert (p["outcome"], p["dmin"], p["dmax"], p["f_u"], p["f_v"], p["f_out"], p["f_cost"]) == ("run", 0, 30, "5", FILES[0], FILES[1], FILES[2])
    p = plan(lib, ["-m", "-M", "a"] + FILES, {})
    assert (p["outcome"], p["min_file"], p["max_file"], p["ranged"], p["f_u"], p["f_cost"]) == ("run", "-M", "", 1, "a", FILES[2])
    p = plan(lib, ["-t", "-p", "-s", "cubic"] + FILES + ["no_cost.tif", "no_back.tif", "extra"], {})
    assert (p["outcome"], p["distance"], p["prefilter"], p["refine"], p["f_cost"], p["f_back"]) == ("run", "-p", "none", "cubic", "no_cost.tif", "no_back.tif")
    p = plan(lib, FILES, dict(TSGM="2", USE_TRUNCATED_LINEAR_POTENTIALS="1", TSGM_FIX_OVERCOUNT="0", CENSUS_NCC_WIN="5x", TESTLRRL_TAU="2.5", MEDIAN="2",
                              MGM_BATCH_LR="0", MGM_MS_SLACK="4", MGM_MS_RADIUS="1", MGM_DEVICE="3", MGM_PLACE_TRIES="2", MGM_HIP_STATS="1",
                              MGM_HIP_KERNELS="1", MGM_HIP_ORDERLY_EXIT="1", MGM_DEVICES="2,0,1x", MGM_SPECKLE="8", MGM_SPECKLE_DIFF="0.5",
                              MGM_FILL_HOLES_DIRS="4", MGM_FILL_HOLES_DIST="7", MGM_UNIQUENESS_RADIUS="2", MGM_SUBPIX_INTERP="linear"))
    got = {f: p[f] for f in ("TSGM", "FH", "FIX", "census_win", "tau", "median", "batch_lr", "ms_slack", "ms_radius", "device", "place_tries", "stats",
                             "kernels", "orderly_exit", "devices", "devices_comma", "speckle", "speckle_diff", "fill_dirs", "fill_dist", "uniq_radius",
                             "subpix_interp")}
    assert got == dict(TSGM=2, FH=1, FIX=0, census_win=5, tau="2.5", median="2", batch_lr=0, ms_slack=4, ms_radius=1, device=3, place_tries=2, stats=1,
                       kernels=1, orderly_exit=1, devices=[2, 0, 1], devices_comma=1, speckle=8, speckle_diff="0.5", fill_dirs=4, fill_dist=7,
                       uniq_radius=2, subpix_interp="linear")


# ---- refuse_on_session: the literal strings of the program before the planner (its three `&& multi` blocks and the height rule)
SESSION_MODES = [(dict(MGM_RIGHT_FROM_LEFT="1"), [], "mgm: MGM_RIGHT_FROM_LEFT=1 does not combine with several MGM_DEVICES\n"),
                 ({}, ["-c", "f"], "mgm: -c / MGM_UNIQUENESS does not combine with several MGM_DEVICES\n"),
                 (dict(MGM_UNIQUENESS="0.3"), [], "mgm: -c / MGM_UNIQUENESS does not combine with several MGM_DEVICES\n"),
                 (dict(MGM_SUBPIX="2"), [], "mgm: MGM_SUBPIX does not combine with several MGM_DEVICES\n"),
                 (dict(MGM_SUBPIX="4"), [], "mgm: MGM_SUBPIX does not combine with several MGM_DEVICES\n")]


def test_refuse_on_session(lib):
    for env, args, msg in SESSION_MODES:
        assert plan(lib, args + FILES, env)["outcome"] == "run"
        assert refuse(lib, args + FILES, env, 1, 48, 48) == dict(code=2, err=msg)
        assert refuse(lib, args + FILES, env, 0, 48, 48) == dict(code=0, err="")
    # a plain job, and the modes that combine with everything, run on several devices
    for env in ({}, dict(MGM_SPECKLE="8", MGM_FILL_HOLES="median", MGM_FILL_HOLES_OCC="sechigh", MEDIAN="1"), dict(MGM_RIGHT_FROM_LEFT="1", TESTLRRL="0")):
        assert refuse(lib, FILES, env, 1, 48, 40) == dict(code=0, err="")
    height = "mgm: MGM_RIGHT_FROM_LEFT=1 needs two images of one height\n"
    assert refuse(lib, FILES, dict(MGM_RIGHT_FROM_LEFT="1"), 0, 48, 40) == dict(code=2, err=height)
    assert refuse(lib, FILES, dict(MGM_RIGHT_FROM_LEFT="1"), 0, 40, 40) == dict(code=0, err="")
    assert refuse(lib, FILES, dict(MGM_SUBPIX="2"), 0, 48, 40) == dict(code=0, err="")
    # where two apply: the first mode, and the devices before the heights
    assert refuse(lib, ["-c", "f"] + FILES, dict(MGM_RIGHT_FROM_LEFT="1"), 1, 48, 40) == dict(code=2, err=SESSION_MODES[0][2])
    assert refuse(lib, ["-c", "f"] + FILES, dict(MGM_SUBPIX="2"), 1, 48, 48) == dict(code=2, err=SESSION_MODES[1][2])
    assert refuse(lib, ["-c", "f"] + FILES, dict(MGM_RIGHT_FROM_LEFT="1"), 0, 48, 40) == dict(code=2, err=height)


def test_first_mode_and_first_blocker_win(lib):
    every = ["-m", "a", "-M", "b", "-S", "2", "-s", "cubic", "-c", "f"] + FILES
    env = dict(MGM_RIGHT_FROM_LEFT="1", MGM_SUBPIX="2", TSGM_ITER="2", MGM_DEVICES="0,1")
    order = ["range images (-m/-M)", "-S > 1", "TSGM_ITER != 1", "a refinement other than none or vfit", "several MGM_DEVICES"]
    assert plan(lib, every, env)["err"] == "mgm: MGM_RIGHT_FROM_LEFT=1 does not combine with %s\n" % order[0]
    assert plan(lib, every[4:], env)["err"] == "mgm: MGM_RIGHT_FROM_LEFT=1 does not combine with %s\n" % order[1]
    assert plan(lib, every[6:], env)["err"] == "mgm: MGM_RIGHT_FROM_LEFT=1 does not combine with %s\n" % order[2]
    del env["TSGM_ITER"]
    assert plan(lib, every[6:], env)["err"] == "mgm: MGM_RIGHT_FROM_LEFT=1 does not combine with %s\n" % order[3]
    assert plan(lib, every[8:], env)["err"] == "mgm: MGM_RIGHT_FROM_LEFT=1 does not combine with %s\n" % order[4]
    del env["MGM_RIGHT_FROM_LEFT"]
    assert plan(lib, every[6:], env)["err"] == "mgm: -c / MGM_UNIQUENESS does not combine with %s\n" % order[4]  # (a refinement does not block it)
    assert plan(lib, every[10:], env)["err"] == "mgm: MGM_SUBPIX does not combine with %s\n" % order[4]
    assert plan(lib, FILES, dict(MGM_SUBPIX="2", MGM_RIGHT_FROM_LEFT="1", MGM_DEVICES="0,"))["err"] == "mgm: MGM_RIGHT_FROM_LEFT=1 does not combine with several MGM_DEVICES\n"
    assert plan(lib, FILES, dict(MGM_SUBPIX="2", MGM_RIGHT_FROM_LEFT="1"))["err"] == "mgm: MGM_SUBPIX does not combine with MGM_RIGHT_FROM_LEFT=1\n"
    p = plan(lib, FILES, dict(MGM_SUBPIX="2", MGM_RIGHT_FROM_LEFT="1", TESTLRRL="0", MGM_FILL_HOLES="min", MGM_FILL_HOLES_OCC="max"))
    assert (p["outcome"], p["code"]) == ("refuse", 2) and p["err"].startswith("mgm: MGM_FILL_HOLES_OCC needs the right view")


# ---- purity
def test_a_plan_does_not_read_the_process_environment(lib, monkeypatch):
    picks = [r for _, _, r in rows()][::97]
    before = [plan_bytes(lib, *request(r)) for r in picks]
    for name in PLANNER_ENV:  # conflicting with every value the table uses, and bad where a value can be
        monkeypatch.setenv(name, "7,8" if name == "MGM_DEVICES" else "0" if name == "TESTLRRL" else "x")
    assert [plan_bytes(lib, *request(r)) for r in picks] == before


def test_a_plan_does_not_depend_on_the_plans_before_it(lib):
    a, b = request(TABLE["combos"][5]), (["-S", "3", "-c", "g", "-r", "1", "-R", "9"] + FILES, dict(MGM_DEVICES="4,5,6", TSGM_ITER="3", MGM_SUBPIX="4"))
    pa, pb = plan_bytes(lib, *a), plan_bytes(lib, *b)
    assert pa != pb
    assert (plan_bytes(lib, *a), plan_bytes(lib, *b)) == (pa, pb)
    assert (plan_bytes(lib, *b), plan_bytes(lib, *a), plan_bytes(lib, *a)) == (pb, pa, pa)


# ---- the program itself, on lines that end before any device is touched
def cover():
    """The first row of the table for every distinct stderr text and every distinct stdout text of a line that ended or was refused."""
    first = {}
    for s, k, r in rows():
        if r[1] is not None:
            for key in (("err", r[3]), ("out", r[2])):
                first.setdefault(key, (s, k))
    return sorted(set(first.values()))


def test_the_cover_is_small_and_complete():
    c = cover()
    assert len(c) <= 64
    texts = lambda rs: ({r[2] for r in rs}, {r[3] for r in rs})  # (as indices into the list of messages)
    assert texts([TABLE[s][k] for s, k in c]) == texts([r for _, _, r in rows() if r[1] is not None])
    firsts = {tuple(request(TABLE[s][k])[0][:1]) for s, k in c}
    assert {("-h",), ("-?",), ("--version",), ("--help",)} <= firsts


def test_the_program_answers_the_cover_as_recorded():
    base = {k: v for k, v in os.environ.items() if k not in PLANNER_ENV}
    for s, k in cover():
        r = TABLE[s][k]
        args, env = request(r)
        got = subprocess.run(["mgm"] + args, executable=MGM, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
        assert (got.returncode, got.stdout, got.stderr) == (r[1], TABLE["messages"][r[2]], TABLE["messages"][r[3]]), (s, k, args, env)


if __name__ == "__main__" and "--rows" in sys.argv:
    for _, _, r in rows():  # T token ... / E name=value ... / a line with a dot
        a, e = request(r)
        print("".join("T %s\n" % t for t in ["mgm"] + a) + "".join("E %s=%s\n" % kv for kv in e.items()) + ".")
