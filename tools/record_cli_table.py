#!/usr/bin/env python3
"""Record what the `mgm` program answers to command lines that never reach a device: tests/golden/cli_table.json.

Run ONCE against the binary whose behaviour is to be kept (mgm_amd/bin/mgm, or the one given as the first argument), before
src/mgm_jobplan.h or the program changes; tests/test_jobplan.py then holds plan_job() and the program to the table.  None
of the file names exists, so a line that is refused ends with its message and a line that would run ends with
`mgm: cannot open no_u.png` (exit code 1) within milliseconds, with or without a GPU in the machine.  The program is started
under the name `mgm`, whatever its path: one message quotes argv[0].

The table is made of ATOMS -- a piece of command line and/or environment, stored once -- and rows [atoms, code, out, err]:
the row's arguments are its atoms' arguments one after the other, its environment their union, `out` and `err` index the
list of messages.  A row that got as far as opening its inputs is stored as "runs": code and err are null."""
import itertools
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["no_u.png", "no_v.png", "no_out.tif"]
# every variable plan_job() reads: the recording and the tests start from an environment without them
PLANNER_ENV = ["MGM_UNIQUENESS", "MGM_UNIQUENESS_RADIUS", "MGM_SPECKLE", "MGM_SPECKLE_DIFF", "MGM_FILL_HOLES", "MGM_FILL_HOLES_DIRS",
               "MGM_FILL_HOLES_DIST", "MGM_FILL_HOLES_OCC", "MGM_SUBPIX", "MGM_SUBPIX_INTERP", "TSGM", "USE_TRUNCATED_LINEAR_POTENTIALS",
               "TSGM_FIX_OVERCOUNT", "CENSUS_NCC_WIN", "TSGM_ITER", "TESTLRRL", "TESTLRRL_TAU", "MEDIAN", "MGM_RIGHT_FROM_LEFT", "MGM_BATCH_LR",
               "MGM_MS_SLACK", "MGM_MS_RADIUS", "MGM_DEVICE", "MGM_DEVICES", "MGM_PLACE_TRIES", "MGM_HIP_STATS", "MGM_HIP_KERNELS",
               "MGM_HIP_ORDERLY_EXIT", "WITH_MGM2"]

MODES = [dict(env={"MGM_RIGHT_FROM_LEFT": "1"}), dict(args=["-c", "f"]), dict(env={"MGM_UNIQUENESS": "0.3"}), dict(env={"MGM_SUBPIX": "2"}),
         dict(env={"MGM_FILL_HOLES": "median", "MGM_FILL_HOLES_OCC": "sechigh"})]
# (blockers of one group set the same thing: they are not paired with each other)
BLOCKERS = [[dict(args=["-m", "a", "-M", "b"])], [dict(args=["-S", "2"])], [dict(env={"TSGM_ITER": v}) for v in ("2", "0", "1.5")],
            [dict(env={"MGM_DEVICES": v}) for v in ("0,1", "0,", "0")], [dict(env={"TESTLRRL": "0"})],
            [dict(args=["-s", v]) for v in ("parabola", "cubic", "parabolaOCV", "vfit")]]
BAD_VALUES = ["", "none", "3x", "-1", "0.5", "nan", "99999999999"]
VALUE_VARS = ["MGM_UNIQUENESS", "MGM_UNIQUENESS_RADIUS", "MGM_SPECKLE", "MGM_SPECKLE_DIFF", "MGM_FILL_HOLES", "MGM_FILL_HOLES_DIRS",
              "MGM_FILL_HOLES_DIST", "MGM_FILL_HOLES_OCC", "MGM_SUBPIX", "MGM_SUBPIX_INTERP"]
# which check comes first: every variable bad at once, then without the first, without the first two, ... (the order parse checks them in),
# a bad value beside a refused combination, and -S out of range beside each
FIRST_OF = VALUE_VARS[:4] + ["MGM_FILL_HOLES", "MGM_FILL_HOLES_DIRS", "MGM_FILL_HOLES_DIST", "MGM_FILL_HOLES_OCC", "MGM_SUBPIX", "MGM_SUBPIX_INTERP"]


class Table:
    def __init__(self):
        self.atoms, self.index = [], {}

    def atom(self, args=(), env=None):
        a = dict(args=list(args), env=dict(env or {}))
        key = json.dumps(a, sort_keys=True)
        if key not in self.index:
            self.index[key] = len(self.atoms)
            self.atoms.append(a)
        return self.index[key]

    def line(self, ids):
        args, env = [], {}
        for i in ids:
            args += self.atoms[i]["args"]
            env.update(self.atoms[i]["env"])
        return args, env


def main():
    exe = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "mgm_amd", "bin", "mgm")
    T = Table()
    files = T.atom(FILES)
    modes = [T.atom(**m) for m in MODES]
    blockers = [[T.atom(**b) for b in group] for group in BLOCKERS]
    sections = {"combos": [], "early": [], "values": []}

    crosses = [[]] + [[b] for g in blockers for b in g]
    crosses += [[a, b] for g, h in itertools.combinations(blockers, 2) for a in g for b in h]
    for k in range(len(modes) + 1):
        for subset in itertools.combinations(modes, k):
            for cross in crosses:
                sections["combos"].append(list(subset) + cross + [files])

    for first in ("-h", "-?", "--version", "--help"):
        sections["early"].append([T.atom([first])])
        sections["early"].append([T.atom([first]), files])
    sections["early"] += [[], [T.atom(FILES[:1])], [T.atom(FILES[:2])], [T.atom(["-r"]), files], [T.atom(["-S", "2"]), T.atom(FILES[:2])],
                          [T.atom(["-r", "1", "-R", "2"]), T.atom(FILES[:2])], [T.atom(["-c"]), files],
                          # pick_option's surgery: an option's value may be the next option's name
                          [T.atom(["-r", "-R", "5"]), files], [T.atom(["-m", "-M", "a"]), files], [T.atom(["-S", "-c", "f"]), files],
                          [T.atom(["-t", "-p", "-s", "cubic"]), files, T.atom(["no_cost.tif", "no_back.tif", "extra"])]]

    for var in VALUE_VARS:
        for val in BAD_VALUES:
            sections["values"].append([T.atom(env={var: val}), files])
    fill = T.atom(env={"MGM_FILL_HOLES": "max"})
    for val in BAD_VALUES + ["seclow"]:  # (the occlusions' rule beside a mismatches' rule)
        sections["values"].append([fill, T.atom(env={"MGM_FILL_HOLES_OCC": val}), files])
    for val in ("0", "9", "-1", "8", "x", "1.5"):
        sections["values"].append([T.atom(["-S", val]), files])
    bad = {v: T.atom(env={v: "x"}) for v in FIRST_OF}
    for k in range(len(FIRST_OF)):
        sections["values"].append([bad[v] for v in FIRST_OF[k:]] + [files])
        sections["values"].append([bad[v] for v in FIRST_OF[k:]] + [T.atom(["-S", "9"]), files])
    refused = [modes[0], blockers[1][0]]  # MGM_RIGHT_FROM_LEFT=1 with -S 2
    for v in FIRST_OF:
        sections["values"].append(refused + [bad[v], files])
    sections["values"].append([T.atom(["-S", "9"]), modes[3], blockers[0][0], files])

    base = {k: v for k, v in os.environ.items() if k not in PLANNER_ENV}

    def run(ids):
        args, env = T.line(ids)
        r = subprocess.run(["mgm"] + args, executable=exe, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
        return r.returncode, r.stdout, r.stderr

    messages, midx = [], {}

    def msg(s):
        if s not in midx:
            midx[s] = len(messages)
            messages.append(s)
        return midx[s]

    out = {}
    with ThreadPoolExecutor(8) as pool:
        for name, rows in sections.items():
            out[name] = []
            for ids, (code, so, se) in zip(rows, pool.map(run, rows)):
                last = se.splitlines()[-1] if se.splitlines() else ""
                if code == 1 and last.startswith("mgm: cannot open "):
                    out[name].append([ids, None, msg(so), None])
                else:
                    out[name].append([ids, code, msg(so), msg(se)])
    table = dict(atoms=T.atoms, messages=messages, **out)
    path = os.path.join(ROOT, "tests", "golden", "cli_table.json")
    with open(path, "w") as f:
        json.dump(table, f, separators=(",", ":"))
        f.write("\n")
    print("%s: %d rows (%s), %d atoms, %d messages, %d bytes" % (path, sum(len(v) for v in out.values()),
          ", ".join("%s %d" % (k, len(v)) for k, v in out.items()), len(T.atoms), len(messages), os.path.getsize(path)))


if __name__ == "__main__":
    main()
