"""MGM_ENERGY / MGM_ENERGY_MAP at the command line's planning stage (src/mgm_jobplan.h), on the program itself: these lines end or
are refused before any device is touched -- bad values with exit code 1 and nothing on stdout, modes that do not combine with exit
code 2 behind the job's range line, through the one exclusion table -- and without the three variables a refused or ended line is
what it was (tests/test_jobplan.py holds the recorded table)."""
import os
import subprocess

import energy_runs as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MGM = os.path.join(ROOT, "mgm_amd", "bin", "mgm")
FILES = ["no_u.png", "no_v.png", "no_out.tif"]


def run(args, env):
    base = {k: v for k, v in os.environ.items() if not k.startswith(("MGM_", "TSGM"))}
    return subprocess.run(["mgm"] + args.split() + FILES, executable=MGM, env=dict(base, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                          timeout=60)


def test_refusals_through_the_exclusion_table():
    for args, env, blocker in er.ENERGY_REFUSALS:
        for conn in ("4", "8"):
            r = run(args, dict(env, MGM_ENERGY=conn))
            assert (r.returncode, r.stdout, r.stderr) == (2, "-30 30\n", "mgm: MGM_ENERGY does not combine with %s\n" % blocker), (args, env, r)
    # an earlier row of the table still wins, and TSGM_DEBUG changes nothing about a refusal
    r = run("-S 2 -c f", dict(MGM_ENERGY="4", TSGM_DEBUG="1"))
    assert (r.returncode, r.stdout, r.stderr) == (2, "-30 30\n", "mgm: -c / MGM_UNIQUENESS does not combine with -S > 1\n")
    r = run("-S 2", dict(MGM_ENERGY="8", MGM_SUBPIX="4", MGM_DEVICES="0,1"))
    assert (r.returncode, r.stdout, r.stderr) == (2, "-30 30\n", "mgm: MGM_SUBPIX does not combine with -S > 1\n")


def test_bad_values_end_at_parse_time():
    for env, msg in er.ENERGY_BAD_VALUES:
        r = run("", env)
        assert (r.returncode, r.stdout, r.stderr) == (1, "", msg), (env, r)
    # --help is pinned and does not name the new variables
    r = run("", {})
    h = subprocess.run(["mgm", "--help"], executable=MGM, stdout=subprocess.PIPE, text=True).stdout
    assert "MGM_ENERGY" not in h and "TSGM_DEBUG" not in h
