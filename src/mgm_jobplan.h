// mgm_jobplan.h -- what one `mgm` command line is going to do, decided in ONE place before anything is done.
//
// plan_job(tokens, env) is a pure function: the command line's tokens and a lookup of environment parameters in, a JobPlan
// out.  Standard library only -- no device, no image I/O, no getenv (the program passes getenv in, tests/jobplan_harness.cc
// a dictionary), nothing printed.  A plan is one of three things: RUN; END before anything happens (--help, a bad value:
// code, stdout text, stderr text); REFUSE (modes that do not combine: code 2 and a line on stderr, printed after the job's
// `dmin dmax` line as the program always has).  refuse_on_session() is the part of the same rules that can only be known once
// the device side is up (resident mode: an earlier line brought several devices up) and the images are decoded.
//
// The next mode that does not combine with something gets a row in EXCLUSIONS below, and a sentence in HELP_TEXT.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace mgm_cli {

struct Opts {
    int dmin, dmax, NDIR;
    float P1, P2, aP2, aThresh, truncDist;
    std::string distance, prefilter, refine;
    int TSGM, FH, FIX, census_win;
    int subpix = 1;                      // MGM_SUBPIX: labels per pixel of disparity, 1 (off), 2 or 4
    std::string subpix_interp = "cubic"; // MGM_SUBPIX_INTERP: linear or cubic
};

struct JobPlan {
    enum Outcome { RUN, END, REFUSE };
    Outcome outcome = RUN;
    int code = 0;          // END, REFUSE: the exit code of the command line
    std::string out_text;  // END: what goes to stdout ...
    std::string err_text;  // END, REFUSE: ... and to stderr
    // ---- the command line
    Opts o{};
    std::string min_file, max_file, nolr_file, f_u, f_v, f_out, f_cost, f_back;
    int nscales = 1;          // -S: levels of the coarse-to-fine driver (1: the single-scale path)
    std::string conf_file;    // -c: the left->right run's confidence map
    double uniq = 0;          // MGM_UNIQUENESS: the uniqueness filter's ratio (0: off)
    int uniq_radius = 1;      // MGM_UNIQUENESS_RADIUS: labels around the winner the runner-up stays away from
    int speckle = 0;          // MGM_SPECKLE: components of the final left map of at most this many pixels go (0: off)
    float speckle_diff = 1;   // MGM_SPECKLE_DIFF: neighbours are joined up to this difference
    std::string fill;         // MGM_FILL_HOLES: median, min or max -- the final left map's holes are filled (empty: off)
    int fill_dirs = 8;        // MGM_FILL_HOLES_DIRS: 2, 4 or 8 rays
    int fill_dist = 0;        // MGM_FILL_HOLES_DIST: a candidate is at most this many steps away (0: no limit)
    std::string fill_occ;     // MGM_FILL_HOLES_OCC: the occlusions' rule -- the holes are classified, `fill` is the mismatches' (empty: off)
    std::string votes_file;   // -C: the left->right run's consensus votes (empty: off)
    int consensus = 0;        // MGM_CONSENSUS: each run's map is NaN where fewer than this many passes vote for it (0: off)
    float consensus_tol = 1;  // MGM_CONSENSUS_TOL: a pass votes when its own winner is at most this many labels from the map
    int energy = 0;           // MGM_ENERGY: 4 or 8 neighbours -- the model energy of every run and iteration on stderr (0: off)
    std::string energy_map;   // MGM_ENERGY_MAP: the left->right run's last map of it (empty: off)
    // ---- derived from the environment
    // main()'s loops are `for (int i = 0; i < TSGM_ITER(); i++)` on a DOUBLE (mgm.cc:377, 406): ceil() iterations; none at
    // all for TSGM_ITER <= 0 -- the maps then stay the zero images they were allocated as (mgm.cc:360-365)
    int iterations = 1;
    bool both = true;         // TESTLRRL != 0: the right->left run and the left-right test
    float tau = 1;            // TESTLRRL_TAU
    double median = 0;        // MEDIAN: != 0: the median filter runs, with radius (int)median
    bool ranged = false;      // -m/-M: range images
    // MGM_RIGHT_FROM_LEFT=1 (this program's own mode), with TESTLRRL != 0 only: the right map of the left-right
    // test comes out of the left run's aggregated volume (mgm_wta_right_dev) instead of a second run
    bool rfl = false;
    // TSGM_DEBUG != 0 (the reference's, mgm.cc:27): its debug lines on stdout, the three energies of every iteration among them
    // (DESIGN.md 7i).  Off in the modes the reference does not have -- -S > 1, MGM_SUBPIX, MGM_RIGHT_FROM_LEFT=1 -- and on several
    // devices (looked at once they are up): there is no reference stdout to equal there, and the variable stays ignored as it always was
    bool debug = false;
    bool uq = false;          // -c FILE / MGM_UNIQUENESS=r: the runner-up search of a run right behind its aggregation
    bool batch_lr = true;     // MGM_BATCH_LR: both runs of a pair through one launch of the pass kernel
    int ms_slack = 3, ms_radius = 2;  // MGM_MS_SLACK, MGM_MS_RADIUS (-S: the window around the coarser level's disparities)
    int device = 0;           // MGM_DEVICE
    std::vector<int> devices; // MGM_DEVICES=a,b,...: several GPUs of this node
    bool devices_comma = false;  // ... and whether that string holds a comma: "several MGM_DEVICES" before any device is up
    int place_tries = 0;      // MGM_PLACE_TRIES
    bool stats = false, kernels = false, orderly_exit = false;  // MGM_HIP_STATS, MGM_HIP_KERNELS, MGM_HIP_ORDERLY_EXIT
    // (WITH_MGM2 is accepted and changes nothing: see the header comment of mgm_main.cc)
};

using EnvLookup = std::function<const char *(const char *)>;

// ---- which modes exclude which: THE table ---------------------------------------------------------------------------------
enum Blocker { B_RANGED, B_SCALES, B_ITER, B_REFINE, B_RFL, B_DEVICES, B_SUBPIX, N_BLOCKERS };  // (in the order they are looked at)
static const char *const BLOCKER_NAME[N_BLOCKERS] = {
    "range images (-m/-M)", "-S > 1", "TSGM_ITER != 1", "a refinement other than none or vfit", "MGM_RIGHT_FROM_LEFT=1", "several MGM_DEVICES",
    "MGM_SUBPIX"};
enum Mode { M_RFL, M_UQ, M_SUBPIX, M_CONSENSUS, M_ENERGY, N_MODES };  // (as well)
static const struct {
    const char *name;
    bool blocked_by[N_BLOCKERS];
} EXCLUSIONS[N_MODES] = {
    //                        -m/-M  -S>1   ITER   refine rfl    devices subpix
    {"MGM_RIGHT_FROM_LEFT=1", {true, true, true, true, false, true, false}},
    {"-c / MGM_UNIQUENESS", {true, true, true, false, false, true, false}},
    {"MGM_SUBPIX", {true, true, true, false, true, true, false}},
    {"-C / MGM_CONSENSUS", {false, false, false, false, false, true, false}},
    {"MGM_ENERGY", {false, true, false, false, true, true, true}},
};

// "mgm: <mode> does not combine with <blocker>\n" for the first mode that is on and its first blocker that holds; else empty
inline std::string first_exclusion(const bool (&mode)[N_MODES], const bool (&blocker)[N_BLOCKERS])
{
    for (int m = 0; m < N_MODES; m++)
        for (int b = 0; mode[m] && b < N_BLOCKERS; b++)
            if (blocker[b] && EXCLUSIONS[m].blocked_by[b]) return std::string("mgm: ") + EXCLUSIONS[m].name + " does not combine with " + BLOCKER_NAME[b] + "\n";
    return "";
}

static const char *const HELP_TEXT =
    "mgm [options] in_u in_v out_disp [out_cost [out_backflow]]   (in: png tif pgm ppm pfm npy; out: tif pfm npy)\n"
    "options: -r dmin(-30) -R dmax(30) -O NDIR(4) -P1 (8) -P2 (32) -p prefilter(none) -t distance(ad)\n"
    "         -truncDist (inf) -s subpix(none) -aP1 (1) -aP2 (1) -aThresh (5) -m FILE -M FILE -l FILE\n"
    "         -S nscales(1): coarse to fine over up to 8 half-size levels (this program's own mode, not the reference's)\n"
    "         -c FILE: the left->right run's confidence map, 1 - cost1/cost2 of the winner and the runner-up (own mode)\n"
    "environment: CENSUS_NCC_WIN=3 TESTLRRL=1 TESTLRRL_TAU=1.0 MEDIAN=0 TSGM=4 TSGM_ITER=1\n"
    "             TSGM_FIX_OVERCOUNT=1 USE_TRUNCATED_LINEAR_POTENTIALS=0 MGM_DEVICE=0 MGM_DEVICES=0,1,...\n"
    "             MGM_MS_SLACK=3 MGM_MS_RADIUS=2 (-S: window around the coarser level's disparities)\n"
    "             MGM_RIGHT_FROM_LEFT=0 (1, with TESTLRRL != 0: no right->left run; the right map is read out of the left run's\n"
    "              aggregated volume along its diagonals, and stdout has the line `right from left` in place of that run's\n"
    "              lines; not with -m/-M, -S > 1, TSGM_ITER != 1, several MGM_DEVICES, -s parabola|cubic|parabolaOCV: exit code 2)\n"
    "             MGM_UNIQUENESS=0 (r in (0,1]: each run's map is NaN where 1 - cost1/cost2 < r, cost2 the aggregated cost of the\n"
    "              best label more than MGM_UNIQUENESS_RADIUS=1 away from the winner; applied right after the run's refinement,\n"
    "              before MEDIAN, the left-right test and the -l map; with MGM_RIGHT_FROM_LEFT=1 only the left map is filtered:\n"
    "              the right view has no runner-up; -c and MGM_UNIQUENESS not with -m/-M, -S > 1, TSGM_ITER != 1, several\n"
    "              MGM_DEVICES: exit code 2)\n"
    "             MGM_SPECKLE=0 (n > 0: the speckle filter -- every 4-connected component of finite pixels of the final left map,\n"
    "              neighbours joined where they differ by at most MGM_SPECKLE_DIFF=1, that has at most n pixels becomes NaN; runs\n"
    "              last but for MGM_FILL_HOLES, after MEDIAN and the left-right test and before the back-projected image, with -S\n"
    "              on the full-size map only; leaves the -l map, the cost map and stdout as they are; combines with every other mode)\n"
    "             MGM_FILL_HOLES=none (median, min or max: hole filling -- every non-finite pixel of the final left map takes the\n"
    "              median (the upper one) / minimum / maximum of the nearest finite pixels along the first MGM_FILL_HOLES_DIRS=8\n"
    "              (2, 4 or 8) of the rays (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,+1) (+1,-1) (-1,-1), each at most\n"
    "              MGM_FILL_HOLES_DIST=0 steps away (0: no limit); rays read the unfilled map; a hole that no ray serves stays;\n"
    "              runs last, after MGM_SPECKLE, and before the back-projected image, with -S on the full-size map only; leaves\n"
    "              the -l map, the cost map, -c's map and stdout as they are; combines with every other mode)\n"
    "             MGM_FILL_HOLES_OCC=none (seclow, sechigh, min, max or median, with MGM_FILL_HOLES: the holes are classified first --\n"
    "              a hole (x,y) is a mismatch when a pixel xr of the right map as it entered the left-right test, x+dmin <= xr <=\n"
    "              x+dmax of -r/-R, lands within TESTLRRL_TAU of it, |xr + right(xr,y) - x| <= tau, else an occlusion; occlusions take\n"
    "              this rule, mismatches MGM_FILL_HOLES's; seclow / sechigh: the second lowest / second highest candidate -- the\n"
    "              background's is sechigh for a range like -r -64 -R 0, seclow for positive disparities; needs the right view:\n"
    "              TESTLRRL=0 leaves none, whatever MGM_RIGHT_FROM_LEFT is: exit code 2; the class map has no file option)\n"
    "             MGM_SUBPIX=1 (2 or 4: labels every half / quarter pixel -- both runs match against the other image shifted by\n"
    "              k/s pixels, MGM_SUBPIX_INTERP=cubic (Keys; or linear), and aggregate s*(dmax-dmin)+1 labels; each run's map is\n"
    "              divided by s right after its refinement, before MGM_UNIQUENESS, MEDIAN, the left-right test and the -l map, so\n"
    "              TESTLRRL_TAU, MGM_SPECKLE_DIFF, -r/-R and every output stay in pixels; -P1/-P2, -s and MGM_UNIQUENESS_RADIUS act\n"
    "              per FINE label: a slope of one pixel takes s steps of P1; not with -m/-M, -S > 1, TSGM_ITER != 1,\n"
    "              MGM_RIGHT_FROM_LEFT=1, several MGM_DEVICES, nor any other value: exit code 2)\n"
    "             (with several MGM_DEVICES, -S / -m -M / TSGM_ITER > 1 run on the first device; in --batch mode a FIRST line\n"
    "              of that kind brings up one device for the whole batch, a later one leaves the other lines their devices)\n"
    "resident mode: mgm --batch FILE|-   (one such command line per line of FILE, one device context for all)";

// ---- the two readers of environment values --------------------------------------------------------------------------------
// the reference's "smart parameters" (smartparameter.h:26-50): a double, and the default for whatever sscanf does not take
inline double env_param(const EnvLookup &env, const char *name, double dflt)
{
    const char *s = env(name);
    double y;
    if (s && sscanf(s, "%lf", &y) == 1) return y;
    return dflt;
}
// this program's own parameters: a value that is no number is refused (false), not replaced by the default
inline bool env_strict(const EnvLookup &env, const char *name, double dflt, double *y)
{
    const char *s = env(name);
    char *end = nullptr;
    *y = s ? strtod(s, &end) : dflt;
    return !s || (end != s && !*end);
}
inline bool env_flag(const EnvLookup &env, const char *name)  // MGM_HIP_*: on for an integer other than 0
{
    const char *s = env(name);
    return s && atoi(s) != 0;
}

// pick_option (mgm.cc:165-179): single-dash name, value = next argv, both removed
inline const char *pick_option(int *argc, const char **argv, const char *opt, const char *dflt)
{
    for (int i = 0; i < *argc - 1; i++)
        if (argv[i][0] == '-' && 0 == strcmp(argv[i] + 1, opt)) {
            const char *r = argv[i + 1];
            *argc -= 2;
            for (int j = i; j < *argc; j++) argv[j] = argv[j + 2];
            return r;
        }
    return dflt;
}

// `tokens`: the command line, argv[0] included
inline JobPlan plan_job(const std::vector<std::string> &tokens, const EnvLookup &env)
{
    JobPlan p;
    std::vector<const char *> av;
    for (auto &t : tokens) av.push_back(t.c_str());
    av.push_back(nullptr);
    int argc = (int)tokens.size();
    const char **argv = av.data();
    auto end = [&](int code, const char *out, const std::string &err = "") {
        p.outcome = JobPlan::END;
        p.code = code;
        if (out) p.out_text = std::string(out) + "\n";
        p.err_text = err;
        return p;
    };
    if (argc < 2 || !strcmp(argv[1], "-h")) return end(0, "usage:\n\tmgm [-options] u v out [cost [backflow]]");
    if (!strcmp(argv[1], "-?")) return end(0, "Compute stereo disparities by the MGM algorithm.");
    if (!strcmp(argv[1], "--version")) return end(0, "mgm 2.0 (mgm-hip, MI355X)");
    if (!strcmp(argv[1], "--help")) return end(0, HELP_TEXT);
    if (argc < 4)
        return end(1, nullptr, std::string("too few parameters\n   usage: ") + argv[0] +
                                   "  [-r dmin -R dmax] [-m dminImg -M dmaxImg] [-O NDIR: 2, (4), 8] u v out [cost [backflow]]\n");
    // mgm.cc:303-318, in the same order (the order matters for pick_option's argv surgery)
    p.min_file = pick_option(&argc, argv, "m", "");
    p.max_file = pick_option(&argc, argv, "M", "");
    Opts &o = p.o;
    o.dmin = atoi(pick_option(&argc, argv, "r", "-30"));
    o.dmax = atoi(pick_option(&argc, argv, "R", "30"));
    o.NDIR = atoi(pick_option(&argc, argv, "O", "4"));
    o.P1 = (float)atof(pick_option(&argc, argv, "P1", "8"));
    o.P2 = (float)atof(pick_option(&argc, argv, "P2", "32"));
    pick_option(&argc, argv, "aP1", "1");  // accepted and unused, as in the reference
    o.aP2 = (float)atof(pick_option(&argc, argv, "aP2", "1"));
    o.aThresh = (float)atof(pick_option(&argc, argv, "aThresh", "5"));
    o.distance = pick_option(&argc, argv, "t", "ad");
    o.prefilter = pick_option(&argc, argv, "p", "none");
    o.refine = pick_option(&argc, argv, "s", "none");
    o.truncDist = (float)atof(pick_option(&argc, argv, "truncDist", "inf"));
    p.nolr_file = pick_option(&argc, argv, "l", "");
    p.nscales = atoi(pick_option(&argc, argv, "S", "1"));
    p.conf_file = pick_option(&argc, argv, "c", "");
    p.uniq = env_param(env, "MGM_UNIQUENESS", 0);
    p.uniq_radius = (int)env_param(env, "MGM_UNIQUENESS_RADIUS", 1);
    if (!(p.uniq >= 0 && p.uniq <= 1)) return end(1, nullptr, "mgm: MGM_UNIQUENESS must be a ratio in [0, 1]\n");
    if (p.uniq_radius < 0) return end(1, nullptr, "mgm: MGM_UNIQUENESS_RADIUS must be >= 0\n");
    const auto whole = [](double x) { return x >= 0 && x <= 2147483647.0 && x == std::floor(x); };
    double n, df, nd, dist, cs, ct;
    p.votes_file = pick_option(&argc, argv, "C", "");
    if (!env_strict(env, "MGM_CONSENSUS", 0, &cs) || !whole(cs)) return end(1, nullptr, "mgm: MGM_CONSENSUS must be an integer >= 0 (passes; 0: off)\n");
    if (!env_strict(env, "MGM_CONSENSUS_TOL", 1, &ct) || !(ct >= 0) || !std::isfinite(ct) || !std::isfinite((float)ct))
        return end(1, nullptr, "mgm: MGM_CONSENSUS_TOL must be a finite number >= 0 (labels)\n");
    p.consensus = (int)cs;
    p.consensus_tol = (float)ct;
    double en;
    if (!env_strict(env, "MGM_ENERGY", 0, &en) || !(en == 0 || en == 4 || en == 8)) return end(1, nullptr, "mgm: MGM_ENERGY must be 4 or 8 (neighbours; 0: off)\n");
    p.energy = (int)en;
    if (const char *em = env("MGM_ENERGY_MAP")) p.energy_map = em;
    if (!p.energy_map.empty() && p.energy == 0) return end(1, nullptr, "mgm: MGM_ENERGY_MAP needs MGM_ENERGY=4 or 8\n");
    if (!env_strict(env, "MGM_SPECKLE", 0, &n) || !whole(n)) return end(1, nullptr, "mgm: MGM_SPECKLE must be an integer >= 0 (pixels)\n");
    if (!env_strict(env, "MGM_SPECKLE_DIFF", 1, &df) || !(df >= 0)) return end(1, nullptr, "mgm: MGM_SPECKLE_DIFF must be a number >= 0\n");
    p.speckle = (int)n;
    p.speckle_diff = (float)df;
    const auto word = [&](const char *name, const char *dflt) {
        const char *s = env(name);
        return std::string(s ? s : dflt);
    };
    const auto one_of = [](const std::string &s, std::initializer_list<const char *> words) {
        for (const char *w : words)
            if (s == w) return true;
        return false;
    };
    const std::string m = word("MGM_FILL_HOLES", "");
    if (!one_of(m, {"", "none", "median", "min", "max"})) return end(1, nullptr, "mgm: MGM_FILL_HOLES must be median, min, max or none\n");
    if (!env_strict(env, "MGM_FILL_HOLES_DIRS", 8, &nd) || !(nd == 2 || nd == 4 || nd == 8)) return end(1, nullptr, "mgm: MGM_FILL_HOLES_DIRS must be 2, 4 or 8\n");
    if (!env_strict(env, "MGM_FILL_HOLES_DIST", 0, &dist) || !whole(dist))
        return end(1, nullptr, "mgm: MGM_FILL_HOLES_DIST must be an integer >= 0 (steps; 0: no limit)\n");
    p.fill = m == "none" ? "" : m;
    const std::string oc = word("MGM_FILL_HOLES_OCC", "");
    if (!one_of(oc, {"", "none", "seclow", "sechigh", "min", "max", "median"}))
        return end(1, nullptr, "mgm: MGM_FILL_HOLES_OCC must be seclow, sechigh, min, max, median or none\n");
    p.fill_occ = oc == "none" ? "" : oc;
    if (!p.fill_occ.empty() && p.fill.empty())
        return end(1, nullptr, "mgm: MGM_FILL_HOLES_OCC needs MGM_FILL_HOLES=median, min or max (the mismatches' rule)\n");
    p.fill_dirs = (int)nd;
    p.fill_dist = (int)dist;
    const std::string sp = word("MGM_SUBPIX", "1");  // (exit code 2: a command line the reference takes, refused here)
    o.subpix_interp = word("MGM_SUBPIX_INTERP", "cubic");
    if (!one_of(sp, {"1", "2", "4"})) return end(2, nullptr, "mgm: MGM_SUBPIX must be 1 (off), 2 or 4\n");
    if (!one_of(o.subpix_interp, {"linear", "cubic"})) return end(2, nullptr, "mgm: MGM_SUBPIX_INTERP must be linear or cubic\n");
    o.subpix = sp[0] - '0';
    if (p.nscales < 1 || p.nscales > 8) return end(1, nullptr, "mgm: -S nscales must be 1..8\n");
    if (argc > 1) p.f_u = argv[1];
    if (argc > 2) p.f_v = argv[2];
    if (argc > 3) p.f_out = argv[3];
    if (argc > 4) p.f_cost = argv[4];
    if (argc > 5) p.f_back = argv[5];
    if (argc < 4) return end(1, nullptr, "too few parameters\n");
    o.TSGM = (int)env_param(env, "TSGM", 4);
    o.FH = (int)env_param(env, "USE_TRUNCATED_LINEAR_POTENTIALS", 0);
    o.FIX = (int)env_param(env, "TSGM_FIX_OVERCOUNT", 1);
    o.census_win = (int)env_param(env, "CENSUS_NCC_WIN", 3);

    const double TSGM_ITER = env_param(env, "TSGM_ITER", 1);
    p.iterations = TSGM_ITER > 0 ? (int)std::ceil(TSGM_ITER) : 0;
    p.both = env_param(env, "TESTLRRL", 1) != 0;
    p.tau = (float)env_param(env, "TESTLRRL_TAU", 1.0);
    p.median = env_param(env, "MEDIAN", 0);
    p.ranged = !p.min_file.empty();
    p.rfl = env_param(env, "MGM_RIGHT_FROM_LEFT", 0) != 0 && p.both;
    p.uq = p.uniq != 0 || !p.conf_file.empty();
    p.debug = env_param(env, "TSGM_DEBUG", 0) != 0 && p.nscales == 1 && o.subpix == 1 && !p.rfl;
    p.batch_lr = env_param(env, "MGM_BATCH_LR", 1) != 0;
    p.ms_slack = (int)env_param(env, "MGM_MS_SLACK", 3);
    p.ms_radius = (int)env_param(env, "MGM_MS_RADIUS", 2);
    p.device = (int)env_param(env, "MGM_DEVICE", 0);
    p.place_tries = (int)env_param(env, "MGM_PLACE_TRIES", 0);
    p.stats = env_flag(env, "MGM_HIP_STATS");
    p.kernels = env_flag(env, "MGM_HIP_KERNELS");
    p.orderly_exit = env_flag(env, "MGM_HIP_ORDERLY_EXIT");
    if (const char *dl = env("MGM_DEVICES")) {  // "0,1,2,3"
        p.devices_comma = strchr(dl, ',') != nullptr;
        for (const char *q = dl; *q;) {
            char *e;
            const long d = strtol(q, &e, 10);
            if (e == q) break;
            p.devices.push_back((int)d);
            q = *e == ',' ? e + 1 : e;
        }
    }

    const bool mode[N_MODES] = {p.rfl, p.uq, o.subpix > 1, p.consensus != 0 || !p.votes_file.empty(), p.energy != 0};
    const bool blocker[N_BLOCKERS] = {p.ranged, p.nscales > 1, p.iterations != 1, o.refine == "parabola" || o.refine == "cubic" || o.refine == "parabolaOCV",
                                      p.rfl, p.devices_comma, o.subpix > 1};
    p.err_text = first_exclusion(mode, blocker);
    // MGM_FILL_HOLES_OCC: the classification reads the right map that entered the left-right test
    if (p.err_text.empty() && !p.fill_occ.empty() && !p.both)
        p.err_text = "mgm: MGM_FILL_HOLES_OCC needs the right view: TESTLRRL=0 leaves none (MGM_RIGHT_FROM_LEFT takes effect only with TESTLRRL != 0)\n";
    if (!p.err_text.empty()) {
        p.outcome = JobPlan::REFUSE;
        p.code = 2;
    }
    return p;
}

// What of a RUN plan can only be refused once the device side is up and the images are decoded: `multi_up` -- several devices
// are up in this session (resident mode: an earlier line brought them up, this line's MGM_DEVICES had no say); u_ny, v_ny --
// the heights of the two images.  code 0: go on.
struct Refusal {
    int code = 0;
    std::string err_text;
};
inline Refusal refuse_on_session(const JobPlan &p, bool multi_up, int u_ny, int v_ny)
{
    const bool mode[N_MODES] = {p.rfl, p.uq, p.o.subpix > 1, p.consensus != 0 || !p.votes_file.empty(), p.energy != 0};
    bool blocker[N_BLOCKERS] = {};
    blocker[B_DEVICES] = multi_up;
    Refusal r;
    r.err_text = first_exclusion(mode, blocker);
    if (r.err_text.empty() && p.rfl && u_ny != v_ny) r.err_text = "mgm: MGM_RIGHT_FROM_LEFT=1 needs two images of one height\n";
    if (!r.err_text.empty()) r.code = 2;
    return r;
}

}  // namespace mgm_cli
