// mgm_main.cc -- the `mgm` command line on top of libmgm_hip.so.
//
// A from-scratch restatement of the reference's host program (mgm.cc:266-450): same
// options, same environment parameters, same stdout, same left->right / right->left
// orchestration and post-processing -- with the hot path (cost volume, aggregation, WTA,
// refinement; mgm.cc:372-385 and 405-414) running on the MI355X through the C ABI of
// include/mgm_hip.h.  Everything here is host glue; no stereo arithmetic of the path is
// computed on the CPU.  Image files (src/imgio.h): PNG, TIFF, PGM/PPM, PFM and .npy in -- what the
// reference's iio decodes them to -- and float TIFF, PFM or .npy out.
//
// This program's own modes beside the reference's options (each documented in README.md and DESIGN.md 7a-7i): -S, -c, -C FILE /
// MGM_CONSENSUS=k / MGM_CONSENSUS_TOL=1 (the consensus votes, 7h: how many passes vote for a run's map; `--help` does not name these
// three yet), MGM_RIGHT_FROM_LEFT, MGM_UNIQUENESS, MGM_SPECKLE, MGM_FILL_HOLES*, MGM_SUBPIX, and MGM_ENERGY=4|8 / MGM_ENERGY_MAP=FILE
// (7i: the model energy of every run and iteration on stderr; not in `--help` either).  TSGM_DEBUG=1 is the reference's own: its
// debug lines on stdout, the three energies of every iteration among them (7i).
//
// A command line is a JOB with three stages: DECODE (host: the input files -> planar float images), DEVICE (this thread:
// uploads, every kernel of the path, downloads; the job's stdout is written here, in order) and ENCODE (host: the output
// files).  A 1920x1080x256 pair is ~17 ms of device work between ~19 ms of decoding and ~9 ms of encoding, so the program
// is organised around its HOST costs:
//   * one-shot (`mgm u v out`): both inputs are decoded on their own threads while this thread brings the device context
//     up, and the context is torn down on a thread of its own while the outputs are encoded and written;
//   * resident (`mgm --batch FILE`): the three stages of consecutive jobs OVERLAP -- a decoder thread works ahead of the
//     device stage, a writer thread behind it -- and the device objects of a pair (images, volumes, maps) are kept and
//     refilled by the next pair of the same geometry instead of being freed and allocated again.  A failing job (bad
//     option, unreadable file, device-side refusal) fails alone: every device-side error is an exception caught per job.
//     A line whose input file is an earlier line's OUTPUT (a coarse-to-fine chain: -m/-M written by the line before) is
//     decoded only once that output has been written: lines behave as if run one after the other.
// MGM_HIP_STATS=1 prints the wall-time breakdown on stderr; MGM_HIP_KERNELS=1 the names of the kernels a job launched.
//
// WITH_MGM2=1 (mgm_naive_parallelism, mgm_core.cc:632-831): every pass on its own private Lr volume, all passes in
// flight at once, then the volumes accumulated into S -- which is how the device path is organised anyway
// (DESIGN.md 4).  The reference accumulates in thread-finish order (798-805); here the order is always 0, 1, ..., 7:
// what its default build (Makefile:1, no OpenMP) and any run with one thread compute, and one member of the outcome
// set of a threaded run.  So the flag is accepted and changes nothing.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unistd.h>
#include <vector>

#include "../include/mgm_hip.h"
#include "imgio.h"
#include "mgm_jobplan.h"

using mgm_cli::JobPlan;
using mgm_cli::Opts;

// ---- MGM_HIP_STATS=1: where the wall time of the run goes (stderr, one line) ------------------
struct Stopwatch {
    bool on;
    explicit Stopwatch(const JobPlan &p) : on(p.stats) {}
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    std::string line;
    void mark(const char *what)
    {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        char buf[96];
        snprintf(buf, sizeof buf, " %s %.1f", what, std::chrono::duration<double, std::milli>(now - last).count());
        line += buf;
        last = now;
    }
    // milliseconds between exec and main(): dynamic loading of the HIP runtime and its static initialisers (10 ms ticks)
    static double premain_ms()
    {
        double up = 0;
        long long start = 0;
        if (FILE *f = fopen("/proc/uptime", "r")) {
            if (fscanf(f, "%lf", &up) != 1) up = 0;
            fclose(f);
        }
        if (FILE *f = fopen("/proc/self/stat", "r")) {
            char buf[1024];
            const size_t n = fread(buf, 1, sizeof buf - 1, f);
            fclose(f);
            buf[n] = 0;
            if (const char *q = strrchr(buf, ')')) {  // fields after "(comm)": state is #3, starttime #22
                int field = 2;
                for (q++; *q && field < 22; q++)
                    if (*q == ' ') field++;
                start = atoll(q);
            }
        }
        return (up - (double)start / 100.0) * 1e3;
    }
    double pre = on ? premain_ms() : 0;
    void report(const char *stage)
    {
        if (!on) return;
        fprintf(stderr, "[mgm stats] exec -> main() ~%.0f ms (10 ms ticks);[mgm stats] %s, ms:%s | total %.1f\n", pre, stage, line.c_str(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
};

static void remove_nonfinite(HostImg &u, float v)  // img_tools.h:37-41
{
    for (float &x : u.data)
        if (!std::isfinite(x)) x = v;
}

// A device-side failure: thrown, never exit() -- in resident mode the job fails and the next one runs.
// code(): the process exit code of a one-shot run (2: valid in the reference, refused here).
struct DeviceError : std::runtime_error {
    int rc;
    DeviceError(int rc_, const std::string &m) : std::runtime_error(m), rc(rc_) {}
    int code() const { return rc == MGM_ERR_UNSUPPORTED ? 2 : 1; }
};
[[noreturn]] static void die(mgm_ctx *ctx, int rc, const char *what)
{
    char head[96];
    snprintf(head, sizeof head, "%s failed (%d): ", what, rc);
    throw DeviceError(rc, std::string(head) + (ctx ? mgm_last_error(ctx) : ""));
}

// One run of the path: mgm.cc:372 + 376-385 (u,v) or 373 + 405-414 (v,u with the negated range), in stages so
// that the two runs of a pair can share one launch of the pass kernel (mgm_aggregate_batch_dev).
struct Run {
    mgm_img *du = nullptr, *dv = nullptr, *dw = nullptr, *dout = nullptr, *dcost = nullptr, *dspare = nullptr;
    mgm_cv *C = nullptr;
    bool weighted_msg = false, borrowed_uv = false, ragged = false;
    int nx = 0, ny = 0, nch = 0, vnx = 0, vny = 0, dmin = 0, dmax = 0;  // (what the kept objects were made for)
    int subpix = 1;  // ... and the label spacing of C: its labels are subpix * dmin .. subpix * dmax
};

static void free_run(mgm_ctx *ctx, Run &r)
{
    mgm_cv_free(ctx, r.C);
    if (!r.borrowed_uv) {
        mgm_img_free(ctx, r.du);
        mgm_img_free(ctx, r.dv);
    }
    for (mgm_img *im : {r.dw, r.dout, r.dcost, r.dspare}) mgm_img_free(ctx, im);
    r = Run();
}

struct ImgHold {  // a device image freed with its scope (several in one declaration: the last one first)
    mgm_ctx *ctx;
    mgm_img *im = nullptr;
    ~ImgHold() { mgm_img_free(ctx, im); }
};

// the device image of `h`: a kept one of the same size refilled, else a new one
static void upload_into(mgm_ctx *ctx, const HostImg &h, mgm_img **im)
{
    int nx = 0, ny = 0, nch = 0, rc;
    if (*im && mgm_img_dims(*im, &nx, &ny, &nch) == MGM_OK && nx == h.nx && ny == h.ny && nch == h.nch) {
        if ((rc = mgm_img_update(ctx, *im, h.data.data()))) die(ctx, rc, "upload");
        return;
    }
    mgm_img_free(ctx, *im);
    *im = nullptr;
    if ((rc = mgm_img_upload(ctx, h.data.data(), h.nx, h.ny, h.nch, im))) die(ctx, rc, "upload");
}
static void image_like(mgm_ctx *ctx, int nx, int ny, int nch, mgm_img **im)  // a kept image of that size, or a new one
{
    int ax = 0, ay = 0, ac = 0, rc;
    if (*im && mgm_img_dims(*im, &ax, &ay, &ac) == MGM_OK && ax == nx && ay == ny && ac == nch) return;
    mgm_img_free(ctx, *im);
    *im = nullptr;
    if ((rc = mgm_img_create(ctx, nx, ny, nch, im))) die(ctx, rc, "mgm_img_create");
}

// `r` may hold the objects of an earlier pair (resident mode): what fits is refilled in place, the rest replaced.
// `uv_from`: the run of the same pair the other way round, whose uploaded images this one borrows (v,u instead of u,v).
static void prepare_run(mgm_ctx *ctx, const HostImg &u, const HostImg &v, int dmin, int dmax, const Opts &o, Run &r,
                        const HostImg *lo = nullptr, const HostImg *hi = nullptr, const Run *uv_from = nullptr)
{
    int rc;
    bool ragged = false;
    if (lo) {  // range images (-m/-M, mgm.cc:342-353): Dvec takes them as ints (mgm_costvolume.h:323)
        dmin = (int)lo->data[0];
        dmax = (int)hi->data[0];
        for (size_t i = 0; i < lo->data.size(); i++) ragged |= (int)lo->data[i] != dmin || (int)hi->data[i] != dmax;
    }
    if (ragged)
        for (size_t i = 0; i < lo->data.size(); i++) {
            dmin = std::min(dmin, (int)lo->data[i]);
            dmax = std::max(dmax, (int)hi->data[i]);
        }
    const bool keep = r.C && !r.ragged && !ragged && r.nx == u.nx && r.ny == u.ny && r.nch == u.nch && r.vnx == v.nx && r.vny == v.ny &&
                      r.dmin == dmin && r.dmax == dmax && r.subpix == o.subpix && r.borrowed_uv == (uv_from != nullptr);
    if (!keep) free_run(ctx, r);
    r.nx = u.nx, r.ny = u.ny, r.nch = u.nch, r.vnx = v.nx, r.vny = v.ny, r.dmin = dmin, r.dmax = dmax, r.ragged = ragged;
    r.weighted_msg = false;
    r.subpix = o.subpix;
    if (uv_from) {
        r.du = uv_from->dv;
        r.dv = uv_from->du;
        r.borrowed_uv = true;
    } else {
        upload_into(ctx, u, &r.du);
        upload_into(ctx, v, &r.dv);
    }
    // compute_mgm_weights(u, aP2, aThresh)   [aP1 is parsed and unused in the reference too, mgm.cc:372].  With -aP2 1 (the
    // default) every weight is 1 whatever the image (ws(), mgm_weights.h:38-42, returns aP3 or 1): mgm() then takes the
    // unweighted update functions (mgm_core.cc:420-423) -- no planes to compute, upload or scan.
    if (o.aP2 != 1.0f) {
        if ((rc = mgm_weights_dev(ctx, r.du, o.aP2, o.aThresh, &r.dw))) die(ctx, rc, "mgm_weights");
        // mgm() announces the weighted mode on stdout (mgm_core.cc:420-423)
        std::vector<float> w((size_t)u.npix() * 8);
        if ((rc = mgm_img_download(ctx, r.dw, w.data()))) die(ctx, rc, "download");
        r.weighted_msg = std::any_of(w.begin(), w.end(), [](float x) { return x != 1.0f; });
    } else if (r.dw) {
        mgm_img_free(ctx, r.dw);
        r.dw = nullptr;
    }
    if (ragged) {
        ImgHold dhi{ctx}, dlo{ctx};
        if ((rc = mgm_img_upload(ctx, lo->data.data(), u.nx, u.ny, 1, &dlo.im)) || (rc = mgm_img_upload(ctx, hi->data.data(), u.nx, u.ny, 1, &dhi.im)))
            die(ctx, rc, "upload");
        if ((rc = mgm_costvolume_build_ranged_dev(ctx, r.du, r.dv, dlo.im, dhi.im, dmin, dmax, o.prefilter.c_str(), o.distance.c_str(), o.truncDist,
                                                  o.census_win, &r.C)))
            die(ctx, rc, "mgm_costvolume_build_ranged");
    } else if (o.subpix > 1) {  // MGM_SUBPIX: the fine volume, labels subpix * dmin .. subpix * dmax (never with range images)
        if ((rc = mgm_costvolume_build_subpix_dev(ctx, r.du, r.dv, dmin, dmax, o.subpix, o.subpix_interp.c_str(), o.prefilter.c_str(), o.distance.c_str(),
                                                  o.truncDist, o.census_win, &r.C)))
            die(ctx, rc, "mgm_costvolume_build_subpix");
    } else if ((rc = mgm_costvolume_build_dev(ctx, r.du, r.dv, dmin, dmax, o.prefilter.c_str(), o.distance.c_str(), o.truncDist, o.census_win, &r.C))) {
        die(ctx, rc, "mgm_costvolume_build");
    }
    image_like(ctx, u.nx, u.ny, 1, &r.dout);
    image_like(ctx, u.nx, u.ny, 1, &r.dcost);
}

static void aggregate_run(mgm_ctx *ctx, const Opts &o, Run &r)
{
    const int rc = mgm_aggregate_dev(ctx, r.C, r.dw, o.P1, o.P2, o.NDIR, o.TSGM, o.FH, o.FIX, o.refine.c_str(), r.dout, r.dcost, nullptr);
    if (rc) die(ctx, rc, "mgm_aggregate");
}

// MGM_DEVICES=a,b,...: the passes of each mgm() run sharded over several GPUs of the node (mgm_multi_aggregate: every
// device builds the cost volume from the images, runs its block of passes, row slabs travel over RCCL, ordered sum and
// WTA per device, rows gathered on the first device).  `r` has been prepared on the first device.
static void aggregate_run_multi(mgm_multi *m, const HostImg &u, const HostImg &v, int dmin, int dmax, const Opts &o, Run &r)
{
    const int n = mgm_multi_size(m);
    std::vector<Run> shadow(n);
    std::vector<const mgm_cv *> Cs(n);
    std::vector<const mgm_img *> Ws(n);
    Cs[0] = r.C;
    Ws[0] = r.dw;
    auto drop = [&] {
        for (int k = 1; k < n; k++) free_run(mgm_multi_ctx(m, k), shadow[k]);
    };
    try {
        for (int k = 1; k < n; k++) {
            prepare_run(mgm_multi_ctx(m, k), u, v, dmin, dmax, o, shadow[k]);
            Cs[k] = shadow[k].C;
            Ws[k] = shadow[k].dw;
        }
    } catch (...) {
        drop();
        throw;
    }
    const int rc = mgm_multi_aggregate(m, Cs.data(), r.dw ? Ws.data() : nullptr, o.P1, o.P2, o.NDIR, o.TSGM, o.FH, o.FIX, o.refine.c_str(), r.dout, r.dcost);
    drop();
    if (rc) {
        char head[96];
        snprintf(head, sizeof head, "mgm_multi_aggregate failed (%d): ", rc);
        throw DeviceError(rc, std::string(head) + mgm_multi_last_error(m));
    }
}

// what mgm() and print_solution_energy put on stdout for one run (mgm_core.cc:420-423, 491; mgm_print_energy.h:100-112):
// `energy` is the rest of the digits' line under TSGM_DEBUG, else the line just ends
static void report_run(const Opts &o, const Run &r, const std::string &energy = "")
{
    if (r.weighted_msg) printf(" USING IMAGE DEPENDENT WEIGHTS\n");
    for (int p = 0; p < o.NDIR; p++) printf("%d", p);
    printf("%s", energy.empty() ? "\n" : energy.c_str());
    fflush(stdout);
}

// the reference's tables of names (mgm_costvolume.h:170-207, mgm_refine.h:15-35): an unknown name is the first entry
static int name_index(const std::string &n, std::initializer_list<const char *> names)
{
    int r = 0, i = 0;
    for (const char *s : names) {
        if (n == s) r = i;
        i++;
    }
    return r;
}
static const std::initializer_list<const char *> REFINEMENTS = {"none", "vfit", "parabola", "cubic", "parabolaOCV"};

// TSGM_DEBUG: what allocate_and_fill_sgm_costvolume says about one volume build (mgm_costvolume.h:357-383)
static void debug_costvolume_lines(const Opts &o)
{
    static const char *const dist[] = {"ad", "sd", "census", "ncc", "btad", "btsd"}, *const pre[] = {"none", "census", "sobelx", "gblur"};
    int di = name_index(o.distance, {"ad", "sd", "census", "ncc", "btad", "btsd"}), pi = name_index(o.prefilter, {"none", "census", "sobelx", "gblur"});
    if (di == 2 || pi == 1) {
        printf("costvolume: changing both distance and prefilter to CENSUS\n");
        di = 2, pi = 1;
    }
    printf("costvolume: selecting distance  %s\n", dist[di]);
    printf("costvolume: selecting prefilter %s\n", pre[pi]);
    printf("costvolume: truncate distances at %f\n", o.truncDist);
    if (pi == 1) printf("costvolume: applying census with window of size %d\n", o.census_win / 2 * 2 + 1);
    if (pi == 2) printf("costvolume: applying sobel filter\n");
    if (pi == 3) printf("costvolume: applying gblur(s=1) filter\n");
    fflush(stdout);
}

// TSGM_DEBUG and MGM_ENERGY: the energy of the UNREFINED map of every iteration of a run
struct Probe {
    bool debug = false;       // TSGM_DEBUG: the reference's three figures on stdout, behind the digits of the passes
    int conn = 0;             // MGM_ENERGY: the model energy over 4 or 8 neighbours on stderr (0: off)
    mgm_img **map = nullptr;  // MGM_ENERGY_MAP: where the model energy's map of this run goes (nullptr: nowhere)
    char run = 'L';
    bool on() const { return debug || conn != 0; }
};

static HostImg download(mgm_ctx *ctx, const mgm_img *im, int nx, int ny, int nch)
{
    HostImg h;
    h.nx = nx;
    h.ny = ny;
    h.nch = nch;
    h.data.resize((size_t)nx * ny * nch);
    const int rc = mgm_img_download(ctx, im, h.data.data());
    if (rc) die(ctx, rc, "download");
    return h;
}

// MGM_SUBPIX: a run's refined map from fine labels to pixels, in place, right after its search
static void rescale_run(mgm_ctx *ctx, const Opts &o, Run &r)
{
    if (o.subpix <= 1) return;
    if (int rc = mgm_subpix_scale_dev(ctx, r.dout, o.subpix, r.dout)) die(ctx, rc, "mgm_subpix_scale");
}

// outoff = median_filter(outoff, MEDIAN) on the device (mgm.cc:396, 419), any radius
static void median_run(mgm_ctx *ctx, Run &r, int radius)
{
    int rc;
    image_like(ctx, r.nx, r.ny, 1, &r.dspare);
    if ((rc = mgm_median_dev(ctx, r.dout, radius, r.dspare))) die(ctx, rc, "mgm_median");
    std::swap(r.dout, r.dspare);
}

// -c / MGM_UNIQUENESS, right behind the aggregation of `r`: the runner-up search over the Lr volumes the context
// still holds of that run, then conf = 1 - cost1 / cost2 into *conf (if wanted) and, with ratio != 0, NaN into the run's
// (refined) map wherever conf < ratio
static void uniqueness_run(mgm_ctx *ctx, const Opts &o, Run &r, float ratio, int radius, mgm_img **conf)
{
    ImgHold out2{ctx}, cost2{ctx}, cost1{ctx};
    int rc;
    for (mgm_img **im : {&out2.im, &cost2.im, &cost1.im})
        if ((rc = mgm_img_create(ctx, r.nx, r.ny, 1, im))) die(ctx, rc, "mgm_img_create");
    if (conf && (rc = mgm_img_create(ctx, r.nx, r.ny, 1, conf))) die(ctx, rc, "mgm_img_create");
    if ((rc = mgm_wta_runnerup_dev(ctx, r.C, o.NDIR, o.FIX, radius, out2.im, cost2.im, nullptr, cost1.im))) die(ctx, rc, "mgm_wta_runnerup");
    if ((rc = mgm_uniqueness_dev(ctx, r.dout, cost1.im, cost2.im, ratio, ratio != 0 ? r.dout : nullptr, conf ? *conf : nullptr)))
        die(ctx, rc, "mgm_uniqueness");
}

// -C / MGM_CONSENSUS, right behind the search, the refinement and the last iteration of `r` and before its map
// is rescaled (MGM_SUBPIX: the tolerance is per fine label): how many passes of the aggregation the context still holds vote
// for the run's map, into *votes (if wanted) and, with minvotes > 0, NaN into the map wherever fewer do
static void consensus_run(mgm_ctx *ctx, const Opts &o, Run &r, float tol, int minvotes, mgm_img **votes)
{
    ImgHold mine{ctx};
    int rc;
    if ((rc = mgm_img_create(ctx, r.nx, r.ny, 1, votes ? votes : &mine.im))) die(ctx, rc, "mgm_img_create");
    mgm_img *vt = votes ? *votes : mine.im;
    if ((rc = mgm_wta_consensus_dev(ctx, r.C, o.NDIR, r.dout, tol, vt, nullptr))) die(ctx, rc, "mgm_wta_consensus");
    if (minvotes > 0 && (rc = mgm_consensus_filter_dev(ctx, r.dout, vt, minvotes, r.dout))) die(ctx, rc, "mgm_consensus_filter");
}

// MGM_SPECKLE=maxsize: the speckle filter, in place, on a job's FINAL left map
static void speckle_map(mgm_ctx *ctx, mgm_img *d, int maxsize, float maxdiff)
{
    if (int rc = mgm_speckle_dev(ctx, d, maxsize, maxdiff, d, nullptr)) die(ctx, rc, "mgm_speckle");
}

// MGM_FILL_HOLES=median|min|max: hole filling, in place, on a job's FINAL left map, after every rejection step
static void fill_holes_map(mgm_ctx *ctx, mgm_img *d, const std::string &mode, int dirs, int maxdist)
{
    if (int rc = mgm_fill_holes_dev(ctx, d, mode.c_str(), dirs, maxdist, d, nullptr)) die(ctx, rc, "mgm_fill_holes");
}

// MGM_FILL_HOLES_OCC=seclow|sechigh|min|max|median: the holes of the final left map are classified from the right map
// as it entered the left-right test (`other`), over -r/-R at TESTLRRL_TAU; occlusions take `occ`, mismatches MGM_FILL_HOLES's rule
static void fill_holes_classified_map(mgm_ctx *ctx, mgm_img *d, const mgm_img *other, int dmin, int dmax, float tau, const std::string &occ,
                                      const std::string &mis, int dirs, int maxdist)
{
    ImgHold cls{ctx};
    int nx, ny, nch, rc;
    if ((rc = mgm_img_dims(d, &nx, &ny, &nch)) || (rc = mgm_img_create(ctx, nx, ny, 1, &cls.im))) die(ctx, rc, "mgm_img_create");
    if ((rc = mgm_classify_holes_dev(ctx, d, other, dmin, dmax, tau, cls.im))) die(ctx, rc, "mgm_classify_holes");
    if ((rc = mgm_fill_holes_classified_dev(ctx, d, cls.im, occ.c_str(), mis.c_str(), dirs, maxdist, d, nullptr))) die(ctx, rc, "mgm_fill_holes_classified");
}

// iterations 2..TSGM_ITER of main()'s loop (mgm.cc:377-388): the ranges narrow around the previous solution
// (update_dmin_dmax), the volume -- and with it every scan-line pass -- stays the same, so only the winner search and
// the refinement are redone, on the Lr volumes the context still holds
// ... and what the run says about every iteration, the first one included (report_run).  With a probe: the energies of the
// iteration's UNREFINED map (mgm()'s own outoff, mgm.cc:381-383), against the volume built before the loop -- the run's map itself
// when there is no refinement, else the same winner search again without one, over the iteration's ranges.
static std::string probe_iteration(mgm_ctx *ctx, const Opts &o, Run &r, const Probe &pb, int iter, const mgm_img *dlo, const mgm_img *dhi)
{
    if (!pb.on()) return "";
    ImgHold unc{ctx}, un{ctx};
    const mgm_img *d = r.dout;
    int rc;
    if (name_index(o.refine, REFINEMENTS) != 0) {
        if ((rc = mgm_img_create(ctx, r.nx, r.ny, 1, &un.im)) || (rc = mgm_img_create(ctx, r.nx, r.ny, 1, &unc.im))) die(ctx, rc, "mgm_img_create");
        if ((rc = mgm_wta_windowed_dev(ctx, r.C, o.NDIR, o.FIX, "none", dlo, dhi, un.im, unc.im))) die(ctx, rc, "mgm_wta_windowed");
        d = un.im;
    }
    mgm_energy_params q{};
    q.P1 = o.P1, q.P2 = o.P2;
    mgm_energy_totals t{};
    std::string line;
    if (pb.debug) {  // mgm_print_energy.h:104-107
        float e[3];
        for (q.kind = 0; q.kind < 3; q.kind++) {
            if ((rc = mgm_energy_dev(ctx, r.C, d, &q, nullptr, &t))) die(ctx, rc, "mgm_energy");
            e[q.kind] = t.serial;
        }
        char buf[160];
        snprintf(buf, sizeof buf, " ENERGY L1trunc: %.9e\tL1: %.9e\tL2: %.9e\n", e[0], e[1], e[2]);
        line = buf;
    }
    if (pb.conn) {
        q.kind = 3, q.connectivity = pb.conn, q.use_fh = o.FH != 0, q.w8 = r.dw;
        if (pb.map) image_like(ctx, r.nx, r.ny, 1, pb.map);
        if ((rc = mgm_energy_dev(ctx, r.C, d, &q, pb.map ? *pb.map : nullptr, &t))) die(ctx, rc, "mgm_energy");
        fprintf(stderr, "[mgm energy] run=%c iter=%d total=%.17g data=%.17g smooth=%.17g finite=%llu/%llu\n", pb.run, iter, t.total, t.data, t.smooth,
                t.finite, t.pixels);
    }
    return line;
}

static void iterate_run(mgm_ctx *ctx, const Opts &o, Run &r, int iterations, int dmin, int dmax, const Probe &pb, const HostImg *lo0 = nullptr,
                        const HostImg *hi0 = nullptr)
{
    const int refining = name_index(o.refine, REFINEMENTS);
    ImgHold dhi{ctx}, dlo{ctx};
    int rc;
    if (iterations >= 2 || (pb.on() && refining)) {  // the ranges as device images: of the first iteration, then narrowed in place
        std::vector<float> lo((size_t)r.nx * r.ny, (float)dmin), hi((size_t)r.nx * r.ny, (float)dmax);
        if (lo0) {
            lo = lo0->data;
            hi = hi0->data;
        }
        if ((rc = mgm_img_upload(ctx, lo.data(), r.nx, r.ny, 1, &dlo.im)) || (rc = mgm_img_upload(ctx, hi.data(), r.nx, r.ny, 1, &dhi.im))) die(ctx, rc, "upload");
    }
    for (int it = 0; it < iterations; it++) {
        if (it > 0) {
            if ((rc = mgm_update_ranges_dev(ctx, r.dout, dlo.im, dhi.im, 3, 2))) die(ctx, rc, "mgm_update_ranges");
            if ((rc = mgm_wta_windowed_dev(ctx, r.C, o.NDIR, o.FIX, o.refine.c_str(), dlo.im, dhi.im, r.dout, r.dcost))) die(ctx, rc, "mgm_wta_windowed");
        }
        report_run(o, r, probe_iteration(ctx, o, r, pb, it, dlo.im, dhi.im));
        if (pb.debug && refining) {  // mgm_refine.h:47-49
            printf("refinement: using %s\n", REFINEMENTS.begin()[refining]);
            fflush(stdout);
        }
    }
}

// The device side of the process: created for the first job, kept for the following ones (resident mode) together with
// the device objects of the last pair (refilled by the next pair of the same geometry).
struct Session {
    mgm_ctx *ctx = nullptr;
    mgm_multi *multi = nullptr;
    std::vector<int> devs;
    bool tried = false, resident = false;
    int rc_ctx = 0;
    Run L, R;
};

// ---- a job ------------------------------------------------------------------------------------------------------------
struct Job {
    std::vector<std::string> tok;  // the command line (argv[0] included)
    JobPlan p;                     // what it is going to do (mgm_jobplan.h)
    // decoded
    HostImg u, v, rlo, rhi;
    std::exception_ptr decode_err;
    // results of the device stage
    HostImg outoff, outcost, syn, nolr, conf, votes, energy;
    int rc = 0;  // the job's exit code
};

// a job whose plan is to end before any work: its texts, its code
static bool ends_early(Job &j)
{
    if (j.p.outcome != JobPlan::END) return false;
    fputs(j.p.out_text.c_str(), stdout);
    fputs(j.p.err_text.c_str(), stderr);
    j.rc = j.p.code;
    return true;
}

// DECODE: the input files of a job (any thread; touches neither the device nor stdout).  Both images on their own threads.
static void decode_job(Job &j)
{
    if (j.p.outcome != JobPlan::RUN) return;
    std::exception_ptr eu, ev;
    std::thread tv([&] { try { j.v = imgio::read(j.p.f_v); remove_nonfinite(j.v, 0); } catch (...) { ev = std::current_exception(); } });
    try {
        j.u = imgio::read(j.p.f_u);
        remove_nonfinite(j.u, 0);
    } catch (...) {
        eu = std::current_exception();
    }
    tv.join();
    j.decode_err = eu ? eu : ev;
    if (!j.decode_err && j.p.ranged) {
        try {
            j.rlo = imgio::read(j.p.min_file);
            j.rhi = imgio::read(j.p.max_file);
        } catch (...) {
            j.decode_err = std::current_exception();
        }
    }
}

// ENCODE: the output files of a job (any thread)
static void encode_job(Job &j)
{
    if (j.p.outcome == JobPlan::END || j.rc != 0) return;
    const JobPlan &p = j.p;
    try {
        if (!p.nolr_file.empty()) imgio::write(p.nolr_file, j.nolr);
        if (!p.conf_file.empty()) imgio::write(p.conf_file, j.conf);
        if (!p.votes_file.empty()) imgio::write(p.votes_file, j.votes);
        if (!p.energy_map.empty() && !j.energy.data.empty()) imgio::write(p.energy_map, j.energy);  // (no iteration: no map)
        imgio::write(p.f_out, j.outoff);
        if (!p.f_cost.empty()) imgio::write(p.f_cost, j.outcost);
        if (!p.f_back.empty()) imgio::write(p.f_back, j.syn);
    } catch (const std::exception &e) {
        fprintf(stderr, "mgm: %s\n", e.what());
        j.rc = 1;
    }
}

static void bring_up(Session &S, const JobPlan &p)
{
    if (S.tried) return;  // (resident mode: the first job brings the device side up, the others find it there)
    S.tried = true;
    S.devs = p.devices;
    if (S.devs.size() > 1 && (p.iterations > 1 || p.ranged)) {
        fprintf(stderr, "mgm: MGM_DEVICES: TSGM_ITER > 1 and range images run on the first device only\n");
        S.devs.resize(1);
    }
    if (S.devs.size() > 1 && p.nscales > 1) {
        fprintf(stderr, "mgm: MGM_DEVICES: -S (coarse to fine) runs on the first device only\n");
        S.devs.resize(1);
    }
    if (S.devs.size() > 1) {
        if ((S.rc_ctx = mgm_multi_create(S.devs.data(), (int)S.devs.size(), &S.multi)) == 0) S.ctx = mgm_multi_ctx(S.multi, 0);
    } else {
        S.rc_ctx = mgm_ctx_create(S.devs.size() == 1 ? S.devs[0] : p.device, &S.ctx);
        // MGM_PLACE_TRIES=n: a context that stays may try n physical placements of its workspace and keep the fastest (off by default: three
        // more allocations of a 34 GB workspace cost ~2 s, what 100 further pairs gain back)
        if (S.rc_ctx == 0 && S.resident) (void)mgm_ctx_set_placement_tries(S.ctx, p.place_tries);
        if (S.rc_ctx == 0 && p.kernels) (void)mgm_timing_enable(S.ctx, 1);
    }
}

// MGM_HIP_KERNELS=1: which kernels the job ran, in launch order, on stderr (tests assert which pass kernel a command line took)
static void report_kernels(mgm_ctx *ctx)
{
    const int n = mgm_timing_count(ctx);
    fprintf(stderr, "[mgm kernels]");
    for (int k = 0; k < n; k++) {
        const char *name = nullptr;
        float ms = 0;
        if (mgm_timing_get(ctx, k, &name, &ms) == 0 && name) fprintf(stderr, " %s", name);
    }
    fprintf(stderr, "\n");
    (void)mgm_timing_reset(ctx);
}

// The end of every job, on its final left map `out`: MGM_SPECKLE, then MGM_FILL_HOLES (7e; with MGM_FILL_HOLES_OCC
// classified from `right_nolr`, the right map as it entered the left-right test, 7f) -- after every rejection step, before the
// back-projected image is made --, then the downloads: the map, the cost map, -c's map, the back-projected image (mgm.cc:433-443)
// of du and dv.  `between`: what the caller does after the last kernel is enqueued and before the first download.
static void finish_job(mgm_ctx *ctx, Job &j, mgm_img *out, const mgm_img *right_nolr, const mgm_img *cost, const mgm_img *conf, const mgm_img *du,
                       const mgm_img *dv, Stopwatch &sw, const std::function<void()> &between)
{
    const JobPlan &p = j.p;
    const HostImg &u = j.u;
    if (p.speckle > 0) speckle_map(ctx, out, p.speckle, p.speckle_diff);
    if (!p.fill_occ.empty()) fill_holes_classified_map(ctx, out, right_nolr, p.o.dmin, p.o.dmax, p.tau, p.fill_occ, p.fill, p.fill_dirs, p.fill_dist);
    else if (!p.fill.empty()) fill_holes_map(ctx, out, p.fill, p.fill_dirs, p.fill_dist);
    between();
    j.outoff = download(ctx, out, u.nx, u.ny, 1);
    sw.mark("device+download");
    if (!p.f_cost.empty()) j.outcost = download(ctx, cost, u.nx, u.ny, 1);
    if (conf) j.conf = download(ctx, conf, u.nx, u.ny, 1);
    if (!p.f_back.empty()) {
        ImgHold syn{ctx};
        int rc;
        if ((rc = mgm_img_create(ctx, u.nx, u.ny, u.nch, &syn.im))) die(ctx, rc, "mgm_img_create");
        if ((rc = mgm_backproject_dev(ctx, du, dv, out, syn.im))) die(ctx, rc, "mgm_backproject");
        j.syn = download(ctx, syn.im, u.nx, u.ny, u.nch);
    }
}

// -S nscales > 1: the pair coarse to fine (mgm_multiscale_pair_dev; DESIGN.md "multiscale" -- this program's own mode, the
// reference has none).  stdout: level by level from the coarsest, the lines a single-scale job prints for that level.  The
// nolr map, the cost map and the back-projected image refer to the full-size level.  Device objects are this job's own.
// `o`: the job's options with the penalties scaled by the number of channels.
static void multiscale_job(Session &S, Job &j, const Opts &o, const HostImg *plo, const HostImg *phi, Stopwatch &sw)
{
    mgm_ctx *ctx = S.ctx;
    const JobPlan &pl = j.p;
    free_run(ctx, S.R);  // (kept from an earlier single-scale pair)
    free_run(ctx, S.L);
    const HostImg &u = j.u, &v = j.v;
    // (rnolr -- MGM_FILL_HOLES_OCC: the full-size right map before its left-right test)
    ImgHold votes{ctx}, rnolr{ctx}, nolr{ctx}, cost{ctx}, out{ctx}, dhi{ctx}, dlo{ctx}, dv{ctx}, du{ctx};
    int rc;
    if ((rc = mgm_img_upload(ctx, u.data.data(), u.nx, u.ny, u.nch, &du.im)) || (rc = mgm_img_upload(ctx, v.data.data(), v.nx, v.ny, v.nch, &dv.im)))
        die(ctx, rc, "upload");
    if (plo && ((rc = mgm_img_upload(ctx, plo->data.data(), u.nx, u.ny, 1, &dlo.im)) || (rc = mgm_img_upload(ctx, phi->data.data(), u.nx, u.ny, 1, &dhi.im))))
        die(ctx, rc, "upload");
    for (mgm_img **im : {&out.im, &cost.im}) image_like(ctx, u.nx, u.ny, 1, im);
    if (!pl.nolr_file.empty()) image_like(ctx, u.nx, u.ny, 1, &nolr.im);
    if (!pl.fill_occ.empty()) image_like(ctx, v.nx, v.ny, 1, &rnolr.im);
    if (!pl.votes_file.empty()) image_like(ctx, u.nx, u.ny, 1, &votes.im);
    mgm_ms_level levels[8] = {};
    int nlev = 0;
    mgm_ms_params p{};
    p.struct_size = sizeof p;
    p.nscales = pl.nscales;
    p.slack = pl.ms_slack;
    p.radius = pl.ms_radius;
    p.dmin = o.dmin, p.dmax = o.dmax;
    p.lo = dlo.im, p.hi = dhi.im;
    p.P1 = o.P1, p.P2 = o.P2, p.NDIR = o.NDIR, p.TSGM = o.TSGM, p.use_fh = o.FH, p.fix_overcount = o.FIX;
    p.aP2 = o.aP2, p.aThresh = o.aThresh;
    p.prefilter = o.prefilter.c_str(), p.distance = o.distance.c_str(), p.truncDist = o.truncDist, p.census_win = o.census_win;
    p.refine = o.refine.c_str();
    p.iterations = pl.iterations, p.median = (int)pl.median, p.testlrrl = pl.both, p.tau = pl.tau;
    p.levels_run = &nlev, p.levels = levels;
    p.outR_nolr = rnolr.im;
    p.consensus_tol = pl.consensus_tol, p.consensus_min = pl.consensus, p.votesL = votes.im;
    sw.mark("upload");
    if ((rc = mgm_multiscale_pair_dev(ctx, du.im, dv.im, &p, out.im, cost.im, nullptr, nullptr, nolr.im))) die(ctx, rc, "mgm_multiscale_pair");
    for (int s = nlev - 1; s >= 0; s--)
        for (int k = 0; k < (pl.both ? 2 : 1); k++)
            for (int it = 0; it < pl.iterations; it++) {
                Run r;
                r.weighted_msg = levels[s].weighted[k] != 0;
                report_run(o, r);
            }
    sw.mark("enqueue");
    // (speckle and fill: once, on level 0's final map)
    finish_job(ctx, j, out.im, rnolr.im, cost.im, nullptr, du.im, dv.im, sw, [&] {
        if (!pl.nolr_file.empty()) j.nolr = download(ctx, nolr.im, u.nx, u.ny, 1);
        if (!pl.votes_file.empty()) j.votes = download(ctx, votes.im, u.nx, u.ny, 1);
    });
    sw.mark("download(rest)");
}

// DEVICE: everything between the decoded inputs and the downloaded maps; the job's stdout.  `decoded`: waits for the
// job's DECODE stage (which may run beside the context's creation).  Returns the job's exit code; device objects stay in
// S.L / S.R (kept for the next pair, or torn down by the caller).
static int device_job(Session &S, Job &j, const std::function<void()> &decoded, Stopwatch &sw)
{
    const JobPlan &p = j.p;
    Opts o = p.o;
    printf("%d %d\n", o.dmin, o.dmax);  // mgm.cc:328
    fflush(stdout);
    auto refused = [](int code, const std::string &err) {
        fputs(err.c_str(), stderr);
        return code;
    };
    if (p.outcome == JobPlan::REFUSE) return refused(p.code, p.err_text);
    try {
        bring_up(S, p);
        sw.mark("context");
        decoded();
        sw.mark("decode(rest)");
        if (j.decode_err) std::rethrow_exception(j.decode_err);
        mgm_ctx *ctx = S.ctx;
        mgm_multi *multi = S.multi;
        if (S.rc_ctx && S.devs.size() > 1) {
            fprintf(stderr, "mgm: MGM_DEVICES: cannot set up %d devices (mgm_multi_create = %d): %s\n", (int)S.devs.size(), S.rc_ctx, mgm_multi_last_error(nullptr));
            return 1;
        }
        if (S.rc_ctx) {
            fprintf(stderr, "mgm: no usable MI355X device (mgm_ctx_create = %d); there is no CPU path\n", S.rc_ctx);
            return 1;
        }
        if (multi && p.nscales > 1) {  // (resident mode: an earlier line brought several devices up)
            fprintf(stderr, "mgm: MGM_DEVICES: -S (coarse to fine) runs on the first device only\n");
            multi = nullptr;
        }
        if (multi && p.ranged) {
            fprintf(stderr, "mgm: --batch with MGM_DEVICES: range images are not supported on several devices\n");
            return 1;
        }
        const HostImg &u = j.u, &v = j.v;
        const mgm_cli::Refusal no = mgm_cli::refuse_on_session(p, multi != nullptr, u.ny, v.ny);
        if (no.code) return refused(no.code, no.err_text);
        HostImg &rlo = j.rlo, &rhi = j.rhi;  // -m / -M range images of the left->right run (mgm.cc:342-353); the right->left run keeps -r/-R
        if (p.ranged) {
            if (rlo.nx != u.nx || rlo.ny != u.ny || rhi.nx != u.nx || rhi.ny != u.ny || rlo.nch != 1 || rhi.nch != 1) {
                fprintf(stderr, "mgm: the -m/-M images must have the size of the left image\n");
                return 1;
            }
            remove_nonfinite(rlo, (float)o.dmin);
            remove_nonfinite(rhi, (float)o.dmax);
            for (size_t i = 0; i < rlo.data.size(); i++)
                if (rhi.data[i] < rlo.data[i] + 1) rhi.data[i] = ceilf(rlo.data[i] + 1);
        }
        const HostImg *plo = p.ranged ? &rlo : nullptr, *phi = p.ranged ? &rhi : nullptr;
        o.P1 *= u.nch;  // mgm.cc:356-357
        o.P2 *= u.nch;

        int rc;
        Run &L = S.L, &R = S.R;
        ImgHold dconf{ctx};  // -c: the confidence map, until it is downloaded
        ImgHold dvotes{ctx};  // -C: the votes map, until it is downloaded
        const bool cs = p.consensus != 0 || !p.votes_file.empty();
        ImgHold denergy{ctx};  // MGM_ENERGY_MAP: the left run's model-energy map, until it is downloaded
        Probe probeL, probeR;  // TSGM_DEBUG (ignored on several devices, as ever) / MGM_ENERGY
        probeL.debug = probeR.debug = p.debug && !multi;
        probeL.conn = probeR.conn = p.energy;
        probeL.map = p.energy_map.empty() ? nullptr : &denergy.im;
        probeR.run = 'R';
        const int ITER = p.iterations;
        const bool both = p.both, rfl = p.rfl;
        if (p.nscales > 1) {
            multiscale_job(S, j, o, plo, phi, sw);
            if (p.kernels && !multi) report_kernels(ctx);
            return 0;
        }
        if (!both && R.C) free_run(ctx, R);  // (kept from an earlier pair, not wanted by this one)
        prepare_run(ctx, u, v, o.dmin, o.dmax, o, L, plo, phi);
        bool together = false, r_ready = false;
        auto zero_run = [&](Run &r) {  // no iteration: mgm() is never called, outoff / outcost keep their zeros
            const std::vector<float> z((size_t)r.nx * r.ny, 0.0f);
            for (mgm_img **im : {&r.dout, &r.dcost})
                if ((rc = mgm_img_update(ctx, *im, z.data()))) die(ctx, rc, "upload");
        };
        // the right->left run reads the same two images the other way round: it borrows the left->right run's uploads
        // (not when the ranges are images: that run keeps -r/-R and is prepared -- and freed -- on its own)
        auto prepare_R = [&] {
            prepare_run(ctx, v, u, -o.dmax, -o.dmin, o, R, nullptr, nullptr, &L);  // mgm.cc:366, 405
            r_ready = true;
        };
        if (ITER == 0) {
            zero_run(L);
            together = true;  // (nothing to aggregate)
        }
        if (ITER > 0 && !multi && both && !rfl && !plo && u.nx == v.nx && u.ny == v.ny && p.batch_lr) {
            // both runs of the pair (mgm.cc:376-385 and 405-414) through ONE launch of the pass kernel
            prepare_R();
            const mgm_cv *Cs[2] = {L.C, R.C};
            const mgm_img *Ws[2] = {L.dw, R.dw};
            mgm_img *Os[2] = {L.dout, R.dout}, *Cc[2] = {L.dcost, R.dcost};
            rc = mgm_aggregate_batch_dev(ctx, 2, Cs, L.dw ? Ws : nullptr, o.P1, o.P2, o.NDIR, o.TSGM, o.FH, o.FIX, o.refine.c_str(), Os, Cc, nullptr);
            if (rc == MGM_OK) together = true;
            else if (rc == MGM_ERR_NOMEM) {  // 2*NDIR Lr volumes do not fit: one run after the other, as the reference does
                free_run(ctx, R);
                r_ready = false;
            } else if (rc != MGM_ERR_UNSUPPORTED) die(ctx, rc, "mgm_aggregate_batch");
            // (UNSUPPORTED: one image weighted, the other not -- the two runs take different update functions)
        }
        sw.mark("upload+enqueue");
        if (probeL.debug) debug_costvolume_lines(o);  // (of the left->right volume: built above, said here, where the reference builds it)
        if (ITER > 0) {
            if (multi) aggregate_run_multi(multi, u, v, o.dmin, o.dmax, o, L);
            else if (!together) aggregate_run(ctx, o, L);
            iterate_run(ctx, o, L, ITER, o.dmin, o.dmax, probeL, plo, phi);
            if (cs) consensus_run(ctx, o, L, p.consensus_tol, p.consensus, p.votes_file.empty() ? nullptr : &dvotes.im);
            rescale_run(ctx, o, L);
            if (p.uq) uniqueness_run(ctx, o, L, (float)p.uniq, p.uniq_radius, p.conf_file.empty() ? nullptr : &dconf.im);
        }
        if (p.median != 0) median_run(ctx, L, (int)p.median);
        if (!p.nolr_file.empty()) j.nolr = download(ctx, L.dout, L.nx, L.ny, 1);
        if (rfl) {
            // the right map out of the left run: no volume, no passes (R keeps only its two maps)
            if (R.C || R.nx != v.nx || R.ny != v.ny) free_run(ctx, R);
            R.nx = v.nx, R.ny = v.ny, R.nch = v.nch;
            image_like(ctx, v.nx, v.ny, 1, &R.dout);
            image_like(ctx, v.nx, v.ny, 1, &R.dcost);
            if ((rc = mgm_wta_right_dev(ctx, L.C, o.NDIR, o.FIX, o.refine.c_str(), R.dout, R.dcost))) die(ctx, rc, "mgm_wta_right");
            printf("right from left\n");
            fflush(stdout);
            if (p.median != 0) median_run(ctx, R, (int)p.median);
        } else if (both) {
            if (!r_ready) prepare_R();
            if (probeR.debug) debug_costvolume_lines(o);
            if (ITER == 0) {
                zero_run(R);
            } else {
                if (multi) aggregate_run_multi(multi, v, u, -o.dmax, -o.dmin, o, R);
                else if (!together) aggregate_run(ctx, o, R);
                iterate_run(ctx, o, R, ITER, -o.dmax, -o.dmin, probeR);
                if (p.consensus != 0) consensus_run(ctx, o, R, p.consensus_tol, p.consensus, nullptr);
                rescale_run(ctx, o, R);
                if (p.uniq != 0) uniqueness_run(ctx, o, R, (float)p.uniq, p.uniq_radius, nullptr);
            }
            if (p.median != 0) median_run(ctx, R, (int)p.median);
        }
        if (both) {
            // leftright_test both ways on copies of the unchecked maps (mgm.cc:420-423)
            image_like(ctx, L.nx, L.ny, 1, &L.dspare);
            image_like(ctx, R.nx, R.ny, 1, &R.dspare);
            if ((rc = mgm_leftright_dev(ctx, R.dout, L.dout, p.tau, R.dspare)) || (rc = mgm_leftright_dev(ctx, L.dout, R.dout, p.tau, L.dspare)))
                die(ctx, rc, "mgm_leftright");
            std::swap(L.dout, L.dspare);
            std::swap(R.dout, R.dspare);
        }
        // (with several devices `ctx` is the device that holds the gathered map; after the swap above R.dspare is the right map as it
        // entered the left-right test)
        finish_job(ctx, j, L.dout, R.dspare, L.dcost, dconf.im, L.du, L.dv, sw, [&] { sw.mark("enqueue(rest)"); });
        if (!p.votes_file.empty()) {  // (no iteration: mgm() was never called, no pass has voted)
            if (!dvotes.im) {
                image_like(ctx, u.nx, u.ny, 1, &dvotes.im);
                const std::vector<float> z((size_t)u.npix(), 0.0f);
                if ((rc = mgm_img_update(ctx, dvotes.im, z.data()))) die(ctx, rc, "upload");
            }
            j.votes = download(ctx, dvotes.im, u.nx, u.ny, 1);
        }
        if (denergy.im) j.energy = download(ctx, denergy.im, u.nx, u.ny, 1);
        sw.mark("download(rest)");
        if (p.kernels && !multi) report_kernels(ctx);
    } catch (const std::exception &e) {  // (a DeviceError, an unreadable input)
        fprintf(stderr, "mgm: %s\n", e.what());
        // whatever the failed job left half-made goes; the context stays (resident mode: the next job starts clean)
        if (S.ctx) {
            free_run(S.ctx, S.R);
            free_run(S.ctx, S.L);
        }
        const DeviceError *de = dynamic_cast<const DeviceError *>(&e);
        return de ? de->code() : 1;
    }
    return 0;
}

static void teardown(Session &S)
{
    if (S.ctx) {
        free_run(S.ctx, S.R);
        free_run(S.ctx, S.L);
    }
    if (S.multi) mgm_multi_destroy(S.multi);
    else if (S.ctx) mgm_ctx_destroy(S.ctx);
    S.ctx = nullptr;
    S.multi = nullptr;
}

// ---- one-shot ---------------------------------------------------------------------------------------------------------
static int run_one(int argc, char **argv)
{
    Job j;
    for (int i = 0; i < argc; i++) j.tok.push_back(argv[i]);
    j.p = mgm_cli::plan_job(j.tok, getenv);
    if (ends_early(j)) return j.rc;
    Stopwatch sw(j.p);
    Session S;
    // decode both inputs on their own threads while this one brings the device up (process start + HIP initialisation
    // + context is most of a run's wall time: the device work of a full-HD pair is ~17 ms)
    std::thread dec([&] { decode_job(j); });
    bool joined = false;
    j.rc = device_job(S, j, [&] { dec.join(); joined = true; }, sw);
    if (!joined) dec.join();
    if (j.rc) {
        fflush(stdout);
        fflush(stderr);
        return j.rc;  // (the process ends through the runtime's own handlers: a failed run is not timed)
    }
    // the device side is torn down (volumes, tens of GB of workspace) while the outputs are encoded and written
    std::thread down([&] { teardown(S); });
    encode_job(j);
    sw.mark("encode+write");
    down.join();
    sw.mark("teardown(rest)");
    sw.report("one-shot");
    // Everything is written and the device side is down: leave without the HIP runtime's own exit handlers (unloading
    // code objects, closing the device: tens of ms that produce nothing).  MGM_HIP_ORDERLY_EXIT=1 keeps them.
    fflush(stdout);
    fflush(stderr);
    if (!j.p.orderly_exit) _exit(j.rc);
    return j.rc;
}

// ---- RESIDENT MODE: `mgm --batch FILE` (FILE = - : stdin) ---------------------------------------------------------------
// Every non-empty line of FILE is one command line of this program without its name -- options, u, v, out [cost
// [backflow]] -- and all of them run in THIS process, on one device context: HIP start-up (~0.1 s) and the allocation of
// the tens of GB of workspace are paid once.  Per job, stdout and every output file are what the one-shot command writes
// (the environment parameters are the process's, the same for all lines).  A `#` at the start of a token starts a comment.
// The stages of consecutive jobs overlap: job n+1 (and n+2) is decoded, and job n-1 encoded, while job n is on the
// device; stdout keeps the order of the lines.  Exit code: 0 if every line succeeded, else 1 (the remaining lines still
// run: a failing job -- unreadable input, bad option, device-side refusal, unwritable output -- fails alone).
static int run_batch(const char *file)
{
    FILE *f = strcmp(file, "-") ? fopen(file, "r") : stdin;
    if (!f) {
        fprintf(stderr, "mgm: --batch: cannot open %s\n", file);
        return 1;
    }
    std::vector<std::unique_ptr<Job>> jobs;
    std::vector<size_t> lineno;
    {
        char *buf = nullptr;
        size_t cap = 0, ln = 0;
        ssize_t n;
        while ((n = getline(&buf, &cap, f)) >= 0) {  // (lines of any length)
            ln++;
            std::unique_ptr<Job> j(new Job);
            j->tok.push_back("mgm");
            const std::string l(buf, (size_t)n);
            size_t i = 0;
            while (i < l.size()) {
                while (i < l.size() && strchr(" \t\r\n", l[i])) i++;
                size_t k = i;
                while (k < l.size() && !strchr(" \t\r\n", l[k])) k++;
                if (k > i && l[i] == '#') break;  // a comment: only where a token starts (a '#' inside a path is part of it)
                if (k > i) j->tok.push_back(l.substr(i, k - i));
                i = k;
            }
            if (j->tok.size() > 1) {
                jobs.push_back(std::move(j));
                lineno.push_back(ln);
            }
        }
        free(buf);
    }
    if (f != stdin) fclose(f);
    const size_t N = jobs.size();
    for (auto &j : jobs) j->p = mgm_cli::plan_job(j->tok, getenv);  // (every line with the process's environment)

    // the decoder works at most AHEAD jobs ahead of the device stage (each decoded pair holds its images in memory)
    constexpr size_t AHEAD = 2;
    std::mutex mu;
    std::condition_variable cv;
    size_t decoded = 0, on_device = 0, to_write = 0, written = 0;  // jobs [0, decoded) are decoded; the device stage is at job on_device; [0, to_write) may be written; [0, written) are
    //  a line may consume what an earlier line produces (coarse-to-fine: the -m/-M range images of line k written by line k - 1):
    // the decoder then waits for the writer -- needs[k] = how many jobs must have been WRITTEN before job k's inputs are read
    std::vector<size_t> needs(N, 0);
    for (size_t k = 0; k < N; k++) {
        const JobPlan &j = jobs[k]->p;
        for (size_t m = 0; m < k; m++) {
            const JobPlan &e = jobs[m]->p;
            for (const std::string *in : {&j.f_u, &j.f_v, &j.min_file, &j.max_file})
                for (const std::string *out : {&e.f_out, &e.f_cost, &e.f_back, &e.nolr_file, &e.conf_file, &e.votes_file, &e.energy_map})
                    if (!in->empty() && *in == *out) needs[k] = m + 1;
        }
    }
    std::thread decoder([&] {
        for (size_t k = 0; k < N; k++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return k < on_device + 1 + AHEAD && written >= needs[k]; });
            }
            decode_job(*jobs[k]);
            {
                std::lock_guard<std::mutex> lk(mu);
                decoded = k + 1;
            }
            cv.notify_all();
        }
    });
    int bad = 0;
    std::thread writer([&] {
        for (size_t k = 0; k < N; k++) {
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return k < to_write; });
            }
            Job &j = *jobs[k];
            encode_job(j);
            if (j.rc != 0) {
                fprintf(stderr, "mgm: --batch: line %zu failed\n", lineno[k]);
                std::lock_guard<std::mutex> lk(mu);
                bad = 1;
            }
            // the job is done: its images go
            j.u = j.v = j.rlo = j.rhi = j.outoff = j.outcost = j.syn = j.nolr = j.conf = j.votes = j.energy = HostImg();
            {
                std::lock_guard<std::mutex> lk(mu);
                written = k + 1;
            }
            cv.notify_all();
        }
    });
    Session S;
    S.resident = true;
    for (size_t k = 0; k < N; k++) {
        Job &j = *jobs[k];
        {
            std::lock_guard<std::mutex> lk(mu);
            on_device = k;
        }
        cv.notify_all();
        if (!ends_early(j)) {
            Stopwatch sw(j.p);
            j.rc = device_job(S, j, [&] {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return decoded > k; });
            }, sw);
            sw.report("resident job, device stage");
        }
        fflush(stdout);
        {
            std::lock_guard<std::mutex> lk(mu);
            to_write = k + 1;
        }
        cv.notify_all();
    }
    {
        std::lock_guard<std::mutex> lk(mu);
        on_device = N;
    }
    cv.notify_all();
    decoder.join();
    writer.join();
    return bad;  // (the process leaves through _exit: no teardown)
}

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "--batch")) {
        const int r = run_batch(argv[2]);
        fflush(stdout);
        fflush(stderr);
        _exit(r);  // (as the one-shot run: without the HIP runtime's exit handlers)
    }
    return run_one(argc, argv);
}
