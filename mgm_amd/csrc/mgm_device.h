// mgm_device.h -- shared host/device declarations of libmgm_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mgm_fillplan.h"  // c8_supported, padded_labels
#include "mgm_geom.h"  // kMaxDirs, kMaxBatch, kMaxBands, kCensusMaxWords, PassGeom, the pass table

namespace mgm {

constexpr int kMaxLPL = 32;          // disparities per lane of the fast kernels -> L <= 2048 (the fastest stop at 8: 512 labels)
constexpr int kMaxLabels = 1 << 22;  // (index arithmetic; the reference's Dvec has no limit, dvec.cc:60) beyond 2048 labels: the generic
                                     // kernels (mgm_pass_exact.hip, k_wta_any); FH beyond 8192: convolution arrays in global scratch
constexpr int kWave = 64;            // CDNA wavefront

struct PassVolume {
    const float *C;     // [npix][L]
    const uint8_t *C8;  // [npix][L] compact costs, PassParams::cbytes bytes each (integers, all-ones = +INF: c8_encode /
                        // c16_encode) or nullptr (all volumes alike)
    float *Lr;          // NDIR volumes, pass p at Lr + (p - pass0)*nvol
    const float *w8;    // 8 planes [npix] or nullptr (all volumes alike)
    const float *rlo, *rhi;  // ragged volume: per-pixel range images (only the weighted FH kernels read them), or nullptr
    // two-valued weights (k_pass2, W2): one selector word per pixel, bit p = "the weight of plane p is not 1" (k_wsel), and
    // the penalties scaled by the other value a: P1*a, P2*a (P2*a = +INF where the cap cannot bind, like PassParams::P2)
    const unsigned *wsel;
    float p1a, p2a;
};
struct PassParams {
    PassVolume vol[kMaxBatch];
    float *hand;        // hand-off slabs  [volume*8 + pass][2][LLmax][NS*LP]; the kernels with self-validating slabs (k_pass2,
                        // TAGS): [volume][pass: g.hand_base][band][LL][LP], every slot written once per launch
    long long hand_vstride;   // ... slabs per volume (group)
    unsigned hand_tag[kMaxDirs];  // ... per pass, the tag of this launch: sign bit every handed-over word carries (0 or 0x80000000).
                              // A pass's slots are written once per launch OF THAT PASS, so the tag alternates per pass
                              // (direction-sharded callers launch the passes of one volume one at a time)
    float *handm;       // hand-off minima [volume*8 + pass][2][LLmax]
    unsigned *prog;     // progress words  [volume*8 + pass][maxbands]
    unsigned *ticket;   // work-item ticket counter
    unsigned *err;      // watchdog word
    const int2 *tasks;  // ticket -> (volume*8 + pass, band + (strip << 16) + (plain hand-off << 24)); tasks[-8 .. -1]: the
                        // XCD queues (first ticket, count) of an xcdq launch
    unsigned *qticket;  // xcdq: the eight queues' ticket counters + the count of workgroups that have left
    int xcdq;                 // 1: per-XCD work queues (k_pass2, XCDQ)
    int subv;                 // volumes per wave (1; 2 at 128 labels, 4 at 64: k_pass2<..., SUBV>); work items then address groups of volumes
    int wg_per_cu;            // 1 or 2 workgroups per compute unit (second build; plan_dense)
    int deep;                 // 1: the build with deeper DMA rings (k_pass2, DEEP; compact unweighted kernels)
    int oneb;                 // 1: the queue kernels built for one band per CU (k_pass2, ONEB: no 64-VGPR cap)
    int cbytes;               // bytes per compact cost of PassVolume::C8 (1 or 2)
    int xflags;               // development experiments (MGM_HIP_XFLAGS): 1 skip Lr stores, 2 skip C DMA, 4 ignore
                              // inter-band waits, 8 skip step barriers, 16 Lr stores into a cache-resident window (-DMGM_P2_XFLAG16 builds only); all of them need a -DMGM_P2_DEV=1 build
    unsigned long long *dbg;  // nullptr, or 8 words per ticket of timing diagnostics (MGM_HIP_DEBUG_STATS)
    unsigned long long tl_addr;  // device address of 8 words per ticket: the queue kernels' timeline (-DMGM_P2_TIMELINE=1 builds; MGM_HIP_TIMELINE)
    int tl_on;                   // ... 1: record it
    long long min_k;    // 0: no chunk minima.  Else the compute waves of k_pass2 (CHMIN) store, per pass, pixel and chunk of 32 labels, the
                        // minimum of Lr over the chunk -- one float per 32 of the Lr workspace, at (index of the chunk's first Lr
                        // float) / 32: the word of the chunk whose LAST 16 bytes start at byte address A is at (A >> 5) + min_k,
                        // min_k = minima - (workspace >> 5) - 3 for a 32-byte aligned workspace
    long long npix, nvol;
    int L, MGM, NDIR, dmin;
    int fh2_ragged;     // 1: FH, TSGM = 2, no weights, ragged volume: update_cost2_trunclinear with its boundary fix-up
    int Lreal;          // labels that exist (<= L): a label count the second build does not take runs padded to L with +INF costs
    int pass0;          // pass p writes its Lr volume to slot p - pass0
    int LLmax, maxbands;
    float P1, P2;
    PassGeom g[kMaxDirs];
};

struct WtaParams {
    const float *C;
    const uint8_t *C8;  // compact copy of C (see PassParams) or nullptr
    int cbytes;         // bytes per compact cost (1 or 2)
    const float *Lr;    // NDIR volumes
    float *S;           // nullptr or corrected volume out
    float *out, *outcost;
    long long npix, nvol;
    int L, NDIR, FIX, dmin, refine;  // refine: 0 none, 1 vfit
    int Lreal;                       // labels that exist (<= L, the stride of C / C8 / Lr); S is written with stride Lreal
    // mgm() called with range images narrower or wider than the volume's own range (mgm.cc:377-388, every TSGM_ITER
    // iteration after the first): the winner is sought among the disparities [(int)wlo, (int)whi] of each pixel; a
    // disparity of that window outside the volume holds S = 0 - (NDIR-1)*INF (0 without the over-count fix).
    const float *wlo, *whi;          // nullptr: the whole range
    // ragged C (CostParams::rlo/rhi): a disparity outside the pixel's own range does not exist in C either
    const float *clo, *chi;
    int num_cu;                      // compute units of the device (grid sizing)
    // the pruned search (k_wta_pruned): per pass, pixel and chunk of 32 labels the minimum of Lr over the chunk, written by the pass
    // kernel (PassParams::min_k) -- word (p * nvol + pix * L) / 32 + chunk --, or nullptr: the plain search
    const float *Lmin;
    unsigned long long *stats;       // nullptr, or 64 words 128 bytes apart the pruned search's waves add (pixels << 32 | chunks loaded) to
};

// the right view's winner search over the left run's Lr volumes (k_wta_right, mgm_wta.hip)
struct WtaRightParams {
    const float *C;      // costs of the left volume, label stride Lk (read with the over-count fix only) ...
    const uint8_t *C8;   // ... or their compact copy, cbytes bytes per cost
    int cbytes;
    const float *Lr;     // NDIR volumes [ny*nx][Lk], pass p at Lr + p*nvol
    float *out, *outcost;  // [ny][vnx]
    long long nvol;
    int nx, ny, vnx;
    int L, Lk;           // labels that exist, label stride (>= L)
    int NDIR, FIX, dmin, dmax, refine;  // refine: 0 none, 1 vfit
    int num_cu;
    int seg, ring;       // set by the launcher: right pixels per workgroup, entries of the LDS ring
};
struct WtaChoice;  // (mgm_planner.h: what plan_wta / plan_wta_right decided)
struct WtaRightChoice;
hipError_t launch_wta_right(const WtaRightParams &p, const WtaRightChoice &c, hipStream_t s);

// the runner-up search over the same Lr volumes (k_wta_runnerup, mgm_wta.hip): per pixel the winner of the plain
// search and the first strict minimum among the finite entries more than `radius` labels away from it
struct WtaRunnerupParams {
    const float *C;      // costs, label stride Lk (read with the over-count fix only) ...
    const uint8_t *C8;   // ... or their compact copy, cbytes bytes per cost
    int cbytes;
    const float *Lr;     // NDIR volumes [npix][Lk], pass p at Lr + p*nvol
    float *out2, *cost2;  // [npix] the runner-up's label and S there (NaN, +INF: none)
    float *out1, *cost1;  // [npix] the winner's, unrefined; each may be nullptr
    long long npix, nvol;
    int L, Lk;           // labels that exist, label stride (>= L)
    int NDIR, FIX, dmin;
    int radius;          // 0 .. L (the host clamps: at L no entry is far enough from any winner)
};
struct RunnerupChoice;  // (mgm_planner.h: what plan_wta_runnerup decided)
hipError_t launch_wta_runnerup(const WtaRunnerupParams &p, const RunnerupChoice &c, hipStream_t s);
// conf = 1 - cost1 / cost2, out = conf < ratio ? NaN : d (mgm_post.hip); out and conf may each be nullptr, out may be d
hipError_t launch_uniqueness(const float *d, const float *cost1, const float *cost2, long long n, float ratio, float *out, float *conf,
                             hipStream_t s);

// the consensus votes over the same Lr volumes, each taken alone (mgm_consensus.hip): per pixel and pass the first
// strict minimum among the finite entries the pixel owns, and how many of those winners lie within tol of the map d.  No costs.
struct WtaConsensusParams {
    const float *Lr;         // NDIR volumes [npix][Lk], pass p at Lr + p*nvol
    const float *d;          // [npix] the map to judge, in labels; nullptr with votes == nullptr
    float *votes;            // [npix] or nullptr
    float *winners;          // [NDIR][npix] or nullptr: (float)(w_p + dmin), NaN without a winner
    const float *rlo, *rhi;  // a ragged volume on its dense hull: the pixel owns [(int)rlo, (int)rhi] inside the volume; else nullptr
    const int *rec;          // the range-proportional layout: [npix][4] records (disparity of slot 0, lowest, highest, 0); Lk = L = slots
    long long npix, nvol;
    int L, Lk;               // labels that exist, label stride (>= L)
    int NDIR, dmin;
    float tol;
};
struct ConsensusChoice;  // (mgm_planner.h: what plan_wta_consensus decided)
hipError_t launch_wta_consensus(const WtaConsensusParams &p, const ConsensusChoice &c, hipStream_t s);
// out = votes < (float)minvotes ? NaN : d (mgm_post.hip); out may be d
hipError_t launch_consensus_filter(const float *d, const float *votes, long long n, int minvotes, float *out, hipStream_t s);

// the speckle filter (mgm_speckle.hip): connected components of the finite pixels under |d(p) - d(q)| <= maxdiff on
// 4-neighbours; out = NaN on the components of at most maxsize pixels, size_map = the size of every pixel's component
struct SpeckleParams {
    const float *d;    // [nx*ny] the map (out may be d: k_speckle_apply reads d[p] before it writes out[p])
    float *out, *size_map;  // each may be nullptr
    int *parent, *cnt;      // the scratch planes, nx*ny int32 each; every word of both is written by k_speckle_local
    int nx, ny, maxsize;
    float maxdiff;
};
struct SpeckleChoice;  // (mgm_planner.h: what plan_speckle decided)
enum SpecklePhase { kSpeckleLocal = 0, kSpeckleSeams, kSpeckleCount, kSpeckleApply, kSpecklePhases };
const char *speckle_phase_name(int phase);  // "k_speckle_local", ...
hipError_t launch_speckle_phase(int phase, const SpeckleParams &p, const SpeckleChoice &c, hipStream_t s);

// solution energy (mgm_energy.hip): per pixel the cost of the map's label plus edge terms over its neighbours --
// the reference's evaluate_energy_4connected (kinds 0-2) or the pairwise functional of the run (kind 3) -- into E and / or into one
// fp64 partial per block of kEnergyThreads pixels
struct EnergyParams {
    const float *d;  // [nx*ny] the map
    float *E;        // [nx*ny] the energy map, or nullptr
    void *partials;  // [blocks][4] 8-byte words: data, smooth, total (fp64), finite pixels (uint64); or nullptr
    const float *w8;  // kind 3: [8][nx*ny] weights, or nullptr (ones)
    // the copy of the volume that is read (plan_energy_copy): `stride` cost slots per pixel of `cb` bytes (4: floats; 1 / 2: codes)
    const void *cost;
    const int *records;      // range-proportional copy: four ints per pixel (disparity of slot 0, lo, hi, 0); else nullptr
    const float *rlo, *rhi;  // ragged volume: the range images a pixel owns its labels by; else nullptr
    int cb, stride, dmin, L;
    int nx, ny, kind, connectivity, use_fh;
    float P1, P2;
};
hipError_t launch_energy(const EnergyParams &p, long long blocks, hipStream_t s);

// hole filling (mgm_holes.hip): per hole (a non-finite pixel) the nearest finite pixel along each of `dirs` rays of
// the ORIGINAL map, at most maxdist steps away (0: any); out = their median / minimum / maximum, filled = 1 where a hole got a value
struct HolesParams {
    const float *d;       // [nx*ny] the map (out may be d: k_holes_apply reads d[p] before it writes out[p], the candidates are finished)
    float *out, *filled;  // each may be nullptr
    float *planes;        // scratch: `dirs` candidate planes of nx*ny floats, plane k written at every hole by direction k (NaN: none)
    int *cpos;            // scratch: the bands' carry-outs of directions 2.., [direction - 2][band][line]: the row of the band's last
    float *cval;          //          finite pixel in walking order on that line (-1: none) and its value
    int nx, ny, dirs, maxdist;
    int mode;             // 0 median (upper), 1 min, 2 max; with cls also 3 seclow, 4 sechigh
    // the classified fill: nullptr, or [nx*ny] classes -- a hole with cls == 1 takes mode_occ, every other hole `mode`
    const float *cls;
    int mode_occ;
};
struct HolesChoice;  // (mgm_planner.h: what plan_holes decided)
enum HolesPhase { kHolesRows = 0, kHolesCarry, kHolesWalk, kHolesApply, kHolesPhases };
const char *holes_phase_name(int phase);  // "k_holes_rows", ...
// dirs = 2 has no columns and no diagonals: its carry and walk phases launch nothing (the caller skips them: holes_phase_runs)
inline bool holes_phase_runs(int phase, int dirs) { return dirs > 2 || (phase != kHolesCarry && phase != kHolesWalk); }
hipError_t launch_holes_phase(int phase, const HolesParams &p, const HolesChoice &c, hipStream_t s);
// hole classification (k_holes_classify, mgm_holes.hip): cls = 0 on finite pixels, 2 on the holes that a pixel of the
// other view's row points back at within tau (a mismatch), 1 on the other holes (an occlusion)
struct HolesClassifyParams {
    const float *d;      // [nx*ny] the map with holes
    const float *other;  // [vnx*ny] the other view's map as it went into the left-right test
    float *cls;          // [nx*ny]
    int nx, ny, vnx, dmin, dmax;
    float tau;
};
struct HolesClassifyChoice;  // (mgm_planner.h: what plan_holes_classify decided)
hipError_t launch_holes_classify(const HolesClassifyParams &p, const HolesClassifyChoice &c, hipStream_t s);

// sub-pixel label spacing (mgm_subpix.hip): the phase image v_k of v at the shift k/s (k_subpix_phase), the fine
// volume gathered from the s phase volumes (k_cv_interleave), and the maps' rescale out = in / s (k_scale_map; out may be in)
enum SubpixInterp { kSubpixLinear = 0, kSubpixCubic };
hipError_t launch_subpix_phase(const float *v, int vnx, long long nrows, int s, int k, int interp, float *out, hipStream_t st);
struct SubpixParams {
    const void *phase[4];  // the s phase volumes [npix][in_slots], all in one form: one-byte codes (cb = 1) or fp32 (cb = 4)
    void *F;               // [npix][slots] in that form; F(p, o') = phase[o' % s](p, o' / s) for o' < labels, the code of +INF beyond
    long long npix;
    int labels, slots, in_slots, s, cb;
};
struct SubpixChoice;  // (mgm_planner.h: what plan_subpix decided)
hipError_t launch_cv_interleave(const SubpixParams &p, const SubpixChoice &c, hipStream_t st);
hipError_t launch_scale_map(const float *in, long long n, int s, float *out, hipStream_t st);

// ---- ragged volumes in the range-proportional layout (mgm_pass_rel.hip, k_wta_rel): 64 label slots per pixel placed at the
// pixel's own window, slot k <-> disparity base + k
struct RelVolume {
    const uint8_t *c8;       // [npix][slots] cost codes of cb bytes (all ones = +INF: the slot is not a disparity of the pixel, or its cost is +INF)
    const int *base;         // [npix][4] the pixel's record: disparity of slot 0 (= its lowest disparity - 1), lowest, highest, 0
    const float *rlo, *rhi;  // [npix] the pixel's own range (the volume's range images)
    float *Lr;               // NDIR volumes [npix][slots], pass p at Lr + (p - pass0)*nvol
    const float *w8;         // 8 planes [npix] or nullptr
};
struct RelParams {
    RelVolume vol[kMaxBatch];
    float *hand;        // self-validating hand-off slots [volume][pass: g.hand_base][band][LL][NS*64 + 4]: slab(s), minimum, base + bias, padding;
                        // every word of a slot carries the launch's tag in its sign bit (mgm_pass_rel.hip)
    long long hand_vstride;  // slots per volume
    unsigned tag;       // 0 or 0x80000000
    unsigned *ticket, *err;
    const int2 *tasks;  // ticket -> (volume*8 + pass, band)
    long long npix, nvol;
    int MGM, NDIR, pass0, LLmax, maxbands, weighted;
    int ld;             // steps of LDS-DMA the loader keeps in flight (2..5; every step of lead is a step of lag per band)
    int slots, cb;      // the volumes' range-proportional format: 64 or 128 label slots per pixel, 1 or 2 bytes per cost (round 6)
    int fh2;            // FH potentials, TSGM = 2, no weights: update_cost2_trunclinear with its boundary fix-up (k_pass_rel, FH2)
    int cost2;          // TSGM = 2 without weights, Hirschmueller: update_cost2's association (every term halved before the sum)
    int fh_multi;       // FH: the pixel's TSGM min-convolutions side by side (k_pass_rel<true, false, TSGM>) instead of one after the other
    int diag_any;       // some pass of the launch walks anti-diagonals (g.diag): the workgroups carry a second hand ring
    float P1, P2;
    unsigned long long *tl;  // nullptr, or 8 words per work item (MGM_HIP_TIMELINE; tools/timeline.py): start, end, waited, slow paths, where, steps, polls
    PassGeom g[kMaxDirs];
};
hipError_t launch_rel_gather(const float *C, const float *rlo, const float *rhi, long long npix, int L, int dmin, int slots, int cb, uint8_t *rel8, int *relb,
                             unsigned *flag, hipStream_t s);
hipError_t launch_cost_census_rel(const uint32_t *cu, const uint32_t *cv, int nx, int ny, int vnx, int vny, int dmin, int L, float trunc, const float *rlo,
                                  const float *rhi, int slots, uint8_t *rel8, int *relb, unsigned *flag, hipStream_t s);
hipError_t launch_rel_expand(const uint8_t *rel8, const int *relb, long long npix, int L, int dmin, int slots, int cb, float *C, hipStream_t s);
struct PassKernelChoice;  // (mgm_planner.h: the instance plan_dense / plan_rel chose)
hipError_t launch_pass_rel(const RelParams &p, const PassKernelChoice &c, int ntasks, hipStream_t s);
int pass_rel_phases();  // words per work item of phase clocks behind the timeline words (0: not a -DMGM_REL_PHASES=1 build)
struct WtaRelParams {
    const uint8_t *c8;
    const int *base;
    const float *rlo, *rhi;
    const float *Lr;
    const float *wlo, *whi;  // nullptr: the window is the pixel's own range
    float *out, *outcost;
    long long npix, nvol;
    int NDIR, FIX, refine;   // refine: index into the reference's table (0 none, 1 vfit, 2 parabola, 3 cubic, 4 parabolaOCV)
    int num_cu;
    int slots, cb;           // the volume's range-proportional format
};
hipError_t launch_wta_rel(const WtaRelParams &p, hipStream_t s);
hipError_t launch_rel_S(const WtaRelParams &p, int L, int dmin, float *S, hipStream_t s);  // the corrected S on the dense hull from the range-proportional Lr volumes

// the slow, operand-order-faithful pass kernel (mgm_pass_exact.hip): one pass of one volume
struct ExactPass {       // one pass of the reference's table (mgm_core.cc:463-471, 481-484)
    float *Lr;           // this pass's volume [npix][L]: written whole by the launch (a pixel that is not updated keeps C, 495-498)
    int d[4][2];         // neighbour offsets
    int wplane[4];       // weight plane of neighbour k
    int inc_x, inc_y, row_major;
    int jj0, njj;        // this launch: first jj of the diagonal that lies inside the image, and how many
};
struct ExactParams {
    const float *C;      // [npix][L]
    float *mins;         // [npass][npix] slab minima of the pixels visited so far
    float *fhscratch;    // FH potentials with more than 8192 labels: npass x max(nx, ny) x 4 x L floats (the convolution arrays of a
                         // diagonal's pixels, which fit the LDS up to 8192 labels), else unused
    const float *w8;     // 8 planes or nullptr
    const float *rlo, *rhi;  // ragged volume: per-pixel range images, or nullptr
    int nx, ny, L, dmin;
    float P1, P2;
    int MGM, mode;       // mode: 0 update_cost2, 1 update_costW, 2 update_cost2_trunclinear, 3 update_costW_trunclinear
    int npass;           // passes of this launch: blockIdx.y (round 6: the passes are independent -- one launch per DIAGONAL serves them all)
    int ii;              // diagonal
    ExactPass pass[kMaxDirs];
};
hipError_t launch_pass_exact(const ExactParams &p, hipStream_t s);

// launchers (one per translation unit)
hipError_t launch_pass(const PassParams &p, const PassKernelChoice &c, int ntasks, hipStream_t s);
int pass_ns(bool fh, bool weighted);  // slabs per hand-off slot
int pass_lpl(int L);                  // disparities per lane the pass kernel is instantiated for
// second build (LDS-DMA loader waves); pass2_lines(L) = lines per band, 0 if L is not supported by it
int pass2_lines(int L, bool c8);
bool pass2_devtools();  // built with -DMGM_P2_DEV=1 (MGM_HIP_DEBUG_STATS / MGM_HIP_XFLAGS are honoured)
bool pass2_timeline();  // built with -DMGM_P2_TIMELINE=1 (MGM_HIP_TIMELINE is honoured)
hipError_t launch_pass2(const PassParams &p, const PassKernelChoice &c, int ntasks, hipStream_t s);
template <int LPL>
hipError_t launch_pass2_lpl(const PassParams &p, const PassKernelChoice &c, int ntasks, hipStream_t s);
hipError_t launch_compact(const float *C, long long n, uint8_t *C8, int cbytes, unsigned *bad8, hipStream_t s);
hipError_t launch_nanscan(const float *C, long long n, unsigned *flag, hipStream_t s);
hipError_t launch_pad(const float *C, long long npix, int L, int LP, float *Cp, uint8_t *C8p, int cbytes, unsigned *bad8, hipStream_t s);
hipError_t launch_expand(const uint8_t *C8, int cbytes, long long n, float *C, hipStream_t s);
hipError_t launch_expand_padded(const uint8_t *C8, int cbytes, long long npix, int L, int LP, float *C, hipStream_t s);
hipError_t launch_wta(const WtaParams &p, const WtaChoice &c, hipStream_t s);
long long tune_num(const char *key, long long dflt);  // development switches (MGM_HIP_TUNE; mgm_ctx.hip)
hipError_t launch_median(const float *u, int nx, int ny, int nch, int radius, float *out, hipStream_t s);
hipError_t launch_leftright(const float *dx, int nc, int nr, const float *Rdx, int Rnc, float threshold, float *out,
                            hipStream_t s);
hipError_t launch_backproject(const float *u, int nx, int ny, int nch, const float *v, int vnx, int vny, const float *disp,
                              float *out, hipStream_t s);
hipError_t launch_refine(const float *S, long long npix, int L, int dmin, int method, const float *wlo, const float *whi,
                         float vout, float *out, float *outcost, hipStream_t s);
hipError_t launch_update_ranges(const float *outoff, int nx, int ny, int slack, int radius, float *dminI, float *dmaxI,
                                float *scratch2, hipStream_t s);
hipError_t launch_minmax(const float *u, long long n, unsigned *mm, hipStream_t s);
// mgm_pyramid.hip: the resampling steps of the coarse-to-fine driver ("multiscale")
hipError_t launch_zoom_out(const float *in, int nx, int ny, int nch, float *out, hipStream_t s);
hipError_t launch_ranges_zoom_out(const float *lo, const float *hi, int nx, int ny, float *lo2, float *hi2, hipStream_t s);
hipError_t launch_ranges_from_coarse(const float *coarse, int nx, int ny, int slack, int radius, const unsigned *mm, float *lo,
                                     float *hi, int *hull, hipStream_t s);
hipError_t launch_ranges_hull(const float *lo, const float *hi, long long n, int *hull, hipStream_t s);
hipError_t launch_fill(float *p, long long n, float value, hipStream_t s);
hipError_t launch_census(const float *u, int nx, int ny, int nch, int winradius, uint32_t *out, hipStream_t s);
struct CostParams {
    const float *u, *v;          // planar images (float, or census words reinterpreted)
    const uint32_t *cu, *cv;     // census words (planar) when prefiltered
    float *C;
    uint8_t *C8;                 // compact copy, written alongside C
    int cbytes;                  // its bytes per cost (1 or 2)
    unsigned *bad8;              // set to 1 if some cost is not representable in the compact form
    int nx, ny, vnx, vny, nch;   // nch = channels of the (prefiltered) images
    int dmin, L;
    int Lreal;                   // k_cost_diffx / k_cost_census8*: the label slots Lreal..L-1 of the (padded) layout get +INF; else = L
    int costfn;                  // 0 ad, 1 sd, 2 census, 3 ncc, 4 btad, 5 btsd
    int hwin;                    // ncc: half window (CENSUS_NCC_WIN / 2)
    float trunc;                 // truncDist * nch
    // ragged volume (per-pixel ranges from range images, mgm_costvolume.h:276-299, 323): pixel p only has the
    // disparities [(int)rlo(p), (int)rhi(p)]; the others are +INF in the dense layout and exempt from the
    // "no finite cost => zeros" rule.  nullptr: every pixel has the whole range.
    const float *rlo, *rhi;
    // ncc: scratch for the per-pixel window statistics of the two images (k_ncc_stats): (2*nch + 1) planes of nx*ny /
    // vnx*vny floats each -- mean and variance term per channel, then the "window inside the image and NaN-free" flag --
    // or nullptr (the general kernel recomputes every window for every label).  Birchfield-Tomasi costs: the two ends of the
    // interval every sample spans (k_bt_spans), 2*nch planes per image.
    float *ncc_u, *ncc_v;
};
// the instance plan_cost_kernel (mgm_fillplan.h) chose for the volume `p` describes (mgm_cost_fast.hip: a table that decides nothing)
hipError_t launch_cost(const CostParams &p, const CostKernelChoice &k, hipStream_t s);
hipError_t launch_cost_general(const CostParams &p, unsigned grid, hipStream_t s);  // (mgm_cost.hip; called by launch_cost)
hipError_t launch_filter2d(const float *u, int nx, int ny, int nch, const float *taps, int fnx, int fny, float *out,
                           hipStream_t s);
hipError_t launch_weights(const float *u, int nx, int ny, int nch, float aP, float aThresh, float *w8,
                          hipStream_t s);
hipError_t launch_selftest_div3(unsigned long long *nbad, hipStream_t s);
hipError_t launch_any_not_one(const float *w, long long n, unsigned *flag, hipStream_t s);
// what values do the weights take?  out[0] = 1 if some weight is not 1.0; out[1], out[2] = smallest and largest bit pattern
// among the weights that are not 1.0 and are positive finite floats; out[3] = 1 if some weight is neither (negative, 0, NaN, INF)
hipError_t launch_weight_values(const float *w, long long n, unsigned *out4, hipStream_t s);
// selector words of two-valued weights: sel[p] bit k = (w[k*npix + p] != 1.0f), k = 0..7
hipError_t launch_wsel(const float *w8, long long npix, unsigned *sel, hipStream_t s);
// ... and which of the two transforms of a pixel anybody reads: out[q] = sel[q] | need << 8 (k_wneed; d[pass][k] = neighbour offsets
// of the reference's pass table, plane[pass][k] = their weight planes)
hipError_t launch_wneed(const unsigned *sel, int nx, int ny, int MGM, const int (*d)[4][2], const int (*plane)[4], unsigned *out, hipStream_t s);
hipError_t launch_probe_streams(float *base, long long stride, int nstreams, long long floats_per_stream, hipStream_t s);
hipError_t launch_check_tags(const float *slabs, long long nwords, unsigned tag, unsigned *count, hipStream_t s);
hipError_t launch_xcc_census(unsigned *mask, hipStream_t s);

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ float f_inf() { return __builtin_huge_valf(); }
__device__ __forceinline__ bool finite_bits(float x)
{
    return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) != 0x7f800000u;
}
// floats ordered through their bit patterns, so that integer atomics can reduce them (k_minmax, k_wta_right's keys)
__device__ __forceinline__ unsigned f2ord(float f)
{
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned o)
{
    return __builtin_bit_cast(float, (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// Compact cost: an fp32 cost that is an integer in [0, 254] or +INF is stored as one byte
// (255 = +INF).  Census costs with one descriptor word and AD costs of 8-bit images qualify; the
// conversion back is exact.  Returns 256 if x is not representable.
__device__ __forceinline__ unsigned c8_encode(float x)
{
    if (x == __builtin_huge_valf()) return 255u;
    const float r = __builtin_rintf(x);
    const bool neg0 = __builtin_bit_cast(unsigned, x) == 0x80000000u;  // -0 would come back as +0
    return (x >= 0.0f && x <= 254.0f && r == x && !neg0) ? (unsigned)r : 256u;
}
__device__ __forceinline__ float c8_decode(unsigned b) { return b == 255u ? __builtin_huge_valf() : (float)b; }
// The same with TWO bytes per cost (round 4): integers in [0, 65534] or +INF (65535) -- absolute differences summed over
// the channels of a colour pair (up to 765), squared differences of one channel (up to 65025).  Returns 65536 if x is not
// representable.  cb = bytes per compact cost (1 or 2) picks between the two forms.
__device__ __forceinline__ unsigned c16_encode(float x)
{
    if (x == __builtin_huge_valf()) return 65535u;
    const float r = __builtin_rintf(x);
    const bool neg0 = __builtin_bit_cast(unsigned, x) == 0x80000000u;
    return (x >= 0.0f && x <= 65534.0f && r == x && !neg0) ? (unsigned)r : 65536u;
}
__device__ __forceinline__ float c16_decode(unsigned h) { return h == 65535u ? __builtin_huge_valf() : (float)h; }

// DPP lane shifts over the whole wave (gfx9 wave_shr / wave_shl).
// shr1: lane l receives lane l-1 (lane 0 gets `fill`).
__device__ __forceinline__ float dpp_shr1(float v, float fill)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill),
                                                                 __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
// shl1: lane l receives lane l+1 (lane 63 gets `fill`).
__device__ __forceinline__ float dpp_shl1(float v, float fill)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill),
                                                                 __builtin_bit_cast(int, v), 0x130, 0xf, 0xf, false));
}
// generic DPP move: lanes without a source (row edge / masked row) receive `fill`
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_mov(float v, float fill)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, fill),
                                                                 __builtin_bit_cast(int, v), CTRL, ROWMASK, 0xf, false));
}
__device__ __forceinline__ float readlane_f(float v, int l)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// Fused DPP arithmetic, written as inline assembly: the compiler keeps a DPP move, its fill value and
// the arithmetic apart (four issue slots where one or two do), and with four waves per SIMD every
// VALU slot of the scan-line kernels costs 16 cycles of the SIMD.  The s_nop ahead of each DPP
// instruction covers the "VALU writes a VGPR, DPP reads it" hazard (2 wait states), which the
// compiler's hazard recogniser does not see through inline assembly.
//   MGM_DPP_MIN(name, ctrl):  c = min(c, t[source lane]);  lanes without a source lane keep c
//   MGM_DPP_ADD(name, ctrl):  t = c[source lane] + addend; lanes without a source lane read 0,
//                             so `addend` must be +INF there
#define MGM_DPP_MIN(name, ctrl)                                                                            \
    __device__ __forceinline__ float name(float c, float t)                                                \
    {                                                                                                      \
        asm("s_nop 1\n\tv_min_f32_dpp %0, %1, %0 " ctrl " bank_mask:0xf" : "+v"(c) : "v"(t));              \
        return c;                                                                                          \
    }
#define MGM_DPP_ADD(name, ctrl)                                                                            \
    __device__ __forceinline__ float name(float c, float addend)                                           \
    {                                                                                                      \
        float t;                                                                                           \
        asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %2 " ctrl " bank_mask:0xf bound_ctrl:0" : "=v"(t) : "v"(c), "v"(addend)); \
        return t;                                                                                          \
    }
MGM_DPP_MIN(dpp_min_row_shr1, "row_shr:1 row_mask:0xf")
MGM_DPP_MIN(dpp_min_row_shr2, "row_shr:2 row_mask:0xf")
MGM_DPP_MIN(dpp_min_row_shr4, "row_shr:4 row_mask:0xf")
MGM_DPP_MIN(dpp_min_row_shr8, "row_shr:8 row_mask:0xf")
MGM_DPP_MIN(dpp_min_row_shl1, "row_shl:1 row_mask:0xf")
MGM_DPP_MIN(dpp_min_row_shl2, "row_shl:2 row_mask:0xf")
MGM_DPP_MIN(dpp_min_row_shl4, "row_shl:4 row_mask:0xf")
MGM_DPP_MIN(dpp_min_row_shl8, "row_shl:8 row_mask:0xf")
MGM_DPP_MIN(dpp_min_bcast15, "row_bcast:15 row_mask:0xa")
MGM_DPP_MIN(dpp_min_bcast31, "row_bcast:31 row_mask:0xc")
MGM_DPP_ADD(dpp_add_bcast15, "row_bcast:15 row_mask:0xf")
MGM_DPP_ADD(dpp_add_bcast31, "row_bcast:31 row_mask:0xf")
MGM_DPP_ADD(dpp_add_wave_shr1, "wave_shr:1 row_mask:0xf")
MGM_DPP_ADD(dpp_add_wave_shl1, "wave_shl:1 row_mask:0xf")
#undef MGM_DPP_MIN
#undef MGM_DPP_ADD
// The same on NK independent values in ONE block (round 6, fh_scan_multi): one s_nop for the block, the NK DPP instructions back to
// back -- the chains of NK side-by-side scans interleave at every stage instead of running one after the other (the compiler keeps
// inline-assembly blocks in source order).
#define MGM_DPP_MIN_N(name, ctrl)                                                                                                     \
    template <int NK>                                                                                                                 \
    __device__ __forceinline__ void name(float (&c)[NK], const float (&t)[NK])                                                        \
    {                                                                                                                                 \
        static_assert(NK >= 1 && NK <= 4, "one to four chains");                                                                      \
        if constexpr (NK == 1)                                                                                                        \
            asm("s_nop 1\n\tv_min_f32_dpp %0, %1, %0 " ctrl " bank_mask:0xf" : "+v"(c[0]) : "v"(t[0]));                               \
        else if constexpr (NK == 2)                                                                                                   \
            asm("s_nop 1\n\tv_min_f32_dpp %0, %2, %0 " ctrl " bank_mask:0xf\n\tv_min_f32_dpp %1, %3, %1 " ctrl " bank_mask:0xf"      \
                : "+v"(c[0]), "+v"(c[1])                                                                                              \
                : "v"(t[0]), "v"(t[1]));                                                                                              \
        else if constexpr (NK == 3)                                                                                                   \
            asm("s_nop 1\n\tv_min_f32_dpp %0, %3, %0 " ctrl " bank_mask:0xf\n\tv_min_f32_dpp %1, %4, %1 " ctrl                       \
                " bank_mask:0xf\n\tv_min_f32_dpp %2, %5, %2 " ctrl " bank_mask:0xf"                                                   \
                : "+v"(c[0]), "+v"(c[1]), "+v"(c[2])                                                                                  \
                : "v"(t[0]), "v"(t[1]), "v"(t[2]));                                                                                   \
        else                                                                                                                          \
            asm("s_nop 1\n\tv_min_f32_dpp %0, %4, %0 " ctrl " bank_mask:0xf\n\tv_min_f32_dpp %1, %5, %1 " ctrl                       \
                " bank_mask:0xf\n\tv_min_f32_dpp %2, %6, %2 " ctrl " bank_mask:0xf\n\tv_min_f32_dpp %3, %7, %3 " ctrl                \
                " bank_mask:0xf"                                                                                                      \
                : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3])                                                                      \
                : "v"(t[0]), "v"(t[1]), "v"(t[2]), "v"(t[3]));                                                                        \
    }
#define MGM_DPP_ADD_N(name, ctrl)                                                                                                     \
    template <int NK>                                                                                                                 \
    __device__ __forceinline__ void name(float (&t)[NK], const float (&c)[NK], const float (&a)[NK])                                  \
    {                                                                                                                                 \
        static_assert(NK >= 1 && NK <= 4, "one to four chains");                                                                      \
        if constexpr (NK == 1)                                                                                                        \
            asm("s_nop 1\n\tv_add_f32_dpp %0, %1, %2 " ctrl " bank_mask:0xf bound_ctrl:0" : "=&v"(t[0]) : "v"(c[0]), "v"(a[0]));      \
        else if constexpr (NK == 2)                                                                                                   \
            asm("s_nop 1\n\tv_add_f32_dpp %0, %2, %4 " ctrl " bank_mask:0xf bound_ctrl:0\n\tv_add_f32_dpp %1, %3, %5 " ctrl          \
                " bank_mask:0xf bound_ctrl:0"                                                                                         \
                : "=&v"(t[0]), "=&v"(t[1])                                                                                            \
                : "v"(c[0]), "v"(c[1]), "v"(a[0]), "v"(a[1]));                                                                        \
        else if constexpr (NK == 3)                                                                                                   \
            asm("s_nop 1\n\tv_add_f32_dpp %0, %3, %6 " ctrl " bank_mask:0xf bound_ctrl:0\n\tv_add_f32_dpp %1, %4, %7 " ctrl          \
                " bank_mask:0xf bound_ctrl:0\n\tv_add_f32_dpp %2, %5, %8 " ctrl " bank_mask:0xf bound_ctrl:0"                         \
                : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2])                                                                               \
                : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(a[0]), "v"(a[1]), "v"(a[2]));                                                  \
        else                                                                                                                          \
            asm("s_nop 1\n\tv_add_f32_dpp %0, %4, %8 " ctrl " bank_mask:0xf bound_ctrl:0\n\tv_add_f32_dpp %1, %5, %9 " ctrl          \
                " bank_mask:0xf bound_ctrl:0\n\tv_add_f32_dpp %2, %6, %10 " ctrl                                                     \
                " bank_mask:0xf bound_ctrl:0\n\tv_add_f32_dpp %3, %7, %11 " ctrl " bank_mask:0xf bound_ctrl:0"                        \
                : "=&v"(t[0]), "=&v"(t[1]), "=&v"(t[2]), "=&v"(t[3])                                                                  \
                : "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(a[0]), "v"(a[1]), "v"(a[2]), "v"(a[3]));                            \
    }
MGM_DPP_MIN_N(dpp_min_row_shr1_n, "row_shr:1 row_mask:0xf")
MGM_DPP_MIN_N(dpp_min_row_shr2_n, "row_shr:2 row_mask:0xf")
MGM_DPP_MIN_N(dpp_min_row_shr4_n, "row_shr:4 row_mask:0xf")
MGM_DPP_MIN_N(dpp_min_row_shr8_n, "row_shr:8 row_mask:0xf")
MGM_DPP_MIN_N(dpp_min_row_shl1_n, "row_shl:1 row_mask:0xf")
MGM_DPP_MIN_N(dpp_min_row_shl2_n, "row_shl:2 row_mask:0xf")
MGM_DPP_MIN_N(dpp_min_row_shl4_n, "row_shl:4 row_mask:0xf")
MGM_DPP_MIN_N(dpp_min_row_shl8_n, "row_shl:8 row_mask:0xf")
MGM_DPP_ADD_N(dpp_add_wave_shr1_n, "wave_shr:1 row_mask:0xf")
MGM_DPP_ADD_N(dpp_add_wave_shl1_n, "wave_shl:1 row_mask:0xf")
#undef MGM_DPP_MIN_N
#undef MGM_DPP_ADD_N

// wave-wide minimum, result uniform (SGPR).  NaN-free inputs only.
__device__ __forceinline__ float wave_min(float v)
{
    v = dpp_min_row_shr1(v, v);
    v = dpp_min_row_shr2(v, v);
    v = dpp_min_row_shr4(v, v);
    v = dpp_min_row_shr8(v, v);  // lane 15 of every row: the row's minimum
    v = dpp_min_bcast15(v, v);   // rows 1 and 3 take in the row before them
    v = dpp_min_bcast31(v, v);   // rows 2 and 3 take in lane 31
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
#endif

}  // namespace mgm
