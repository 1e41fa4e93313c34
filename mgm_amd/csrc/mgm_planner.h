// mgm_planner.h -- the launch plan of the pass kernels as pure functions: everything a K3 launch is decided by goes in as a
// request of integers (DenseRequest, RelRequest), everything decided comes out as a plan (the build, the label width, wave
// sharing, workgroups per CU, deep rings, per-XCD queues, strips, the hand-off layout, the ticket order and the dealt task
// table).  Plain C++17, standard headers only: no device, no context, no environment -- mgm_plan.hip fills the requests,
// caches the plans BY the requests and launches; tests/test_planner.py runs the planner on the host.
// The winner search is planned here as well (plan_wta, plan_wta_right, plan_wta_runnerup, plan_wta_rel at the end: which
// instance, which grid, pruned or not); tests/test_wta_plan.py, tests/test_runnerup_plan.py.
// ... and the speckle filter's tile, grids and scratch (plan_speckle); tests/test_speckle_plan.py.
// ... and hole filling's chunk, band, grids and scratch (plan_holes); tests/test_holes_plan.py.
// ... and hole classification's segment, span, grid and LDS bytes (plan_holes_classify); tests/test_occlusion_model.py.
// ... and which kernels take an aggregation call at all (plan_agg_route, plan_subbatch, plan_dense_kernels behind them: pure functions
// that ASK for the facts of the device they need, one at a time); tests/test_route_plan.py.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <type_traits>
#include <utility>
#include <vector>

#include "mgm_fillplan.h"  // padded_labels
#include "mgm_geom.h"

namespace mgm {

struct Task {  // ticket -> (volume group * 8 + pass, band + (strip << 16) + (bit 24)); uploaded as int2
    int x, y;
};

// Canonical geometry of a pass (see PassGeom).  Returns false if the table
// entry does not reduce to one of the two canonical neighbour orders.
inline bool make_geom(int pass, int nx, int ny, int R, int MGM, bool slope1_ok, PassGeom &g)
{
    const RefPass &rp = kPasses[pass];
    const long long sx = rp.inc_x ? 1 : -1, sy = rp.inc_y ? 1 : -1;
    g.base = (long long)(rp.inc_y ? 0 : ny - 1) * nx + (rp.inc_x ? 0 : nx - 1);
    if (rp.row_major) {
        g.NL = ny;
        g.LL = nx;
        g.istep = sx;
        g.jstep = sy * nx;
    } else {
        g.NL = nx;
        g.LL = ny;
        g.istep = sy * nx;
        g.jstep = sx;
    }
    int kind[4];
    for (int k = 0; k < 4; k++) {
        const int dx = rp.d[k][0], dy = rp.d[k][1];
        const int di = rp.row_major ? dx * (int)sx : dy * (int)sy;
        const int dj = rp.row_major ? dy * (int)sy : dx * (int)sx;
        if (di == -1 && dj == 0) kind[k] = 0;        // inline
        else if (di == 0 && dj == -1) kind[k] = 1;   // same
        else if (di == -1 && dj == -1) kind[k] = 2;  // back
        else if (di == 1 && dj == -1) kind[k] = 3;   // fwd
        else return false;
        g.wplane[k] = kPassToChannel[k][pass];
    }
    if (kind[0] == 0 && kind[1] == 1 && kind[2] == 2 && kind[3] == 3) g.form = 0;
    else if (kind[0] == 3 && kind[1] == 2 && kind[2] == 1 && kind[3] == 0) g.form = 1;
    else return false;
    g.nbands = (g.NL + R - 1) / R;
    // form 0 sums inline, same, back, fwd: with MGM <= 3 the fwd neighbour (i+1, j-1) is never read,
    // so a line only has to stay ONE pixel behind the previous one (second K3 build only)
    g.slope = (slope1_ok && g.form == 0 && MGM <= 3) ? 1 : 2;
    g.nstrips = 1;
    g.split = g.LL;
    g.hand_base = 0;
    g.diag = 0;
    g.wmax = 0;
    g.swap = 0;
    return true;
}

// How many per-XCD work queues a launch can use on this device: the XCC ids 0 .. n-1 a 2048-workgroup launch saw
// (k_xcc_census), if they are exactly that -- 8 on an MI355X in SPX mode, fewer on a partitioned device, 0 = no queues.
inline int xcc_queues(int mask)
{
    int n = 0;
    while (n < 8 && ((mask >> n) & 1)) n++;
    return (n >= 2 && mask == (1 << n) - 1) ? n : 0;
}

// ---- requests: what a plan is a function of, and nothing else ------------------------------------------------------------
// Integer-only aggregates without padding: two requests are the same plan exactly when their bytes are equal, which is what
// the contexts' caches compare (mgm_plan.hip).  P1 / P2 are not plan inputs.
enum { kWeightsNone = 0, kWeightsTwoValued = 1, kWeightsGeneral = 2 };
struct DenseRequest {
    int nx, ny, L;             // image, label slots the kernels see (the padded count of a padded launch)
    int nb, first, count;      // volumes; passes [first, first + count) ...
    int layout_ndir;           // ... of a hand-off region laid out for the passes [0, layout_ndir)
    int MGM, fh;               // TSGM neighbours; 1: FH potentials
    int wmode;                 // kWeights*: none / 1 and one other positive value in every volume / anything else
    int use_c8, cb;            // compact costs, bytes per cost
    int first_build, ragged;   // the first build only (forced, or negative penalties); some volume has per-pixel ranges
    int lines2, lpl, ns;       // what the kernels report: pass2_lines(L * dense_subv(request), use_c8), pass_lpl(L), pass_ns(fh, weighted)
    int devtools;              // pass2_devtools(): a development build of the pass kernels
    int num_cu, xcc_mask;      // compute units; XCC ids a launch sees (k_xcc_census; -1: not looked)
    // development switches and tune values (DevSwitches, MGM_HIP_TUNE)
    int subv, deep, wg_per_cu, strips, xcdq, xcdq_k, one_queue, w2, oneb;
};
struct RelRequest {
    int nx, ny, NDIR, nb, MGM;
    int fh, pube, fh2;         // FH potentials; the producer publishes E; update_cost2_trunclinear
    int slots, cb;             // the volumes' range-proportional format
    int R, HS;                 // lines per band, floats per hand-off slot (kRelLines, rel_hand_floats)
    int diag_fits;             // a workgroup with the second hand ring of the anti-diagonal passes fits the LDS (rel_wg_lds_bytes)
    int num_cu;
    // tune values: rel_wg 0 = by the launch's shape; rel_prio as resolved by the caller (default 5 for one volume, else 0)
    // rel_multi 0: FH on 64 slots of one-byte costs runs the one-after-the-other build (an A/B switch)
    int rel_wg, rel_prio, rel_lag, rel_lagd, rel_slots, rel_slope1, rel_swap, rel_diag, rel_strips, rel_multi;
};
static_assert(std::has_unique_object_representations_v<DenseRequest>, "DenseRequest: integers only, no padding (compared bytewise)");
static_assert(std::has_unique_object_representations_v<RelRequest>, "RelRequest: integers only, no padding (compared bytewise)");
template <class Req>
inline bool same_request(const Req &a, const Req &b)
{
    return memcmp(&a, &b, sizeof(Req)) == 0;
}

// ---- the hand-off region's layout: what a region of self-validating slots was last cleared for ---------------------------
// Nothing that differs between launches which share a region: not the passes a launch runs, not its strips, not its weights.
struct HandLayout {
    int nx = 0, ny = 0;
    int npass = 0;        // passes laid out (0: no region known)
    int groups = 0;       // volume groups
    int slot_floats = 0;  // floats per slot
    int slots = 0;        // label slots per pixel of the range-proportional format (0: the dense kernels' region)
    int R = 0;
    struct Pass {
        long long hand_base;
        int nbands, lines;  // lines: slot lines per band (LL, or 2 * wmax on anti-diagonals)
        int slope, diag, swap;
    } pass[kMaxDirs] = {};
    long long per_group() const { return npass ? pass[npass - 1].hand_base + (long long)pass[npass - 1].nbands * pass[npass - 1].lines : 0; }
    bool operator==(const HandLayout &o) const
    {
        if (nx != o.nx || ny != o.ny || npass != o.npass || groups != o.groups || slot_floats != o.slot_floats || slots != o.slots || R != o.R) return false;
        for (int q = 0; q < npass; q++) {
            const Pass &a = pass[q], &b = o.pass[q];
            if (a.hand_base != b.hand_base || a.nbands != b.nbands || a.lines != b.lines || a.slope != b.slope || a.diag != b.diag || a.swap != b.swap) return false;
        }
        return true;
    }
    bool operator!=(const HandLayout &o) const { return !(*this == o); }
};
// lays the passes [0, npass) out behind each other (sets g[q].hand_base); returns the layout
inline HandLayout lay_out_hand(PassGeom *g, int npass, int nx, int ny, int groups, int slot_floats, int slots, int R)
{
    HandLayout h;
    h.nx = nx, h.ny = ny, h.npass = npass, h.groups = groups, h.slot_floats = slot_floats, h.slots = slots, h.R = R;
    long long per_vol = 0;
    for (int q = 0; q < npass; q++) {
        g[q].hand_base = per_vol;
        const int lines = g[q].diag ? 2 * g[q].wmax : g[q].LL;
        h.pass[q] = HandLayout::Pass{per_vol, g[q].nbands, lines, g[q].slope, g[q].diag, g[q].swap};
        per_vol += (long long)g[q].nbands * lines;
    }
    return h;
}

// ---- the tags of a region of self-validating slots, as a state machine ---------------------------------------------------
// The second build's unweighted kernels (mgm_pass2.hip, TAGS) and the range-proportional kernels (k_pass_rel) hand slabs from band
// to band that validate themselves: one slot per (volume, pass, band, pixel), written once per launch OF THAT PASS with the tag
// in the sign bits.  A pass's tag alternates between its consecutive launches over the same slots; a region that moved or is
// wanted in another layout is cleared first (all-ones words) and starts every pass again with tag 0.  A region is laid out for
// the passes [0, layout.npass) and is one protocol's alone, so neither a caller that launches the passes one by one nor one that
// alternates weighted and unweighted runs makes it be cleared again.  The tags are only good for a launch that really rewrites
// every slot of its passes: between hand_begin and hand_commit (after the kernel has been enqueued) the layout counts as
// unknown, so an error return in between cannot leave slots behind that carry the tag of the launch after next; whoever learns
// that a launch may not have written all its slots (a hand-off time-out), or frees the region, calls hand_forget.
constexpr unsigned kHandTagBit = 0x80000000u;
constexpr int kHandClearByte = 0xff;  // what a region is cleared with: its words then have the tag bit set
struct HandTags {
    HandLayout layout;            // what the region was last cleared for (npass 0: unknown -- the next launch clears it)
    unsigned tag[kMaxDirs] = {};  // per pass: the tag its slots carry after its last launch
};
struct HandStep { bool clear; unsigned tag[kMaxDirs]; };  // clear the region first; the tags of the launch's passes [first, end) (the others: 0)
inline HandStep hand_begin(HandTags &t, const HandLayout &want, int first, int end, bool moved)
{
    HandStep s{};
    s.clear = moved || t.layout.npass == 0 || t.layout != want;
    for (int k = 0; s.clear && k < kMaxDirs; k++) t.tag[k] = kHandTagBit;
    for (int k = first; k < end; k++) s.tag[k] = t.tag[k] ^= kHandTagBit;
    t.layout = HandLayout{};
    return s;
}
inline void hand_commit(HandTags &t, const HandLayout &layout) { t.layout = layout; }  // (enqueued: every slot of the launch's passes will carry its tag)
inline void hand_forget(HandTags &t) { t.layout = HandLayout{}; }

// ---- the launch as a list-scheduling problem, simulated ---------------------------------------------------------------
// A chain = the bands of one pass (or one strip of it) of one volume, band b READY once band b-1 (of both strips) started
// `skew` steps earlier; `nqueues` queues of `slots` band slots each, band b of chain k belonging to queue
// (b / QK + k.chain) % nqueues; a free slot starts, among the heads of the chains whose next band belongs to its queue, the
// ready one with the longest remaining chain (none ready: the one that will be first).  Returns the makespan in steps;
// `order` = the items by their start in that schedule -- per queue, the order in which the queue hands them out.
struct SimChain {
    int x, st, nb, sib, chain;
    double skew, len;
    // bands that differ (the anti-diagonal passes of k_pass_rel): band b is ready bskew[b] steps after band b-1 started, runs blen[b]
    // steps, and brem[b] steps of the chain remain behind its start; empty: skew / len for every band
    std::vector<double> bskew, blen, brem;
    double skew_of(int b) const { return bskew.empty() ? skew : bskew[b]; }
    double len_of(int b) const { return blen.empty() ? len : blen[b]; }
    double rem_of(int b) const { return brem.empty() ? (double)(nb - 1 - b) * skew + len : brem[b]; }
    double gap_of(int b) const { return bskew.empty() ? skew : std::min(bskew[b], 4.0); }  // (a band cannot end before its predecessor + this)
};
inline double simulate_schedule(const std::vector<SimChain> &chains, int nqueues, int slots, int QK, std::vector<Task> &order)
{
    const int n = (int)chains.size();
    std::vector<std::vector<double>> start(n), end(n);
    std::vector<int> next(n, 0);
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        start[i].assign(chains[i].nb, 0.0);
        end[i].assign(chains[i].nb, 0.0);
        total += (size_t)chains[i].nb;
    }
    auto queue_of = [&](int i, int b) { return nqueues <= 1 ? 0 : (b / QK + chains[i].chain) % nqueues; };
    typedef std::pair<double, int> Slot;  // (free at, queue)
    std::vector<Slot> heap;
    for (int q = 0; q < std::max(1, nqueues); q++)
        for (int k = 0; k < slots; k++) heap.push_back(Slot(0.0, q));
    std::make_heap(heap.begin(), heap.end(), std::greater<Slot>());
    order.clear();
    const double INF = 1e300;
    double makespan = 0.0;
    size_t guard = 0;
    while (order.size() < total && !heap.empty() && guard++ < 64 * total + 4096) {
        std::pop_heap(heap.begin(), heap.end(), std::greater<Slot>());
        const Slot sl = heap.back();
        heap.pop_back();
        const double t = sl.first;
        int best = -1;
        double best_rem = -1, best_ready = INF;
        bool best_is_ready = false, later = false;
        for (int i = 0; i < n; i++) {
            const SimChain &k = chains[i];
            if (next[i] >= k.nb) continue;
            const int b = next[i];
            if (queue_of(i, b) != sl.second) {
                for (int bb = b + 1; bb < k.nb && !later; bb += std::max(1, QK)) later = queue_of(i, bb) == sl.second;
                continue;
            }
            double ready = 0.0;
            if (b > 0) {
                ready = start[i][b - 1] + k.skew_of(b);
                if (k.sib >= 0) ready = next[k.sib] > b - 1 ? std::max(ready, start[k.sib][b - 1] + k.skew) : INF;
            }
            const double rem = k.rem_of(b);
            const bool is_ready = ready <= t;
            const bool better = best < 0 || (is_ready != best_is_ready ? is_ready : (is_ready ? rem > best_rem : (ready != best_ready ? ready < best_ready : rem > best_rem)));
            if (better) best = i, best_rem = rem, best_ready = ready, best_is_ready = is_ready;
        }
        if (best < 0 || best_ready >= INF) {
            // nothing of this queue can start yet (its next bands follow bands of other queues, or the other strip): look again
            // when the next slot frees; a queue with nothing left retires its slots
            if (best < 0 && !later) continue;
            const double again = heap.empty() ? t + 1.0 : std::max(t, heap.front().first) + 1.0;
            heap.push_back(Slot(again, sl.second));
            std::push_heap(heap.begin(), heap.end(), std::greater<Slot>());
            continue;
        }
        const SimChain &k = chains[best];
        const int b = next[best]++;
        const double st_eff = std::max(t, best_ready);
        double en = st_eff + k.len_of(b);
        if (b > 0) en = std::max(en, end[best][b - 1] + k.gap_of(b));  // (it cannot overtake its predecessor)
        start[best][b] = st_eff;
        end[best][b] = en;
        makespan = std::max(makespan, en);
        heap.push_back(Slot(en, sl.second));
        std::push_heap(heap.begin(), heap.end(), std::greater<Slot>());
        order.push_back(Task{k.x, b + (k.st << 16)});
    }
    if (order.size() < total) {  // (cannot happen; never lose an item to the model)
        for (int i = 0; i < n; i++)
            for (int b = next[i]; b < chains[i].nb; b++) order.push_back(Task{chains[i].x, b + (chains[i].st << 16)});
        makespan = INF;
    }
    return makespan;
}

// The chains of a launch: every (volume group, pass, strip) of the passes [first, first + count).  What the MODEL assumes per
// band -- the two planners differ in it, not in the construction: a band trails the one before it by slope x lines + a lag
// (by the slope of the pass), walks its lines + `len_extra` steps, and on the anti-diagonals of k_pass_rel (g.diag) is ready
// `diag_lag` steps + the shift of its first line after the band before it.
struct ChainModel {
    double lag_slope1, lag_slope2, len_extra, diag_lag;
};
inline std::vector<SimChain> make_chains(const PassGeom *geoms, int ngroups, int first, int count, int R, const ChainModel &m)
{
    std::vector<SimChain> ch;
    for (int v = 0; v < ngroups; v++)
        for (int q = first; q < first + count; q++)
            for (int st = 0; st < geoms[q].nstrips; st++) {
                const PassGeom &g = geoms[q];
                SimChain k;
                k.x = v * kMaxDirs + q, k.st = st, k.nb = g.nbands, k.chain = v * count + (q - first);
                k.sib = g.nstrips == 2 ? (int)ch.size() + (st == 0 ? 1 : -1) : -1;  // (a band waits for BOTH strips of the band before it)
                k.skew = (double)g.slope * R + (g.slope == 1 ? m.lag_slope1 : m.lag_slope2);
                k.len = (g.nstrips == 2 ? (st == 0 ? g.split : g.LL - g.split) + R - 1 : g.LL) + (double)g.slope * (R - 1) + m.len_extra;
                if (g.diag) {  // band b walks lines [lo_b, hi_b] of the pass, one step behind band b - 1 (+ the lag)
                    auto lo = [&](int b) { return std::max(0, b * R - g.LL + 1); };
                    auto hi = [&](int b) { return std::min(g.NL - 1, b * R + R - 1); };
                    k.bskew.assign(g.nbands, 0.0), k.blen.assign(g.nbands, 0.0), k.brem.assign(g.nbands, 0.0);
                    for (int b = 0; b < g.nbands; b++) {
                        k.bskew[b] = b > 0 ? (double)(lo(b) - lo(b - 1)) + m.diag_lag : 0.0;
                        k.blen[b] = (double)(hi(b) - lo(b)) + 2.0;
                    }
                    for (int b = g.nbands - 1; b >= 0; b--) k.brem[b] = b == g.nbands - 1 ? k.blen[b] : std::max(k.blen[b], k.bskew[b + 1] + k.brem[b + 1]);
                }
                ch.push_back(k);
            }
    return ch;
}

// ---- the pruned winner search (k_wta_pruned, mgm_wta.hip) ------------------------------------------------------------------
// Does this launch of the pass kernel write the chunk minima of Lr (PassParams::min_k), and does the winner search behind it
// read them instead of every Lr slab?  A function of the values below and nothing else; a request of its own because
// DenseRequest is what the task tables are cached by, and the table does not depend on this.
//   * the kernels that write minima: the second build's 256-label instances with one volume per wave, one-byte compact
//     costs, unit weights and slabs of E (k_pass2, CHMIN) -- what cfg3 / cfg3h run at any batch size;
//   * a search that can use them: the caller's own, right behind the launch, over all passes of the volume (not the
//     direction-sharded or multi-device building blocks, whose search runs elsewhere or on other slabs), no S volume
//     wanted, refinement none or vfit, no padded label slots, no per-pixel ranges;
//   * MGM_HIP_WTA_PRUNE=0 (`enabled` 0) keeps the plain search for A/B runs and tests.
struct PruneRequest {
    int enabled;            // the environment switch
    int search_follows;     // the caller searches all passes of every volume right behind this launch (mgm_aggregate*)
    int want_S, refine;     // the search writes the corrected volume; refinement index (0 none, 1 vfit, 2.. a second kernel on S)
    int first, count, slot0, nslots;  // passes of the launch and where their volumes go
    int L, Lreal, ragged;   // label slots the kernels see, labels that exist, per-pixel ranges
    int R2, subv, tags, w2, wk, lpl;  // the plan's decisions (DensePlan) and the kernels' labels per lane
    int use_c8, cb;         // compact costs, bytes per cost
    int stride_mod32;       // floats between consecutive Lr volumes, modulo 32 (a chunk's word is found by its address)
};
static_assert(std::has_unique_object_representations_v<PruneRequest>, "PruneRequest: integers only, no padding");
constexpr int kChunkLabels = 32;  // labels per chunk minimum: 128 bytes of an Lr slab
inline bool plan_wta_prune(const PruneRequest &q)
{
    const bool kernel_writes = q.R2 != 0 && q.lpl == 4 && q.L == 256 && q.subv == 1 && q.tags != 0 && q.w2 == 0 && q.wk == 0 && q.use_c8 != 0 && q.cb == 1;
    const bool search_reads = q.search_follows != 0 && q.want_S == 0 && (q.refine == 0 || q.refine == 1) && q.Lreal == q.L && q.ragged == 0 && q.first == 0 &&
                              q.slot0 == 0 && q.nslots == q.count;
    return q.enabled != 0 && kernel_writes && search_reads && q.stride_mod32 == 0;
}

// ---- which instance of a pass kernel a launch runs ---------------------------------------------------------------------------
// Decided by plan_dense / plan_rel from their own request and decisions; the launchers (mgm_pass.hip, mgm_pass2.hip,
// mgm_pass_rel.hip) are tables from a choice to its instance.  tests/test_pass_kernel_plan.py holds the planner against a
// restatement of the launchers it replaced.
enum PassFamily { kPassRefuse = 0, kPassFirst, kPassSecond, kPassRel };
struct PassKernelChoice {
    int family;  // kPassRefuse: no instance serves the launch (the plan's err is kPlanNoKernel)
    // the instance's template arguments: k_pass<LPL, FH, WEIGHTED, R>, k_pass2<LPL, FH, WEIGHTED, MGM, C8, SUBV, DEEP, XCDQ, ONEB, W2>
    // (C8: bytes per compact cost, 0 = fp32 costs), k_pass_rel<FH, PUBE, NK, SPL, CB, FH2>; those an instance does not have are 0
    int LPL, FH, WEIGHTED, R, MGM, C8, SUBV, DEEP, XCDQ, ONEB, W2, PUBE, NK, SPL, CB, FH2;
    // dynamic LDS bytes of the launch (the second build: the FLOOR of the request -- what the instance itself needs depends on
    // the build's macros and stays in mgm_pass2.hip); threads per workgroup (the first build only)
    int lds, block;
};
static_assert(std::has_unique_object_representations_v<PassKernelChoice>, "PassKernelChoice: integers only, no padding");

// The instances that are built, family by family: the planner refuses what these deny, the launchers instantiate exactly what
// they admit.  `dev`: a development build of the second build (-DMGM_P2_DEV=1), which has no queue and no W2 instances -- with the
// timers compiled in, the compiler fails on some of them ("Operand has incorrect register class", V_CMP_NE_U32 on src_shared_base).
constexpr bool pass_instance(int LPL, int R) { return R == 4 ? (LPL == 12 || LPL == 16 || LPL == 24 || LPL == 32) : (R == kR && (LPL == 1 || LPL == 2 || LPL == 3 || LPL == 4 || LPL == 6 || LPL == 8)); }
constexpr bool pass2_instance(bool dev, int LPL, bool FH, bool WEIGHTED, int MGM, int C8, int SUBV, bool DEEP, bool XCDQ, bool ONEB, bool W2)
{
    if (!(LPL == 1 || LPL == 2 || LPL == 3 || LPL == 4 || LPL == 6 || LPL == 8 || LPL == 12 || LPL == 16) || MGM < 1 || MGM > 4) return false;
    const bool slabs_of_E = !WEIGHTED && !(FH && MGM == 2);  // the unweighted kernels whose slabs do not travel with their minimum
    // two-valued weights: the compact kernels with deep rings and per-XCD queues, one band per CU, up to 256 labels
    if (W2) return !dev && LPL <= 4 && !WEIGHTED && C8 == 1 && SUBV == 1 && DEEP && XCDQ && ONEB;
    if (WEIGHTED && LPL >= 12) return false;  // (768 / 1024 labels: the weighted kernels' rings do not fit the LDS; first build)
    // several volumes per wave (128 / 64 labels): no queues (no gain measured there: cfg2 x 4..16, cfg5 x 4..16 within noise)
    if (SUBV != 1) return (SUBV == 2 || SUBV == 4) && LPL == 4 && slabs_of_E && C8 == 1 && !XCDQ && !ONEB;
    if (ONEB && !XCDQ) return false;
    if (XCDQ && (dev || !DEEP)) return false;
    if (DEEP) return slabs_of_E && (C8 == 1 || (C8 == 2 && LPL <= 8));  // deep DMA rings: compact costs
    return C8 == 0 || C8 == 1;  // (two bytes per cost, round 4: the kernels with deep rings only)
}
constexpr bool pass_rel_instance(bool FH, bool PUBE, int NK, int SPL, int CB, bool FH2)
{
    if (!(SPL == 4 || SPL == 8) || !(CB == 1 || CB == 2 || CB == 4)) return false;
    if (!FH) return NK == 0 && !FH2;
    if (PUBE) return false;
    // update_cost2_trunclinear: on 128 slots of fp32 costs its rings + the cost pieces exceed the LDS (plan_agg_route keeps that one on the dense hull)
    if (FH2) return NK == 2 && !(SPL == 8 && CB == 4);
    // (NK 0: the one-after-the-other build, kept for the form round 5 measured, as an A/B switch -- tune rel_multi=0)
    return NK == 0 ? (SPL == 4 && CB == 1) : (NK >= 1 && NK <= 4);
}
inline bool pass_instance_exists(const PassKernelChoice &k, bool dev)
{
    if (k.family == kPassFirst) return pass_instance(k.LPL, k.R);
    if (k.family == kPassSecond) return pass2_instance(dev, k.LPL, k.FH, k.WEIGHTED, k.MGM, k.C8, k.SUBV, k.DEEP, k.XCDQ, k.ONEB, k.W2);
    return k.family == kPassRel && pass_rel_instance(k.FH, k.PUBE, k.NK, k.SPL, k.CB, k.FH2);
}
// the instance as a kernel trace prints it, e.g. "k_pass2<4, true, false, 2, 1, 1, true, true, true, false>"; returns strlen
inline int pass_kernel_name(const PassKernelChoice &k, char *buf, size_t cap)
{
    auto b = [](int v) { return v ? "true" : "false"; };
    if (k.family == kPassFirst) return snprintf(buf, cap, "k_pass<%d, %s, %s, %d>", k.LPL, b(k.FH), b(k.WEIGHTED), k.R);
    if (k.family == kPassSecond)
        return snprintf(buf, cap, "k_pass2<%d, %s, %s, %d, %d, %d, %s, %s, %s, %s>", k.LPL, b(k.FH), b(k.WEIGHTED), k.MGM, k.C8, k.SUBV, b(k.DEEP), b(k.XCDQ), b(k.ONEB), b(k.W2));
    if (k.family == kPassRel) return snprintf(buf, cap, "k_pass_rel<%s, %s, %d, %d, %d, %s>", b(k.FH), b(k.PUBE), k.NK, k.SPL, k.CB, b(k.FH2));
    return snprintf(buf, cap, "refused");
}

// ---- the dense kernels (k_pass / k_pass2) --------------------------------------------------------------------------------
enum { kPlanOk = 0, kPlanNotCanonical = 1, kPlanTooManyBands = 2, kPlanLostQueues = 3, kPlanNoKernel = 4 };
struct DensePlan {
    int err = kPlanOk;
    PassKernelChoice kernel = {};       // the instance the launch runs (err kPlanNoKernel: none does)
    // the decisions
    int subv = 1, ngroups = 0, Lk = 0;  // volumes per wave, volume groups, label slots of a wave
    int R2 = 0, R = 0;                  // lines per band of the second build (0: the first build runs), of the launch
    int w2 = 0, wk = 0;                 // the two-valued weights' kernels; the general weighted kernels
    int tags = 0, NS = 1, LPk = 0;      // self-validating hand-off slots; slabs per slot; floats per slot of that protocol
    int wg_per_cu = 1, deep = 0, oneb = 0;
    int xcdq = 0, nq = 8, QK = 1 << 20, one_queue = 0;
    int any_strips = 0;
    int maxLL = 0;
    double load_ratio = 0;        // band-steps per CU over the longest chain of the launch
    double t_one = 0, t_q = 0;    // simulated makespans (steps): one queue, the per-XCD queues
    PassGeom g[kMaxDirs] = {};
    long long hand_vstride = 0;
    HandLayout hand;              // (tags only)
    std::vector<Task> order;      // the global ticket order
    std::vector<Task> table;      // as uploaded: the eight queues' (first ticket, count), then the items (bit 24: plain hand-off)
    int ntasks = 0;
};

// 128 / 64 labels: 2 / 4 volumes of the launch share every wave of the 256-label kernels (k_pass2<..., SUBV>) -- a
// step is mostly fixed cost, so it may as well serve several volumes.  Compact costs, no weights, not FH with
// TSGM = 2 (whose slabs travel with their minimum), and a volume count that divides.
// Only from two such groups on, though: sharing a wave halves the band-steps but makes every step the longer step of
// the 256-label kernels, and a launch of one group is bound by its chain of bands, i.e. by the step (round 3,
// 1920x1080x128 x 2: K3 3.74 ms sharing, 3.11 ms as two plain work items; x 4: the same either way).
// (reads nothing of the request that depends on it: the caller asks before it fills `lines2`)
inline int dense_subv(const DenseRequest &q)
{
    if (!q.first_build && q.use_c8 && q.cb == 1 && q.wmode == kWeightsNone && !(q.fh && q.MGM == 2) && (q.L == 128 || q.L == 64) && q.nb % (256 / q.L) == 0 &&
        (q.subv == 2 || (q.subv == 1 && q.nb / (256 / q.L) >= 2)))
        return 256 / q.L;
    return 1;
}

// longest remaining chain first: item (p, b) is followed, band after band, by (nbands - 1 - b) hand-offs of slope * R + lag
// steps and its own walk.  A valid order by itself (within a pass the remaining chain shrinks with b): what a launch takes
// when the simulation gives up.
inline std::vector<Task> order_by_remaining_chain(const PassGeom *geoms, int ngroups, int first, int count, int R, double lag)
{
    std::vector<Task> tasks;
    for (int v = 0; v < ngroups; v++)
        for (int q = first; q < first + count; q++)
            for (int b = 0; b < geoms[q].nbands; b++)
                for (int st = 0; st < geoms[q].nstrips; st++) tasks.push_back(Task{v * kMaxDirs + q, b + (st << 16)});
    auto rem = [&](const Task &t) {
        const PassGeom &g = geoms[t.x % kMaxDirs];
        const int b = t.y & 0xffff, st = (t.y >> 16) & 0xff;
        const double walk = (g.nstrips == 2 ? (st == 0 ? g.split : g.LL - g.split) + R - 1 : g.LL) + (double)g.slope * R;
        return (double)(g.nbands - 1 - b) * (g.slope * R + lag) + walk;
    };
    std::stable_sort(tasks.begin(), tasks.end(), [&](const Task &a, const Task &b) {
        const double ra = rem(a), rb = rem(b);
        return ra != rb ? ra > rb : a.x < b.x;
    });
    return tasks;
}

inline DensePlan plan_dense(const DenseRequest &q)
{
    DensePlan p;
    const int nx = q.nx, ny = q.ny, L = q.L, nb = q.nb, first = q.first, count = q.count, MGM = q.MGM, PEND = first + count;
    const bool fh = q.fh != 0, weighted = q.wmode != kWeightsNone, use_c8 = q.use_c8 != 0, first_build = q.first_build != 0;
    const int lpl = q.lpl, LP = lpl * 64;
    // (768 / 1024 labels with weights that are not two-valued-and-narrow: the weighted kernels of the second build stop at
    // 512 labels -- two slabs per slot do not fit the LDS beyond -- so those take the first build, which has no compact costs)
    const bool wide_weighted = weighted && lpl > 8;
    // second build (LDS-DMA loaders) whenever the slabs are whole DMA pieces
    const int subv = p.subv = dense_subv(q);
    const int ngroups = p.ngroups = nb / subv;  // work items address groups of `subv` volumes
    const int Lk = p.Lk = L * subv;             // label slots of a wave
    const int R2 = p.R2 = (first_build || wide_weighted) ? 0 : q.lines2;
    const int R = p.R = R2 ? R2 : (lpl > 8 ? 4 : kR);  // (more than 512 labels: the first build with bands of four lines)
    int maxLL = 0, maxbands = 0;
    for (int k = 0; k < std::max(PEND, q.layout_ndir); k++) {
        if (!make_geom(k, nx, ny, R, MGM, R2 != 0, p.g[k])) return p.err = kPlanNotCanonical, p;
        maxLL = std::max(maxLL, p.g[k].LL);
        maxbands = std::max(maxbands, p.g[k].nbands);
    }
    p.maxLL = maxLL;
    if (maxbands > kMaxBands) return p.err = kPlanTooManyBands, p;
    // Two-valued weights (k_pass2, W2): the compact kernels with deep rings and per-XCD queues, every volume's weights 1 and
    // one other positive value.  Anything they do not cover -- fp32 costs, more than 256 labels, launches too small for the
    // queues, a partitioned device, FH on ragged volumes (which borrows the weighted kernels) -- keeps the general
    // weighted kernels.
    // (FH on a ragged volume WITH two-valued weights as well: the producer-side transforms of W2 convolve over the SENDING pixel's
    // slab -- found by the long random campaign of tests/test_gpu_rel.py in round 5, where the range-proportional kernels and the
    // reference agreed and this path did not)
    bool w2 = q.wmode == kWeightsTwoValued && q.w2 && R2 && use_c8 && q.cb == 1 && lpl <= 4 && !(fh && q.ragged) && !q.devtools && q.xcdq != 0 && q.deep != 0;
    if (w2) {
        int items = 0;
        for (int k = first; k < PEND; k++) items += nb * p.g[k].nbands;
        w2 = items >= 32;
    }
    w2 = w2 && xcc_queues(q.xcc_mask) > 0;
    const bool wk = weighted && !w2;  // the general weighted kernels (consumer-side transforms, progress words)
    p.w2 = w2, p.wk = wk;
    p.NS = w2 ? 2 : q.ns;
    const int LPk = p.LPk = (subv > 1 ? Lk : LP) * (w2 ? 2 : 1);  // floats per hand-off slot of the self-validating protocol
    // The second build's unweighted kernels hand slabs from band to band that validate themselves (mgm_pass2.hip, TAGS):
    // one slot per (volume, pass, band, pixel), written once per launch OF THAT PASS with the tag in the sign bits.  The
    // region is laid out for the passes [0, layout_ndir) and is this protocol's alone, so neither a caller that launches
    // the passes one by one nor one that alternates weighted and unweighted runs makes it be cleared again (mgm_plan.hip).
    const bool tags = R2 && !wk && (w2 || !(fh && MGM == 2));
    p.tags = tags;
    if (tags) {
        p.hand = lay_out_hand(p.g, q.layout_ndir, nx, ny, ngroups, LPk, 0, R);
        p.hand_vstride = p.hand.per_group();
    }

    double load_ratio = 0;  // band-steps per CU over the longest chain of the launch
    {
        // Two bands per CU pay when the launch is bound by throughput, not by the longest chain of bands: compare the
        // band-steps one CU has to run with the critical path of the slowest pass (steps of slope*lines + line length
        // + the hand-off lag per band: ~3 steps with self-validating slabs, ~10 with progress words).  Measured on
        // 1920x1080 (round 2, after the hand-off rewrite): the FH kernels -- long dependent instruction chains per step --
        // gain from the second band from a ratio of ~1.8 on (three cfg3 volumes per launch; 12 volumes: 64 -> 51 ms); the
        // Hirschmueller kernels only at large batches of 256 labels (+3 % at 12 volumes), and lose 3-10 % at 128 labels
        // or small batches: their steps are short enough for one band to keep the CU's issue slots busy.
        double work = 0, chain = 0;
        const double lag = tags ? 3.0 : 10.0;
        for (int k = first; k < PEND; k++) {
            const PassGeom &g = p.g[k];
            work += (double)ngroups * g.nbands * (g.LL + g.slope * R);
            chain = std::max(chain, (double)g.slope * g.NL + g.LL + lag * g.nbands);
        }
        // (round 3, with the XCD queues: two 256-label FH volumes, ratio 1.66, K3 10.29 -> 9.93 ms with the second band; one
        // volume -- 0.83 -- loses 20 % with it: the FH threshold moved from 1.8 to 1.5)
        p.wg_per_cu = (work / (double)q.num_cu > (fh ? 1.5 : 8.0) * chain) ? 2 : 1;
        load_ratio = work / (double)q.num_cu / chain;
        // Deep DMA rings (k_pass2, DEEP) for every compact unweighted launch: same-process A/B runs of round 3
        // (tools/ab_env.sh, shallow -> deep) give -13 % of K3 for one 128-label volume, -15 % at 4096x4096x192, -3 % for
        // one or two 256-label FH volumes, -3 % for 8 or 16 128-label volumes, and 0..-1 % for twelve 256-label ones.
        p.deep = (tags && use_c8) ? 1 : 0;
    }
    p.load_ratio = load_ratio;
    if (q.deep >= 0) p.deep = (tags && use_c8 && q.deep) ? 1 : 0;
    if (q.wg_per_cu) p.wg_per_cu = q.wg_per_cu;
    // Per-XCD work queues (k_pass2, XCDQ): launches in which the chains of bands matter.  The workgroups stay and work a
    // queue off (a band that follows another on a CU starts at once instead of waiting for a workgroup to be dispatched),
    // and most hand-offs stay inside an XCD's L2.  Same-box A/B runs (round 3, 1920x1080, K3 without -> with queues):
    // 256 labels FH x 1 6.9 -> 6.4 ms, x 2 11.0 -> 10.3, x 3 14.6 -> 13.9, x 4 18.6 -> 17.8, x 6 and x 12 (load/chain 5
    // and 10) 0 .. +1 %; Hirschmueller x 1 5.4 -> 4.85, x 2 8.6 -> 8.15; 128 labels x 1 2.38 -> 2.07, x 3 4.40 -> 4.24;
    // 4096x4096x192 x 1 +-0, x 2 (load/chain 5.4) +1 %.  One queue for all XCDs (MGM_HIP_XCDQ=2: the staying workgroups
    // alone) gives 6.5, 5.2 and 2.08 ms for the three single volumes, 16.3 instead of 15.3 for three 256-label ones.
    // Needs all eight XCC ids to show up in a launch (a partitioned device shows fewer), and a launch large enough for
    // the dispatcher's round robin to have put several workgroups on every XCD: a queue is only worked off by
    // workgroups that find themselves on its XCD -- a small launch keeps the single ticket counter.
    bool xcdq = false;
    int nitems = 0;  // work items of the launch (before strips) = its workgroups
    for (int k = first; k < PEND; k++) nitems += ngroups * p.g[k].nbands;
    // Hirschmueller potentials (short steps: the second band per CU never gave them more than 3 %): with the queues, ONE band per
    // CU is the better schedule at every batch size -- same-box A/B runs of 256-label volumes, two bands per CU without
    // queues -> one with: x 8 0.964 -> 0.985 of the roofline, x 12 0.957 -> 0.981 (K3 46.9 -> 44.9 ms); 4096x4096x192 x 2 +-0 --,
    // so they take the queues whatever the load; the FH kernels, which need the second band from a load/chain of 1.5 on,
    // below a load/chain of 4.
    const bool always_q = !fh;
    if (tags && p.deep && subv == 1 && R2 && nitems >= 32 && !q.devtools && (w2 || q.xcdq >= 1 || (q.xcdq < 0 && (always_q || load_ratio < 4.0))))
        xcdq = xcc_queues(q.xcc_mask) > 0;
    const int nq = p.nq = xcdq ? xcc_queues(q.xcc_mask) : 8;  // queues of the launch (the XCDs of the device)
    if (xcdq && always_q && !q.wg_per_cu) p.wg_per_cu = 1;
    if (w2) {
        if (!xcdq || !p.deep) return p.err = kPlanLostQueues, p;
        p.wg_per_cu = 1;  // (two slabs per slot: one band per CU)
    }
    p.xcdq = xcdq;
    p.oneb = (xcdq && p.wg_per_cu < 2 && q.oneb) ? 1 : 0;
    // The instance: what was decided above, as template arguments.  A combination nothing is built for ends here (a switch that
    // takes the deep rings from two-byte costs, a label count without an object of the second build) instead of at the launch.
    PassKernelChoice &kn = p.kernel;
    kn.LPL = R2 ? (subv > 1 ? 4 : (L % 64 ? 0 : L / 64)) : lpl, kn.FH = fh, kn.WEIGHTED = R2 ? wk : weighted;
    if (R2) {
        kn.family = kPassSecond, kn.MGM = MGM, kn.C8 = use_c8 ? (q.cb == 2 ? 2 : 1) : 0, kn.SUBV = subv, kn.DEEP = p.deep, kn.XCDQ = xcdq, kn.W2 = w2;
        kn.ONEB = w2 ? 1 : p.oneb;  // (the W2 kernels exist as one-band builds only: MGM_HIP_ONEB=0 does not reach them)
        // Occupancy is chosen per launch through the LDS request: the compact unweighted kernels are built for two
        // workgroups per CU (<= 64 VGPRs, < 80 KB of LDS).  Two bands per CU hide each other's barrier and LDS stalls --
        // right when the launch is throughput-bound (a batch of volumes); a single volume is bound by the chain of
        // bands, where the doubled step latency costs more than it gives, so it asks for > half the LDS and runs alone.
        kn.lds = p.wg_per_cu < 2 ? 81 * 1024 : 0;
    } else {
        kn.family = kPassFirst, kn.R = R;
        kn.lds = (int)sizeof(float) * (R * 2 * ((weighted && !fh) ? 2 : 1) * LP + R * 2) + 16, kn.block = R * 64;  // (two slabs per slot: weighted Hirschmueller)
    }
    if (!pass_instance_exists(kn, q.devtools != 0)) return kn = PassKernelChoice{}, p.err = kPlanNoKernel, p;
    // Two strips per line: the passes without an in-line dependency -- form 1 with 2 or 3 neighbours -- walk their lines
    // from both image edges inwards (mgm_pass2.hip): half the line length in the critical path of a pass, bands that
    // live half as long, for twice the work items, each with its own pipeline ramp and hand-off lag (and 1-2 % of the
    // pixels of such a pass computed twice).  Round 3, same-box A/B runs:
    //   * with the deep rings alone the strips LOSE on whole volumes (strips -> none, 1920x1080: 256 labels x 1 K3 7.60 ->
    //     7.21 ms FH, 5.42 -> 5.15 Hirschmueller; 4096x4096x192 27.5 -> 26.2; two or three volumes -2..-5 % too) and win
    //     where a launch runs only a FEW passes of one volume (a rank of a direction-sharded run; 4096x4096x192,
    //     tools/time_passes.py, none -> strips: one pass 8.8 -> 7.8-8.0 ms, two 10.7 -> 9.7, four 15.5 -> 14.9-15.2);
    //   * with the XCD queues -- a finished strip's successor starts at once -- they win wherever the chains dominate
    //     (none -> strips, 1920x1080x256: FH x 1 6.47 -> 6.18, x 2 10.25 -> 10.0, x 3 14.0 -> 13.5 but x 4 17.7 -> 18.1;
    //     Hirschmueller x 1 4.85 -> 4.70, x 2 and x 3 +-0; 4096x4096x192 x 1 (load/chain 2.7) 26.5 -> 27.0, x 2 50.9 -> 52.6;
    //     a rank's four passes of 4096x4096x192 9.6 -> 8.4 with queues and strips together): on below a load/chain of 2.
    bool any_strips = false;
    if (tags && !w2 && (q.strips == 1 || (q.strips < 0 && ((ngroups == 1 && count <= 4 && p.wg_per_cu == 1) || (xcdq && load_ratio < 2.0)))))
        for (int k = first; k < PEND; k++)
            if (p.g[k].form == 1 && (MGM == 2 || MGM == 3) && p.g[k].LL >= 8 * R) {
                p.g[k].nstrips = 2;
                p.g[k].split = p.g[k].LL / 2;
                any_strips = true;
            }
    p.any_strips = any_strips;
    // bands per queue block: a pass stays on one XCD when the passes of the launch fill the eight queues evenly; otherwise
    // blocks of two bands, which spread four or twelve passes over all XCDs at the price of every second hand-off
    // crossing.
    // Measured (K3, block 0 / 1 / 2, no queues): 1920x1080x256 FH x 2 10.2 / 10.9 / 11.3 (11.4), x 3 14.2 / 15.5 / 15.5 (16.5),
    // x 4 17.7 / 18.4 / 17.9 (19.1); Hirschmueller x 3 13.0 / 13.35 / 13.4 (13.5); 128 labels x 1 (four passes) 2.85 / 2.08 /
    // 2.07 (2.35); 4096x4096x192 x 1 27.2 / 27.5 / 26.4 (27.65) -- lines that long keep far more bands in flight than an
    // XCD has CUs, and a pinned pass that takes longer than the others leaves the other XCDs idle at the end.
    int QK = ((ngroups * count) % nq == 0 && maxLL <= 3000) ? 0 : 2;
    if (q.xcdq_k >= 0) QK = q.xcdq_k;
    if (QK <= 0) QK = 1 << 20;
    p.QK = QK;

    // task table: ticket -> (pass, band [, strip]); item (p, b, .) always follows the items (p, b-1, .)
    // LIST SCHEDULING, simulated (simulate_schedule, above): the tickets come out in the order in which a machine of
    // band slots that always starts, among the items whose predecessor band is far enough ahead (READY), the one with
    // the longest remaining chain would start them.  The launch then follows that schedule by itself -- every free
    // workgroup takes the next ticket of its queue -- as far as its step times match the model's (one step = one time
    // unit for every pass), and an item taken early merely waits, as it always could.  What a plain
    // longest-remaining-chain order gets wrong is the START of the launch: it hands the first 256 tickets to some sixty
    // consecutive bands of the two longest chains, of which band k cannot move before k * (slope * R) steps have
    // passed (timeline, round 5: 43 % of the CUs waiting through the first millisecond; before that, rounds 1-4 dealt by
    // relative progress b / nbands and left 14-24 % of a single launch's CU-time as tail: docs/experiments.md).
    // The same simulation DECIDES between the per-XCD queues and one queue for all XCDs (write-through hand-offs
    // everywhere): a pass pinned to an XCD runs in whole rounds of that XCD's 32 CUs -- 72 row bands of 2.3 ms are three
    // rounds, the last one a quarter full (1920x1080x256 FH x 1, K3: pinned 6.08 ms, one queue 5.76; two volumes, two
    // passes per XCD: 10.25 against 11.04) -- so the plan takes the single queue where its simulated makespan is
    // shorter by more than what the crossing hand-offs cost (4 %).
    const double lagS = tags ? 5.0 : 12.0;
    const std::vector<SimChain> ch = make_chains(p.g, ngroups, first, count, R, ChainModel{lagS, lagS, 3.0, 0.0});
    size_t total = 0;
    for (const SimChain &k : ch) total += (size_t)k.nb;
    const int slots = std::max(1, q.num_cu * std::max(1, p.wg_per_cu));
    std::vector<Task> ord_one, ord_q;
    const double t_one = simulate_schedule(ch, 1, slots, 1 << 20, ord_one);
    double t_q = t_one;
    if (xcdq) t_q = simulate_schedule(ch, nq, std::max(1, slots / nq), QK, ord_q);
    const int forced = q.one_queue;
    // (launches that run two bands per CU keep their queues: with the doubled step the pinned dealing measured 5 % FASTER
    // for two and four 256-label FH volumes although the model says otherwise -- 9.67 against 10.18 ms, 17.7 against 18.3)
    const bool one_queue = xcdq && (q.xcdq == 2 || forced > 0 || (forced < 0 && p.wg_per_cu < 2 && t_one * 1.04 < t_q));
    const bool sim_ok = ((xcdq && !one_queue) ? t_q : t_one) < 1e299 && ((xcdq && !one_queue) ? ord_q : ord_one).size() == total;
    // (never seen: the simulation gave up.  Its leftovers are NOT a valid order -- a strip's band would precede the
    // other strip's band before it -- so the launch takes the sorted order: longest remaining chain first, which is one)
    if (sim_ok) p.order = (xcdq && !one_queue) ? ord_q : ord_one;
    else p.order = order_by_remaining_chain(p.g, ngroups, first, count, R, tags ? 3.0 : 10.0);
    p.one_queue = one_queue, p.t_one = t_one, p.t_q = t_q;
    p.ntasks = (int)p.order.size();

    // The table's header: the eight XCD queues (first ticket, count).  xcdq: the sorted items are dealt to the queues
    // in blocks of QK consecutive bands of a pass, consecutive blocks to consecutive queues, the passes staggered;
    // every queue keeps the global order (what the progress argument of k_pass2 rests on), and an item whose
    // successor band sits in the same queue is marked for a plain hand-off (bit 24).
    p.table.assign(8, Task{0, 0});
    if (xcdq) {
        std::vector<Task> qs[8];
        for (const Task &t : p.order) {
            const int v = t.x / kMaxDirs, k = t.x % kMaxDirs, b = t.y & 0xffff;
            const int chain = v * count + (k - first);
            const bool same = b + 1 < p.g[k].nbands && (b + 1) / QK == b / QK;
            if (one_queue) qs[0].push_back(t);  // (one queue for all XCDs, write-through hand-offs)
            else qs[(b / QK + chain) % nq].push_back(Task{t.x, t.y | (same ? 1 << 24 : 0)});
        }
        int at = 0;
        for (int k = 0; k < 8; k++) {
            p.table[k] = Task{at, (int)qs[k].size()};
            at += (int)qs[k].size();
            p.table.insert(p.table.end(), qs[k].begin(), qs[k].end());
        }
    } else
        p.table.insert(p.table.end(), p.order.begin(), p.order.end());
    return p;
}

// ---- the range-proportional kernels (k_pass_rel) -------------------------------------------------------------------------
struct RelPlan {
    int err = kPlanOk;
    PassKernelChoice kernel = {};  // the instance the launch runs (err kPlanNoKernel: none does)
    int rel_wg = 1;    // workgroups (4 compute waves + the loader) per CU
    int diag_any = 0;  // some pass walks anti-diagonals
    int swapmask = 0;  // the passes walked with exchanged roles
    int maxLL = 0;
    PassGeom g[kMaxDirs] = {};
    long long hand_vstride = 0;
    HandLayout hand;
    std::vector<Task> order;  // the global ticket order
    std::vector<Task> table;  // as uploaded: the order, bit 24 = issue priority
    int ntasks = 0;
};

// the chains of a range-proportional launch as the planner's model has them (`g`: the plan's geometry)
inline std::vector<SimChain> rel_chains(const RelRequest &q, const PassGeom *g)
{
    return make_chains(g, q.nb, 0, q.NDIR, q.R, ChainModel{1.0 + (double)q.rel_lag, 2.0 + (double)q.rel_lag, 1.0, 7.0 + (double)q.rel_lagd});
}

inline RelPlan plan_rel(const RelRequest &q)
{
    RelPlan p;
    const int nx = q.nx, ny = q.ny, NDIR = q.NDIR, nb = q.nb, MGM = q.MGM, R = q.R;
    const bool fh = q.fh != 0;
    int maxLL = 0, maxbands = 0;
    for (int k = 0; k < NDIR; k++) {
        // (round 6) form-0 passes with TSGM <= 3 walk slope 1 (make_geom decides; tune rel_slope1=0: slope 2 everywhere, as in round 5)
        if (!make_geom(k, nx, ny, R, MGM, q.rel_slope1 != 0, p.g[k])) return p.err = kPlanNotCanonical, p;
        maxLL = std::max(maxLL, p.g[k].LL);
        maxbands = std::max(maxbands, p.g[k].nbands);
        // (round 6) two strips per line for the form-1 passes: no pixel of those passes depends on its own line with TSGM <= 3, so the
        // two halves of a band's lines are two work items (k_pass_rel).  Measured, 1920x1080, windows of 49 labels: FH x 1 8.91 -> 8.12 ms,
        // x 4 13.33 -> 12.89; Hirschmueller x 1 6.13 -> 5.53 (tune rel_strips=0: none)
        // (round 6, later) ... and better: those passes ACROSS their lines, bands of anti-diagonals in lock step (k_pass_rel, g.diag) -- the
        // chain of a pass is NL + bands x lag steps instead of 2 NL + LL / 2 + bands x lag.  Two hand-off lines per band and a second hand
        // ring in LDS: where that does not fit (the three-slab entries of 128 slots with two-byte costs) the strips stay.  tune rel_diag=0: strips
        // (round 6, last) form-0 passes with TSGM <= 3 and more lines than pixels per line (the column passes of a landscape image) are walked
        // with the roles of i and j exchanged: (i - 1, j), (i, j - 1), (i - 1, j - 1) is symmetric in them, the depth NL + LL stays, but a band
        // trails the band before it by ~2 x 16 steps in practice (the pace of a chain is that of its slowest band), so FEWER bands of longer
        // lines end sooner: 68 x D + 1920 against 120 x D + 1080.  tune rel_swap=0: none
        // (FH x 1 5.73 -> 5.27 ms, x 2 7.34 -> 7.04, windows of 101 labels 8.58 -> 7.9, x 4 unchanged; the short steps of the Hirschmueller launches lose
        // 1-2 % with it -- 4.17 / 5.03 / 8.05 -> 4.19 / 5.16 / 8.16 -- and keep their walks: rel_swap=2 forces it there too)
        if ((q.rel_swap >= 2 || (q.rel_swap == 1 && fh)) && p.g[k].form == 0 && MGM <= 3 && p.g[k].slope == 1 && p.g[k].NL > p.g[k].LL) {
            PassGeom &g = p.g[k];
            std::swap(g.NL, g.LL);
            std::swap(g.istep, g.jstep);
            g.swap = 1;
            p.swapmask |= 1 << k;
            g.nbands = (g.NL + R - 1) / R;
            g.split = g.LL;
            maxLL = std::max(maxLL, g.LL);
        }
        const bool diag_ok = q.rel_diag != 0 && p.g[k].form == 1 && MGM <= 3 && q.diag_fits;
        if (diag_ok) {
            PassGeom &g = p.g[k];
            g.diag = 1;
            g.slope = 0;
            g.nbands = (g.NL + g.LL - 1 + R - 1) / R;
            g.wmax = std::min(g.NL, g.LL + R);
            p.diag_any = 1;
        } else if (q.rel_strips != 0 && p.g[k].form == 1 && MGM <= 3 && p.g[k].LL >= 8 * R) {
            p.g[k].nstrips = 2;
            p.g[k].split = p.g[k].LL / 2;
        }
        maxbands = std::max(maxbands, p.g[k].nbands);
    }
    p.maxLL = maxLL;
    if (maxbands > kMaxBands) return p.err = kPlanTooManyBands, p;
    // the instance: the volumes' format, the potentials, how many of a pixel's min-convolutions run side by side
    PassKernelChoice &kn = p.kernel;
    kn.family = kPassRel, kn.FH = fh, kn.PUBE = !fh && q.pube, kn.SPL = q.slots == 128 ? 8 : 4, kn.CB = q.cb == 4 ? 4 : (q.cb == 2 ? 2 : 1);
    if (fh && !(kn.SPL == 4 && kn.CB == 1 && !q.rel_multi)) kn.FH2 = q.fh2 != 0, kn.NK = kn.FH2 ? 2 : (MGM >= 1 && MGM <= 3 ? MGM : 4);
    if (!pass_instance_exists(kn, false)) return kn = PassKernelChoice{}, p.err = kPlanNoKernel, p;
    // self-validating hand-off slots, one per (volume, pass, band, pixel): written once per launch with the launch's tag (see
    // k_pass_rel); another geometry clears the region (all-ones words) and starts again with tag 0
    p.hand = lay_out_hand(p.g, NDIR, nx, ny, nb, q.HS, q.slots, R);
    p.hand_vstride = p.hand.per_group();
    // workgroups (4 compute waves + the loader) per CU: tune rel_wg forces it
    // (measured, round 6, 1920x1080 windows of 49 labels, FH with the side-by-side convolutions: x 1 7.87 / 8.20 / 8.53 ms at 1 / 2 / 3 per CU,
    // x 2 13.0 / 8.6 / 9.6, x 4 24.3 / 14.1 / 12.9; Hirschmueller the same order)
    // (with the anti-diagonal passes a single launch is no longer one long chain: x 1 6.89 / 6.32 / 6.47 ms at 1 / 2 / 3, x 2 11.5 / 7.82 / 7.76,
    // x 4 22.0 / 13.0 / 12.3; Hirschmueller x 1 5.45 / 4.62 / 4.36)
    const int rel_wg = p.rel_wg = q.rel_wg > 0 ? std::min(q.rel_wg, 6) : (nb <= 1 ? (fh ? 2 : 3) : 3);
    // Occupancy through the LDS request, as for the second build: rel_wg workgroups (of 4 compute waves: one per SIMD) share a
    // CU -- one for a launch bound by its chains of bands, more for a batch (throughput): more than a (rel_wg + 1)-th of the LDS
    kn.lds = (int)std::max(rel_wg_lds_bytes(kn.FH || kn.PUBE, 16 * kn.SPL, kn.CB, kn.FH2 != 0, p.diag_any != 0), (long long)kLdsBytes / (rel_wg + 1) + 1024);
    // the task table: the simulated list schedule of the launch (one ticket counter)
    // (slope of the lock-step diagonal x lines + the lag the MODEL assumes per band.  The tickets are the start order of the
    // simulated schedule, so these constants decide who holds a band slot while it waits: with the hand-off's real ~4 steps on
    // every chain, the anti-diagonal bands -- ready every few steps -- took the first 400 of 512 slots and sat in them.  Measured
    // (tools/ab_rel_lag.sh): 1-2 steps on the line walks, 7 on the anti-diagonals: x 1 6.15 -> 5.72 ms, Hirschmueller x 2 5.42 -> 5.0,
    // windows of 101 labels 9.09 -> 8.5, four volumes unchanged; tune rel_lag / rel_lagd: added to them)
    const std::vector<SimChain> ch = rel_chains(q, p.g);
    (void)simulate_schedule(ch, 1, std::max(1, (int)((long long)(q.num_cu * rel_wg) * q.rel_slots / 100)), 1 << 20, p.order);
    p.table = p.order;
    // workgroups that share a CU slow each other down (a step of 1.07 us becomes ~1.5): the bands of the longest chains -- what the
    // launch ends with -- get the issue priority (bit 24 of the task word; tune rel_prio=0: none, =100: every chain within x % of the longest)
    {
        const double pct = (double)q.rel_prio;  // (x 1 6.25 -> 6.03 ms, Hirschmueller 4.36 -> 4.22; x 4 12.3 -> 12.4: not there)
        double longest = 0.0;
        for (const SimChain &k : ch) longest = std::max(longest, k.rem_of(0));
        for (Task &t : p.table)
            for (const SimChain &k : ch)
                if (k.x == t.x && k.st == ((t.y >> 16) & 0xff)) {
                    if (pct > 0.0 && k.rem_of(0) >= longest * (1.0 - pct / 100.0) && rel_wg > 1) t.y |= 1 << 24;
                    break;
                }
    }
    p.ntasks = (int)p.table.size();
    return p;
}

// ---- the winner search (mgm_wta.hip) ---------------------------------------------------------------------------------------
// Which kernel instance a search runs on, and on how many workgroups: a function of the request and nothing else.  mgm_plan.hip
// fills the requests (run_wta, run_wta_right, run_wta_runnerup), the launchers of mgm_wta.hip are tables from a choice to its instance, and
// tests/test_wta_plan.py holds the planner against a restatement of the launchers it replaced.
struct WtaRequest {
    long long npix;           // pixels of the call
    int L, Lreal, NDIR, lpl;  // label stride, labels that exist, passes; what the kernels report: pass_lpl(L)
    int cbytes, compact;      // bytes per cost of the compact copy; the search reads a compact copy (WtaParams::C8)
    int refine, want_S;       // refinement index; the search writes the corrected volume
    int window, ragged;       // range images given (WtaParams::wlo); the volume has ranges of its own (WtaParams::clo)
    // the volume was a slot of the context's last dense launch; that launch wrote its chunk minima and they are still there; the Lr
    // pointer, its stride and NDIR are that launch's own (the slot's first volume, every pass of it)
    int in_last_run, last_min, lr_is_last;
    int pix0_zero, padded, nvol_mod32, num_cu;  // the call starts at pixel 0; the launch ran with padded labels; Lr stride % 32; CUs
    // the switches (WtaSwitches, mgm_host.h): MGM_HIP_WTA_PRUNE / wta_prune, then MGM_HIP_TUNE=wta_prune_ppw=1|2,
    // wta_prune_wg=<workgroups per CU>, wta_wg_per_cu=<the same for the plain search>, wta_packed=0, wta_wide4=0, wta_quad=0
    int sw_prune, sw_prune_ppw, sw_prune_wg, sw_wg_per_cu, sw_packed, sw_wide4, sw_quad;
};
static_assert(std::has_unique_object_representations_v<WtaRequest>, "WtaRequest: integers only, no padding");
enum WtaFamily { kWtaRefuse = 0, kWtaPlain, kWtaPacked, kWtaQuad, kWtaAny, kWtaPruned };
struct WtaChoice {
    long long grid;  // workgroups of 256 threads
    int family;      // kWtaRefuse: hipErrorInvalidValue
    // the instance's template arguments: k_wta<LPL, PPW, EXACT, MAXD, SUB> (plain and packed), k_wta_q<64 * LPL, MAXD>,
    // k_wta_pruned<PPW, MAXD, ALLD>, k_wta_any (none); those an instance does not have are 0
    int LPL, PPW, EXACT, MAXD, SUB, ALLD;
    int prune;       // the search reads the chunk minima: WtaParams::Lmin is to be passed
};
static_assert(std::has_unique_object_representations_v<WtaChoice>, "WtaChoice: integers only, no padding");
constexpr int kWtaWidestLabels = 2048;  // the widest k_wta instance (64 * kMaxLPL; mgm_wta.hip asserts it)

inline WtaChoice plan_wta(const WtaRequest &q)
{
    WtaChoice c{};
    const long long cus = q.num_cu > 0 ? q.num_cu : 256;
    const int maxd = q.NDIR <= 4 ? 4 : kMaxDirs;
    // The pruned search: the volume was a slot of the context's last dense launch, that launch wrote the chunk minima of its Lr
    // volumes (decided by plan_wta_prune for exactly this search) and the call reads that slot's volumes whole.  (sw_prune: what
    // plan_wta_prune was asked with -- a search of a slot runs in the call that launched it, or has a window.)
    c.prune = q.sw_prune != 0 && q.in_last_run != 0 && q.last_min != 0 && q.want_S == 0 && q.window == 0 && q.ragged == 0 && q.refine <= 1 && q.padded == 0 &&
              q.pix0_zero != 0 && q.compact != 0 && q.cbytes == 1 && q.L == 256 && q.lr_is_last != 0;
    if (c.prune) {
        // (what k_wta_pruned is built for, checked where it is launched from: 256 labels, no padding, one-byte compact costs, ...)
        if (q.Lreal != 256 || q.nvol_mod32 != 0) return c;
        // pw: k_wta_pruned's PPW, groups of eight pixels per wave and turn (a wave takes 8 * pw pixels, so the grid below holds up
        // to eight times the waves the pixels need: the kernel maps pixels onto whatever grid it is given, the rest end at once)
        const int pw = (q.sw_prune_ppw == 1 || (q.NDIR != 4 && q.NDIR != 8)) ? 1 : 2;
        c.grid = std::min((q.npix + 4 * pw - 1) / (4 * pw), cus * (q.sw_prune_wg > 0 ? q.sw_prune_wg : 64));
        c.family = kWtaPruned, c.PPW = pw, c.MAXD = maxd, c.ALLD = (q.NDIR == 4 || q.NDIR == 8) ? 1 : 0;
        return c;
    }
    const int per_cu = q.sw_wg_per_cu > 0 ? q.sw_wg_per_cu : 0;
    const int exact = q.Lreal == q.L ? 1 : 0;
    const bool packed = q.sw_packed != 0 && exact && (q.L == 128 || q.L == 64) && q.npix % (256 / q.L) == 0;
    // A bounded grid (workgroups of 4 waves), grid-stride beyond it.  Measured at 1920x1080 (8 / 4 directions): one pixel per
    // slab is fastest at ~768 workgroups per CU (2.99 ms at 16 -> 2.73 ms: 6.4 TB/s, the read ceiling of the part), several
    // pixels per slab at ~128 (0.83 -> 0.80 ms); far larger grids lose again.
    c.grid = std::min((q.npix + 3) / 4, cus * (per_cu ? per_cu : (packed ? 128 : 768)));  // (an upper bound: waves take several pixels per iteration)
    if (q.L > kWtaWidestLabels) {
        c.family = kWtaAny;
        return c;
    }
    // 192 / 384 labels: four / two pixels per three 256-float slabs
    if (q.sw_quad != 0 && exact && (q.L == 192 || q.L == 384) && q.npix % (768 / q.L) == 0 && q.window == 0 && q.ragged == 0 && q.refine <= 1) {
        c.grid = std::min((q.npix / (768 / q.L) + 3) / 4, cus * (per_cu ? per_cu : 256));
        c.family = kWtaQuad, c.LPL = q.L / 64, c.MAXD = maxd;
        return c;
    }
    // 128 and 64 labels: two / four pixels per 256-float slab (16-byte loads, one butterfly for all of them)
    if (packed) {
        c.family = kWtaPacked, c.LPL = 4, c.PPW = q.NDIR <= 4 ? 4 : 2, c.EXACT = 1, c.MAXD = maxd, c.SUB = 256 / q.L;
        return c;
    }
    // pixels per wave and iteration of the instances without a padding lane (up to 512 labels; 768 and 1024: one)
    int ppw = 0;
    switch (q.lpl) {
        case 1: case 2: ppw = 4; break;
        case 3: ppw = 2; break;
        case 4: ppw = 3; break;
        case 6: case 8: case 12: case 16: case 24: case 32: ppw = 1; break;
        default: return c;
    }
    c.family = kWtaPlain, c.LPL = q.lpl, c.PPW = 1, c.MAXD = kMaxDirs, c.SUB = 1;
    if (q.L == 64 * q.lpl && q.lpl <= 16) {  // (24 and 32 labels per lane: the guarded instances only)
        c.EXACT = 1, c.PPW = ppw;
        if (q.lpl <= 8 && q.NDIR <= 4 && q.sw_wide4 != 0) c.PPW = 2 * ppw, c.MAXD = 4;  // at most 4 directions: twice the slabs fit the registers
    }
    return c;
}

// the right view's search (k_wta_right / k_wta_right_any)
struct WtaRightRequest {
    int L, Lk, nx, ny, vnx, dmin, dmax, num_cu;
    int sw_right_seg, sw_right_any;  // MGM_HIP_TUNE=wta_right_seg=<right pixels per workgroup>; MGM_HIP_WTA_RIGHT_ANY=1: the diagonal walk everywhere
};
static_assert(std::has_unique_object_representations_v<WtaRightRequest>, "WtaRightRequest: integers only, no padding");
enum WtaRightFamily { kRightRefuse = 0, kRightStream, kRightDiagonal };
struct WtaRightChoice {
    long long grid;
    int family, LPL, PPW;  // k_wta_right<LPL, PPW>; the diagonal walk has no arguments (0)
    int seg, ring;         // WtaRightParams::seg / ring of the streaming kernel: right pixels per workgroup, entries of the LDS ring
};
inline WtaRightChoice plan_wta_right(const WtaRightRequest &q)
{
    WtaRightChoice c{};
    if (q.L < 1 || q.Lk < q.L || q.nx < 1 || q.ny < 1 || q.vnx < 1 || q.dmax - q.dmin + 1 != q.L) return c;
    const int cus = q.num_cu > 0 ? q.num_cu : 256;
    const int lpl = q.Lk % 64 == 0 ? q.Lk / 64 : 0;
    const bool stream = q.sw_right_any == 0 && (lpl == 1 || lpl == 2 || lpl == 3 || lpl == 4 || lpl == 6 || lpl == 8 || lpl == 12 || lpl == 16);
    if (!stream) {
        c.family = kRightDiagonal;
        c.grid = std::min(((long long)q.vnx * q.ny + 3) / 4, (long long)cus * 64);
        return c;
    }
    // Segments of a row: a workgroup re-reads the L-1 left pixels ahead of its segment, so a row is split only as far as the
    // device needs workgroups (about four per compute unit), and never below max(64, L) right pixels.
    const int want = (4 * cus + q.ny - 1) / q.ny;  // segments per row
    int seg = std::max((q.vnx + want - 1) / want, std::max(64, q.L));
    if (q.sw_right_seg > 0) seg = q.sw_right_seg;
    c.seg = std::min(seg, q.vnx);
    c.grid = (long long)q.ny * ((q.vnx + c.seg - 1) / c.seg);
    if (c.grid > 0x7fffffffll) return c;
    c.family = kRightStream, c.LPL = lpl, c.PPW = lpl <= 4 ? 2 : 1;
    c.ring = 64;
    while (c.ring < q.L - 1 + 2 * 4 * c.PPW) c.ring *= 2;
    return c;
}

// the runner-up search (k_wta_runnerup<LPL, PPW, MAXD> / k_wta_runnerup_any)
struct RunnerupRequest {
    long long npix;  // pixels of the call
    int L, Lk, NDIR, num_cu;    // labels that exist, label stride, passes; compute units of the device (0: unknown)
    int sw_any, sw_wg_per_cu;   // MGM_HIP_WTA_RUNNERUP_ANY=1: the generic kernel everywhere; MGM_HIP_WTA_RUNNERUP_WG=<workgroups per CU> (0: kRunnerupWgPerCu)
};
static_assert(std::has_unique_object_representations_v<RunnerupRequest>, "RunnerupRequest: integers only, no padding");
enum RunnerupFamily { kRunnerupRefuse = 0, kRunnerupStream, kRunnerupAny };
struct RunnerupChoice {
    long long grid;              // workgroups of 256 threads
    int family, LPL, PPW, MAXD;  // k_wta_runnerup<LPL, PPW, MAXD>; the generic kernel has no arguments (0)
};
static_assert(std::has_unique_object_representations_v<RunnerupChoice>, "RunnerupChoice: integers only, no padding");
constexpr long long kRunnerupWgPerCu = 768;
inline RunnerupChoice plan_wta_runnerup(const RunnerupRequest &q)
{
    RunnerupChoice c{};
    if (q.npix < 1 || q.L < 1 || q.Lk < q.L || q.NDIR < 1 || q.NDIR > kMaxDirs || q.sw_wg_per_cu < 0) return c;
    const long long cus = q.num_cu > 0 ? q.num_cu : 256;
    const int lpl = q.Lk % 64 == 0 ? q.Lk / 64 : 0;
    // pixels per wave and turn: those of the k_wta instances without a padding lane (plan_wta), whose registers are known to fit
    int ppw = 0;
    switch (lpl) {
        case 1: case 2: ppw = 4; break;
        case 3: ppw = 2; break;
        case 4: ppw = 3; break;
        case 6: case 8: case 12: case 16: ppw = 1; break;
        default: break;
    }
    int per_wave = 1;  // pixels a wave takes per turn of its grid-stride loop
    if (q.sw_any != 0 || ppw == 0) {  // any other stride (no multiple of 64, beyond 1024 labels), or forced
        c.family = kRunnerupAny;
    } else {
        c.family = kRunnerupStream, c.LPL = lpl, c.PPW = ppw, c.MAXD = kMaxDirs;
        if (lpl <= 8 && q.NDIR <= 4) c.PPW = 2 * ppw, c.MAXD = 4;  // at most 4 directions: twice the slabs fit the registers
        per_wave = c.PPW;
    }
    // A bounded grid (workgroups of 4 waves), grid-stride beyond it: exactly the waves the pixels need, at most plan_wta's figure
    // for one pixel per slab per CU -- the kernel reads the volumes exactly as k_wta does.  That figure is k_wta's; it has NOT
    // been measured for this kernel (the one measurement of it, against k_wta at this cap, is in docs/experiments.md,
    // "runner-up search").  The switch lowers the cap so that small volumes take several turns of the loop (tests).
    const long long waves = (q.npix + per_wave - 1) / per_wave;
    c.grid = std::min((waves + 3) / 4, cus * (q.sw_wg_per_cu > 0 ? q.sw_wg_per_cu : kRunnerupWgPerCu));
    return c;
}

// the consensus votes (k_wta_consensus<LPL, PPW, MAXD> / k_wta_consensus_any / k_wta_consensus_rel<SPL>, mgm_consensus.hip)
struct ConsensusRequest {
    long long npix;  // pixels of the call
    int L, Lk, NDIR, num_cu;    // labels that exist, label stride, passes; compute units of the device (0: unknown)
    int slots;                  // 0: the dense layout; 64 / 128: the range-proportional layout with that many label slots per pixel (L, Lk are not looked at)
    int sw_any, sw_wg_per_cu;   // MGM_HIP_WTA_CONSENSUS_ANY=1: the generic kernel everywhere; MGM_HIP_WTA_CONSENSUS_WG=<workgroups per CU> (0: the family's cap)
    int hull;                   // a ragged volume on its dense hull: the dense kernels mask by the pixel's own range.  No choice depends on it
                                // today; it is part of the request so that one that does stays this function's decision
};
static_assert(std::has_unique_object_representations_v<ConsensusRequest>, "ConsensusRequest: integers only, no padding");
enum ConsensusFamily { kConsensusRefuse = 0, kConsensusStream, kConsensusAny, kConsensusRel };
struct ConsensusChoice {
    long long grid;                   // workgroups of 256 threads
    int family, LPL, PPW, MAXD, SPL;  // k_wta_consensus<LPL, PPW, MAXD>, k_wta_consensus_rel<SPL>; those an instance does not have are 0
    int per_wave;                     // pixels a wave takes per turn of its grid-stride loop: PPW, 1 (generic), 4 (range-proportional)
};
static_assert(std::has_unique_object_representations_v<ConsensusChoice>, "ConsensusChoice: integers only, no padding");
constexpr long long kConsensusWgPerCu = kRunnerupWgPerCu, kConsensusRelWgPerCu = 64;  // (plan_wta_runnerup's and plan_wta_rel's caps)
inline ConsensusChoice plan_wta_consensus(const ConsensusRequest &q)
{
    ConsensusChoice c{};
    if (q.npix < 1 || q.NDIR < 1 || q.NDIR > kMaxDirs || q.sw_wg_per_cu < 0) return c;
    if (q.slots != 0 && q.slots != 64 && q.slots != 128) return c;
    if (q.slots == 0 && (q.L < 1 || q.Lk < q.L)) return c;
    const long long cus = q.num_cu > 0 ? q.num_cu : 256;
    long long cap = kConsensusWgPerCu;
    if (q.sw_any != 0) {  // forced: the generic kernel reads either layout
        c.family = kConsensusAny, c.per_wave = 1;
    } else if (q.slots != 0) {
        c.family = kConsensusRel, c.SPL = q.slots / 16, c.per_wave = 4;
        cap = kConsensusRelWgPerCu;
    } else {
        // the instances, their pixels per wave and turn: those of the runner-up search (plan_wta_runnerup), which keeps the costs and
        // the sum in registers besides -- what fits there fits here
        const int lpl = q.Lk % 64 == 0 ? q.Lk / 64 : 0;
        int ppw = 0;
        switch (lpl) {
            case 1: case 2: ppw = 4; break;
            case 3: ppw = 2; break;
            case 4: ppw = 3; break;
            case 6: case 8: case 12: case 16: ppw = 1; break;
            default: break;
        }
        if (ppw == 0) {  // any other stride (no multiple of 64, beyond 1024 labels)
            c.family = kConsensusAny, c.per_wave = 1;
        } else {
            c.family = kConsensusStream, c.LPL = lpl, c.PPW = ppw, c.MAXD = kMaxDirs;
            if (lpl <= 8 && q.NDIR <= 4) c.PPW = 2 * ppw, c.MAXD = 4;  // at most 4 directions: twice the slabs fit the registers
            c.per_wave = c.PPW;
        }
    }
    // A bounded grid (workgroups of 4 waves), grid-stride beyond it: exactly the waves the pixels need, at most the cap of the search
    // that reads the same volumes the same way (plan_wta_runnerup's; plan_wta_rel's on the range-proportional layout).  Neither
    // figure has been measured for these kernels.  The switch lowers the cap so that small volumes take several turns of the loop (tests).
    const long long waves = (q.npix + c.per_wave - 1) / c.per_wave;
    c.grid = std::min((waves + 3) / 4, cus * (q.sw_wg_per_cu > 0 ? q.sw_wg_per_cu : cap));
    return c;
}

// the search on the range-proportional layout (k_wta_rel<SPL, CB>): label slots per lane, bytes per cost code
struct WtaRelRequest {
    long long npix, num_cu;
    int slots, cb;
};
static_assert(std::has_unique_object_representations_v<WtaRelRequest>, "WtaRelRequest: integers only, no padding");
struct WtaRelChoice {
    long long grid;
    int SPL, CB;
};
inline WtaRelChoice plan_wta_rel(const WtaRelRequest &q)
{
    const long long groups = (q.npix + 15) / 16;  // four waves of four pixels per block
    return WtaRelChoice{std::max(1ll, std::min(groups, q.num_cu * 64)), q.slots == 128 ? 8 : 4, q.cb == 4 ? 4 : (q.cb == 2 ? 2 : 1)};
}

// ---- the speckle filter (mgm_speckle.hip) ------------------------------------------------------------------------
// Connected-component labelling by tiles: k_speckle_local labels one tile per workgroup in LDS, k_speckle_seams joins the tiles
// across their right and bottom seams (one thread per pixel pair), k_speckle_count and k_speckle_apply run one thread per pixel.
// The tile, the four grids and the scratch are decided here and nowhere else; tests/test_speckle_plan.py.
struct SpeckleRequest {
    int nx, ny;
    int num_cu;  // compute units of the device (0: unknown).  The tile is one shape today: the field is part of the request so that a
                 // tile chosen by the device's width stays this function's decision and the launcher's interface does not change
};
static_assert(std::has_unique_object_representations_v<SpeckleRequest>, "SpeckleRequest: integers only, no padding");
enum SpeckleFamily { kSpeckleRefuse = 0, kSpeckleTiles };
struct SpeckleChoice {
    long long scratch_bytes;                                 // `planes` int32 planes of nx*ny
    long long grid_local, grid_seams, grid_count, grid_apply;  // workgroups of kSpeckleThreads threads, each >= 1
    int family;
    int tw, th;      // the tile: tw x th pixels, kSpeckleThreads threads, (tw*th) / kSpeckleThreads pixels per thread
    int ntx, nty;    // tiles per axis (the last one of an axis may be ragged)
    int planes;      // int32 planes of the scratch: parent, cnt
};
static_assert(std::has_unique_object_representations_v<SpeckleChoice>, "SpeckleChoice: integers only, no padding");
constexpr int kSpeckleThreads = 256, kSpeckleTileW = 64, kSpeckleTileH = 16, kSpecklePlanes = 2;
constexpr long long kSpeckleMaxPixels = 2147483647ll;  // pixel indices and component sizes are int32
inline SpeckleChoice plan_speckle(const SpeckleRequest &q)
{
    SpeckleChoice c{};
    if (q.nx < 1 || q.ny < 1 || (long long)q.nx * q.ny > kSpeckleMaxPixels) return c;
    const long long npix = (long long)q.nx * q.ny;
    c.family = kSpeckleTiles;
    c.tw = kSpeckleTileW, c.th = kSpeckleTileH;
    c.ntx = (int)(((long long)q.nx + c.tw - 1) / c.tw), c.nty = (int)(((long long)q.ny + c.th - 1) / c.th);  // (nx + tw may pass 2^31)
    c.planes = kSpecklePlanes;
    c.scratch_bytes = (long long)c.planes * npix * 4;
    // pixel pairs across the seams: (ntx - 1) vertical seams of ny pairs, (nty - 1) horizontal seams of nx pairs (a single tile: none,
    // and a grid of one workgroup whose threads all leave)
    const long long pairs = (long long)(c.ntx - 1) * q.ny + (long long)(c.nty - 1) * q.nx;
    c.grid_local = (long long)c.ntx * c.nty;
    c.grid_seams = std::max(1ll, (pairs + kSpeckleThreads - 1) / kSpeckleThreads);
    c.grid_count = c.grid_apply = (npix + kSpeckleThreads - 1) / kSpeckleThreads;
    return c;
}

// ---- hole filling (mgm_holes.hip) ----------------------------------------------------------------------------------
// Per direction a running "last valid pixel" along rows, columns and diagonals: k_holes_rows takes a row per wave in chunks of
// `chunk` pixels (directions 0, 1); k_holes_carry / k_holes_walk take one lane per column or diagonal and one band of `band` rows
// per workgroup row (directions 2..7: first every band's carry-out, then every band from its carry-in); k_holes_apply runs one
// thread per pixel.  The chunk, the band, the grids and the scratch are decided here and nowhere else; tests/test_holes_plan.py.
struct HolesRequest {
    int nx, ny;
    int dirs;    // 2, 4 or 8
    int num_cu;  // compute units of the device (0: unknown).  Chunk and band are one choice per shape today: the field is part of the
                 // request so that a choice by the device's width stays this function's decision
};
static_assert(std::has_unique_object_representations_v<HolesRequest>, "HolesRequest: integers only, no padding");
enum HolesFamily { kHolesRefuse = 0, kHolesLines };
struct HolesChoice {
    long long scratch_bytes;  // 4 * (planes * nx*ny + 2 * carry_words)
    long long grid_rows;      // k_holes_rows: workgroups of kHolesThreads threads, one wave per (row, direction 0 / 1)
    long long grid_walk;      // k_holes_carry, k_holes_walk: workgroups along the lines; the launch is grid_walk x nbands x walk_dirs
    long long grid_apply;     // k_holes_apply: one thread per pixel
    long long nlines;         // lanes of a band: nx + ny - 1 diagonals (the columns are the first nx of them)
    long long carry_words;    // words of ONE carry plane (positions int32, values float): walk_dirs * nbands * nlines
    int family;
    int chunk;      // pixels of a row that a wave takes at a time
    int band;       // rows per band
    int nbands;     // bands (the last one may be ragged); at most `band` of them, see plan_holes
    int walk_dirs;  // directions 2 .. dirs-1: 0, 2 or 6
    int planes;     // candidate planes of nx*ny floats: dirs
};
static_assert(std::has_unique_object_representations_v<HolesChoice>, "HolesChoice: integers only, no padding");
constexpr int kHolesThreads = 256, kHolesChunk = 64, kHolesMinBand = 64;  // (the chunk is a wave's width: one pixel per lane)
constexpr long long kHolesMaxPixels = 2147483647ll;  // pixel coordinates, distances and line indices are int32 / fit 2^32
inline HolesChoice plan_holes(const HolesRequest &q)
{
    HolesChoice c{};
    if (q.nx < 1 || q.ny < 1 || (long long)q.nx * q.ny > kHolesMaxPixels) return c;
    if (q.dirs != 2 && q.dirs != 4 && q.dirs != 8) return c;
    const long long npix = (long long)q.nx * q.ny;
    c.family = kHolesLines;
    c.chunk = kHolesChunk;
    // the band: at least kHolesMinBand rows and at least sqrt(ny), so that there are never more bands than a band has rows -- the
    // walk kernel looks back over the earlier bands' carry-outs, at most nbands - 1 of them per lane, which then costs no more than
    // the band's own walk
    long long b = kHolesMinBand;
    while (b * b < q.ny) b++;
    c.band = (int)b;
    c.nbands = (int)((q.ny + b - 1) / b);
    c.walk_dirs = q.dirs - 2;
    c.planes = q.dirs;
    c.nlines = (long long)q.nx + q.ny - 1;
    c.carry_words = (long long)c.walk_dirs * c.nbands * c.nlines;
    c.scratch_bytes = 4 * ((long long)c.planes * npix + 2 * c.carry_words);
    c.grid_rows = (2ll * q.ny * kHolesChunk + kHolesThreads - 1) / kHolesThreads;
    c.grid_walk = (c.nlines + kHolesThreads - 1) / kHolesThreads;
    c.grid_apply = (npix + kHolesThreads - 1) / kHolesThreads;
    return c;
}

// ---- hole classification (k_holes_classify, mgm_holes.hip) -----------------------------------------------------------
// A workgroup takes `seg` pixels of a row at a time (one per thread) and stages the other view's landing coordinates of the columns
// the segment's holes can name -- [x0 + dmin, x1 + dmax] cut to the other view -- in LDS, `span` of them at a time: a label range
// of any length L is a loop over spans, never a larger allocation.  The launch is grid_x segments x grid_y workgroup rows; a
// workgroup row strides over the image rows.  tests/test_occlusion_model.py.
struct HolesClassifyRequest {
    int nx, ny;   // the map with holes
    int vnx;      // the other view's width (its height is ny)
    int num_cu;   // compute units of the device (0: unknown); one choice per shape today, as in HolesRequest
    long long L;  // labels of the range: dmax - dmin + 1 >= 1 (64 bits: the difference of two ints)
};
static_assert(std::has_unique_object_representations_v<HolesClassifyRequest>, "HolesClassifyRequest: integers only, no padding");
struct HolesClassifyChoice {
    long long grid_x;     // segments of a row
    long long grid_y;     // workgroup rows: min(ny, kHolesClsMaxRows); workgroup row r takes the image rows r, r + grid_y, ...
    int lds_bytes;        // 4 * (span + seg + kHolesClsWords): landing coordinates, the segment's hole list, the waves' counts
    int family;           // kHolesRefuse or kHolesLines (the one kernel there is)
    int seg;              // pixels of a row per workgroup and turn: kHolesThreads
    int span;             // landing coordinates staged at a time: a multiple of the wave's width, at most kHolesClsMaxSpan
};
static_assert(std::has_unique_object_representations_v<HolesClassifyChoice>, "HolesClassifyChoice: integers only, no padding");
constexpr int kHolesClsMaxSpan = 1024, kHolesClsMaxRows = 65535, kHolesClsWords = 8;
inline HolesClassifyChoice plan_holes_classify(const HolesClassifyRequest &q)
{
    HolesClassifyChoice c{};
    if (q.nx < 1 || q.ny < 1 || (long long)q.nx * q.ny > kHolesMaxPixels) return c;  // (what plan_holes refuses)
    if (q.vnx < 1 || q.L < 1) return c;
    c.family = kHolesLines;
    c.seg = kHolesThreads;
    // the columns one full segment can name: seg + L - 1 (L is at most 2^32: no overflow in 64 bits), never more than the other view has
    const long long want = std::min<long long>(std::min<long long>(q.L, kHolesClsMaxSpan) + c.seg - 1, q.vnx);
    c.span = (int)std::min<long long>(kHolesClsMaxSpan, (want + kHolesChunk - 1) / kHolesChunk * kHolesChunk);
    c.grid_x = ((long long)q.nx + c.seg - 1) / c.seg;
    c.grid_y = std::min<long long>(q.ny, kHolesClsMaxRows);
    c.lds_bytes = 4 * (c.span + c.seg + kHolesClsWords);
    return c;
}

// ---- sub-pixel label spacing (k_cv_interleave, mgm_subpix.hip) -----------------------------------------------------
// The fine volume F(p, o') = C_{o' mod s}(p, o' div s) is GATHERED from the s phase volumes at once: a workgroup takes `pix`
// consecutive pixels and writes their rows of F -- one contiguous span of memory -- in chunks of `vec` costs per thread, every chunk
// one aligned 16-byte store, reading each phase's rows of the same pixels (contiguous as well).  One-byte codes: a row has `slots`
// label slots (a multiple of 64: the compact or the padded compact form), the slots beyond `labels` get the code of +INF; fp32: a row
// has exactly `labels` floats, so rows are only 4-byte aligned and the chunks are cut from the workgroup's span instead (pix is a
// multiple of four: the span starts 16-byte aligned).  The pixels per workgroup, the grid and the family are decided here and
// nowhere else; tests/test_subpix_plan.py.
struct SubpixRequest {
    long long npix;  // pixels of the volume
    int labels;      // L' = s * (L - 1) + 1 labels of the fine volume
    int slots;       // label slots of a pixel's row of F: cb = 1: labels or the padded count (a multiple of 64); cb = 4: labels
    int in_slots;    // label slots of a pixel's row of a phase volume (>= L = (labels - 1) / s + 1; cb = 4: exactly L)
    int s;           // phases: 2 or 4
    int cb;          // bytes per cost of the form the phases are in and F gets: 1 (codes) or 4 (fp32)
    int num_cu;      // compute units of the device (0: unknown); one choice per shape today, as in HolesRequest
};
static_assert(std::has_unique_object_representations_v<SubpixRequest>, "SubpixRequest: integers only, no padding");
enum SubpixFamily { kSubpixRefuse = 0, kSubpixCodes, kSubpixFloats };
struct SubpixChoice {
    long long grid;  // workgroups of kSubpixThreads threads; workgroup b takes the pixels [b * pix, min(npix, (b + 1) * pix))
    int family;
    int pix;         // pixels per workgroup
    int vec;         // costs per thread and chunk: 16 codes or 4 floats (16 bytes either way)
    int chunks;      // chunks of a full workgroup: pix * slots / vec (codes: whole rows; floats: the last one may be cut)
};
static_assert(std::has_unique_object_representations_v<SubpixChoice>, "SubpixChoice: integers only, no padding");
constexpr int kSubpixThreads = 256, kSubpixSpanBytes = 16384;  // bytes of F per workgroup, at least: four chunks per thread
constexpr int kSubpixMaxLabels = 1 << 22;                      // (kMaxLabels, mgm_device.h: what mgm_cv_create admits)
inline SubpixChoice plan_subpix(const SubpixRequest &q)
{
    SubpixChoice c{};
    if (q.npix < 1 || q.labels < 1 || q.labels > kSubpixMaxLabels || (q.s != 2 && q.s != 4) || (q.labels - 1) % q.s) return c;
    const int L = (q.labels - 1) / q.s + 1;  // labels of a phase volume
    long long pix;
    if (q.cb == 1) {
        if (q.slots < q.labels || q.slots % 64 || q.in_slots < L || q.in_slots % 64) return c;
        c.family = kSubpixCodes, c.vec = 16;
        pix = std::max<long long>(1, (kSubpixSpanBytes + q.slots - 1) / q.slots);
    } else if (q.cb == 4) {
        if (q.slots != q.labels || q.in_slots != L) return c;
        c.family = kSubpixFloats, c.vec = 4;
        pix = std::max<long long>(1, (kSubpixSpanBytes / 4 + q.labels - 1) / q.labels);
        pix = (pix + 3) / 4 * 4;
    } else {
        return c;
    }
    // (the costs of a workgroup index in 32 bits: at most 4 * 2^22 floats, or 16384 + slots codes)
    const long long grid = (q.npix + pix - 1) / pix;
    if (grid > 2147483647ll) return SubpixChoice{};
    c.grid = grid, c.pix = (int)pix;
    c.chunks = (int)((pix * q.slots + c.vec - 1) / c.vec);
    return c;
}

// ---- which kernels take an aggregation call ----------------------------------------------------------------------------------
// Three decisions that need facts only the device knows (the weights' values, whether a volume's compact or range-proportional copy
// is usable, whether a padded copy fits a compact form), and must not ask for one they can do without: a call that is no candidate
// for the range-proportional kernels never scans its weights for them, a padded launch tries two-byte costs only after one-byte
// costs failed.  So ONE protocol: a fact of the device starts as -1 in the request ("not probed"), and the planner returns either a
// finished decision (need == kNeedNothing) or the one fact it wants next; the driver (mgm_api.hip, mgm_plan.hip) probes it, writes
// it into the request and asks again.  The floats of a call enter as the predicates the code has always used.  tests/test_route_plan.py
// holds the three to a transcription of the control flow they replace, probe for probe.
enum PlanNeed {
    kNeedNothing = 0,
    kNeedWeightValues,  // the weights' values, all volumes in one scan
    kNeedRelCopy,       // volume `arg`: is its range-proportional copy usable, and in which format (rel_resolve)
    kNeedCompactCopy,   // volume `arg`: its compact copy and whether it holds NaN costs (c8_resolve)
    kNeedPadTry,        // do the padded copies of all volumes fit compact costs of `arg` bytes (k_pad + read-back)
};

// the range-proportional kernels (run_rel) or the dense hull (run_passes)?
struct RouteRequest {
    int n, MGM, fh, want_S;
    int weights_given;                  // the call has weight images
    int p1_nonneg, p2_nonneg, p2_finite;  // P1 >= 0, P2 >= 0, P2 < +INF
    int only_rel;                       // every volume's ONLY copy is the range-proportional one
    int rel_enabled;                    // MGM_HIP_REL / tune rel: not 0
    int sw_rel, sw_rel_tie, sw_rel_S, sw_rel_fh2;  // tune rel, rel_tie, rel_S, rel_fh2
    int w_odd, w_any;                   // (device) some weight is not positive and finite; some weight is not 1
    int rel_usable[kMaxBatch], rel_slots[kMaxBatch], rel_cb[kMaxBatch];  // (device) per volume, after rel_resolve
};
static_assert(std::has_unique_object_representations_v<RouteRequest>, "RouteRequest: integers only, no padding");
enum { kRouteDense = 0, kRouteRel = 1 };
struct RouteDecision {
    int need, arg;
    int route, rel_weighted;  // rel_weighted: the range-proportional launch runs its weighted kernels (0 on the dense route, which decides for itself)
};
inline RouteDecision plan_agg_route(const RouteRequest &q)
{
    RouteDecision d{};
    const bool fh = q.fh != 0;
    // (round 6: with slope 1, two strips and the 5.6 ms launch the tie is gone: every usable copy is walked; tune rel_tie=0 restores round 5's rule)
    const bool rel_pays = fh || q.weights_given || q.n >= 2 || q.only_rel || q.sw_rel >= 2 || q.sw_rel_tie != 0;
    //  the hand-off of k_pass_rel keeps the launch's tag in the sign bit of every published word, so every L / E / minimum
    // must be >= +0: non-negative penalties and, for weighted launches, positive finite weights: anything else takes the dense kernels.
    bool sign_ok = q.p1_nonneg && q.p2_nonneg;
    bool weighted = q.weights_given != 0;
    const bool candidate = (!q.want_S || q.sw_rel_S != 0) && q.p2_finite && rel_pays && sign_ok && q.rel_enabled;
    if (candidate && weighted) {
        if (q.w_odd < 0) return d.need = kNeedWeightValues, d;
        sign_ok = !q.w_odd;
        if (q.MGM == 2 && !q.w_any) weighted = false;  // planes of ones: the reference runs unweighted
    }
    const bool fn_ok = q.MGM != 2 || weighted || !fh || q.sw_rel_fh2 != 0;  // (update_cost2_trunclinear: k_pass_rel FH2)
    if (!(candidate && sign_ok && fn_ok)) return d;
    for (int v = 0; v < q.n; v++) {  // (one format per launch; the first volume that fails ends the asking)
        if (q.rel_usable[v] < 0) return d.need = kNeedRelCopy, d.arg = v, d;
        if (!(q.rel_usable[v] && q.rel_slots[v] == q.rel_slots[0] && q.rel_cb[v] == q.rel_cb[0])) return d;
    }
    // the one combination whose LDS rings do not fit a CU: update_cost2_trunclinear ([L][F][B] entries) on 128 slots of fp32 costs
    // (116 KB of rings + 64 KB of cost pieces): the dense hull keeps it
    if (fh && q.MGM == 2 && !weighted && q.rel_slots[0] == 128 && q.rel_cb[0] == 4) return d;
    d.route = kRouteRel, d.rel_weighted = weighted ? 1 : 0;
    return d;
}

// The sub-batches of a call.  The Lr volumes of a launch take NDIR x W x H x label slots floats per volume; a batch that does not
// fit the caller's workspace limit is run as several launches over the largest sub-batches that do, and one the device cannot hold
// (MGM_ERR_NOMEM) in halves.  The two routes differ in their allowances and their rounding, and keep them:
//   * dense: + ~7 % of hand-off slots, + the chunk minima where a launch may write them (one float per 32 of Lr); multiples of
//     four volumes, else two, so that volumes keep sharing waves at 64 / 128 labels; halves stay even above four;
//   * range-proportional: + ~16 % (two hand-off lines per band on the anti-diagonal passes); no rounding.
struct SubbatchRequest {
    long long npix, ws_limit, lr_pad;  // pixels; mgm_ctx_set_workspace_limit (0: none); floats between Lr volumes (lr_pad_floats)
    int route, n, NDIR;
    int L, rel_slots;                  // labels of the volumes; label slots of their range-proportional format
    int want_S, refine, prune_enabled;  // what the minima term asks (plan_wta_prune)
};
static_assert(std::has_unique_object_representations_v<SubbatchRequest>, "SubbatchRequest: integers only, no padding");
inline int plan_subbatch(const SubbatchRequest &q)
{
    int chunk = q.n;
    if (!q.ws_limit) return chunk;
    if (q.route == kRouteRel) {
        const double per_vol = 4.0 * ((double)q.npix * q.rel_slots + (double)q.lr_pad) * q.NDIR * 1.16;
        while (chunk > 1 && per_vol * chunk > (double)q.ws_limit) chunk--;
        return chunk;
    }
    const int Lk = padded_labels(q.L) ? padded_labels(q.L) : q.L;
    const double per_vol = 4.0 * ((double)q.npix * Lk + (double)q.lr_pad) * q.NDIR *
                           (1.07 + ((q.L == 256 && !q.want_S && q.refine <= 1 && q.prune_enabled) ? 1.0 / kChunkLabels : 0.0));
    while (chunk > 1 && per_vol * chunk > (double)q.ws_limit) chunk--;
    if (chunk >= 4) chunk -= chunk % 4;
    else if (chunk == 3) chunk = 2;
    return chunk;
}
inline int shrink_after_nomem(int route, int m)  // a launch of m > 1 volumes did not fit the device
{
    if (route == kRouteRel) return std::max(1, m / 2);
    return std::max(m > 4 ? (m / 2) - (m / 2) % 2 : m / 2, 1);
}

// What the volumes and weights of a dense launch ARE, and with that, which kernels can take them (run_passes, stage 1).
struct DenseKernelsRequest {
    int nb, MGM, fh, allow_pad, Lreal;
    int p1_nonneg, p2_nonneg, p2_finite;
    int force_build;                    // mgm_ctx::force_build (1: the first build only)
    int lines_real, lines_pad;          // pass2_lines(Lreal, false); pass2_lines(padded_labels(Lreal), false), 0 if there is none
    int lpl_real, lpl_pad;              // pass_lpl of the two
    int sw_pad, sw_c8, sw_deep;         // DevSwitches
    int weights_given;                  // the call has weight images ...
    int w_given[kMaxBatch];             // ... for this volume
    int ragged, nan_words, same_hull;   // some volume has per-pixel ranges / costs that are descriptor words; all volumes share dmin
    int p8_valid[kMaxBatch], p8_L[kMaxBatch], p8_cb[kMaxBatch];  // the padded compact copy the cost kernel wrote (mgm_cv::p8)
    int pad_hint;                       // the first volume's mgm_cv::pad_hint
    // (device) the weights' values per volume: some != 1; some not positive and finite; the values != 1 are ONE value
    int w_not_one[kMaxBatch], w_odd[kMaxBatch], w_one_other[kMaxBatch];
    // (device) c8_resolve per volume: compact copy usable, its bytes per cost, NaN costs found
    int c8_use[kMaxBatch], c8_bytes[kMaxBatch], nan_found[kMaxBatch];
    int pad_fits[3];                    // (device) [bytes per cost]: the padded copies fit that compact form
};
static_assert(std::has_unique_object_representations_v<DenseKernelsRequest>, "DenseKernelsRequest: integers only, no padding");
enum { kDenseOk = 0, kDenseMixedWeights, kDenseRaggedHulls, kDenseFh2NeedsSecondBuild };
struct DenseKernels {
    int need = kNeedNothing, arg = 0, err = kDenseOk;
    int exact = 0;        // the slow operand-order-faithful kernel takes the call (run_passes_exact)
    int first_build = 0;  // the first build only
    int L = 0;            // label slots the kernels see (padded launch: the next count of the second build)
    int padded = 0, own_padded = 0;  // ... padded; every volume carries the padded compact copy K2 wrote (mgm_cv::p8)
    int use_c8 = 1, cb = 1;          // compact costs of this many bytes
    int weighted = 0, weighted_given = 0;  // the weighted kernels run; the caller's weights hold a value != 1
    int w2cand = 0;       // every weighted volume's weights are 1 and ONE other positive finite value
    int ragged = 0, fh2_ragged = 0;
    int borrow_ones = 0;  // a ragged FH launch without weights borrows the weighted kernels with all-ones weights
    int need_pad_f32 = 0;  // the launch reads padded fp32 copies (pad_f32)
    int pad_hint = -1;    // >= 0: what the pad tries found, to be remembered in the volumes (mgm_cv::pad_hint)
};
constexpr int kFastKernelLabels = 2048;  // no fast pass kernel is built wider (64 * kMaxLPL; mgm_plan.hip asserts it)
inline DenseKernels plan_dense_kernels(const DenseKernelsRequest &q)
{
    DenseKernels d;
    auto ask = [](int need, int arg) { DenseKernels a; return a.need = need, a.arg = arg, a; };
    auto refuse = [](int err) { DenseKernels a; return a.err = err, a; };
    const bool fh = q.fh != 0, ragged = q.ragged != 0;
    // The second build's unweighted kernels keep the sign bit of the slabs they hand from band to band for a validity
    // tag, which needs E = T - m >= +0, i.e. non-negative penalties (mgm_pass2.hip, TAGS): anything else takes the first build.
    const bool first_build = q.force_build == 1 || !q.p1_nonneg || !q.p2_nonneg;
    // A label count the second build does not take (not 64, 128, 192, 256, 384 or 512) runs PADDED: the kernels see
    // the next such count, the extra label slots hold +INF costs -- "no such label", exactly what a read past a Dvec
    // returns (dvec.cc:129) -- and stay +INF through every update: C = +INF there and every pixel of a volume with a
    // uniform range has a finite minimum, so the added term is finite.
    // (weights with more than 512 labels run on the first build, which takes any label count as it is: no padding then)
    const bool padded = q.allow_pad && !first_build && q.lines_real == 0 && q.sw_pad && !(q.weights_given && q.Lreal > 512) && padded_labels(q.Lreal) != 0;
    const int L = padded ? padded_labels(q.Lreal) : q.Lreal, lpl = padded ? q.lpl_pad : q.lpl_real;
    d.first_build = first_build, d.L = L, d.padded = padded, d.ragged = ragged;

    // weighted? (mgm_core.cc:420-423: any value != 1.0 switches every update) -- and what values do the weights take: the
    // planes compute_mgm_weights makes hold 1 and ONE other value, which the pass kernel exploits (k_pass2, W2)
    bool weighted = false, w2cand = false, wodd = false;  // wodd: a weight that is not positive and finite (<= 0, NaN, INF)
    if (q.weights_given) {
        if (q.w_not_one[0] < 0) return ask(kNeedWeightValues, 0);
        w2cand = true;
        for (int v = 0; v < q.nb; v++) {
            const bool wv = q.w_given[v] && q.w_not_one[v];
            // Planes of ones beside real weights: with TSGM != 2 the reference calls the SAME update function either way
            // (update_costW[_trunclinear] with DeltaI = 1.0, mgm_core.cc:563-575), so the launch simply runs weighted; with
            // TSGM = 2 the unweighted volume is update_cost2's, a different function: not in one launch.
            if (v && wv != weighted && (q.MGM == 2 || !q.w_given[v])) return refuse(kDenseMixedWeights);
            weighted = weighted || wv;
            wodd = wodd || (wv && q.w_odd[v]);
            w2cand = w2cand && (!wv || (!q.w_odd[v] && q.w_one_other[v]));
        }
        w2cand = w2cand && weighted;
    }
    d.weighted_given = weighted;  // (before the ragged FH path borrows the weighted kernels below)
    // Volumes whose aggregation can meet NaNs take the slow kernel that keeps the operand order of the reference's minima
    // (mgm_pass_exact.hip; the fast builds are compiled NaN-free):
    //   * costs that are descriptor WORDS differenced as floats (-p census with a non-census distance, > 24 bits);
    //   * a ragged volume with P2 = +INF: the dense layout relies on every slab keeping a finite minimum, which a finite
    //     P2 guarantees (every term is capped at m + P2); with P2 = +INF a pixel whose neighbours' ranges miss its own gets
    //     an all-INF slab and the next one INF - INF = NaN;
    //   * (found below, by the scan of an uploaded volume) NaN costs.
    //   * more than 2048 labels: no fast kernel is built that wide (the reference's Dvec has no label limit, dvec.cc:60).
    //   * (round 6, found by the ragged parity tests of tests/) FH potentials on a ragged volume with a NEGATIVE slope -- P1 < 0, or a
    //     weight <= 0 / NaN scaling it: the fast kernels mask the neighbour's slab to the receiving pixel's range and convolve
    //     over the whole hull, which equals the reference's convolution over the range (mgm_core.cc:242-271) only while the
    //     ramp the forward pass leaves ABOVE the range cannot flow back into it (M[rh] + 2 P1 >= M[rh]).
    d.exact = (ragged && !q.p2_finite) || q.Lreal > kFastKernelLabels || (ragged && fh && (!q.p1_nonneg || wodd)) || q.nan_words;
    if (d.exact) return d;
    if (fh && ragged && !q.same_hull) return refuse(kDenseRaggedHulls);
    // FH potentials on a ragged volume: the min-convolution runs over the RECEIVING pixel's range (mgm_core.cc:242-271), so
    // it cannot be done once by the producer.  The weighted FH kernels convolve on the consumer side anyway: use them,
    // with all-ones weights if the caller has none (update_costW_trunclinear with DeltaI = 1 is what the reference calls
    // then, mgm_core.cc:563-570) -- except for TSGM = 2 without weights, which is update_cost2_trunclinear with its
    // boundary fix-up (166-186, 197-219): the second build has it (combine_fh2_ragged); the first build does not
    if (fh && ragged && !weighted) {
        d.fh2_ragged = q.MGM == 2;
        if (d.fh2_ragged && (first_build || (padded ? q.lines_pad : q.lines_real) == 0)) return refuse(kDenseFh2NeedsSecondBuild);
        d.borrow_ones = 1;
        weighted = true;
    }
    d.weighted = weighted, d.w2cand = w2cand;

    // compact costs when the volumes allow it (c8_resolve also resolves mgm_cv::nan_state: one scan per filling of a volume)
    for (int v = 0; v < q.nb; v++)
        if (q.c8_use[v] < 0) return ask(kNeedCompactCopy, v);
    for (int v = 0; v < q.nb; v++) d.exact |= q.nan_found[v] != 0;
    if (d.exact) return d;
    bool use_c8 = true;
    int cb = 1;  // bytes per compact cost of this launch
    // padded launch whose volumes all carry the padded compact copy K2 wrote (mgm_cv::p8): nothing to pad or encode
    bool own_padded = padded && q.sw_c8;
    for (int v = 0; v < q.nb && own_padded; v++) own_padded = q.p8_valid[v] && q.p8_L[v] == L && q.p8_cb[v] == q.p8_cb[0];
    if (own_padded) {
        cb = q.p8_cb[0];
    } else if (padded) {
        // padded copies of the costs: a compact form if every volume allows it -- the one that worked for the first volume
        // last time first (mgm_cv::pad_hint), then the other --, else fp32
        const int tries[3] = {q.pad_hint == 0 ? 0 : (q.pad_hint == 2 ? 2 : 1), q.pad_hint == 2 ? 1 : 2, 0};
        use_c8 = false;
        for (int t = 0; t < 3 && q.sw_c8 && !use_c8; t++) {
            const int tb = tries[t];
            if (tb == 0 || (tb == 2 && L > 512)) break;
            if (q.pad_fits[tb] < 0) return ask(kNeedPadTry, tb);
            if (q.pad_fits[tb]) use_c8 = true, cb = tb;
        }
        d.pad_hint = use_c8 ? cb : 0;
        d.need_pad_f32 = !use_c8;
    } else {
        for (int v = 0; v < q.nb; v++) use_c8 = use_c8 && q.c8_use[v] && q.c8_bytes[v] == q.c8_bytes[0];
        cb = use_c8 ? q.c8_bytes[0] : 1;
    }
    // Two bytes per cost: read by the unweighted kernels with deep rings that publish E, up to 512 labels (k_pass2, C8 == 2);
    // everything else reads the fp32 volume.  Since round 4 K2 writes AD / SD volumes compact-ONLY (f32_state 0), so a
    // weighted launch, FH with TSGM = 2 or a shallow-ring launch on such a volume pays an expansion (ensure_f32: k_expand
    // plus a W*H*L fp32 allocation) the first time -- correct, but four times the cost bytes; bench.py's cost_bytes prices
    // weighted launches on fp32 costs for that reason.
    if (use_c8 && cb == 2 && (weighted || (fh && q.MGM == 2) || lpl > 8 || q.sw_deep == 0)) {
        own_padded = false;
        if (padded) d.need_pad_f32 = 1;
        use_c8 = false;
    }
    // (768 / 1024 labels with weights that are not two-valued-and-narrow: the weighted kernels of the second build stop at
    // 512 labels -- two slabs per slot do not fit the LDS beyond -- so those take the first build, which has no compact costs)
    if (first_build || (weighted && lpl > 8)) use_c8 = false;
    d.use_c8 = use_c8, d.cb = cb, d.own_padded = own_padded;
    return d;
}

}  // namespace mgm
