// mgm_host.h -- host-side internals shared by the translation units behind the C ABI of libmgm_hip.so
// (mgm_ctx.hip: contexts, images, switches, timing; mgm_fillplan.h: how a cost volume gets filled, as pure functions of a
// request; mgm_volume.hip: the volumes -- the stages of a filling around that plan and everything that allocates, converts or
// invalidates one of a volume's copies; mgm_planner.h: the launch plan of the pass kernels as pure functions of a request;
// mgm_plan.hip: the stages of a pass launch around it, the plans' caches and the winner search, planned there too; mgm_api.hip: weights,
// aggregation calls, the steps around them).  Nothing here is exported through include/mgm_hip.h; no compute happens on the
// host and there is no CPU fallback.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mgm_hip.h"
#include "mgm_device.h"
#include "mgm_energyplan.h"
#include "mgm_fillplan.h"
#include "mgm_planner.h"

using namespace mgm;

struct mgm_img {
    float *d;
    int nx, ny, nch;
    int device;  // the device the pixels live on (mgm_img_device)
};
struct mgm_cv {
    float *d;
    int nx, ny, dmin, dmax;
    // compact (one byte per cost) copy used by K3 / k_wta when every cost is an integer 0..254 or +INF
    uint8_t *d8 = nullptr;
    int cbytes = 1;            // bytes per cost of the compact copy: 1 (0..254, 255 = +INF) or 2 (0..65534, 65535 = +INF; round 4:
                               // absolute differences of colour pairs, squared differences)
    size_t d8_cap = 0;         // bytes allocated at d8
    mutable int pad_hint = 1;  // a label count that runs padded: the compact form its padded copy took last time (0: none did)
    unsigned *bad8 = nullptr;  // device word: 1 = not representable
    CopyState c8_state = CopyState::None;  // (mgm_fillplan.h: none, written and not checked, valid, invalid)
    // K2 skips the fp32 write when its costs are known to fit the compact form (single-word census):
    // nothing on the hot path reads `d` then, and it is decoded from d8 if somebody asks for it.
    int f32_state = 1;         // 1 current, 0 stale (d8 holds the volume)
    FillMemory mem;            // what the next filling starts from (mgm_fillplan.h): diff_fails, diff_wide, rel_hint_slots
    // A label count that the pass kernels run PADDED (151 -> 192, ...): K2 may write the padded compact copy itself --
    // [npix][p8_L] costs of p8_cb bytes, the label slots beyond the real count +INF -- instead of an fp32 volume that every
    // aggregation call pads and encodes again (run_passes).  p8_state Valid (and then the ONLY copy until somebody asks
    // for the fp32 volume: f32_state 0), else None.
    uint8_t *p8 = nullptr;
    size_t p8_cap = 0;
    int p8_L = 0, p8_cb = 1;
    CopyState p8_state = CopyState::None;  // (None or Valid)
    mgm_ctx *owner = nullptr;
    // ragged volume: the per-pixel range images it was built from (device, nx*ny floats each), else nullptr.
    // dmin/dmax are then the hull of all ranges; labels outside a pixel's own range hold +INF.
    float *rlo = nullptr, *rhi = nullptr;
    // built by `-p census` with a non-census distance from descriptors of more than 24 bits: costs are differences of
    // descriptor WORDS read as floats (mgm_costvolume.h:355-362), NaN patterns included.  The volume itself is
    // reproduced bit for bit; what the reference's aggregation makes of NaN costs depends on operand order.
    bool nan_words = false;
    // Does the volume hold NaN costs?  The scan-line kernels are compiled NaN-free (mgm_pass_common.h) and what the
    // reference makes of a NaN cost depends on the operand order of its minima, so such a volume is refused by
    // mgm_aggregate* instead of being aggregated into something unspecified.  0 not scanned (uploaded / written through
    // mgm_cv_device_ptr), 1 flag word on the device is current but not read back, 2 clean, -1 holds NaN.
    CopyState nan_state = CopyState::None;
    // bumped whenever the contents may have changed: contexts remember (pointer, generation) of the volumes of their
    // last aggregation, so a refilled volume, or a new one at a recycled address, is not mistaken for one of them
    unsigned long long gen = 0;
    // ragged volume, range-proportional copy (round 5; mgm_pass_rel.hip): 64 cost bytes per pixel placed at its own window +
    // a 16-byte record per pixel (disparity of slot 0, lo, hi) + a flag word, one allocation [npix*64 bytes][npix*16 bytes][flag]; rel_state 0 none, 1 written (flag
    // not read back yet), 2 usable, -1 not usable (a window wider than 62 labels, a cost that is not a byte)
    // (round 6) the copy's FORMAT: rel_slots = 64 or 128 label slots per pixel (windows of up to 62 / 126 labels), rel_cb = 1 or 2 bytes
    // per cost code; [npix * rel_slots * rel_cb bytes of costs][npix * 16 bytes of records][flag word].  A gathered copy starts in the
    // narrowest form its cost function allows and is gathered again wider if the flag word asks for it (rel_resolve).
    uint8_t *relbuf = nullptr;
    size_t rel_cap = 0;
    CopyState rel_state = CopyState::None;
    int rel_slots = 64, rel_cb = 1;
    size_t rel_cost_bytes() const { return (size_t)nx * ny * (size_t)rel_slots * (size_t)rel_cb; }
    int *rel_records() const { return reinterpret_cast<int *>(relbuf + rel_cost_bytes()); }
    unsigned *rel_flag() const { return reinterpret_cast<unsigned *>(relbuf + rel_cost_bytes() + (size_t)nx * ny * 16); }
    // the relative copy is the ONLY copy (single-word census: K2 wrote it straight from the descriptors, f32_state 0);
    // ensure_f32 expands it into the dense hull on demand
    bool rel_only = false;
    // a caller-provided volume whose refill FAILED half-way holds neither its old costs nor new ones: mgm_aggregate*
    // refuses it (MGM_ERR_INVALID) until a later mgm_costvolume_build* has filled it
    bool unfilled = false;
};
unsigned long long next_cv_generation();

struct Buf {  // grow-only device scratch
    void *p = nullptr;
    size_t cap = 0;
};
struct HandRegion { Buf buf; HandTags tags; };  // a region of self-validating hand-off slots and what its words carry (mgm_planner.h)

// The task tables of earlier launches, by the request they were planned for (mgm_planner.h): request -> (plan, device table).
// Bounded: the oldest entry is dropped (cache_put, mgm_plan.hip, which synchronises before it frees a buffer).  A caller that
// launches the passes of a volume one by one alternates between eight of them.
template <class Req, class Plan>
struct PlanCache {
    struct Entry {
        Req req;
        Plan plan;  // the decisions; its ticket order and table live on the device only (buf: plan.ntasks items behind the header)
        Buf buf;
        unsigned long long fnv;  // FNV-1a of the table's bytes (show_plan)
    };
    static constexpr size_t kMaxEntries = 24;
    std::vector<Entry> entries;
    const Entry *find(const Req &r) const
    {
        for (const Entry &e : entries)
            if (same_request(e.req, r)) return &e;
        return nullptr;
    }
    void free_all()  // (the caller has synchronised)
    {
        for (Entry &e : entries)
            if (e.buf.p) (void)hipFree(e.buf.p);
        entries.clear();
    }
};

// What the context's last DENSE aggregation left behind, for whoever searches or downloads it later (the winner search of the same
// call, mgm_wta_windowed_dev, mgm_wta_right_dev, mgm_wta_runnerup_dev, mgm_lr_device_ptr, mgm_debug_download_*).  Written by the remember stage of
// run_passes (mgm_plan.hip) and by nobody else.
struct DenseRun {
    long long nvol = 0;    // floats per Lr volume
    long long stride = 0;  // floats between the Lr volumes of consecutive passes (>= nvol)
    int ndir = 0;          // Lr volumes per slot
    int batch = 0;         // slots: the volumes of the launch
    int L = 0, Lk = 0;     // labels of that aggregation, and the label stride its kernels ran with (>= L)
    bool wrote_min = false;  // the launch wrote the chunk minima of its Lr volumes (mgm_ctx::lmin)
    PassKernelChoice kernel = {};  // the instance that ran (family kPassRefuse: k_pass_exact, which has one)
    bool pad_c8 = false;   // a padded launch (Lk > L) read compact padded copies of its volumes ...
    int pad_cb = 1;        // ... of this many bytes per cost ...
    const uint8_t *pad_ptr[kMaxBatch] = {};  // ... here: the context's pad8 buffers, or the volumes' own padded copies (mgm_cv::p8)
    const mgm_cv *cvs[kMaxBatch] = {};       // the volumes (identities) ...
    unsigned long long gens[kMaxBatch] = {};  // ... and their generations at that time
    // "no dense aggregation to search": after a trim, or once a range-proportional aggregation has become the context's last.
    // (`stride` stays: mgm_debug_probe_workspace probes the workspace, which a range-proportional aggregation leaves alone, at
    // the stride of the last dense launch.)
    void clear()
    {
        const long long keep = stride;
        *this = DenseRun{};
        stride = keep;
    }
    void forget(const mgm_cv *cv)  // (mgm_cv_free: the address may be handed out again)
    {
        for (int v = 0; v < kMaxBatch; v++)
            if (cvs[v] == cv) cvs[v] = nullptr;
    }
    // is slot v still the volume it was, with the contents it had?
    bool current(int v) const { return v >= 0 && v < batch && cvs[v] && cvs[v]->gen == gens[v]; }
    int slot_of(const mgm_cv *C) const  // the slot of C, or -1 (a volume given twice: its last slot)
    {
        int slot = -1;
        for (int v = 0; v < batch; v++)
            if (cvs[v] == C && current(v)) slot = v;
        return slot;
    }
    bool padded() const { return Lk > L; }
    // pass `pass` of slot `slot` in the Lr workspace (mgm_ctx::lr), and its chunk minima in mgm_ctx::lmin (one float per 32 of
    // the workspace)
    const float *lr(const Buf &ws, int slot, int pass) const { return (const float *)ws.p + ((size_t)slot * ndir + pass) * stride; }
    const float *lmin(const Buf &mins, int slot, int pass) const { return (const float *)mins.p + ((size_t)slot * ndir + pass) * (size_t)(stride / kChunkLabels); }
};
// ... and its last aggregation on the range-proportional copies of ragged volumes (mgm_pass_rel.hip; Lr volumes in mgm_ctx::lr_rel)
struct RelRun {
    int batch = 0, ndir = 0;
    int slots = 0;  // label slots per pixel of volume 0's copy at that launch (the Lr stride mgm_debug_download_lr reads at)
    PassKernelChoice kernel = {};  // the instance that ran
    long long stride = 0;
    const mgm_cv *cvs[kMaxBatch] = {};
    unsigned long long gens[kMaxBatch] = {};
    void clear() { *this = RelRun{}; }
    void forget(const mgm_cv *cv)
    {
        for (int v = 0; v < kMaxBatch; v++)
            if (cvs[v] == cv) cvs[v] = nullptr;
    }
    int slot_of(const mgm_cv *C) const  // the slot of C with the contents it had, or -1
    {
        for (int v = 0; v < batch; v++)
            if (cvs[v] == C && gens[v] == C->gen) return v;
        return -1;
    }
    const float *lr(const Buf &ws, int slot, int pass) const { return (const float *)ws.p + ((size_t)slot * ndir + pass) * stride; }
};

struct Timing {
    const char *name;
    hipEvent_t a, b;
    bool alias = false;  // a second name for the entry before it: the same two events (destroyed once, with that entry)
};

struct mgm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // workspace
    Buf exact_mins, exact_scratch;  // slab minima / (FH beyond 8192 labels) convolution arrays of the operand-order-faithful pass kernel
    Buf lr, hand2, handm, words, census_u, census_v, dbg, stmp, ones8;  // hand2: the slots of the kernels without tags
    Buf lr_rel;                 // the range-proportional kernels' (mgm_pass_rel.hip) Lr volumes [volume][pass][npix][slots]
    HandRegion hand, hand_rel;  // self-validating slabs of k_pass2 (TAGS) / of the range-proportional kernels (forget_hand_regions)
    // chunk minima of the dense Lr volumes (k_pass2, CHMIN): one float per 32 of c->lr, written by the last dense launch iff
    // last.wrote_min; the pruned winner search reads them (run_wta).  wta_stats: its two counters' word on the device (timing or
    // debug statistics on), wta_stats_n: searches counted into it since the last aggregation call began (0: none was pruned)
    Buf lmin, wta_stats;  // (wta_stats: kWtaStatBytes)
    Buf speckle;          // mgm_speckle_dev: the parent and count planes of its labelling (plan_speckle's scratch_bytes)
    Buf holes;            // mgm_fill_holes_dev: the candidate planes and the bands' carries (plan_holes's scratch_bytes)
    Buf energy;           // mgm_energy_dev: the blocks' partials (plan_energy_launch's partial_bytes), then a map when the caller passes none
    // mgm_costvolume_build_subpix_dev: the phase image, refilled in place for every k > 0, and the s phase volumes the
    // fine volume is gathered from; kept for the next call of the same geometry, released by mgm_ctx_trim (subpix_release)
    mgm_img *subpix_img = nullptr;
    mgm_cv *subpix_cv[4] = {};
    int wta_stats_n = 0;
    DenseRun last;    // the last aggregation, if it was a dense one ...
    RelRun rel_last;  // ... or a range-proportional one (each remember stage clears the other)
    // Pipelined contexts (mgm_ctx_set_pipeline, depth >= 2): aggregation calls are DEFERRED and gathered -- up to `depth`
    // calls of the same geometry and settings become ONE launch of the pass kernel (see PendingAgg, pipe_flush)
    struct PendingAgg {
        std::vector<const mgm_cv *> C;
        std::vector<const mgm_img *> w8;  // empty: unweighted
        std::vector<mgm_img *> out, outcost;
        float P1, P2;
        int NDIR, MGM, use_fh, fix_overcount;
        std::string refine;
        bool has_refine;
    };
    int pipe_depth = 1;
    std::vector<PendingAgg> pend;
    // mgm_ctx_set_placement_tries: how many physical placements of a NEW Lr workspace the context may try (0: take what the
    // allocator gives); placed_ptr / placed_cap: the allocation that has been through it
    int place_tries = 0;
    const void *placed_ptr = nullptr;
    size_t placed_cap = 0;
    size_t ws_limit = 0;  // mgm_ctx_set_workspace_limit: cap on the Lr + hand-off workspace of one pass launch (0 = none)
    int debug_stats = 0;  // MGM_HIP_DEBUG_STATS=1: per-workgroup timing summary of K3 on stderr
    unsigned *h_words = nullptr;  // pinned mirrors (HostWord below)
    PlanCache<DenseRequest, DensePlan> dense_plans;  // plans + task tables of the dense kernels' launches, by request
    PlanCache<RelRequest, RelPlan> rel_plans;        // ... of the range-proportional kernels'
    int force_build = 0;  // 0 auto, 1 first build only (MGM_HIP_PASS_BUILD=1)
    Buf padf[kMaxBatch], pad8[kMaxBatch];  // padded copies of the cost volumes of a launch whose label count was padded
    Buf wsel[kMaxBatch], wvals;            // two-valued weights (k_pass2, W2): selector words per volume; the value scan's words
    bool pending_check = false;
    int num_cu = 256;  // hipDeviceProp_t::multiProcessorCount
    int xcc_mask = -1;  // XCC ids the workgroups of a launch see (k_xcc_census; -1: not looked yet)
    // timing
    bool timing = false;
    std::vector<Timing> tim;
};

constexpr int kWtaStatSlots = 64;  // the pruned search's counters: one word per 128 bytes, a workgroup adds to slot blockIdx.x % 64
constexpr size_t kWtaStatBytes = (size_t)kWtaStatSlots * 128;
// The context's control words (mgm_ctx::words; zeroed when they come into being, ensure_words): who lives where.  Tenants that
// may be live at the same time have words of their own (the assertions below); only the queue tickets alias the progress words.
constexpr int kProgWords = kMaxBatch * kMaxDirs * kMaxBands, kQueueTickets = 9;  // prog[volume*8 + pass][band]; the per-XCD queues' tickets of k_pass2
enum CtrlWord : int {
    kWordTicket = 0,    // the pass kernels' ticket counter, reset before every launch
    kWordWatchdog = 1,  // STICKY: set by a hand-off that timed out, cleared by the host alone (check_watchdog)
    kWordFlag = 3,      // one call's flag or count: set, read back (read_word) and done with before the call returns
    kWordProg = 4,      // progress words of the kernels without tags; ALIAS: the queue tickets (kernels with tags, which have no progress words)
    kWordPyr = kWordProg + kProgWords,  // mgm_pyramid.hip: minimum / maximum of a coarse map (2 words), integer hull (2)
    kWordRanges = kWordPyr + 4,         // mgm_update_ranges_dev: global minimum / maximum (2 words)
    kWordCount64 = kWordRanges + 2,     // mgm_selftest_div3: one 64-bit counter (2 words)
    kCtrlWordsTotal = kWordCount64 + 2  // what ensure_words reserves
};
static_assert(kWordTicket < kWordWatchdog && kWordWatchdog < kWordFlag && kWordFlag < kWordProg && kQueueTickets <= kProgWords, "control words: one tenant each");
static_assert(kWordProg % 4 == 0 && kWordCount64 % 2 == 0, "progress words 16-byte aligned, the 64-bit counter 8-byte aligned");
inline unsigned *ctrl_word(const mgm_ctx *c, CtrlWord w) { return (unsigned *)c->words.p + w; }
enum HostWord : int { kHostWatchdog = 1, kHostFlag = 3, kHostWords = 16 };  // mgm_ctx::h_words: the mirrors of watch_launch and read_word

// Development switches (A/B timing, tests of the fall-back paths), read once per process; everything is on by default.
struct DevSwitches {
    bool c8;         // MGM_HIP_C8=0: never use the compact (1 byte per label) cost volumes
    bool lazy_f32;   // MGM_HIP_LAZY_F32=0: always materialise the fp32 volume next to the compact one
    bool pad;        // MGM_HIP_PAD=0: no padding of label counts to the next count of the second build
    int subv;        // MGM_HIP_SUBV=0: one volume per wave also at 128 / 64 labels; 2: volumes share waves whenever they can
    int deep;        // MGM_HIP_DEEP=0|1: never / always the pass kernels with deep DMA rings (default: by the launch's shape)
    int wg_per_cu;   // MGM_HIP_WG_PER_CU=1|2: override the occupancy heuristic of the pass kernel (0 = heuristic)
    int xflags;      // MGM_HIP_XFLAGS: experiment bits of development builds (mgm_device.h)
    int strips;      // MGM_HIP_STRIPS=0|1: never / always walk the lines of passes 4-7 as two strips (default: chain-bound launches only)
    int xcdq;        // MGM_HIP_XCDQ=0|1: never / whenever possible the per-XCD work queues of k_pass2 (default: chain-bound launches)
    int xcdq_k;      // MGM_HIP_XCDQ_K: consecutive bands of a pass per queue block (0: a pass stays on one XCD; default: by the launch's shape)
    bool w2;         // MGM_HIP_W2=0: two-valued weights take the general weighted kernels too (A/B)
    bool oneb;       // MGM_HIP_ONEB=0: launches that run one band per CU keep the queue kernels capped at 64 VGPRs (A/B)
    long long lr_pad;  // MGM_HIP_LR_PAD: floats between consecutive Lr volumes beyond their size, in 256-byte blocks (67)
};
const DevSwitches &dev();
long long lr_pad_floats();
// ... and the winner search's (MGM_HIP_TUNE=wta_*; A/B timing), copied into every request of its planner (plan_wta, plan_wta_right)
struct WtaSwitches {
    int prune_ppw;  // wta_prune_ppw=1|2: groups of eight pixels per wave and turn of the pruned search (k_wta_pruned's PPW; default 1)
    int prune_wg;   // wta_prune_wg=<workgroups per CU> of the pruned search (0: 64)
    int wg_per_cu;  // wta_wg_per_cu=<workgroups per CU> of the plain search (0: by the instance)
    int packed;     // wta_packed=0: one pixel per slab also at 128 / 64 labels
    int wide4;      // wta_wide4=0: the 8-direction instance also for NDIR <= 4
    int quad;       // wta_quad=0: 192 / 384 labels on k_wta<3> / <6>
    int right_seg;  // wta_right_seg=<right pixels per workgroup> of the right view's search (0: by the device)
};
const WtaSwitches &wta_switches();

// Development switches live behind ONE variable: MGM_HIP_TUNE="key=value,key=value" (keys are the lower-case names of
// DevSwitches' comments: deep, xcdq, xcdq_k, strips, wg_per_cu, subv, c8, pad, lazy_f32, w2, oneb, lr_pad, xflags, pass_build,
// debug_stats, check_tags, show_plan, wta_*); the individual MGM_HIP_<KEY> variables of rounds 1-3 are still read (tests and
// tools use them).  A build with -DMGM_HIP_RELEASE compiles the parser out: every switch then has its default.
// (declared in mgm_device.h: mgm::tune_num(key, default))

int fail(mgm_ctx *c, int code, const std::string &msg);
int hipfail(mgm_ctx *c, hipError_t e, const char *what);
#define HIPCHK(c, call)                                          \
    do {                                                         \
        hipError_t e__ = (call);                                 \
        if (e__ != hipSuccess) return hipfail((c), e__, #call);  \
    } while (0)
hipError_t dev_malloc(void **p, size_t bytes);
int reserve(mgm_ctx *c, Buf &b, size_t bytes);
int ensure_words(mgm_ctx *c);
int read_word(mgm_ctx *c, const unsigned *dev, unsigned *out);  // one device word, through the pinned flag mirror; synchronises
int watch_launch(mgm_ctx *c);  // after a pass launch: the watchdog word's copy follows it (check_watchdog looks at it later)
inline void forget_hand_regions(mgm_ctx *c) { hand_forget(c->hand.tags), hand_forget(c->hand_rel.tags); }  // their slots may carry anything: the next launch clears them

struct TimeScope {  // brackets one kernel launch with events when timing is on
    mgm_ctx *c;
    Timing t{};
    bool on;
    const char *kernel = nullptr;  // which kernel was chosen for it (plan_cost_kernel): listed after `name` with the same time
    TimeScope(mgm_ctx *ctx, const char *name) : c(ctx), on(ctx->timing)
    {
        if (!on) return;
        t.name = name;
        if (hipEventCreate(&t.a) != hipSuccess || hipEventCreate(&t.b) != hipSuccess) {
            on = false;
            return;
        }
        (void)hipEventRecord(t.a, c->stream);
    }
    ~TimeScope()
    {
        if (!on) return;
        (void)hipEventRecord(t.b, c->stream);
        c->tim.push_back(t);
        if (kernel) {
            t.name = kernel;
            t.alias = true;
            c->tim.push_back(t);
        }
    }
};

int distance_index(const char *n);
int prefilter_index(const char *n);
int refinement_index(const char *n);
int check_watchdog(mgm_ctx *c, bool block = true);

// pipelined contexts (mgm_ctx_set_pipeline): see mgm_api.hip
int pipe_flush(mgm_ctx *c);
inline int pipe_join(mgm_ctx *c) { return (c && !c->pend.empty()) ? pipe_flush(c) : MGM_OK; }
bool pipe_uses(const mgm_ctx *c, const void *obj);

// volumes and their copies (mgm_volume.hip)
int cv_alloc_f32(mgm_ctx *c, mgm_cv *cv);
int cv_create(mgm_ctx *c, int nx, int ny, int dmin, int dmax, bool alloc_f32, mgm_cv **out);
int ensure_f32(mgm_ctx *c, const mgm_cv *ccv);
int c8_alloc(mgm_ctx *c, mgm_cv *cv, int cb = 1);
int c8_resolve(mgm_ctx *c, const mgm_cv *ccv, bool *use);

int p8_alloc(mgm_ctx *c, mgm_cv *cv, int LP, int cb);
int rel_resolve(mgm_ctx *c, const mgm_cv *cv, bool *usable);
int rel_alloc(mgm_ctx *c, mgm_cv *cv, int slots, int cb);  // (re)allocates relbuf for the format and sets rel_slots / rel_cb; MGM_OK also when the device has no room (relbuf stays null)
void subpix_release(mgm_ctx *c);  // frees the sub-pixel build's scratch image and volumes (the caller has synchronised)
int subpix_interp_index(const char *name);  // "linear" 0, "cubic" 1, anything else (NULL included) -1

// the launch plan (mgm_plan.hip)
int run_passes(mgm_ctx *c, const mgm_cv *const *Cs, const mgm_img *const *w8s, int nb, float P1, float P2, int MGM, int use_fh, int first,
               int count, bool allow_pad = false, int slot0 = 0, int nslots = 0, int layout_ndir = 0, int search_refine = -1, bool search_S = false);
bool wta_prune_enabled();  // MGM_HIP_WTA_PRUNE=0 (read at every call) or tune wta_prune=0: the plain winner search everywhere
int run_wta(mgm_ctx *c, const mgm_cv *C, long long pix0, long long npix, const float *lr, long long lr_stride, int NDIR, int fix_overcount,
            int ridx, float *out, float *outcost, float *Sout, const float *wlo = nullptr, const float *whi = nullptr, int slot = -1);
int run_wta_right(mgm_ctx *c, const mgm_cv *C, int slot, int NDIR, int fix_overcount, int ridx, int vnx, float *out, float *outcost);
int run_wta_runnerup(mgm_ctx *c, const mgm_cv *C, int slot, int NDIR, int fix_overcount, int radius, float *out2, float *cost2, float *out1,
                     float *cost1);
int run_wta_consensus(mgm_ctx *c, const mgm_cv *C, int slot, bool rel, int NDIR, const float *d, float tol, float *votes, float *winners);
// the range-proportional path of ragged volumes (mgm_plan.hip): is this call one it takes?  then the passes + the winner search
bool rel_enabled();
int weights_have_odd_values(mgm_ctx *c, const mgm_img *const *w8s, int nb, long long npix, bool *odd, bool *any = nullptr);
int run_rel(mgm_ctx *c, const mgm_cv *const *Cs, const mgm_img *const *w8s, int nb, float P1, float P2, int MGM, int use_fh, int NDIR,
            int fix_overcount, int ridx, mgm_img *const *outs, mgm_img *const *outcosts, mgm_cv **S = nullptr);
int run_wta_rel(mgm_ctx *c, const mgm_cv *C, int slot, int NDIR, int fix_overcount, int ridx, const float *wlo, const float *whi, float *out,
                float *outcost, float *Sout = nullptr);
int run_wta_refine(mgm_ctx *c, const mgm_cv *C, long long pix0, long long npix, const float *lr, long long lr_stride, int NDIR,
                   int fix_overcount, int ridx, float *out, float *outcost, float *Sout, const float *wlo = nullptr,
                   const float *whi = nullptr, int slot = -1);
