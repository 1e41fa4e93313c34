// mgm_fillplan.h -- how a cost volume gets filled, as pure functions: everything the filling is decided by goes in as a request
// (FillRequest), everything decided before the first launch comes out as a plan (plan_fill: the refusal, the scratch of the
// inputs, the first attempt), and "this attempt came back with this flag word" gives the next attempt (fill_step, rel_next_format).
// Plain C++17, standard headers only: no device, no context, no environment -- mgm_volume.hip fills the request, launches the
// attempts and commits the last one to the volume; tests/test_fillplan.py runs the policy on the host.  Which K2 kernel writes an
// attempt is decided here as well (plan_cost_kernel, at the end): launch_cost is a table from its choice to an instance.
#pragma once
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "../../include/mgm_hip.h"  // the error codes of a refusal
#include "mgm_geom.h"

namespace mgm {

// The label counts that have compact forms, in blocks of 64 labels: one list for padded_labels and the instances of the census kernels.
#define MGM_LABEL_BLOCKS(X) X(1) X(2) X(3) X(4) X(6) X(8) X(12) X(16)
// The label count the pass kernels run `L` labels at (151 -> 192 slots, ...); 0: beyond their largest.
inline int padded_labels(int L)
{
#define X(n) 64 * n,
    for (int lp : {MGM_LABEL_BLOCKS(X)})
#undef X
        if (lp >= L) return lp;
    return 0;
}
// compact-cost support: label counts for which the C8 forms of K3 / k_wta exist
inline bool c8_supported(int L) { return L > 0 && padded_labels(L) == L; }

// A truncation under which every bit count has a one-byte code: +INF, or a whole number 0..254 with a clear sign bit.
inline bool is_byte_code(float t) { return t == __builtin_huge_valf() || (t >= 0.0f && !std::signbit(t) && t <= 254.0f && t == rintf(t)); }

// Bytes per cost of a compact form over `labels` label slots: census costs are bit counts (one byte); absolute differences of
// a one-channel 8-bit pair stay below 256, of a colour pair below 766, squared differences below 65026 per channel: two bytes
// (up to 512 labels: the pass kernels that read them).  The flag word tells afterwards whether every cost really had the form.
inline int compact_cost_bytes(int costfn, int nch, bool diff_wide, int labels)
{
    return (costfn == 2 || (costfn == 0 && nch == 1 && !diff_wide) || labels > 512) ? 1 : 2;
}

// What the restructured K2 kernels ask of a volume, beyond their cost function and target -- the predicates plan_cost_kernel
// chooses by and plan_fill reserves scratch and attempts the padded layout by.
// k_cost_diffx: truncDist = +INF or a non-negative number with a clear sign bit (min(e, truncDist) is v_min_f32 there), and
// pixel groups that index in 32 bits
inline bool diffx_takes(float trunc, long long npix) { return trunc >= 0.0f && !std::signbit(trunc) && npix < 0x7fffffffll; }
// k_cost_ncc reads the window statistics of k_ncc_stats: dense volumes of up to four channels (its window and label limits:
// kNccMaxHw, kNccMaxL); k_cost_btx the sample spans of k_bt_spans: dense volumes
inline bool ncc_stats_serve(bool ragged, int nch) { return !ragged && nch <= 4; }
inline bool bt_spans_serve(bool ragged) { return !ragged; }

// What a volume remembers of its earlier fillings.
struct FillMemory {
    int diff_fails = 0;        // AD / SD fillings in a row that did not fit a compact form: after two, refills go straight to the fp32 kernel
    bool diff_wide = false;    // ... did not fit ONE byte per cost but does fit two: refills start there
    int rel_hint_slots = 64;   // the width the last direct filling needed: a refill starts there
};

struct FillRequest {
    int nx, ny, vnx, vny, nch;  // the two images
    int L;                      // labels of the volume (of the hull, for a ragged one)
    int dist, pre;              // distance_index / prefilter_index of what the caller asked for
    int census_win;
    float truncDist;
    bool ragged;
    FillMemory mem;
    bool c8, pad, lazy_f32, rel, rel_direct;  // the development switches the filling reads (all on by default)
};

// The forms a filling is written in.
enum class FillForm {
    RelDirect,    // the range-proportional copy alone (k_cost_census_rel): `slots` label slots per pixel, one byte per cost
    Padded,       // the padded compact copy alone (mgm_cv::p8): `slots` label slots, the ones beyond the real count +INF
    CompactOnly,  // the compact copy alone (mgm_cv::d8)
    General,      // the fp32 volume, with a compact twin of `cbytes` bytes per cost (0: without)
};
struct FillAttempt {
    FillForm form;
    int slots;      // label slots of the target: RelDirect 64 / 128 per pixel, Padded the padded label count, CompactOnly the labels; General 0
    int cbytes;     // bytes per cost of the compact target or twin
    bool readback;  // the flag word is read back at once (false: the form fits by construction, or cannot fail)
};

enum class FillInputs { Plain, Census, Sobelx, Gblur, NccStats, BtSpans };  // what is computed from the images before K2

struct FillPlan {
    int err = MGM_OK;  // a refusal, decided before anything is touched ...
    const char *msg = nullptr;  // ... and its message
    int costfn, pre;   // the cost function (picked BEFORE the consistency fix, mgm_costvolume.h:355) and the prefilter after it (358-362)
    int census_words;  // 32-bit words of a census descriptor (0: no census prefilter)
    bool nan_words;    // descriptor words of more than 24 bits read as floats (mgm_cv::nan_words)
    int nch;           // channels of the (prefiltered) images K2 reads: the descriptor words, or the images' channels
    float trunc;       // truncDist * nch (mgm_costvolume.h:401,405)
    FillInputs inputs;
    size_t bytes_u, bytes_v, bytes_tmp;  // scratch of the inputs: per image (the context's census buffers) and the blur's temporary
    FillAttempt first;    // where the filling starts
    FillAttempt general;  // where it ends if nothing narrower works out: the fp32 volume (and what a direct attempt without room falls to)
    int gather_cb;        // ragged volume that ends in General: bytes per cost its gathered copy starts with (64 slots); 0: no gathered copy
};

inline FillPlan plan_fill(const FillRequest &q)
{
    FillPlan p{};
    p.costfn = q.dist;
    p.pre = (q.dist == 2 || q.pre == 1) ? 1 : q.pre;
    p.nch = q.nch;
    p.inputs = FillInputs::Plain;
    const size_t npu = (size_t)q.nx * q.ny, npv = (size_t)q.vnx * q.vny;
    if (p.pre == 1) {
        const int wr = q.census_win / 2, side = 2 * wr + 1, nbits = q.nch * (side * side - 1);
        if (wr < 1 || nbits % 8) {  // census_tools.cc:81 asserts this
            p.err = MGM_ERR_INVALID, p.msg = "census: nch*(win*win-1) must be a positive multiple of 8";
            return p;
        }
        p.census_words = (nbits / 8 + 3) / 4;
        if (p.census_words > kCensusMaxWords) {
            p.err = MGM_ERR_UNSUPPORTED, p.msg = "census descriptor longer than 256 bits";
            return p;
        }
        p.nan_words = p.costfn != 2 && nbits > 24;
        p.nch = p.census_words;  // (-p census with an ad/sd cost: words read as floats)
        p.inputs = FillInputs::Census;
        p.bytes_u = sizeof(unsigned) * npu * p.census_words, p.bytes_v = sizeof(unsigned) * npv * p.census_words;
    } else if (p.pre == 2 || p.pre == 3) {  // sobelx / gblur of both images (mgm_costvolume.h:366-373), then AD or SD on them
        p.inputs = p.pre == 2 ? FillInputs::Sobelx : FillInputs::Gblur;
        p.bytes_u = sizeof(float) * npu * q.nch, p.bytes_v = sizeof(float) * npv * q.nch;
        if (p.pre == 3) p.bytes_tmp = p.bytes_u > p.bytes_v ? p.bytes_u : p.bytes_v;
    } else if (p.costfn == 3 && ncc_stats_serve(q.ragged, q.nch)) {
        // clipped NCC on the plain images: the per-pixel window statistics are computed once (k_ncc_stats), in the census
        // buffers, which this combination leaves free
        p.inputs = FillInputs::NccStats;
        p.bytes_u = sizeof(float) * npu * (2 * q.nch + 1), p.bytes_v = sizeof(float) * npv * (2 * q.nch + 1);
    } else if (p.costfn >= 4 && bt_spans_serve(q.ragged)) {
        // Birchfield-Tomasi on the plain images: the interval every sample spans is computed once (k_bt_spans), likewise
        p.inputs = FillInputs::BtSpans;
        p.bytes_u = sizeof(float) * npu * 2 * q.nch, p.bytes_v = sizeof(float) * npv * 2 * q.nch;
    }
    p.trunc = q.truncDist * (float)p.nch;

    // Which costs can have a compact form.  (NCC costs are (nch - clipped NCC) * 64 and Birchfield-Tomasi costs are built on
    // half-way interpolants: practically never whole numbers, so none is attempted -- one byte store per label of K2, for
    // nothing.)  Neither is one attempted for census over several descriptor words (thirds or halves of bit counts), for
    // differences of blurred images or of descriptor words read as floats, nor for a volume whose last two fillings did not fit.
    const bool diff = p.costfn <= 1 && (p.pre == 0 || p.pre == 2);  // absolute / squared differences of (sobelx-filtered) images
    const bool census1 = p.costfn == 2 && p.census_words == 1;      // bit counts over one descriptor word
    const bool tried = q.mem.diff_fails < 2;
    // min(popcount, trunc) in integers (k_cost_census8*, k_cost_census_rel): every cost has a compact form and none is NaN BY
    // CONSTRUCTION -- nothing to read back, a refilled volume costs no synchronisation
    const bool census_fits = census1 && is_byte_code(p.trunc);
    const bool diff_may_fit = diff && diffx_takes(p.trunc, (long long)q.nx * q.ny);
    const bool compact = q.c8 && c8_supported(q.L);
    const int cb = compact_cost_bytes(p.costfn, q.nch, q.mem.diff_wide, q.L);
    const bool twin = compact && (census1 || (diff && tried));

    p.general = FillAttempt{FillForm::General, 0, twin ? cb : 0, false};
    // A ragged volume that ends with its fp32 hull also gets a gathered RANGE-PROPORTIONAL copy (mgm_pass_rel.hip), in the
    // narrowest form the cost function can have: one byte for single-word census and grey-level absolute differences, two for
    // the other absolute / squared differences; the flag word (read back by the first aggregation, rel_next_format) widens it
    // (... and the fp32 cost itself -- four bytes -- for what has no integer form)
    p.gather_cb = !(q.ragged && q.rel) ? 0 : (census1 || (p.costfn == 0 && q.nch == 1 && p.pre == 0)) ? 1 : diff ? 2 : 4;

    const int LP = (!c8_supported(q.L) && q.c8 && q.pad && q.lazy_f32 && !q.ragged) ? padded_labels(q.L) : 0;
    if (q.ragged && census_fits && q.rel && q.lazy_f32 && q.rel_direct) {
        // A ragged single-word census volume: the range-proportional copy ALONE, straight from the descriptor words -- neither the
        // fp32 hull nor its compact twin is written; whoever wants the hull gets it from ensure_f32.  The flag word (a window
        // wider than the slots take) is read back at once.
        p.first = FillAttempt{FillForm::RelDirect, q.mem.rel_hint_slots == 128 ? 128 : 64, 1, true};
    } else if (LP && tried && (census_fits || diff_may_fit)) {
        // A label count that the pass kernels run padded: the same two families of costs write the PADDED compact copy
        // themselves instead of an fp32 volume that every aggregation call would pad and encode again.
        p.first = FillAttempt{FillForm::Padded, LP, compact_cost_bytes(p.costfn, q.nch, q.mem.diff_wide, LP), !census_fits};
    } else if (twin && !q.ragged && q.lazy_f32 && (census_fits || diff)) {
        // The compact copy alone: the fp32 volume -- which neither K3 nor k_wta reads then -- is only materialised on demand
        // (ensure_f32).  Differences of 8-bit images are whole numbers: the flag word is read back at once -- the read-back the
        // aggregation would do anyway (c8_resolve).
        p.first = FillAttempt{FillForm::CompactOnly, q.L, cb, !census_fits};
    } else {
        p.first = p.general;
    }
    return p;
}

// "This attempt came back with this flag word: what next?"  done: the attempt stands (it fitted, or could not fail) and `mem`
// is what the volume remembers from now on; else `next` is the attempt to make.  The ladders: 64 -> 128 slots; one -> two bytes
// per cost where the kernel says two would do (flag == 1) and the label count has kernels that read them; else the fp32 fill.
struct FillStep {
    bool done;
    FillAttempt next;
    FillMemory mem;
};
inline FillStep fill_step(const FillPlan &p, const FillAttempt &a, unsigned flag, FillMemory mem)
{
    FillStep s{true, a, mem};
    if (a.form == FillForm::General) return s;
    const bool fits = !a.readback || flag == 0u;
    if (a.form == FillForm::RelDirect) {
        if (fits) s.mem.rel_hint_slots = a.slots;
        else if (a.slots < 128) s.next.slots = 128;  // (round 6: windows of up to 62 labels in 64 slots per pixel, else up to 126 in 128)
        else s.next = p.general;  // a window wider than 126 labels: the general path
        s.done = fits;
        return s;
    }
    if (fits) {
        if (a.readback || a.form == FillForm::Padded) s.mem.diff_fails = 0;
        return s;
    }
    s.done = false;
    if (a.cbytes == 1 && flag == 1u && a.slots <= 512) {  // one byte per cost was too narrow (a grey pair with a difference of 255)
        s.mem.diff_wide = true;
        s.next.cbytes = 2;
        return s;
    }
    // does not fit (float-valued images, a fractional truncDist): filled again by the general kernel, fp32 volume and all,
    // and so are its refills after the second time
    s.mem.diff_fails++;
    s.next = FillAttempt{FillForm::General, 0, 0, false};
    return s;
}

// What a volume knows of one of its copies (the compact one, the range-proportional one) or of its NaN scan.
enum class CopyState : int {
    Invalid = -1,  // checked: not usable (a cost without a code, a window too wide; the NaN scan: the volume holds NaN)
    None = 0,      // no such copy (the NaN scan: not scanned)
    Written = 1,   // written, its flag word on the device not read back yet
    Valid = 2,     // checked: usable (the NaN scan: clean)
};
// What the volume knows of its copies after a filling, from the attempt that stands (mgm_cv's fields of the same names).
struct FillState {
    CopyState c8_state, nan_state, rel_state;
    bool keep_rel_state;  // a dense filling that ended on a flag word read back at once leaves rel_state alone (as it always did)
    CopyState p8_state;  // (None or Valid)
    int f32_state;
    bool rel_only;
};
inline FillState fill_state(const FillRequest &q, const FillAttempt &a)
{
    const bool general = a.form == FillForm::General, direct = a.form == FillForm::RelDirect;
    FillState s{};
    s.f32_state = general;  // (else the compact / range-proportional copy holds the volume: ensure_f32)
    // the general kernels flag NaN costs as they write them; the integer forms are NaN-free by construction or by their flag word
    s.nan_state = general ? CopyState::Written : CopyState::Valid;
    s.p8_state = a.form == FillForm::Padded ? CopyState::Valid : CopyState::None;
    // (a direct or padded filling leaves no compact hull: c8_resolve makes one from the expanded volume if a dense launch wants it;
    // an fp32 volume without a twin where the pass kernels would read one has none BY VERDICT)
    if (a.form == FillForm::CompactOnly) s.c8_state = CopyState::Valid;
    else if (general && a.cbytes) s.c8_state = CopyState::Written;
    else s.c8_state = (general && q.c8 && c8_supported(q.L)) ? CopyState::Invalid : CopyState::None;
    s.rel_only = direct;
    s.rel_state = direct ? CopyState::Valid : CopyState::None;  // (General: until the copy is gathered)
    s.keep_rel_state = a.form == FillForm::Padded || (a.form == FillForm::CompactOnly && a.readback);
    return s;
}

// The continuation of the ladder for a GATHERED range-proportional copy, whose flag word the first aggregation reads back
// (rel_resolve): bit 0 = a window wider than the format's slots - 2, bit 1 = a cost without the format's code.  The copy is
// gathered again one step wider -- 64 -> 128 slots, one -> two -> four bytes per cost (four: the fp32 cost itself) -- while the
// fp32 hull it is gathered from is current; what fits neither keeps the dense hull.  false: give the copy up.
inline bool rel_next_format(unsigned flag, bool hull_current, int *slots, int *cb)
{
    const int s = (flag & 1u) ? *slots * 2 : *slots, b = (flag & 2u) ? *cb * 2 : *cb;
    if (s > 128 || b > 4 || !hull_current) return false;
    *slots = s, *cb = b;
    return true;
}

// ---- which K2 kernel writes an attempt ----------------------------------------------------------------------------------------
// Everything the choice depends on (mgm_volume.hip: cost_request builds it from the attempt, run_attempts sets the pointers it
// stands for): the restructured kernels of mgm_cost_fast.hip each take one family of volumes, the general k_cost (mgm_cost.hip)
// whatever is left -- ragged volumes, prefiltered NCC / Birchfield-Tomasi, label counts that are not multiples of four --, and
// nothing but the former writes a padded layout.  A RelDirect attempt is not K2's (k_cost_census_rel).
constexpr int kNccPxb = 32;     // k_cost_ncc: pixels of a row per workgroup
constexpr int kNccMaxHw = 3;    // windows up to 7x7 (CENSUS_NCC_WIN <= 7); wider ones take the general kernel
constexpr int kNccMaxL = 1024;  // LDS: (PXB + L + 2*hw) floats per row and channel

struct CostKernelRequest {
    int costfn, nch, nx, ny, vnx, vny;  // the cost function (0 ad, 1 sd, 2 census, 3 ncc, 4 btad, 5 btsd) and what it reads
    int L, Lreal;                       // label slots of the layout being written; the labels among them
    int cbytes, hwin;
    float trunc;
    bool f32, compact;  // an fp32 target exists; a compact target exists
    bool ragged;
    bool scratch;       // the per-image scratch of the window statistics / sample spans exists (FillInputs::NccStats, BtSpans)
};
enum class CostFamily { Refused, Ncc, BtxBt, BtxDiff, BtxCensus, Diffx, Census8x, Census8, General };
enum class CostPre { None, NccStats, BtSpans };  // the kernel that runs on either image first
struct CostInstance {
    CostFamily family;
    int FN, W4;       // k_cost_btx<FN, W4>; W4 of k_cost_census8x
    int CB, SD, NCH;  // k_cost_diffx<CB, NCH, SD>: NCH 1, 3 or 0 = any
    int LN;           // k_cost_census8x<L, W4>: the label count; k_cost_census8<LPL>: labels per lane
    int HW;           // k_cost_ncc<HW>
};
struct CostKernelChoice : CostInstance {
    CostPre pre;
    unsigned pre_grid_u, pre_grid_v;
    unsigned grid;
    size_t lds;        // dynamic LDS bytes (k_cost_ncc)
    unsigned tb;       // the census kernels' truncation as a byte
    const char *name;  // what the timing table lists next to "k_cost"
};

// The instances launch_cost has, family by family -- the planner returns one of these or Refused.
constexpr CostInstance kCostInstances[] = {
    {CostFamily::Ncc, 0, 0, 0, 0, 0, 0, 1}, {CostFamily::Ncc, 0, 0, 0, 0, 0, 0, 2}, {CostFamily::Ncc, 0, 0, 0, 0, 0, 0, 3},
    {CostFamily::BtxBt, 4, 0}, {CostFamily::BtxBt, 4, 1}, {CostFamily::BtxBt, 5, 0}, {CostFamily::BtxBt, 5, 1},
    {CostFamily::BtxDiff, 0, 0}, {CostFamily::BtxDiff, 0, 1}, {CostFamily::BtxDiff, 1, 0}, {CostFamily::BtxDiff, 1, 1},
    {CostFamily::BtxCensus, 2, 0}, {CostFamily::BtxCensus, 2, 1},
    {CostFamily::Diffx, 0, 0, 1, 0, 1}, {CostFamily::Diffx, 0, 0, 1, 0, 3}, {CostFamily::Diffx, 0, 0, 1, 0, 0},
    {CostFamily::Diffx, 0, 0, 1, 1, 1}, {CostFamily::Diffx, 0, 0, 1, 1, 3}, {CostFamily::Diffx, 0, 0, 1, 1, 0},
    {CostFamily::Diffx, 0, 0, 2, 0, 1}, {CostFamily::Diffx, 0, 0, 2, 0, 3}, {CostFamily::Diffx, 0, 0, 2, 0, 0},
    {CostFamily::Diffx, 0, 0, 2, 1, 1}, {CostFamily::Diffx, 0, 0, 2, 1, 3}, {CostFamily::Diffx, 0, 0, 2, 1, 0},
#define X(n) {CostFamily::Census8x, 0, 0, 0, 0, 0, 64 * n}, {CostFamily::Census8x, 0, 1, 0, 0, 0, 64 * n}, {CostFamily::Census8, 0, 0, 0, 0, 0, n},
    MGM_LABEL_BLOCKS(X)
#undef X
    {CostFamily::General},
};

// The name of an instance in the timing table: the family, and the template arguments the tests tell instances apart by.
inline const char *cost_kernel_name(const CostInstance &k)
{
    switch (k.family) {
    case CostFamily::Ncc: return "k_cost_ncc";
    case CostFamily::BtxBt: return k.W4 ? "k_cost_btx_bt_w4" : "k_cost_btx_bt";
    case CostFamily::BtxDiff: return k.W4 ? "k_cost_btx_diff_w4" : "k_cost_btx_diff";
    case CostFamily::BtxCensus: return k.W4 ? "k_cost_btx_census_w4" : "k_cost_btx_census";
    case CostFamily::Diffx: return k.CB == 2 ? (k.NCH ? "k_cost_diffx_2b" : "k_cost_diffx_2b_anych") : (k.NCH ? "k_cost_diffx_1b" : "k_cost_diffx_1b_anych");
    case CostFamily::Census8x: return k.W4 ? "k_cost_census8x_w4" : "k_cost_census8x";
    case CostFamily::Census8: return "k_cost_census8";
    case CostFamily::General:
    case CostFamily::Refused: break;  // (a refusal is the general kernel's: it is the one that cannot write the layout)
    }
    return "k_cost_general";
}

inline CostKernelChoice plan_cost_kernel(const CostKernelRequest &q)
{
    CostKernelChoice c{};
    const long long npix = (long long)q.nx * q.ny, vpix = (long long)q.vnx * q.vny;
    const long long ngrp = ((long long)q.nx + 3) / 4 * q.ny;  // groups of four pixels of a row (widened first: nx + 3 may not fit an int)
    const bool f32_alone = q.f32 && !q.compact && !q.ragged, compact_alone = !q.f32 && q.compact;
    const auto at_most = [](long long n, long long cap) { return n > cap ? cap : n; };
    const long long nbtx = at_most((ngrp + 3) / 4, 256 * 64);  // k_cost_btx: a wavefront per group, at least one workgroup
    if (q.costfn == 3 && q.scratch && f32_alone && ncc_stats_serve(q.ragged, q.nch) && q.hwin >= 1 && q.hwin <= kNccMaxHw && q.L <= kNccMaxL) {
        c.family = CostFamily::Ncc, c.HW = q.hwin;
        c.pre = CostPre::NccStats, c.pre_grid_u = (unsigned)((npix + 255) / 256), c.pre_grid_v = (unsigned)((vpix + 255) / 256);
        c.lds = sizeof(float) * (size_t)q.nch * (2 * q.hwin + 1) * ((kNccPxb + 2 * q.hwin) + (kNccPxb + q.L - 1 + 2 * q.hwin));
        c.grid = (unsigned)(((long long)q.nx + kNccPxb - 1) / kNccPxb * q.ny);
    } else if ((q.costfn == 4 || q.costfn == 5) && q.scratch && f32_alone && bt_spans_serve(q.ragged) && q.L % 4 == 0) {
        c.family = CostFamily::BtxBt, c.FN = q.costfn, c.W4 = q.nx % 4 == 0;
        c.pre = CostPre::BtSpans, c.pre_grid_u = (unsigned)((npix * q.nch + 255) / 256), c.pre_grid_v = (unsigned)((vpix * q.nch + 255) / 256);
        c.grid = (unsigned)(nbtx < 1 ? 1 : nbtx);
    } else if (q.costfn >= 0 && q.costfn <= 2 && f32_alone && q.L % 4 == 0) {
        // differences / census over several descriptor words without a compact form: the fp32 volume alone
        c.family = q.costfn == 2 ? CostFamily::BtxCensus : CostFamily::BtxDiff, c.FN = q.costfn, c.W4 = q.nx % 4 == 0;
        c.grid = (unsigned)(nbtx < 1 ? 1 : nbtx);
    } else if (compact_alone && (q.costfn == 0 || q.costfn == 1) && !q.ragged && diffx_takes(q.trunc, npix) && c8_supported(q.L) &&
               (q.cbytes == 1 || q.cbytes == 2) && q.L * q.cbytes <= 1024) {
        c.family = CostFamily::Diffx, c.CB = q.cbytes, c.SD = q.costfn == 1, c.NCH = (q.nch == 1 || q.nch == 3) ? q.nch : 0;
        c.grid = (unsigned)at_most((ngrp * 4 * q.L * q.cbytes / 4096 + 3) / 4 + 1, 256 * 32);
    } else if (compact_alone && q.costfn == 2 && q.nch == 1 && c8_supported(q.L)) {
        // four pixels per lane where the groups index in 32 bits, else one wavefront per pixel (every compact label count is a multiple of 64)
        c.tb = q.trunc == __builtin_huge_valf() ? 255u : (unsigned)q.trunc;
        if (npix < 0x7fffffffll) {
            c.family = CostFamily::Census8x, c.LN = q.L, c.W4 = q.nx % 4 == 0;
            c.grid = (unsigned)at_most((ngrp * 4 * q.L / 4096 + 3) / 4 + 1, 256 * 32);
        } else {
            c.family = CostFamily::Census8, c.LN = q.L / 64;
            c.grid = (unsigned)at_most((npix + 3) / 4, 256 * 32);
        }
    } else if (q.Lreal == q.L) {
        c.family = CostFamily::General;
        c.grid = (unsigned)((npix + 3) / 4);
    }  // (else Refused: only the restructured kernels write a padded layout)
    bool exists = false;
    for (const CostInstance &k : kCostInstances)
        exists |= k.family == c.family && k.FN == c.FN && k.W4 == c.W4 && k.CB == c.CB && k.SD == c.SD && k.NCH == c.NCH && k.LN == c.LN && k.HW == c.HW;
    if (!exists) c = CostKernelChoice{};
    c.name = cost_kernel_name(c);
    return c;
}

// The request of one attempt of a planned filling (not of a RelDirect one: that is k_cost_census_rel's).
inline CostKernelRequest cost_request(const FillRequest &q, const FillPlan &p, const FillAttempt &a)
{
    CostKernelRequest r{};
    r.costfn = p.costfn, r.nch = p.nch, r.nx = q.nx, r.ny = q.ny, r.vnx = q.vnx, r.vny = q.vny;
    r.L = a.form == FillForm::Padded ? a.slots : q.L, r.Lreal = q.L;
    r.cbytes = a.cbytes, r.hwin = q.census_win / 2, r.trunc = p.trunc;
    r.f32 = a.form == FillForm::General;
    r.compact = a.form == FillForm::Padded || a.form == FillForm::CompactOnly || (r.f32 && a.cbytes != 0);
    r.ragged = q.ragged;
    r.scratch = p.inputs == FillInputs::NccStats || p.inputs == FillInputs::BtSpans;
    return r;
}

}  // namespace mgm
