// mgm_geom.h -- the limits, the reference's pass table and the canonical geometry of a pass: plain C++ shared by the kernels
// (mgm_device.h) and the HIP-free launch planner (mgm_planner.h).  Standard headers only.
#pragma once

namespace mgm {

constexpr int kMaxDirs = 8;
constexpr int kMaxBands = 4096;
constexpr int kR = 16;  // lines per band (waves per workgroup) of the pass kernel
constexpr int kCensusMaxWords = 8;  // 32-bit census words per pixel

// Geometry of one pass in canonical coordinates (i = position along the scan
// line, j = line index).  Derived on the host from the reference's pass table
// (mgm_core.cc:463-471): pixel(i,j) = base + i*istep + j*jstep.  In these
// coordinates every pass has the same four neighbours
//   inline (i-1,j)   same (i,j-1)   back (i-1,j-1)   fwd (i+1,j-1)
// and only the ORDER in which they are summed differs:
//   form 0 (passes 0-3): inline, same, back, fwd
//   form 1 (passes 4-7): fwd, back, same, inline
struct PassGeom {
    int NL, LL;        // number of lines, pixels per line
    int form;          // 0 / 1
    int nbands;        // ceil(NL / R)
    int slope;         // pixels of lead a line keeps over the next one: 2, or 1 when no fwd neighbour is used
    long long base;    // pixel index of (0,0)
    long long istep;   // pixel-index step along the line
    long long jstep;   // pixel-index step between lines
    int wplane[4];     // weight plane of neighbour k (mgm_core.cc:481-484)
    int nstrips, split;   // 2: the lines of this pass are walked as two strips [0, split) and [split, LL) by two workgroups per band
                          // (k_pass2, TAGS, form 1 with 2 or 3 neighbours: no in-line dependency), both from the image edge inwards
    long long hand_base;  // self-validating hand-off slabs (k_pass2, TAGS): first slab of this pass within a volume's region
    int swap;             // k_pass_rel only (round 6): a form-0 pass with 2 or 3 neighbours walked with the roles of i and j exchanged (NL, LL, istep,
                          // jstep are the exchanged ones): the in-line neighbour and the one on the line before swap places, the third stays
    int diag, wmax;       // k_pass_rel only (round 6): 1 = the pass is walked along the ANTI-DIAGONALS of (i, j), all lines of a band at the
                          // same step (form 1 with 2 or 3 neighbours: every neighbour sits on the line before); wmax: hand-off slots per line
};

// The workgroup of the range-proportional kernel (k_pass_rel), for the kernel and the planner alike: 4 compute waves of four lines
// each + a loader wave; a 4-deep LDS ring per line; 8 slots in each of the rings the loader fills (costs, records, weights, the
// previous band's slabs); 160 KB of LDS per CU.
constexpr int kRelWaves = 4, kRelLines = 16, kRelRing = 4, kRelStage = 8, kLdsBytes = 160 * 1024;
// floats per hand-off slot: a lane's worth of guard words + the values + another guard (one slab: FH, or the producer publishes E),
// else two slabs; update_cost2_trunclinear (fh2): + the forward and backward passes; + the header's 4
constexpr int rel_hand_floats(bool one_slab, int slots, bool fh2) { return (fh2 ? 3 * slots + 2 * (slots / 16) : (one_slab ? slots + 2 * (slots / 16) : 2 * slots)) + 4; }
// LDS bytes of a workgroup: the lines' rings, the hand ring (a second one with anti-diagonal passes), records and weights, the cost
// pieces, the loader's words, the ticket, the lines' state
constexpr long long rel_wg_lds_bytes(bool one_slab, int slots, int cb, bool fh2, bool diag)
{
    const long long HS = rel_hand_floats(one_slab, slots, fh2);
    return 4 * (kRelLines * kRelRing * HS + (diag ? 2 : 1) * kRelStage * HS + 2 * kRelStage * kRelLines * 4) + (long long)kRelStage * kRelLines * slots * cb +
           4 * (kRelStage + 4) + 16 + 4 * kRelLines * 24;
}

// The build macros of the second build of K3 that its kernels (mgm_pass2.hip, one unit per LPL) and its dispatch unit
// (mgm_pass2_dispatch.hip) both read -- MGM_P2_DEFINES of a tuning or development build reaches both, and the defaults stand here alone.
#ifndef MGM_P2_NC
#define MGM_P2_NC 14       // lines per band (compute waves) with fp32 costs, up to 256 labels
#endif
#ifndef MGM_P2_C8_NL
#define MGM_P2_C8_NL 1     // loader waves with compact costs
#endif
#ifndef MGM_P2_C8_NC
#define MGM_P2_C8_NC (16 - MGM_P2_C8_NL)   // lines per band with compact costs (tuning experiments: 7)
#endif
#ifndef MGM_P2_DEV
#define MGM_P2_DEV 0   // 1: in-kernel timers and experiment switches (development builds: MGM_P2_DEFINES=-DMGM_P2_DEV=1);
#endif                 // the run-time tests alone cost the issue-bound FH kernel 6 %, so product builds compile them out
#ifndef MGM_P2_TIMELINE
#define MGM_P2_TIMELINE 0  // 1: the queue kernels record, per work item, start / end / time waited for the predecessor band / where it
#endif                     // ran (PassParams::tl; MGM_HIP_TIMELINE=<file>; tools/timeline.py).  Variant builds only: tools/sweep_build.sh tl -DMGM_P2_TIMELINE=1
// Lines per band of the second build at LPL * 64 labels, 0 = no such unit.  `compact`: compact costs in a form this label count has
// (c8_supported, mgm_fillplan.h); they need fewer loader waves.  The planner sizes bands by this (pass2_lines) and the kernels their
// workgroups (Plan::NC, mgm_pass2.hip, which asserts the two equal).
constexpr int pass2_band_lines(int lpl, bool compact)
{
    if (lpl == 1 || lpl == 2 || lpl == 3 || lpl == 4) return compact ? MGM_P2_C8_NC : MGM_P2_NC;
    if (lpl == 6 || lpl == 8 || lpl == 12 || lpl == 16) return 7;  // (768 / 1024 labels: round 4)
    return 0;
}

// One launch of the pass kernel may aggregate several cost volumes of identical geometry (the
// left->right and right->left volumes of a stereo pair, consecutive pairs): work items are then (volume, pass,
// band), and the long dependency chains of one volume's column passes are hidden behind the other
// volumes' work.
constexpr int kMaxBatch = 16;

// The reference's pass table, mgm_core.cc:463-471, as data.
struct RefPass {
    int d[4][2];
    int inc_x, inc_y, row_major;
};
static const RefPass kPasses[8] = {
    {{{-1, 0}, {0, -1}, {-1, -1}, {1, -1}}, 1, 1, 1}, {{{1, 0}, {0, 1}, {1, 1}, {-1, 1}}, 0, 0, 1},
    {{{0, 1}, {-1, 0}, {-1, 1}, {-1, -1}}, 1, 0, 0},  {{{0, -1}, {1, 0}, {1, -1}, {1, 1}}, 0, 1, 0},
    {{{-1, -1}, {1, -1}, {0, -1}, {1, 0}}, 0, 1, 1},  {{{1, -1}, {1, 1}, {1, 0}, {0, 1}}, 0, 0, 0},
    {{{1, 1}, {-1, 1}, {0, 1}, {-1, 0}}, 1, 0, 1},    {{{-1, 1}, {-1, -1}, {-1, 0}, {0, -1}}, 1, 1, 0},
};
static const int kPassToChannel[4][8] = {  // mgm_core.cc:481-484
    {0, 1, 2, 3, 4, 5, 6, 7}, {3, 2, 0, 1, 5, 6, 7, 4}, {4, 6, 7, 5, 3, 1, 2, 0}, {5, 7, 4, 6, 1, 2, 0, 3}};

}  // namespace mgm
