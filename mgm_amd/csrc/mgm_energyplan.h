// mgm_energyplan.h -- which copy of a cost volume mgm_energy_dev reads, and how its one launch is cut into blocks, as pure
// functions.  Plain C++17, standard headers only: no device, no context -- mgm_api.hip fills the request from the
// volume's fields, mgm_energy.hip launches what comes out; tests/energy_plan_harness.cc runs it on the host.
//
// The kernel reads ONE cost per pixel, so it reads whatever copy is current and never asks for another one to be made: no
// expansion, no compaction, no read-back of a flag word.  The order is ensure_f32's (mgm_volume.hip): the fp32 array when it is
// current; else the range-proportional copy of a volume that has nothing else; else the padded compact copy; else the compact one.
#pragma once
#include <type_traits>

#include "mgm_fillplan.h"  // CopyState

namespace mgm {

struct EnergyCopyRequest {
    int f32_state;  // mgm_cv::f32_state (1: the fp32 array is current) ...
    int has_f32;    // ... and whether it is allocated
    int rel_only, rel_state, has_rel, rel_slots, rel_cb;  // the range-proportional copy (CopyState as an int)
    int p8_state, has_p8, p8_L, p8_cb;                    // the padded compact copy
    int c8_state, has_c8, cbytes;                         // the compact copy
    int L;                                                // labels of the volume (of the hull, for a ragged one)
    int unfilled;                                         // a refill failed half-way: the volume holds nothing
};
static_assert(std::has_unique_object_representations_v<EnergyCopyRequest>, "EnergyCopyRequest: integers only, no padding");

enum EnergyCopy { kEnergyCopyNone = 0, kEnergyCopyF32, kEnergyCopyRel, kEnergyCopyPadded, kEnergyCopyCompact };
struct EnergyCopyChoice {
    int copy;    // EnergyCopy; None: no copy holds the volume (MGM_ERR_INVALID)
    int cb;      // bytes per cost: 4 the float itself, 1 / 2 a code (255 / 65535 = +INF)
    int stride;  // cost slots per pixel: L, the padded label count, or the slots of the range-proportional copy
};
static_assert(std::has_unique_object_representations_v<EnergyCopyChoice>, "EnergyCopyChoice: integers only, no padding");

inline EnergyCopyChoice plan_energy_copy(const EnergyCopyRequest &q)
{
    const auto usable = [](int s) { return s == (int)CopyState::Written || s == (int)CopyState::Valid; };
    const auto code_bytes = [](int cb) { return cb == 1 || cb == 2; };
    EnergyCopyChoice c{};
    if (q.L < 1 || q.unfilled) return c;
    if (q.f32_state && q.has_f32) return EnergyCopyChoice{kEnergyCopyF32, 4, q.L};
    if (q.f32_state) return c;  // (claims an array it does not have)
    if (q.rel_only && q.rel_state == (int)CopyState::Valid && q.has_rel && (q.rel_slots == 64 || q.rel_slots == 128) &&
        (code_bytes(q.rel_cb) || q.rel_cb == 4))
        return EnergyCopyChoice{kEnergyCopyRel, q.rel_cb, q.rel_slots};
    if (q.p8_state == (int)CopyState::Valid && q.has_p8 && q.p8_L >= q.L && code_bytes(q.p8_cb)) return EnergyCopyChoice{kEnergyCopyPadded, q.p8_cb, q.p8_L};
    if (usable(q.c8_state) && q.has_c8 && code_bytes(q.cbytes)) return EnergyCopyChoice{kEnergyCopyCompact, q.cbytes, q.L};
    return c;
}

// The launch: one lane per pixel in raster order, kEnergyThreads consecutive pixels per workgroup, one partial per workgroup.  The
// partition depends on nx * ny alone, so the partials -- and their sum in index order -- are the same bits from call to call.
constexpr int kEnergyThreads = 256;
constexpr int kEnergyPartialWords = 4;  // per block: data, smooth, total (fp64) and the count of finite pixels (as a 64-bit integer)
constexpr long long kEnergyMaxPixels = 2147483647ll;
struct EnergyLaunch {
    long long blocks;         // 0: refused (no pixels, or more than 2^31 - 1 of them)
    long long partial_bytes;  // blocks * 4 * 8
};
inline EnergyLaunch plan_energy_launch(int nx, int ny)
{
    EnergyLaunch l{};
    const long long npix = (long long)nx * ny;
    if (nx < 1 || ny < 1 || npix > kEnergyMaxPixels) return l;
    l.blocks = (npix + kEnergyThreads - 1) / kEnergyThreads;
    l.partial_bytes = l.blocks * kEnergyPartialWords * 8;
    return l;
}

}  // namespace mgm
