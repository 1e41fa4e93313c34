// mgm_pass2_dispatch.hip -- picks the per-LPL object of the second K3 build
// (mgm_pass2.hip is compiled once per LPL with -DMGM_P2_LPL=n).
#include "mgm_device.h"
#include "mgm_planner.h"

namespace mgm {

// whether the second build carries its in-kernel timers / experiment switches (MGM_HIP_DEBUG_STATS, MGM_HIP_XFLAGS)
bool pass2_devtools() { return MGM_P2_DEV != 0; }
bool pass2_timeline() { return MGM_P2_TIMELINE != 0; }

// lines per band of the second build (0 = this L is not supported by it): the rule is pass2_band_lines's (mgm_geom.h)
int pass2_lines(int L, bool c8) { return L % 64 ? 0 : pass2_band_lines(L / 64, c8 && c8_supported(L)); }

hipError_t launch_pass2(const PassParams &p, const PassKernelChoice &c, int ntasks, hipStream_t s)
{
    switch (c.LPL) {
#define X(n) case n: return launch_pass2_lpl<n>(p, c, ntasks, s);
        X(1) X(2) X(3) X(4) X(6) X(8) X(12) X(16)
#undef X
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mgm
