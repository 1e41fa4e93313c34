// speckle_plan_harness.cc -- plan_speckle (mgm_amd/csrc/mgm_planner.h) behind a C interface for tests/test_speckle_plan.py and
// tests/test_gpu_speckle.py (which reads the tile from it).  Built with plain g++ and no ROCm include path, like runnerup_plan_harness.cc.
#include "mgm_planner.h"

using namespace mgm;

extern "C" {

int speckle_request_bytes() { return (int)sizeof(SpeckleRequest); }
int speckle_choice_bytes() { return (int)sizeof(SpeckleChoice); }
int speckle_threads() { return kSpeckleThreads; }

// `n` requests as their bytes, one after the other (integers only, no padding: static_assert in the header); per request
// out[11] = family, tw, th, ntx, nty, planes, grid_local, grid_seams, grid_count, grid_apply, scratch_bytes
void speckle_plan(const unsigned char *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        SpeckleRequest q;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        const SpeckleChoice c = plan_speckle(q);
        const long long v[11] = {c.family, c.tw, c.th, c.ntx, c.nty, c.planes, c.grid_local, c.grid_seams, c.grid_count, c.grid_apply, c.scratch_bytes};
        memcpy(out + (size_t)i * 11, v, sizeof v);
    }
}

}  // extern "C"
