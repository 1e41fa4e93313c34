// holes_plan_harness.cc -- plan_holes (mgm_amd/csrc/mgm_planner.h) behind a C interface for tests/test_holes_plan.py and
// tests/test_gpu_holes.py (which reads the chunk and the band from it).  Built with plain g++ and no ROCm include path, like
// speckle_plan_harness.cc.
#include "mgm_planner.h"

using namespace mgm;

extern "C" {

int holes_request_bytes() { return (int)sizeof(HolesRequest); }
int holes_choice_bytes() { return (int)sizeof(HolesChoice); }
int holes_threads() { return kHolesThreads; }

// `n` requests as their bytes, one after the other (integers only, no padding: static_assert in the header); per request
// out[12] = family, chunk, band, nbands, walk_dirs, planes, grid_rows, grid_walk, grid_apply, nlines, carry_words, scratch_bytes
void holes_plan(const unsigned char *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        HolesRequest q;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        const HolesChoice c = plan_holes(q);
        const long long v[12] = {c.family, c.chunk, c.band, c.nbands, c.walk_dirs, c.planes, c.grid_rows, c.grid_walk, c.grid_apply, c.nlines,
                                 c.carry_words, c.scratch_bytes};
        memcpy(out + (size_t)i * 12, v, sizeof v);
    }
}

}  // extern "C"
