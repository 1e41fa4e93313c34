// runnerup_plan_harness.cc -- plan_wta_runnerup (mgm_amd/csrc/mgm_planner.h) behind a C interface for
// tests/test_runnerup_plan.py.  Built with plain g++ and no ROCm include path, like wta_plan_harness.cc.
#include "mgm_planner.h"

using namespace mgm;

extern "C" {

int runnerup_request_bytes() { return (int)sizeof(RunnerupRequest); }
int runnerup_choice_bytes() { return (int)sizeof(RunnerupChoice); }
long long runnerup_wg_per_cu() { return kRunnerupWgPerCu; }

// `n` requests as their bytes, one after the other (integers only, no padding: static_assert in the header); per request
// out[5] = family, LPL, PPW, MAXD, grid
void runnerup_plan(const unsigned char *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        RunnerupRequest q;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        const RunnerupChoice c = plan_wta_runnerup(q);
        const long long v[5] = {c.family, c.LPL, c.PPW, c.MAXD, c.grid};
        memcpy(out + (size_t)i * 5, v, sizeof v);
    }
}

}  // extern "C"
