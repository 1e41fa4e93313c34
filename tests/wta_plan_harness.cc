// wta_plan_harness.cc -- plan_wta, plan_wta_right and plan_wta_rel (mgm_amd/csrc/mgm_planner.h) behind a C interface for
// tests/test_wta_plan.py.  Built with plain g++ and no ROCm include path, like planner_harness.cc.
#include "mgm_planner.h"

using namespace mgm;

extern "C" {

int wta_request_bytes() { return (int)sizeof(WtaRequest); }
int wta_right_request_bytes() { return (int)sizeof(WtaRightRequest); }
int wta_rel_request_bytes() { return (int)sizeof(WtaRelRequest); }

// `n` requests as their bytes, one after the other (integers only, no padding: static_assert in the header); per request
// out[9] = family, LPL, PPW, EXACT, MAXD, SUB, ALLD, grid, prune
void wta_plan(const unsigned char *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        WtaRequest q;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        const WtaChoice c = plan_wta(q);
        const long long v[9] = {c.family, c.LPL, c.PPW, c.EXACT, c.MAXD, c.SUB, c.ALLD, c.grid, c.prune};
        memcpy(out + (size_t)i * 9, v, sizeof v);
    }
}

// out[6] = family, LPL, PPW, seg, ring, grid
void wta_right_plan(const unsigned char *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        WtaRightRequest q;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        const WtaRightChoice c = plan_wta_right(q);
        const long long v[6] = {c.family, c.LPL, c.PPW, c.seg, c.ring, c.grid};
        memcpy(out + (size_t)i * 6, v, sizeof v);
    }
}

// out[3] = SPL, CB, grid
void wta_rel_plan(const unsigned char *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        WtaRelRequest q;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        const WtaRelChoice c = plan_wta_rel(q);
        const long long v[3] = {c.SPL, c.CB, c.grid};
        memcpy(out + (size_t)i * 3, v, sizeof v);
    }
}

}  // extern "C"
