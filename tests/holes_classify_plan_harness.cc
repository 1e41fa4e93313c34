// holes_classify_plan_harness.cc -- plan_holes_classify (mgm_amd/csrc/mgm_planner.h) behind a C interface for
// tests/test_occlusion_model.py and tests/test_gpu_occlusion.py (which reads the segment and the span from it).  Built with plain g++
// and no ROCm include path, like holes_plan_harness.cc.
#include "mgm_planner.h"

using namespace mgm;

extern "C" {

int holes_classify_request_bytes() { return (int)sizeof(HolesClassifyRequest); }
int holes_classify_choice_bytes() { return (int)sizeof(HolesClassifyChoice); }
int holes_classify_threads() { return kHolesThreads; }
int holes_classify_max_span() { return kHolesClsMaxSpan; }

// `n` requests, each five int64: nx, ny, vnx, L, num_cu; per request out[6] = family, seg, span, grid_x, grid_y, lds_bytes
void holes_classify_plan(const long long *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        const long long *r = reqs + (size_t)i * 5;
        HolesClassifyRequest q{};
        q.nx = (int)r[0], q.ny = (int)r[1], q.vnx = (int)r[2], q.L = r[3], q.num_cu = (int)r[4];
        const HolesClassifyChoice c = plan_holes_classify(q);
        const long long v[6] = {c.family, c.seg, c.span, c.grid_x, c.grid_y, c.lds_bytes};
        memcpy(out + (size_t)i * 6, v, sizeof v);
    }
}

}  // extern "C"
