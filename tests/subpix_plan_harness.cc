// subpix_plan_harness.cc -- plan_subpix (mgm_amd/csrc/mgm_planner.h) behind a C interface for tests/test_subpix_plan.py.  Built with
// plain g++ and no ROCm include path, like holes_plan_harness.cc.
#include "mgm_planner.h"

using namespace mgm;

extern "C" {

int subpix_request_bytes() { return (int)sizeof(SubpixRequest); }
int subpix_choice_bytes() { return (int)sizeof(SubpixChoice); }
int subpix_threads() { return kSubpixThreads; }
int subpix_span_bytes() { return kSubpixSpanBytes; }
int subpix_max_labels() { return kSubpixMaxLabels; }

// `n` requests of seven 64-bit integers each: npix, labels, slots, in_slots, s, cb, num_cu; per request
// out[5] = family, grid, pix, vec, chunks
void subpix_plan(const long long *reqs, int n, long long *out)
{
    for (int i = 0; i < n; i++) {
        const long long *r = reqs + (size_t)i * 7;
        const SubpixRequest q{r[0], (int)r[1], (int)r[2], (int)r[3], (int)r[4], (int)r[5], (int)r[6]};
        const SubpixChoice c = plan_subpix(q);
        const long long v[5] = {c.family, c.grid, c.pix, c.vec, c.chunks};
        memcpy(out + (size_t)i * 5, v, sizeof v);
    }
}

}  // extern "C"
