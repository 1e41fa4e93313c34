// prune_harness.cc -- plan_wta_prune (mgm_amd/csrc/mgm_planner.h) behind a C interface for tests/test_wta_prune_planner.py.
// Built with plain g++ and no ROCm include path, like planner_harness.cc.
#include "mgm_planner.h"

using namespace mgm;

extern "C" {

int prune_request_fields() { return (int)(sizeof(PruneRequest) / sizeof(int)); }
int dense_request_fields() { return (int)(sizeof(DenseRequest) / sizeof(int)); }

// the decision for a request given field by field (the order of PruneRequest)
int prune_decision(const int *a)
{
    PruneRequest q;
    memcpy(&q, a, sizeof q);  // (integers only, no padding: static_assert in the header)
    return plan_wta_prune(q) ? 1 : 0;
}

// ... and for a launch as mgm_plan.hip fills it: the plan of `dense` (the fields of DenseRequest, in order) decides R2, subv,
// tags, w2, wk; call = {enabled, search_follows, want_S, refine, slot0, nslots, Lreal, stride_mod32}
int prune_for_launch(const int *dense, const int *call)
{
    DenseRequest d;
    memcpy(&d, dense, sizeof d);
    const DensePlan p = plan_dense(d);
    if (p.err) return -1;
    PruneRequest q{};
    q.enabled = call[0], q.search_follows = call[1], q.want_S = call[2], q.refine = call[3];
    q.first = d.first, q.count = d.count, q.slot0 = call[4], q.nslots = call[5];
    q.L = d.L, q.Lreal = call[6], q.ragged = d.ragged;
    q.R2 = p.R2, q.subv = p.subv, q.tags = p.tags, q.w2 = p.w2, q.wk = p.wk, q.lpl = d.lpl;
    q.use_c8 = d.use_c8, q.cb = d.cb, q.stride_mod32 = call[7];
    return plan_wta_prune(q) ? 1 : 0;
}

}  // extern "C"
