// route_plan_harness.cc -- plan_agg_route, plan_subbatch / shrink_after_nomem and plan_dense_kernels (mgm_amd/csrc/mgm_planner.h)
// behind a C interface for tests/test_route_plan.py.  Built with plain g++ and no ROCm include path, like planner_harness.cc.
// The two planners that ask for facts are DRIVEN here the way mgm_api.hip / mgm_plan.hip drive them: ask, copy the one named
// fact from a table into the request, ask again -- the table being the same request with every fact of the device filled in.
#include "mgm_planner.h"

using namespace mgm;

enum { kMaxLog = 24 };  // a weight scan + 16 volumes + two pad tries, with room to spare

extern "C" {

int route_request_bytes() { return (int)sizeof(RouteRequest); }
int subbatch_request_bytes() { return (int)sizeof(SubbatchRequest); }
int dense_kernels_request_bytes() { return (int)sizeof(DenseKernelsRequest); }

// per request out[3 + 2 * kMaxLog] = route, rel_weighted, probes (-1: the planner kept asking), then (need, arg) per probe
void route_drive(const unsigned char *reqs, const unsigned char *facts, int n, int *out)
{
    for (int i = 0; i < n; i++) {
        RouteRequest q, f;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        memcpy(&f, facts + (size_t)i * sizeof f, sizeof f);
        int *o = out + (size_t)i * (3 + 2 * kMaxLog), nlog = 0;
        RouteDecision d;
        while ((d = plan_agg_route(q)).need != kNeedNothing && nlog < kMaxLog) {
            o[3 + 2 * nlog] = d.need, o[4 + 2 * nlog] = d.arg, nlog++;
            if (d.need == kNeedWeightValues) q.w_odd = f.w_odd, q.w_any = f.w_any;
            else if (d.need == kNeedRelCopy) q.rel_usable[d.arg] = f.rel_usable[d.arg], q.rel_slots[d.arg] = f.rel_slots[d.arg], q.rel_cb[d.arg] = f.rel_cb[d.arg];
            else nlog = kMaxLog;
        }
        o[0] = d.route, o[1] = d.rel_weighted, o[2] = d.need == kNeedNothing ? nlog : -1;
    }
}

// per request out[17 + 2 * kMaxLog] = err, exact, first_build, L, padded, own_padded, use_c8, cb, weighted, weighted_given, w2cand, ragged,
// fh2_ragged, borrow_ones, need_pad_f32, pad_hint, probes, then (need, arg) per probe
void dense_kernels_drive(const unsigned char *reqs, const unsigned char *facts, int n, int *out)
{
    for (int i = 0; i < n; i++) {
        DenseKernelsRequest q, f;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        memcpy(&f, facts + (size_t)i * sizeof f, sizeof f);
        int *o = out + (size_t)i * (17 + 2 * kMaxLog), nlog = 0;
        DenseKernels d;
        while ((d = plan_dense_kernels(q)).need != kNeedNothing && nlog < kMaxLog) {
            o[17 + 2 * nlog] = d.need, o[18 + 2 * nlog] = d.arg, nlog++;
            if (d.need == kNeedWeightValues) {
                memcpy(q.w_not_one, f.w_not_one, sizeof q.w_not_one);
                memcpy(q.w_odd, f.w_odd, sizeof q.w_odd);
                memcpy(q.w_one_other, f.w_one_other, sizeof q.w_one_other);
            } else if (d.need == kNeedCompactCopy)
                q.c8_use[d.arg] = f.c8_use[d.arg], q.c8_bytes[d.arg] = f.c8_bytes[d.arg], q.nan_found[d.arg] = f.nan_found[d.arg];
            else if (d.need == kNeedPadTry && d.arg >= 1 && d.arg <= 2)
                q.pad_fits[d.arg] = f.pad_fits[d.arg];
            else
                nlog = kMaxLog;
        }
        const int v[17] = {d.err, d.exact, d.first_build, d.L, d.padded, d.own_padded, d.use_c8, d.cb, d.weighted, d.weighted_given, d.w2cand, d.ragged,
                           d.fh2_ragged, d.borrow_ones, d.need_pad_f32, d.pad_hint, d.need == kNeedNothing ? nlog : -1};
        memcpy(o, v, sizeof v);
    }
}

// out[n] = the first chunk
void subbatch_plan(const unsigned char *reqs, int n, int *out)
{
    for (int i = 0; i < n; i++) {
        SubbatchRequest q;
        memcpy(&q, reqs + (size_t)i * sizeof q, sizeof q);
        out[i] = plan_subbatch(q);
    }
}
int subbatch_shrink(int route, int m) { return shrink_after_nomem(route, m); }

}  // extern "C"
