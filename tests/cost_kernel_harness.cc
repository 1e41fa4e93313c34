// cost_kernel_harness.cc -- plan_cost_kernel and cost_request (mgm_amd/csrc/mgm_fillplan.h) behind a C interface for
// tests/test_cost_kernel_plan.py and tests/test_gpu_cost_choice.py.  Built with plain g++ and no ROCm include path, like
// fillplan_harness.cc.
#include <cstring>

#include "mgm_fillplan.h"

using namespace mgm;

namespace {

constexpr int kReqInts = 14, kOutInts = 14, kNameBytes = 24, kFillInts = 18, kMaxAttempts = 8;

void put_choice(const CostKernelChoice &c, long long *o, char *name)
{
    const long long v[kOutInts] = {(int)c.family, c.FN, c.W4, c.CB, c.SD, c.NCH, c.LN, c.HW, (int)c.pre, c.pre_grid_u, c.pre_grid_v, c.grid, (long long)c.lds, c.tb};
    memcpy(o, v, sizeof v);
    strncpy(name, c.name, kNameBytes);  // (pads with zeros)
}

FillRequest fill_request(const int *a, float truncDist)  // the columns of tests/test_fillplan.py
{
    FillRequest q{};
    q.nx = a[0], q.ny = a[1], q.vnx = a[2], q.vny = a[3], q.nch = a[4], q.L = a[5], q.dist = a[6], q.pre = a[7], q.census_win = a[8];
    q.truncDist = truncDist;
    q.ragged = a[9] != 0;
    q.mem.diff_fails = a[10], q.mem.diff_wide = a[11] != 0, q.mem.rel_hint_slots = a[12];
    q.c8 = a[13] != 0, q.pad = a[14] != 0, q.lazy_f32 = a[15] != 0, q.rel = a[16] != 0, q.rel_direct = a[17] != 0;
    return q;
}

}  // namespace

extern "C" {

int cost_kernel_c8_supported(int L) { return c8_supported(L); }
void cost_kernel_limits(int *out) { out[0] = kReqInts, out[1] = kOutInts, out[2] = kNameBytes, out[3] = kFillInts, out[4] = kMaxAttempts; }

// n requests [n][kReqInts] = costfn, nch, nx, ny, vnx, vny, L, Lreal, cbytes, hwin, fp32 target, compact target, ragged, scratch (and the
// truncation) -> out [n][kOutInts] = family, FN, W4, CB, SD, NCH, LN, HW, pre, pre_grid_u, pre_grid_v, grid, lds, tb; names [n][kNameBytes]
void cost_kernel_plan(int n, const int *req, const float *trunc, long long *out, char *names)
{
    for (int i = 0; i < n; i++) {
        const int *a = req + (size_t)i * kReqInts;
        CostKernelRequest q{};
        q.costfn = a[0], q.nch = a[1], q.nx = a[2], q.ny = a[3], q.vnx = a[4], q.vny = a[5], q.L = a[6], q.Lreal = a[7], q.cbytes = a[8], q.hwin = a[9];
        q.trunc = trunc[i];
        q.f32 = a[10] != 0, q.compact = a[11] != 0, q.ragged = a[12] != 0, q.scratch = a[13] != 0;
        put_choice(plan_cost_kernel(q), out + (size_t)i * kOutInts, names + (size_t)i * kNameBytes);
    }
}

// The instance list: out [count][8] = family, FN, W4, CB, SD, NCH, LN, HW and the name of each; returns the count.
int cost_kernel_instances(int room, long long *out, char *names)
{
    int n = 0;
    for (const CostInstance &k : kCostInstances) {
        if (n < room) {
            const long long v[8] = {(int)k.family, k.FN, k.W4, k.CB, k.SD, k.NCH, k.LN, k.HW};
            memcpy(out + (size_t)n * 8, v, sizeof v);
            strncpy(names + (size_t)n * kNameBytes, cost_kernel_name(k), kNameBytes);
        }
        n++;
    }
    return n;
}

// The walks of n fill requests [n][kFillInts] under scripted flag words, as the driver makes them (run_attempts, mgm_volume.hip):
// every attempt but a RelDirect one goes through cost_request and plan_cost_kernel.  walks [n][1 + 2 * kMaxAttempts] = attempts made
// (0: the request is refused by plan_fill), then (form, family or -1 for a RelDirect attempt) of each; names [n][kMaxAttempts][kNameBytes].
void cost_kernel_walks(int n, const int *req, const float *truncDist, int nflags, const unsigned *flags, long long *walks, char *names)
{
    memset(walks, 0, sizeof(long long) * (size_t)n * (1 + 2 * kMaxAttempts));
    memset(names, 0, (size_t)n * kMaxAttempts * kNameBytes);
    for (int i = 0; i < n; i++) {
        const FillRequest q = fill_request(req + (size_t)i * kFillInts, truncDist[i]);
        const FillPlan p = plan_fill(q);
        if (p.err) continue;
        long long *wo = walks + (size_t)i * (1 + 2 * kMaxAttempts);
        FillMemory mem = q.mem;
        FillAttempt a = p.first;
        for (int k = 0; k < kMaxAttempts; k++) {
            wo[1 + 2 * k] = (int)a.form, wo[2 + 2 * k] = -1;
            if (a.form != FillForm::RelDirect) {
                const CostKernelChoice c = plan_cost_kernel(cost_request(q, p, a));
                wo[2 + 2 * k] = (int)c.family;
                strncpy(names + ((size_t)i * kMaxAttempts + k) * kNameBytes, c.name, kNameBytes);
            }
            const FillStep s = fill_step(p, a, flags[k < nflags ? k : nflags - 1], mem);
            mem = s.mem;
            wo[0] = k + 1;
            if (s.done) break;
            a = s.next;
        }
    }
}

}  // extern "C"
