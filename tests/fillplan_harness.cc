// fillplan_harness.cc -- how a cost volume gets filled (mgm_amd/csrc/mgm_fillplan.h) behind a C interface for
// tests/test_fillplan.py.  Built with plain g++ and no ROCm include path: that it compiles is the test that the policy is HIP-free.
#include <cstring>

#include "mgm_fillplan.h"

using namespace mgm;

namespace {

constexpr int kReqInts = 18, kPlanInts = 20, kMaxAttempts = 8, kWalkInts = 5 + 4 * kMaxAttempts;

FillRequest request(const int *a, float truncDist)
{
    FillRequest q{};
    q.nx = a[0], q.ny = a[1], q.vnx = a[2], q.vny = a[3], q.nch = a[4], q.L = a[5], q.dist = a[6], q.pre = a[7], q.census_win = a[8];
    q.truncDist = truncDist;
    q.ragged = a[9] != 0;
    q.mem.diff_fails = a[10], q.mem.diff_wide = a[11] != 0, q.mem.rel_hint_slots = a[12];
    q.c8 = a[13] != 0, q.pad = a[14] != 0, q.lazy_f32 = a[15] != 0, q.rel = a[16] != 0, q.rel_direct = a[17] != 0;
    return q;
}

void put_attempt(const FillAttempt &a, long long *out) { out[0] = (int)a.form, out[1] = a.slots, out[2] = a.cbytes, out[3] = a.readback; }

}  // namespace

extern "C" {

void fillplan_limits(int *out) { out[0] = kReqInts, out[1] = kPlanInts, out[2] = kWalkInts, out[3] = kMaxAttempts; }

// The refusal's message of one request ("" where the request is planned).
const char *fillplan_message(const int *req, float truncDist)
{
    const FillPlan p = plan_fill(request(req, truncDist));
    return p.msg ? p.msg : "";
}

// n requests -> plans [n][kPlanInts]: err, costfn, pre, census_words, nan_words, nch, bits of trunc, inputs, bytes_u, bytes_v,
// bytes_tmp, first (form, slots, cbytes, readback), general (likewise), gather_cb -- and walks [n][kWalkInts] with the scripted flag
// words (attempt i comes back with flags[min(i, nflags - 1)]): attempts made (-1: no end within kMaxAttempts), the memory afterwards
// (diff_fails, diff_wide, rel_hint_slots), a spare word, then the attempts (form, slots, cbytes, readback).
void fillplan_batch(int n, const int *req, const float *truncDist, int nflags, const unsigned *flags, long long *plans, long long *walks)
{
    for (int i = 0; i < n; i++) {
        const FillRequest q = request(req + (size_t)i * kReqInts, truncDist[i]);
        const FillPlan p = plan_fill(q);
        long long *po = plans + (size_t)i * kPlanInts, *wo = walks + (size_t)i * kWalkInts;
        memset(po, 0, sizeof(long long) * kPlanInts);
        memset(wo, 0, sizeof(long long) * kWalkInts);
        po[0] = p.err;
        if (p.err) continue;
        unsigned tb;
        memcpy(&tb, &p.trunc, 4);
        po[1] = p.costfn, po[2] = p.pre, po[3] = p.census_words, po[4] = p.nan_words, po[5] = p.nch, po[6] = tb, po[7] = (int)p.inputs;
        po[8] = (long long)p.bytes_u, po[9] = (long long)p.bytes_v, po[10] = (long long)p.bytes_tmp;
        put_attempt(p.first, po + 11);
        put_attempt(p.general, po + 15);
        po[19] = p.gather_cb;
        FillMemory mem = q.mem;
        FillAttempt a = p.first;
        wo[0] = -1;
        for (int k = 0; k < kMaxAttempts; k++) {
            put_attempt(a, wo + 5 + 4 * k);
            const FillStep s = fill_step(p, a, flags[k < nflags ? k : nflags - 1], mem);
            mem = s.mem;
            if (s.done) {
                wo[0] = k + 1;
                break;
            }
            a = s.next;
        }
        wo[1] = mem.diff_fails, wo[2] = mem.diff_wide, wo[3] = mem.rel_hint_slots;
    }
}

// The gathered copy's ladder: returns 1 and the wider format, or 0 (the copy is given up).
int fillplan_rel_next_format(unsigned flag, int hull_current, int *slots, int *cb) { return rel_next_format(flag, hull_current != 0, slots, cb); }

int fillplan_padded_labels(int L) { return padded_labels(L); }
int fillplan_c8_supported(int L) { return c8_supported(L); }
int fillplan_is_byte_code(float t) { return is_byte_code(t); }

}  // extern "C"
