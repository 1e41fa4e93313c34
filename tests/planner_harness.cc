// planner_harness.cc -- the launch planner (mgm_amd/csrc/mgm_planner.h) behind a C interface for tests/test_planner.py.
// Built with plain g++ and no ROCm include path: that it compiles is the test that the planner is HIP-free.
#include "mgm_planner.h"

using namespace mgm;

namespace {

DenseRequest dense_request(const int *a)
{
    DenseRequest q{};
    q.nx = a[0], q.ny = a[1], q.L = a[2], q.nb = a[3], q.first = a[4], q.count = a[5], q.layout_ndir = a[6], q.MGM = a[7], q.fh = a[8];
    q.wmode = a[9], q.use_c8 = a[10], q.cb = a[11], q.first_build = a[12], q.ragged = a[13];
    q.lines2 = a[14], q.lpl = a[15], q.ns = a[16], q.devtools = a[17], q.num_cu = a[18], q.xcc_mask = a[19];
    q.subv = a[20], q.deep = a[21], q.wg_per_cu = a[22], q.strips = a[23], q.xcdq = a[24], q.xcdq_k = a[25], q.one_queue = a[26], q.w2 = a[27], q.oneb = a[28];
    return q;
}

RelRequest rel_request(const int *a)
{
    RelRequest q{};
    q.nx = a[0], q.ny = a[1], q.NDIR = a[2], q.nb = a[3], q.MGM = a[4], q.fh = a[5], q.pube = a[6], q.fh2 = a[7], q.slots = a[8], q.cb = a[9];
    q.R = a[10], q.HS = a[11], q.diag_fits = a[12], q.num_cu = a[13];
    q.rel_wg = a[14], q.rel_prio = a[15], q.rel_lag = a[16], q.rel_lagd = a[17], q.rel_slots = a[18], q.rel_slope1 = a[19], q.rel_swap = a[20], q.rel_diag = a[21],
    q.rel_strips = a[22], q.rel_multi = a[23];
    return q;
}

// per pass: NL, LL, form, nbands, slope, nstrips, split, swap, diag, wmax; hand_base apart (64 bits)
void put_geoms(const PassGeom *g, int *geom, long long *hand_base)
{
    for (int k = 0; k < kMaxDirs; k++) {
        const int v[10] = {g[k].NL, g[k].LL, g[k].form, g[k].nbands, g[k].slope, g[k].nstrips, g[k].split, g[k].swap, g[k].diag, g[k].wmax};
        for (int i = 0; i < 10; i++) geom[k * 10 + i] = v[i];
        hand_base[k] = g[k].hand_base;
    }
}

int put_tasks(const std::vector<Task> &t, int *out, int cap)
{
    if ((int)t.size() > cap) return -1;
    for (size_t i = 0; i < t.size(); i++) out[2 * i] = t[i].x, out[2 * i + 1] = t[i].y;
    return (int)t.size();
}

}  // namespace

extern "C" {

void planner_limits(int *out)
{
    out[0] = (int)(sizeof(DenseRequest) / sizeof(int));  // fields of the requests: a new one has to reach dense_request / rel_request above
    out[1] = (int)(sizeof(RelRequest) / sizeof(int));
    out[2] = kMaxBands;
}

int planner_dense_subv(const int *req) { return dense_subv(dense_request(req)); }  // (reads nothing that depends on it: lines2 may be 0)
int dense_requests_equal(const int *a, const int *b) { return same_request(dense_request(a), dense_request(b)) ? 1 : 0; }
int rel_requests_equal(const int *a, const int *b) { return same_request(rel_request(a), rel_request(b)) ? 1 : 0; }

// scal: err, subv, ngroups, Lk, R2, R, w2, wk, tags, NS, LPk, wg_per_cu, deep, oneb, xcdq, nq, QK, one_queue, any_strips, maxLL, ntasks,
// hand_vstride, hand layout: npass, groups, slot_floats, slots, R.  Returns the number of table entries (header included), -1: cap too small.
int planner_dense(const int *req, long long *scal, int *geom, long long *hand_base, int *order, int *table, int cap)
{
    const DensePlan p = plan_dense(dense_request(req));
    const long long s[27] = {p.err, p.subv, p.ngroups, p.Lk, p.R2, p.R, p.w2, p.wk, p.tags, p.NS, p.LPk, p.wg_per_cu, p.deep, p.oneb, p.xcdq, p.nq, p.QK, p.one_queue,
                             p.any_strips, p.maxLL, p.ntasks, p.hand_vstride, p.hand.npass, p.hand.groups, p.hand.slot_floats, p.hand.slots, p.hand.R};
    for (int i = 0; i < 27; i++) scal[i] = s[i];
    put_geoms(p.g, geom, hand_base);
    if (put_tasks(p.order, order, cap) < 0) return -1;
    return put_tasks(p.table, table, cap + 8);
}

// scal: err, rel_wg, diag_any, swapmask, maxLL, ntasks, hand_vstride, hand layout: npass, groups, slot_floats, slots, R
int planner_rel(const int *req, long long *scal, int *geom, long long *hand_base, int *order, int *table, int cap)
{
    const RelPlan p = plan_rel(rel_request(req));
    const long long s[12] = {p.err, p.rel_wg, p.diag_any, p.swapmask, p.maxLL, p.ntasks, p.hand_vstride, p.hand.npass, p.hand.groups, p.hand.slot_floats, p.hand.slots, p.hand.R};
    for (int i = 0; i < 12; i++) scal[i] = s[i];
    put_geoms(p.g, geom, hand_base);
    if (put_tasks(p.order, order, cap) < 0) return -1;
    return put_tasks(p.table, table, cap);
}

// the longest chain of a range-proportional launch and every chain's length, as the planner's model has them (what the issue
// priority of the task words is decided by): out[(group * 8 + pass) * 2 + strip] = remaining chain at band 0, 0 where there is none
void planner_rel_chains(const int *req, double *out)
{
    const RelRequest q = rel_request(req);
    const RelPlan p = plan_rel(q);
    for (int i = 0; i < kMaxBatch * kMaxDirs * 2; i++) out[i] = 0.0;
    if (p.err) return;
    const std::vector<SimChain> ch = rel_chains(q, p.g);
    for (const SimChain &k : ch) out[k.x * 2 + k.st] = k.rem_of(0);
}

}  // extern "C"
