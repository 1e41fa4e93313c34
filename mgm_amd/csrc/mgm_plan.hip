// mgm_plan.hip -- a pass launch as stages around the HIP-free planner (mgm_planner.h): resolve the operands on the device,
// fill the request, plan or fetch the plan from the context's cache, reserve the workspace and tag the hand-off region, fill
// the kernel's parameters, launch, remember; and the winner search behind it.  See mgm_host.h.
#include "mgm_host.h"

static_assert(sizeof(Task) == sizeof(int2) && alignof(Task) <= alignof(int2), "task tables are uploaded as the kernels' int2");

static unsigned long long fnv1a64(const void *data, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) h = (h ^ ((const unsigned char *)data)[i]) * 1099511628211ull;
    return h;
}

// ---- helpers of the stages -------------------------------------------------------------------------------------------------
// What values do the weights take?  out[4 * v ..]: launch_weight_values' four words of volume v (volumes without weights keep
// the initial words).  One small scan + read-back per call.
static int scan_weights(mgm_ctx *c, const mgm_img *const *w8s, int nb, long long npix, unsigned *out)
{
    int r;
    if ((r = reserve(c, c->wvals, sizeof(unsigned) * 4 * kMaxBatch))) return r;
    unsigned init[4 * kMaxBatch];
    for (int v = 0; v < nb; v++) init[4 * v] = 0u, init[4 * v + 1] = 0xffffffffu, init[4 * v + 2] = 0u, init[4 * v + 3] = 0u;
    HIPCHK(c, hipMemcpyAsync(c->wvals.p, init, sizeof(unsigned) * 4 * nb, hipMemcpyHostToDevice, c->stream));
    for (int v = 0; v < nb; v++)
        if (w8s[v]) HIPCHK(c, launch_weight_values(w8s[v]->d, npix * 8, (unsigned *)c->wvals.p + 4 * v, c->stream));
    HIPCHK(c, hipMemcpyAsync(out, c->wvals.p, sizeof(unsigned) * 4 * nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MGM_OK;
}

// Weighted launches of the range-proportional kernels: does any weight image hold a value that is not positive and finite
// (<= 0, NaN, INF)?
int weights_have_odd_values(mgm_ctx *c, const mgm_img *const *w8s, int nb, long long npix, bool *odd, bool *any)
{
    *odd = false;
    if (any) *any = false;
    unsigned got[4 * kMaxBatch];
    if (int r = scan_weights(c, w8s, nb, npix, got)) return r;
    for (int v = 0; v < nb; v++) {
        *odd = *odd || (w8s[v] && got[4 * v + 3] != 0);
        if (any) *any = *any || (w8s[v] && got[4 * v] != 0);  // a value != 1.0: the run is a weighted one (mgm_core.cc:420-423)
    }
    return MGM_OK;
}

// The XCC ids the workgroups of a launch see (k_xcc_census): looked at once per context, one small launch and a 4-byte
// read-back; the planner takes the mask as an input.
static int ensure_xcc_mask(mgm_ctx *c)
{
    if (c->xcc_mask >= 0) return MGM_OK;
    unsigned *flag = ctrl_word(c, kWordFlag), mask = 0;
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(unsigned), c->stream));
    HIPCHK(c, launch_xcc_census(flag, c->stream));
    if (int r = read_word(c, flag, &mask)) return r;
    c->xcc_mask = (int)mask;
    return MGM_OK;
}

// A new plan's table goes to the device and the plan into the cache, both or neither: a failure on the way leaves the
// cache as it was.  The cache is bounded -- the oldest entry is dropped; the stream is idle by then (the upload is waited
// for), so no launch still reads the buffer that is freed.
template <class Req, class Plan>
static int cache_put(mgm_ctx *c, PlanCache<Req, Plan> &cache, const Req &req, Plan &plan, const typename PlanCache<Req, Plan>::Entry **out)
{
    Buf fresh{};
    const size_t bytes = sizeof(Task) * plan.table.size();
    if (int r = reserve(c, fresh, bytes)) return r;
    hipError_t ce = hipMemcpyAsync(fresh.p, plan.table.data(), bytes, hipMemcpyHostToDevice, c->stream);
    if (ce == hipSuccess) ce = hipStreamSynchronize(c->stream);
    if (ce != hipSuccess) {
        (void)hipFree(fresh.p);
        return hipfail(c, ce, "task table upload");
    }
    if (cache.entries.size() >= cache.kMaxEntries) {
        if (cache.entries.front().buf.p) (void)hipFree(cache.entries.front().buf.p);
        cache.entries.erase(cache.entries.begin());
    }
    const unsigned long long fnv = fnv1a64(plan.table.data(), bytes);
    std::vector<Task>().swap(plan.order);  // (the entry keeps the decisions; the table lives on the device)
    std::vector<Task>().swap(plan.table);
    cache.entries.push_back({req, plan, fresh, fnv});
    *out = &cache.entries.back();
    return MGM_OK;
}

// `launch`: the launch a plan without a kernel instance used to fail at (its message names the call as it always has)
static int plan_error(mgm_ctx *c, int err, const char *launch)
{
    if (err == kPlanNoKernel) return hipfail(c, hipErrorInvalidValue, launch);
    if (err == kPlanNotCanonical) return fail(c, MGM_ERR_INTERNAL, "pass table does not reduce to canonical form");
    if (err == kPlanTooManyBands) return fail(c, MGM_ERR_UNSUPPORTED, "image side exceeds 65536 pixels");
    return fail(c, MGM_ERR_INTERNAL, "two-valued weights: the launch plan lost its queues");
}

// "this was the context's last aggregation": what mgm_wta_windowed_dev / mgm_debug_download_lr / the winner search of a later
// call find (DenseRun, RelRun: mgm_host.h).  pad8: the padded compact copies of a padded launch (per volume), or nullptr;
// minima: the launch wrote the chunk minima of its Lr volumes.
// kernel: the instance that ran (nullptr: k_pass_exact)
static void remember_dense(mgm_ctx *c, const mgm_cv *const *Cs, int nb, long long nvol, long long lr_stride, int nslots, int Lreal, int Lk, int pad_cb,
                           const uint8_t *const *pad8, bool minima, const PassKernelChoice *kernel)
{
    c->rel_last.clear();  // (an earlier range-proportional aggregation of the same volume is no longer the context's last)
    DenseRun &d = c->last;
    d = DenseRun{};
    d.nvol = nvol, d.stride = lr_stride, d.ndir = nslots, d.batch = nb, d.L = Lreal, d.Lk = Lk;
    d.wrote_min = minima;
    if (kernel) d.kernel = *kernel;
    d.pad_c8 = pad8 != nullptr, d.pad_cb = pad_cb;
    for (int v = 0; v < nb; v++) d.pad_ptr[v] = pad8 ? pad8[v] : nullptr, d.cvs[v] = Cs[v], d.gens[v] = Cs[v]->gen;
}
static void remember_rel(mgm_ctx *c, const mgm_cv *const *Cs, int nb, int NDIR, long long stride, const PassKernelChoice &kernel)
{
    c->last.clear();  // (the dense Lr workspace no longer belongs to these volumes)
    RelRun &d = c->rel_last;
    d = RelRun{};
    d.batch = nb, d.ndir = NDIR, d.stride = stride, d.slots = Cs[0]->rel_slots, d.kernel = kernel;
    for (int v = 0; v < nb; v++) d.cvs[v] = Cs[v], d.gens[v] = Cs[v]->gen;
}

// MGM_HIP_TIMELINE=<file>: one line per work item of the launch (tools/timeline.py reads them) -- where the compute units'
// time goes.  `table`: the launch's task table on the device, `header` words of queues in front of its `ntasks` items
// (8: the dense kernels, whose lines name strip and queue; 0: the range-proportional kernels, with `nph` phase clocks per
// item behind the timeline words in a development build); `head` / `tail`: the line of the launch, around its time.
static int dump_timeline(mgm_ctx *c, const char *file, const void *table, int header, int ntasks, int nph, const std::string &head, const std::string &tail)
{
    std::vector<unsigned long long> d((size_t)ntasks * (8 + nph));
    std::vector<int2> tk((size_t)ntasks + header);
    HIPCHK(c, hipMemcpyAsync(d.data(), c->dbg.p, d.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(tk.data(), table, tk.size() * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    FILE *f = fopen(file, "a");
    if (!f) return MGM_OK;
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int i = 0; i < ntasks; i++) {
        if (d[(size_t)i * 8]) t0 = std::min(t0, d[(size_t)i * 8]);
        t1 = std::max(t1, d[(size_t)i * 8 + 1]);
    }
    const double tick = 1e-2;  // wall_clock64: 100 MHz -> 0.01 us
    fprintf(f, "%s %.1f %s\n", head.c_str(), (double)(t1 - t0) * tick, tail.c_str());
    for (int i = 0; i < ntasks; i++) {
        int queue = 0;
        for (int q = 0; q < header; q++)
            if (i >= tk[q].x && i < tk[q].x + tk[q].y) queue = q;
        const int2 t = tk[(size_t)i + header];
        const unsigned long long *w = &d[(size_t)i * 8];
        fprintf(f, "item %d %d %d %d %d %.2f %.2f %.2f %llu %llu %llu %llu %llu\n", i, t.x, t.y & 0xffff, header ? (t.y >> 16) & 0xff : 0, queue,
                (double)(w[0] - t0) * tick, (double)(w[1] - t0) * tick, (double)w[2] * tick, w[3], w[4] & 0xffffffffull, w[4] >> 32, w[5], w[6]);
        if (nph) {  // (development build) clocks per wave: compute, publish, barrier x 4 waves; loader: issue, retire, barrier
            const unsigned long long *q = &d[(size_t)ntasks * 8 + (size_t)i * nph];
            fprintf(f, "phases %d", i);
            for (int k = 0; k < 16; k++) fprintf(f, " %llu", q[k]);
            fprintf(f, "\n");
        }
    }
    fclose(f);
    return MGM_OK;
}

// MGM_HIP_DEBUG_STATS (development builds of the pass kernels): where does K3's time go?  dbg: 16 words per work item;
// items: the launch's task table on the device, behind its header.
static int print_pass_stats(mgm_ctx *c, const unsigned long long *dbg, const int2 *items, int ntasks, int first, int PEND)
{
    std::vector<unsigned long long> d((size_t)ntasks * 16);
    std::vector<int2> tk(ntasks);
    HIPCHK(c, hipMemcpyAsync(d.data(), dbg, d.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(tk.data(), items, tk.size() * sizeof(int2), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int i = 0; i < ntasks; i++) {
        t0 = std::min(t0, d[i * 16 + 0]);
        t1 = std::max(t1, d[i * 16 + 2]);
    }
    const double tick = 1e-2;  // wall_clock64: 100 MHz -> 0.01 us
    fprintf(stderr, "[mgm stats] %d workgroups, kernel span %.1f us\n", ntasks, (t1 - t0) * tick);
    if (c->debug_stats >= 2)  // one line per work item: pass, band, strip, ticket, start / first step / end (us), time in the slow path
        for (int i = 0; i < ntasks; i++)
            fprintf(stderr, "[mgm item] %d %d %d %d %.1f %.1f %.1f %.1f\n", tk[i].x % kMaxDirs, tk[i].y & 0xffff, (tk[i].y >> 16) & 0xff, i,
                    (d[i * 16 + 0] - t0) * tick, (d[i * 16 + 1] - t0) * tick, (d[i * 16 + 2] - t0) * tick, d[i * 16 + 6] * tick);
    for (int q = first; q < PEND; q++) {
        double run = 0, slow = 0, pro = 0, nslow = 0, nspin = 0, steps = 0, first = 1e30, last = 0;
        double ai = 0, ar = 0, ab = 0, bi = 0, br = 0, bb = 0, cb = 0, fsw = 0, fn = 0, fmx = 0, frep = 0;
        int n = 0;
        double fa = 0, fb = 0, fc = 0;
        bool dec = false;
        for (int i = 0; i < ntasks; i++)
            if (tk[i].x % kMaxDirs == q) {
                n++;
                if (d[i * 16 + 1] >> 63) {  // barrier-free build: failed polls of the profiled wave by cause
                    dec = true;
                    fa += (double)((d[i * 16 + 1] >> 42) & 0x1fffff);
                    fb += (double)((d[i * 16 + 1] >> 21) & 0x1fffff);
                    fc += (double)(d[i * 16 + 1] & 0x1fffff);
                    d[i * 16 + 1] = d[i * 16 + 0];
                }
                run += (d[i * 16 + 2] - d[i * 16 + 1]) * tick;
                pro += (d[i * 16 + 1] - d[i * 16 + 0]) * tick;
                slow += d[i * 16 + 6] * tick;
                nslow += d[i * 16 + 3];
                nspin += d[i * 16 + 4];
                steps = (double)d[i * 16 + 7];
                ai += d[i * 16 + 8] * tick; ar += d[i * 16 + 9] * tick; ab += d[i * 16 + 10] * tick;
                bi += d[i * 16 + 11] * tick; br += d[i * 16 + 12] * tick; bb += d[i * 16 + 13] * tick;
                cb += d[i * 16 + 14] * tick;
                fsw += (double)(d[i * 16 + 15] >> 44); fn += (double)((d[i * 16 + 15] >> 18) & 0x3ffff);
                frep += (double)(d[i * 16 + 15] & 0x3ffff);
                fmx = std::max(fmx, (double)((d[i * 16 + 15] >> 36) & 0xff));
                first = std::min(first, (double)(d[i * 16 + 0] - t0) * tick);
                last = std::max(last, (double)(d[i * 16 + 2] - t0) * tick);
            }
        fprintf(stderr,
                "[mgm stats] pass %d: %d bands x %.0f steps; per band: prologue %.1f us, main loop %.1f us (%.3f us/step), "
                "slow-path %.1f us in %.1f polls (%.0f spins); pass active %.1f..%.1f us\n",
                q, n, steps, pro / n, run / n, run / n / steps, slow / n, nslow / n, nspin / n, first, last);
        fprintf(stderr,
                "[mgm stats]         loader A: issue %.0f retire %.0f barrier %.0f us | compute wave: barrier-wait %.0f us; "
                "kcycles per band: lds-read %.0f combine %.0f store+min %.0f transform %.0f lds-write %.0f\n",
                ai / n, ar / n, ab / n, cb / n, nslow / n / 1e3, nspin / n / 1e3, bi / tick / n / 1e3, br / tick / n / 1e3,
                bb / tick / n / 1e3);
        if (dec)
            fprintf(stderr, "[mgm stats]         failed polls per band: previous line %.0f, next line %.0f, DMA %.0f\n", fa / n,
                    fb / n, fc / n);
        if (fn > 0)
            fprintf(stderr, "[mgm stats]         FH min-convolution: %.3f sweeps per slab (fwd+bwd, minimum 2), worst %.0f, %.2f%% of slabs repaired\n",
                    fsw / fn, fmx, 100.0 * frep / fn);
    }
    return MGM_OK;
}

// K3 for the volumes whose aggregation can meet NaNs: the slow, operand-order-faithful kernel (mgm_pass_exact.hip) --
// the reference's own update functions and schedule, one launch per diagonal, every minimum as the reference writes it.
static int run_passes_exact(mgm_ctx *c, const mgm_cv *const *Cs, const mgm_img *const *w8s, int nb, float P1, float P2, int MGM,
                            bool fh, bool weighted, int first, int count, int slot0, int nslots)
{
    const mgm_cv *C = Cs[0];
    const int nx = C->nx, ny = C->ny, L = C->dmax - C->dmin + 1;
    const long long npix = (long long)nx * ny, nvol = npix * L;
    const long long lr_stride = nvol + lr_pad_floats();
    int r;
    if ((r = reserve(c, c->lr, sizeof(float) * (size_t)lr_stride * nslots * nb))) return r;
    if ((r = reserve(c, c->exact_mins, sizeof(float) * (size_t)npix * count))) return r;
    const bool big_fh = fh && (size_t)L * 16 > 128 * 1024;  // the four convolution arrays of a pixel do not fit the LDS
    if (big_fh && (r = reserve(c, c->exact_scratch, sizeof(float) * (size_t)count * std::max(nx, ny) * 4 * (size_t)L))) return r;
    ExactParams p{};
    p.nx = nx;
    p.ny = ny;
    p.L = L;
    p.P1 = P1;
    p.P2 = P2;
    p.MGM = MGM;
    // which of the four update functions (mgm_core.cc:548-571)
    p.mode = weighted ? (fh ? 3 : 1) : (fh ? (MGM == 2 ? 2 : 3) : (MGM == 2 ? 0 : 1));
    p.mins = (float *)c->exact_mins.p;
    p.fhscratch = big_fh ? (float *)c->exact_scratch.p : nullptr;
    for (int v = 0; v < nb; v++) {
        if ((r = ensure_f32(c, Cs[v]))) return r;
        p.C = Cs[v]->d;
        p.dmin = Cs[v]->dmin;
        p.w8 = weighted ? w8s[v]->d : nullptr;
        p.rlo = Cs[v]->rlo;
        p.rhi = Cs[v]->rhi;
        // (round 6) all passes of the volume in ONE sweep of launches, one per diagonal (they are independent: blockIdx.y = pass);
        // every pixel writes its whole slab when its diagonal comes, so Lr = CC (495-498) needs no copy
        p.npass = count;
        for (int q = first; q < first + count; q++) {
            const RefPass &rp = kPasses[q];
            ExactPass &g = p.pass[q - first];
            for (int k = 0; k < 4; k++) {
                g.d[k][0] = rp.d[k][0];
                g.d[k][1] = rp.d[k][1];
                g.wplane[k] = kPassToChannel[k][q];
            }
            g.inc_x = rp.inc_x;
            g.inc_y = rp.inc_y;
            g.row_major = rp.row_major;
            g.Lr = (float *)c->lr.p + ((size_t)v * nslots + slot0 + (q - first)) * lr_stride;
        }
        TimeScope t(c, "k_pass_exact");
        HIPCHK(c, launch_pass_exact(p, c->stream));
    }
    remember_dense(c, Cs, nb, nvol, lr_stride, nslots, L, L, 1, nullptr, false, nullptr);
    return MGM_OK;
}

// ---- K3 on the dense layout --------------------------------------------------------------------------------------------------
// Stage 1 of a dense launch: what the volumes and weights of the call ARE, found out on the device -- the weights' values,
// NaN costs, the compact and padded forms of the costs -- and with that, which kernels can take them: the decision is
// plan_dense_kernels' (mgm_planner.h), which asks for those facts one at a time; what is left here is probing and materialising.
static_assert(kFastKernelLabels == kMaxLPL * 64, "plan_dense_kernels: the widest fast pass kernel");
struct DenseOperands : DenseKernels {
    int Lreal = 0;              // labels of the volumes
    float w2a[kMaxBatch] = {};  // two-valued weights: the other value
    const float *ones8 = nullptr;  // all-ones weights of a ragged FH launch without weights (it borrows the weighted kernels)
};

static int pad_f32(mgm_ctx *c, const mgm_cv *const *Cs, int nb, long long npix, int Lreal, int L)
{
    for (int v = 0; v < nb; v++) {
        int r;
        if ((r = ensure_f32(c, Cs[v]))) return r;
        if ((r = reserve(c, c->padf[v], sizeof(float) * (size_t)npix * L))) return r;
        TimeScope t(c, "k_pad");
        HIPCHK(c, launch_pad(Cs[v]->d, npix, Lreal, L, (float *)c->padf[v].p, nullptr, 1, nullptr, c->stream));
    }
    return MGM_OK;
}

// padded copies of the costs of all volumes as compact costs of `tb` bytes (mgm_ctx::pad8): *fits = every cost has a code
static int try_pad(mgm_ctx *c, const mgm_cv *const *Cs, int nb, long long npix, int Lreal, int L, int tb, int *fits)
{
    unsigned *flag = ctrl_word(c, kWordFlag), misfits = 0;
    int r;
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(unsigned), c->stream));
    for (int v = 0; v < nb; v++) {
        if ((r = ensure_f32(c, Cs[v]))) return r;
        if ((r = reserve(c, c->pad8[v], (size_t)npix * L * tb))) return r;
        TimeScope ts(c, "k_pad");
        HIPCHK(c, launch_pad(Cs[v]->d, npix, Lreal, L, nullptr, (uint8_t *)c->pad8[v].p, tb, flag, c->stream));
    }
    if ((r = read_word(c, flag, &misfits))) return r;
    *fits = misfits == 0;
    return MGM_OK;
}

// A launch's region of self-validating slots (HandTags): room, its tags, the clear they may ask for.  The caller commits after the enqueue.
static int begin_hand(mgm_ctx *c, HandRegion &h, size_t bytes, const HandLayout &want, int first, int end, HandStep *step)
{
    const void *before = h.buf.p;
    if (int r = reserve(c, h.buf, bytes)) return r;
    *step = hand_begin(h.tags, want, first, end, h.buf.p != before);
    if (step->clear) HIPCHK(c, hipMemsetAsync(h.buf.p, kHandClearByte, bytes, c->stream));
    return MGM_OK;
}

static int dense_error(mgm_ctx *c, int err)
{
    if (err == kDenseMixedWeights) return fail(c, MGM_ERR_UNSUPPORTED, "batched volumes must be all weighted or all unweighted");
    if (err == kDenseRaggedHulls) return fail(c, MGM_ERR_UNSUPPORTED, "batched ragged volumes must share their hull under FH potentials");
    return fail(c, MGM_ERR_UNSUPPORTED, "FH potentials with TSGM=2 and no weights on a ragged cost volume need the second build");
}

static int resolve_dense_operands(mgm_ctx *c, const mgm_cv *const *Cs, const mgm_img *const *w8s, int nb, float P1, float P2, int MGM, bool fh, bool allow_pad,
                                  DenseOperands &o)
{
    const int Lreal = o.Lreal = Cs[0]->dmax - Cs[0]->dmin + 1, LP = padded_labels(Lreal);
    const long long npix = (long long)Cs[0]->nx * Cs[0]->ny;
    int r;
    // the request: what is known without the device ...
    DenseKernelsRequest q{};
    q.nb = nb, q.MGM = MGM, q.fh = fh, q.allow_pad = allow_pad, q.Lreal = Lreal;
    q.p1_nonneg = P1 >= 0.0f, q.p2_nonneg = P2 >= 0.0f, q.p2_finite = P2 < __builtin_huge_valf();
    q.force_build = c->force_build, q.lines_real = pass2_lines(Lreal, false), q.lines_pad = LP ? pass2_lines(LP, false) : 0;
    q.lpl_real = pass_lpl(Lreal), q.lpl_pad = LP ? pass_lpl(LP) : 0;
    q.sw_pad = dev().pad, q.sw_c8 = dev().c8, q.sw_deep = dev().deep;
    q.weights_given = w8s && w8s[0], q.same_hull = 1, q.pad_hint = Cs[0]->pad_hint;
    for (int v = 0; v < nb; v++) {
        q.w_given[v] = w8s && w8s[v];
        q.ragged |= Cs[v]->rlo != nullptr, q.nan_words |= Cs[v]->nan_words, q.same_hull &= Cs[v]->dmin == Cs[0]->dmin;
        q.p8_valid[v] = Cs[v]->p8_state == CopyState::Valid, q.p8_L[v] = Cs[v]->p8_L, q.p8_cb[v] = Cs[v]->p8_cb;
    }
    // ... and what is not: -1 until the planner has asked for it
    for (int v = 0; v < kMaxBatch; v++) q.w_not_one[v] = q.w_odd[v] = q.w_one_other[v] = q.c8_use[v] = q.c8_bytes[v] = q.nan_found[v] = -1;
    q.pad_fits[0] = q.pad_fits[1] = q.pad_fits[2] = -1;
    DenseKernels d;
    while ((d = plan_dense_kernels(q)).need != kNeedNothing) {
        if (d.need == kNeedWeightValues) {
            unsigned got[4 * kMaxBatch];
            if ((r = scan_weights(c, w8s, nb, npix, got))) return r;
            for (int v = 0; v < nb; v++) {
                q.w_not_one[v] = got[4 * v] != 0, q.w_odd[v] = got[4 * v + 3] != 0, q.w_one_other[v] = got[4 * v + 1] == got[4 * v + 2];
                if (q.w_given[v] && q.w_not_one[v]) memcpy(&o.w2a[v], &got[4 * v + 1], 4);
                else o.w2a[v] = 1.0f;  // (planes of ones in a weighted launch: no selector bit is set, the other value is never used)
            }
        } else if (d.need == kNeedCompactCopy) {
            bool u = false;
            if ((r = c8_resolve(c, Cs[d.arg], &u))) return r;
            q.c8_use[d.arg] = u, q.c8_bytes[d.arg] = Cs[d.arg]->cbytes, q.nan_found[d.arg] = Cs[d.arg]->nan_state == CopyState::Invalid;
        } else if ((r = try_pad(c, Cs, nb, npix, Lreal, LP, d.arg, &q.pad_fits[d.arg])))  // kNeedPadTry (a padded launch: LP label slots)
            return r;
    }
    if (d.err) return dense_error(c, d.err);
    static_cast<DenseKernels &>(o) = d;
    if (d.exact) return MGM_OK;
    // materialise: the borrowed weights, what the pad tries found, the padded fp32 copies
    if (d.borrow_ones) {
        if ((r = reserve(c, c->ones8, sizeof(float) * (size_t)npix * 8))) return r;
        std::vector<float> one((size_t)npix * 8, 1.0f);
        HIPCHK(c, hipMemcpyAsync(c->ones8.p, one.data(), sizeof(float) * one.size(), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        o.ones8 = (const float *)c->ones8.p;
    }
    if (d.pad_hint >= 0)
        for (int v = 0; v < nb; v++) Cs[v]->pad_hint = d.pad_hint;
    if (d.need_pad_f32 && (r = pad_f32(c, Cs, nb, npix, Lreal, d.L))) return r;
    return MGM_OK;
}

// slot0 / nslots: pass p's Lr volume goes to workspace slot slot0 + (p - first) of nslots (a caller that launches the
// passes of one volume one at a time keeps them all: mgm_aggregate_passes_at_dev); layout_ndir: the hand-off region is
// laid out for the passes [0, layout_ndir) whichever of them this launch runs, so that such a caller's launches share it.
// K3 for the passes [first, first+count) of the reference's table over `nb` cost volumes of identical geometry in one launch
// (see PassVolume); volume v's Lr volumes end up at lr + v*nslots*lr_stride.  Shared by mgm_aggregate_dev and the
// direction-sharded multi-GPU path.
int run_passes(mgm_ctx *c, const mgm_cv *const *Cs, const mgm_img *const *w8s, int nb, float P1, float P2, int MGM,
               int use_fh, int first, int count, bool allow_pad, int slot0, int nslots, int layout_ndir, int search_refine, bool search_S)
{
    if (nslots <= 0) nslots = slot0 + count;
    if (layout_ndir < first + count) layout_ndir = first + count;
    const mgm_cv *C = Cs[0];
    const int nx = C->nx, ny = C->ny;
    const int PEND = first + count;
    const bool fh = use_fh > 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (int r0 = check_watchdog(c, false)) return r0;  // (without waiting: the word is sticky on the device)
    int r;
    if ((r = ensure_words(c))) return r;
    HIPCHK(c, hipMemsetAsync(ctrl_word(c, kWordTicket), 0, sizeof(unsigned), c->stream));  // (the progress words: below, where they are used)

    // 1. the operands, on the device
    DenseOperands o;
    if ((r = resolve_dense_operands(c, Cs, w8s, nb, P1, P2, MGM, fh, allow_pad, o))) return r;
    if (o.exact) return run_passes_exact(c, Cs, w8s, nb, P1, P2, MGM, fh, o.weighted_given, first, count, slot0, nslots);
    const int L = o.L, Lreal = o.Lreal;
    const long long npix = (long long)nx * ny, nvol = npix * L;
    if (!o.first_build && (r = ensure_xcc_mask(c))) return r;

    // 2. the request: everything the plan is a function of
    DenseRequest q{};
    q.nx = nx, q.ny = ny, q.L = L, q.nb = nb, q.first = first, q.count = count, q.layout_ndir = layout_ndir, q.MGM = MGM, q.fh = fh ? 1 : 0;
    q.wmode = o.weighted ? (o.w2cand ? kWeightsTwoValued : kWeightsGeneral) : kWeightsNone;
    q.use_c8 = o.use_c8 ? 1 : 0, q.cb = o.cb, q.first_build = o.first_build ? 1 : 0, q.ragged = o.ragged ? 1 : 0;
    q.lpl = pass_lpl(L), q.ns = pass_ns(fh, o.weighted), q.devtools = pass2_devtools() ? 1 : 0;
    q.num_cu = c->num_cu, q.xcc_mask = c->xcc_mask;
    q.subv = dev().subv, q.deep = dev().deep, q.wg_per_cu = dev().wg_per_cu, q.strips = dev().strips, q.xcdq = dev().xcdq, q.xcdq_k = dev().xcdq_k;
    q.one_queue = (int)tune_num("one_queue", -1), q.w2 = dev().w2 ? 1 : 0, q.oneb = dev().oneb ? 1 : 0;
    q.lines2 = pass2_lines(L * dense_subv(q), o.use_c8);

    // 3. the plan: the context's, if it has launched this request before
    const bool show = tune_num("show_plan", 0) != 0;  // development aid: what the launch heuristics decided
    const auto *e = c->dense_plans.find(q);
    DensePlan fresh;
    if (!e && (fresh = plan_dense(q)).err)
        return plan_error(c, fresh.err, fresh.R2 ? "launch_pass2(p, ntasks, fh, w2 ? 2 : (wk ? 1 : 0), c->stream)" : "launch_pass(p, ntasks, R, fh, o.weighted ? 1 : 0, c->stream)");
    if (show) {
        const DensePlan &d = e ? e->plan : fresh;
        char name[96];
        pass_kernel_name(d.kernel, name, sizeof name);
        fprintf(stderr, "[mgm plan] kernel %s\n", name);
        fprintf(stderr, "[mgm plan] %dx%dx%d passes %d..%d x %d volumes: load/chain %.2f, %d wg/cu, deep %d, subv %d, strips %d, xcd queues %d (block %d; xcc ids seen 0x%x)\n", nx, ny, L,
                first, PEND - 1, nb, d.load_ratio, d.wg_per_cu, d.deep, d.subv, d.any_strips, d.xcdq, d.QK >= (1 << 20) ? 0 : d.QK, (unsigned)c->xcc_mask);
        if (!e)
            fprintf(stderr, "[mgm plan] simulated makespan (steps): one queue %.0f, %d queues (block %d) %.0f -> %s\n", d.t_one, d.nq, d.QK >= (1 << 20) ? 0 : d.QK, d.t_q,
                    d.one_queue ? "one queue" : (d.xcdq ? "per-XCD queues" : "ticket counter"));
    }
    if (!e && (r = cache_put(c, c->dense_plans, q, fresh, &e))) return r;
    if (show) fprintf(stderr, "[mgm plan] table: %d tasks, fnv1a %016llx\n", e->plan.ntasks, e->fnv);
    const DensePlan &plan = e->plan;
    const int ntasks = plan.ntasks, subv = plan.subv, ngroups = plan.ngroups, Lk = plan.Lk, R2 = plan.R2, LPk = plan.LPk, maxLL = plan.maxLL;
    const bool w2 = plan.w2, wk = plan.wk, tags = plan.tags, xcdq = plan.xcdq;

    // 4. the workspace; the hand-off region, cleared or tagged
    // Consecutive passes' volumes are staggered by an odd number of 256-byte blocks so that the
    // NDIR slabs of one pixel (read together by k_wta) do not fall on the same HBM channel.
    const long long lr_stride = nvol + lr_pad_floats();
    if ((r = reserve(c, c->lr, sizeof(float) * (size_t)lr_stride * nslots * nb))) return r;
    PassParams p{};
    // Chunk minima for the pruned winner search (mgm_planner.h, plan_wta_prune): one float per 32 of the Lr workspace, in a
    // grow-only buffer of their own beside it; a launch that does not write them leaves none behind (remember_dense).
    // search_refine >= 0: the caller's own search follows this launch (mgm_aggregate*, a pipelined context's flush included: both
    // run inside one call, so the minima are still there) -- the direction-sharded and multi-device callers pass -1.
    PruneRequest pq{};
    pq.enabled = wta_prune_enabled() ? 1 : 0, pq.search_follows = search_refine >= 0 ? 1 : 0, pq.want_S = search_S ? 1 : 0, pq.refine = std::max(search_refine, 0);
    pq.first = first, pq.count = count, pq.slot0 = slot0, pq.nslots = nslots, pq.L = L, pq.Lreal = Lreal, pq.ragged = o.ragged ? 1 : 0;
    pq.R2 = R2, pq.subv = subv, pq.tags = tags ? 1 : 0, pq.w2 = w2 ? 1 : 0, pq.wk = wk ? 1 : 0, pq.lpl = q.lpl, pq.use_c8 = o.use_c8 ? 1 : 0, pq.cb = o.cb;
    pq.stride_mod32 = (int)(lr_stride % 32);
    const bool minima = plan_wta_prune(pq);
    if (minima) {
        if ((r = reserve(c, c->lmin, sizeof(float) * ((size_t)lr_stride * nslots * nb / kChunkLabels + 8)))) return r;
        p.min_k = (long long)(uintptr_t)c->lmin.p - (long long)((uintptr_t)c->lr.p >> 5) - 3;
    }
    // (the region with tags is laid out for the passes [0, layout_ndir); the other kernels' slots live in `hand2`)
    if (tags) {
        HandStep step;
        if ((r = begin_hand(c, c->hand, sizeof(float) * (size_t)ngroups * plan.hand_vstride * LPk, plan.hand, first, PEND, &step))) return r;
        for (int k = 0; k < kMaxDirs; k++) p.hand_tag[k] = step.tag[k];
        p.hand = (float *)c->hand.buf.p;
    } else {
        if ((r = reserve(c, c->hand2, sizeof(float) * (size_t)nb * kMaxDirs * 2 * maxLL * plan.NS * (subv > 1 ? Lk : q.lpl * 64)))) return r;
        p.hand = (float *)c->hand2.p;
        HIPCHK(c, hipMemsetAsync(ctrl_word(c, kWordProg), 0, sizeof(unsigned) * (size_t)nb * kMaxDirs * kMaxBands, c->stream));
    }
    if ((r = reserve(c, c->handm, sizeof(float) * (size_t)nb * kMaxDirs * 2 * maxLL))) return r;

    // 5. the kernel's parameters
    const uint8_t *pad8[kMaxBatch] = {};
    for (int v = 0; v < nb; v++) {
        if (!o.use_c8 && (r = ensure_f32(c, Cs[v]))) return r;
        pad8[v] = (o.padded && o.use_c8) ? (o.own_padded ? Cs[v]->p8 : (const uint8_t *)c->pad8[v].p) : nullptr;
        p.vol[v].C = o.padded ? (const float *)c->padf[v].p : Cs[v]->d;
        p.vol[v].C8 = o.use_c8 ? (o.padded ? pad8[v] : Cs[v]->d8) : nullptr;
        p.vol[v].Lr = (float *)c->lr.p + ((size_t)v * nslots + slot0) * lr_stride;
        p.vol[v].w8 = o.ones8 ? o.ones8 : (o.weighted ? w8s[v]->d : nullptr);
        p.vol[v].rlo = (fh && o.ragged) ? Cs[v]->rlo : nullptr;
        p.vol[v].rhi = (fh && o.ragged) ? Cs[v]->rhi : nullptr;
        if (w2) {
            if ((r = reserve(c, c->wsel[v], sizeof(unsigned) * 2 * (size_t)npix))) return r;
            HIPCHK(c, launch_wsel(w8s[v]->d, npix, (unsigned *)c->wsel[v].p, c->stream));
            {   // ... + which of a pixel's two transforms its readers pick (k_wneed): what the kernel gets is the combined word
                int dd[8][4][2], pl[8][4];
                for (int k = 0; k < 8; k++)
                    for (int n = 0; n < 4; n++) {
                        dd[k][n][0] = kPasses[k].d[n][0];
                        dd[k][n][1] = kPasses[k].d[n][1];
                        pl[k][n] = kPassToChannel[n][k];
                    }
                HIPCHK(c, launch_wneed((const unsigned *)c->wsel[v].p, nx, ny, MGM, dd, pl, (unsigned *)c->wsel[v].p + npix, c->stream));
            }
            p.vol[v].wsel = (const unsigned *)c->wsel[v].p + npix;
            p.vol[v].p1a = P1 * o.w2a[v];  // (fp32 products, rounded once: what update_costW computes for D = a)
            p.vol[v].p2a = P2 * o.w2a[v];
            // (FH: the cap min(., m + P2*a) is skipped where it cannot bind, as for the unit penalties below)
            if (fh && p.vol[v].p1a >= 0.0f && p.vol[v].p2a >= 4.0f * (float)Lk * p.vol[v].p1a + 4096.0f) p.vol[v].p2a = __builtin_huge_valf();
        }
    }
    for (int k = 0; k < kMaxDirs; k++) p.g[k] = plan.g[k];
    p.hand_vstride = plan.hand_vstride;
    p.wg_per_cu = plan.wg_per_cu;
    p.deep = plan.deep;
    p.handm = (float *)c->handm.p;
    p.ticket = ctrl_word(c, kWordTicket);
    p.err = ctrl_word(c, kWordWatchdog);
    p.prog = ctrl_word(c, kWordProg);
    p.tasks = (const int2 *)e->buf.p + 8;  // (behind the header)
    p.xcdq = xcdq ? (plan.one_queue ? 2 : 1) : 0;
    p.oneb = plan.oneb;
    p.cbytes = o.use_c8 ? o.cb : 1;
    p.qticket = ctrl_word(c, kWordProg);  // (the progress words of the other protocol: the kernels with tags do not use them)
    if (xcdq) HIPCHK(c, hipMemsetAsync(p.qticket, 0, kQueueTickets * sizeof(unsigned), c->stream));
    p.npix = npix;
    p.nvol = lr_stride;
    p.L = L;
    p.Lreal = Lreal;
    p.subv = subv;
    p.fh2_ragged = o.fh2_ragged ? 1 : 0;
    p.MGM = MGM;
    p.dmin = C->dmin;
    p.NDIR = PEND;
    p.pass0 = first;
    p.LLmax = maxLL;
    p.maxbands = kMaxBands;
    p.P1 = P1;
    p.P2 = P2;
    // FH potentials, unweighted, compact costs: min(minconv(L)[o], m + P2) is minconv(L)[o] itself whenever P2 exceeds the
    // longest ramp of a slab by a wide margin -- every label is reached from the slab's minimum in at most L-1 steps of
    // P1, the costs are integers <= 254, so every value of a slab stays below 254 + (L-1)*P1 and the rounding of a ramp
    // of L-1 additions at that magnitude is far below one step.  The kernels skip the cap for P2 = INF (wave-uniform),
    // so it is passed as INF then: same bits, five instructions of the FH step fewer (the reference's own example,
    // P1 = 2, P2 = 20000, is such a case).
    if (fh && tags && o.use_c8 && P1 >= 0.0f && P2 >= 4.0f * (float)Lk * P1 + 4096.0f) p.P2 = __builtin_huge_valf();
    p.dbg = nullptr;
    p.tl_addr = 0;
    p.tl_on = 0;
    p.xflags = dev().xflags;
    // MGM_HIP_TIMELINE=<file> with a -DMGM_P2_TIMELINE=1 build of the pass kernels: one line per work item of every queue
    // launch (tools/timeline.py reads them) -- where the compute units' time goes in a single launch
    const char *tl_file = (xcdq && R2 && pass2_timeline()) ? getenv("MGM_HIP_TIMELINE") : nullptr;
    if (tl_file && *tl_file) {
        if ((r = reserve(c, c->dbg, sizeof(unsigned long long) * 8 * (size_t)ntasks))) return r;
        HIPCHK(c, hipMemsetAsync(c->dbg.p, 0, sizeof(unsigned long long) * 8 * (size_t)ntasks, c->stream));
        p.tl_addr = (unsigned long long)(uintptr_t)c->dbg.p;
        p.tl_on = 1;
    }
    if ((p.xflags || c->debug_stats) && R2 && !pass2_devtools())
        return fail(c, MGM_ERR_UNSUPPORTED, "MGM_HIP_XFLAGS / MGM_HIP_DEBUG_STATS need a development build of the pass kernels "
                                            "(MGM_P2_DEFINES=-DMGM_P2_DEV=1 python -m mgm_amd.build --force)");
    if (c->debug_stats && R2) {
        if ((r = reserve(c, c->dbg, sizeof(unsigned long long) * 16 * (size_t)ntasks))) return r;
        HIPCHK(c, hipMemsetAsync(c->dbg.p, 0, sizeof(unsigned long long) * 16 * (size_t)ntasks, c->stream));
        p.dbg = (unsigned long long *)c->dbg.p;
    }

    // 6. the launch
    {
        TimeScope t(c, R2 ? "k_pass2" : "k_pass");
        if (R2) HIPCHK(c, launch_pass2(p, plan.kernel, ntasks, c->stream));
        else HIPCHK(c, launch_pass(p, plan.kernel, ntasks, c->stream));
    }
    if (tags) {
        hand_commit(c->hand.tags, plan.hand);
        // MGM_HIP_CHECK_TAGS=1 (debug; synchronises): the invariant the tag protocol rests on, checked after the launch --
        // every word of the slots of this launch's passes (all bands but the last, which hands nothing over) carries the
        // launch's tag.  A slot the kernel skipped would keep its OLD tag and validate a stale slab two launches later.
        if (tune_num("check_tags", 0) != 0) {
            unsigned *flag = ctrl_word(c, kWordFlag), stale = 0;
            HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(unsigned), c->stream));
            for (int v = 0; v < ngroups; v++)
                for (int k = first; k < PEND; k++) {
                    const long long nw = (long long)(p.g[k].nbands - 1) * p.g[k].LL * LPk;
                    if (nw <= 0) continue;
                    HIPCHK(c, launch_check_tags(p.hand + ((long long)v * p.hand_vstride + p.g[k].hand_base) * LPk, nw, c->hand.tags.tag[k], flag, c->stream));
                }
            if ((r = read_word(c, flag, &stale))) return r;
            if (stale != 0) {
                hand_forget(c->hand.tags);
                return fail(c, MGM_ERR_INTERNAL, "hand-off slots: " + std::to_string(stale) + " words do not carry the launch's tag");
            }
        }
    }
    if ((r = watch_launch(c))) return r;
    if (p.tl_on) {
        char head[96], tail[96];
        snprintf(head, sizeof head, "launch %d %d %d %d %d", nx, ny, L, ntasks, p.wg_per_cu);
        snprintf(tail, sizeof tail, "volumes %d fh %d mgm %d strips %d", nb, fh ? 1 : 0, MGM, plan.any_strips);
        if ((r = dump_timeline(c, tl_file, e->buf.p, 8, ntasks, 0, head, tail))) return r;
    }
    if (p.dbg && (r = print_pass_stats(c, p.dbg, (const int2 *)e->buf.p + 8, ntasks, first, PEND))) return r;

    // 7. what the context's last aggregation was: this dense one
    remember_dense(c, Cs, nb, nvol, lr_stride, nslots, Lreal, L, o.cb, (o.padded && o.use_c8) ? pad8 : nullptr, minima, &plan.kernel);
    return MGM_OK;
}

// MGM_HIP_WTA_PRUNE=0 (read at every call: tests switch it inside one process): the plain winner search everywhere
bool wta_prune_enabled()
{
    const char *e = getenv("MGM_HIP_WTA_PRUNE");
    return !(e && atoi(e) == 0) && tune_num("wta_prune", 1) != 0;
}

// The costs a search of C reads: the padded copies of the context's last dense launch if C ran as slot `slot` of it with a padded
// label count (compact, else fp32), else the volume's own compact copy, else its fp32 volume (brought up to date here).
// "Padded" is ONE rule: the caller names a slot, the launch padded, and the volume has the label count of that launch.
// run_wta_right used to ask `Lk > L` alone: its only caller, mgm_wta_right_dev, finds the slot with DenseRun::slot_of and
// refuses a volume whose label count is not the launch's, so both other terms held at every call.
struct CostSource {
    const float *C;
    const uint8_t *C8;
    int cbytes, L;  // bytes per compact cost; label stride of the copy
    bool padded;
};
static int cost_source(mgm_ctx *c, const mgm_cv *C, int slot, CostSource *out)
{
    const DenseRun &d = c->last;
    const int Lreal = C->dmax - C->dmin + 1;
    CostSource s{};
    s.padded = slot >= 0 && d.padded() && d.L == Lreal;
    s.L = s.padded ? d.Lk : Lreal;
    if (s.padded) {
        s.C = d.pad_c8 ? nullptr : (const float *)c->padf[slot].p;
        s.cbytes = d.pad_c8 ? d.pad_cb : 1;
        s.C8 = d.pad_c8 ? d.pad_ptr[slot] : nullptr;
    } else {
        // (two-byte costs: the exact k_wta instances and k_wta_q read them -- label counts of the compact pass kernels)
        s.cbytes = C->cbytes;
        s.C8 = (C->c8_state == CopyState::Valid && c->force_build != 1) ? C->d8 : nullptr;
        if (!s.C8)
            if (int r = ensure_f32(c, C)) return r;
        s.C = C->d;
    }
    *out = s;
    return MGM_OK;
}

// K4-K6 over `npix` pixels starting at pixel `pix0` of C, reading pass p's Lr from lr + p*lr_stride.
// `slot` >= 0: the volume was slot `slot` of the context's last aggregation; if that launch ran with a padded label
// count, its padded cost copies and label stride are used (cost_source).  slot < 0: plain [pix][L] layout.
int run_wta(mgm_ctx *c, const mgm_cv *C, long long pix0, long long npix, const float *lr, long long lr_stride, int NDIR,
            int fix_overcount, int ridx, float *out, float *outcost, float *Sout, const float *wlo, const float *whi, int slot)
{
    const DenseRun &d = c->last;
    // 1. the costs
    CostSource src;
    if (int r = cost_source(c, C, slot, &src)) return r;
    const int L = src.L;

    // 2. the request: the call, what the last dense launch left for it, the switches
    const WtaSwitches &sw = wta_switches();
    WtaRequest q{};
    q.npix = npix;
    q.L = L, q.Lreal = C->dmax - C->dmin + 1, q.NDIR = NDIR, q.lpl = pass_lpl(L);
    q.cbytes = src.cbytes, q.compact = src.C8 ? 1 : 0;
    q.refine = ridx, q.want_S = Sout ? 1 : 0;
    q.window = wlo ? 1 : 0, q.ragged = C->rlo ? 1 : 0;
    q.in_last_run = slot >= 0 ? 1 : 0, q.last_min = (d.wrote_min && c->lmin.p) ? 1 : 0;
    q.lr_is_last = (slot >= 0 && NDIR == d.ndir && lr == d.lr(c->lr, slot, 0) && lr_stride == d.stride) ? 1 : 0;
    q.pix0_zero = pix0 == 0 ? 1 : 0, q.padded = src.padded ? 1 : 0, q.nvol_mod32 = (int)(lr_stride % 32), q.num_cu = c->num_cu;
    q.sw_prune = wta_prune_enabled() ? 1 : 0, q.sw_prune_ppw = sw.prune_ppw, q.sw_prune_wg = sw.prune_wg, q.sw_wg_per_cu = sw.wg_per_cu;
    q.sw_packed = sw.packed, q.sw_wide4 = sw.wide4, q.sw_quad = sw.quad;

    // 3. the plan: family, instance, grid, pruned or not
    const WtaChoice choice = plan_wta(q);

    // 4. the kernel's parameters
    WtaParams w{};
    w.C = src.C ? src.C + pix0 * L : nullptr;
    w.cbytes = src.cbytes;
    w.C8 = src.C8 ? src.C8 + pix0 * L * src.cbytes : nullptr;
    w.Lr = lr;
    w.S = Sout;
    w.out = out;
    w.outcost = outcost;
    w.npix = npix;
    w.nvol = lr_stride;
    w.L = L;
    w.Lreal = q.Lreal;
    w.NDIR = NDIR;
    w.FIX = fix_overcount;
    w.dmin = C->dmin;
    w.refine = ridx;
    // range images are whole-image arrays; this call may cover a slab of rows starting at pix0
    w.wlo = wlo ? wlo + pix0 : nullptr;
    w.whi = whi ? whi + pix0 : nullptr;
    w.clo = C->rlo ? C->rlo + pix0 : nullptr;
    w.chi = C->rhi ? C->rhi + pix0 : nullptr;
    w.num_cu = c->num_cu;

    // 5. the pruned search reads the slot's chunk minima; its two counters (mgm_debug_wta_stats) only while somebody is looking:
    // timing or debug statistics on
    if (choice.prune) {
        w.Lmin = d.lmin(c->lmin, slot, 0);
        if ((c->timing || c->debug_stats) && npix < (1ll << 24)) {
            const bool fresh = c->wta_stats.p == nullptr;
            if (int r = reserve(c, c->wta_stats, kWtaStatBytes)) return r;
            if (fresh || c->wta_stats_n == 0) HIPCHK(c, hipMemsetAsync(c->wta_stats.p, 0, kWtaStatBytes, c->stream));
            w.stats = (unsigned long long *)c->wta_stats.p;
            c->wta_stats_n++;
        }
    }

    // 6. the launch
    TimeScope t(c, "k_wta");
    if (hipError_t e = launch_wta(w, choice, c->stream)) return hipfail(c, e, "launch_wta(w, c->stream)");  // (the message names the call as it always has)
    return MGM_OK;
}

// The right view's winners (vnx x C->ny) out of the Lr volumes of slot `slot` of the context's last dense aggregation
// (mgm_wta_right_dev has checked that C is that volume).  Costs and label stride as run_wta takes them for such a slot.
int run_wta_right(mgm_ctx *c, const mgm_cv *C, int slot, int NDIR, int fix_overcount, int ridx, int vnx, float *out, float *outcost)
{
    const DenseRun &d = c->last;
    CostSource src{};
    src.cbytes = 1;
    if (fix_overcount == 1)  // (else the costs are not read)
        if (int r = cost_source(c, C, slot, &src)) return r;
    WtaRightParams w{};
    w.C = src.C;
    w.C8 = src.C8;
    w.cbytes = src.cbytes;
    w.Lr = d.lr(c->lr, slot, 0);
    w.out = out;
    w.outcost = outcost;
    w.nvol = d.stride;
    w.nx = C->nx;
    w.ny = C->ny;
    w.vnx = vnx;
    w.L = C->dmax - C->dmin + 1;
    w.Lk = d.Lk;
    w.NDIR = NDIR;
    w.FIX = fix_overcount;
    w.dmin = C->dmin;
    w.dmax = C->dmax;
    w.refine = ridx;
    w.num_cu = c->num_cu;
    // MGM_HIP_WTA_RIGHT_ANY=1 (read at every call: tests switch it inside one process): the diagonal walk everywhere
    const char *ea = getenv("MGM_HIP_WTA_RIGHT_ANY");
    const WtaRightChoice choice = plan_wta_right(WtaRightRequest{w.L, w.Lk, w.nx, w.ny, w.vnx, w.dmin, w.dmax, w.num_cu, wta_switches().right_seg, (ea && atoi(ea) != 0) ? 1 : 0});
    TimeScope t(c, "k_wta_right");
    if (hipError_t e = launch_wta_right(w, choice, c->stream)) return hipfail(c, e, "launch_wta_right(w, c->stream)");  // (as above)
    return MGM_OK;
}

// The runner-up search over the Lr volumes of slot `slot` of the context's last dense aggregation
// (mgm_wta_runnerup_dev has checked that C is that volume).  Costs and label stride as run_wta_right takes them.  Reads the
// context's record of that aggregation and leaves it, the chunk minima and the search statistics as they are.
int run_wta_runnerup(mgm_ctx *c, const mgm_cv *C, int slot, int NDIR, int fix_overcount, int radius, float *out2, float *cost2, float *out1,
                     float *cost1)
{
    const DenseRun &d = c->last;
    CostSource src{};
    src.cbytes = 1;
    if (fix_overcount == 1) {  // (else the costs are not read)
        if (int r = cost_source(c, C, slot, &src)) return r;
        if (src.L != d.Lk) return fail(c, MGM_ERR_INTERNAL, "run_wta_runnerup: the costs' label stride is not the last aggregation's");
    }
    WtaRunnerupParams w{};
    w.C = src.C;
    w.C8 = src.C8;
    w.cbytes = src.cbytes;
    w.Lr = d.lr(c->lr, slot, 0);
    w.out2 = out2;
    w.cost2 = cost2;
    w.out1 = out1;
    w.cost1 = cost1;
    w.npix = (long long)C->nx * C->ny;
    w.nvol = d.stride;
    w.L = C->dmax - C->dmin + 1;
    w.Lk = d.Lk;
    w.NDIR = NDIR;
    w.FIX = fix_overcount;
    w.dmin = C->dmin;
    w.radius = std::min(radius, w.L);  // (at L no entry is far enough from any winner: the same result, and o1 + radius stays small)
    // MGM_HIP_WTA_RUNNERUP_ANY=1 (read at every call: tests switch it inside one process): the generic kernel everywhere
    // ... MGM_HIP_WTA_RUNNERUP_WG=<workgroups per CU> (the same): a lower cap of the grid, so that small volumes take several turns
    const char *ea = getenv("MGM_HIP_WTA_RUNNERUP_ANY"), *ew = getenv("MGM_HIP_WTA_RUNNERUP_WG");
    const RunnerupChoice choice = plan_wta_runnerup(RunnerupRequest{w.npix, w.L, w.Lk, NDIR, c->num_cu, (ea && atoi(ea) != 0) ? 1 : 0, ew ? std::max(0, atoi(ew)) : 0});
    TimeScope t(c, "k_wta_runnerup");
    // (a second name with the same time: which family ran -- tests assert that the forcing switch was honoured)
    t.kernel = choice.family == kRunnerupAny ? "k_wta_runnerup_any" : "k_wta_runnerup_stream";
    if (hipError_t e = launch_wta_runnerup(w, choice, c->stream)) return hipfail(c, e, "launch_wta_runnerup(w, c->stream)");
    return MGM_OK;
}

// The consensus votes over the Lr volumes of the context's last aggregation of C, each pass taken alone
// (mgm_wta_consensus_dev has checked that C is such a volume): slot `slot` of the dense run, or with rel = true of the
// range-proportional one.  Reads the context's record of that aggregation and leaves it, the chunk minima and the search
// statistics as they are.  No costs are read.
int run_wta_consensus(mgm_ctx *c, const mgm_cv *C, int slot, bool rel, int NDIR, const float *d, float tol, float *votes, float *winners)
{
    WtaConsensusParams w{};
    w.d = d;
    w.votes = votes;
    w.winners = winners;
    w.npix = (long long)C->nx * C->ny;
    w.NDIR = NDIR;
    w.dmin = C->dmin;
    w.tol = tol;
    if (rel) {
        w.Lr = c->rel_last.lr(c->lr_rel, slot, 0);
        w.nvol = c->rel_last.stride;
        w.rec = C->rel_records();
        w.L = w.Lk = C->rel_slots;
    } else {
        w.Lr = c->last.lr(c->lr, slot, 0);
        w.nvol = c->last.stride;
        w.rlo = C->rlo;  // a ragged volume whose last run was dense: the hull, masked by the pixel's own range
        w.rhi = C->rhi;
        w.L = C->dmax - C->dmin + 1;
        w.Lk = c->last.Lk;
    }
    // MGM_HIP_WTA_CONSENSUS_ANY=1 (read at every call: tests switch it inside one process): the generic kernel everywhere
    // ... MGM_HIP_WTA_CONSENSUS_WG=<workgroups per CU> (the same): a lower cap of the grid, so that small volumes take several turns
    const char *ea = getenv("MGM_HIP_WTA_CONSENSUS_ANY"), *ew = getenv("MGM_HIP_WTA_CONSENSUS_WG");
    const ConsensusChoice choice = plan_wta_consensus(ConsensusRequest{w.npix, w.L, w.Lk, NDIR, c->num_cu, rel ? w.Lk : 0, (ea && atoi(ea) != 0) ? 1 : 0,
                                                                       ew ? std::max(0, atoi(ew)) : 0, (!rel && C->rlo) ? 1 : 0});
    TimeScope t(c, "k_wta_consensus");
    // (a second name with the same time: which family ran -- tests assert the route and that the forcing switch was honoured)
    t.kernel = choice.family == kConsensusAny ? "k_wta_consensus_any" : (choice.family == kConsensusRel ? "k_wta_consensus_rel" : "k_wta_consensus_stream");
    if (hipError_t e = launch_wta_consensus(w, choice, c->stream)) return hipfail(c, e, "launch_wta_consensus(w, c->stream)");
    return MGM_OK;
}

// K4-K6 with any refinement of the reference's table: none/vfit are fused into k_wta; parabola, cubic and
// parabolaOCV (refine.h:6-145) run as a second kernel on the corrected S (the caller's, or a scratch volume).
int run_wta_refine(mgm_ctx *c, const mgm_cv *C, long long pix0, long long npix, const float *lr, long long lr_stride,
                   int NDIR, int fix_overcount, int ridx, float *out, float *outcost, float *Sout,
                   const float *wlo, const float *whi, int slot)
{
    if (!wlo && C->rlo) {  // a ragged volume: S is allocated from the same range images (mgm_core.cc:426)
        wlo = C->rlo;
        whi = C->rhi;
    }
    if (ridx <= 1 && !wlo) return run_wta(c, C, pix0, npix, lr, lr_stride, NDIR, fix_overcount, ridx, out, outcost, Sout, nullptr, nullptr, slot);
    if (ridx == 0) return run_wta(c, C, pix0, npix, lr, lr_stride, NDIR, fix_overcount, 0, out, outcost, Sout, wlo, whi, slot);
    const int L = C->dmax - C->dmin + 1;
    int r;
    if (!Sout) {
        if ((r = reserve(c, c->stmp, sizeof(float) * (size_t)npix * L))) return r;
        Sout = (float *)c->stmp.p;
    }
    if ((r = run_wta(c, C, pix0, npix, lr, lr_stride, NDIR, fix_overcount, 0, out, outcost, Sout, wlo, whi, slot))) return r;
    // what a disparity of a pixel's window outside the volume holds: S stays 0, minus (NDIR-1)*C with C = +INF
    float vout = 0.0f;
    if (fix_overcount == 1) vout = vout - (float)(NDIR - 1) * __builtin_huge_valf();
    TimeScope t(c, "k_refine");
    HIPCHK(c, launch_refine(Sout, npix, L, C->dmin, ridx, wlo ? wlo + pix0 : nullptr, whi ? whi + pix0 : nullptr, vout, out,
                            outcost, c->stream));
    return MGM_OK;
}


// ---- ragged volumes on their range-proportional copies (mgm_pass_rel.hip, k_wta_rel; round 5) -------------------------------
// MGM_HIP_REL=0 (read at every call: tests switch it inside one process): ragged volumes keep the dense-hull kernels
bool rel_enabled()
{
    const char *e = getenv("MGM_HIP_REL");
    return !(e && atoi(e) == 0) && tune_num("rel", 1) != 0;
}

int run_wta_rel(mgm_ctx *c, const mgm_cv *C, int slot, int NDIR, int fix_overcount, int ridx, const float *wlo, const float *whi, float *out,
                float *outcost, float *Sout)
{
    const size_t npix = (size_t)C->nx * C->ny;
    WtaRelParams w{};
    w.c8 = C->relbuf;
    w.base = C->rel_records();
    w.slots = C->rel_slots;
    w.cb = C->rel_cb;
    w.rlo = C->rlo;
    w.rhi = C->rhi;
    w.Lr = c->rel_last.lr(c->lr_rel, slot, 0);
    w.wlo = wlo;
    w.whi = whi;
    w.out = out;
    w.outcost = outcost;
    w.npix = (long long)npix;
    w.nvol = c->rel_last.stride;
    w.NDIR = NDIR;
    w.FIX = fix_overcount;
    w.refine = ridx;
    w.num_cu = c->num_cu;
    {
        TimeScope t(c, "k_wta");
        HIPCHK(c, launch_wta_rel(w, c->stream));
    }
    if (Sout) {  // the caller wants the corrected aggregated volume mgm() returns: on the dense hull
        TimeScope t(c, "k_rel_S");
        HIPCHK(c, launch_rel_S(w, C->dmax - C->dmin + 1, C->dmin, Sout, c->stream));
    }
    return MGM_OK;
}

int run_rel(mgm_ctx *c, const mgm_cv *const *Cs, const mgm_img *const *w8s, int nb, float P1, float P2, int MGM, int use_fh, int NDIR,
            int fix_overcount, int ridx, mgm_img *const *outs, mgm_img *const *outcosts, mgm_cv **S)
{
    const mgm_cv *C = Cs[0];
    const int nx = C->nx, ny = C->ny;
    const long long npix = (long long)nx * ny;
    int r;
    HIPCHK(c, hipSetDevice(c->device));
    if (int r0 = check_watchdog(c, false)) return r0;
    if ((r = ensure_words(c))) return r;

    // 1. the operands (the volumes' copies and the weights' values were resolved by the caller: rel_resolve, weights_have_odd_values)
    const bool fh = use_fh > 0;
    const bool pube = !fh && !(w8s && w8s[0]);  // unit weights, Hirschmueller: the producer publishes E (k_pass_rel, PUBE)
    const int slots = C->rel_slots, rcb = C->rel_cb;  // (every volume of the launch has this format: aggregate_batch_now)
    const bool fh2 = fh && MGM == 2 && !(w8s && w8s[0]);  // update_cost2_trunclinear (the caller passes weights only if some weight != 1)
    bool weighted = false;
    for (int v = 0; v < nb; v++) weighted = weighted || (w8s && w8s[v]);
    if (weighted)
        for (int v = 0; v < nb; v++)
            if (!w8s[v]) return fail(c, MGM_ERR_INVALID, "mgm_aggregate_batch: weights for all volumes or for none");

    // 2. the request
    RelRequest q{};
    q.nx = nx, q.ny = ny, q.NDIR = NDIR, q.nb = nb, q.MGM = MGM, q.fh = fh ? 1 : 0, q.pube = pube ? 1 : 0, q.fh2 = fh2 ? 1 : 0, q.slots = slots, q.cb = rcb;
    q.R = kRelLines, q.HS = rel_hand_floats(fh || pube, slots, fh2);
    q.diag_fits = rel_wg_lds_bytes(fh || pube, slots, rcb, fh2, true) <= kLdsBytes ? 1 : 0;
    q.num_cu = c->num_cu;
    q.rel_wg = (int)tune_num("rel_wg", 0), q.rel_prio = (int)tune_num("rel_prio", nb <= 1 ? 5 : 0), q.rel_lag = (int)tune_num("rel_lag", 0);
    q.rel_lagd = (int)tune_num("rel_lagd", 0), q.rel_slots = (int)tune_num("rel_slots", 100), q.rel_slope1 = (int)tune_num("rel_slope1", 1);
    q.rel_swap = (int)tune_num("rel_swap", 1), q.rel_diag = (int)tune_num("rel_diag", 1), q.rel_strips = (int)tune_num("rel_strips", 1);
    q.rel_multi = tune_num("rel_multi", 1) != 0 ? 1 : 0;

    // 3. the plan: the simulated list schedule of the launch (one ticket counter), the context's if it has launched this request before
    const auto *e = c->rel_plans.find(q);
    if (!e) {
        RelPlan fresh = plan_rel(q);
        if (fresh.err) return plan_error(c, fresh.err, "launch_pass_rel(p, ntasks, fh, pube, rel_wg, c->stream)");
        if ((r = cache_put(c, c->rel_plans, q, fresh, &e))) return r;
    }
    const RelPlan &plan = e->plan;
    const int ntasks = plan.ntasks, rel_wg = plan.rel_wg;
    if (tune_num("show_plan", 0)) {
        char name[96];
        pass_kernel_name(plan.kernel, name, sizeof name);
        fprintf(stderr, "[mgm plan] rel table: %d tasks, fnv1a %016llx, kernel %s\n", ntasks, e->fnv, name);
    }

    // 4. the workspace; the hand-off region, cleared or tagged
    const long long stride = npix * slots + lr_pad_floats();
    if ((r = reserve(c, c->lr_rel, sizeof(float) * (size_t)stride * NDIR * nb))) return r;
    RelParams p{};
    // (every launch runs all NDIR passes of the layout, so their tags stay in lockstep: the kernel takes one)
    HandStep step;
    if ((r = begin_hand(c, c->hand_rel, sizeof(float) * (size_t)nb * plan.hand_vstride * q.HS, plan.hand, 0, NDIR, &step))) return r;
    p.tag = step.tag[0];

    // 5. the kernel's parameters
    for (int v = 0; v < nb; v++) {
        p.vol[v].c8 = Cs[v]->relbuf;
        p.vol[v].base = Cs[v]->rel_records();
        p.vol[v].rlo = Cs[v]->rlo;
        p.vol[v].rhi = Cs[v]->rhi;
        p.vol[v].Lr = (float *)c->lr_rel.p + (size_t)v * NDIR * stride;
        p.vol[v].w8 = weighted ? w8s[v]->d : nullptr;
    }
    for (int k = 0; k < kMaxDirs; k++) p.g[k] = plan.g[k];
    p.hand_vstride = plan.hand_vstride;
    p.diag_any = plan.diag_any;
    p.hand = (float *)c->hand_rel.buf.p;
    p.ticket = ctrl_word(c, kWordTicket);
    p.err = ctrl_word(c, kWordWatchdog);
    p.tasks = (const int2 *)e->buf.p;
    p.npix = npix;
    p.nvol = stride;
    p.MGM = MGM;
    p.NDIR = NDIR;
    p.pass0 = 0;
    p.LLmax = plan.maxLL;
    p.maxbands = kMaxBands;
    p.weighted = weighted ? 1 : 0;
    p.P1 = P1;
    p.P2 = P2;
    // the loader's lead: every step of it is a step of lag per band (round 5: 3 for batches; with the anti-diagonal passes 2 is as good there)
    p.ld = (int)std::min(5LL, std::max(2LL, tune_num("rel_ld", 2)));  // (2 against 3: x 2 7.76 / 7.81 ms, x 4 12.30 / 12.39)
    p.fh_multi = q.rel_multi;
    p.cost2 = (pube && MGM == 2) ? 1 : 0;
    p.fh2 = fh2 ? 1 : 0;
    p.slots = slots;
    p.cb = rcb;
    p.tl = nullptr;
    // MGM_HIP_TIMELINE=<file>: one line per work item (tools/timeline.py) -- where the compute units' time goes
    const char *tl_file = getenv("MGM_HIP_TIMELINE");
    const int nph = pass_rel_phases();
    if (tl_file && *tl_file) {
        if ((r = reserve(c, c->dbg, sizeof(unsigned long long) * (8 + nph) * (size_t)ntasks))) return r;
        HIPCHK(c, hipMemsetAsync(c->dbg.p, 0, sizeof(unsigned long long) * (8 + nph) * (size_t)ntasks, c->stream));
        p.tl = (unsigned long long *)c->dbg.p;
    }
    HIPCHK(c, hipMemsetAsync(p.ticket, 0, sizeof(unsigned), c->stream));

    // 6. the launch
    {
        TimeScope t(c, "k_pass_rel");
        HIPCHK(c, launch_pass_rel(p, plan.kernel, ntasks, c->stream));
    }
    hand_commit(c->hand_rel.tags, plan.hand);
    if ((r = watch_launch(c))) return r;
    if (p.tl) {
        char head[96], tail[96];
        snprintf(head, sizeof head, "launch %d %d %d %d %d", nx, ny, 64, ntasks, rel_wg);
        snprintf(tail, sizeof tail, "volumes %d fh %d mgm %d rel 1", nb, fh ? 1 : 0, MGM);
        if ((r = dump_timeline(c, tl_file, e->buf.p, 0, ntasks, nph, head, tail))) return r;
    }

    // 7. what the context's last aggregation was: this one; and the winner search on it
    remember_rel(c, Cs, nb, NDIR, stride, plan.kernel);
    for (int v = 0; v < nb; v++) {
        float *Sout = nullptr;
        if (S) {
            if ((r = mgm_cv_create(c, nx, ny, Cs[v]->dmin, Cs[v]->dmax, &S[v]))) return r;
            Sout = S[v]->d;
        }
        if ((r = run_wta_rel(c, Cs[v], v, NDIR, fix_overcount, ridx, nullptr, nullptr, outs[v]->d, outcosts[v]->d, Sout))) return r;
    }
    return MGM_OK;
}
