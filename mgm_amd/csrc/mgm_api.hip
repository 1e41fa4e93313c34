// mgm_api.hip -- the C ABI of libmgm_hip.so (include/mgm_hip.h), compute side: edge weights, the aggregation calls (immediate,
// batched, deferred), the direction-sharding building blocks and the steps main() applies around the path.  Contexts and
// images: mgm_ctx.hip; cost volumes: mgm_volume.hip; the launch plan: mgm_plan.hip.  No compute happens on the host and there
// is no CPU fallback.
#include "mgm_host.h"

extern "C" {

// ---- weights ------------------------------------------------------------------
int mgm_weights_dev(mgm_ctx *c, const mgm_img *u, float aP, float aThresh, mgm_img **w8)
{
    if (!c || !u || !w8) return fail(c, MGM_ERR_INVALID, "mgm_weights: null argument");
    const bool provided = *w8 != nullptr;  // (a caller that computes weights pair after pair refills its image)
    int r = MGM_OK;
    if (provided) {
        if ((*w8)->nx != u->nx || (*w8)->ny != u->ny || (*w8)->nch != 8)
            return fail(c, MGM_ERR_INVALID, "mgm_weights: *w8 is non-NULL but is not an nx*ny*8 image");
        if (pipe_uses(c, *w8))  // (pipelined context: a deferred aggregation still wants the weights it holds now)
            if ((r = pipe_flush(c))) return r;
    } else if ((r = mgm_img_create(c, u->nx, u->ny, 8, w8)))
        return r;
    HIPCHK(c, hipSetDevice(c->device));
    TimeScope t(c, "k_weights");
    const hipError_t e = launch_weights(u->d, u->nx, u->ny, u->nch, aP, aThresh, (*w8)->d, c->stream);
    if (e != hipSuccess) {
        r = hipfail(c, e, "k_weights");
        if (!provided) {
            mgm_img_free(c, *w8);
            *w8 = nullptr;
        }
        return r;
    }
    return MGM_OK;
}


static int check_aggregate_args(mgm_ctx *c, int n, const mgm_cv *const *C, const mgm_img *const *w8, int NDIR, int MGM, mgm_img *const *out,
                                mgm_img *const *outcost)
{
    if (!c || !C || !out || !outcost || n < 1) return fail(c, MGM_ERR_INVALID, "mgm_aggregate: null argument");
    if (n > kMaxBatch) return fail(c, MGM_ERR_INVALID, "mgm_aggregate_batch: at most 16 volumes per call");
    if (NDIR < 1 || NDIR > kMaxDirs)  // the reference reads past its 8-entry table for -O 16 (mgm_core.cc:489)
        return fail(c, MGM_ERR_INVALID, "NDIR must be 1..8");
    if (MGM < 1 || MGM > 4) return fail(c, MGM_ERR_INVALID, "MGM (TSGM) must be 1..4");
    for (int v = 0; v < n; v++)
        if (!C[v] || !out[v] || !outcost[v]) return fail(c, MGM_ERR_INVALID, "mgm_aggregate: null argument");
    for (int v = 0; v < n; v++)
        if (C[v]->unfilled) return fail(c, MGM_ERR_INVALID, "mgm_aggregate: the last mgm_costvolume_build of this volume failed; it holds no costs");
    const int nx = C[0]->nx, ny = C[0]->ny, L = C[0]->dmax - C[0]->dmin + 1;
    for (int v = 0; v < n; v++) {
        if (C[v]->nx != nx || C[v]->ny != ny || C[v]->dmax - C[v]->dmin + 1 != L)
            return fail(c, MGM_ERR_INVALID, "mgm_aggregate_batch: the volumes must have the same size and label count");
        if (out[v]->nx != nx || out[v]->ny != ny || outcost[v]->nx != nx || outcost[v]->ny != ny)
            return fail(c, MGM_ERR_INVALID, "mgm_aggregate: output image size mismatch");
        if (w8 && w8[v] && (w8[v]->nx != nx || w8[v]->ny != ny || w8[v]->nch != 8))
            return fail(c, MGM_ERR_INVALID, "mgm_aggregate: weights must be nx*ny*8");
        if (w8 && (w8[v] == nullptr) != (w8[0] == nullptr))
            return fail(c, MGM_ERR_INVALID, "mgm_aggregate_batch: weights for all volumes or for none");
    }
    return MGM_OK;
}

// mgm_ctx_set_placement_tries: the Lr workspace has just been (re)allocated by `launch` -- time that very launch on a few physical
// placements and keep the fastest (the launch is idempotent: same inputs, same Lr volumes, whichever allocation).  `r`: the
// launch's result; returns what the last launch on the kept workspace gave.  *stop: an error ends the call here (no halving).
static int place_workspace(mgm_ctx *c, int r, const std::function<int()> &launch, bool *stop)
{
    *stop = false;
    if (!(r == MGM_OK && c->place_tries >= 2 && c->lr.p && (c->lr.p != c->placed_ptr || c->lr.cap != c->placed_cap) && c->lr.cap >= (1ull << 28))) return r;
    *stop = true;
    auto timed = [&](float *ms) -> int {
        struct Ev {  // (destroyed on every exit path)
            hipEvent_t e = nullptr;
            ~Ev() { if (e) (void)hipEventDestroy(e); }
        } a, b;
        HIPCHK(c, hipEventCreate(&a.e));
        HIPCHK(c, hipEventCreate(&b.e));
        HIPCHK(c, hipEventRecord(a.e, c->stream));
        int rr = launch();
        if (rr == MGM_OK) {
            HIPCHK(c, hipEventRecord(b.e, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipEventElapsedTime(ms, a.e, b.e));
        }
        return rr;
    };
    float best = 0;
    if ((r = timed(&best))) return r;  // (the first run, the caller's, was the warm-up)
    struct Held {  // the allocations that are only held so that the next try lands elsewhere: freed on every exit path
        std::vector<Buf> v;
        void release() { for (Buf &h : v) if (h.p) (void)hipFree(h.p); v.clear(); }
        ~Held() { release(); }
        void push_back(const Buf &b) { v.push_back(b); }
    } held;
    for (int t = 1; t < c->place_tries && r == MGM_OK; t++) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || fr < c->lr.cap + (1ull << 30)) break;  // no room for a second workspace
        Buf old = c->lr;
        c->lr = Buf{};
        float ms = 0;
        int rr = launch();  // allocates; warm-up
        if (rr == MGM_OK) rr = timed(&ms);
        if (rr != MGM_OK) {  // (out of memory after all: back to what we had)
            if (c->lr.p) (void)hipFree(c->lr.p);
            c->lr = old;
            (void)hipGetLastError();
            c->err.clear();
            r = launch();
            break;
        }
        if (tune_num("show_plan", 0)) fprintf(stderr, "[mgm place] try %d: %.3f ms (best so far %.3f)\n", t, ms, best);
        if (ms < best * 0.985f) {  // the new placement is the faster one: the old allocation is only held (so that the next try lands elsewhere)
            held.push_back(old);
            best = ms;
        } else {  // keep the old one: hold the new one instead, and run the launch on the old workspace again (its Lr volumes are what k_wta reads)
            held.push_back(c->lr);
            c->lr = old;
            r = launch();
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    held.release();
    c->placed_ptr = c->lr.p;
    c->placed_cap = c->lr.cap;
    *stop = false;
    return r;
}

// Range-proportional kernels or dense hull: plan_agg_route (mgm_planner.h) asks for the facts it needs, one at a time.
static int resolve_route(mgm_ctx *c, int n, const mgm_cv *const *C, const mgm_img *const *w8, float P1, float P2, int MGM, int use_fh, bool want_S,
                         RouteDecision *out)
{
    RouteRequest q{};
    q.n = n, q.MGM = MGM, q.fh = use_fh > 0, q.want_S = want_S, q.weights_given = w8 && w8[0];
    q.p1_nonneg = P1 >= 0.0f, q.p2_nonneg = P2 >= 0.0f, q.p2_finite = P2 < __builtin_huge_valf();
    q.only_rel = 1;
    for (int v = 0; v < n; v++) q.only_rel = q.only_rel && C[v]->rel_only;
    q.rel_enabled = rel_enabled(), q.sw_rel = (int)tune_num("rel", 1), q.sw_rel_tie = (int)tune_num("rel_tie", 1);
    q.sw_rel_S = (int)tune_num("rel_S", 1), q.sw_rel_fh2 = (int)tune_num("rel_fh2", 1);
    q.w_odd = q.w_any = -1;
    for (int v = 0; v < kMaxBatch; v++) q.rel_usable[v] = q.rel_slots[v] = q.rel_cb[v] = -1;
    for (;;) {
        const RouteDecision d = *out = plan_agg_route(q);
        if (d.need == kNeedNothing) return MGM_OK;
        int r;
        bool odd = false, any = false, u = false;
        if (d.need == kNeedWeightValues) {
            if ((r = weights_have_odd_values(c, w8, n, (long long)C[0]->nx * C[0]->ny, &odd, &any))) return r;
            q.w_odd = odd, q.w_any = any;
        } else {  // kNeedRelCopy
            if ((r = rel_resolve(c, C[d.arg], &u))) return r;
            q.rel_usable[d.arg] = u, q.rel_slots[d.arg] = C[d.arg]->rel_slots, q.rel_cb[d.arg] = C[d.arg]->rel_cb;
        }
    }
}

// The aggregation itself, now: one pass launch over the batch (several if it does not fit), then the winner search per volume.
static int aggregate_batch_now(mgm_ctx *c, int n, const mgm_cv *const *C, const mgm_img *const *w8, float P1, float P2, int NDIR,
                               int MGM, int use_fh, int fix_overcount, const char *refine, mgm_img *const *out,
                               mgm_img *const *outcost, mgm_cv **S)
{
    const int nx = C[0]->nx, ny = C[0]->ny, L = C[0]->dmax - C[0]->dmin + 1;
    const int ridx = refinement_index(refine);
    HIPCHK(c, hipSetDevice(c->device));
    int r = MGM_OK;
    const long long npix = (long long)nx * ny;
    if (S)
        for (int v = 0; v < n; v++) S[v] = nullptr;
    c->wta_stats_n = 0;  // (mgm_debug_wta_stats: the pruned searches of THIS call)
    // Ragged volumes whose range-proportional copies are usable take the kernels that walk the pixels' own windows
    // (mgm_pass_rel.hip): not with P2 = +INF (all-INF slabs: the operand-order-faithful kernel), negative penalties or odd weights
    // (plan_agg_route, mgm_planner.h).
    // Measured (round 5, 1920x1080, windows of 49 labels in a hull of 256, K3 + search): FH 21.3 + 3.9 ms on the hull (the general
    // weighted kernels: the min-convolution runs over the RECEIVING pixel's range) -> 14.0 + 1.5 ms; free-form weights,
    // Hirschmueller: 11.4 + 3.9 -> 7.1 + 1.5; unit weights, Hirschmueller: 4.75 + 3.9 on the hull's queue kernels against
    // 7.1 + 1.5 + 0.45 (gather) -- a tie then; round 6 (slope 1, two strips): 5.3 + 3.7 ms against 5.6 + 0.8, the gather paid either
    // way: every usable copy is walked.  Census volumes whose ONLY copy is the range-proportional one would first have to be expanded
    // and encoded again for the hull, 2.2 ms.
    RouteDecision route;
    if ((r = resolve_route(c, n, C, w8, P1, P2, MGM, use_fh, S != nullptr, &route))) return r;
    const bool rel = route.route == kRouteRel;
    // what the winner search behind a dense launch will be: run_passes decides with it whether the launch writes the chunk minima
    // the pruned search reads (mgm_planner.h, plan_wta_prune)
    const bool search_S = S != nullptr;
    // the passes of the volumes [v0, v0 + m) -- and, on the range-proportional route, their winner search
    auto launch = [&](int v0, int m) -> int {
        if (rel) return run_rel(c, C + v0, route.rel_weighted ? w8 + v0 : nullptr, m, P1, P2, MGM, use_fh, NDIR, fix_overcount, ridx, out + v0, outcost + v0, S ? S + v0 : nullptr);
        return run_passes(c, C + v0, (w8 && w8[0]) ? w8 + v0 : nullptr, m, P1, P2, MGM, use_fh, 0, NDIR, /*allow_pad=*/true, 0, 0, 0, ridx, search_S);
    };
    // The sub-batches (plan_subbatch): what fits the workspace limit, halved when the device cannot hold it either -- same results,
    // the later volumes just wait their turn.
    SubbatchRequest sq{};
    sq.npix = npix, sq.ws_limit = (long long)c->ws_limit, sq.lr_pad = lr_pad_floats(), sq.route = route.route, sq.n = n, sq.NDIR = NDIR, sq.L = L;
    sq.rel_slots = C[0]->rel_slots, sq.want_S = S != nullptr, sq.refine = ridx, sq.prune_enabled = wta_prune_enabled();
    int chunk = plan_subbatch(sq);
    for (int v0 = 0; v0 < n && !r;) {
        const int m = std::min(chunk, n - v0);
        r = launch(v0, m);
        if (!rel) {
            bool stop = false;
            r = place_workspace(c, r, [&] { return launch(v0, m); }, &stop);
            if (stop) break;
        }
        if (r == MGM_ERR_NOMEM && m > 1) {  // does not fit the device either: halve and try again
            chunk = shrink_after_nomem(route.route, m);
            if (rel) {
                (void)hipGetLastError();
                c->err.clear();
            }
            r = MGM_OK;
            continue;
        }
        for (int v = 0; v < m && !r && !rel; v++) {  // (the dense route's search; run_rel has done its own)
            float *Sout = nullptr;
            if (S) {
                if ((r = mgm_cv_create(c, nx, ny, C[v0 + v]->dmin, C[v0 + v]->dmax, &S[v0 + v]))) break;
                Sout = S[v0 + v]->d;
            }
            r = run_wta_refine(c, C[v0 + v], 0, npix, c->last.lr(c->lr, v, 0), c->last.stride, NDIR, fix_overcount, ridx, out[v0 + v]->d, outcost[v0 + v]->d,
                               Sout, nullptr, nullptr, v);
        }
        v0 += m;
    }
    if (r && S && !rel) {  // no S volume of a failed dense call is handed out (run_rel leaves what it made)
        const std::string msg = c->err;
        for (int v = 0; v < n; v++) {
            if (S[v]) mgm_cv_free(c, S[v]);
            S[v] = nullptr;
        }
        c->err = msg;
    }
    return r;
}

// Pipelined context: everything that has been deferred, as ONE batch (the calls were checked to fit together when they
// were queued).  An error is the error of the call that made the flush happen.
extern "C++" int pipe_flush(mgm_ctx *c)
{
    if (c->pend.empty()) return MGM_OK;
    std::vector<mgm_ctx::PendingAgg> q;
    q.swap(c->pend);  // (nothing below may see them as pending any more)
    std::vector<const mgm_cv *> Cs;
    std::vector<const mgm_img *> Ws;
    std::vector<mgm_img *> Os, Ks;
    for (const auto &a : q) {
        Cs.insert(Cs.end(), a.C.begin(), a.C.end());
        Ws.insert(Ws.end(), a.w8.begin(), a.w8.end());
        Os.insert(Os.end(), a.out.begin(), a.out.end());
        Ks.insert(Ks.end(), a.outcost.begin(), a.outcost.end());
    }
    const auto &a = q[0];
    int r = aggregate_batch_now(c, (int)Cs.size(), Cs.data(), Ws.empty() ? nullptr : Ws.data(), a.P1, a.P2, a.NDIR, a.MGM, a.use_fh,
                                a.fix_overcount, a.has_refine ? a.refine.c_str() : nullptr, Os.data(), Ks.data(), nullptr);
    if (r == MGM_ERR_UNSUPPORTED && q.size() > 1) {
        // Calls that each are fine may not go into ONE launch (e.g. weight planes that are all ones beside real ones: "all
        // weighted or all unweighted" is decided on the values): run them as the caller issued them.
        r = MGM_OK;
        for (const auto &b : q) {
            const int rb = aggregate_batch_now(c, (int)b.C.size(), b.C.data(), b.w8.empty() ? nullptr : b.w8.data(), b.P1, b.P2, b.NDIR,
                                               b.MGM, b.use_fh, b.fix_overcount, b.has_refine ? b.refine.c_str() : nullptr,
                                               const_cast<mgm_img **>(b.out.data()), const_cast<mgm_img **>(b.outcost.data()), nullptr);
            if (rb != MGM_OK && r == MGM_OK) r = rb;
        }
    }
    return r;
}

int mgm_aggregate_batch_dev(mgm_ctx *c, int n, const mgm_cv *const *C, const mgm_img *const *w8, float P1, float P2, int NDIR,
                            int MGM, int use_fh, int fix_overcount, const char *refine, mgm_img *const *out,
                            mgm_img *const *outcost, mgm_cv **S)
{
    if (int r = check_aggregate_args(c, n, C, w8, NDIR, MGM, out, outcost)) return r;
    if (c->pipe_depth < 2) return aggregate_batch_now(c, n, C, w8, P1, P2, NDIR, MGM, use_fh, fix_overcount, refine, out, outcost, S);
    // Pipelined context (mgm_ctx_set_pipeline): the call is DEFERRED -- remembered, not run -- until `depth` calls have been
    // gathered, and those then run as one batch: ONE launch of the pass kernel over all their volumes, where the chains of
    // bands of one volume fill the gaps of the others'.  A call that does not fit what is waiting (other geometry or
    // settings, weighted against unweighted, S wanted, an operand that a waiting call already uses as an output, more than
    // 16 volumes together) makes the waiting ones run first.
    const bool weighted_call = w8 && w8[0];
    bool fits = !S;
    int waiting = 0;
    if (!c->pend.empty()) {
        const auto &a = c->pend[0];
        for (const auto &q : c->pend) waiting += (int)q.C.size();
        const mgm_cv *A = a.C[0];
        fits = fits && A->nx == C[0]->nx && A->ny == C[0]->ny && A->dmax - A->dmin == C[0]->dmax - C[0]->dmin && a.P1 == P1 && a.P2 == P2 &&
               a.NDIR == NDIR && a.MGM == MGM && a.use_fh == use_fh && a.fix_overcount == fix_overcount && a.has_refine == (refine != nullptr) &&
               (!refine || a.refine == refine) && !a.w8.empty() == weighted_call && waiting + n <= kMaxBatch;
        for (int v = 0; v < n && fits; v++) fits = !pipe_uses(c, out[v]) && !pipe_uses(c, outcost[v]);
    }
    for (int v = 0; v < n && fits; v++)  // (within the call: an image cannot be two outputs)
        for (int u = 0; u < n; u++) fits = fits && out[v] != outcost[u] && (u == v || (out[v] != out[u] && outcost[v] != outcost[u]));
    if (!fits) {
        if (int r = pipe_flush(c)) return r;
        if (S) return aggregate_batch_now(c, n, C, w8, P1, P2, NDIR, MGM, use_fh, fix_overcount, refine, out, outcost, S);
    }
    mgm_ctx::PendingAgg a;
    a.C.assign(C, C + n);
    if (weighted_call) a.w8.assign(w8, w8 + n);
    a.out.assign(out, out + n);
    a.outcost.assign(outcost, outcost + n);
    a.P1 = P1, a.P2 = P2, a.NDIR = NDIR, a.MGM = MGM, a.use_fh = use_fh, a.fix_overcount = fix_overcount;
    a.has_refine = refine != nullptr;
    a.refine = refine ? refine : "";
    c->pend.push_back(std::move(a));
    if ((int)c->pend.size() >= c->pipe_depth) return pipe_flush(c);
    return MGM_OK;
}

int mgm_aggregate_dev(mgm_ctx *c, const mgm_cv *C, const mgm_img *w8, float P1, float P2, int NDIR, int MGM, int use_fh,
                      int fix_overcount, const char *refine, mgm_img *out, mgm_img *outcost, mgm_cv **S)
{
    return mgm_aggregate_batch_dev(c, 1, &C, w8 ? &w8 : nullptr, P1, P2, NDIR, MGM, use_fh, fix_overcount, refine, &out,
                                   &outcost, S);
}

// ---- direction sharding (multi-GPU): run a subset of the passes, sum slabs of Lr volumes ----------
int mgm_aggregate_passes_dev(mgm_ctx *c, const mgm_cv *C, const mgm_img *w8, float P1, float P2, int MGM, int use_fh,
                             int first_pass, int n_passes)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !C) return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes: null argument");
    if (C->unfilled) return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes: the last mgm_costvolume_build of this volume failed; it holds no costs");
    if (first_pass < 0 || n_passes < 1 || first_pass + n_passes > kMaxDirs)
        return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes: passes must lie in 0..7");
    if (MGM < 1 || MGM > 4) return fail(c, MGM_ERR_INVALID, "MGM (TSGM) must be 1..4");
    if (w8 && (w8->nx != C->nx || w8->ny != C->ny || w8->nch != 8))
        return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes: weights must be nx*ny*8");
    HIPCHK(c, hipSetDevice(c->device));
    return run_passes(c, &C, w8 ? &w8 : nullptr, 1, P1, P2, MGM, use_fh, first_pass, n_passes);
}

// The same with the caller saying where the Lr volumes go: pass p lands in workspace slot slot0 + (p - first_pass) of
// n_slots, and the context lays its hand-off region out for the passes [0, NDIR_total).  A caller that launches the
// passes of one volume one at a time (to send pass k's slabs while pass k+1 runs) keeps all of them this way.
int mgm_aggregate_passes_at_dev(mgm_ctx *c, const mgm_cv *C, const mgm_img *w8, float P1, float P2, int MGM, int use_fh,
                                int first_pass, int n_passes, int slot0, int n_slots, int NDIR_total)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !C) return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes_at: null argument");
    if (C->unfilled) return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes: the last mgm_costvolume_build of this volume failed; it holds no costs");
    if (first_pass < 0 || n_passes < 1 || first_pass + n_passes > kMaxDirs || NDIR_total > kMaxDirs)
        return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes_at: passes must lie in 0..7");
    if (slot0 < 0 || n_slots < slot0 + n_passes || n_slots > kMaxDirs)
        return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes_at: the passes do not fit the slots");
    if (MGM < 1 || MGM > 4) return fail(c, MGM_ERR_INVALID, "MGM (TSGM) must be 1..4");
    if (w8 && (w8->nx != C->nx || w8->ny != C->ny || w8->nch != 8))
        return fail(c, MGM_ERR_INVALID, "mgm_aggregate_passes_at: weights must be nx*ny*8");
    HIPCHK(c, hipSetDevice(c->device));
    return run_passes(c, &C, w8 ? &w8 : nullptr, 1, P1, P2, MGM, use_fh, first_pass, n_passes, false, slot0, n_slots, NDIR_total);
}

void *mgm_lr_device_ptr(mgm_ctx *c, int slot)
{
    (void)pipe_join(c);
    if (!c || !c->lr.p || slot < 0 || slot >= c->last.ndir || c->last.Lk != c->last.L) return nullptr;
    return const_cast<float *>(c->last.lr(c->lr, 0, slot));  // (the volumes of a single-volume launch: its passes)
}

int mgm_wta_rows_dev(mgm_ctx *c, const mgm_cv *C, int row0, int nrows, const void *lr_slabs, int NDIR, int fix_overcount,
                     const char *refine, void *out_rows, void *outcost_rows)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !C || !lr_slabs || !out_rows || !outcost_rows) return fail(c, MGM_ERR_INVALID, "mgm_wta_rows: null argument");
    if (row0 < 0 || nrows < 1 || row0 + nrows > C->ny || NDIR < 1 || NDIR > kMaxDirs)
        return fail(c, MGM_ERR_INVALID, "mgm_wta_rows: bad row range or NDIR");
    const int ridx = refinement_index(refine);
    HIPCHK(c, hipSetDevice(c->device));
    const long long L = C->dmax - C->dmin + 1, slab = (long long)nrows * C->nx * L;
    return run_wta_refine(c, C, (long long)row0 * C->nx, (long long)nrows * C->nx, (const float *)lr_slabs, slab, NDIR,
                   fix_overcount, ridx, (float *)out_rows, (float *)outcost_rows, nullptr);
}

int mgm_aggregate(mgm_ctx *c, const mgm_cv *C, const float *w8, float P1, float P2, int NDIR, int MGM, int use_fh,
                  int fix_overcount, const char *refine, float *out, float *outcost, mgm_cv **S)
{
    if (!c || !C || !out || !outcost) return fail(c, MGM_ERR_INVALID, "mgm_aggregate: null argument");
    mgm_img *dw = nullptr, *dout = nullptr, *dcost = nullptr;
    int r = MGM_OK;
    if (w8) r = mgm_img_upload(c, w8, C->nx, C->ny, 8, &dw);
    if (!r) r = mgm_img_create(c, C->nx, C->ny, 1, &dout);
    if (!r) r = mgm_img_create(c, C->nx, C->ny, 1, &dcost);
    if (!r) r = mgm_aggregate_dev(c, C, dw, P1, P2, NDIR, MGM, use_fh, fix_overcount, refine, dout, dcost, S);
    if (!r) r = mgm_img_download(c, dout, out);
    if (!r) r = mgm_img_download(c, dcost, outcost);
    mgm_img_free(c, dw);
    mgm_img_free(c, dout);
    mgm_img_free(c, dcost);
    return r;
}

int mgm_debug_download_lr(mgm_ctx *c, int pass, float *dense)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (c && dense && c->rel_last.batch > 0 && c->last.ndir == 0 && c->rel_last.cvs[0] && c->lr_rel.p) {
        // the last aggregation ran on the range-proportional copy (k_pass_rel): volume 0's pass, expanded on the host to the dense
        // hull -- label o <-> slot o + dmin - base(p) of the pixel's 64, +INF where the pixel has no such label (test aid only)
        if (pass < 0 || pass >= c->rel_last.ndir) return fail(c, MGM_ERR_INVALID, "mgm_debug_download_lr: no such pass");
        const mgm_cv *C = c->rel_last.cvs[0];
        // (a volume refilled since -- another slot count, other records -- no longer describes the Lr volumes of that launch)
        if (c->rel_last.slot_of(C) != 0 || C->rel_slots != c->rel_last.slots)
            return fail(c, MGM_ERR_INVALID, "mgm_debug_download_lr: the volume of the last aggregation has been refilled since");
        const size_t npix = (size_t)C->nx * C->ny;
        const int L = C->dmax - C->dmin + 1;
        HIPCHK(c, hipSetDevice(c->device));
        const size_t slots = (size_t)C->rel_slots;
        std::vector<float> slabs(npix * slots);
        std::vector<int> rec(npix * 4);
        HIPCHK(c, hipMemcpyAsync(slabs.data(), c->rel_last.lr(c->lr_rel, 0, pass), sizeof(float) * npix * slots,
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(rec.data(), C->rel_records(), sizeof(int) * npix * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t p = 0; p < npix; p++) {
            const int b = rec[p * 4], lo = rec[p * 4 + 1], hi = rec[p * 4 + 2];
            for (int o = 0; o < L; o++) {
                const int d = C->dmin + o;
                dense[p * L + o] = (d >= lo && d <= hi) ? slabs[p * slots + (d - b)] : __builtin_huge_valf();
            }
        }
        return MGM_OK;
    }
    if (!c || !dense || pass < 0 || pass >= c->last.ndir || !c->lr.p)
        return fail(c, MGM_ERR_INVALID, "mgm_debug_download_lr: nothing to download");
    HIPCHK(c, hipSetDevice(c->device));
    // (a launch with a padded label count keeps Lk floats per pixel, of which the first L exist)
    const DenseRun &d = c->last;
    HIPCHK(c, hipMemcpy2DAsync(dense, sizeof(float) * d.L, d.lr(c->lr, 0, pass), sizeof(float) * d.Lk, sizeof(float) * d.L, (size_t)(d.nvol / d.Lk),
                               hipMemcpyDeviceToHost, c->stream));
    return mgm_ctx_synchronize(c);
}

// Test aid: where volume 0's Lr volume of pass `pass` of the last range-proportional run lies, [npix][slots] floats, with the format
// it was written in -- refused exactly where the range-proportional branch of mgm_debug_download_lr refuses.
void *mgm_debug_rel_lr_device_ptr(mgm_ctx *c, int pass, int *slots, int *cb, long long *pass_stride, void **records)
{
    if (pipe_join(c)) return nullptr;
    if (!c || !(c->rel_last.batch > 0 && c->last.ndir == 0 && c->rel_last.cvs[0] && c->lr_rel.p)) return nullptr;  // no such run
    if (pass < 0 || pass >= c->rel_last.ndir) return nullptr;
    const mgm_cv *C = c->rel_last.cvs[0];
    if (c->rel_last.slot_of(C) != 0 || C->rel_slots != c->rel_last.slots || !C->relbuf) return nullptr;  // refilled since
    if (slots) *slots = C->rel_slots;
    if (cb) *cb = C->rel_cb;
    if (pass_stride) *pass_stride = c->rel_last.stride;
    if (records) *records = C->rel_records();
    return const_cast<float *>(c->rel_last.lr(c->lr_rel, 0, pass));
}

// Test aid: where pass `pass` of volume `volume` of the last DENSE run lies, [npix][*Lk] floats of which the first L of a pixel are
// labels -- whatever the label stride (mgm_lr_device_ptr refuses a padded one and serves volume 0 only).  Launches nothing.
void *mgm_debug_lr_device_ptr(mgm_ctx *c, int volume, int pass, int *Lk, long long *pass_stride)
{
    if (pipe_join(c)) return nullptr;
    if (!c || !c->lr.p || c->last.ndir < 1 || c->last.batch < 1) return nullptr;  // no such run
    if (volume < 0 || volume >= c->last.batch || pass < 0 || pass >= c->last.ndir) return nullptr;
    if (Lk) *Lk = c->last.Lk;
    if (pass_stride) *pass_stride = c->last.stride;
    return const_cast<float *>(c->last.lr(c->lr, volume, pass));
}

// Test aid: the un-windowed search (and k_rel_S) of run_rel's step 7 again, on the Lr volumes as they lie in the workspace.
int mgm_debug_wta_rel_again_dev(mgm_ctx *c, const mgm_cv *C, int NDIR, int fix_overcount, const char *refine, mgm_img *out, mgm_img *outcost,
                                mgm_cv **S)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (S) *S = nullptr;
    if (!c || !C || !out || !outcost) return fail(c, MGM_ERR_INVALID, "mgm_debug_wta_rel_again: null argument");
    for (const mgm_img *im : {(const mgm_img *)out, (const mgm_img *)outcost})
        if (im->nx != C->nx || im->ny != C->ny || im->nch != 1) return fail(c, MGM_ERR_INVALID, "mgm_debug_wta_rel_again: image size mismatch");
    const int v = c->rel_last.slot_of(C);
    if (v < 0 || c->rel_last.ndir != NDIR || c->last.ndir != 0 || !c->lr_rel.p || !C->relbuf)
        return fail(c, MGM_ERR_INVALID, "mgm_debug_wta_rel_again: this volume was not part of the context's last range-proportional aggregation with NDIR passes");
    HIPCHK(c, hipSetDevice(c->device));
    float *Sout = nullptr;
    if (S) {
        if (int r = mgm_cv_create(c, C->nx, C->ny, C->dmin, C->dmax, S)) return r;
        Sout = (*S)->d;
    }
    const int r = run_wta_rel(c, C, v, NDIR, fix_overcount, refinement_index(refine), nullptr, nullptr, out->d, outcost->d, Sout);
    if (r && S) {  // no S volume of a failed call is handed out
        const std::string msg = c->err;
        mgm_cv_free(c, *S);
        *S = nullptr;
        c->err = msg;
    }
    return r;
}

int mgm_debug_download_lmin(mgm_ctx *c, int slot, int pass, float *out)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !out) return fail(c, MGM_ERR_INVALID, "mgm_debug_download_lmin: null argument");
    const DenseRun &d = c->last;
    if (!d.wrote_min || !c->lmin.p || !c->lr.p || d.stride % kChunkLabels != 0)
        return fail(c, MGM_ERR_INVALID, "mgm_debug_download_lmin: the context's last aggregation wrote no chunk minima");
    if (slot < 0 || slot >= d.batch || pass < 0 || pass >= d.ndir)
        return fail(c, MGM_ERR_INVALID, "mgm_debug_download_lmin: no such slot or pass");
    if (!d.current(slot))
        return fail(c, MGM_ERR_INVALID, "mgm_debug_download_lmin: the volume of the last aggregation has been refilled since");
    HIPCHK(c, hipSetDevice(c->device));
    // where the search finds them (run_wta): slot k's passes behind each other, one word per 32 floats of the Lr workspace
    const size_t nchunk = (size_t)(d.nvol / kChunkLabels);  // (pixels x L / 32)
    HIPCHK(c, hipMemcpyAsync(out, d.lmin(c->lmin, slot, pass), sizeof(float) * nchunk, hipMemcpyDeviceToHost, c->stream));
    return mgm_ctx_synchronize(c);
}

int mgm_debug_wta_stats(mgm_ctx *c, unsigned long long *pixels, unsigned long long *chunks)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !pixels || !chunks) return fail(c, MGM_ERR_INVALID, "mgm_debug_wta_stats: null argument");
    *pixels = *chunks = 0;
    if (c->wta_stats_n == 0 || !c->wta_stats.p) return MGM_OK;  // no search of the last aggregation call was a counted pruned one
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<unsigned long long> w(kWtaStatBytes / sizeof(unsigned long long));
    HIPCHK(c, hipMemcpyAsync(w.data(), c->wta_stats.p, kWtaStatBytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < kWtaStatSlots; k++) {  // (pixels << 32 | chunks per slot)
        *pixels += w[(size_t)k * 16] >> 32;
        *chunks += w[(size_t)k * 16] & 0xffffffffull;
    }
    return MGM_OK;
}

int mgm_debug_last_pass_kernel(mgm_ctx *c, char *buf, int cap)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !buf || cap < 1) return fail(c, MGM_ERR_INVALID, "mgm_debug_last_pass_kernel: null argument");
    if (!c->last.batch && !c->rel_last.batch) return fail(c, MGM_ERR_INVALID, "mgm_debug_last_pass_kernel: no aggregation to report");
    const PassKernelChoice &k = c->last.batch ? c->last.kernel : c->rel_last.kernel;
    if (k.family == kPassRefuse) snprintf(buf, (size_t)cap, "k_pass_exact");  // (a dense run without a planned instance)
    else pass_kernel_name(k, buf, (size_t)cap);
    return MGM_OK;
}

// ---- self-tests -------------------------------------------------------------------
// Diagnostic: the rate (GB/s) at which the store pattern of the pass kernels lands on the context's Lr workspace as it is
// placed now -- `nstreams` volumes at the last aggregation's stride written side by side (tools/bimodal_probe.py).
int mgm_debug_probe_workspace(mgm_ctx *c, int nstreams, float *gbps)
{
    if (int jr = pipe_join(c)) return jr;
    if (!c || !gbps || nstreams < 1 || nstreams > 64) return fail(c, MGM_ERR_INVALID, "mgm_debug_probe_workspace: bad arguments");
    if (!c->lr.p || c->last.stride <= 0) return fail(c, MGM_ERR_INVALID, "mgm_debug_probe_workspace: no aggregation has run on this context");
    HIPCHK(c, hipSetDevice(c->device));
    const long long stride = c->last.stride;
    const long long have = (long long)(c->lr.cap / sizeof(float));
    if ((long long)nstreams * stride > have) nstreams = (int)(have / stride);
    if (nstreams < 1) return fail(c, MGM_ERR_INVALID, "mgm_debug_probe_workspace: workspace smaller than one volume");
    const long long per = std::min<long long>(stride, (1ll << 28)) / 4 * 4;  // at most 1 GiB per stream
    hipEvent_t a, b;
    HIPCHK(c, hipEventCreate(&a));
    HIPCHK(c, hipEventCreate(&b));
    HIPCHK(c, launch_probe_streams((float *)c->lr.p, stride, nstreams, per, c->stream));  // (warm)
    HIPCHK(c, hipEventRecord(a, c->stream));
    HIPCHK(c, launch_probe_streams((float *)c->lr.p, stride, nstreams, per, c->stream));
    HIPCHK(c, hipEventRecord(b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *gbps = (float)((double)per * 4.0 * nstreams / (ms * 1e-3) / 1e9);
    return MGM_OK;
}

int mgm_selftest_div3(mgm_ctx *c, unsigned long long *nbad)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !nbad) return fail(c, MGM_ERR_INVALID, "mgm_selftest_div3: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_words(c))) return r;
    unsigned long long *d = (unsigned long long *)ctrl_word(c, kWordCount64);
    HIPCHK(c, hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(c, launch_selftest_div3(d, c->stream));
    HIPCHK(c, hipMemcpyAsync(nbad, d, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MGM_OK;
}

// ---- refinement -----------------------------------------------------------------
int mgm_refine_dev(mgm_ctx *c, const mgm_cv *S, const char *method, mgm_img *out, mgm_img *outcost)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !S || !out || !outcost) return fail(c, MGM_ERR_INVALID, "mgm_refine: null argument");
    if (out->nx != S->nx || out->ny != S->ny || outcost->nx != S->nx || outcost->ny != S->ny)
        return fail(c, MGM_ERR_INVALID, "mgm_refine: image size mismatch");
    const int m = refinement_index(method);
    if (m == 0) return MGM_OK;  // "none" and unknown names (mgm_refine.h:28-35)
    HIPCHK(c, hipSetDevice(c->device));
    TimeScope t(c, "k_refine");
    HIPCHK(c, launch_refine(S->d, (long long)S->nx * S->ny, S->dmax - S->dmin + 1, S->dmin, m, nullptr, nullptr, 0.0f, out->d,
                            outcost->d, c->stream));
    return MGM_OK;
}

int mgm_wta_windowed_dev(mgm_ctx *c, const mgm_cv *C, int NDIR, int fix_overcount, const char *refine, const mgm_img *dminI,
                         const mgm_img *dmaxI, mgm_img *out, mgm_img *outcost)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !C || !dminI || !dmaxI || !out || !outcost) return fail(c, MGM_ERR_INVALID, "mgm_wta_windowed: null argument");
    const int nx = C->nx, ny = C->ny, L = C->dmax - C->dmin + 1;
    for (const mgm_img *im : {dminI, dmaxI, (const mgm_img *)out, (const mgm_img *)outcost})
        if (im->nx != nx || im->ny != ny || im->nch != 1) return fail(c, MGM_ERR_INVALID, "mgm_wta_windowed: image size mismatch");
    if (const int v = c->rel_last.slot_of(C); v >= 0 && c->rel_last.ndir == NDIR) {  // the context's last aggregation of this volume ran on its range-proportional copy
        HIPCHK(c, hipSetDevice(c->device));
        return run_wta_rel(c, C, v, NDIR, fix_overcount, refinement_index(refine), dminI->d, dmaxI->d, out->d, outcost->d);
    }
    const int slot = c->last.slot_of(C);
    if (!c->lr.p || slot < 0 || c->last.ndir != NDIR || c->last.L != L)
        return fail(c, MGM_ERR_INVALID, "mgm_wta_windowed: this volume was not part of the context's last aggregation with NDIR passes");
    HIPCHK(c, hipSetDevice(c->device));
    return run_wta_refine(c, C, 0, (long long)nx * ny, c->last.lr(c->lr, slot, 0), c->last.stride, NDIR, fix_overcount,
                          refinement_index(refine), out->d, outcost->d, nullptr, dminI->d, dmaxI->d, slot);
}

int mgm_wta_right_dev(mgm_ctx *c, const mgm_cv *C, int NDIR, int fix_overcount, const char *refine, mgm_img *outR, mgm_img *outcostR)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !C || !outR || !outcostR) return fail(c, MGM_ERR_INVALID, "mgm_wta_right: null argument");
    const int L = C->dmax - C->dmin + 1, vnx = outR->nx;
    if (vnx < 1 || outR->ny != C->ny || outR->nch != 1 || outcostR->nx != vnx || outcostR->ny != C->ny || outcostR->nch != 1)
        return fail(c, MGM_ERR_INVALID, "mgm_wta_right: image size mismatch (the two outputs are vnx x ny x 1, ny the volume's)");
    const int ridx = refinement_index(refine);
    if (ridx > 1) return fail(c, MGM_ERR_UNSUPPORTED, "mgm_wta_right: refinement none or vfit only");
    if (C->rlo) return fail(c, MGM_ERR_UNSUPPORTED, "mgm_wta_right: a ragged volume (built from range images) has no right view here");
    if (c->rel_last.slot_of(C) >= 0)
        return fail(c, MGM_ERR_UNSUPPORTED, "mgm_wta_right: the last aggregation of this volume ran on its range-proportional copy");
    const int slot = c->last.slot_of(C);
    if (!c->lr.p || slot < 0 || c->last.ndir != NDIR || c->last.L != L)
        return fail(c, MGM_ERR_INVALID, "mgm_wta_right: this volume was not part of the context's last aggregation with NDIR passes");
    HIPCHK(c, hipSetDevice(c->device));
    return run_wta_right(c, C, slot, NDIR, fix_overcount, ridx, vnx, outR->d, outcostR->d);
}

int mgm_wta_runnerup_dev(mgm_ctx *c, const mgm_cv *C, int NDIR, int fix_overcount, int radius, mgm_img *out2, mgm_img *cost2, mgm_img *out1,
                         mgm_img *cost1)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !C || !out2 || !cost2) return fail(c, MGM_ERR_INVALID, "mgm_wta_runnerup: null argument");
    if (radius < 0) return fail(c, MGM_ERR_INVALID, "mgm_wta_runnerup: radius must be >= 0");
    for (const mgm_img *im : {(const mgm_img *)out2, (const mgm_img *)cost2, (const mgm_img *)out1, (const mgm_img *)cost1})
        if (im && (im->nx != C->nx || im->ny != C->ny || im->nch != 1))
            return fail(c, MGM_ERR_INVALID, "mgm_wta_runnerup: image size mismatch (every output is nx x ny x 1, the volume's)");
    const int L = C->dmax - C->dmin + 1;
    if (C->rlo) return fail(c, MGM_ERR_UNSUPPORTED, "mgm_wta_runnerup: a ragged volume (built from range images) has no runner-up search here");
    if (c->rel_last.slot_of(C) >= 0)
        return fail(c, MGM_ERR_UNSUPPORTED, "mgm_wta_runnerup: the last aggregation of this volume ran on its range-proportional copy");
    const int slot = c->last.slot_of(C);
    if (!c->lr.p || slot < 0 || c->last.ndir != NDIR || c->last.L != L)
        return fail(c, MGM_ERR_INVALID, "mgm_wta_runnerup: this volume was not part of the context's last aggregation with NDIR passes");
    HIPCHK(c, hipSetDevice(c->device));
    return run_wta_runnerup(c, C, slot, NDIR, fix_overcount, radius, out2->d, cost2->d, out1 ? out1->d : nullptr, cost1 ? cost1->d : nullptr);
}

int mgm_uniqueness_dev(mgm_ctx *c, const mgm_img *d, const mgm_img *cost1, const mgm_img *cost2, float ratio, mgm_img *out, mgm_img *conf)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !d || !cost1 || !cost2 || (!out && !conf)) return fail(c, MGM_ERR_INVALID, "mgm_uniqueness: null argument (at least one of out, conf)");
    if (!(ratio >= 0.0f && ratio <= 1.0f)) return fail(c, MGM_ERR_INVALID, "mgm_uniqueness: ratio must be finite and in [0, 1]");
    for (const mgm_img *im : {d, cost1, cost2, (const mgm_img *)out, (const mgm_img *)conf})
        if (im && (im->nx != d->nx || im->ny != d->ny || im->nch != 1)) return fail(c, MGM_ERR_INVALID, "mgm_uniqueness: image size mismatch (one channel, one size)");
    if (conf && (conf == d || conf == cost1 || conf == cost2 || conf == out)) return fail(c, MGM_ERR_INVALID, "mgm_uniqueness: conf must be an image of its own");
    if (out && (out == cost1 || out == cost2)) return fail(c, MGM_ERR_INVALID, "mgm_uniqueness: out may be d, not a cost map");
    HIPCHK(c, hipSetDevice(c->device));
    TimeScope t(c, "k_uniqueness");
    HIPCHK(c, launch_uniqueness(d->d, cost1->d, cost2->d, (long long)d->nx * d->ny, ratio, out ? out->d : nullptr, conf ? conf->d : nullptr, c->stream));
    return MGM_OK;
}

// The consensus votes: dense volumes, ragged volumes on their hull and ragged volumes aggregated on their
// range-proportional copy alike -- no cost is read and no sum is formed, so nothing ties the measure to one layout.
int mgm_wta_consensus_dev(mgm_ctx *c, const mgm_cv *C, int NDIR, const mgm_img *d, float tol, mgm_img *votes, mgm_img *winners)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !C || (!votes && !winners) || (votes && !d)) return fail(c, MGM_ERR_INVALID, "mgm_wta_consensus: null argument (at least one of votes, winners; d with votes)");
    if (!(tol >= 0.0f) || !std::isfinite(tol)) return fail(c, MGM_ERR_INVALID, "mgm_wta_consensus: tol must be finite and >= 0");
    if (NDIR < 1 || NDIR > kMaxDirs) return fail(c, MGM_ERR_INVALID, "mgm_wta_consensus: NDIR must be 1..8");
    for (const mgm_img *im : {d, (const mgm_img *)votes})
        if (im && (im->nx != C->nx || im->ny != C->ny || im->nch != 1))
            return fail(c, MGM_ERR_INVALID, "mgm_wta_consensus: image size mismatch (d and votes are nx x ny x 1, the volume's)");
    if (winners && (winners->nx != C->nx || winners->ny != C->ny || winners->nch != NDIR))
        return fail(c, MGM_ERR_INVALID, "mgm_wta_consensus: image size mismatch (winners is nx x ny x NDIR)");
    if ((votes && votes == d) || (winners && (winners == d || winners == votes)))
        return fail(c, MGM_ERR_INVALID, "mgm_wta_consensus: votes and winners must be images of their own");
    const int L = C->dmax - C->dmin + 1;
    if (const int v = c->rel_last.slot_of(C); v >= 0) {  // the context's last aggregation of this volume ran on its range-proportional copy
        if (c->rel_last.ndir != NDIR || c->last.ndir != 0 || !c->lr_rel.p || !C->relbuf || C->rel_slots != c->rel_last.slots || (C->rel_slots != 64 && C->rel_slots != 128))
            return fail(c, MGM_ERR_INVALID, "mgm_wta_consensus: this volume was not part of the context's last aggregation with NDIR passes");
        HIPCHK(c, hipSetDevice(c->device));
        return run_wta_consensus(c, C, v, true, NDIR, d ? d->d : nullptr, tol, votes ? votes->d : nullptr, winners ? winners->d : nullptr);
    }
    const int slot = c->last.slot_of(C);
    if (!c->lr.p || slot < 0 || c->last.ndir != NDIR || c->last.L != L)
        return fail(c, MGM_ERR_INVALID, "mgm_wta_consensus: this volume was not part of the context's last aggregation with NDIR passes");
    HIPCHK(c, hipSetDevice(c->device));
    return run_wta_consensus(c, C, slot, false, NDIR, d ? d->d : nullptr, tol, votes ? votes->d : nullptr, winners ? winners->d : nullptr);
}

int mgm_consensus_filter_dev(mgm_ctx *c, const mgm_img *d, const mgm_img *votes, int minvotes, mgm_img *out)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !d || !votes || !out) return fail(c, MGM_ERR_INVALID, "mgm_consensus_filter: null argument");
    if (minvotes < 0) return fail(c, MGM_ERR_INVALID, "mgm_consensus_filter: minvotes must be >= 0");
    for (const mgm_img *im : {d, votes, (const mgm_img *)out})
        if (im->nx != d->nx || im->ny != d->ny || im->nch != 1) return fail(c, MGM_ERR_INVALID, "mgm_consensus_filter: image size mismatch (one channel, one size)");
    if (votes == d || out == votes) return fail(c, MGM_ERR_INVALID, "mgm_consensus_filter: out may be d, not the votes");
    HIPCHK(c, hipSetDevice(c->device));
    TimeScope t(c, "k_consensus_filter");
    HIPCHK(c, launch_consensus_filter(d->d, votes->d, (long long)d->nx * d->ny, minvotes, out->d, c->stream));
    return MGM_OK;
}

int mgm_update_ranges_dev(mgm_ctx *c, const mgm_img *outoff, mgm_img *dminI, mgm_img *dmaxI, int slack, int radius)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !outoff || !dminI || !dmaxI) return fail(c, MGM_ERR_INVALID, "mgm_update_ranges: null argument");
    for (const mgm_img *im : {(const mgm_img *)dminI, (const mgm_img *)dmaxI})
        if (im->nx != outoff->nx || im->ny != outoff->ny || im->nch != 1 || outoff->nch != 1)
            return fail(c, MGM_ERR_INVALID, "mgm_update_ranges: image size mismatch");
    if (radius < 0 || radius > 16) return fail(c, MGM_ERR_INVALID, "mgm_update_ranges: radius must be 0..16");
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if ((r = ensure_words(c))) return r;
    TimeScope t(c, "k_update_ranges");
    HIPCHK(c, launch_update_ranges(outoff->d, outoff->nx, outoff->ny, slack, radius, dminI->d, dmaxI->d, (float *)ctrl_word(c, kWordRanges), c->stream));
    return MGM_OK;
}

int mgm_median_dev(mgm_ctx *c, const mgm_img *in, int radius, mgm_img *out)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !in || !out || in == out) return fail(c, MGM_ERR_INVALID, "mgm_median: bad arguments");
    if (out->nx != in->nx || out->ny != in->ny || out->nch != in->nch) return fail(c, MGM_ERR_INVALID, "mgm_median: image size mismatch");
    if (radius < 1 || radius > 1024) return fail(c, MGM_ERR_INVALID, "mgm_median: radius must be 1..1024");
    // Beyond radius 7 the order statistic costs 33 sweeps of the (2r+1)^2 window per pixel, read straight from memory
    // (no tiling): bounded here so that the call finishes in about a minute at most -- 1920x1080 up to radius ~190;
    // the launches themselves are cut into pieces of bounded work (mgm_post.hip).
    constexpr double kMedianMaxReads = 1.0e13;
    if (radius > 7 && 33.0 * (2.0 * radius + 1.0) * (2.0 * radius + 1.0) * (double)in->nx * in->ny * in->nch > kMedianMaxReads)
        return fail(c, MGM_ERR_UNSUPPORTED, "mgm_median: window too large for this image (33 * (2r+1)^2 * pixels must stay below 1e13)");
    HIPCHK(c, hipSetDevice(c->device));
    TimeScope t(c, "k_median");
    HIPCHK(c, launch_median(in->d, in->nx, in->ny, in->nch, radius, out->d, c->stream));
    return MGM_OK;
}

// The speckle filter (mgm_speckle.hip): plan_speckle decides the tile, the grids and the scratch, the four phases are four
// launches on the context's stream.  "k_speckle" brackets the call in the timing table, each phase is listed inside it under its
// kernel's name.
int mgm_speckle_dev(mgm_ctx *c, const mgm_img *d, int maxsize, float maxdiff, mgm_img *out, mgm_img *size_map)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !d || (!out && !size_map)) return fail(c, MGM_ERR_INVALID, "mgm_speckle: null argument (at least one of out, size_map)");
    if (maxsize < 0) return fail(c, MGM_ERR_INVALID, "mgm_speckle: maxsize must be >= 0");
    if (!(maxdiff >= 0.0f)) return fail(c, MGM_ERR_INVALID, "mgm_speckle: maxdiff must be >= 0 (+INF allowed, NaN not)");
    for (const mgm_img *im : {d, (const mgm_img *)out, (const mgm_img *)size_map})
        if (im && (im->nx != d->nx || im->ny != d->ny || im->nch != 1)) return fail(c, MGM_ERR_INVALID, "mgm_speckle: image size mismatch (one channel, one size)");
    if (size_map && (size_map == d || size_map == out)) return fail(c, MGM_ERR_INVALID, "mgm_speckle: size_map must be an image of its own");
    const SpeckleChoice choice = plan_speckle(SpeckleRequest{d->nx, d->ny, c->num_cu});
    if (choice.family == kSpeckleRefuse) return fail(c, MGM_ERR_UNSUPPORTED, "mgm_speckle: more than 2^31 - 1 pixels (pixel indices are int32)");
    HIPCHK(c, hipSetDevice(c->device));
    if (int r = reserve(c, c->speckle, (size_t)choice.scratch_bytes)) return r;
    SpeckleParams p{};
    p.d = d->d;
    p.out = out ? out->d : nullptr;
    p.size_map = size_map ? size_map->d : nullptr;
    p.parent = (int *)c->speckle.p;
    p.cnt = p.parent + (size_t)d->nx * d->ny;
    p.nx = d->nx, p.ny = d->ny, p.maxsize = maxsize, p.maxdiff = maxdiff;
    TimeScope t(c, "k_speckle");
    for (int phase = 0; phase < kSpecklePhases; phase++) {
        TimeScope tp(c, speckle_phase_name(phase));
        if (hipError_t e = launch_speckle_phase(phase, p, choice, c->stream)) return hipfail(c, e, speckle_phase_name(phase));
    }
    return MGM_OK;
}

// Hole filling (mgm_holes.hip): plan_holes decides the chunk, the band, the grids and the scratch, every phase is a
// launch of its own on the context's stream.  "k_holes" brackets the call in the timing table, each phase is listed inside it under
// its own name (dirs = 2 has no column and no diagonal phases).
int mgm_fill_holes_dev(mgm_ctx *c, const mgm_img *d, const char *mode, int dirs, int maxdist, mgm_img *out, mgm_img *filled)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !d || (!out && !filled)) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes: null argument (at least one of out, filled)");
    const int m = !mode ? -1 : (!strcmp(mode, "median") ? 0 : (!strcmp(mode, "min") ? 1 : (!strcmp(mode, "max") ? 2 : -1)));
    if (m < 0) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes: mode must be median, min or max");
    if (dirs != 2 && dirs != 4 && dirs != 8) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes: dirs must be 2, 4 or 8");
    if (maxdist < 0) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes: maxdist must be >= 0 (0: no limit)");
    for (const mgm_img *im : {d, (const mgm_img *)out, (const mgm_img *)filled})
        if (im && (im->nx != d->nx || im->ny != d->ny || im->nch != 1)) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes: image size mismatch (one channel, one size)");
    if (filled && (filled == d || filled == out)) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes: filled must be an image of its own");
    const HolesChoice choice = plan_holes(HolesRequest{d->nx, d->ny, dirs, c->num_cu});
    if (choice.family == kHolesRefuse) return fail(c, MGM_ERR_UNSUPPORTED, "mgm_fill_holes: more than 2^31 - 1 pixels (pixel coordinates are int32)");
    HIPCHK(c, hipSetDevice(c->device));
    if (int r = reserve(c, c->holes, (size_t)choice.scratch_bytes)) return r;
    HolesParams p{};
    p.d = d->d;
    p.out = out ? out->d : nullptr;
    p.filled = filled ? filled->d : nullptr;
    p.planes = (float *)c->holes.p;
    p.cpos = (int *)(p.planes + (size_t)choice.planes * d->nx * d->ny);
    p.cval = (float *)(p.cpos + choice.carry_words);
    p.nx = d->nx, p.ny = d->ny, p.dirs = dirs, p.maxdist = maxdist, p.mode = m;
    TimeScope t(c, "k_holes");
    for (int phase = 0; phase < kHolesPhases; phase++) {
        if (!holes_phase_runs(phase, dirs)) continue;
        TimeScope tp(c, holes_phase_name(phase));
        if (hipError_t e = launch_holes_phase(phase, p, choice, c->stream)) return hipfail(c, e, holes_phase_name(phase));
    }
    return MGM_OK;
}

// Hole classification (k_holes_classify in mgm_holes.hip): plan_holes_classify decides the grid, the span and the LDS
// bytes; one launch, no scratch.
int mgm_classify_holes_dev(mgm_ctx *c, const mgm_img *d, const mgm_img *other, int dmin, int dmax, float tau, mgm_img *cls)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !d || !other || !cls) return fail(c, MGM_ERR_INVALID, "mgm_classify_holes: null argument");
    if (d->nch != 1 || other->nch != 1 || cls->nch != 1) return fail(c, MGM_ERR_INVALID, "mgm_classify_holes: every image has one channel");
    if (other->ny != d->ny) return fail(c, MGM_ERR_INVALID, "mgm_classify_holes: the other view's map must have d's height");
    if (cls->nx != d->nx || cls->ny != d->ny) return fail(c, MGM_ERR_INVALID, "mgm_classify_holes: cls must have d's size");
    if (cls == d || cls == other) return fail(c, MGM_ERR_INVALID, "mgm_classify_holes: cls must be an image of its own");
    if (dmin > dmax) return fail(c, MGM_ERR_INVALID, "mgm_classify_holes: dmin must be <= dmax");
    if (!(tau >= 0.0f && tau < __builtin_inff())) return fail(c, MGM_ERR_INVALID, "mgm_classify_holes: tau must be finite and >= 0");
    const HolesClassifyChoice choice = plan_holes_classify(HolesClassifyRequest{d->nx, d->ny, other->nx, c->num_cu, (long long)dmax - dmin + 1});
    if (choice.family == kHolesRefuse) return fail(c, MGM_ERR_UNSUPPORTED, "mgm_classify_holes: more than 2^31 - 1 pixels (pixel coordinates are int32)");
    HIPCHK(c, hipSetDevice(c->device));
    HolesClassifyParams p{};
    p.d = d->d, p.other = other->d, p.cls = cls->d;
    p.nx = d->nx, p.ny = d->ny, p.vnx = other->nx, p.dmin = dmin, p.dmax = dmax, p.tau = tau;
    TimeScope t(c, "k_holes_classify");
    if (hipError_t e = launch_holes_classify(p, choice, c->stream)) return hipfail(c, e, "k_holes_classify");
    return MGM_OK;
}

// The classified fill: mgm_fill_holes_dev's phases on the same scratch with the classified instance of the apply phase.
static int holes_mode5(const char *m)
{
    static const char *const names[5] = {"median", "min", "max", "seclow", "sechigh"};
    for (int k = 0; m && k < 5; k++)
        if (!strcmp(m, names[k])) return k;
    return -1;
}
int mgm_fill_holes_classified_dev(mgm_ctx *c, const mgm_img *d, const mgm_img *cls, const char *mode_occ, const char *mode_mis, int dirs, int maxdist,
                                  mgm_img *out, mgm_img *filled)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !d || !cls || (!out && !filled)) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes_classified: null argument (at least one of out, filled)");
    const int mo = holes_mode5(mode_occ), mm = holes_mode5(mode_mis);
    if (mo < 0 || mm < 0) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes_classified: a mode must be median, min, max, seclow or sechigh");
    if (dirs != 2 && dirs != 4 && dirs != 8) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes_classified: dirs must be 2, 4 or 8");
    if (maxdist < 0) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes_classified: maxdist must be >= 0 (0: no limit)");
    for (const mgm_img *im : {d, cls, (const mgm_img *)out, (const mgm_img *)filled})
        if (im && (im->nx != d->nx || im->ny != d->ny || im->nch != 1))
            return fail(c, MGM_ERR_INVALID, "mgm_fill_holes_classified: image size mismatch (one channel, one size)");
    if (filled && (filled == d || filled == cls || filled == out)) return fail(c, MGM_ERR_INVALID, "mgm_fill_holes_classified: filled must be an image of its own");
    const HolesChoice choice = plan_holes(HolesRequest{d->nx, d->ny, dirs, c->num_cu});
    if (choice.family == kHolesRefuse) return fail(c, MGM_ERR_UNSUPPORTED, "mgm_fill_holes_classified: more than 2^31 - 1 pixels (pixel coordinates are int32)");
    HIPCHK(c, hipSetDevice(c->device));
    if (int r = reserve(c, c->holes, (size_t)choice.scratch_bytes)) return r;
    HolesParams p{};
    p.d = d->d;
    p.cls = cls->d;
    p.out = out ? out->d : nullptr;
    p.filled = filled ? filled->d : nullptr;
    p.planes = (float *)c->holes.p;
    p.cpos = (int *)(p.planes + (size_t)choice.planes * d->nx * d->ny);
    p.cval = (float *)(p.cpos + choice.carry_words);
    p.nx = d->nx, p.ny = d->ny, p.dirs = dirs, p.maxdist = maxdist, p.mode = mm, p.mode_occ = mo;
    TimeScope t(c, "k_holes");
    for (int phase = 0; phase < kHolesPhases; phase++) {
        if (!holes_phase_runs(phase, dirs)) continue;
        TimeScope tp(c, holes_phase_name(phase));
        if (hipError_t e = launch_holes_phase(phase, p, choice, c->stream)) return hipfail(c, e, holes_phase_name(phase));
    }
    return MGM_OK;
}

// Solution energy (mgm_energy.hip): plan_energy_copy names the copy of the volume that is current -- none is made,
// decoded or checked for this --, plan_energy_launch the blocks; one launch.  Totals: the blocks' partials and the map come back,
// the partials are added in index order and the map in raster order (the reference's fp32 sum has no other form).
int mgm_energy_dev(mgm_ctx *c, const mgm_cv *C, const mgm_img *d, const mgm_energy_params *q, mgm_img *E, mgm_energy_totals *tot)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !C || !d || !q || (!E && !tot)) return fail(c, MGM_ERR_INVALID, "mgm_energy: null argument (at least one of E, totals)");
    if (q->kind < 0 || q->kind > 3) return fail(c, MGM_ERR_INVALID, "mgm_energy: kind must be 0 (L1trunc), 1 (L1), 2 (L2) or 3 (model)");
    if (!(q->P1 >= 0.0f && q->P1 < __builtin_inff())) return fail(c, MGM_ERR_INVALID, "mgm_energy: P1 must be finite and >= 0");
    if (!(q->P2 >= 0.0f)) return fail(c, MGM_ERR_INVALID, "mgm_energy: P2 must be >= 0 (+INF allowed, NaN not)");
    if (q->kind == 3 && q->connectivity != 4 && q->connectivity != 8) return fail(c, MGM_ERR_INVALID, "mgm_energy: connectivity must be 4 or 8");
    const mgm_img *w8 = q->kind == 3 ? q->w8 : nullptr;
    if (d->nx != C->nx || d->ny != C->ny || d->nch != 1) return fail(c, MGM_ERR_INVALID, "mgm_energy: d must be a one-channel map of the volume's size");
    if (E && (E->nx != d->nx || E->ny != d->ny || E->nch != 1 || E == d)) return fail(c, MGM_ERR_INVALID, "mgm_energy: E must be a one-channel image of d's size, not d");
    if (w8 && (w8->nx != d->nx || w8->ny != d->ny || w8->nch != 8 || w8 == E)) return fail(c, MGM_ERR_INVALID, "mgm_energy: w8 must have d's size and 8 channels");
    const EnergyLaunch launch = plan_energy_launch(d->nx, d->ny);
    if (launch.blocks < 1) return fail(c, MGM_ERR_UNSUPPORTED, "mgm_energy: more than 2^31 - 1 pixels");
    const long long L = (long long)C->dmax - C->dmin + 1;
    EnergyCopyRequest rq{};
    rq.f32_state = C->f32_state, rq.has_f32 = C->d != nullptr;
    rq.rel_only = C->rel_only, rq.rel_state = (int)C->rel_state, rq.has_rel = C->relbuf != nullptr, rq.rel_slots = C->rel_slots, rq.rel_cb = C->rel_cb;
    rq.p8_state = (int)C->p8_state, rq.has_p8 = C->p8 != nullptr, rq.p8_L = C->p8_L, rq.p8_cb = C->p8_cb;
    rq.c8_state = (int)C->c8_state, rq.has_c8 = C->d8 != nullptr, rq.cbytes = C->cbytes;
    rq.L = (int)L, rq.unfilled = C->unfilled;
    const EnergyCopyChoice copy = plan_energy_copy(rq);
    if (copy.copy == kEnergyCopyNone) return fail(c, MGM_ERR_INVALID, "mgm_energy: the cost volume holds no costs (a refill failed, or no copy of it is current)");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)d->nx * d->ny, pbytes = (size_t)launch.partial_bytes;
    if (tot)
        if (int r = reserve(c, c->energy, pbytes + (E ? 0 : npix * sizeof(float)))) return r;
    EnergyParams p{};
    p.d = d->d;
    p.E = E ? E->d : (tot ? reinterpret_cast<float *>((char *)c->energy.p + pbytes) : nullptr);
    p.partials = tot ? c->energy.p : nullptr;
    p.w8 = w8 ? w8->d : nullptr;
    p.cost = copy.copy == kEnergyCopyF32 ? (const void *)C->d : copy.copy == kEnergyCopyRel ? (const void *)C->relbuf : copy.copy == kEnergyCopyPadded ? (const void *)C->p8 : (const void *)C->d8;
    p.records = copy.copy == kEnergyCopyRel ? C->rel_records() : nullptr;
    p.rlo = C->rlo, p.rhi = C->rlo ? C->rhi : nullptr;
    p.cb = copy.cb, p.stride = copy.stride, p.dmin = C->dmin, p.L = (int)L;
    p.nx = d->nx, p.ny = d->ny, p.kind = q->kind, p.connectivity = q->kind == 3 ? q->connectivity : 4, p.use_fh = q->use_fh != 0;
    p.P1 = q->P1, p.P2 = q->P2;
    {
        TimeScope t(c, "k_energy");
        if (hipError_t e = launch_energy(p, launch.blocks, c->stream)) return hipfail(c, e, "k_energy");
    }
    if (!tot) return MGM_OK;
    std::vector<double> part((size_t)launch.blocks * kEnergyPartialWords);
    std::vector<float> map(npix);
    HIPCHK(c, hipMemcpyAsync(part.data(), p.partials, pbytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(map.data(), p.E, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    mgm_energy_totals r{};
    for (long long b = 0; b < launch.blocks; b++) {  // in index order
        unsigned long long n;
        memcpy(&n, &part[(size_t)b * kEnergyPartialWords + 3], sizeof n);
        r.data += part[(size_t)b * kEnergyPartialWords], r.smooth += part[(size_t)b * kEnergyPartialWords + 1], r.total += part[(size_t)b * kEnergyPartialWords + 2];
        r.finite += n;
    }
    r.pixels = npix;
    float serial = 0;
    for (size_t i = 0; i < npix; i++) serial = serial + map[i];  // ENERGY += G (mgm_print_energy.h:74-80)
    r.serial = serial;
    *tot = r;
    return MGM_OK;
}

// Sub-pixel label spacing (mgm_subpix.hip): the phase image on its own (the build makes its own in the context's
// scratch) and the rescale of a map from fine labels to pixels.
int mgm_subpix_phase_dev(mgm_ctx *c, const mgm_img *v, int s, int k, const char *interp, mgm_img **out)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !v || !out) return fail(c, MGM_ERR_INVALID, "mgm_subpix_phase: null argument");
    if (s != 1 && s != 2 && s != 4) return fail(c, MGM_ERR_INVALID, "mgm_subpix_phase: s must be 1, 2 or 4");
    if (k < 0 || k >= s) return fail(c, MGM_ERR_INVALID, "mgm_subpix_phase: k must be 0 .. s-1");
    const int ip = subpix_interp_index(interp);
    if (ip < 0) return fail(c, MGM_ERR_INVALID, "mgm_subpix_phase: interp must be linear or cubic");
    if (*out && ((*out)->nx != v->nx || (*out)->ny != v->ny || (*out)->nch != v->nch || *out == v))
        return fail(c, MGM_ERR_INVALID, "mgm_subpix_phase: *out is non-NULL but is v or has a different geometry");
    HIPCHK(c, hipSetDevice(c->device));
    const bool provided = *out != nullptr;
    if (!provided)
        if (int r = mgm_img_create(c, v->nx, v->ny, v->nch, out)) return r;
    hipError_t e;
    if (k == 0) {  // v_0 is v, the same bits
        e = hipMemcpyAsync((*out)->d, v->d, sizeof(float) * (size_t)v->nx * v->ny * v->nch, hipMemcpyDeviceToDevice, c->stream);
    } else {
        TimeScope t(c, "k_subpix_phase");
        e = launch_subpix_phase(v->d, v->nx, (long long)v->ny * v->nch, s, k, ip, (*out)->d, c->stream);
    }
    if (e != hipSuccess) {
        const int r = hipfail(c, e, "k_subpix_phase");
        if (!provided) {
            const std::string msg = c->err;
            mgm_img_free(c, *out);
            *out = nullptr;
            c->err = msg;
        }
        return r;
    }
    return MGM_OK;
}

int mgm_subpix_scale_dev(mgm_ctx *c, const mgm_img *in, int s, mgm_img *out)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !in || !out) return fail(c, MGM_ERR_INVALID, "mgm_subpix_scale: null argument");
    if (s != 1 && s != 2 && s != 4) return fail(c, MGM_ERR_INVALID, "mgm_subpix_scale: s must be 1, 2 or 4");
    if (out->nx != in->nx || out->ny != in->ny || out->nch != in->nch) return fail(c, MGM_ERR_INVALID, "mgm_subpix_scale: image size mismatch");
    HIPCHK(c, hipSetDevice(c->device));
    TimeScope t(c, "k_scale_map");
    HIPCHK(c, launch_scale_map(in->d, (long long)in->nx * in->ny * in->nch, s, out->d, c->stream));
    return MGM_OK;
}

int mgm_leftright_dev(mgm_ctx *c, const mgm_img *d, const mgm_img *other, float tau, mgm_img *out)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !d || !other || !out || out == other) return fail(c, MGM_ERR_INVALID, "mgm_leftright: bad arguments");
    if (d->nch != 1 || other->nch != 1 || out->nch != 1 || out->nx != d->nx || out->ny != d->ny || other->ny < d->ny)
        return fail(c, MGM_ERR_INVALID, "mgm_leftright: image size mismatch");
    HIPCHK(c, hipSetDevice(c->device));
    TimeScope t(c, "k_leftright");
    HIPCHK(c, launch_leftright(d->d, d->nx, d->ny, other->d, other->nx, tau, out->d, c->stream));
    return MGM_OK;
}

int mgm_backproject_dev(mgm_ctx *c, const mgm_img *u, const mgm_img *v, const mgm_img *disp, mgm_img *out)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !u || !v || !disp || !out) return fail(c, MGM_ERR_INVALID, "mgm_backproject: null argument");
    if (u->nch != v->nch || disp->nx != u->nx || disp->ny != u->ny || disp->nch != 1 || out->nx != u->nx || out->ny != u->ny ||
        out->nch != u->nch)
        return fail(c, MGM_ERR_INVALID, "mgm_backproject: image size mismatch");
    HIPCHK(c, hipSetDevice(c->device));
    TimeScope t(c, "k_backproject");
    HIPCHK(c, launch_backproject(u->d, u->nx, u->ny, u->nch, v->d, v->nx, v->ny, disp->d, out->d, c->stream));
    return MGM_OK;
}

int mgm_refine(mgm_ctx *c, const mgm_cv *S, const char *method, float *out, float *outcost)
{
    if (!c || !S || !out || !outcost) return fail(c, MGM_ERR_INVALID, "mgm_refine: null argument");
    mgm_img *dout = nullptr, *dcost = nullptr;
    int r = mgm_img_upload(c, out, S->nx, S->ny, 1, &dout);
    if (!r) r = mgm_img_upload(c, outcost, S->nx, S->ny, 1, &dcost);
    if (!r) r = mgm_refine_dev(c, S, method, dout, dcost);
    if (!r) r = mgm_img_download(c, dout, out);
    if (!r) r = mgm_img_download(c, dcost, outcost);
    mgm_img_free(c, dout);
    mgm_img_free(c, dcost);
    return r;
}

}  // extern "C"
