// mgm_volume.hip -- cost volumes and their copies: the one owner of everything that allocates, converts or invalidates a copy
// of a volume (the fp32 array, the compact copy, the padded compact copy, the range-proportional copy).  A filling is a list of
// stages around the HIP-free plan of mgm_fillplan.h: validate and plan, prepare the volume, prepare the inputs, run the attempts,
// commit the last one, gather.  See mgm_host.h.
#include "mgm_host.h"

unsigned long long next_cv_generation()
{
    static unsigned long long g = 0;
    return ++g;
}

// ---- the four ways the contents of a volume change under its copies, each written once -------------------------------------------
// About to be refilled (costvolume_fill): no compact copy yet; K2 flags NaN costs as it writes them.
static void cv_about_to_be_refilled(mgm_cv *cv)
{
    cv->nan_words = false;
    cv->gen = next_cv_generation();
    cv->c8_state = cv->p8_state = CopyState::None;
    cv->nan_state = CopyState::Written;
}
// The refill failed after the volume's state had been touched (a reservation that ran out of memory, a kernel launch error): it
// must not pass for a filled one -- no compact copy, no "NaN-free" verdict.
static void cv_refill_failed(mgm_cv *cv)
{
    cv->c8_state = CopyState::Invalid;
    cv->p8_state = cv->nan_state = CopyState::None;
}
// Freshly uploaded (mgm_cv_upload): the fp32 array alone, not scanned.
static void cv_freshly_uploaded(mgm_cv *cv) { cv->c8_state = cv->p8_state = cv->nan_state = CopyState::None; }
// Written from outside (mgm_cv_device_ptr): the caller may write through the pointer -- the compact copy is derived again at the
// next use, and the range-proportional copy no longer stands for the volume.
static void cv_written_from_outside(mgm_cv *cv)
{
    cv_freshly_uploaded(cv);
    cv->rel_only = false;
    if (cv->rel_state == CopyState::Valid || cv->rel_state == CopyState::Written) cv->rel_state = CopyState::None;
    cv->gen = next_cv_generation();
}

// ---- allocation of the copies -------------------------------------------------------------------------------------------------
// The fp32 array of a volume is allocated when somebody needs it: a volume K2 fills in the compact form only (single-word
// census costs) never does on the hot path.
int cv_alloc_f32(mgm_ctx *c, mgm_cv *cv)
{
    if (cv->d) return MGM_OK;
    const size_t n = (size_t)cv->nx * cv->ny * (size_t)(cv->dmax - cv->dmin + 1);
    hipError_t e = dev_malloc((void **)&cv->d, sizeof(float) * n);
    if (e != hipSuccess) {
        cv->d = nullptr;
        return fail(c, MGM_ERR_NOMEM, std::string("cost volume (fp32): ") + hipGetErrorString(e));
    }
    return MGM_OK;
}
int cv_create(mgm_ctx *c, int nx, int ny, int dmin, int dmax, bool alloc_f32, mgm_cv **out)
{
    if (!c || !out || nx <= 0 || ny <= 0 || dmax < dmin) return fail(c, MGM_ERR_INVALID, "mgm_cv_create: bad arguments");
    const long long L = (long long)dmax - dmin + 1;
    if (L > kMaxLabels)
        return fail(c, MGM_ERR_UNSUPPORTED, "more than 4 194 304 disparity labels per pixel are not supported");
    HIPCHK(c, hipSetDevice(c->device));
    mgm_cv *cv = new mgm_cv();
    cv->d = nullptr;
    cv->nx = nx;
    cv->ny = ny;
    cv->dmin = dmin;
    cv->dmax = dmax;
    cv->owner = c;
    if (alloc_f32)
        if (int r = cv_alloc_f32(c, cv)) {
            delete cv;
            return r;
        }
    if (dev_malloc((void **)&cv->bad8, 64) != hipSuccess) {
        if (cv->d) (void)hipFree(cv->d);
        delete cv;
        return fail(c, MGM_ERR_NOMEM, "mgm_cv_create: flag word");
    }
    cv->gen = next_cv_generation();
    *out = cv;
    return MGM_OK;
}
int c8_alloc(mgm_ctx *c, mgm_cv *cv, int cb)
{
    const size_t n = (size_t)cv->nx * cv->ny * (size_t)(cv->dmax - cv->dmin + 1) * cb + 64;
    if (cv->d8 && cv->d8_cap < n) {  // (refilled with a cost that takes the wider form)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(cv->d8);
        cv->d8 = nullptr;
    }
    if (!cv->d8) {
        if (dev_malloc((void **)&cv->d8, n) != hipSuccess) {
            cv->d8 = nullptr;
            cv->d8_cap = 0;
            return fail(c, MGM_ERR_NOMEM, "hipMalloc of the compact cost volume failed");
        }
        cv->d8_cap = n;
    }
    cv->cbytes = cb;
    return MGM_OK;
}
// room for a padded compact copy of LP label slots, cb bytes each (mgm_cv::p8)
int p8_alloc(mgm_ctx *c, mgm_cv *cv, int LP, int cb)
{
    const size_t n = (size_t)cv->nx * cv->ny * (size_t)LP * cb + 64;
    if (cv->p8 && cv->p8_cap < n) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(cv->p8);
        cv->p8 = nullptr;
    }
    if (!cv->p8) {
        if (dev_malloc((void **)&cv->p8, n) != hipSuccess) {
            cv->p8 = nullptr;
            cv->p8_cap = 0;
            return fail(c, MGM_ERR_NOMEM, "hipMalloc of the padded compact cost volume failed");
        }
        cv->p8_cap = n;
    }
    cv->p8_L = LP;
    cv->p8_cb = cb;
    return MGM_OK;
}
int rel_alloc(mgm_ctx *c, mgm_cv *cv, int slots, int cb)
{
    const size_t npix = (size_t)cv->nx * cv->ny, need = npix * (size_t)slots * (size_t)cb + npix * 16 + 16;
    HIPCHK(c, hipSetDevice(c->device));
    if (cv->rel_cap < need) {
        if (cv->relbuf) {
            HIPCHK(c, hipStreamSynchronize(c->stream));  // (a kernel may still be reading the old copy)
            (void)hipFree(cv->relbuf);
        }
        cv->relbuf = nullptr;
        cv->rel_cap = 0;
        if (dev_malloc((void **)&cv->relbuf, need) == hipSuccess) cv->rel_cap = need;
        else (void)hipGetLastError();
    }
    cv->rel_slots = slots;
    cv->rel_cb = cb;
    return MGM_OK;
}

// ---- conversions between the copies ------------------------------------------------------------------------------------------
// make cv->d current (see mgm_cv::f32_state); enqueued on the context's stream
int ensure_f32(mgm_ctx *c, const mgm_cv *ccv)
{
    mgm_cv *cv = const_cast<mgm_cv *>(ccv);
    if (cv->f32_state) return MGM_OK;
    if (cv->rel_only && cv->rel_state == CopyState::Valid && cv->relbuf) {  // K2 wrote the range-proportional copy alone (ragged census volume)
        if (int r = cv_alloc_f32(c, cv)) return r;
        const long long npix = (long long)cv->nx * cv->ny;
        TimeScope t(c, "k_expand");
        HIPCHK(c, launch_rel_expand(cv->relbuf, cv->rel_records(), npix, cv->dmax - cv->dmin + 1, cv->dmin, cv->rel_slots, cv->rel_cb, cv->d, c->stream));
        cv->f32_state = 1;
        return MGM_OK;
    }
    if (cv->p8_state == CopyState::Valid) {  // K2 wrote the padded compact copy alone
        if (int r = cv_alloc_f32(c, cv)) return r;
        TimeScope t(c, "k_expand");
        HIPCHK(c, launch_expand_padded(cv->p8, cv->p8_cb, (long long)cv->nx * cv->ny, cv->dmax - cv->dmin + 1, cv->p8_L, cv->d, c->stream));
        cv->f32_state = 1;
        return MGM_OK;
    }
    if (!cv->d8 || (cv->c8_state != CopyState::Written && cv->c8_state != CopyState::Valid)) return fail(c, MGM_ERR_INTERNAL, "cost volume has neither an fp32 nor a compact copy");
    if (int r = cv_alloc_f32(c, cv)) return r;
    TimeScope t(c, "k_expand");
    HIPCHK(c, launch_expand(cv->d8, cv->cbytes, (long long)cv->nx * cv->ny * (cv->dmax - cv->dmin + 1), cv->d, c->stream));
    cv->f32_state = 1;
    return MGM_OK;
}
// Decide (once per filling of the volume) whether the compact copy can stand in for C, and whether the volume
// holds NaN costs (mgm_cv::nan_state).  Costs one 4-byte device->host read per filling; MGM_HIP_C8=0 disables the
// compact path.  An uploaded volume is scanned here: by k_compact where it gets a compact copy, else by k_nanscan.
int c8_resolve(mgm_ctx *c, const mgm_cv *ccv, bool *use)
{
    mgm_cv *cv = const_cast<mgm_cv *>(ccv);
    *use = false;
    const int L = cv->dmax - cv->dmin + 1;
    const bool enabled = dev().c8 && c8_supported(L);
    const long long n = (long long)cv->nx * cv->ny * L;
    bool launched = false;
    if (enabled && cv->c8_state == CopyState::None) {  // uploaded / externally written volume: make the compact copy now (one byte per cost)
        int r = ensure_f32(c, cv);  // (a ragged census volume that only has its range-proportional copy)
        if (r) return r;
        r = c8_alloc(c, cv, 1);
        if (r) return r;
        HIPCHK(c, hipMemsetAsync(cv->bad8, 0, 4, c->stream));
        TimeScope t(c, "k_compact");
        HIPCHK(c, launch_compact(cv->d, n, cv->d8, 1, cv->bad8, c->stream));
        cv->c8_state = CopyState::Written;
        cv->nan_state = CopyState::Written;
        launched = true;
    }
    if (cv->nan_state == CopyState::None) {
        if (int r = ensure_f32(c, cv)) return r;
        if (!launched) HIPCHK(c, hipMemsetAsync(cv->bad8, 0, 4, c->stream));
        TimeScope t(c, "k_nanscan");
        HIPCHK(c, launch_nanscan(cv->d, n, cv->bad8, c->stream));
        cv->nan_state = CopyState::Written;
    }
    if (cv->c8_state == CopyState::Written || cv->nan_state == CopyState::Written) {
        unsigned bad = 0;
        if (int r = read_word(c, cv->bad8, &bad)) return r;
        if (cv->c8_state == CopyState::Written) cv->c8_state = (bad & 1u) ? CopyState::Invalid : CopyState::Valid;
        if (cv->nan_state == CopyState::Written) cv->nan_state = (bad & 2u) ? CopyState::Invalid : CopyState::Valid;
        // an uploaded volume of whole numbers beyond 254 (absolute differences of a colour pair computed elsewhere): the
        // two-byte form, where the pass kernels read it (up to 512 labels) -- k_compact says whether it would fit
        if (launched && cv->c8_state == CopyState::Invalid && cv->nan_state == CopyState::Valid && !(bad & 8u) && L <= 512 && cv->f32_state) {
            if (int r = c8_alloc(c, cv, 2)) return r;
            HIPCHK(c, hipMemsetAsync(cv->bad8, 0, 4, c->stream));
            {
                TimeScope t(c, "k_compact");
                HIPCHK(c, launch_compact(cv->d, n, cv->d8, 2, cv->bad8, c->stream));
            }
            if (int r = read_word(c, cv->bad8, &bad)) return r;
            cv->c8_state = (bad & 1u) ? CopyState::Invalid : CopyState::Valid;
        }
        if (cv->c8_state == CopyState::Invalid && !cv->f32_state)
            return fail(c, MGM_ERR_INTERNAL, "cost volume predicted to fit the compact form does not");
    }
    *use = enabled && cv->c8_state == CopyState::Valid;
    return MGM_OK;
}
int rel_resolve(mgm_ctx *c, const mgm_cv *ccv, bool *usable)
{
    mgm_cv *cv = const_cast<mgm_cv *>(ccv);
    *usable = false;
    if (!cv->rlo || !cv->relbuf || cv->rel_state == CopyState::None || cv->rel_state == CopyState::Invalid) return MGM_OK;
    if (cv->rel_state == CopyState::Written) {
        HIPCHK(c, hipSetDevice(c->device));
        if (int r = ensure_words(c)) return r;
        // the flag word of the gathered copy: while it asks for a wider format and rel_next_format (mgm_fillplan.h) has one, the copy is
        // gathered again; what fits none keeps the dense hull
        for (int round = 0; round < 4; round++) {
            unsigned f = 0;
            if (int r = read_word(c, cv->rel_flag(), &f)) return r;
            if (f == 0u) {
                cv->rel_state = CopyState::Valid;
                break;
            }
            int slots = cv->rel_slots, cb = cv->rel_cb;
            if (!rel_next_format(f, cv->f32_state && cv->d, &slots, &cb)) break;
            if (int r = rel_alloc(c, cv, slots, cb)) return r;
            if (!cv->relbuf) break;
            HIPCHK(c, hipMemsetAsync(cv->rel_flag(), 0, 4, c->stream));
            TimeScope t(c, "k_rel_gather");
            HIPCHK(c, launch_rel_gather(cv->d, cv->rlo, cv->rhi, (long long)cv->nx * cv->ny, cv->dmax - cv->dmin + 1, cv->dmin, slots, cb, cv->relbuf,
                                        cv->rel_records(), cv->rel_flag(), c->stream));
        }
        if (cv->rel_state == CopyState::Written) cv->rel_state = CopyState::Invalid;
    }
    *usable = cv->rel_state == CopyState::Valid;
    return MGM_OK;
}

// ---- the filling ------------------------------------------------------------------------------------------------------------------
// gblur_gray with sigma = 1 (img_tools.h:140-180): the taps are computed on the host exactly as there; returns their number
static int gblur_taps(float k[39])
{
    const float sigma = 1.0f;
    const float radius = 3 * fabsf(sigma);
    int rr = (int)ceil((double)(1 + 2 * radius));
    rr = rr < 1 ? 1 : (rr > 39 ? 39 : rr);
    const int cw = (rr - 1) / 2;
    float m = 0;
    for (int i = 0; i < rr; i++) {
        const float x = (float)hypot((double)(i - cw), 0.0);
        const float g = (float)exp((double)(-x * x / (2 * sigma * sigma)));  // (double-precision exp, as compiled there)
        k[i] = g;
        m += g;
    }
    for (int i = 0; i < rr; i++) k[i] /= m;
    return rr;
}

// Stage 2: the volume forgets what it held, its flag word is cleared and it keeps its own copy of the range images (K4-K6 need
// them again).
static int prepare_volume(mgm_ctx *c, mgm_cv *cv, const mgm_img *rloI, const mgm_img *rhiI)
{
    cv_about_to_be_refilled(cv);
    HIPCHK(c, hipMemsetAsync(cv->bad8, 0, 4, c->stream));
    if (rloI) {
        const size_t nb = sizeof(float) * (size_t)cv->nx * cv->ny;
        for (float **q : {&cv->rlo, &cv->rhi})
            if (!*q && dev_malloc((void **)q, nb) != hipSuccess) {
                *q = nullptr;
                return fail(c, MGM_ERR_NOMEM, "mgm_costvolume_build: range images");
            }
        HIPCHK(c, hipMemcpyAsync(cv->rlo, rloI->d, nb, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(cv->rhi, rhiI->d, nb, hipMemcpyDeviceToDevice, c->stream));
    } else if (cv->rlo) {  // a refilled volume that used to be ragged
        (void)hipFree(cv->rlo);
        (void)hipFree(cv->rhi);
        cv->rlo = cv->rhi = nullptr;
    }
    return MGM_OK;
}

// Stage 3: what K2 reads instead of the plain images -- census descriptors, filtered images -- or next to them (window
// statistics, sample spans), in the context's census buffers.
static int prepare_inputs(mgm_ctx *c, const FillPlan &plan, const mgm_img *u, const mgm_img *v, CostParams &p)
{
    int r;
    if (plan.bytes_u && ((r = reserve(c, c->census_u, plan.bytes_u)) || (r = reserve(c, c->census_v, plan.bytes_v)))) return r;
    switch (plan.inputs) {
    case FillInputs::Plain: break;
    case FillInputs::Census:
        for (const mgm_img *im : {u, v}) {
            TimeScope t(c, "k_census");
            HIPCHK(c, launch_census(im->d, im->nx, im->ny, im->nch, p.hwin, (uint32_t *)(im == u ? c->census_u.p : c->census_v.p), c->stream));
        }
        p.cu = (const uint32_t *)c->census_u.p;
        p.cv = (const uint32_t *)c->census_v.p;
        break;
    case FillInputs::Sobelx: {
        TimeScope t(c, "k_filter2d");
        static const float sob[9] = {-1, 0, 1, -2, 0, 2, -1, 0, 1};  // img_tools.h:129-137
        HIPCHK(c, launch_filter2d(u->d, u->nx, u->ny, u->nch, sob, 3, 3, (float *)c->census_u.p, c->stream));
        HIPCHK(c, launch_filter2d(v->d, v->nx, v->ny, v->nch, sob, 3, 3, (float *)c->census_v.p, c->stream));
        break;
    }
    case FillInputs::Gblur: {
        TimeScope t(c, "k_filter2d");
        float k[39];
        const int rr = gblur_taps(k);
        if ((r = reserve(c, c->stmp, plan.bytes_tmp))) return r;
        HIPCHK(c, launch_filter2d(u->d, u->nx, u->ny, u->nch, k, rr, 1, (float *)c->stmp.p, c->stream));
        HIPCHK(c, launch_filter2d((const float *)c->stmp.p, u->nx, u->ny, u->nch, k, 1, rr, (float *)c->census_u.p, c->stream));
        HIPCHK(c, launch_filter2d(v->d, v->nx, v->ny, v->nch, k, rr, 1, (float *)c->stmp.p, c->stream));
        HIPCHK(c, launch_filter2d((const float *)c->stmp.p, v->nx, v->ny, v->nch, k, 1, rr, (float *)c->census_v.p, c->stream));
        break;
    }
    case FillInputs::NccStats:
    case FillInputs::BtSpans:
        p.ncc_u = (float *)c->census_u.p;
        p.ncc_v = (float *)c->census_v.p;
        break;
    }
    if (plan.inputs == FillInputs::Census || plan.inputs == FillInputs::Sobelx || plan.inputs == FillInputs::Gblur) {
        p.u = (const float *)c->census_u.p;  // (-p census with an ad/sd cost: words read as floats)
        p.v = (const float *)c->census_v.p;
    }
    return MGM_OK;
}

// Stage 4: the attempts, from the plan's first one to the one that stands.  Each: room for its target, a clear flag word, the
// kernel plan_cost_kernel chooses for it, the flag word read back where the attempt says so, and fill_step's verdict.
static int run_attempts(mgm_ctx *c, mgm_cv *cv, const FillRequest &req, const FillPlan &plan, const CostParams &p, FillAttempt *last, FillMemory *mem)
{
    int r;
    for (FillAttempt a = plan.first;;) {
        CostParams q = p;
        unsigned *flag = cv->bad8;
        q.C = nullptr, q.C8 = nullptr;
        switch (a.form) {
        case FillForm::RelDirect:
            if ((r = rel_alloc(c, cv, a.slots, a.cbytes))) return r;
            flag = cv->relbuf ? cv->rel_flag() : nullptr;
            break;
        case FillForm::Padded:
            if ((r = p8_alloc(c, cv, a.slots, a.cbytes))) return r;
            q.C8 = cv->p8;
            q.L = a.slots;
            break;
        case FillForm::General:
            if ((r = cv_alloc_f32(c, cv))) return r;
            q.C = cv->d;
            if (!a.cbytes) break;  // (no compact form: the fp32 volume alone)
            [[fallthrough]];
        case FillForm::CompactOnly:
            if ((r = c8_alloc(c, cv, a.cbytes))) return r;
            q.C8 = cv->d8;
            break;
        }
        q.cbytes = a.cbytes;
        if (!flag) {  // (the device has no room for the range-proportional copy)
            a = plan.general;
            continue;
        }
        if (flag != cv->bad8) HIPCHK(c, hipMemsetAsync(flag, 0, 4, c->stream));  // (bad8: cleared by prepare_volume and after a misfit)
        {
            TimeScope t(c, "k_cost");
            if (a.form == FillForm::RelDirect) {
                t.kernel = "k_cost_census_rel";
                HIPCHK(c, launch_cost_census_rel(p.cu, p.cv, p.nx, p.ny, p.vnx, p.vny, p.dmin, p.L, p.trunc, p.rlo, p.rhi, a.slots, cv->relbuf, cv->rel_records(),
                                                 flag, c->stream));
            } else {
                const CostKernelChoice k = plan_cost_kernel(cost_request(req, plan, a));
                t.kernel = k.name;
                HIPCHK(c, launch_cost(q, k, c->stream));  // (a refused choice: hipErrorInvalidValue)
            }
        }
        unsigned word = 0u;
        if (a.readback && (r = read_word(c, flag, &word))) return r;
        const FillStep s = fill_step(plan, a, word, *mem);
        *mem = s.mem;
        if (s.done) {
            *last = a;
            return MGM_OK;
        }
        if (flag == cv->bad8) HIPCHK(c, hipMemsetAsync(flag, 0, 4, c->stream));
        a = s.next;
    }
}

// Stage 5: what the volume knows of its copies, from the attempt that stands.
static void commit_fill(mgm_cv *cv, const FillRequest &q, const FillPlan &plan, const FillAttempt &a, const FillMemory &mem)
{
    const FillState s = fill_state(q, a);
    cv->mem = mem;
    cv->nan_words = plan.nan_words;
    cv->f32_state = s.f32_state;
    cv->nan_state = s.nan_state;
    cv->p8_state = s.p8_state;
    cv->c8_state = s.c8_state;
    cv->rel_only = s.rel_only;
    if (!s.keep_rel_state) cv->rel_state = s.rel_state;
}

// Stage 6: a ragged volume that has its fp32 hull also gets its RANGE-PROPORTIONAL copy (mgm_pass_rel.hip): 64 cost codes per
// pixel at the pixel's own window -- what the aggregation then walks instead of the hull, if every window is at most 62 labels
// wide and every cost has the code (the flag word is read back by the first aggregation, rel_resolve).
static int gather_rel(mgm_ctx *c, mgm_cv *cv, int cb)
{
    if (int r = rel_alloc(c, cv, 64, cb)) return r;
    if (!cv->relbuf) return MGM_OK;
    HIPCHK(c, hipMemsetAsync(cv->rel_flag(), 0, 4, c->stream));
    TimeScope t(c, "k_rel_gather");
    HIPCHK(c, launch_rel_gather(cv->d, cv->rlo, cv->rhi, (long long)cv->nx * cv->ny, cv->dmax - cv->dmin + 1, cv->dmin, 64, cb, cv->relbuf, cv->rel_records(),
                                cv->rel_flag(), c->stream));
    cv->rel_state = CopyState::Written;
    return MGM_OK;
}

static int costvolume_fill(mgm_ctx *c, const mgm_img *u, const mgm_img *v, int dmin, int dmax, const mgm_img *rloI,
                           const mgm_img *rhiI, const char *prefilter, const char *distance, float truncDist, int census_win,
                           mgm_cv **out)
{
    // validate and plan (a refusal leaves a provided volume as it was)
    if (u->nch != v->nch) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build: channel counts differ");
    HIPCHK(c, hipSetDevice(c->device));
    const FillRequest q{u->nx, u->ny, v->nx, v->ny, u->nch, dmax - dmin + 1, distance_index(distance), prefilter_index(prefilter), census_win, truncDist,
                        rloI != nullptr, *out ? (*out)->mem : FillMemory{}, dev().c8, dev().pad, dev().lazy_f32, rel_enabled(), tune_num("rel_direct", 1) != 0};
    const FillPlan plan = plan_fill(q);
    if (plan.err) return fail(c, plan.err, plan.msg);
    int r = MGM_OK;
    if (*out) {  // caller-provided volume to refill (must have the right geometry)
        if ((*out)->nx != u->nx || (*out)->ny != u->ny || (*out)->dmin != dmin || (*out)->dmax != dmax)
            return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build: *C is non-NULL but has a different geometry");
        // (pipelined context: a deferred aggregation still wants the costs this volume holds now)
        if (pipe_uses(c, *out) && (r = pipe_flush(c))) return r;
    } else if ((r = cv_create(c, u->nx, u->ny, dmin, dmax, false, out))) {
        return r;
    }
    mgm_cv *cv = *out;
    if ((r = prepare_volume(c, cv, rloI, rhiI))) return r;

    CostParams p{};
    p.u = u->d, p.v = v->d, p.nx = u->nx, p.ny = u->ny, p.vnx = v->nx, p.vny = v->ny;
    p.bad8 = cv->bad8, p.rlo = cv->rlo, p.rhi = cv->rhi;
    p.dmin = dmin, p.L = p.Lreal = q.L;
    p.costfn = plan.costfn, p.nch = plan.nch, p.trunc = plan.trunc;
    p.hwin = census_win / 2;  // computeC_clippedNCC: CENSUS_NCC_WIN()/2
    if ((r = prepare_inputs(c, plan, u, v, p))) return r;

    FillAttempt last{};
    FillMemory mem = q.mem;
    if ((r = run_attempts(c, cv, q, plan, p, &last, &mem))) return r;
    commit_fill(cv, q, plan, last, mem);
    if (last.form == FillForm::General && plan.gather_cb) return gather_rel(c, cv, plan.gather_cb);
    return MGM_OK;
}

// A volume this call created does not outlive a failure of the call (a caller-provided one stays the caller's).
static int costvolume_build(mgm_ctx *c, const mgm_img *u, const mgm_img *v, int dmin, int dmax, const mgm_img *rloI,
                            const mgm_img *rhiI, const char *prefilter, const char *distance, float truncDist, int census_win,
                            mgm_cv **out)
{
    if (!c || !u || !v || !out) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build: null argument");
    const bool provided = *out != nullptr;
    const int r = costvolume_fill(c, u, v, dmin, dmax, rloI, rhiI, prefilter, distance, truncDist, census_win, out);
    if (*out) {
        // the mark that makes mgm_aggregate* refuse a provided volume whose refill failed
        (*out)->unfilled = r != MGM_OK;
        if (r != MGM_OK) cv_refill_failed(*out);
    }
    if (r != MGM_OK && !provided && *out) {
        const std::string msg = c->err;  // (mgm_cv_free synchronises and may touch the message)
        mgm_cv_free(c, *out);
        *out = nullptr;
        c->err = msg;
    }
    return r;
}

// ---- sub-pixel label spacing: the fine volume gathered from s ordinary builds -----------------------------------------
void subpix_release(mgm_ctx *c)
{
    if (c->subpix_img) {
        (void)hipFree(c->subpix_img->d);
        delete c->subpix_img;
        c->subpix_img = nullptr;
    }
    for (mgm_cv *&cv : c->subpix_cv)
        if (cv) {
            mgm_cv_free(c, cv);
            cv = nullptr;
        }
}
int subpix_interp_index(const char *name)
{
    if (name && !strcmp(name, "linear")) return kSubpixLinear;
    if (name && !strcmp(name, "cubic")) return kSubpixCubic;
    return -1;
}

// The s phase volumes C_k = build(u, v_k) over [dmin, dmax], in the context's scratch (v_0 = v; v_k, k > 0: the scratch image).
static int subpix_build_phases(mgm_ctx *c, const mgm_img *u, const mgm_img *v, int dmin, int dmax, int s, int interp, const char *prefilter,
                               const char *distance, float truncDist, int census_win)
{
    int r;
    bool synced = false;
    const auto sync_once = [&]() -> int {  // (kernels of an earlier call may still read what is about to be freed)
        if (!synced) HIPCHK(c, hipStreamSynchronize(c->stream));
        synced = true;
        return MGM_OK;
    };
    if (c->subpix_img && (c->subpix_img->nx != v->nx || c->subpix_img->ny != v->ny || c->subpix_img->nch != v->nch)) {
        if ((r = sync_once())) return r;
        (void)hipFree(c->subpix_img->d);
        delete c->subpix_img;
        c->subpix_img = nullptr;
    }
    if (!c->subpix_img && (r = mgm_img_create(c, v->nx, v->ny, v->nch, &c->subpix_img))) return r;
    for (int k = 0; k < 4; k++) {
        mgm_cv *&cv = c->subpix_cv[k];
        if (cv && (k >= s || cv->nx != u->nx || cv->ny != u->ny || cv->dmin != dmin || cv->dmax != dmax)) {
            mgm_cv_free(c, cv);  // (synchronises)
            cv = nullptr;
        }
    }
    for (int k = 0; k < s; k++) {
        const mgm_img *vk = v;
        if (k > 0) {
            TimeScope t(c, "k_subpix_phase");
            HIPCHK(c, launch_subpix_phase(v->d, v->nx, (long long)v->ny * v->nch, s, k, interp, c->subpix_img->d, c->stream));
            vk = c->subpix_img;
        }
        if ((r = costvolume_build(c, u, vk, dmin, dmax, nullptr, nullptr, prefilter, distance, truncDist, census_win, &c->subpix_cv[k]))) return r;
    }
    return MGM_OK;
}

// The gather.  When the plan of a direct build of F's label count starts in a one-byte form that fits by construction (single-word
// census under a truncation that is a byte code) and every phase holds valid one-byte codes, F gets that form -- the compact copy,
// or the padded compact copy where the builder would have written one -- and its fp32 copy is stale.  In every other case the phases
// are brought to fp32 (ensure_f32) and F is an fp32 volume that knows nothing of its copies, like an uploaded one.
static int subpix_gather(mgm_ctx *c, const mgm_img *u, const mgm_img *v, int s, const char *prefilter, const char *distance, float truncDist,
                         int census_win, mgm_cv *F)
{
    int r;
    const int Lf = F->dmax - F->dmin + 1;
    const long long npix = (long long)F->nx * F->ny;
    const FillRequest q{u->nx, u->ny, v->nx, v->ny, u->nch, Lf, distance_index(distance), prefilter_index(prefilter), census_win, truncDist,
                        false, FillMemory{}, dev().c8, dev().pad, dev().lazy_f32, rel_enabled(), tune_num("rel_direct", 1) != 0};
    const FillPlan plan = plan_fill(q);
    const FillAttempt a = plan.first;
    bool codes = !plan.err && (a.form == FillForm::CompactOnly || a.form == FillForm::Padded) && !a.readback && a.cbytes == 1;
    SubpixParams p{};
    p.npix = npix, p.labels = Lf, p.s = s;
    for (int k = 0; k < s && codes; k++) {  // every phase in ONE one-byte form
        const mgm_cv *P = c->subpix_cv[k];
        const bool c8 = P->c8_state == CopyState::Valid && P->d8 && P->cbytes == 1, p8 = P->p8_state == CopyState::Valid && P->p8 && P->p8_cb == 1;
        const int slots = c8 ? P->dmax - P->dmin + 1 : p8 ? P->p8_L : 0;
        codes = slots != 0 && (k == 0 || slots == p.in_slots);
        p.in_slots = slots;
        p.phase[k] = c8 ? P->d8 : P->p8;
    }
    bool nan_words = false;
    if (codes) {
        p.cb = 1, p.slots = a.slots;
        if (a.form == FillForm::Padded) {
            if ((r = p8_alloc(c, F, a.slots, 1))) return r;
            p.F = F->p8;
        } else {
            if ((r = c8_alloc(c, F, 1))) return r;
            p.F = F->d8;
        }
    } else {
        for (int k = 0; k < s; k++) {
            if ((r = ensure_f32(c, c->subpix_cv[k]))) return r;
            p.phase[k] = c->subpix_cv[k]->d;
            nan_words |= c->subpix_cv[k]->nan_words;
        }
        if ((r = cv_alloc_f32(c, F))) return r;
        p.cb = 4, p.slots = Lf, p.in_slots = (Lf - 1) / s + 1, p.F = F->d;
    }
    const SubpixChoice choice = plan_subpix(SubpixRequest{p.npix, p.labels, p.slots, p.in_slots, p.s, p.cb, c->num_cu});
    if (choice.family == kSubpixRefuse) return fail(c, MGM_ERR_INTERNAL, "mgm_costvolume_build_subpix: no launch plan for this volume");
    {
        TimeScope t(c, "k_cv_interleave");
        if (hipError_t e = launch_cv_interleave(p, choice, c->stream)) return hipfail(c, e, "k_cv_interleave");
    }
    if (codes) {
        commit_fill(F, q, plan, a, FillMemory{});
    } else {
        cv_freshly_uploaded(F);
        F->mem = FillMemory{};
        F->f32_state = 1;
        F->rel_only = false;
        F->rel_state = CopyState::None;
        F->nan_words = nan_words;
    }
    return MGM_OK;
}

static int costvolume_build_subpix(mgm_ctx *c, const mgm_img *u, const mgm_img *v, int dmin, int dmax, int s, const char *interp, const char *prefilter,
                                   const char *distance, float truncDist, int census_win, mgm_cv **out)
{
    if (!c || !u || !v || !out) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_subpix: null argument");
    if (s != 1 && s != 2 && s != 4) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_subpix: s must be 1, 2 or 4");
    const int ip = subpix_interp_index(interp);
    if (ip < 0) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_subpix: interp must be linear or cubic");
    if (dmax < dmin) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_subpix: dmax < dmin");
    if (u->nch != v->nch) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_subpix: channel counts differ");
    const long long flo = (long long)s * dmin, fhi = (long long)s * dmax;
    if (flo < -2147483647ll - 1 || fhi > 2147483647ll) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_subpix: s * dmin .. s * dmax does not fit an int");
    if (fhi - flo + 1 > kMaxLabels) return fail(c, MGM_ERR_UNSUPPORTED, "more than 4 194 304 disparity labels per pixel are not supported");
    if (s == 1) return costvolume_build(c, u, v, dmin, dmax, nullptr, nullptr, prefilter, distance, truncDist, census_win, out);  // F is C_0
    HIPCHK(c, hipSetDevice(c->device));
    int r;
    if (*out) {
        if ((*out)->nx != u->nx || (*out)->ny != u->ny || (*out)->dmin != (int)flo || (*out)->dmax != (int)fhi)
            return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_subpix: *F is non-NULL but has a different geometry");
        if (pipe_uses(c, *out) && (r = pipe_flush(c))) return r;
        for (const mgm_cv *P : c->subpix_cv)
            if (P == *out) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_subpix: *F is one of the context's own volumes");
    }
    // a refusal of the ordinary build (a census window that is no multiple of 8 bits, ...) comes before anything is touched
    if ((r = subpix_build_phases(c, u, v, dmin, dmax, s, ip, prefilter, distance, truncDist, census_win))) return r;
    const bool provided = *out != nullptr;
    if (!provided && (r = cv_create(c, u->nx, u->ny, (int)flo, (int)fhi, false, out))) return r;
    mgm_cv *F = *out;
    r = prepare_volume(c, F, nullptr, nullptr);
    if (!r) r = subpix_gather(c, u, v, s, prefilter, distance, truncDist, census_win, F);
    F->unfilled = r != MGM_OK;
    if (r != MGM_OK) {
        cv_refill_failed(F);
        if (!provided) {
            const std::string msg = c->err;
            mgm_cv_free(c, F);
            *out = nullptr;
            c->err = msg;
        }
    }
    return r;
}

extern "C" {

int mgm_costvolume_build_subpix_dev(mgm_ctx *c, const mgm_img *u, const mgm_img *v, int dmin, int dmax, int s, const char *interp,
                                    const char *prefilter, const char *distance, float truncDist, int census_win, mgm_cv **F)
{
    return costvolume_build_subpix(c, u, v, dmin, dmax, s, interp, prefilter, distance, truncDist, census_win, F);
}

int mgm_costvolume_build_dev(mgm_ctx *c, const mgm_img *u, const mgm_img *v, int dmin, int dmax, const char *prefilter,
                             const char *distance, float truncDist, int census_win, mgm_cv **out)
{
    return costvolume_build(c, u, v, dmin, dmax, nullptr, nullptr, prefilter, distance, truncDist, census_win, out);
}

int mgm_costvolume_build_ranged_dev(mgm_ctx *c, const mgm_img *u, const mgm_img *v, const mgm_img *dminI, const mgm_img *dmaxI,
                                    int hull_min, int hull_max, const char *prefilter, const char *distance, float truncDist,
                                    int census_win, mgm_cv **out)
{
    if (!c || !u || !dminI || !dmaxI) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_ranged: null argument");
    for (const mgm_img *im : {dminI, dmaxI})
        if (im->nx != u->nx || im->ny != u->ny || im->nch != 1)
            return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build_ranged: the range images must have the left image's size");
    return costvolume_build(c, u, v, hull_min, hull_max, dminI, dmaxI, prefilter, distance, truncDist, census_win, out);
}

int mgm_costvolume_build(mgm_ctx *c, const float *u, const float *v, int nx, int ny, int nch, int vnx, int vny,
                         const float *dminI, const float *dmaxI, const char *prefilter, const char *distance,
                         float truncDist, int census_win, mgm_cv **out)
{
    if (!c || !u || !v || !dminI || !dmaxI || !out) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build: null argument");
    // Dvec::init receives the float range values converted to int (dvec.cc:55-60)
    int dmin = (int)dminI[0], dmax = (int)dmaxI[0];
    bool ragged = false;
    for (long long i = 0; i < (long long)nx * ny; i++) {
        const int lo = (int)dminI[i], hi = (int)dmaxI[i];
        if (hi < lo) return fail(c, MGM_ERR_INVALID, "mgm_costvolume_build: a pixel's range is empty (dmax < dmin)");
        ragged |= lo != dmin || hi != dmax;
    }
    if (ragged)  // the dense layout spans the hull of all ranges
        for (long long i = 0; i < (long long)nx * ny; i++) {
            dmin = std::min(dmin, (int)dminI[i]);
            dmax = std::max(dmax, (int)dmaxI[i]);
        }
    mgm_img *du = nullptr, *dv = nullptr, *dlo = nullptr, *dhi = nullptr;
    *out = nullptr;
    int r = mgm_img_upload(c, u, nx, ny, nch, &du);
    if (!r) r = mgm_img_upload(c, v, vnx, vny, nch, &dv);
    if (!r && ragged) r = mgm_img_upload(c, dminI, nx, ny, 1, &dlo);
    if (!r && ragged) r = mgm_img_upload(c, dmaxI, nx, ny, 1, &dhi);
    if (!r)
        r = ragged ? mgm_costvolume_build_ranged_dev(c, du, dv, dlo, dhi, dmin, dmax, prefilter, distance, truncDist, census_win, out)
                   : mgm_costvolume_build_dev(c, du, dv, dmin, dmax, prefilter, distance, truncDist, census_win, out);
    if (!r) r = mgm_ctx_synchronize(c);
    for (mgm_img *im : {du, dv, dlo, dhi}) mgm_img_free(c, im);
    return r;
}

// ---- volumes --------------------------------------------------------------
int mgm_cv_create(mgm_ctx *c, int nx, int ny, int dmin, int dmax, mgm_cv **out) { return cv_create(c, nx, ny, dmin, dmax, true, out); }
int mgm_cv_upload(mgm_ctx *c, const float *dense, int nx, int ny, int dmin, int dmax, mgm_cv **out)
{
    if (!dense) return fail(c, MGM_ERR_INVALID, "mgm_cv_upload: null host pointer");
    int r = mgm_cv_create(c, nx, ny, dmin, dmax, out);
    if (r) return r;
    const size_t n = (size_t)nx * ny * (size_t)(dmax - dmin + 1);
    hipError_t e = hipMemcpyAsync((*out)->d, dense, sizeof(float) * n, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        r = hipfail(c, e, "mgm_cv_upload: copy");
        mgm_cv_free(c, *out);
        *out = nullptr;
        return r;
    }
    cv_freshly_uploaded(*out);
    return MGM_OK;
}
int mgm_cv_download(mgm_ctx *c, const mgm_cv *cv, float *dense)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !cv || !dense) return fail(c, MGM_ERR_INVALID, "mgm_cv_download: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    if (int r = ensure_f32(c, cv)) return r;
    const size_t n = (size_t)cv->nx * cv->ny * (size_t)(cv->dmax - cv->dmin + 1);
    HIPCHK(c, hipMemcpyAsync(dense, cv->d, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    return mgm_ctx_synchronize(c);
}
int mgm_cv_dims(const mgm_cv *cv, int *nx, int *ny, int *dmin, int *dmax)
{
    if (!cv) return MGM_ERR_INVALID;
    if (nx) *nx = cv->nx;
    if (ny) *ny = cv->ny;
    if (dmin) *dmin = cv->dmin;
    if (dmax) *dmax = cv->dmax;
    return MGM_OK;
}
int mgm_cv_device(const mgm_cv *cv) { return (cv && cv->owner) ? cv->owner->device : -1; }
void *mgm_cv_device_ptr(mgm_cv *cv)
{
    if (cv) (void)pipe_join(cv->owner);
    if (!cv) return nullptr;
    if (cv->owner && ensure_f32(cv->owner, cv)) return nullptr;
    cv_written_from_outside(cv);
    return cv->d;
}
int mgm_cv_free(mgm_ctx *c, mgm_cv *cv)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!cv) return MGM_OK;
    // (freed through another context, or with none: the context that made the volume may still hold deferred calls on it)
    if (cv->owner && cv->owner != c && pipe_uses(cv->owner, cv)) (void)pipe_join(cv->owner);
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    for (mgm_ctx *o : {c, cv->owner})  // no context's record of its last aggregation keeps the address
        if (o) {
            o->last.forget(cv);
            o->rel_last.forget(cv);
        }
    if (cv->d) (void)hipFree(cv->d);
    if (cv->d8) (void)hipFree(cv->d8);
    if (cv->p8) (void)hipFree(cv->p8);
    if (cv->bad8) (void)hipFree(cv->bad8);
    if (cv->relbuf) (void)hipFree(cv->relbuf);
    if (cv->rlo) (void)hipFree(cv->rlo);
    if (cv->rhi) (void)hipFree(cv->rhi);
    delete cv;
    return MGM_OK;
}

}  // extern "C"
