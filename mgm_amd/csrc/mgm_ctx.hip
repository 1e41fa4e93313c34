// mgm_ctx.hip -- contexts, images, development switches, timing: the part of the C ABI of libmgm_hip.so (include/mgm_hip.h)
// that owns the contexts' memory (the volumes and their copies: mgm_volume.hip).  See mgm_host.h.
#include "mgm_host.h"

// ---- development switches: ONE place, ONE variable -------------------------------------------------------------------------
// MGM_HIP_TUNE="key=value,key=value,..." -- or, as in rounds 1-3 (tests and tools still use them), the individual variables
// MGM_HIP_<KEY>.  Read once per process.  -DMGM_HIP_RELEASE compiles all of it out: every switch keeps its default.
long long mgm::tune_num(const char *key, long long dflt)
{
#ifdef MGM_HIP_RELEASE
    (void)key;
    return dflt;
#else
    static const std::vector<std::pair<std::string, long long>> table = [] {
        std::vector<std::pair<std::string, long long>> t;
        if (const char *e = getenv("MGM_HIP_TUNE")) {
            std::string s(e);
            size_t i = 0;
            while (i < s.size()) {
                size_t j = s.find(',', i);
                if (j == std::string::npos) j = s.size();
                const std::string item = s.substr(i, j - i);
                const size_t q = item.find('=');
                if (q != std::string::npos && q > 0) t.emplace_back(item.substr(0, q), atoll(item.c_str() + q + 1));
                i = j + 1;
            }
        }
        return t;
    }();
    for (const auto &kv : table)
        if (kv.first == key) return kv.second;
    std::string legacy = "MGM_HIP_";
    for (const char *q = key; *q; q++) legacy += (char)toupper((unsigned char)*q);
    if (const char *e = getenv(legacy.c_str())) return atoll(e);
    return dflt;
#endif
}

const DevSwitches &dev()
{
    static const DevSwitches d = [] {
        auto on = [](const char *n) { return tune_num(n, 1) != 0; };
        return DevSwitches{on("c8"), on("lazy_f32"), on("pad"), (int)tune_num("subv", 1), (int)tune_num("deep", -1),
                           (int)tune_num("wg_per_cu", 0), (int)tune_num("xflags", 0), (int)tune_num("strips", -1), (int)tune_num("xcdq", -1),
                           (int)tune_num("xcdq_k", -1), on("w2"), on("oneb"), 64ll * tune_num("lr_pad", 67)};
    }();
    return d;
}
long long lr_pad_floats() { return dev().lr_pad; }
const WtaSwitches &wta_switches()
{
    // (wta_prune_ppw: 1 since the search keeps two rounds of chunk loads in flight, which only the PPW = 1 instances have registers for)
    static const WtaSwitches w{(int)tune_num("wta_prune_ppw", 1),(int)tune_num("wta_prune_wg", 0), (int)tune_num("wta_wg_per_cu", 0),
                               tune_num("wta_packed", 1) != 0, tune_num("wta_wide4", 1) != 0, tune_num("wta_quad", 1) != 0,
                               (int)tune_num("wta_right_seg", 0)};
    return w;
}

int fail(mgm_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    return code;
}
int hipfail(mgm_ctx *c, hipError_t e, const char *what)
{
    // (round 6) the runtime keeps its last error until somebody reads it, and every launch wrapper ends with `return hipGetLastError()`:
    // an error that was returned DIRECTLY by a call (hipFuncSetAttribute refusing an LDS request, ...) would otherwise be reported once
    // more by the next, innocent, launch of the process
    (void)hipGetLastError();
    return fail(c, MGM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(c, call)                                          \
    do {                                                         \
        hipError_t e__ = (call);                                 \
        if (e__ != hipSuccess) return hipfail((c), e__, #call);  \
    } while (0)

// hipMalloc whose failure does not outlive the call: the runtime keeps the last error until somebody reads it, and every
// launch wrapper here ends with `return hipGetLastError()` -- without this, the first kernel launched after an
// MGM_ERR_NOMEM return (the smaller chunk mgm_aggregate_batch_dev retries with, or simply the caller's next call) would
// report the stale hipErrorOutOfMemory as its own.
hipError_t dev_malloc(void **p, size_t bytes)
{
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        *p = nullptr;
        (void)hipGetLastError();
    }
    return e;
}

int reserve(mgm_ctx *c, Buf &b, size_t bytes)
{
    if (bytes <= b.cap) return MGM_OK;
    if (b.p) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    hipError_t e = dev_malloc(&b.p, bytes);
    if (e != hipSuccess) {
        return fail(c, MGM_ERR_NOMEM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    }
    b.cap = bytes;
    return MGM_OK;
}

// the control words (CtrlWord, mgm_host.h): zeroed when they come into being -- no launch resets the watchdog word (check_watchdog)
int ensure_words(mgm_ctx *c)
{
    const void *before = c->words.p;
    if (int r = reserve(c, c->words, sizeof(unsigned) * (size_t)kCtrlWordsTotal)) return r;
    if (c->words.p != before) HIPCHK(c, hipMemsetAsync(c->words.p, 0, c->words.cap, c->stream));
    return MGM_OK;
}
int read_word(mgm_ctx *c, const unsigned *dev, unsigned *out)
{
    HIPCHK(c, hipMemcpyAsync(c->h_words + kHostFlag, dev, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *out = c->h_words[kHostFlag];
    return MGM_OK;
}

// name tables with the reference's silent fall-back to entry 0
int distance_index(const char *n)  // mgm_costvolume.h:170-190
{
    static const char *t[] = {"ad", "sd", "census", "ncc", "btad", "btsd", nullptr};
    int r = 0;
    for (int i = 0; t[i]; i++)
        if (n && !strcmp(n, t[i])) r = i;
    return r;
}
int prefilter_index(const char *n)  // mgm_costvolume.h:194-207
{
    static const char *t[] = {"none", "census", "sobelx", "gblur", nullptr};
    int r = 0;
    for (int i = 0; t[i]; i++)
        if (n && !strcmp(n, t[i])) r = i;
    return r;
}
int refinement_index(const char *n)  // mgm_refine.h:15-35
{
    static const char *t[] = {"none", "vfit", "parabola", "cubic", "parabolaOCV", nullptr};
    int r = 0;
    for (int i = 0; t[i]; i++)
        if (n && !strcmp(n, t[i])) r = i;
    return r;
}

// The watchdog word of the pass kernel is STICKY on the device: no launch resets it, a copy of it follows every pass
// launch into its pinned mirror (watch_launch), and only the host clears it, once it has seen it set.  A hand-off time-out of one launch is
// therefore reported by whichever call next finds the stream idle (block = false: pass launches look without waiting --
// nothing on the hot path synchronises for it) or synchronises anyway (block = true), and cannot be overwritten by a
// later launch's copy.
int watch_launch(mgm_ctx *c)
{
    HIPCHK(c, hipMemcpyAsync(c->h_words + kHostWatchdog, ctrl_word(c, kWordWatchdog), sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    c->pending_check = true;
    return MGM_OK;
}
int check_watchdog(mgm_ctx *c, bool block)
{
    if (!c->pending_check) return MGM_OK;
    if (block) HIPCHK(c, hipStreamSynchronize(c->stream));
    else if (hipStreamQuery(c->stream) != hipSuccess) return MGM_OK;  // still running: the word is looked at later
    c->pending_check = false;
    if (c->h_words[kHostWatchdog] != 0) {
        c->h_words[kHostWatchdog] = 0;
        if (c->words.p) (void)hipMemsetAsync(ctrl_word(c, kWordWatchdog), 0, sizeof(unsigned), c->stream);
        forget_hand_regions(c);  // (the launch, dense or range-proportional, may have left its hand-off slots half written)
        return fail(c, MGM_ERR_INTERNAL, "pass kernel watchdog: inter-band hand-off timed out");
    }
    return MGM_OK;
}

bool pipe_uses(const mgm_ctx *c, const void *obj)  // is `obj` (a volume or an image) an operand of a deferred call?
{
    if (!c || !obj) return false;
    for (const auto &q : c->pend) {
        for (const mgm_cv *x : q.C) if (x == obj) return true;
        for (const mgm_img *x : q.w8) if (x == obj) return true;
        for (const mgm_img *x : q.out) if (x == obj) return true;
        for (const mgm_img *x : q.outcost) if (x == obj) return true;
    }
    return false;
}

// the grow-only workspace: what mgm_ctx_trim hands back (the control words stay until the context goes)
static std::vector<Buf *> workspace_bufs(mgm_ctx *c)
{
    std::vector<Buf *> bufs = {&c->lr, &c->hand.buf, &c->hand2, &c->handm, &c->exact_mins, &c->exact_scratch, &c->census_u, &c->census_v, &c->dbg, &c->stmp, &c->ones8,
                               &c->lr_rel, &c->hand_rel.buf, &c->lmin, &c->wta_stats, &c->wvals, &c->speckle, &c->holes, &c->energy};
    for (int v = 0; v < kMaxBatch; v++) bufs.insert(bufs.end(), {&c->padf[v], &c->pad8[v], &c->wsel[v]});
    return bufs;
}
static void release(Buf &b) { if (b.p) (void)hipFree(b.p), b = Buf{}; }

// ---------------------------------------------------------------------------
extern "C" {

const char *mgm_version(void) { return "mgm-hip 0.1 (gfx950)"; }

int mgm_ctx_create(int device, mgm_ctx **out)
{
    if (!out) return MGM_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return MGM_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return MGM_ERR_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return MGM_ERR_HIP;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MGM_ERR_HIP;  // the kernels exist for gfx950 only
    mgm_ctx *c = new mgm_ctx();
    c->device = device;
    c->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return MGM_ERR_HIP;
    }
    if (hipHostMalloc((void **)&c->h_words, kHostWords * sizeof(unsigned), hipHostMallocDefault) != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return MGM_ERR_HIP;
    }
    memset(c->h_words, 0, kHostWords * sizeof(unsigned));
    c->force_build = (int)tune_num("pass_build", 0);
    c->debug_stats = (int)tune_num("debug_stats", 0);
    *out = c;
    return MGM_OK;
}

int mgm_ctx_destroy(mgm_ctx *c)
{
    if (!c) return MGM_OK;
    (void)hipSetDevice(c->device);
    (void)pipe_join(c);  // (deferred calls of a pipelined context still write the caller's images)
    (void)hipStreamSynchronize(c->stream);
    c->dense_plans.free_all();
    c->rel_plans.free_all();
    for (Buf *b : workspace_bufs(c)) release(*b);
    subpix_release(c);
    release(c->words);
    for (auto &t : c->tim) {
        if (t.alias) continue;
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    if (c->h_words) (void)hipHostFree(c->h_words);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return MGM_OK;
}

// Pipelined context: see mgm_hip.h.  depth 1 switches it off (after running whatever was deferred).
int mgm_ctx_set_pipeline(mgm_ctx *c, int depth)
{
    if (!c) return MGM_ERR_INVALID;
    if (depth < 1 || depth > kMaxBatch) return fail(c, MGM_ERR_INVALID, "mgm_ctx_set_pipeline: depth must be 1..16");
    if (int r = mgm_ctx_synchronize(c)) return r;
    c->pipe_depth = depth;
    return MGM_OK;
}

// The workspace (Lr volumes, hand-off slots, census images, ...) only ever grows with the largest call seen; this hands
// it back to the device.  The next call allocates what it needs again; mgm_wta_windowed_dev / mgm_debug_download_lr /
// mgm_lr_device_ptr have nothing to work on until the next aggregation.
int mgm_ctx_trim(mgm_ctx *c)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c) return MGM_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (int r = mgm_ctx_synchronize(c)) return r;
    c->last.clear();
    c->rel_last.clear();
    c->wta_stats_n = 0;
    for (Buf *b : workspace_bufs(c)) release(*b);
    subpix_release(c);
    forget_hand_regions(c);
    c->dense_plans.free_all();
    c->rel_plans.free_all();
    return MGM_OK;
}

int mgm_ctx_set_workspace_limit(mgm_ctx *c, unsigned long long bytes)
{
    if (!c) return MGM_ERR_INVALID;
    c->ws_limit = (size_t)bytes;
    return MGM_OK;
}

int mgm_ctx_set_placement_tries(mgm_ctx *c, int tries)
{
    if (!c || tries < 0 || tries > 8) return MGM_ERR_INVALID;
    c->place_tries = tries;
    return MGM_OK;
}

int mgm_ctx_mem_info(mgm_ctx *c, unsigned long long *free_bytes, unsigned long long *total_bytes)
{
    if (!c) return MGM_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    size_t f = 0, t = 0;
    HIPCHK(c, hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return MGM_OK;
}

const char *mgm_last_error(const mgm_ctx *c) { return c ? c->err.c_str() : "null context"; }

void *mgm_ctx_stream(mgm_ctx *c) { return c ? (void *)c->stream : nullptr; }

int mgm_ctx_synchronize(mgm_ctx *c)
{
    if (!c) return MGM_ERR_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    if (int r = pipe_join(c)) return r;  // (pipelined context: run what has been deferred)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return check_watchdog(c);
}

int mgm_timing_enable(mgm_ctx *c, int enable)
{
    if (!c) return MGM_ERR_INVALID;
    c->timing = enable != 0;
    return MGM_OK;
}
int mgm_timing_reset(mgm_ctx *c)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c) return MGM_ERR_INVALID;
    (void)hipStreamSynchronize(c->stream);
    for (auto &t : c->tim) {
        if (t.alias) continue;
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    c->tim.clear();
    return MGM_OK;
}
int mgm_timing_count(mgm_ctx *c) { return c ? (int)c->tim.size() : 0; }
int mgm_timing_get(mgm_ctx *c, int idx, const char **name, float *ms)
{
    if (!c || idx < 0 || idx >= (int)c->tim.size()) return MGM_ERR_INVALID;
    HIPCHK(c, hipEventSynchronize(c->tim[idx].b));
    float t = 0;
    HIPCHK(c, hipEventElapsedTime(&t, c->tim[idx].a, c->tim[idx].b));
    if (name) *name = c->tim[idx].name;
    if (ms) *ms = t;
    return MGM_OK;
}

// ---- images ---------------------------------------------------------------
int mgm_img_create(mgm_ctx *c, int nx, int ny, int nch, mgm_img **out)
{
    if (!c || !out || nx <= 0 || ny <= 0 || nch <= 0) return fail(c, MGM_ERR_INVALID, "mgm_img_create: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    mgm_img *im = new mgm_img{nullptr, nx, ny, nch, c->device};
    hipError_t e = dev_malloc((void **)&im->d, sizeof(float) * (size_t)nx * ny * nch);
    if (e != hipSuccess) {
        delete im;
        return fail(c, MGM_ERR_NOMEM, std::string("mgm_img_create: ") + hipGetErrorString(e));
    }
    *out = im;
    return MGM_OK;
}
int mgm_img_upload(mgm_ctx *c, const float *host, int nx, int ny, int nch, mgm_img **out)
{
    if (!host) return fail(c, MGM_ERR_INVALID, "mgm_img_upload: null host pointer");
    int r = mgm_img_create(c, nx, ny, nch, out);
    if (r) return r;
    hipError_t e = hipMemcpyAsync((*out)->d, host, sizeof(float) * (size_t)nx * ny * nch, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {  // nothing this call created outlives its failure
        r = hipfail(c, e, "mgm_img_upload: copy");
        mgm_img_free(c, *out);
        *out = nullptr;
        return r;
    }
    return MGM_OK;
}
// Refill an existing image from the host (same size): no allocation, what a caller with a stream of same-sized inputs wants.
int mgm_img_update(mgm_ctx *c, mgm_img *im, const float *host)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: a deferred call may still read or write the image)
    if (!c || !im || !host) return fail(c, MGM_ERR_INVALID, "mgm_img_update: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(im->d, host, sizeof(float) * (size_t)im->nx * im->ny * im->nch, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host buffer is the caller's again on return)
    return MGM_OK;
}
int mgm_img_download(mgm_ctx *c, const mgm_img *im, float *host)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !im || !host) return fail(c, MGM_ERR_INVALID, "mgm_img_download: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host, im->d, sizeof(float) * (size_t)im->nx * im->ny * im->nch, hipMemcpyDeviceToHost,
                             c->stream));
    return mgm_ctx_synchronize(c);
}
int mgm_img_dims(const mgm_img *im, int *nx, int *ny, int *nch)
{
    if (!im) return MGM_ERR_INVALID;
    if (nx) *nx = im->nx;
    if (ny) *ny = im->ny;
    if (nch) *nch = im->nch;
    return MGM_OK;
}
void *mgm_img_device_ptr(mgm_img *im) { return im ? im->d : nullptr; }
int mgm_img_device(const mgm_img *im) { return im ? im->device : -1; }
int mgm_img_free(mgm_ctx *c, mgm_img *im)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!im) return MGM_OK;
    if (c) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
    }
    (void)hipFree(im->d);
    delete im;
    return MGM_OK;
}

}  // extern "C"
