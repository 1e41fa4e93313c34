// mgm_pyramid.hip -- the coarse-to-fine (multiscale) driver: its resampling kernels and its C ABI (include/mgm_hip.h).
//
// The reference has no multiscale program, so the DEFINITION is this project's ("multiscale"); it is made of
// reference steps -- update_dmin_dmax (mgm.cc:120-158), everything main() does for a pair -- and three resampling rules that
// are exact in fp32:
//
//   k_zoom_out            out(x,y) = ((a + b) + (c + d)) * 0.25f over the 2x2 block at (2x, 2y), indices clamped
//   k_ranges_zoom_out     lo' = floorf(0.5f * min lo), hi' = ceilf(0.5f * max hi) over the same four pixels
//   k_ranges_from_coarse  U(x,y) = 2.0f * D(x >> 1, y >> 1); update_dmin_dmax(U, lo, hi) + the two
//                         remove_nonfinite_values_Img calls -- FUSED: only the coarse map is read
//
// One thread per output pixel, W*H work: none of this is EXPECTED to show next to the pass kernels (not measured on a device
// yet: docs/experiments.md).  Default floating point
// (NaN-honouring, no contraction).  The driver itself (mgm_multiscale_pair_dev) is host glue over the existing entry points.
#include <climits>
#include <cstddef>

#include "mgm_host.h"

namespace mgm {

__device__ __forceinline__ bool pyr_finite(float x) { return (__builtin_bit_cast(unsigned, x) & 0x7f800000u) != 0x7f800000u; }

__global__ void __launch_bounds__(256) k_fill(float *__restrict__ p, long long n, float value)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = value;
}

__global__ void __launch_bounds__(256) k_zoom_out(const float *__restrict__ in, int nx, int ny, int nch, float *__restrict__ out)
{
    const int ox = (nx + 1) / 2, oy = (ny + 1) / 2;
    const long long onpix = (long long)ox * oy;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= onpix * nch) return;
    const long long p = idx % onpix;
    const int x = (int)(p % ox), y = (int)(p / ox);
    const float *pl = in + (idx / onpix) * (long long)nx * ny;
    const int x0 = 2 * x, y0 = 2 * y;
    const int x1 = x0 + 1 < nx ? x0 + 1 : nx - 1, y1 = y0 + 1 < ny ? y0 + 1 : ny - 1;
    const float a = pl[x0 + (long long)y0 * nx], b = pl[x1 + (long long)y0 * nx];
    const float c = pl[x0 + (long long)y1 * nx], d = pl[x1 + (long long)y1 * nx];
    out[idx] = ((a + b) + (c + d)) * 0.25f;
}

__global__ void __launch_bounds__(256) k_ranges_zoom_out(const float *__restrict__ lo, const float *__restrict__ hi, int nx, int ny,
                                                         float *__restrict__ lo2, float *__restrict__ hi2)
{
    const int ox = (nx + 1) / 2, oy = (ny + 1) / 2;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)ox * oy) return;
    const int x = (int)(idx % ox), y = (int)(idx / ox);
    const int x0 = 2 * x, y0 = 2 * y;
    const int x1 = x0 + 1 < nx ? x0 + 1 : nx - 1, y1 = y0 + 1 < ny ? y0 + 1 : ny - 1;
    const long long q[4] = {x0 + (long long)y0 * nx, x1 + (long long)y0 * nx, x0 + (long long)y1 * nx, x1 + (long long)y1 * nx};
    float a = lo[q[0]], b = hi[q[0]];
    for (int k = 1; k < 4; k++) {
        a = __builtin_fminf(a, lo[q[k]]);
        b = __builtin_fmaxf(b, hi[q[k]]);
    }
    lo2[idx] = __builtin_floorf(0.5f * a);
    hi2[idx] = __builtin_ceilf(0.5f * b);
}

// The integer hull of a block's ranges into hull[0] (min) / hull[1] (max): wave-level butterfly, one LDS step, then ONE
// atomic pair per block.  Every lane of the block must get here (lanes without a pixel pass INT_MAX / INT_MIN).
__device__ __forceinline__ void block_hull(int lo, int hi, int *hull)
{
    __shared__ int s_lo[4], s_hi[4];
    for (int off = 32; off >= 1; off >>= 1) {
        const int l2 = __shfl_xor(lo, off, 64), h2 = __shfl_xor(hi, off, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            lo = s_lo[w] < lo ? s_lo[w] : lo;
            hi = s_hi[w] > hi ? s_hi[w] : hi;
        }
        atomicMin(hull + 0, lo);
        atomicMax(hull + 1, hi);
    }
}
// Dvec's constructor takes the float ranges as ints (mgm_costvolume.h:323): truncation toward zero
__device__ __forceinline__ int range_int(float v) { return (int)v; }

__global__ void k_hull_init(int *hull)
{
    hull[0] = INT_MAX;
    hull[1] = INT_MIN;
}

__global__ void __launch_bounds__(256) k_ranges_hull(const float *__restrict__ lo, const float *__restrict__ hi, long long n, int *hull)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < n;
    block_hull(live ? range_int(lo[idx]) : INT_MAX, live ? range_int(hi[idx]) : INT_MIN, hull);
}

// Fine pixel (i, j): the (2r+1)^2 Neumann-clamped window of U = 2 D(x >> 1, y >> 1) is the RECTANGLE of coarse pixels
// [clamp(i-r) >> 1, clamp(i+r) >> 1] x [clamp(j-r) >> 1, clamp(j+r) >> 1] (consecutive fine columns hit consecutive coarse
// ones), every one of them at least once.  fmin / fmax over a set do not depend on order or multiplicity, and each sample's
// 2d -+ slack is computed as update_dmin_dmax would on the zoomed-in map, so lo / hi are its results bit for bit.
// mm: finite minimum / maximum of the COARSE map (k_minmax); those of U are twice that, exactly.
__global__ void __launch_bounds__(256) k_ranges_from_coarse(const float *__restrict__ coarse, int nx, int ny, int slack, int r,
                                                            const unsigned *__restrict__ mm, float *__restrict__ dminI,
                                                            float *__restrict__ dmaxI, int *hull)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = idx < (long long)nx * ny;
    int ilo = INT_MAX, ihi = INT_MIN;
    if (live) {
        const int cnx = (nx + 1) / 2;
        const int i = (int)(idx % nx), j = (int)(idx / nx);
        const float gmin = 2.0f * ord2f(mm[0]), gmax = 2.0f * ord2f(mm[1]);
        const int x0 = (i - r > 0 ? i - r : 0) >> 1, x1 = (i + r < nx ? i + r : nx - 1) >> 1;
        const int y0 = (j - r > 0 ? j - r : 0) >> 1, y1 = (j + r < ny ? j + r : ny - 1) >> 1;
        float dmin = __builtin_huge_valf(), dmax = -__builtin_huge_valf();
        for (int y = y0; y <= y1; y++)
            for (int x = x0; x <= x1; x++) {
                const float v = 2.0f * coarse[x + (long long)y * cnx];
                const float a = pyr_finite(v) ? v - slack : gmin - slack;
                const float b = pyr_finite(v) ? v + slack : gmax + slack;
                dmin = __builtin_fminf(dmin, a);
                dmax = __builtin_fmaxf(dmax, b);
            }
        float lo = dminI[idx], hi = dmaxI[idx];
        if (pyr_finite(dmin)) {
            lo = dmin;
            hi = dmax;
        }
        // remove_nonfinite_values_Img(dminI, gmin), (dmaxI, gmax)  (mgm.cc:387-388)
        lo = pyr_finite(lo) ? lo : gmin;
        hi = pyr_finite(hi) ? hi : gmax;
        dminI[idx] = lo;
        dmaxI[idx] = hi;
        ilo = range_int(lo);
        ihi = range_int(hi);
    }
    if (hull) block_hull(ilo, ihi, hull);  // (uniform over the launch: no lane diverges around the barrier)
}

static inline unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_fill(float *p, long long n, float value, hipStream_t s)
{
    hipLaunchKernelGGL(k_fill, dim3(blocks_for(n)), dim3(256), 0, s, p, n, value);
    return hipGetLastError();
}
hipError_t launch_zoom_out(const float *in, int nx, int ny, int nch, float *out, hipStream_t s)
{
    const long long n = (long long)((nx + 1) / 2) * ((ny + 1) / 2) * nch;
    hipLaunchKernelGGL(k_zoom_out, dim3(blocks_for(n)), dim3(256), 0, s, in, nx, ny, nch, out);
    return hipGetLastError();
}
hipError_t launch_ranges_zoom_out(const float *lo, const float *hi, int nx, int ny, float *lo2, float *hi2, hipStream_t s)
{
    const long long n = (long long)((nx + 1) / 2) * ((ny + 1) / 2);
    hipLaunchKernelGGL(k_ranges_zoom_out, dim3(blocks_for(n)), dim3(256), 0, s, lo, hi, nx, ny, lo2, hi2);
    return hipGetLastError();
}
hipError_t launch_ranges_from_coarse(const float *coarse, int nx, int ny, int slack, int radius, const unsigned *mm, float *lo,
                                     float *hi, int *hull, hipStream_t s)
{
    const long long n = (long long)nx * ny;
    if (slack < 0) slack = -slack;  // mgm.cc:130
    if (hull) hipLaunchKernelGGL(k_hull_init, dim3(1), dim3(1), 0, s, hull);
    hipLaunchKernelGGL(k_ranges_from_coarse, dim3(blocks_for(n)), dim3(256), 0, s, coarse, nx, ny, slack, radius, mm, lo, hi, hull);
    return hipGetLastError();
}
hipError_t launch_ranges_hull(const float *lo, const float *hi, long long n, int *hull, hipStream_t s)
{
    hipLaunchKernelGGL(k_hull_init, dim3(1), dim3(1), 0, s, hull);
    hipLaunchKernelGGL(k_ranges_hull, dim3(blocks_for(n)), dim3(256), 0, s, lo, hi, n, hull);
    return hipGetLastError();
}

}  // namespace mgm

// ---- host side ----------------------------------------------------------------------------------------------------------
// The four control words this unit owns (kWordPyr, mgm_host.h): the finite minimum / maximum of a coarse map and the
// integer hull.  No pass launch addresses them.
static unsigned *pyr_mm(mgm_ctx *c) { return ctrl_word(c, kWordPyr); }
static int *pyr_hull(mgm_ctx *c) { return (int *)ctrl_word(c, kWordPyr) + 2; }

static int read_hull(mgm_ctx *c, int *hull_min, int *hull_max)
{
    int h[2];
    HIPCHK(c, hipMemcpyAsync(h, pyr_hull(c), sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *hull_min = h[0];
    *hull_max = h[1];
    return MGM_OK;
}

// *out NULL: a new image; else it must have that size
static int out_image(mgm_ctx *c, const char *who, int nx, int ny, int nch, mgm_img **out, bool *created)
{
    *created = false;
    if (*out) {
        if ((*out)->nx != nx || (*out)->ny != ny || (*out)->nch != nch)
            return fail(c, MGM_ERR_INVALID, std::string(who) + ": the output image is non-NULL but has another size");
        return MGM_OK;
    }
    *created = true;
    return mgm_img_create(c, nx, ny, nch, out);
}

extern "C" {

int mgm_multiscale_levels(int nx, int ny, int vnx, int vny, int nscales, int *dims)
{
    if (nx < 1 || ny < 1 || vnx < 1 || vny < 1 || nscales < 1 || nscales > 8) return -MGM_ERR_INVALID;
    int d[4] = {nx, ny, vnx, vny}, S = 0;
    for (int s = 0; s < nscales; s++) {
        if (s > 0) {
            int e[4];
            for (int k = 0; k < 4; k++) e[k] = (d[k] + 1) / 2;
            if (std::min(std::min(e[0], e[1]), std::min(e[2], e[3])) < 16) break;
            for (int k = 0; k < 4; k++) d[k] = e[k];
        }
        if (dims)
            for (int k = 0; k < 4; k++) dims[4 * s + k] = d[k];
        S = s + 1;
    }
    return S;
}

int mgm_zoom_out_dev(mgm_ctx *c, const mgm_img *in, mgm_img **out)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !in || !out || in == *out) return fail(c, MGM_ERR_INVALID, "mgm_zoom_out: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    bool created;
    if (int r = out_image(c, "mgm_zoom_out", (in->nx + 1) / 2, (in->ny + 1) / 2, in->nch, out, &created)) return r;
    TimeScope t(c, "k_zoom_out");
    const hipError_t e = launch_zoom_out(in->d, in->nx, in->ny, in->nch, (*out)->d, c->stream);
    if (e != hipSuccess) {
        const int r = hipfail(c, e, "k_zoom_out");
        if (created) {
            mgm_img_free(c, *out);
            *out = nullptr;
        }
        return r;
    }
    return MGM_OK;
}

int mgm_ranges_zoom_out_dev(mgm_ctx *c, const mgm_img *lo, const mgm_img *hi, mgm_img **lo2, mgm_img **hi2)
{
    if (int jr = pipe_join(c)) return jr;
    if (!c || !lo || !hi || !lo2 || !hi2 || lo2 == hi2 || (*lo2 && *lo2 == *hi2)) return fail(c, MGM_ERR_INVALID, "mgm_ranges_zoom_out: bad arguments");
    if (lo->nx != hi->nx || lo->ny != hi->ny || lo->nch != 1 || hi->nch != 1)
        return fail(c, MGM_ERR_INVALID, "mgm_ranges_zoom_out: lo and hi must be one-channel images of one size");
    HIPCHK(c, hipSetDevice(c->device));
    const int ox = (lo->nx + 1) / 2, oy = (lo->ny + 1) / 2;
    bool made_lo = false, made_hi = false;
    int r = out_image(c, "mgm_ranges_zoom_out", ox, oy, 1, lo2, &made_lo);
    if (!r && (r = out_image(c, "mgm_ranges_zoom_out", ox, oy, 1, hi2, &made_hi))) made_hi = false;
    if (!r) {
        TimeScope t(c, "k_ranges_zoom_out");
        const hipError_t e = launch_ranges_zoom_out(lo->d, hi->d, lo->nx, lo->ny, (*lo2)->d, (*hi2)->d, c->stream);
        if (e != hipSuccess) r = hipfail(c, e, "k_ranges_zoom_out");
    }
    if (r) {  // hand out nothing this call created
        const std::string msg = c->err;
        if (made_lo && *lo2) mgm_img_free(c, *lo2), *lo2 = nullptr;
        if (made_hi && *hi2) mgm_img_free(c, *hi2), *hi2 = nullptr;
        c->err = msg;
    }
    return r;
}

int mgm_ranges_from_coarse_dev(mgm_ctx *c, const mgm_img *coarse, mgm_img *lo, mgm_img *hi, int slack, int radius, int *hull_min,
                               int *hull_max)
{
    if (int jr = pipe_join(c)) return jr;
    if (!c || !coarse || !lo || !hi || lo == hi) return fail(c, MGM_ERR_INVALID, "mgm_ranges_from_coarse: null argument");
    if ((hull_min == nullptr) != (hull_max == nullptr)) return fail(c, MGM_ERR_INVALID, "mgm_ranges_from_coarse: hull_min and hull_max go together");
    if (lo->nx != hi->nx || lo->ny != hi->ny || lo->nch != 1 || hi->nch != 1)
        return fail(c, MGM_ERR_INVALID, "mgm_ranges_from_coarse: lo and hi must be one-channel images of one size");
    if (coarse->nch != 1 || coarse->nx != (lo->nx + 1) / 2 || coarse->ny != (lo->ny + 1) / 2)
        return fail(c, MGM_ERR_INVALID, "mgm_ranges_from_coarse: the coarse map must be ((nx+1)/2, (ny+1)/2) for nx*ny ranges");
    if (radius < 0 || radius > 16) return fail(c, MGM_ERR_INVALID, "mgm_ranges_from_coarse: radius must be 0..16");
    HIPCHK(c, hipSetDevice(c->device));
    if (int r = ensure_words(c)) return r;
    {
        TimeScope t(c, "k_minmax");
        HIPCHK(c, launch_minmax(coarse->d, (long long)coarse->nx * coarse->ny, pyr_mm(c), c->stream));
    }
    {
        TimeScope t(c, "k_ranges_from_coarse");
        HIPCHK(c, launch_ranges_from_coarse(coarse->d, lo->nx, lo->ny, slack, radius, pyr_mm(c), lo->d, hi->d, hull_min ? pyr_hull(c) : nullptr,
                                            c->stream));
    }
    return hull_min ? read_hull(c, hull_min, hull_max) : MGM_OK;
}

}  // extern "C"

// ---- the driver -----------------------------------------------------------------------------------------------------------
namespace {

// Everything the driver allocates, freed in one place whatever the way out.
struct MsState {
    mgm_ctx *c;
    std::vector<mgm_img *> u, v;           // [s]; [0] are the caller's
    std::vector<mgm_img *> blo[2], bhi[2];  // base ranges per run [s] (null: uniform run -- no images needed at that level)
    mgm_img *prev[2] = {nullptr, nullptr};  // the coarser level's final maps
    // the current level
    mgm_img *lo[2] = {}, *hi[2] = {}, *w[2] = {}, *out[2] = {}, *cost[2] = {}, *spare[2] = {}, *ilo = nullptr, *ihi = nullptr, *votes = nullptr;
    mgm_cv *C[2] = {};
    explicit MsState(mgm_ctx *ctx) : c(ctx) {}
    void free_level(bool keep_out)
    {
        for (int k = 0; k < 2; k++) {
            mgm_cv_free(c, C[k]);
            C[k] = nullptr;
            for (mgm_img **im : {&lo[k], &hi[k], &w[k], &cost[k], &spare[k]}) {
                mgm_img_free(c, *im);
                *im = nullptr;
            }
            if (!keep_out) {
                mgm_img_free(c, out[k]);
                out[k] = nullptr;
            }
        }
        for (mgm_img **im : {&ilo, &ihi, &votes}) {
            mgm_img_free(c, *im);
            *im = nullptr;
        }
    }
    ~MsState()
    {
        const std::string msg = c->err;  // (the frees synchronise and may touch the message)
        free_level(false);
        for (int k = 0; k < 2; k++) {
            mgm_img_free(c, prev[k]);
            for (auto *vec : {&blo[k], &bhi[k]})
                for (size_t s = 0; s < vec->size(); s++) mgm_img_free(c, (*vec)[s]);
        }
        for (auto *vec : {&u, &v})
            for (size_t s = 1; s < vec->size(); s++) mgm_img_free(c, (*vec)[s]);
        c->err = msg;
    }
};

int new_filled(mgm_ctx *c, int nx, int ny, float value, mgm_img **out)
{
    if (int r = mgm_img_create(c, nx, ny, 1, out)) return r;
    HIPCHK(c, launch_fill((*out)->d, (long long)nx * ny, value, c->stream));
    return MGM_OK;
}
int copy_image(mgm_ctx *c, const mgm_img *src, mgm_img *dst)
{
    HIPCHK(c, hipMemcpyAsync(dst->d, src->d, sizeof(float) * (size_t)src->nx * src->ny * src->nch, hipMemcpyDeviceToDevice, c->stream));
    return MGM_OK;
}
int clone_image(mgm_ctx *c, const mgm_img *src, mgm_img **out)
{
    if (int r = mgm_img_create(c, src->nx, src->ny, src->nch, out)) return r;
    return copy_image(c, src, *out);
}

int ms_run(mgm_ctx *c, const mgm_img *u0, const mgm_img *v0, const mgm_ms_params &p, mgm_img *outL, mgm_img *costL, mgm_img *outR,
           mgm_img *costR, mgm_img *nolr)
{
    int r;
    int dims[8][4];
    const int S = mgm_multiscale_levels(u0->nx, u0->ny, v0->nx, v0->ny, p.nscales, &dims[0][0]);
    const int nrun = p.testlrrl ? 2 : 1;
    const bool given = p.lo != nullptr;
    const bool weighted = p.aP2 != 1.0f;
    MsState st(c);
    // ---- the pyramids: images, and the base ranges of each run (uniform ranges stay two numbers per level) ----
    st.u.assign(S, nullptr);
    st.v.assign(S, nullptr);
    st.u[0] = const_cast<mgm_img *>(u0);
    st.v[0] = const_cast<mgm_img *>(v0);
    for (int s = 1; s < S; s++) {
        if ((r = mgm_zoom_out_dev(c, st.u[s - 1], &st.u[s])) || (r = mgm_zoom_out_dev(c, st.v[s - 1], &st.v[s]))) return r;
    }
    float ulo[2][8], uhi[2][8];  // the uniform base range of run k at level s: the zoom-out rule applied to a constant
    ulo[0][0] = (float)p.dmin, uhi[0][0] = (float)p.dmax;
    ulo[1][0] = (float)-p.dmax, uhi[1][0] = (float)-p.dmin;  // mgm.cc:368
    for (int k = 0; k < 2; k++)
        for (int s = 1; s < S; s++) ulo[k][s] = floorf(0.5f * ulo[k][s - 1]), uhi[k][s] = ceilf(0.5f * uhi[k][s - 1]);
    if (given) {
        st.blo[0].assign(S, nullptr);
        st.bhi[0].assign(S, nullptr);
        // ([0] stays null: level 0's base ranges are the caller's images, read only -- every level works on its own copy)
        for (int s = 1; s < S; s++)
            if ((r = mgm_ranges_zoom_out_dev(c, s == 1 ? p.lo : st.blo[0][s - 1], s == 1 ? p.hi : st.bhi[0][s - 1], &st.blo[0][s], &st.bhi[0][s]))) return r;
    }
    if (p.levels_run) *p.levels_run = S;

    for (int s = S - 1; s >= 0; s--) {
        const bool finest = s == 0, coarsest = s == S - 1;
        const mgm_img *U[2] = {st.u[s], st.v[s]}, *V[2] = {st.v[s], st.u[s]};
        mgm_ms_level info{};
        info.nx = dims[s][0], info.ny = dims[s][1], info.vnx = dims[s][2], info.vny = dims[s][3];
        bool ranged[2] = {false, false};
        int hmin[2] = {0, 0}, hmax[2] = {0, 0};
        for (int k = 0; k < nrun; k++) {
            const int nx = U[k]->nx, ny = U[k]->ny;
            const bool has_base = k == 0 && given;
            ranged[k] = has_base || !coarsest;
            hmin[k] = (int)ulo[k][s];
            hmax[k] = (int)uhi[k][s];
            if (ranged[k]) {
                if (has_base) {
                    if ((r = clone_image(c, s == 0 ? p.lo : st.blo[0][s], &st.lo[k])) || (r = clone_image(c, s == 0 ? p.hi : st.bhi[0][s], &st.hi[k]))) return r;
                } else if ((r = new_filled(c, nx, ny, ulo[k][s], &st.lo[k])) || (r = new_filled(c, nx, ny, uhi[k][s], &st.hi[k])))
                    return r;
                if (!coarsest) {
                    if ((r = mgm_ranges_from_coarse_dev(c, st.prev[k], st.lo[k], st.hi[k], p.slack, p.radius, &hmin[k], &hmax[k]))) return r;
                } else {
                    if ((r = ensure_words(c))) return r;
                    TimeScope t(c, "k_ranges_hull");
                    HIPCHK(c, launch_ranges_hull(st.lo[k]->d, st.hi[k]->d, (long long)nx * ny, pyr_hull(c), c->stream));
                    if ((r = read_hull(c, &hmin[k], &hmax[k]))) return r;
                }
            }
        }
        // the two runs can share a launch when their volumes have one size and one label count (a wider hull than the ranges
        // need is legal: the labels nobody owns read +INF); under FH ragged volumes must also share hull_min
        for (int k = 0; k < nrun; k++) info.hull_min[k] = hmin[k], info.hull_max[k] = hmax[k];  // (reported: the hull of the RANGES, before any widening)
        bool together = nrun == 2 && p.iterations > 0 && U[0]->nx == U[1]->nx && U[0]->ny == U[1]->ny;
        if (together && (ranged[0] || ranged[1])) {
            const int L0 = hmax[0] - hmin[0] + 1, L1 = hmax[1] - hmin[1] + 1;
            const int shorter = L0 < L1 ? 0 : 1;
            if (p.use_fh > 0 && hmin[0] != hmin[1]) together = false;
            else if (L0 != L1 && !ranged[shorter]) together = false;  // (a uniform volume's labels are all real: its range is not ours to widen)
            else hmax[shorter] += std::abs(L0 - L1);
        }
        for (int k = 0; k < nrun; k++) {
            const int nx = U[k]->nx, ny = U[k]->ny;
            if (weighted) {
                if ((r = mgm_weights_dev(c, U[k], p.aP2, p.aThresh, &st.w[k]))) return r;
                bool odd = false, any = false;
                const mgm_img *w1[1] = {st.w[k]};
                if ((r = weights_have_odd_values(c, w1, 1, (long long)nx * ny, &odd, &any))) return r;
                info.weighted[k] = any;
            }
            if (ranged[k])
                r = mgm_costvolume_build_ranged_dev(c, U[k], V[k], st.lo[k], st.hi[k], hmin[k], hmax[k], p.prefilter, p.distance, p.truncDist,
                                                    p.census_win, &st.C[k]);
            else
                r = mgm_costvolume_build_dev(c, U[k], V[k], hmin[k], hmax[k], p.prefilter, p.distance, p.truncDist, p.census_win, &st.C[k]);
            if (r) return r;
            // the finest level writes the caller's images
            mgm_img *fo = k == 0 ? outL : outR, *fc = k == 0 ? costL : costR;
            if (finest && fo) st.out[k] = nullptr;
            if (!(finest && fo) && (r = mgm_img_create(c, nx, ny, 1, &st.out[k]))) return r;
            if (!(finest && fc) && (r = mgm_img_create(c, nx, ny, 1, &st.cost[k]))) return r;
        }
        mgm_img *O[2], *K[2];
        for (int k = 0; k < nrun; k++) {
            O[k] = st.out[k] ? st.out[k] : (k == 0 ? outL : outR);
            K[k] = st.cost[k] ? st.cost[k] : (k == 0 ? costL : costR);
        }
        if (p.iterations == 0)
            for (int k = 0; k < nrun; k++) {  // mgm() is never called: the maps keep their zeros (mgm.cc:360-365)
                HIPCHK(c, launch_fill(O[k]->d, (long long)O[k]->nx * O[k]->ny, 0.0f, c->stream));
                HIPCHK(c, launch_fill(K[k]->d, (long long)K[k]->nx * K[k]->ny, 0.0f, c->stream));
            }
        if (together) {
            const mgm_cv *Cs[2] = {st.C[0], st.C[1]};
            const mgm_img *Ws[2] = {st.w[0], st.w[1]};
            r = mgm_aggregate_batch_dev(c, 2, Cs, weighted ? Ws : nullptr, p.P1, p.P2, p.NDIR, p.TSGM, p.use_fh, p.fix_overcount, p.refine, O, K, nullptr);
            if (r == MGM_ERR_NOMEM || r == MGM_ERR_UNSUPPORTED) {  // (no room for 2 NDIR Lr volumes; one run weighted, the other not)
                together = false;
                (void)hipGetLastError();
                c->err.clear();
            } else if (r)
                return r;
        }
        info.batched = together;
        for (int k = 0; k < nrun && p.iterations > 0; k++) {
            if (!together &&
                (r = mgm_aggregate_dev(c, st.C[k], st.w[k], p.P1, p.P2, p.NDIR, p.TSGM, p.use_fh, p.fix_overcount, p.refine, O[k], K[k], nullptr)))
                return r;
            if (p.iterations > 1) {  // mgm.cc:377-388: the ranges narrow around the solution, the volume -- and every pass -- stays
                const int nx = U[k]->nx, ny = U[k]->ny;
                if (ranged[k]) {
                    if ((r = clone_image(c, st.lo[k], &st.ilo)) || (r = clone_image(c, st.hi[k], &st.ihi))) return r;
                } else if ((r = new_filled(c, nx, ny, ulo[k][s], &st.ilo)) || (r = new_filled(c, nx, ny, uhi[k][s], &st.ihi)))
                    return r;
                for (int it = 1; it < p.iterations; it++) {
                    if ((r = mgm_update_ranges_dev(c, O[k], st.ilo, st.ihi, 3, 2))) return r;
                    if ((r = mgm_wta_windowed_dev(c, st.C[k], p.NDIR, p.fix_overcount, p.refine, st.ilo, st.ihi, O[k], K[k]))) return r;
                }
                mgm_img_free(c, st.ilo);
                mgm_img_free(c, st.ihi);
                st.ilo = st.ihi = nullptr;
            }
            // the consensus votes: the finest level only, on the run's map as its search, refinement and iterations left
            // it; the aggregation the context holds is this run's (or the launch both runs shared)
            if (finest && (p.consensus_min > 0 || (k == 0 && p.votesL))) {
                mgm_img *vt = (k == 0 && p.votesL) ? p.votesL : nullptr;
                if (!vt && (r = mgm_img_create(c, O[k]->nx, O[k]->ny, 1, &st.votes))) return r;
                if ((r = mgm_wta_consensus_dev(c, st.C[k], p.NDIR, O[k], p.consensus_tol, vt ? vt : st.votes, nullptr))) return r;
                if (p.consensus_min > 0 && (r = mgm_consensus_filter_dev(c, O[k], vt ? vt : st.votes, p.consensus_min, O[k]))) return r;
                mgm_img_free(c, st.votes);
                st.votes = nullptr;
            }
        }
        if (finest && p.iterations == 0 && p.votesL) HIPCHK(c, launch_fill(p.votesL->d, (long long)p.votesL->nx * p.votesL->ny, 0.0f, c->stream));
        // MEDIAN, the map before the left-right test, the two tests on copies of the unchecked maps (mgm.cc:396-423)
        for (int k = 0; k < nrun; k++) {
            if (p.median != 0 || nrun == 2)
                if ((r = mgm_img_create(c, O[k]->nx, O[k]->ny, 1, &st.spare[k]))) return r;
            if (p.median != 0) {
                if ((r = mgm_median_dev(c, O[k], p.median, st.spare[k])) || (r = copy_image(c, st.spare[k], O[k]))) return r;
            }
        }
        if (finest && nolr && (r = copy_image(c, O[0], nolr))) return r;
        if (finest && nrun == 2 && p.outR_nolr && (r = copy_image(c, O[1], p.outR_nolr))) return r;
        if (nrun == 2) {
            if ((r = mgm_leftright_dev(c, O[1], O[0], p.tau, st.spare[1])) || (r = mgm_leftright_dev(c, O[0], O[1], p.tau, st.spare[0]))) return r;
            for (int k = 0; k < 2; k++)
                if ((r = copy_image(c, st.spare[k], O[k]))) return r;
        }
        if (p.levels) p.levels[s] = info;
        // this level's maps are the next one's priors
        for (int k = 0; k < 2; k++) {
            mgm_img_free(c, st.prev[k]);
            st.prev[k] = st.out[k];
            st.out[k] = nullptr;
        }
        st.free_level(true);
    }
    return MGM_OK;
}

}  // namespace

extern "C" int mgm_multiscale_pair_dev(mgm_ctx *c, const mgm_img *u, const mgm_img *v, const mgm_ms_params *pp, mgm_img *outL, mgm_img *costL,
                                       mgm_img *outR, mgm_img *costR, mgm_img *outL_nolr)
{
    if (int jr = pipe_join(c)) return jr;  // (pipelined context: run what has been deferred first)
    if (!c || !u || !v || !pp || !outL || !costL) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: null argument");
    if (pp->struct_size < offsetof(mgm_ms_params, levels_run)) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: struct_size is smaller than the first version of mgm_ms_params");
    mgm_ms_params p{};
    memcpy(&p, pp, std::min<size_t>(pp->struct_size, sizeof p));  // (fields beyond the caller's struct: zero = absent)
    if (p.nscales < 1 || p.nscales > 8) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: nscales must be 1..8");
    if (c->pipe_depth > 1) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: not on a pipelined context (every level needs the one before)");
    if (p.radius < 0 || p.radius > 16) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: radius must be 0..16");
    if (p.iterations < 0 || p.median < 0) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: iterations and median must be >= 0");
    if (u->nch != v->nch) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: channel counts differ");
    if ((p.lo == nullptr) != (p.hi == nullptr)) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: lo and hi go together");
    for (const mgm_img *im : {p.lo, p.hi})
        if (im && (im->nx != u->nx || im->ny != u->ny || im->nch != 1))
            return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: the range images must have the left image's size");
    for (const mgm_img *im : {(const mgm_img *)outL, (const mgm_img *)costL, (const mgm_img *)outL_nolr})
        if (im && (im->nx != u->nx || im->ny != u->ny || im->nch != 1))
            return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: outL / costL / outL_nolr must be nx*ny");
    for (const mgm_img *im : {(const mgm_img *)outR, (const mgm_img *)costR})
        if (im && (im->nx != v->nx || im->ny != v->ny || im->nch != 1))
            return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: outR / costR must have the right image's size");
    if (p.outR_nolr && (p.outR_nolr->nx != v->nx || p.outR_nolr->ny != v->ny || p.outR_nolr->nch != 1))
        return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: outR_nolr must have the right image's size");
    if (p.consensus_min < 0) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: consensus_min must be >= 0");
    if ((p.consensus_min > 0 || p.votesL) && (!(p.consensus_tol >= 0.0f) || !std::isfinite(p.consensus_tol)))
        return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: consensus_tol must be finite and >= 0");
    if (p.votesL && (p.votesL->nx != u->nx || p.votesL->ny != u->ny || p.votesL->nch != 1))
        return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: votesL must be nx*ny");
    {
        const mgm_img *outs[7] = {outL, costL, outR, costR, outL_nolr, p.outR_nolr, p.votesL};
        for (int a = 0; a < 7; a++)
            for (int b = a + 1; b < 7; b++)
                if (outs[a] && outs[a] == outs[b]) return fail(c, MGM_ERR_INVALID, "mgm_multiscale_pair: the output images must be different images");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const int r = ms_run(c, u, v, p, outL, costL, p.testlrrl ? outR : nullptr, p.testlrrl ? costR : nullptr, outL_nolr);
    if (r != MGM_OK) {  // leave the context usable: nothing of the failed pair is still in flight
        const std::string msg = c->err;
        (void)hipStreamSynchronize(c->stream);
        c->err = msg;
    }
    return r;
}
