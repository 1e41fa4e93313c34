// mgm_subpix.hip -- sub-pixel label spacing: half- and quarter-pixel cost volumes.
//   k_subpix_phase   the phase image v_k of v at the shift t = k/s, element-wise: linear or Keys' cubic (a = -1/2) along x, column
//                    indices clamped, every product rounded and the sums in the written order (the unit is built without contraction)
//   k_cv_interleave  the fine volume F(p, o') = C_{o' mod s}(p, o' div s), gathered from the s phase volumes: each workgroup writes
//                    the rows of plan_subpix's `pix` consecutive pixels, one contiguous span, as aligned 16-byte stores
//   k_scale_map      out = in / s (exact; reads before it writes: out may be in)
// No atomics, no waiting loop: every output has one writer.
#include "mgm_device.h"
#include "mgm_planner.h"

namespace mgm {

static_assert(kSubpixMaxLabels == kMaxLabels, "plan_subpix admits the label counts mgm_cv_create admits");

// Keys' weights at t = 1/4, 1/2, 3/4 (all exact in fp32): w0 v(x-1) + w1 v(x) + w2 v(x+1) + w3 v(x+2)
struct PhaseWeights { float w0, w1, w2, w3; };

__global__ void __launch_bounds__(256) k_subpix_phase(const float *__restrict__ v, int vnx, long long n, int cubic, PhaseWeights w,
                                                      float *__restrict__ out)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int x = (int)(idx % vnx);
    const float *row = v + (idx - x);
    const int last = vnx - 1;
    const float b = row[x], c = row[x + 1 < last ? x + 1 : last];
    float r;
    if (cubic) {
        const float a = row[x > 0 ? x - 1 : 0], d = row[x + 2 < last ? x + 2 : last];
        r = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w.w0, a), __fmul_rn(w.w1, b)), __fmul_rn(w.w2, c)), __fmul_rn(w.w3, d));
    } else {
        r = __fadd_rn(__fmul_rn(w.w1, b), __fmul_rn(w.w2, c));  // (1 - t) v(x) + t v(x + 1)
    }
    out[idx] = r;
}

hipError_t launch_subpix_phase(const float *v, int vnx, long long nrows, int s, int k, int interp, float *out, hipStream_t st)
{
    if ((s != 2 && s != 4) || k < 1 || k >= s || vnx < 1 || nrows < 1) return hipErrorInvalidValue;
    const int q = k * (4 / s);  // quarters: 1, 2, 3
    PhaseWeights w;
    if (interp == kSubpixCubic) {
        static const PhaseWeights keys[3] = {{-9.0f / 128, 111.0f / 128, 29.0f / 128, -3.0f / 128},
                                             {-1.0f / 16, 9.0f / 16, 9.0f / 16, -1.0f / 16},
                                             {-3.0f / 128, 29.0f / 128, 111.0f / 128, -9.0f / 128}};
        w = keys[q - 1];
    } else {
        const float t = 0.25f * (float)q;
        w = PhaseWeights{0.0f, 1.0f - t, t, 0.0f};
    }
    const long long n = nrows * vnx;
    const long long grid = (n + 255) / 256;
    if (grid > 2147483647ll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_subpix_phase, dim3((unsigned)grid), dim3(256), 0, st, v, vnx, n, interp == kSubpixCubic ? 1 : 0, w, out);
    return hipGetLastError();
}

template <int S, class T>
struct PhasePtrs { const T *p[S]; };
template <int S, class T>
__device__ __forceinline__ const T *phase_of(const PhasePtrs<S, T> &ph, unsigned k)  // (selects, not an indexed read of the arguments)
{
    const T *r = ph.p[0];
#pragma unroll
    for (int j = 1; j < S; j++) r = k == (unsigned)j ? ph.p[j] : r;
    return r;
}

// One-byte codes.  A chunk is 16 consecutive label slots of one pixel's row of F: 16 / S codes of each phase, one aligned load per
// phase (rows are multiples of 64 bytes), interleaved in registers; the slots from `labels` on get 255, the code of +INF -- which
// also covers the dropped last label of the phases k > 0 and whatever the phases' own padding holds.
template <int S>
__global__ void __launch_bounds__(kSubpixThreads) k_cv_interleave_codes(PhasePtrs<S, uint8_t> ph, uint8_t *__restrict__ F, long long npix, int labels,
                                                                        int slots, int in_slots, int pix)
{
    constexpr int W = 16 / S;  // codes per phase and chunk: 8 or 4
    const long long p0 = (long long)blockIdx.x * pix;
    const long long left = npix - p0;
    const unsigned npl = (unsigned)(left < pix ? left : pix);
    const unsigned cpp = (unsigned)slots / 16u;  // chunks per pixel
    const unsigned n = npl * cpp;
    for (unsigned j = threadIdx.x; j < n; j += kSubpixThreads) {
        const unsigned pl = j / cpp, ch = j - pl * cpp;
        const unsigned o0 = ch * 16u, i0 = o0 / S;
        const size_t row = (size_t)(p0 + pl) * (size_t)in_slots + i0;
        unsigned in[S][W / 4];
        const bool inside = i0 + W <= (unsigned)in_slots;
#pragma unroll
        for (int k = 0; k < S; k++)
#pragma unroll
            for (int q = 0; q < W / 4; q++) in[k][q] = inside ? reinterpret_cast<const unsigned *>(ph.p[k] + row)[q] : 0xffffffffu;
        unsigned o[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            unsigned word = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int e = 4 * q + b;  // slot o0 + e: phase e % S, its code e / S of this chunk
                const unsigned code = (in[e % S][(e / S) / 4] >> (8 * ((e / S) % 4))) & 0xffu;
                word |= (o0 + e < (unsigned)labels ? code : 255u) << (8 * b);
            }
            o[q] = word;
        }
        *reinterpret_cast<uint4 *>(F + (size_t)(p0 + pl) * (size_t)slots + o0) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

// fp32.  Rows have `labels` floats, any count: the chunks are four consecutive floats of the workgroup's span (which starts 16-byte
// aligned: pix is a multiple of four), so a chunk may run from one pixel's row into the next.
template <int S>
__global__ void __launch_bounds__(kSubpixThreads) k_cv_interleave_floats(PhasePtrs<S, float> ph, float *__restrict__ F, long long npix, int labels, int in_slots,
                                                                         int pix)
{
    const long long p0 = (long long)blockIdx.x * pix;
    const long long left = npix - p0;
    const unsigned npl = (unsigned)(left < pix ? left : pix);
    const unsigned n = npl * (unsigned)labels;
    float *dst = F + (size_t)p0 * (size_t)labels;
    for (unsigned e0 = threadIdx.x * 4u; e0 < n; e0 += kSubpixThreads * 4u) {
        unsigned pl = e0 / (unsigned)labels, o = e0 - pl * (unsigned)labels;
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (e0 + k < n) {
                r[k] = phase_of<S, float>(ph, o % S)[(size_t)(p0 + pl) * (size_t)in_slots + o / S];
                if (++o == (unsigned)labels) o = 0, pl++;
            }
        }
        if (e0 + 4u <= n) {
            *reinterpret_cast<float4 *>(dst + e0) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (e0 + k < n) dst[e0 + k] = r[k];
        }
    }
}

template <int S>
static hipError_t launch_interleave_s(const SubpixParams &p, const SubpixChoice &c, hipStream_t st)
{
    if (c.family == kSubpixCodes) {
        PhasePtrs<S, uint8_t> ph;
        for (int k = 0; k < S; k++) ph.p[k] = (const uint8_t *)p.phase[k];
        hipLaunchKernelGGL(k_cv_interleave_codes<S>, dim3((unsigned)c.grid), dim3(kSubpixThreads), 0, st, ph, (uint8_t *)p.F, p.npix, p.labels, p.slots,
                           p.in_slots, c.pix);
    } else {
        PhasePtrs<S, float> ph;
        for (int k = 0; k < S; k++) ph.p[k] = (const float *)p.phase[k];
        hipLaunchKernelGGL(k_cv_interleave_floats<S>, dim3((unsigned)c.grid), dim3(kSubpixThreads), 0, st, ph, (float *)p.F, p.npix, p.labels, p.in_slots,
                           c.pix);
    }
    return hipGetLastError();
}

hipError_t launch_cv_interleave(const SubpixParams &p, const SubpixChoice &c, hipStream_t st)
{
    // the choice must be the plan of these parameters: the kernels index by it
    const SubpixChoice want = plan_subpix(SubpixRequest{p.npix, p.labels, p.slots, p.in_slots, p.s, p.cb, 0});
    if (want.family == kSubpixRefuse || want.family != c.family || want.pix != c.pix || want.grid != c.grid || !p.F) return hipErrorInvalidValue;
    for (int k = 0; k < p.s; k++)
        if (!p.phase[k]) return hipErrorInvalidValue;
    return p.s == 2 ? launch_interleave_s<2>(p, c, st) : launch_interleave_s<4>(p, c, st);
}

__global__ void __launch_bounds__(256) k_scale_map(const float *in, long long n, float s, float *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[i];
    out[i] = x / s;
}

hipError_t launch_scale_map(const float *in, long long n, int s, float *out, hipStream_t st)
{
    const long long grid = (n + 255) / 256;
    if (n < 1 || grid > 2147483647ll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scale_map, dim3((unsigned)grid), dim3(256), 0, st, in, n, (float)s, out);
    return hipGetLastError();
}

}  // namespace mgm
