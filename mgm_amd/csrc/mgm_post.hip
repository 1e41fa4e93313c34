// mgm_post.hip -- the steps main() applies to the disparity maps right after the path:
//
//   median_filter      img_tools.h:203-238   NaN-aware, window clipped at the border, upper median v[n/2]
//                                            (of the total order: -0 below +0, in both kernels -- DESIGN section 1)
//   leftright_test     mgm.cc:68-91          |x - (Lx + R[Lx])| > tau, or Lx outside the other image  =>  NaN
//   back-projection    mgm.cc:433-443        v sampled at x + d (the reference's float index arithmetic), else u
//   update_dmin_dmax   mgm.cc:120-158        the ranges of the next TSGM_ITER iteration around the current map (k_minmax, k_update_ranges)
//   uniqueness                 conf = 1 - cost1 / cost2 from the runner-up search, conf < ratio  =>  NaN
//
// One thread per pixel; W*H work, nothing here is hot.  Default floating point (NaN-honouring).
#include "mgm_device.h"

namespace mgm {

// The reference gathers the non-NaN samples of the window and takes nth_element(n/2).  Selection without a
// sort: the k-th smallest is the sample with (#smaller) <= k < (#smaller + #equal).
__global__ void __launch_bounds__(256) k_median(const float *__restrict__ u, int nx, int ny, int nch, int radius,
                                                float *__restrict__ out)
{
    const long long npix = (long long)nx * ny;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= npix * nch) return;
    const long long p = idx % npix;
    const int x = (int)(p % nx), y = (int)(p / nx);
    const float *pl = u + (idx / npix) * npix;
    const int x0 = x - radius < 0 ? 0 : x - radius, x1 = x + radius >= nx ? nx - 1 : x + radius;
    const int y0 = y - radius < 0 ? 0 : y - radius, y1 = y + radius >= ny ? ny - 1 : y + radius;
    int n = 0, below = 0;  // samples; samples that order before +0 (the negative ones and the negative zeros)
    for (int j = y0; j <= y1; j++)
        for (int i = x0; i <= x1; i++) {
            const float s = pl[i + (long long)j * nx];
            n += (s == s);
            below += (s < 0.0f) || (__builtin_bit_cast(unsigned, s) == 0x80000000u);
        }
    float res = pl[p];  // an all-NaN window leaves the pixel as it is
    if (n > 0) {
        const int k = n / 2;
        for (int j = y0; j <= y1; j++)
            for (int i = x0; i <= x1; i++) {
                const float s = pl[i + (long long)j * nx];
                if (!(s == s)) continue;
                int less = 0, equal = 0;
                for (int jj = y0; jj <= y1; jj++)
                    for (int ii = x0; ii <= x1; ii++) {
                        const float t = pl[ii + (long long)jj * nx];
                        less += (t < s);
                        equal += (t == s);
                    }
                if (less <= k && k < less + equal) res = s;
            }
        // `t == s` counts both zeros as one value and keeps whichever was met last.  The rule is the total order, -0 below
        // +0 (what k_median_big's keys give): rank k is a negative zero iff it lies below (#negative samples) + (#negative zeros),
        // which the sweep that counted the samples has counted too (no further sweep: docs/experiments.md).
        if (res == 0.0f) res = k < below ? -0.0f : 0.0f;
    }
    out[idx] = res;
}

// Large windows (radius > 7: the kernel above is O(w^4) per pixel): the same order statistic by RADIX SELECTION -- floats
// mapped to keys whose unsigned order is the floats' order, the k-th smallest key found bit by bit from the top with one
// counting sweep of the window per bit (32 w^2 instead of w^4).
__device__ __forceinline__ unsigned order_key(float x)
{
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__global__ void __launch_bounds__(256) k_median_big(const float *__restrict__ u, int nx, int ny, int nch, int radius,
                                                    float *__restrict__ out, long long first, long long last)
{
    const long long npix = (long long)nx * ny;
    const long long idx = first + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= last) return;
    const long long p = idx % npix;
    const int x = (int)(p % nx), y = (int)(p / nx);
    const float *pl = u + (idx / npix) * npix;
    const int x0 = x - radius < 0 ? 0 : x - radius, x1 = x + radius >= nx ? nx - 1 : x + radius;
    const int y0 = y - radius < 0 ? 0 : y - radius, y1 = y + radius >= ny ? ny - 1 : y + radius;
    int n = 0;
    for (int j = y0; j <= y1; j++)
        for (int i = x0; i <= x1; i++) {
            const float s = pl[i + (long long)j * nx];
            n += (s == s);
        }
    float res = pl[p];  // an all-NaN window leaves the pixel as it is
    if (n > 0) {
        int k = n / 2;
        unsigned prefix = 0;  // the bits of the answer above `b`
        for (int b = 31; b >= 0; b--) {
            int zeros = 0;  // samples that agree with the prefix and have bit b clear
            for (int j = y0; j <= y1; j++)
                for (int i = x0; i <= x1; i++) {
                    const float s = pl[i + (long long)j * nx];
                    const unsigned key = order_key(s);
                    const bool match = b == 31 ? true : (key >> (b + 1)) == prefix;
                    zeros += (s == s) && match && !((key >> b) & 1u);
                }
            if (k < zeros) prefix = prefix << 1;
            else {
                k -= zeros;
                prefix = (prefix << 1) | 1u;
            }
        }
        const unsigned ub = (prefix & 0x80000000u) ? (prefix & 0x7fffffffu) : ~prefix;
        res = __builtin_bit_cast(float, ub);
    }
    out[idx] = res;
}

hipError_t launch_median(const float *u, int nx, int ny, int nch, int radius, float *out, hipStream_t s)
{
    const long long n = (long long)nx * ny * nch;
    if (radius > 7) {
        // 33 sweeps of a (2r+1)^2 window per pixel, one thread per pixel: cut into launches of bounded work (~1.5e11 window
        // reads each, a fraction of a second) so that no single kernel runs long enough to look hung; the total is
        // capped by the caller (mgm_median_dev, kMedianMaxReads)
        const double per_pixel = 33.0 * (2.0 * radius + 1.0) * (2.0 * radius + 1.0);
        long long chunk = (long long)(1.5e11 / per_pixel);
        chunk = chunk < 256 ? 256 : (chunk / 256) * 256;
        for (long long a = 0; a < n; a += chunk) {
            const long long b = a + chunk < n ? a + chunk : n;
            hipLaunchKernelGGL(k_median_big, dim3((unsigned)((b - a + 255) / 256)), dim3(256), 0, s, u, nx, ny, nch, radius, out, a, b);
        }
    } else hipLaunchKernelGGL(k_median, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, u, nx, ny, nch, radius, out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_leftright(const float *__restrict__ dx, int nc, int nr, const float *__restrict__ Rdx,
                                                   int Rnc, float threshold, float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)nc * nr) return;
    const int x = (int)(i % nc), y = (int)(i / nc);
    const float d = dx[i];
    // round(x + d) converted to int; a NaN (or huge) disparity lands outside every image
    const double rr = __builtin_round((double)(x + d));
    const int Lx = (rr >= -2147483648.0 && rr <= 2147483647.0) ? (int)rr : -2147483647 - 1;
    float res = __builtin_nanf("");
    if (Lx < Rnc && Lx >= 0) {
        const float Rx = Lx + Rdx[Lx + (long long)y * Rnc];
        if (!(__builtin_fabs((double)(Rx - x)) > (double)threshold)) res = d;
    }
    out[i] = res;
}

hipError_t launch_leftright(const float *dx, int nc, int nr, const float *Rdx, int Rnc, float threshold, float *out,
                            hipStream_t s)
{
    const long long n = (long long)nc * nr;
    hipLaunchKernelGGL(k_leftright, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, dx, nc, nr, Rdx, Rnc, threshold, out);
    return hipGetLastError();
}

// The uniqueness test on the runner-up search's two costs (this project's own step, the reference has none):
// conf = 1 - cost1 / cost2 -- one division, one subtraction (this file is built with -ffp-contract=off), whatever IEEE gives:
// no runner-up (cost2 = +INF) gives 1, no winner (INF / INF) and 0 / 0 give NaN -- and out = conf < ratio ? NaN : d, so a NaN
// conf keeps d.  Every input is read before anything is written: out may be d.
__global__ void __launch_bounds__(256) k_uniqueness(const float *d, const float *__restrict__ cost1, const float *__restrict__ cost2,
                                                    long long n, float ratio, float *out, float *__restrict__ conf)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float q = cost1[i] / cost2[i];
    const float cf = 1.0f - q;
    if (conf) conf[i] = cf;
    if (out) {
        const float v = d[i];
        out[i] = cf < ratio ? __builtin_nanf("") : v;
    }
}

hipError_t launch_uniqueness(const float *d, const float *cost1, const float *cost2, long long n, float ratio, float *out, float *conf,
                             hipStream_t s)
{
    hipLaunchKernelGGL(k_uniqueness, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, cost1, cost2, n, ratio, out, conf);
    return hipGetLastError();
}

// The consensus filter on the votes of mgm_wta_consensus_dev: out = votes < (float)minvotes ? NaN : d, so a NaN vote
// count keeps d.  Both inputs are read before anything is written: out may be d.
__global__ void __launch_bounds__(256) k_consensus_filter(const float *d, const float *__restrict__ votes, long long n, float minvotes, float *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = d[i], k = votes[i];
    out[i] = k < minvotes ? __builtin_nanf("") : v;
}

hipError_t launch_consensus_filter(const float *d, const float *votes, long long n, int minvotes, float *out, hipStream_t s)
{
    hipLaunchKernelGGL(k_consensus_filter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d, votes, n, (float)minvotes, out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) k_backproject(const float *__restrict__ u, int nx, int ny, int nch,
                                                     const float *__restrict__ v, int vnx, int vny,
                                                     const float *__restrict__ disp, float *__restrict__ out)
{
    const int unpix = nx * ny, vnpix = vnx * vny;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)unpix * nch) return;
    const int c = (int)(idx / unpix), p = (int)(idx % unpix);
    const int x = p % nx, y = p / nx;
    const float qx = disp[x + nx * y];
    const float px = x + qx, py = (float)y;
    const bool inside = px >= 0 && py >= 0 && px < vnx && py < vny;
    float r = u[x + y * nx + c * unpix];
    if (inside) {
        unsigned long long k = (unsigned long long)(x + qx + (y + 0.0f) * vnx + c * vnpix);  // (float arithmetic, as there)
        const unsigned long long last = (unsigned long long)vnpix * nch - 1;
        r = v[k < last ? k : last];
    }
    out[idx] = r;
}

hipError_t launch_backproject(const float *u, int nx, int ny, int nch, const float *v, int vnx, int vny, const float *disp,
                              float *out, hipStream_t s)
{
    const long long n = (long long)nx * ny * nch;
    hipLaunchKernelGGL(k_backproject, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, u, nx, ny, nch, v, vnx, vny, disp, out);
    return hipGetLastError();
}

// ---- update_dmin_dmax (mgm.cc:120-158) + the two remove_nonfinite_values_Img calls that follow it (387-388) ------
// global finite minimum / maximum of the disparity map (image_minmax, img_tools.h:183-199): floats ordered
// through their bit patterns so that integer atomics can reduce them
__global__ void __launch_bounds__(256) k_minmax_init(unsigned *mm)
{
    mm[0] = f2ord(__builtin_huge_valf());   // gmin = +INF
    mm[1] = f2ord(-__builtin_huge_valf());  // gmax = -INF
}
__global__ void __launch_bounds__(256) k_minmax(const float *__restrict__ u, long long n, unsigned *mm)
{
    float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float v = u[i];
        if (finite_bits(v)) {
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    }
    atomicMin(mm + 0, f2ord(lo));
    atomicMax(mm + 1, f2ord(hi));
}
__global__ void __launch_bounds__(256) k_update_ranges(const float *__restrict__ outoff, int nx, int ny, int slack, int r,
                                                       const unsigned *__restrict__ mm, float *__restrict__ dminI,
                                                       float *__restrict__ dmaxI)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)nx * ny) return;
    const int i = (int)(idx % nx), j = (int)(idx / nx);
    const float gmin = ord2f(mm[0]), gmax = ord2f(mm[1]);
    float dmin = __builtin_huge_valf(), dmax = -__builtin_huge_valf();
    for (int dj = -r; dj <= r; dj++)
        for (int di = -r; di <= r; di++) {
            int x = i + di, y = j + dj;  // valneumann
            x = x >= 0 ? x : 0;
            x = x < nx ? x : nx - 1;
            y = y >= 0 ? y : 0;
            y = y < ny ? y : ny - 1;
            const float v = outoff[x + (long long)y * nx];
            const float a = finite_bits(v) ? v - slack : gmin - slack;
            const float b = finite_bits(v) ? v + slack : gmax + slack;
            dmin = __builtin_fminf(dmin, a);
            dmax = __builtin_fmaxf(dmax, b);
        }
    float lo = dminI[idx], hi = dmaxI[idx];
    if (finite_bits(dmin)) {
        lo = dmin;
        hi = dmax;
    }
    // remove_nonfinite_values_Img(dminI, gmin), (dmaxI, gmax)
    dminI[idx] = finite_bits(lo) ? lo : gmin;
    dmaxI[idx] = finite_bits(hi) ? hi : gmax;
}

// image_minmax alone: mm[0] / mm[1] receive the finite minimum / maximum of u as ordered bit patterns (+INF / -INF when
// there is no finite sample); mgm_pyramid.hip reads them the same way
hipError_t launch_minmax(const float *u, long long n, unsigned *mm, hipStream_t s)
{
    hipLaunchKernelGGL(k_minmax_init, dim3(1), dim3(1), 0, s, mm);
    long long nb = (n + 255) / 256;
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(k_minmax, dim3((unsigned)nb), dim3(256), 0, s, u, n, mm);
    return hipGetLastError();
}

hipError_t launch_update_ranges(const float *outoff, int nx, int ny, int slack, int radius, float *dminI, float *dmaxI,
                                float *scratch2, hipStream_t s)
{
    unsigned *mm = reinterpret_cast<unsigned *>(scratch2);
    const long long n = (long long)nx * ny;
    if (slack < 0) slack = -slack;
    if (hipError_t e = launch_minmax(outoff, n, mm, s)) return e;
    hipLaunchKernelGGL(k_update_ranges, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, outoff, nx, ny, slack, radius, mm, dminI,
                       dmaxI);
    return hipGetLastError();
}

}  // namespace mgm
