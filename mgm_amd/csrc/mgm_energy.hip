// mgm_energy.hip -- the energy of a solution: how good a disparity map is in the terms of the functional the
// aggregation minimises.  One launch, a lane per pixel in raster order (d, w8 and E are read and written coalesced; the one cost a
// pixel needs is a gather, whatever the layout of the volume).
//
//   kinds 0, 1, 2   evaluate_energy_4connected (mgm_print_energy.h:17-96; what TSGM_DEBUG=1 prints): truncated L1, L1, L2.  In
//                   fp32, one rounding per operation (this file is built with -ffp-contract=off), in the reference's order:
//                     G = 0 + C(p, (int)o)                  Dvec::operator[]: truncation, +INF for a label the pixel does not own
//                     for t = 0..3, r = p + dir[t], q = p + dir[t+1], dirs (-1,0) (0,1) (1,0) (0,-1) (-1,0); BOTH inside the image:
//                       kind 1   G += fabsf(o_r - o) / 4
//                       kind 2   G += sqrtf((o_r - o)^2 + (o_q - o)^2) / 4
//                       kind 0   G += (fabsf(o_r - o) <= 1 ? P1 : P2) / 4
//                   E(p) = G.  A NaN neighbour makes kinds 1 and 2 NaN and takes the P2 branch of kind 0.
//   kind 3          the model energy: data + 0.5 * sum of the weighted potentials of the run's own kind towards the first 4 or 8
//                   neighbours in the order of mgm_weights.h (W, E, S, N, NW, NE, SE, SW).  A pixel whose d is not finite has
//                   E = NaN and is counted nowhere; a neighbour whose d is not finite contributes no term.
//                     data   = C(p, (int)rintf(d))
//                     a      = fabsf(d_q - d_p),  w = w8[k](p) or 1
//                     V      = a == 0 ? 0 : a <= 1 ? fminf(P1*w, P2*w) : P2*w          (Hirschmueller)
//                     V      = fminf((P1*w) * a, P2*w)                                 (truncated linear)
//                     smooth = 0.5f * (((0 + V_k0) + V_k1) + ...),   E = data + smooth
//   a label a pixel does not own reads +INF: outside the volume's range, outside the pixel's own range of a ragged volume, and any d
//   that is not finite or has |d| >= 2^24 (kinds 0-2; kind 3 likewise for |d| >= 2^24)
//
// Totals: every block of kEnergyThreads pixels reduces the data terms, the edge terms and E of its pixels with finite d in fp64 --
// a fixed tree over the block's lanes -- and writes ONE partial; the host adds the partials in index order.  No atomics on floats:
// two calls give the same bits.  (For kinds 0-2 the edge terms are also summed on their own, 0 + t_0 + t_1 ..., for `smooth`.)
#include "mgm_device.h"
#include "mgm_energyplan.h"

namespace mgm {

// the cost of label `lab` at pixel `pix` in whatever copy is being read; +INF where the pixel does not own the label
__device__ __forceinline__ float energy_cost(const EnergyParams &p, long long pix, bool owned, int lab)
{
    const float inf = __builtin_huge_valf();
    if (!owned) return inf;
    const long long o = (long long)lab - p.dmin;
    if (o < 0 || o >= p.L) return inf;
    if (p.rlo && (lab < (int)p.rlo[pix] || lab > (int)p.rhi[pix])) return inf;
    long long k = o;
    if (p.records) {  // range-proportional copy: slot 0 stands for the disparity of the pixel's record
        const int4 rec = *reinterpret_cast<const int4 *>(p.records + pix * 4);
        if (lab < rec.y || lab > rec.z) return inf;
        k = (long long)lab - rec.x;
    }
    if (k < 0 || k >= p.stride) return inf;
    const size_t i = (size_t)pix * (size_t)p.stride + (size_t)k;
    if (p.cb == 4) return reinterpret_cast<const float *>(p.cost)[i];
    if (p.cb == 2) return c16_decode((unsigned)reinterpret_cast<const unsigned short *>(p.cost)[i]);
    return c8_decode((unsigned)reinterpret_cast<const uint8_t *>(p.cost)[i]);
}

__device__ __forceinline__ bool energy_label(float d, bool round, int *lab)
{
    const bool owned = finite_bits(d) && __builtin_fabsf(d) < 16777216.0f;
    *lab = owned ? (int)(round ? __builtin_rintf(d) : d) : 0;
    return owned;
}

__global__ void __launch_bounds__(kEnergyThreads) k_energy(const EnergyParams p)
{
    __shared__ double s_sum[3][kEnergyThreads];
    __shared__ unsigned s_cnt[kEnergyThreads];
    const long long npix = (long long)p.nx * p.ny;
    const long long pix = (long long)blockIdx.x * kEnergyThreads + threadIdx.x;
    float data = 0.0f, smooth = 0.0f, E = 0.0f;
    bool counted = false;
    if (pix < npix) {
        const int y = (int)(pix / p.nx), x = (int)(pix - (long long)y * p.nx);
        const float o = p.d[pix];
        counted = finite_bits(o);
        int lab;
        if (p.kind == 3) {
            // mgm_weights.h:69: W, E, S, N, NW, NE, SE, SW
            constexpr int dx[8] = {-1, 1, 0, 0, -1, 1, 1, -1}, dy[8] = {0, 0, 1, -1, -1, -1, 1, 1};
            const bool owned = energy_label(o, true, &lab);
            data = energy_cost(p, pix, owned, lab);
            float s = 0.0f;
            for (int k = 0; k < p.connectivity; k++) {
                const int qx = x + dx[k], qy = y + dy[k];
                if (qx < 0 || qx >= p.nx || qy < 0 || qy >= p.ny) continue;
                const float oq = p.d[(long long)qy * p.nx + qx];
                if (!finite_bits(oq)) continue;
                const float w = p.w8 ? p.w8[(long long)k * npix + pix] : 1.0f;
                const float a = __builtin_fabsf(oq - o), p1w = p.P1 * w, p2w = p.P2 * w;
                float V;
                if (p.use_fh) V = __builtin_fminf(p1w * a, p2w);
                else V = a == 0.0f ? 0.0f : (a <= 1.0f ? __builtin_fminf(p1w, p2w) : p2w);
                s = s + V;
            }
            smooth = 0.5f * s;
            E = counted ? data + smooth : __builtin_nanf("");
        } else {
            constexpr int dx[5] = {-1, 0, 1, 0, -1}, dy[5] = {0, 1, 0, -1, 0};
            const bool owned = energy_label(o, false, &lab);
            data = energy_cost(p, pix, owned, lab);
            float G = 0.0f + data, s = 0.0f;
            for (int t = 0; t < 4; t++) {
                const int rx = x + dx[t], ry = y + dy[t], qx = x + dx[t + 1], qy = y + dy[t + 1];
                if (rx < 0 || rx >= p.nx || ry < 0 || ry >= p.ny) continue;
                if (qx < 0 || qx >= p.nx || qy < 0 || qy >= p.ny) continue;
                const float dr = p.d[(long long)ry * p.nx + rx] - o;
                float term;
                if (p.kind == 1) {
                    term = __builtin_fabsf(dr) / 4.0f;
                } else if (p.kind == 2) {
                    const float dq = p.d[(long long)qy * p.nx + qx] - o;
                    // (the correctly rounded square root: v_sqrt_f32 plus its correction steps; __fsqrt_rn is the bare instruction here)
                    term = __builtin_sqrtf(dr * dr + dq * dq) / 4.0f;
                } else {
                    term = (__builtin_fabsf(dr) <= 1.0f ? p.P1 : p.P2) / 4.0f;
                }
                G = G + term;
                s = s + term;
            }
            smooth = s;
            E = G;
        }
        if (p.E) p.E[pix] = E;
    }
    if (!p.partials) return;  // (uniform: a kernel argument)
    const int t = threadIdx.x;
    s_sum[0][t] = counted ? (double)data : 0.0;
    s_sum[1][t] = counted ? (double)smooth : 0.0;
    s_sum[2][t] = counted ? (double)E : 0.0;
    s_cnt[t] = counted ? 1u : 0u;
    __syncthreads();
    for (int half = kEnergyThreads / 2; half > 0; half >>= 1) {  // a fixed tree: the same order of additions in every call
        if (t < half) {
            for (int j = 0; j < 3; j++) s_sum[j][t] = s_sum[j][t] + s_sum[j][t + half];
            s_cnt[t] += s_cnt[t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        double *out = reinterpret_cast<double *>(p.partials) + (size_t)blockIdx.x * kEnergyPartialWords;
        out[0] = s_sum[0][0], out[1] = s_sum[1][0], out[2] = s_sum[2][0];
        reinterpret_cast<unsigned long long *>(out)[3] = s_cnt[0];
    }
}

hipError_t launch_energy(const EnergyParams &p, long long blocks, hipStream_t s)
{
    if (blocks < 1 || blocks != plan_energy_launch(p.nx, p.ny).blocks) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_energy, dim3((unsigned)blocks), dim3(kEnergyThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mgm
