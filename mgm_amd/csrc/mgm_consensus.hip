// mgm_consensus.hip -- the consensus votes (this project's own measure, the reference has none): how many of the
// NDIR scan-line passes, each taken ALONE, pick the label a given map holds.
//
//   pass winner   w_p(x) = the first strict minimum, by rising label, among the finite entries of Lr_p(x, .) over the labels the
//                 pixel owns (dense: 0..L-1; a ragged volume on its hull: its own range inside the volume; the range-proportional
//                 layout: the slots of its own range).  Padding slots and unowned slots are never candidates, whatever they hold.
//   vote          w_p exists and fabsf((float)(w_p + dmin) - d(x)) <= tol: one float subtraction, a NaN or infinite d(x) gets none
//   votes(x)      = (float) number of voting passes; winners[p](x) = (float)(w_p + dmin), NaN without a winner
//
// No costs are read and no sum is formed.  No LDS, no atomics, no barriers, no waiting loop: a wave never waits on another.
#include <algorithm>

#include "mgm_device.h"
#include "mgm_planner.h"

namespace mgm {

namespace {

constexpr int NONE = 0x7fffffff;

template <int CTRL>
__device__ __forceinline__ float cs_dpp_fmin(float v)  // min with the lane CTRL names (every lane has one under these controls)
{
    return __builtin_fminf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false)));
}
// over the row of 16 lanes, in every lane of it: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ float row_fmin(float v)
{
    v = cs_dpp_fmin<0xB1>(v);
    v = cs_dpp_fmin<0x4E>(v);
    v = cs_dpp_fmin<0x141>(v);
    return cs_dpp_fmin<0x140>(v);
}
__device__ __forceinline__ float lane_f(float v, int l)  // v of lane l (a constant)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}
// over the wave, wave-uniform: the four rows' minima through scalar registers
__device__ __forceinline__ float wave_fmin(float v)
{
    v = row_fmin(v);
    return __builtin_fminf(__builtin_fminf(lane_f(v, 0), lane_f(v, 16)), __builtin_fminf(lane_f(v, 32), lane_f(v, 48)));
}
// the smaller (value, label) over the wave, in every lane
__device__ __forceinline__ void cs_wave_take(float &best, int &bi)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_xor(best, d);
        const int oi = __shfl_xor(bi, d);
        if (ov < best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
}
// the first index of v that holds m (one does, in the lanes that are asked)
template <int K>
__device__ __forceinline__ int first_equal(const float (&v)[K], float m)
{
    int kk = 0;
#pragma unroll
    for (int k = K - 1; k >= 1; k--) kk = v[k] == m ? k : kk;
    return v[0] == m ? 0 : kk;
}
// a vote: label w (wave- or row-uniform, NONE: no winner) against the map's value
__device__ __forceinline__ int vote_of(int w, int add, float dv, float tol)
{
    return (w != NONE && __builtin_fabsf((float)(w + add) - dv) <= tol) ? 1 : 0;
}
__device__ __forceinline__ float label_of(int w, int add) { return w == NONE ? __builtin_nanf("") : (float)(w + add); }

// the labels a pixel owns on the dense layout, as label indices: the volume's, cut to the pixel's own range on a ragged hull
__device__ __forceinline__ void dense_zone(const WtaConsensusParams &P, long long pix, int &zl, int &zh)
{
    zl = 0, zh = P.L - 1;
    if (P.rlo) {
        const int cl = (int)P.rlo[pix] - P.dmin, ch = (int)P.rhi[pix] - P.dmin;  // Dvec(int min, int max) of allocate_costvolume: float -> int
        zl = cl > zl ? cl : zl;
        zh = ch < zh ? ch : zh;
    }
}

}  // namespace

// STREAMING: the Lr volumes are read exactly as k_wta_runnerup reads them -- one wave per pixel, its 64*LPL label slots in registers,
// every stream a coalesced slab, PPW pixels requested before the first is consumed.  Label stride Lk == 64*LPL.  Lanes hold
// contiguous, rising labels, so a pass's first strict minimum is a value-only wave minimum, the lowest lane that holds it and that
// lane's first slot that does: unowned and non-finite entries enter as +INF, and a minimum of +INF means no winner.
template <int LPL, int PPW, int MAXD>
__global__ void __launch_bounds__(256) k_wta_consensus(const WtaConsensusParams P)
{
    constexpr int LP = LPL * 64;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o0 = lane * LPL;
    // grid-stride over groups of PPW consecutive pixels
    for (long long g0 = ((long long)blockIdx.x * 4 + wv) * PPW; g0 < P.npix; g0 += (long long)gridDim.x * 4 * PPW) {
        float l[MAXD][PPW][LPL];
#pragma unroll
        for (int p = 0; p < MAXD; p++) {
            if (p < P.NDIR) {
#pragma unroll
                for (int u = 0; u < PPW; u++) {
                    const long long g = g0 + u < P.npix ? g0 + u : P.npix - 1;
                    const float *q = P.Lr + (long long)p * P.nvol + g * LP + o0;
#pragma unroll
                    for (int k = 0; k < LPL; k++) l[p][u][k] = q[k];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            if (g0 + u >= P.npix) break;
            const long long pix = g0 + u;
            int zl, zh;
            dense_zone(P, pix, zl, zh);
            const float dv = P.votes ? P.d[pix] : 0.0f;
            int nv = 0;
#pragma unroll
            for (int p = 0; p < MAXD; p++) {
                if (p < P.NDIR) {
                    float v[LPL], m = f_inf();
#pragma unroll
                    for (int k = 0; k < LPL; k++) {
                        const float x = l[p][u][k];
                        v[k] = (o0 + k >= zl && o0 + k <= zh && finite_bits(x)) ? x : f_inf();
                        m = __builtin_fminf(m, v[k]);
                    }
                    const float wm = wave_fmin(m);
                    int w = NONE;
                    if (wm != f_inf()) {  // (wave-uniform) equal values, -0 / +0 included, go to the lowest lane and its first slot
                        const int fl = __builtin_ctzll(__ballot(m == wm));
                        w = fl * LPL + __builtin_amdgcn_readlane(first_equal(v, wm), fl);
                    }
                    nv += vote_of(w, P.dmin, dv, P.tol);
                    if (P.winners && lane == 0) P.winners[(long long)p * P.npix + pix] = label_of(w, P.dmin);
                }
            }
            if (P.votes && lane == 0) P.votes[pix] = (float)nv;
        }
    }
}

// Any label count and label stride (strides that are no multiple of 64, more than 1024 labels) and either layout: one wavefront per
// pixel, the labels strided over the lanes, a (value, label) butterfly per pass.  Nothing here is tuned.
__global__ void __launch_bounds__(256) k_wta_consensus_any(const WtaConsensusParams P)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (long long pix = (long long)blockIdx.x * 4 + wv; pix < P.npix; pix += (long long)gridDim.x * 4) {
        int zl, zh, add = P.dmin;
        if (P.rec) {  // slot k <-> disparity rec.x + k; the pixel owns [rec.y, rec.z]
            const int4 rec = reinterpret_cast<const int4 *>(P.rec)[pix];
            add = rec.x;
            zl = rec.y - rec.x > 0 ? rec.y - rec.x : 0;
            zh = rec.z - rec.x < P.L - 1 ? rec.z - rec.x : P.L - 1;
        } else {
            dense_zone(P, pix, zl, zh);
        }
        const float dv = P.votes ? P.d[pix] : 0.0f;
        int nv = 0;
        for (int p = 0; p < P.NDIR; p++) {
            const float *q = P.Lr + (long long)p * P.nvol + pix * P.Lk;
            float best = f_inf();
            int w = NONE;
            for (int o = zl + lane; o <= zh; o += 64) {
                const float x = q[o];
                if (finite_bits(x) && best > x) {
                    best = x;
                    w = o;
                }
            }
            cs_wave_take(best, w);
            nv += vote_of(w, add, dv, P.tol);
            if (P.winners && lane == 0) P.winners[(long long)p * P.npix + pix] = label_of(w, add);
        }
        if (P.votes && lane == 0) P.votes[pix] = (float)nv;
    }
}

// The RANGE-PROPORTIONAL layout, patterned on k_wta_rel: four pixels per wave, a pixel's 16*SPL slots on a row of 16 lanes, SPL per
// lane (16-byte loads), the pixel's record one int4 (disparity of slot 0, lowest, highest).  The passes' slabs are all requested
// before the first is consumed.  The cost codes are not read, so their width does not matter: two instances.
template <int SPL>
__global__ void __launch_bounds__(256) k_wta_consensus_rel(const WtaConsensusParams P)
{
    constexpr int SLOTS = 16 * SPL;
    typedef float f4 __attribute__((ext_vector_type(4)));
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, grp = lane >> 4;
    const long long nquads = (P.npix + 3) / 4;
    for (long long q4 = (long long)blockIdx.x * 4 + wv; q4 < nquads; q4 += (long long)gridDim.x * 4) {
        const long long pix0 = q4 * 4 + grp;
        const bool live = pix0 < P.npix;
        const long long pix = live ? pix0 : P.npix - 1;
        const int4 rec = reinterpret_cast<const int4 *>(P.rec)[pix];
        const int b = rec.x, lo = rec.y, hi = rec.z;
        float x[kMaxDirs][SPL];
#pragma unroll
        for (int p = 0; p < kMaxDirs; p++) {
            if (p < P.NDIR) {
#pragma unroll
                for (int h = 0; h < SPL / 4; h++) {
                    const f4 t = reinterpret_cast<const f4 *>(P.Lr + (long long)p * P.nvol + pix * SLOTS + SPL * li)[h];
#pragma unroll
                    for (int q = 0; q < 4; q++) x[p][4 * h + q] = t[q];
                }
            }
        }
        const float dv = P.votes ? P.d[pix] : 0.0f;
        int nv = 0;
#pragma unroll
        for (int p = 0; p < kMaxDirs; p++) {
            if (p < P.NDIR) {
                float v[SPL], m = f_inf();
#pragma unroll
                for (int q = 0; q < SPL; q++) {
                    const int dd = b + SPL * li + q;
                    v[q] = (dd >= lo && dd <= hi && finite_bits(x[p][q])) ? x[p][q] : f_inf();
                    m = __builtin_fminf(m, v[q]);
                }
                const float rm = row_fmin(m);
                // the row's lowest lane that holds the minimum (one does), and that lane's first slot that does
                const unsigned row = (unsigned)(__ballot(m == rm) >> (16 * grp)) & 0xffffu;
                const int fl = __builtin_ctz(row | 0x10000u) & 15;
                const int ko = __shfl(first_equal(v, rm), (lane & 48) | fl);
                const int w = rm != f_inf() ? SPL * fl + ko : NONE;
                nv += vote_of(w, b, dv, P.tol);
                if (P.winners && li == 0 && live) P.winners[(long long)p * P.npix + pix] = label_of(w, b);
            }
        }
        if (P.votes && li == 0 && live) P.votes[pix] = (float)nv;
    }
}

// from a choice of the planner (plan_wta_consensus) to its instance; anything else is hipErrorInvalidValue
hipError_t launch_wta_consensus(const WtaConsensusParams &p, const ConsensusChoice &c, hipStream_t s)
{
    if (c.grid < 1 || c.grid > 0x7fffffffll || p.L < 1 || p.Lk < p.L || p.npix < 1 || p.NDIR < 1 || p.NDIR > kMaxDirs || (!p.votes && !p.winners) || (p.votes && !p.d))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)c.grid), block(256);
    if (c.family == kConsensusAny) {
        hipLaunchKernelGGL(k_wta_consensus_any, grid, block, 0, s, p);
        return hipGetLastError();
    }
    if (c.family == kConsensusRel) {
        if (!p.rec || p.Lk != 16 * c.SPL || p.L != p.Lk) return hipErrorInvalidValue;
#define CONSENSUS_REL(SPL_)                                                              \
    if (c.SPL == SPL_) {                                                                 \
        hipLaunchKernelGGL((k_wta_consensus_rel<SPL_>), grid, block, 0, s, p);           \
        return hipGetLastError();                                                        \
    }
        CONSENSUS_REL(4) CONSENSUS_REL(8)
#undef CONSENSUS_REL
        return hipErrorInvalidValue;
    }
    if (c.family != kConsensusStream || p.rec || p.Lk != 64 * c.LPL || p.NDIR > c.MAXD) return hipErrorInvalidValue;
#define CONSENSUS(LPL_, PPW_, MAXD_)                                                      \
    if (c.LPL == LPL_ && c.PPW == PPW_ && c.MAXD == MAXD_) {                              \
        hipLaunchKernelGGL((k_wta_consensus<LPL_, PPW_, MAXD_>), grid, block, 0, s, p);   \
        return hipGetLastError();                                                         \
    }
    CONSENSUS(1, 8, 4) CONSENSUS(1, 4, 8) CONSENSUS(2, 8, 4) CONSENSUS(2, 4, 8) CONSENSUS(3, 4, 4) CONSENSUS(3, 2, 8) CONSENSUS(4, 6, 4) CONSENSUS(4, 3, 8)
    CONSENSUS(6, 2, 4) CONSENSUS(6, 1, 8) CONSENSUS(8, 2, 4) CONSENSUS(8, 1, 8) CONSENSUS(12, 1, 8) CONSENSUS(16, 1, 8)
#undef CONSENSUS
    return hipErrorInvalidValue;
}

}  // namespace mgm
