// mgm_wta.hip -- K4+K5+K6: ordered sum of the per-pass Lr volumes, over-count
// correction, winner-takes-all and (optionally) V-fit refinement, one wavefront
// per pixel.
//
//   S accumulation in pass order      mgm_core.cc:582-587   (S = ((0+L0)+L1)+...)
//   S -= (NDIR-1)*C, first finite     mgm_core.cc:592-609
//   strict minimum wins
//   subpixel_refinement_sgm + VfitMinimum   mgm_refine.h:51-68, refine.h:70-92
//
// Compiled with default floating point: S may hold NaN (inf - inf) and the
// refinement must propagate NaN/inf exactly as IEEE arithmetic does on the CPU.
#include <algorithm>
#include <cstdlib>

#include "mgm_device.h"
#include "mgm_planner.h"

namespace mgm {

// refine.h:70-92
__device__ __forceinline__ void vfit(float v0, float v1, float v2, float &v_min, float &x_min)
{
    if ((v1 > v0) && (v1 > v2)) {
        v_min = v1;
        x_min = 0.0f;
        return;
    }
    float slope = v2 - v1;
    if ((v2 - v1) < (v0 - v1)) slope = v0 - v1;
    x_min = (v0 - v2) / (2.0f * slope);
    v_min = v2 + (x_min - 1.0f) * slope;
}

// PPW slabs per wave and iteration: all of them are requested before the first is consumed.
// One KiB per stream per wave leaves HBM at ~4.7 TB/s, two at ~6 TB/s (tools/microbench/bw.hip).
// MAXD: upper bound of NDIR the instance is built for (4 or 8): with at most 4 directions twice the slabs fit the
// registers of a wave.
// SUB: pixels per slab.  A slab is the 64*LPL consecutive floats a wave loads per stream; with L = 64*LPL/SUB labels
// that is SUB consecutive pixels, each reduced by its own 64/SUB lanes -- 128 labels run as LPL = 4, SUB = 2 (16-byte
// loads, two arg-mins per butterfly) instead of LPL = 2, SUB = 1.  SUB > 1 needs EXACT and npix % SUB == 0.
template <int LPL, int PPW, bool EXACT, int MAXD = kMaxDirs, int SUB = 1>
__global__ void __launch_bounds__(256) k_wta(const WtaParams P)
{
    static_assert(SUB == 1 || EXACT, "several pixels per slab only without padding lanes");
    constexpr int LP = LPL * 64;
    constexpr int LANES = 64 / SUB;  // lanes per pixel
    __shared__ float sS[4][LP];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = P.L;          // label stride of a pixel (a multiple of 64/SUB... when EXACT: L * SUB == LP)
    const int Lr_ = P.Lreal;    // labels that exist
    constexpr bool exact = EXACT;  // no label slot is padding, loads need no guard
    const int Ls = SUB > 1 ? LP : L;          // floats per slab
    const int m0 = lane * LPL;                // this lane's offset in the slab
    const int sub = lane / LANES;             // its pixel of the slab
    const int o0 = (lane % LANES) * LPL;      // its first label
    const bool c8 = P.C8 && exact;  // compact costs: one byte per label (wave-uniform)
    const long long nslab = P.npix / SUB;
    // grid-stride over groups of PPW consecutive slabs
    for (long long g0 = ((long long)blockIdx.x * 4 + wv) * PPW; g0 < nslab; g0 += (long long)gridDim.x * 4 * PPW) {
        float c[PPW][LPL], l[MAXD][PPW][LPL];
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            const long long g = g0 + u < nslab ? g0 + u : nslab - 1;
            if (c8 && P.cbytes == 2) {  // (two bytes per cost: absolute differences of colour pairs, ...)
                const unsigned short *q = reinterpret_cast<const unsigned short *>(P.C8) + g * Ls + m0;
#pragma unroll
                for (int k = 0; k < LPL; k++) c[u][k] = c16_decode(q[k]);
            } else if (c8) {
                const uint8_t *q = P.C8 + g * Ls + m0;
#pragma unroll
                for (int k = 0; k < LPL; k++) c[u][k] = c8_decode(q[k]);
            } else {
                const float *q = P.C + g * Ls + m0;
#pragma unroll
                for (int k = 0; k < LPL; k++) c[u][k] = (exact || m0 + k < L) ? q[k] : f_inf();
            }
        }
#pragma unroll
        for (int p = 0; p < MAXD; p++) {
            if (p < P.NDIR) {
#pragma unroll
                for (int u = 0; u < PPW; u++) {
                    const long long g = g0 + u < nslab ? g0 + u : nslab - 1;
                    const float *q = P.Lr + (long long)p * P.nvol + g * Ls + m0;
#pragma unroll
                    for (int k = 0; k < LPL; k++) l[p][u][k] = (exact || m0 + k < L) ? q[k] : f_inf();
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            if (g0 + u >= nslab) break;
            const long long pix = (g0 + u) * SUB + sub;  // (per lane group)
            // S = ((0 + L0) + L1) + ... in pass order (mgm_core.cc:582-587)
            float S[LPL];
#pragma unroll
            for (int k = 0; k < LPL; k++) S[k] = 0.0f;
#pragma unroll
            for (int p = 0; p < MAXD; p++) {
                if (p < P.NDIR) {
#pragma unroll
                    for (int k = 0; k < LPL; k++) S[k] = S[k] + l[p][u][k];
                }
            }
            if (P.FIX == 1) {
                const float f = (float)(P.NDIR - 1);
#pragma unroll
                for (int k = 0; k < LPL; k++) S[k] = S[k] - f * c[u][k];
            }
            // what a disparity outside the volume -- or, in a ragged volume, outside the pixel's own range -- holds in the
            // reference's S: never incremented (0), then the over-count term with C = +INF (mgm_core.cc:582-599)
            float vout = 0.0f;
            if (P.FIX == 1) vout = vout - (float)(P.NDIR - 1) * f_inf();
            if (P.clo) {
                const int cl = (int)P.clo[pix] - P.dmin, ch = (int)P.chi[pix] - P.dmin;
#pragma unroll
                for (int k = 0; k < LPL; k++)
                    if (o0 + k < cl || o0 + k > ch) S[k] = vout;
            }
            if (P.S) {
                float *q = P.S + pix * Lr_ + o0;
#pragma unroll
                for (int k = 0; k < LPL; k++)
                    if (o0 + k < Lr_) q[k] = S[k];
            }
            // first strict minimum among finite entries, ascending o
            float best = f_inf();
            int bi = 0x7fffffff;
            const bool windowed = P.wlo != nullptr;
            int wl = 0, wh = 0;  // window in label indices
            if (windowed) {
                wl = (int)P.wlo[pix] - P.dmin;  // Dvec(int min, int max) of allocate_costvolume: float -> int
                wh = (int)P.whi[pix] - P.dmin;
            }
#pragma unroll
            for (int k = 0; k < LPL; k++) {
                const float v = S[k];
                if (o0 + k < Lr_ && (!windowed || (o0 + k >= wl && o0 + k <= wh)) && finite_bits(v) && best > v) {
                    best = v;
                    bi = o0 + k;
                }
            }
#pragma unroll
            for (int d = LANES / 2; d >= 1; d >>= 1) {  // (xor partners stay inside the pixel's lane group)
                const float ov = __shfl_xor(best, d);
                const int oi = __shfl_xor(bi, d);
                if (ov < best || (ov == best && oi < bi)) {
                    best = ov;
                    bi = oi;
                }
            }
            if (windowed) {
                // window labels outside the volume, in scan order: below it, (the volume), above it
                if (finite_bits(vout)) {
                    if (wl < 0 && wl <= wh && !(best < vout)) {
                        best = vout;
                        bi = wl;
                    }
                    const int hi0 = wl > Lr_ ? wl : Lr_;
                    if (wh >= Lr_ && hi0 <= wh && vout < best) {
                        best = vout;
                        bi = hi0;
                    }
                }
            }
            float outv, outc = best;
            if (bi == 0x7fffffff) outv = __builtin_nanf("");  // the reference leaves minP uninitialised here
            else outv = (float)(bi + P.dmin);
            if (P.refine == 1 && !windowed) {  // (wave-uniform) every lane stages its part of S, each pixel reads its own
#pragma unroll
                for (int k = 0; k < LPL; k++) sS[wv][m0 + k] = S[k];
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (bi != 0x7fffffff && bi - 1 >= 0 && bi + 2 <= Lr_ - 1) {  // mgm_refine.h:58
                    const float *sp = sS[wv] + sub * L;
                    const float v0 = sp[bi - 1], v1 = sp[bi], v2 = sp[bi + 1];
                    float vmin, dx;
                    vfit(v0, v1, v2, vmin, dx);
                    outv = (float)(bi + P.dmin) + dx;
                    outc = vmin;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next slab overwrites sS
            }
            if (lane % LANES == 0) {
                P.out[pix] = outv;
                P.outcost[pix] = outc;
            }
        }
    }
}

// 192 and 384 labels: the same work with 16-BYTE loads.  Three labels per lane are 12-byte pieces (k_wta<3>: 5.6 TB/s of
// reads where 16-byte pieces reach 6.4, round 2), six are a 16- and an 8-byte piece -- so here a wave takes a GROUP of
// NPX consecutive pixels that fills three 1-KiB slabs exactly (4 x 192 or 2 x 384 labels = 768 floats) and lane l of
// slab j holds the four floats 4*(64 j + l) .. of the group: chunk t = 64 j + l belongs to pixel t / (L/4) and starts at
// its label 4*(t % (L/4)) (a chunk never straddles pixels: L is a multiple of four).  Every lane therefore holds three
// chunks of up to three different pixels; the arg-min of pixel q is a wave-wide butterfly over what each lane holds OF
// THAT PIXEL.  Plain volumes only (no padding, no windows, no ragged ranges): everything else takes k_wta.
template <int L, int MAXD>
__global__ void __launch_bounds__(256) k_wta_q(const WtaParams P)
{
    static_assert(L == 192 || L == 384, "groups of 768 floats");
    constexpr int NPX = 768 / L;   // pixels per group
    constexpr int CPP = L / 4;     // chunks per pixel
    __shared__ float sS[4][768];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const bool c8 = P.C8 != nullptr;
    const long long ngroup = P.npix / NPX;
    int cpix[3], clab[3];  // per slab: this lane's chunk -> pixel of the group, first label
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const int t = 64 * j + lane;
        cpix[j] = t / CPP;
        clab[j] = (t % CPP) * 4;
    }
    for (long long g = (long long)blockIdx.x * 4 + wv; g < ngroup; g += (long long)gridDim.x * 4) {
        float c[3][4], l[MAXD][3][4];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            if (c8 && P.cbytes == 2) {
                const uint2 w = *reinterpret_cast<const uint2 *>(P.C8 + (g * 768 + 256 * j + 4 * lane) * 2);
                c[j][0] = c16_decode(w.x & 65535u); c[j][1] = c16_decode(w.x >> 16);
                c[j][2] = c16_decode(w.y & 65535u); c[j][3] = c16_decode(w.y >> 16);
            } else if (c8) {
                const unsigned w = *reinterpret_cast<const unsigned *>(P.C8 + g * 768 + 256 * j + 4 * lane);
#pragma unroll
                for (int k = 0; k < 4; k++) c[j][k] = c8_decode((w >> (8 * k)) & 255u);
            } else {
                const float4 q = *reinterpret_cast<const float4 *>(P.C + g * 768 + 256 * j + 4 * lane);
                c[j][0] = q.x; c[j][1] = q.y; c[j][2] = q.z; c[j][3] = q.w;
            }
        }
#pragma unroll
        for (int p = 0; p < MAXD; p++)
            if (p < P.NDIR) {
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const float4 q = *reinterpret_cast<const float4 *>(P.Lr + (long long)p * P.nvol + g * 768 + 256 * j + 4 * lane);
                    l[p][j][0] = q.x; l[p][j][1] = q.y; l[p][j][2] = q.z; l[p][j][3] = q.w;
                }
            }
        // S = ((0 + L0) + L1) + ... in pass order, then the over-count term (mgm_core.cc:582-599)
        float S[3][4];
        const float f = (float)(P.NDIR - 1);
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float a = 0.0f;
#pragma unroll
                for (int p = 0; p < MAXD; p++)
                    if (p < P.NDIR) a = a + l[p][j][k];
                if (P.FIX == 1) a = a - f * c[j][k];
                S[j][k] = a;
            }
        if (P.S) {
#pragma unroll
            for (int j = 0; j < 3; j++) *reinterpret_cast<float4 *>(P.S + g * 768 + 256 * j + 4 * lane) = make_float4(S[j][0], S[j][1], S[j][2], S[j][3]);
        }
        // per chunk: first strict minimum among its finite entries, ascending label
        float cb[3];
        int ci[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            cb[j] = f_inf();
            ci[j] = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (finite_bits(S[j][k]) && cb[j] > S[j][k]) {
                    cb[j] = S[j][k];
                    ci[j] = clab[j] + k;
                }
        }
        if (P.refine == 1) {
#pragma unroll
            for (int j = 0; j < 3; j++) *reinterpret_cast<float4 *>(&sS[wv][256 * j + 4 * lane]) = make_float4(S[j][0], S[j][1], S[j][2], S[j][3]);
        }
#pragma unroll
        for (int q = 0; q < NPX; q++) {
            float best = f_inf();
            int bi = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < 3; j++)  // (a lane's chunks of one pixel lie in ascending label order over j)
                if (cpix[j] == q && (cb[j] < best)) {
                    best = cb[j];
                    bi = ci[j];
                }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float ov = __shfl_xor(best, d);
                const int oi = __shfl_xor(bi, d);
                if (ov < best || (ov == best && oi < bi)) {
                    best = ov;
                    bi = oi;
                }
            }
            float outv, outc = best;
            if (bi == 0x7fffffff) outv = __builtin_nanf("");  // the reference leaves minP uninitialised here
            else outv = (float)(bi + P.dmin);
            if (P.refine == 1) {
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (bi != 0x7fffffff && bi - 1 >= 0 && bi + 2 <= L - 1) {  // mgm_refine.h:58
                    const float *sp = sS[wv] + q * L;
                    float vmin, dx;
                    vfit(sp[bi - 1], sp[bi], sp[bi + 1], vmin, dx);
                    outv = (float)(bi + P.dmin) + dx;
                    outc = vmin;
                }
            }
            if (lane == 0) {
                P.out[g * NPX + q] = outv;
                P.outcost[g * NPX + q] = outc;
            }
        }
        if (P.refine == 1) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next group overwrites sS
    }
}

// Any label count (used beyond 2048 labels, where k_wta has no instance): one wavefront per pixel, the labels strided over
// the lanes.  Same arithmetic and the same rules as k_wta -- S = ((0 + L0) + L1) + ... in pass order, the over-count
// term, the first strict minimum among the finite entries of the pixel's window, V-fit on the winner's neighbours --
// with S recomputed for the three labels of the fit instead of being staged.  Nothing here is tuned: the reference's Dvec
// has no label limit (dvec.cc:60), and this keeps the library from having one.
__global__ void __launch_bounds__(256) k_wta_any(const WtaParams P)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = P.L, Lr_ = P.Lreal;
    const float f = (float)(P.NDIR - 1);
    float vout = 0.0f;  // what a disparity outside the volume / the pixel's own range holds in the reference's S
    if (P.FIX == 1) vout = vout - f * f_inf();
    for (long long pix = (long long)blockIdx.x * 4 + wv; pix < P.npix; pix += (long long)gridDim.x * 4) {
        int cl = 0, ch = Lr_ - 1;
        if (P.clo) {
            cl = (int)P.clo[pix] - P.dmin;
            ch = (int)P.chi[pix] - P.dmin;
        }
        const bool windowed = P.wlo != nullptr;
        int wl = 0, wh = 0;
        if (windowed) {
            wl = (int)P.wlo[pix] - P.dmin;
            wh = (int)P.whi[pix] - P.dmin;
        }
        auto S_at = [&](int o) {
            float a = 0.0f;
            for (int p = 0; p < P.NDIR; p++) a = a + P.Lr[(long long)p * P.nvol + pix * L + o];
            if (P.FIX == 1)
                a = a - f * (!P.C8 ? P.C[pix * L + o]
                                   : (P.cbytes == 2 ? c16_decode(reinterpret_cast<const unsigned short *>(P.C8)[pix * L + o]) : c8_decode(P.C8[pix * L + o])));
            if (o < cl || o > ch) a = vout;
            return a;
        };
        float best = f_inf();
        int bi = 0x7fffffff;
        for (int o = lane; o < Lr_; o += 64) {
            const float v = S_at(o);
            if (P.S) P.S[pix * Lr_ + o] = v;
            if ((!windowed || (o >= wl && o <= wh)) && finite_bits(v) && best > v) {
                best = v;
                bi = o;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(best, d);
            const int oi = __shfl_xor(bi, d);
            if (ov < best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if (windowed && finite_bits(vout)) {  // window labels outside the volume, in scan order: below it, (the volume), above it
            if (wl < 0 && wl <= wh && !(best < vout)) {
                best = vout;
                bi = wl;
            }
            const int hi0 = wl > Lr_ ? wl : Lr_;
            if (wh >= Lr_ && hi0 <= wh && vout < best) {
                best = vout;
                bi = hi0;
            }
        }
        float outv, outc = best;
        if (bi == 0x7fffffff) outv = __builtin_nanf("");  // the reference leaves minP uninitialised here
        else outv = (float)(bi + P.dmin);
        if (P.refine == 1 && !windowed && bi != 0x7fffffff && bi - 1 >= 0 && bi + 2 <= Lr_ - 1) {  // mgm_refine.h:58
            float vmin, dx;
            vfit(S_at(bi - 1), S_at(bi), S_at(bi + 1), vmin, dx);
            outv = (float)(bi + P.dmin) + dx;
            outc = vmin;
        }
        if (lane == 0) {
            P.out[pix] = outv;
            P.outcost[pix] = outc;
        }
    }
}

// ---- the pruned search (256 labels, one-byte compact costs, no padding / window / ranges, refinement none or vfit) -----------
// The pass kernel leaves, per pass, pixel and CHUNK of 32 labels (128 bytes of the slab, eight lanes here), the minimum of Lr over
// the chunk (PassParams::min_k).  Put the chunk minimum in the place of every Lr value of the sum and the same arithmetic gives a
// lower bound: fp32 addition and s - f*c are monotone in every operand, so
//     LB(d) = sum_fix(m_0(chunk(d)), ..., m_{N-1}(chunk(d)); C(d)) <= sum_fix(L_0(d), ..., L_{N-1}(d); C(d)) = S(d)
// bit for bit, no epsilon -- as long as both sides are evaluated by the same operations in the same order (sum_fix, below).  The
// winner needs the exact S only where it can lie:
//   (a) costs + N*8 minima of the pixel -> LB of every chunk: the smallest LB over its labels with a finite cost (a label with
//       C = +INF is out, its S is never finite).  s - f*c with f = NDIR-1 >= 0 does not rise with c under fp32 rounding, so that is
//       sum_fix of the minima at the chunk's LARGEST finite cost -- one evaluation per chunk (CPU: tests/test_wta_groups.py);
//   (b) the chunk with the smallest LB (the lowest one on ties) loads its Lr pieces: best0 = its smallest finite S (+INF: none);
//   (c) every other chunk with LB <= best0 loads too -- the set is fixed here, `<=` keeps a tie at a lower label in play; a chunk
//       that stays out has S >= LB > best0 on all its labels;
//   (d) first strict minimum among the finite S of what was loaded = the smallest (S, label); vfit takes S at the winner's two
//       neighbours from the lane that brought the winner (it held them when it took the label) and reads memory only for a
//       neighbour in another chunk (winner at label 32k or 32k + 31), by sum_fix's operations: the same float;
//   (e) nothing finite: NaN label, +INF cost, as in k_wta.
// The steps of a turn are round trips to memory, each starting after the last, and the waves wait on them (profiles/r09_*): (a) of the
// NEXT turn is asked for as soon as this turn's is consumed, (d) has no round trip of its own but for the edge labels, and with one
// group of pixels per wave (c) keeps two rounds in flight.
// On census volumes 1.8-2 of the 8 chunks of a pixel are loaded: 2.4 KB per pixel instead of 8.4.
//
// The layout: a pixel is a GROUP of eight lanes, a wave works on eight consecutive pixels at once (two per DPP row of 16 lanes).
// Lane (g, j) = (lane >> 3, lane & 7) OWNS chunk j of pixel g in (a): its 32 cost bytes, its minimum of every pass, its bound.
// In (b) and (c) the group's eight lanes read ONE chunk together, lane j the four labels 4j.. of it: a 128-byte line per pass
// and group.  (c) is a wave-uniform loop, every group taking its lowest remaining candidate per round; a group with none
// left sits the round out under the exec mask.  All reductions are three DPP steps inside the group.
template <int MAXD, int K>
__device__ __forceinline__ void sum_fix(const float (&l)[MAXD][K], const float (&c)[K], int ndir, int fix, float (&S)[K])
{
    // S = ((0 + L0) + L1) + ... in pass order, then the over-count term (mgm_core.cc:582-599): k_wta's operations, in its order
#pragma unroll
    for (int k = 0; k < K; k++) S[k] = 0.0f;
#pragma unroll
    for (int p = 0; p < MAXD; p++)
        if (p < ndir) {
#pragma unroll
            for (int k = 0; k < K; k++) S[k] = S[k] + l[p][k];
        }
    if (fix == 1) {
        const float f = (float)(ndir - 1);
#pragma unroll
        for (int k = 0; k < K; k++) S[k] = S[k] - f * c[k];
    }
}
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v)  // v of the lane CTRL names (every lane has one)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ float dpp_fmin(float v)  // min with the lane CTRL names
{
    return __builtin_fminf(v, dpp_f<CTRL>(v));
}
// over the eight lanes of a group: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
__device__ __forceinline__ float group_fmin(float v)
{
    v = dpp_fmin<0xB1>(v);
    v = dpp_fmin<0x4E>(v);
    return dpp_fmin<0x141>(v);
}
template <int CTRL>
__device__ __forceinline__ void dpp_take(float &best, int &bi)  // the smaller (S, label) of this lane's and that of the lane CTRL names
{
    const float ov = dpp_f<CTRL>(best);
    const int oi = __builtin_amdgcn_update_dpp(0, bi, CTRL, 0xf, 0xf, false);
    if (ov < best || (ov == best && oi < bi)) {
        best = ov;
        bi = oi;
    }
}
// PPW: groups of eight pixels per wave and iteration (their loads go out together): a wave takes 8 * PPW consecutive pixels per turn
// of its grid-stride loop.  ND: the number of passes, a compile-time constant (no test per pass around the loads).
template <int PPW, int ND>
__device__ __forceinline__ void wta_pruned(const WtaParams &P)
{
    constexpr int MAXD = ND;
    constexpr int L = 256;
    constexpr int NONE = 0x7fffffff;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = lane & 7;      // the chunk this lane owns in (a); its four labels 4j.. of the chunk its group reads in (b), (c)
    const int gsh = lane & ~7;   // first lane of its group: where the group's byte of a ballot starts
    const int ndir = ND, fix = P.FIX;
    const long long mstride = P.nvol / 32;  // chunk minima per pass
    unsigned nloaded = 0, npx = 0;          // (mgm_debug_wta_stats) of this wave
    const long long turn = (long long)gridDim.x * 4 * 8 * PPW;
    long long g0 = ((long long)blockIdx.x * 4 + wv) * (8 * PPW);
    // (a) the chunk's costs and minima, of the turn that starts at pixel g: asked for one turn ahead
    uint4 cq[PPW][2];
    float mn[PPW][MAXD];
    auto load_a = [&](const long long g) {
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            const long long q = g + 8 * u + (lane >> 3), px = q < P.npix ? q : P.npix - 1;
            const uint4 *cp = reinterpret_cast<const uint4 *>(P.C8 + px * L + j * 32);
            cq[u][0] = cp[0], cq[u][1] = cp[1];
#pragma unroll
            for (int p = 0; p < MAXD; p++)
                if (p < ndir) mn[u][p] = P.Lmin[(long long)p * mstride + px * (L / 32) + j];
        }
    };
    if (g0 < P.npix) load_a(g0);
    for (; g0 < P.npix; g0 += turn) {
        long long pix[PPW];
        bool own[PPW];  // the group's pixel exists (the groups past the last pixel repeat it and write nothing)
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            const long long q = g0 + 8 * u + (lane >> 3);
            own[u] = q < P.npix;
            pix[u] = own[u] ? q : P.npix - 1;
        }
        float clb[PPW];
        int seed[PPW];  // the seed chunk, -1: no label can hold a finite S
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            const unsigned w[8] = {cq[u][0].x, cq[u][0].y, cq[u][0].z, cq[u][0].w, cq[u][1].x, cq[u][1].y, cq[u][1].z, cq[u][1].w};
            unsigned m = 0;  // the chunk's largest finite cost + 1, 0: none
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int k = 0; k < 4; k++) m = max(m, (((w[i] >> (8 * k)) & 255u) + 1u) & 255u);  // (255, +INF, wraps to 0)
            float lm[MAXD][1], LB[1];
            const float cm[1] = {(float)((int)m - 1)};
#pragma unroll
            for (int p = 0; p < MAXD; p++) lm[p][0] = p < ndir ? mn[u][p] : 0.0f;
            sum_fix<MAXD>(lm, cm, ndir, fix, LB);
            const float lb = (m != 0u && LB[0] == LB[0]) ? LB[0] : f_inf();  // (a NaN bound drops out: S is NaN on those labels too)
            clb[u] = lb;
            const float gmin = group_fmin(lb);
            const unsigned at = (unsigned)(__builtin_amdgcn_ballot_w64(lb == gmin) >> gsh) & 255u;  // (never 0: gmin is one of them)
            seed[u] = gmin < f_inf() ? __builtin_ctz(at | 256u) : -1;
        }
        // cq and mn are consumed: the next turn's go out now and arrive behind (b), (c) and the stores of this one
        if (g0 + turn < P.npix) load_a(g0 + turn);
        // The group's eight lanes read chunk ck[u] of their pixel, lane j its labels 4j..: a 128-byte line per pass, the requests of all
        // passes (and pixels) back to back; then S of those four labels.  (chunk_S, loaded and consumed in one block, wherever one
        // round is in flight: what a lane would carry across a branch it sat out stays live for the whole loop.)
        auto chunk_load =[&](const int (&ck)[PPW], float (&l)[PPW][MAXD][4], unsigned (&cw)[PPW]) {
#pragma unroll
            for (int u = 0; u < PPW; u++) {
                const long long at = pix[u] * L + ck[u] * 32 + j * 4;
                cw[u] = *reinterpret_cast<const unsigned *>(P.C8 + at);
#pragma unroll
                for (int p = 0; p < MAXD; p++)
                    if (p < ndir) {
                        const float4 q = *reinterpret_cast<const float4 *>(P.Lr + (long long)p * P.nvol + at);
                        l[u][p][0] = q.x, l[u][p][1] = q.y, l[u][p][2] = q.z, l[u][p][3] = q.w;
                    }
            }
        };
        auto chunk_sum = [&](const float (&l)[PPW][MAXD][4], const unsigned (&cw)[PPW], float (&S)[PPW][4]) {
#pragma unroll
            for (int u = 0; u < PPW; u++) {
                float c[4];
#pragma unroll
                for (int k = 0; k < 4; k++) c[k] = c8_decode((cw[u] >> (8 * k)) & 255u);
                sum_fix<MAXD>(l[u], c, ndir, fix, S[u]);
            }
        };
        auto chunk_S = [&](const int (&ck)[PPW], float (&S)[PPW][4]) {
            float l[PPW][MAXD][4];
            unsigned cw[PPW];
            chunk_load(ck, l, cw);
            chunk_sum(l, cw, S);
        };
        // (b) the seed chunks
        float best[PPW];
        int bi[PPW], sck[PPW];
        unsigned cand[PPW];  // the chunks (c) still has to load, a bit each
        // S at the two labels beside the lane's best one, for vfit: kept whenever the lane takes a label -- its own values, or the
        // edge value of the lane beside it (row_shr:1, row_shl:1).  Lanes 0 and 7 of a group get another group's value for a label
        // that lies in another chunk, b % 32 == 0 or 31: (d) knows that from b and fetches S there from memory.
        float nlo[PPW], nhi[PPW];
        auto take = [&](const int u, const float (&S)[4], const int ck, const bool ties) {
            const float lo = dpp_f<0x111>(S[3]), hi = dpp_f<0x101>(S[0]);
#pragma unroll
            for (int k = 0; k < 4; k++) {  // ((c)'s chunks do not arrive by rising label: there the lower label wins a tie)
                const int o = ck * 32 + j * 4 + k;
                if (finite_bits(S[k]) && (S[k] < best[u] || (ties && S[k] == best[u] && o < bi[u]))) {
                    best[u] = S[k];
                    bi[u] = o;
                    nlo[u] = k > 0 ? S[k > 0 ? k - 1 : 0] : lo;
                    nhi[u] = k < 3 ? S[k < 3 ? k + 1 : 3] : hi;
                }
            }
        };
        {
            float S[PPW][4];
#pragma unroll
            for (int u = 0; u < PPW; u++) sck[u] = seed[u] > 0 ? seed[u] : 0;
            chunk_S(sck, S);
#pragma unroll
            for (int u = 0; u < PPW; u++) {
                best[u] = f_inf();
                bi[u] = NONE;
                nlo[u] = nhi[u] = 0.0f;
                if (seed[u] >= 0) take(u, S[u], seed[u], false);
                const float best0 = group_fmin(best[u]);
                // (c)'s set, fixed here: lane (g, j) speaks for chunk j of its pixel
                const bool cd = seed[u] >= 0 && j != seed[u] && clb[u] <= best0;
                const unsigned long long cdm = __builtin_amdgcn_ballot_w64(cd);
                cand[u] = (unsigned)(cdm >> gsh) & 255u;
                const unsigned long long ownm = __builtin_amdgcn_ballot_w64(own[u]);
                nloaded += (unsigned)__builtin_popcountll(cdm & ownm) + (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(own[u] && j == seed[u]));
                npx += (unsigned)__builtin_popcountll(ownm) >> 3;
            }
        }
        // (c) while any group has a candidate left: every group loads its lowest one; a group without any sits the round out under
        // the exec mask (with several pixels per group of lanes: one whose other pixel still has some reads its seed's line again).
        // One group of pixels per wave: the set is fixed, so the next round's loads go out BEFORE this round's are consumed -- two
        // rounds' registers, A and B, in turn (160 VGPRs at 8 passes; with two groups per wave that would be all 256).
        if constexpr (PPW == 1) {
            float lA[PPW][MAXD][4], lB[PPW][MAXD][4];
            unsigned cwA[PPW], cwB[PPW];
            int ckA[PPW], ckB[PPW];
            bool actA[PPW], actB[PPW];
            auto issue = [&](int (&ck)[PPW], bool (&act)[PPW], float (&l)[PPW][MAXD][4], unsigned (&cw)[PPW]) {
                bool more = false;
#pragma unroll
                for (int u = 0; u < PPW; u++) {
                    act[u] = cand[u] != 0u;
                    ck[u] = act[u] ? __builtin_ctz(cand[u]) : sck[u];
                    cand[u] &= cand[u] - 1u;
                    more = more || act[u];
                }
                if (!__builtin_amdgcn_ballot_w64(more)) return false;
                if (more) chunk_load(ck, l, cw);
                return true;
            };
            auto consume = [&](const int (&ck)[PPW], const bool (&act)[PPW], const float (&l)[PPW][MAXD][4], const unsigned (&cw)[PPW]) {
                float S[PPW][4];
                chunk_sum(l, cw, S);
#pragma unroll
                for (int u = 0; u < PPW; u++)
                    if (act[u]) take(u, S[u], ck[u], true);
            };
            if (issue(ckA, actA, lA, cwA))
                for (;;) {
                    const bool nb = issue(ckB, actB, lB, cwB);
                    consume(ckA, actA, lA, cwA);
                    if (!nb) break;
                    const bool na = issue(ckA, actA, lA, cwA);
                    consume(ckB, actB, lB, cwB);
                    if (!na) break;
                }
        } else {
            for (;;) {
                bool more = false;
#pragma unroll
                for (int u = 0; u < PPW; u++) more = more || cand[u] != 0u;
                if (!__builtin_amdgcn_ballot_w64(more)) break;
                if (more) {
                    int ck[PPW];
                    float S[PPW][4];
#pragma unroll
                    for (int u = 0; u < PPW; u++) ck[u] = cand[u] != 0u ? __builtin_ctz(cand[u]) : sck[u];
                    chunk_S(ck, S);
#pragma unroll
                    for (int u = 0; u < PPW; u++)
                        if (cand[u] != 0u) {
                            take(u, S[u], ck[u], true);
                            cand[u] &= cand[u] - 1u;
                        }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            // (d) first strict minimum among the finite entries by rising label: the group's smallest (S, label)
            const int mine = bi[u];
            dpp_take<0xB1>(best[u], bi[u]);
            dpp_take<0x4E>(best[u], bi[u]);
            dpp_take<0x141>(best[u], bi[u]);
            const int b = bi[u];
            // the lane that brought the winner writes the pixel: it holds S beside it (lane 0 where there is no winner)
            const bool writer = b == NONE ? j == 0 : mine == b;
            float outv, outc = best[u];
            if (b == NONE) outv = __builtin_nanf("");  // the reference leaves minP uninitialised here
            else outv = (float)(b + P.dmin);
            if (P.refine == 1) {  // (wave-uniform)
                const bool gate = b != NONE && b - 1 >= 0 && b + 2 <= L - 1;  // mgm_refine.h:58
                // a winner at the first or last label of its chunk: S beside it, in the next chunk, from memory, by sum_fix's operations
                // in its order (the same float) -- whether that chunk was loaded or not.  One ballot: most waves have none.
                const bool below = (b & 31) == 0, fetch = writer && gate && (below || (b & 31) == 31);
                if (__builtin_amdgcn_ballot_w64(fetch)) {
                    if (fetch) {
                        const long long at = pix[u] * L + (below ? b - 1 : b + 1);
                        float a = 0.0f;
#pragma unroll
                        for (int p = 0; p < MAXD; p++)
                            if (p < ndir) a = a + P.Lr[(long long)p * P.nvol + at];
                        if (fix == 1) a = a - (float)(ndir - 1) * c8_decode(P.C8[at]);
                        if (below) nlo[u] = a;
                        else nhi[u] = a;
                    }
                }
                if (gate) {
                    float vmin, dx;
                    vfit(nlo[u], best[u], nhi[u], vmin, dx);
                    outv = (float)(b + P.dmin) + dx;
                    outc = vmin;
                }
            }
            if (writer && own[u]) {
                P.out[pix[u]] = outv;
                P.outcost[pix[u]] = outc;
            }
        }
    }
    // one atomic per wave, spread over 64 words 128 bytes apart: one per wave ITERATION on one word (the first version) serialised
    // a million atomics on one address and took the kernel from 1.x to 12 ms
    if (P.stats && lane == 0) atomicAdd(P.stats + (blockIdx.x & 63) * 16, ((unsigned long long)npx << 32) | nloaded);
}
// MAXD: upper bound of NDIR (what the planner chooses the instance by); ALLD: NDIR == MAXD.  The other pass counts branch once, at
// the top, to a body of their own: a test per pass inside one body costs a scalar condition and an address per pass, more than the
// scalar registers hold.
template <int PPW, int MAXD, bool ALLD>
__global__ void __launch_bounds__(256) k_wta_pruned(const WtaParams P)
{
    if constexpr (ALLD) {
        wta_pruned<PPW, MAXD>(P);
    } else {
#define ND_CASE(N_)                                         \
    case N_:                                                \
        if constexpr (N_ < MAXD) wta_pruned<PPW, N_>(P);    \
        break;
        switch (P.NDIR) {  // (wave-uniform; a count the instance is not built for computes nothing: launch_wta never sends one)
            ND_CASE(1) ND_CASE(2) ND_CASE(3) ND_CASE(4) ND_CASE(5) ND_CASE(6) ND_CASE(7)
            default: break;
        }
#undef ND_CASE
    }
}

// The launch tables: from a choice of the planner (plan_wta, mgm_planner.h) to its instance.  Nothing is decided here; a choice
// that names no instance of its table, and the planner's refusals, are hipErrorInvalidValue.
static_assert(kWtaWidestLabels == kMaxLPL * 64, "plan_wta sends wider volumes to k_wta_any");
hipError_t launch_wta(const WtaParams &p, const WtaChoice &c, hipStream_t s)
{
    const dim3 grid((unsigned)c.grid), block(256);
#define WTA(LPL_, PPW_, EXACT_, MAXD_, SUB_)                                                                     \
    if (c.LPL == LPL_ && c.PPW == PPW_ && c.EXACT == EXACT_ && c.MAXD == MAXD_ && c.SUB == SUB_) {               \
        hipLaunchKernelGGL((k_wta<LPL_, PPW_, EXACT_ != 0, MAXD_, SUB_>), grid, block, 0, s, p);                 \
        return hipGetLastError();                                                                                \
    }
#define WTA_Q(LPL_, MAXD_)                                                                                       \
    if (c.LPL == LPL_ && c.MAXD == MAXD_) {                                                                      \
        hipLaunchKernelGGL((k_wta_q<64 * LPL_, MAXD_>), grid, block, 0, s, p);                                   \
        return hipGetLastError();                                                                                \
    }
#define WTA_PRUNED(PPW_, MAXD_, ALLD_)                                                                           \
    if (c.PPW == PPW_ && c.MAXD == MAXD_ && c.ALLD == ALLD_ && p.NDIR >= 1 && (ALLD_ ? p.NDIR == MAXD_ : p.NDIR < MAXD_)) { \
        hipLaunchKernelGGL((k_wta_pruned<PPW_, MAXD_, ALLD_ != 0>), grid, block, 0, s, p);                       \
        return hipGetLastError();                                                                                \
    }
    switch (c.family) {
        case kWtaPruned:  // (LPL 4: 256 labels) pixels per wave, directions it is built for, exactly that many
            if (!p.Lmin) break;
            WTA_PRUNED(2, 8, 1) WTA_PRUNED(1, 8, 1) WTA_PRUNED(2, 4, 1) WTA_PRUNED(1, 4, 1) WTA_PRUNED(1, 4, 0) WTA_PRUNED(1, 8, 0)
            break;
        case kWtaAny:  // beyond the widest k_wta instance
            hipLaunchKernelGGL(k_wta_any, grid, block, 0, s, p);
            return hipGetLastError();
        case kWtaQuad:  // 192 / 384 labels
            WTA_Q(3, 4) WTA_Q(3, 8) WTA_Q(6, 4) WTA_Q(6, 8)
            break;
        case kWtaPacked:  // 128 and 64 labels: two / four pixels per 256-float slab
            WTA(4, 4, 1, 4, 2) WTA(4, 2, 1, 8, 2) WTA(4, 4, 1, 4, 4) WTA(4, 2, 1, 8, 4)
            break;
        case kWtaPlain:  // per label width: at most 4 directions, up to 8, and the guarded instance of a stride with padding lanes
            WTA(1, 8, 1, 4, 1) WTA(1, 4, 1, 8, 1) WTA(1, 1, 0, 8, 1)
            WTA(2, 8, 1, 4, 1) WTA(2, 4, 1, 8, 1) WTA(2, 1, 0, 8, 1)
            WTA(3, 4, 1, 4, 1) WTA(3, 2, 1, 8, 1) WTA(3, 1, 0, 8, 1)
            WTA(4, 6, 1, 4, 1) WTA(4, 3, 1, 8, 1) WTA(4, 1, 0, 8, 1)
            WTA(6, 2, 1, 4, 1) WTA(6, 1, 1, 8, 1) WTA(6, 1, 0, 8, 1)
            WTA(8, 2, 1, 4, 1) WTA(8, 1, 1, 8, 1) WTA(8, 1, 0, 8, 1)
            // 513..2048 labels: one pixel per wave and iteration, guarded loads
            // (768 and 1024 labels exactly: the second pass-kernel build takes them since round 4, with compact costs)
            WTA(12, 1, 1, 8, 1) WTA(12, 1, 0, 8, 1)
            WTA(16, 1, 1, 8, 1) WTA(16, 1, 0, 8, 1)
            WTA(24, 1, 0, 8, 1)
            WTA(32, 1, 0, 8, 1)
            break;
        default: break;
    }
#undef WTA
#undef WTA_Q
#undef WTA_PRUNED
    return hipErrorInvalidValue;
}

// refine.h:40-68
__device__ __forceinline__ void parabolafit(const float (&v)[4], float &v_min, float &x_min)
{
    if (v[1] > v[0] && v[1] > v[2]) {
        x_min = 0;
        v_min = v[1];
        return;
    }
    const float c = v[1];
    const float b = (v[2] - v[0]) / 2;
    const float a = (v[2] - 2 * v[1] + v[0]) / 2;
    float x = -b / (2 * a);
    if (x > 1) x = 1;
    if (x < -1) x = -1;
    v_min = (a * x + b) * x + c;
    x_min = x;
}

// refine.h:6-38 (the doubling of a and b and the clamp of a are the reference's)
__device__ __forceinline__ void parabolafit_ocv(const float (&v)[4], float &v_min, float &x_min)
{
    if (v[1] > v[0] && v[1] > v[2]) {
        x_min = 0;
        v_min = v[1];
        return;
    }
    const float c = v[1];
    float b = (v[2] - v[0]) / 2;
    float a = (v[2] - 2 * v[1] + v[0]) / 2;
    a *= 2;
    b *= 2;
    a = a > 1.0 ? a : 1.0;
    float x = (-b + a) / (2 * a);
    if (x > 1) x = 1;
    if (x < -1) x = -1;
    v_min = (a * x + b) * x + c;
    x_min = x;
}

// refine.h:94-99: evaluated in double (the literals are doubles), narrowed on return
__device__ __forceinline__ float cubic_interp(const float (&p)[4], const float x)
{
    return p[1] + 0.5 * x *
                      (p[2] - p[0] + x * (2.0 * p[0] - 5.0 * p[1] + 4.0 * p[2] - p[3] + x * (3.0 * (p[1] - p[2]) + p[3] - p[0])));
}

// refine.h:102-145: p = {S[o-1], S[o], S[o+1], S[o+2]}; the cubic treats p[1]..p[2] as the unit interval
__device__ __forceinline__ void cubicfit(const float (&p)[4], float &out_pmin, float &out_xmin)
{
    float pmin, xmin;
    if (p[1] < p[2]) {
        pmin = p[1];
        xmin = 0.0;
    } else {
        pmin = p[2];
        xmin = 1.0;
    }
    const double a = 0.5 * 3.0 * (3.0 * (p[1] - p[2]) + p[3] - p[0]);
    const double b = 2.0 * p[0] - 5.0 * p[1] + 4.0 * p[2] - p[3];
    const double c = 0.5 * (p[2] - p[0]);
    const double discr = b * b - 4.0 * a * c;
    if (discr >= 0) {
        const double z1 = (-b + __builtin_sqrt(discr)) / (2.0 * a);
        const double z2 = (-b - __builtin_sqrt(discr)) / (2.0 * a);
        if (z1 > 0.0 && z1 < 1.0) {
            const float tmp = cubic_interp(p, z1);
            if (tmp < pmin) {
                pmin = tmp;
                xmin = z1;
            }
        }
        if (z2 > 0.0 && z2 < 1.0) {
            const float tmp = cubic_interp(p, z2);
            if (tmp < pmin) {
                pmin = tmp;
                xmin = z2;
            }
        }
    }
    out_pmin = pmin;
    out_xmin = xmin;
}

// K4-K6 on the RANGE-PROPORTIONAL layout (mgm_pass_rel.hip): one wavefront per pixel, one label slot per lane.  The same
// arithmetic and rules as k_wta / k_wta_any + k_refine on the dense hull -- S = ((0 + L0) + L1) + ... in pass order, the
// over-count term, the first strict minimum among the finite entries of the pixel's window scanned by rising disparity,
// the refinement gate of mgm_refine.h:58 on the window -- with "a disparity the pixel does not own" = `vout` (what the
// reference's S holds there: 0 - (NDIR-1)*INF, or 0 without the over-count fix) instead of a stored value.
// SPL, CB (round 6): label slots per lane (4 / 8: 64 / 128 slots per pixel) and bytes per cost code (1 / 2), as in k_pass_rel.
template <int SPL, int CB>
__global__ void __launch_bounds__(256) k_wta_rel(const WtaRelParams P)
{
    constexpr int SLOTS = 16 * SPL;
    // FOUR pixels per wave: a pixel's 64 slots on a row of 16 lanes, 4 per lane (16-byte loads; the first version had one slot per
    // lane, one pixel per wave: 4-byte loads and six LDS-crossbar rounds per pixel, 1.5 ms per 1920x1080 volume where its 4.4 GB ask for 0.7)
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, grp = lane >> 4;
    const float f = (float)(P.NDIR - 1);
    float vout = 0.0f;
    if (P.FIX == 1) vout = vout - f * f_inf();
    const bool vfin = finite_bits(vout);
    const long long nquads = (P.npix + 3) / 4;
    for (long long q4 = (long long)blockIdx.x * 4 + wv; q4 < nquads; q4 += (long long)gridDim.x * 4) {
        const long long pix0 = q4 * 4 + grp;
        const bool live = pix0 < P.npix;
        const long long pix = live ? pix0 : P.npix - 1;
        const int4 rec = reinterpret_cast<const int4 *>(P.base)[pix];  // (the pixel's record: disparity of slot 0, its own range)
        const int b = rec.x, lo = rec.y, hi = rec.z;
        const bool windowed = P.wlo != nullptr;
        const int wl = windowed ? (int)P.wlo[pix] : lo, wh = windowed ? (int)P.whi[pix] : hi;
        typedef float f4 __attribute__((ext_vector_type(4)));
        float a[SPL];
#pragma unroll
        for (int q = 0; q < SPL; q++) a[q] = 0.0f;
        for (int p = 0; p < P.NDIR; p++) {
#pragma unroll
            for (int h = 0; h < SPL / 4; h++) {
                const f4 t = reinterpret_cast<const f4 *>(P.Lr + (long long)p * P.nvol + pix * SLOTS + SPL * li)[h];
#pragma unroll
                for (int q = 0; q < 4; q++) a[4 * h + q] = a[4 * h + q] + t[q];
            }
        }
        if (P.FIX == 1) {
            constexpr int NWORD = SPL * CB / 4;
            unsigned cw[NWORD];
#pragma unroll
            for (int w = 0; w < NWORD; w++) cw[w] = reinterpret_cast<const unsigned *>(P.c8 + (pix * SLOTS + SPL * li) * CB)[w];
#pragma unroll
            for (int q = 0; q < SPL; q++)
                a[q] = a[q] - f * (CB == 1 ? c8_decode((cw[q / 4] >> (8 * (q % 4))) & 255u)
                                           : (CB == 2 ? c16_decode((cw[q / 2] >> (16 * (q % 2))) & 65535u) : __builtin_bit_cast(float, cw[q * CB / 4])));
        }
        float val[SPL];
        // (2) its own disparities inside the window: the first strict minimum by rising disparity = the smallest (value, disparity)
        float cb = f_inf();
        int ci = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < SPL; q++) {
            const int d = b + SPL * li + q;
            const bool own = d >= lo && d <= hi;
            val[q] = own ? a[q] : vout;
            if (own && d >= wl && d <= wh && finite_bits(val[q]) && val[q] < cb) {
                cb = val[q];
                ci = d;
            }
        }
        // butterfly over the row of 16 lanes: quad swaps, then the two mirrors
        dpp_take<0xB1>(cb, ci);
        dpp_take<0x4E>(cb, ci);
        dpp_take<0x141>(cb, ci);
        dpp_take<0x140>(cb, ci);
        // (1) the window's disparities below the pixel's own range: all `vout`, the first of them is the candidate
        float best = f_inf();
        int bi = 0x7fffffff;
        if (wl < lo && wl <= wh && vfin) {
            best = vout;
            bi = wl;
        }
        if (ci != 0x7fffffff && best > cb) {
            best = cb;
            bi = ci;
        }
        // (3) the window's disparities above the own range
        const int hi0 = wl > hi + 1 ? wl : hi + 1;
        if (wh > hi && hi0 <= wh && vfin && vout < best) {
            best = vout;
            bi = hi0;
        }
        float outv, outc = best;
        if (bi == 0x7fffffff) outv = __builtin_nanf("");  // the reference leaves minP uninitialised here
        else outv = (float)bi;
        // the four values around the minimum, from the lanes of the row that hold them (fetched whether or not they are used: every
        // lane takes part in the crossbar reads)
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int sl = (bi == 0x7fffffff ? b : bi) - 1 + k - b;  // slot of that disparity (row-uniform)
            const int e = sl & (SPL - 1);
            float mine = val[0];
#pragma unroll
            for (int q = 1; q < SPL; q++) mine = e == q ? val[q] : mine;
            const float x = __shfl(mine, (lane & 48) | ((sl / SPL) & 15));
            v[k] = (sl >= 0 && sl < SLOTS) ? x : vout;
        }
        if (P.refine >= 1 && bi != 0x7fffffff && bi - 1 >= wl && bi + 2 <= wh) {  // mgm_refine.h:58 (S allocated over the window)
            float vmin = outc, dx = 0;
            if (P.refine == 1) vfit(v[0], v[1], v[2], vmin, dx);
            else if (P.refine == 2) parabolafit(v, vmin, dx);
            else if (P.refine == 3) cubicfit(v, vmin, dx);
            else parabolafit_ocv(v, vmin, dx);
            outv = (float)bi + dx;
            outc = vmin;
        }
        if (li == 0 && live) {
            P.out[pix] = outv;
            P.outcost[pix] = outc;
        }
    }
}
// The corrected aggregated volume mgm() returns (mgm_core.cc:426, 582-601), on the dense hull, from the range-proportional Lr volumes
// (round 6): one thread per (pixel, label).  A label the pixel owns: S = ((0 + L0) + L1) + ... in pass order, minus (NDIR - 1) C
// with the over-count fix; a label it does not own holds what the dense-hull kernels leave there (C = +INF: +INF, or INF - INF =
// NaN with the fix) -- the reference's S has no such label.
__global__ void __launch_bounds__(256) k_rel_S(const WtaRelParams P, long long n, int L, int dmin, float *__restrict__ S)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const long long pix = t / L;
    const int d = dmin + (int)(t - pix * L);
    const int4 rec = reinterpret_cast<const int4 *>(P.base)[pix];
    const float f = (float)(P.NDIR - 1);
    float s = f_inf();
    if (d >= rec.y && d <= rec.z) {
        const long long k = pix * P.slots + (d - rec.x);
        s = 0.0f;
        for (int p = 0; p < P.NDIR; p++) s = s + P.Lr[(long long)p * P.nvol + k];
        if (P.FIX == 1)
            s = s - f * (P.cb == 1 ? c8_decode((unsigned)P.c8[k])
                                   : (P.cb == 2 ? c16_decode((unsigned)reinterpret_cast<const uint16_t *>(P.c8)[k]) : reinterpret_cast<const float *>(P.c8)[k]));
    } else if (P.FIX == 1)
        s = s - f * f_inf();
    S[t] = s;
}
hipError_t launch_rel_S(const WtaRelParams &p, int L, int dmin, float *S, hipStream_t s)
{
    const long long n = p.npix * L;
    hipLaunchKernelGGL(k_rel_S, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n, L, dmin, S);
    return hipGetLastError();
}
hipError_t launch_wta_rel(const WtaRelParams &p, hipStream_t s)
{
    const WtaRelChoice c = plan_wta_rel(WtaRelRequest{p.npix, p.num_cu, p.slots, p.cb});
    const dim3 grid((unsigned)c.grid);
#define WTA_REL(SPL_, CB_)                                                                \
    if (c.SPL == SPL_ && c.CB == CB_) {                                                   \
        hipLaunchKernelGGL((k_wta_rel<SPL_, CB_>), grid, dim3(256), 0, s, p);             \
        return hipGetLastError();                                                         \
    }
    WTA_REL(8, 4) WTA_REL(8, 2) WTA_REL(8, 1) WTA_REL(4, 4) WTA_REL(4, 2) WTA_REL(4, 1)
#undef WTA_REL
    return hipErrorInvalidValue;
}

// Stand-alone refinement on a materialised (corrected) S: one thread per pixel (subpixel_refinement_sgm,
// mgm_refine.h:40-70; method = index into its table: 1 vfit, 2 parabola, 3 cubic, 4 parabolaOCV).  With range
// images (wlo/whi, see WtaParams) the gate uses the pixel's window and disparities outside the volume read `vout`.
__global__ void __launch_bounds__(256) k_refine(const float *__restrict__ S, long long npix, int L, int dmin, int method,
                                                const float *__restrict__ wlo, const float *__restrict__ whi, float vout,
                                                float *__restrict__ out, float *__restrict__ outcost)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float minP = out[i];
    if (!(minP == minP)) return;  // NaN label (no finite S): undefined in the reference
    const int o = (int)minP;
    const int lo = wlo ? (int)wlo[i] : dmin, hi = whi ? (int)whi[i] : dmin + L - 1;
    if (o - 1 >= lo && o + 2 <= hi) {
        const float *Si = S + i * L;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int d = o - 1 + k - dmin;
            v[k] = (d >= 0 && d < L) ? Si[d] : vout;
        }
        float vmin = outcost[i], dx = 0;
        if (method == 1) vfit(v[0], v[1], v[2], vmin, dx);
        else if (method == 2) parabolafit(v, vmin, dx);
        else if (method == 3) cubicfit(v, vmin, dx);
        else parabolafit_ocv(v, vmin, dx);
        out[i] = (float)o + dx;
        outcost[i] = vmin;
    }
}

hipError_t launch_refine(const float *S, long long npix, int L, int dmin, int method, const float *wlo, const float *whi,
                         float vout, float *out, float *outcost, hipStream_t s)
{
    if (method < 1 || method > 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_refine, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, S, npix, L, dmin, method, wlo, whi, vout,
                       out, outcost);
    return hipGetLastError();
}

// ---- the right view's winners out of the LEFT run ("right from left") ----------------------------------------
// Right pixel xr with label e = -dmax..-dmin (index oR = e + dmax) names the match of left pixel x = xr + e with label index
// o = L-1-oR:  S_R(y, xr, oR) = S(y, xr + oR - dmax, L-1-oR), +INF where that left pixel lies outside the image.  The winner is the
// first strict minimum among the finite entries by rising oR (mgm_core.cc:592-609), vfit (refine.h:70-92) on the three entries
// around it under the gate of mgm_refine.h:58 in the right index.
__device__ __forceinline__ float right_cost_at(const WtaRightParams &P, long long i)
{
    if (!P.C8) return P.C[i];
    return P.cbytes == 2 ? c16_decode(reinterpret_cast<const unsigned short *>(P.C8)[i]) : c8_decode(P.C8[i]);
}
// one entry of S_R from memory: the pass volumes summed in pass order, then the over-count term -- k_wta's operations, in its order
__device__ __forceinline__ float right_S_at(const WtaRightParams &P, int y, int xr, int oR)
{
    const int x = xr + oR - P.dmax;
    if (x < 0 || x >= P.nx) return f_inf();
    const long long i = ((long long)y * P.nx + x) * P.Lk + (P.L - 1 - oR);
    float a = 0.0f;
    for (int p = 0; p < P.NDIR; p++) a = a + P.Lr[(long long)p * P.nvol + i];
    if (P.FIX == 1) a = a - (float)(P.NDIR - 1) * right_cost_at(P, i);
    return a;
}
// the two outputs of a right pixel whose winner is entry oR with value v1 (oR < 0: no finite entry)
__device__ __forceinline__ void right_emit(const WtaRightParams &P, int y, int xr, int oR, float v1)
{
    float outv = __builtin_nanf(""), outc = f_inf();  // as k_wta leaves a pixel without a finite entry
    if (oR >= 0) {
        outv = (float)(oR - P.dmax);
        outc = v1;
        if (P.refine == 1 && oR - 1 >= 0 && oR + 2 <= P.L - 1) {  // mgm_refine.h:58
            float vmin, dx;
            vfit(right_S_at(P, y, xr, oR - 1), v1, right_S_at(P, y, xr, oR + 1), vmin, dx);
            outv = (float)(oR - P.dmax) + dx;
            outc = vmin;
        }
    }
    const long long i = (long long)y * P.vnx + xr;
    P.out[i] = outv;
    P.outcost[i] = outc;
}

// STREAMING: the volume is read exactly as k_wta reads it -- a wave takes a left pixel, its 64*LPL label slots in registers, every
// stream a coalesced kilobyte -- and label o of left pixel x is handed to right pixel xr = x + dmin + o.  The running winners of the
// right pixels in flight live in an LDS ring of packed keys (ordered float bits << 32 | oR) combined with a 64-bit atomic minimum:
// the smallest key is the smallest value and, among equal values, the smallest oR -- the first strict minimum, whatever order the
// waves arrive in.  (S is never -0: a sum that starts from +0 cannot be, and neither can x - y; +0 and -0 would order apart.)
// One workgroup walks the left pixels xlo..xhi-1 that reach its segment [xr0, xr1) of one row in chunks of CH = 4*PPW; after the
// chunk that ends before xb, right pixels below xb + dmin are final.  One barrier per chunk: the ring holds L-1 + 2*CH entries, so
// finalising (and clearing) the entries of chunk i never meets the atomics of chunk i+1, and the barrier of chunk i+1 orders the
// clearing before chunk i+2 reuses the slots.  Label stride Lk == 64*LPL; labels L..Lk-1 are padding.
template <int LPL, int PPW>
__global__ void __launch_bounds__(256) k_wta_right(const WtaRightParams P)
{
    constexpr int CH = 4 * PPW;
    extern __shared__ unsigned long long ring[];  // P.ring entries (a power of two >= L-1 + 2*CH)
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int nseg = (P.vnx + P.seg - 1) / P.seg;
    const int y = blockIdx.x / nseg;
    const int xr0 = (blockIdx.x % nseg) * P.seg, xr1 = min(xr0 + P.seg, P.vnx);
    const int xlo = max(0, xr0 - P.dmax), xhi = min(P.nx, xr1 - P.dmin);  // the left pixels that reach the segment
    const unsigned mask = (unsigned)P.ring - 1u;
    const int o0 = lane * LPL;
    const bool c8 = P.C8 != nullptr;
    for (int i = tid; i < P.ring; i += 256) ring[i] = ~0ull;
    int fin = xr0;  // right pixels below it are written
    if (xlo < xhi) {
        // right pixels left of every match: no entry
        const int first = max(xr0, xlo + P.dmin);
        for (int xr = xr0 + tid; xr < first; xr += 256) right_emit(P, y, xr, -1, 0.0f);
        fin = first;
        __syncthreads();
        for (int xa = xlo; xa < xhi; xa += CH) {
            const int xb = min(xa + CH, xhi);
            float c[PPW][LPL], l[kMaxDirs][PPW][LPL];
#pragma unroll
            for (int u = 0; u < PPW; u++) {
                const int x = min(xa + wv * PPW + u, xhi - 1);
                const long long g = ((long long)y * P.nx + x) * (64 * LPL) + o0;
                if (P.FIX != 1) {
#pragma unroll
                    for (int k = 0; k < LPL; k++) c[u][k] = 0.0f;
                } else if (c8 && P.cbytes == 2) {
                    const unsigned short *q = reinterpret_cast<const unsigned short *>(P.C8) + g;
#pragma unroll
                    for (int k = 0; k < LPL; k++) c[u][k] = c16_decode(q[k]);
                } else if (c8) {
                    const uint8_t *q = P.C8 + g;
#pragma unroll
                    for (int k = 0; k < LPL; k++) c[u][k] = c8_decode(q[k]);
                } else {
                    const float *q = P.C + g;
#pragma unroll
                    for (int k = 0; k < LPL; k++) c[u][k] = q[k];
                }
            }
#pragma unroll
            for (int p = 0; p < kMaxDirs; p++) {
                if (p < P.NDIR) {
#pragma unroll
                    for (int u = 0; u < PPW; u++) {
                        const int x = min(xa + wv * PPW + u, xhi - 1);
                        const float *q = P.Lr + (long long)p * P.nvol + ((long long)y * P.nx + x) * (64 * LPL) + o0;
#pragma unroll
                        for (int k = 0; k < LPL; k++) l[p][u][k] = q[k];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < PPW; u++) {
                const int x = xa + wv * PPW + u;
                if (x >= xhi) break;
                // S = ((0 + L0) + L1) + ... in pass order, then the over-count term (mgm_core.cc:582-599)
                float S[LPL];
#pragma unroll
                for (int k = 0; k < LPL; k++) S[k] = 0.0f;
#pragma unroll
                for (int p = 0; p < kMaxDirs; p++) {
                    if (p < P.NDIR) {
#pragma unroll
                        for (int k = 0; k < LPL; k++) S[k] = S[k] + l[p][u][k];
                    }
                }
                if (P.FIX == 1) {
                    const float f = (float)(P.NDIR - 1);
#pragma unroll
                    for (int k = 0; k < LPL; k++) S[k] = S[k] - f * c[u][k];
                }
#pragma unroll
                for (int k = 0; k < LPL; k++) {
                    const int o = o0 + k, xr = x + P.dmin + o;
                    if (o < P.L && xr >= xr0 && xr < xr1 && finite_bits(S[k])) {
                        const unsigned long long key = ((unsigned long long)f2ord(S[k]) << 32) | (unsigned)(P.L - 1 - o);
                        atomicMin(&ring[(unsigned)xr & mask], key);
                    }
                }
            }
            __syncthreads();
            // final now: every right pixel whose last left pixel, xr - dmin, has passed; after the last chunk all that were reached
            const int fe = min(xr1, xb == xhi ? xhi + P.dmax : xb + P.dmin);
            for (int i = lane * 4 + wv; fin + i < fe; i += 256) {  // (spread over the waves: vfit fetches from memory)
                const int xr = fin + i;
                const unsigned long long key = ring[(unsigned)xr & mask];
                ring[(unsigned)xr & mask] = ~0ull;
                if (key == ~0ull) right_emit(P, y, xr, -1, 0.0f);
                else right_emit(P, y, xr, (int)(unsigned)key, ord2f((unsigned)(key >> 32)));
            }
            fin = max(fin, fe);
        }
    }
    // right pixels right of every match (or a segment no left pixel reaches)
    for (int xr = fin + tid; xr < xr1; xr += 256) right_emit(P, y, xr, -1, 0.0f);
}

// Any label count and label stride: one wavefront per right pixel walks its diagonal in memory, the entries strided over the lanes.
// The same arithmetic and rules; nothing here is tuned (a wave touches one line per entry).
__global__ void __launch_bounds__(256) k_wta_right_any(const WtaRightParams P)
{
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long npix = (long long)P.vnx * P.ny;
    for (long long pix = (long long)blockIdx.x * 4 + wv; pix < npix; pix += (long long)gridDim.x * 4) {
        const int y = (int)(pix / P.vnx), xr = (int)(pix % P.vnx);
        float best = f_inf();
        int bi = 0x7fffffff;
        for (int oR = lane; oR < P.L; oR += 64) {
            const float v = right_S_at(P, y, xr, oR);
            if (finite_bits(v) && best > v) {
                best = v;
                bi = oR;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(best, d);
            const int oi = __shfl_xor(bi, d);
            if (ov < best || (ov == best && oi < bi)) {
                best = ov;
                bi = oi;
            }
        }
        if (lane == 0) right_emit(P, y, xr, bi == 0x7fffffff ? -1 : bi, best);
    }
}

hipError_t launch_wta_right(const WtaRightParams &p0, const WtaRightChoice &c, hipStream_t s)
{
    const dim3 grid((unsigned)c.grid), block(256);
    if (c.family == kRightDiagonal) {
        hipLaunchKernelGGL(k_wta_right_any, grid, block, 0, s, p0);
        return hipGetLastError();
    }
    if (c.family != kRightStream) return hipErrorInvalidValue;
    WtaRightParams p = p0;
    p.seg = c.seg;
    p.ring = c.ring;
    const size_t lds = sizeof(unsigned long long) * (size_t)c.ring;
#define WTA_RIGHT(LPL_, PPW_)                                                             \
    if (c.LPL == LPL_ && c.PPW == PPW_) {                                                 \
        hipLaunchKernelGGL((k_wta_right<LPL_, PPW_>), grid, block, lds, s, p);            \
        return hipGetLastError();                                                         \
    }
    WTA_RIGHT(1, 2) WTA_RIGHT(2, 2) WTA_RIGHT(3, 2) WTA_RIGHT(4, 2) WTA_RIGHT(6, 1) WTA_RIGHT(8, 1) WTA_RIGHT(12, 1) WTA_RIGHT(16, 1)
#undef WTA_RIGHT
    return hipErrorInvalidValue;
}

// ---- the runner-up search -------------------------------------------------------------------------------------
// Per pixel: the winner (o1, S(o1)) exactly as k_wta finds it without refinement -- the first strict minimum among the finite
// entries by rising o (mgm_core.cc:592-609) -- and the runner-up (o2, S(o2)): the first strict minimum among the finite entries
// with |o - o1| > radius.  No winner, or no such entry: NaN label, +INF cost.
// the smaller (S, label) over the wave, in every lane
__device__ __forceinline__ void wave_take(float &best, int &bi)
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
__device__ __forceinline__ void runnerup_emit(const WtaRunnerupParams &P, long long pix, float v1, int o1, float v2, int o2)
{
    constexpr int NONE = 0x7fffffff;
    P.out2[pix] = o2 == NONE ? __builtin_nanf("") : (float)(o2 + P.dmin);
    P.cost2[pix] = v2;
    if (P.out1) P.out1[pix] = o1 == NONE ? __builtin_nanf("") : (float)(o1 + P.dmin);
    if (P.cost1) P.cost1[pix] = v1;
}

// STREAMING: the volume is read exactly as k_wta reads it -- one wave per pixel, its 64*LPL label slots in registers, every stream
// a coalesced slab, PPW pixels requested before the first is consumed -- and the slots are scanned twice: for the winner, then,
// with the winner known to every lane, for the best entry outside its exclusion zone.  Label stride Lk == 64*LPL; slots L..Lk-1
// are padding and never candidates.  No LDS, no atomics, no barriers: a wave never waits on another.
template <int LPL, int PPW, int MAXD>
__global__ void __launch_bounds__(256) k_wta_runnerup(const WtaRunnerupParams P)
{
    constexpr int NONE = 0x7fffffff;
    constexpr int LP = LPL * 64;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o0 = lane * LPL;
    const bool c8 = P.C8 != nullptr;
    // grid-stride over groups of PPW consecutive pixels
    for (long long g0 = ((long long)blockIdx.x * 4 + wv) * PPW; g0 < P.npix; g0 += (long long)gridDim.x * 4 * PPW) {
        float c[PPW][LPL], l[MAXD][PPW][LPL];
#pragma unroll
        for (int u = 0; u < PPW; u++) {
            const long long g = g0 + u < P.npix ? g0 + u : P.npix - 1;
            if (P.FIX != 1) {  // (the costs are not read)
#pragma unroll
                for (int k = 0; k < LPL; k++) c[u][k] = 0.0f;
            } else if (c8 && P.cbytes == 2) {
                const unsigned short *q = reinterpret_cast<const unsigned short *>(P.C8) + g * LP + o0;
#pragma unroll
                for (int k = 0; k < LPL; k++) c[u][k] = c16_decode(q[k]);
            } else if (c8) {
                const uint8_t *q = P.C8 + g * LP + o0;
#pragma unroll
                for (int k = 0; k < LPL; k++) c[u][k] = c8_decode(q[k]);
            } else {
                const float *q = P.C + g * LP + o0;
#pragma unroll
                for (int k = 0; k < LPL; k++) c[u][k] = q[k];
            }
        }
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
            // S = ((0 + L0) + L1) + ... in pass order, then the over-count term (mgm_core.cc:582-599): k_wta's operations, in its order
            float S[LPL];
#pragma unroll
            for (int k = 0; k < LPL; k++) S[k] = 0.0f;
#pragma unroll
            for (int p = 0; p < MAXD; p++) {
                if (p < P.NDIR) {
#pragma unroll
                    for (int k = 0; k < LPL; k++) S[k] = S[k] + l[p][u][k];
                }
            }
            if (P.FIX == 1) {
                const float f = (float)(P.NDIR - 1);
#pragma unroll
                for (int k = 0; k < LPL; k++) S[k] = S[k] - f * c[u][k];
            }
            // the winner: first strict minimum among the finite entries, ascending o
            float v1 = f_inf();
            int o1 = NONE;
#pragma unroll
            for (int k = 0; k < LPL; k++) {
                const float v = S[k];
                if (o0 + k < P.L && finite_bits(v) && v1 > v) {
                    v1 = v;
                    o1 = o0 + k;
                }
            }
            wave_take(v1, o1);
            // the runner-up: the same scan over the entries outside [o1 - radius, o1 + radius] (none without a winner)
            float v2 = f_inf();
            int o2 = NONE;
            if (o1 != NONE) {  // (wave-uniform)
                const int zl = o1 - P.radius, zh = o1 + P.radius;
#pragma unroll
                for (int k = 0; k < LPL; k++) {
                    const float v = S[k];
                    if (o0 + k < P.L && (o0 + k < zl || o0 + k > zh) && finite_bits(v) && v2 > v) {
                        v2 = v;
                        o2 = o0 + k;
                    }
                }
            }
            wave_take(v2, o2);
            if (lane == 0) runnerup_emit(P, g0 + u, v1, o1, v2, o2);
        }
    }
}

// Any label count and label stride (strides that are no multiple of 64, more than 1024 labels): one wavefront per pixel, the labels
// strided over the lanes; the second pass recomputes every entry from memory by the same operations.  Nothing here is tuned.
__global__ void __launch_bounds__(256) k_wta_runnerup_any(const WtaRunnerupParams P)
{
    constexpr int NONE = 0x7fffffff;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float f = (float)(P.NDIR - 1);
    for (long long pix = (long long)blockIdx.x * 4 + wv; pix < P.npix; pix += (long long)gridDim.x * 4) {
        auto S_at = [&](int o) {
            const long long i = pix * P.Lk + o;
            float a = 0.0f;
            for (int p = 0; p < P.NDIR; p++) a = a + P.Lr[(long long)p * P.nvol + i];
            if (P.FIX == 1)
                a = a - f * (!P.C8 ? P.C[i] : (P.cbytes == 2 ? c16_decode(reinterpret_cast<const unsigned short *>(P.C8)[i]) : c8_decode(P.C8[i])));
            return a;
        };
        float v1 = f_inf();
        int o1 = NONE;
        for (int o = lane; o < P.L; o += 64) {
            const float v = S_at(o);
            if (finite_bits(v) && v1 > v) {
                v1 = v;
                o1 = o;
            }
        }
        wave_take(v1, o1);
        float v2 = f_inf();
        int o2 = NONE;
        if (o1 != NONE) {  // (wave-uniform)
            const int zl = o1 - P.radius, zh = o1 + P.radius;
            for (int o = lane; o < P.L; o += 64) {
                if (o >= zl && o <= zh) continue;
                const float v = S_at(o);
                if (finite_bits(v) && v2 > v) {
                    v2 = v;
                    o2 = o;
                }
            }
        }
        wave_take(v2, o2);
        if (lane == 0) runnerup_emit(P, pix, v1, o1, v2, o2);
    }
}

// from a choice of the planner (plan_wta_runnerup) to its instance; anything else is hipErrorInvalidValue
hipError_t launch_wta_runnerup(const WtaRunnerupParams &p, const RunnerupChoice &c, hipStream_t s)
{
    if (c.grid < 1 || p.radius < 0 || p.L < 1 || p.Lk < p.L || p.npix < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)c.grid), block(256);
    if (c.family == kRunnerupAny) {
        hipLaunchKernelGGL(k_wta_runnerup_any, grid, block, 0, s, p);
        return hipGetLastError();
    }
    if (c.family != kRunnerupStream || p.Lk != 64 * c.LPL || p.NDIR > c.MAXD) return hipErrorInvalidValue;
#define RUNNERUP(LPL_, PPW_, MAXD_)                                                       \
    if (c.LPL == LPL_ && c.PPW == PPW_ && c.MAXD == MAXD_) {                              \
        hipLaunchKernelGGL((k_wta_runnerup<LPL_, PPW_, MAXD_>), grid, block, 0, s, p);    \
        return hipGetLastError();                                                         \
    }
    RUNNERUP(1, 8, 4) RUNNERUP(1, 4, 8) RUNNERUP(2, 8, 4) RUNNERUP(2, 4, 8) RUNNERUP(3, 4, 4) RUNNERUP(3, 2, 8) RUNNERUP(4, 6, 4) RUNNERUP(4, 3, 8)
    RUNNERUP(6, 2, 4) RUNNERUP(6, 1, 8) RUNNERUP(8, 2, 4) RUNNERUP(8, 1, 8) RUNNERUP(12, 1, 8) RUNNERUP(16, 1, 8)
#undef RUNNERUP
    return hipErrorInvalidValue;
}

}  // namespace mgm
