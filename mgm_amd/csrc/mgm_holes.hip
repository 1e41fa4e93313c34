// mgm_holes.hip -- hole filling (this project's own step, the reference has none): every non-finite pixel of a
// finished disparity map takes the median / minimum / maximum of the nearest finite pixels along 2, 4 or 8 rays.
//
//   valid pixel   d(p) finite; NaN and +-INF pixels are holes
//   directions    0 (+1,0)  1 (-1,0)  2 (0,+1)  3 (0,-1)  4 (+1,+1)  5 (-1,+1)  6 (+1,-1)  7 (-1,-1); `dirs` takes the first 2, 4 or 8
//   candidate     c_k(p) = d(p + t * step_k) for the smallest t >= 1 at which that pixel is inside the image and valid; none when
//                 the ray leaves the image first, or when maxdist > 0 and t > maxdist.  Rays read the ORIGINAL map and pass over holes
//   fill value    the n >= 1 candidates ordered by (value, direction index), the IEEE comparison on the values (so the direction
//                 decides between -0 and +0): min v[0], max v[n-1], median v[n/2] (the upper median)
//   out(p)        = d(p) bit for bit on valid pixels and on holes without a candidate, else the fill value: always one of the
//                 input's values, no float arithmetic anywhere;   filled(p) = 1 where a hole received a value, else 0
//
// The work is O(pixels x dirs) whatever the holes look like: no ray is marched.  Per direction ONE sweep along every line carries
// "the last valid pixel seen: its value and where it was", and a hole's candidate is that pixel, t = the difference of the two
// positions (an int32 subtraction of coordinates: no counter that could overflow on a long line).  Launches, each a phase that
// the next one sees finished:
//
//   k_holes_rows    directions 0, 1: one wave per (row, direction), 64 pixels at a time.  Inside a chunk the nearest valid lane is
//                   found with one ballot and a count of leading / trailing zeros, its value with one cross-lane read; the carry from
//                   the chunks before is wave-uniform
//   k_holes_carry   directions 2..7: one lane per column or diagonal, one band of rows per workgroup row: the band's LAST valid
//                   pixel in walking order on every line (its row, its value), which does not depend on what came before the band
//   k_holes_walk    the same lanes and bands: the carry-in is the nearest earlier band's carry-out that has one, then the band is
//                   walked row by row.  At every row the lanes of a wave read consecutive x
//   k_holes_apply   one thread per pixel: a valid pixel copies, a hole gathers its candidates, orders them with a fixed
//                   compare-exchange network and writes out / filled
// (These are the phases' names in the timing table; k_holes_carry and k_holes_walk are the two instances of k_holes_lines.)
//
// Candidate planes are written at holes only (every hole, every direction: NaN where there is none) and read at holes only.
// No loop here waits for a value that another wave must produce: no flag, no atomic, no barrier across workgroups.
//
// Hole classification lives here too: k_holes_classify tells occlusions from mismatches with the other view's map,
// and the classified instances of k_holes_apply fill each class by its own rule; both are described where they stand.
#include "mgm_device.h"
#include "mgm_planner.h"

namespace mgm {

__device__ __forceinline__ float holes_none() { return __builtin_nanf(""); }
__device__ __forceinline__ bool holes_near(int t, int maxdist) { return maxdist == 0 || t <= maxdist; }

// One wave per (row, direction): direction 1 looks LEFT (the source has the smaller x), so its sweep runs over the chunks from the
// left; direction 0 looks right and runs from the right.  U chunks are loaded before the first of them is looked at: the loads
// depend on no carry.
__global__ void __launch_bounds__(kHolesThreads) k_holes_rows(const float *__restrict__ d, int nx, int ny, int maxdist, float *__restrict__ planes)
{
    constexpr int U = 4;
    static_assert(kHolesChunk == kWave, "one pixel per lane");
    const long long w = (long long)blockIdx.x * (kHolesThreads / kWave) + (threadIdx.x >> 6);
    if (w >= 2ll * ny) return;
    const int k = (int)(w & 1), lane = threadIdx.x & 63;
    const long long y = w >> 1;
    const float *row = d + y * nx;
    float *cand = planes + (long long)k * nx * ny + y * nx;
    const int nchunks = (int)(((long long)nx + kHolesChunk - 1) / kHolesChunk);
    bool has = false;  // the carry: wave-uniform
    int cx = 0;
    float cv = 0.0f;
    for (int i0 = 0; i0 < nchunks; i0 += U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = i0 + u, c = k ? i : nchunks - 1 - i;
            const long long x = (long long)c * kHolesChunk + lane;
            const bool in = i < nchunks && x < nx;
            const float r = row[in ? x : 0];
            v[u] = in ? r : holes_none();
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = i0 + u, c = k ? i : nchunks - 1 - i;
            const long long x = (long long)c * kHolesChunk + lane;
            const bool in = i < nchunks && x < nx;
            const bool valid = in && finite_bits(v[u]);
            const unsigned long long mask = __ballot(valid);
            // the valid lanes on the side this direction looks at, and the nearest of them
            const unsigned long long side = k ? mask & ((1ull << lane) - 1) : mask & ~((2ull << lane) - 1);
            const int j = (k ? 63 - __clzll((long long)side) : __ffsll((long long)side) - 1) & 63;
            float sv = __shfl(v[u], j);  // (every lane takes part, whether it has a source or not)
            int t = k ? lane - j : j - lane;
            bool found = side != 0;
            if (!found && has) {
                sv = cv;
                t = k ? (int)(x - cx) : (int)(cx - x);
                found = true;
            }
            if (in && !valid) cand[x] = (found && holes_near(t, maxdist)) ? sv : holes_none();
            if (mask) {  // the chunk's last valid lane in sweep order is the next chunk's carry
                const int jj = k ? 63 - __clzll((long long)mask) : __ffsll((long long)mask) - 1;
                cx = c * kHolesChunk + jj;
                cv = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v[u]), __builtin_amdgcn_readfirstlane(jj)));
                has = true;
            }
        }
    }
}

// Directions 2..7, one lane per line l: x(y) = l + off + slope * y.  Columns: x = l (the lanes l >= nx have no pixel); the diagonals
// of directions 4 and 7: x - y = l - (ny - 1); those of 5 and 6: x + y = l.  `up`: the source lies at the smaller y, the walk runs
// with growing y (directions 3, 6, 7); else it starts at the band's last row.
struct HolesLine {
    long long off;
    int slope;
    bool up;
};
__device__ __forceinline__ HolesLine holes_line(int k, int ny)
{
    const int slope = (k == 4 || k == 7) ? 1 : ((k == 5 || k == 6) ? -1 : 0);
    return HolesLine{slope == 1 ? -(long long)(ny - 1) : 0ll, slope, k == 3 || k == 6 || k == 7};
}

// blockIdx: x along the lines, y the band, z the direction - 2.  WALK = false: only the band's carry-out is found and written;
// WALK = true: carry-in from the bands before, then the candidates of the band's holes.
template <bool WALK>
__global__ void __launch_bounds__(kHolesThreads) k_holes_lines(const float *__restrict__ d, int nx, int ny, int maxdist, int band, int nbands,
                                                              long long nlines, int *__restrict__ cpos, float *__restrict__ cval,
                                                              float *__restrict__ planes)
{
    const long long l = (long long)blockIdx.x * kHolesThreads + threadIdx.x;
    if (l >= nlines) return;
    const int b = blockIdx.y, k = 2 + blockIdx.z;
    const HolesLine g = holes_line(k, ny);
    const int y0 = (int)((long long)b * band), y1 = (int)min((long long)ny, (long long)y0 + band);  // rows [y0, y1)
    const long long slot = (long long)(k - 2) * nbands * nlines + l;                                  // + band * nlines
    int cy = -1;  // the carry: the row of the last valid pixel seen on this line, its value
    float cv = 0.0f;
    if (WALK)
        for (int bb = g.up ? b - 1 : b + 1; cy < 0 && bb >= 0 && bb < nbands; bb += g.up ? -1 : 1) {
            cy = cpos[slot + bb * nlines];
            cv = cval[slot + bb * nlines];
        }
    float *cand = planes + (long long)k * nx * ny;
    // U rows are loaded before the first of them is looked at: the loads depend on no carry
    constexpr int U = 8;
    const int n = y1 - y0;
    for (int s0 = 0; s0 < n; s0 += U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int y = g.up ? y0 + s0 + u : y1 - 1 - s0 - u;
            const long long x = l + g.off + (long long)g.slope * y;
            v[u] = (s0 + u < n && x >= 0 && x < nx) ? d[(long long)y * nx + x] : holes_none();
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int y = g.up ? y0 + s0 + u : y1 - 1 - s0 - u;
            const long long x = l + g.off + (long long)g.slope * y;
            if (!(s0 + u < n && x >= 0 && x < nx)) continue;
            if (finite_bits(v[u])) {
                cy = y;
                cv = v[u];
            } else if (WALK) cand[(long long)y * nx + x] = (cy >= 0 && holes_near(g.up ? y - cy : cy - y, maxdist)) ? cv : holes_none();
        }
    }
    if (!WALK) {
        cpos[slot + b * nlines] = cy;
        cval[slot + b * nlines] = cv;
    }
}

// a before b in the order of the fill value: by value, equal values by direction index; a missing candidate (NaN) after all others
__device__ __forceinline__ bool holes_before(float a, int ia, float b, int ib)
{
    return finite_bits(a) && (!finite_bits(b) || a < b || (a == b && ia < ib));
}
__device__ __forceinline__ void holes_cx(float &a, int &ia, float &b, int &ib)
{
    if (holes_before(b, ib, a, ia)) {
        const float t = a;
        const int it = ia;
        a = b, ia = ib, b = t, ib = it;
    }
}

// d[p] is read before out[p] is written and the candidates are finished: out may be d (no __restrict__ on either).
// CLS, the classified instance: a hole with cls(p) == 1.0f (an occlusion) takes mode_occ, every other hole `mode`,
// whatever else cls holds there; the modes 3 seclow v[min(1, n-1)] and 4 sechigh v[max(n-2, 0)] exist for it.  cls is read at holes
// only, and like d before out[p] is written.  Without CLS neither cls nor mode_occ is looked at.
template <int DIRS, bool CLS>
__global__ void __launch_bounds__(kHolesThreads) k_holes_apply(const float *d, long long npix, const float *__restrict__ planes, int mode,
                                                              float *out, float *__restrict__ filled, const float *cls, int mode_occ)
{
    static_assert(DIRS == 2 || DIRS == 4 || DIRS == 8, "the compare-exchange networks below");
    const long long p = (long long)blockIdx.x * kHolesThreads + threadIdx.x;
    if (p >= npix) return;
    const float v = d[p];
    float r = v;
    int n = 0;
    if (!finite_bits(v)) {
        float c[DIRS];
        int id[DIRS];
#pragma unroll
        for (int k = 0; k < DIRS; k++) {
            c[k] = planes[k * npix + p];
            id[k] = k;
            n += finite_bits(c[k]) ? 1 : 0;
        }
#define CX(i, j) holes_cx(c[i], id[i], c[j], id[j])
        if (DIRS == 2) CX(0, 1);
        if (DIRS == 4) CX(0, 1), CX(2, 3), CX(0, 2), CX(1, 3), CX(1, 2);
        if (DIRS == 8) {  // Batcher's odd-even merge sort, 19 compare-exchanges
            CX(0, 1), CX(2, 3), CX(4, 5), CX(6, 7);
            CX(0, 2), CX(1, 3), CX(4, 6), CX(5, 7);
            CX(1, 2), CX(5, 6);
            CX(0, 4), CX(1, 5), CX(2, 6), CX(3, 7);
            CX(2, 4), CX(3, 5);
            CX(1, 2), CX(3, 4), CX(5, 6);
        }
#undef CX
        int pick = mode == 1 ? 0 : (mode == 2 ? n - 1 : n / 2);
        if (CLS) {
            const int m = cls[p] == 1.0f ? mode_occ : mode;
            pick = m == 1 ? 0 : (m == 2 ? n - 1 : (m == 3 ? min(1, n - 1) : (m == 4 ? max(n - 2, 0) : n / 2)));
        }
#pragma unroll
        for (int k = 0; k < DIRS; k++)
            if (k == pick && n > 0) r = c[k];
    }
    if (out) out[p] = r;
    if (filled) filled[p] = n > 0 ? 1.0f : 0.0f;
}

// Hole classification: cls = 0 on finite pixels; a hole at (x, y) is a mismatch (2) iff a column xr of the other view
// with max(0, x + dmin) <= xr <= min(vnx - 1, x + dmax) has other(xr, y) finite and fabsf(((float)xr + other(xr, y)) - (float)x) <= tau
// -- some pixel of the other view points back at it -- else an occlusion (1).  In float, in that order (this file is built without
// contraction); a landing coordinate (float)xr + other that overflows to +-INF, like a NaN, matches nothing.
//
// One workgroup per row segment of `seg` = kHolesThreads pixels, one pixel per thread; blockIdx.y strides over the rows.
//   1. every thread reads its pixel; the segment's holes are compacted into an LDS list with one ballot per wave and the waves'
//      counts (a segment without holes writes its zeros and is done)
//   2. the columns the segment's holes can name, [x0 + dmin, x1 + dmax] cut to the other view, are staged in LDS as landing
//      coordinates, `span` at a time (NaN where other is not finite): both maps are read once per segment, whatever L is
//   3. wave w takes the holes w, w + waves, ... one at a time: 64 columns per step, one LDS read and one ballot per step, and it leaves
//      the hole at the first step with a match; a matched hole is marked in the list (its entry turns negative) and skipped in later spans
//   4. every thread looks its hole up in the list by the rank it got in 1. and writes its class
// No atomics, nothing waits on another workgroup; the barriers are the workgroup's own, reached by all its threads (every loop bound
// below is uniform across the workgroup).
__global__ void __launch_bounds__(kHolesThreads) k_holes_classify(const float *__restrict__ d, int nx, int ny, const float *__restrict__ other, int vnx,
                                                                 int dmin, int dmax, float tau, int span, float *__restrict__ cls)
{
    extern __shared__ float holes_cls_lds[];
    constexpr int W = kHolesThreads / kWave;
    static_assert(W <= kHolesClsWords, "one count per wave");
    float *land = holes_cls_lds;                   // [span]
    int *list = (int *)(holes_cls_lds + span);     // [kHolesThreads] the holes' x - x0; -1 - (x - x0) once matched
    int *count = list + kHolesThreads;             // [W] holes per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long x0 = (long long)blockIdx.x * kHolesThreads, x = x0 + threadIdx.x;
    const long long x1 = min(x0 + kHolesThreads, (long long)nx) - 1;  // the segment's last pixel
    // the columns of the other view that the segment's holes can name (empty when lo_all > hi_all: every hole is an occlusion)
    const long long lo_all = max(0ll, x0 + dmin), hi_all = min((long long)vnx - 1, x1 + dmax);
    for (long long y = blockIdx.y; y < ny; y += gridDim.y) {
        const bool in = x < nx;
        const float v = d[in ? y * nx + x : 0];
        const bool hole = in && !finite_bits(v);
        const unsigned long long mask = __ballot(hole);
        if (lane == 0) count[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, nholes = 0;
#pragma unroll
        for (int w = 0; w < W; w++) {
            const int cw = count[w];
            before += w < wave ? cw : 0;
            nholes += cw;
        }
        const int rank = before + __popcll(mask & ((1ull << lane) - 1));
        if (hole) list[rank] = threadIdx.x;
        __syncthreads();  // (the list is complete, and everyone has read count[])
        if (nholes > 0) {
            for (long long s0 = lo_all; s0 <= hi_all; s0 += span) {
                const long long s1 = min(s0 + span - 1, hi_all);  // the span's columns [s0, s1], all inside the other view
                for (long long xr = s0 + threadIdx.x; xr <= s1; xr += kHolesThreads) {
                    const float o = other[y * vnx + xr];
                    land[xr - s0] = finite_bits(o) ? (float)xr + o : holes_none();
                }
                __syncthreads();
                for (int h = wave; h < nholes; h += W) {
                    const int e = list[h];  // wave-uniform
                    if (e < 0) continue;
                    const long long hx = x0 + e;
                    const float fx = (float)hx;
                    const long long lo = max(hx + dmin, s0), hi = min(hx + dmax, s1);
                    bool matched = false;
                    for (long long j0 = lo; j0 <= hi && !matched; j0 += kWave) {
                        const long long j = j0 + lane;
                        const float a = land[j <= hi ? j - s0 : 0];
                        matched = __ballot(j <= hi && fabsf(a - fx) <= tau) != 0;
                    }
                    if (matched && lane == 0) list[h] = -1 - e;
                }
                __syncthreads();  // (the span is done with: land may be overwritten; the marks are visible)
            }
        }
        if (in) cls[y * nx + x] = hole ? (list[rank] < 0 ? 2.0f : 1.0f) : 0.0f;
        // No barrier before the next row: a thread that runs ahead writes only count[], which nobody reads any more after the row's
        // second barrier, and reaches no write of list or land before the next row's first barrier -- which every thread passes only
        // after it has read its list entry above.
    }
}

const char *holes_phase_name(int phase)
{
    static const char *const names[kHolesPhases] = {"k_holes_rows", "k_holes_carry", "k_holes_walk", "k_holes_apply"};
    return phase >= 0 && phase < kHolesPhases ? names[phase] : "";
}

// A table from the planner's choice to the launch: the grids and the band are the choice's, `dirs` selects the instance of k_holes_apply.
hipError_t launch_holes_phase(int phase, const HolesParams &p, const HolesChoice &c, hipStream_t s)
{
    if (c.family != kHolesLines || c.chunk != kHolesChunk || c.planes != p.dirs || c.walk_dirs != p.dirs - 2) return hipErrorInvalidValue;
    if (!holes_phase_runs(phase, p.dirs)) return hipSuccess;
    const long long npix = (long long)p.nx * p.ny;
    const dim3 block(kHolesThreads), lines((unsigned)c.grid_walk, (unsigned)c.nbands, (unsigned)c.walk_dirs);
    switch (phase) {
        case kHolesRows: hipLaunchKernelGGL(k_holes_rows, dim3((unsigned)c.grid_rows), block, 0, s, p.d, p.nx, p.ny, p.maxdist, p.planes); break;
        case kHolesCarry:
            hipLaunchKernelGGL(k_holes_lines<false>, lines, block, 0, s, p.d, p.nx, p.ny, p.maxdist, c.band, c.nbands, c.nlines, p.cpos, p.cval, p.planes);
            break;
        case kHolesWalk:
            hipLaunchKernelGGL(k_holes_lines<true>, lines, block, 0, s, p.d, p.nx, p.ny, p.maxdist, c.band, c.nbands, c.nlines, p.cpos, p.cval, p.planes);
            break;
        case kHolesApply: {
            const dim3 grid((unsigned)c.grid_apply);
#define APPLY(DIRS, CLS) hipLaunchKernelGGL((k_holes_apply<DIRS, CLS>), grid, block, 0, s, p.d, npix, p.planes, p.mode, p.out, p.filled, p.cls, p.mode_occ)
            if (p.cls) {  // the classified instances: p.mode is the mismatches' rule
                if (p.dirs == 2) APPLY(2, true);
                else if (p.dirs == 4) APPLY(4, true);
                else APPLY(8, true);
            } else if (p.dirs == 2) APPLY(2, false);
            else if (p.dirs == 4) APPLY(4, false);
            else APPLY(8, false);
#undef APPLY
            break;
        }
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// The grid, the span and the LDS bytes are the choice's (plan_holes_classify); the segment is the workgroup.
hipError_t launch_holes_classify(const HolesClassifyParams &p, const HolesClassifyChoice &c, hipStream_t s)
{
    if (c.family != kHolesLines || c.seg != kHolesThreads || c.span < 1 || c.span % kHolesChunk || c.span > kHolesClsMaxSpan ||
        c.lds_bytes != 4 * (c.span + c.seg + kHolesClsWords) || c.grid_x < 1 || c.grid_y < 1 || c.grid_y > kHolesClsMaxRows)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_holes_classify, dim3((unsigned)c.grid_x, (unsigned)c.grid_y), dim3(kHolesThreads), (size_t)c.lds_bytes, s, p.d, p.nx, p.ny,
                       p.other, p.vnx, p.dmin, p.dmax, p.tau, c.span, p.cls);
    return hipGetLastError();
}

}  // namespace mgm
