// mgm_speckle.hip -- the speckle filter (this project's own step, the reference has none): connected-component
// labelling of a finished disparity map on the device, then NaN into every component of at most `maxsize` pixels.
//
//   valid pixel   d(p) finite (NaN and +-INF belong to no component and are copied through bit for bit)
//   edge          4-neighbours p, q, both valid, with fabsf(d(p) - d(q)) <= maxdiff: ONE fp32 subtraction (this file is built with
//                 -ffp-contract=off), so -0 / +0 are joined and a difference that overflows is joined under maxdiff = +INF only
//   component     of that graph (chained: a ramp of steps <= maxdiff is one component); size(p) = its pixel count
//   out(p)        = valid(p) && size(p) <= maxsize ? NaN : d(p);   size_map(p) = (float)size(p), 0 on invalid pixels
//
// Block-based union-find.  `parent` holds one int32 per pixel, a linear pixel index; the root of a tree is the SMALLEST index in
// it, and a parent only ever decreases.  Four launches, each a phase that the next one sees finished:
//
//   k_speckle_local   one workgroup per tile: pixels and a tile-local parent array in LDS, unions along the tile's inner row and
//                     column edges by atomicMin on LDS, parents flattened, pixels counted per local root; writes parent[p] = the
//                     global index of p's local root and cnt[p] = that root's pixel count at the root, 0 everywhere else
//                     (EVERY word of both planes: no memset, nothing stale from an earlier call)
//   k_speckle_seams   one thread per pixel pair across a tile's right / bottom seam: lock-free union in global memory
//   k_speckle_count   every tile-local root adds its count to its global root: one atomic per tile-local component
//   k_speckle_apply   one thread per pixel: global root, its total, out and / or size_map
//
// No loop here waits for a value that another wave must produce: no flag, no barrier across workgroups, no watchdog (the comment
// at speckle_union says why every loop ends on its own).
#include "mgm_device.h"
#include "mgm_planner.h"

namespace mgm {

__device__ __forceinline__ bool speckle_joined(float v, float w, float maxdiff)
{
    return finite_bits(v) && finite_bits(w) && __builtin_fabsf(v - w) <= maxdiff;
}

// The parents of one phase's trees: in LDS (k_speckle_local, workgroup scope) or in global memory (agent scope).  Atomic
// read-modify-writes on global memory run at the memory side, and a plain load may be served from an L1 or another XCD's L2 that
// still holds the line as it was (MI355X_MICROARCH.md, coherence table): while a kernel changes parents, every read of one is a
// relaxed atomic load of the scope that the writers use.
template <int SCOPE>
__device__ __forceinline__ int par_load(const int *par, int x)
{
    return __hip_atomic_load(par + x, __ATOMIC_RELAXED, SCOPE);
}
template <int SCOPE>
__device__ __forceinline__ int par_find(const int *par, int x)
{
    // parent[x] < x off the root: the walk goes strictly down and ends at a word that names itself
    for (int p; (p = par_load<SCOPE>(par, x)) != x;) x = p;
    return x;
}

// Lock-free union of the trees of a and b: find both roots, hang the larger under the smaller with atomicMin, and go on from
// the value the atomic returns until the two roots agree.
// NOTHING HERE WAITS: no iteration needs a value that another wave has yet to produce.  Parents only decrease, so a parent read
// late (stale) is a word the tree held earlier -- still a node of the same tree, whose own walk ends at the same root or above a
// later link to it -- and an atomicMin on a word that has meanwhile stopped being a root returns what it displaced:
//   old == a      a was a root and now hangs under b: done
//   old <  a      a had a parent already.  Whether the atomic lowered it (old > b) or not (old <= b), the pair (old, b) is still to be
//                 joined, and both are smaller than a: the larger index of the pair falls strictly with every turn, whatever the
//                 other threads do, so the loop ends after finitely many turns of its own.
template <int SCOPE>
__device__ __forceinline__ void speckle_union(int *par, int a, int b)
{
    for (;;) {
        a = par_find<SCOPE>(par, a);
        b = par_find<SCOPE>(par, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

// One tile of TW x TH pixels per workgroup of kSpeckleThreads threads, (TW * TH) / kSpeckleThreads pixels per thread (pixel i of the tile,
// row-major, belongs to thread i % kSpeckleThreads: a wave touches 64 consecutive pixels of a row).  Pixels of a ragged tile that lie
// outside the image are NaN in LDS: invalid, joined with nothing, never written.  A smaller local index is a smaller global index, so
// the local root (the smallest local index of the component) is the smallest global index of the component inside this tile.
template <int TW, int TH>
__global__ void __launch_bounds__(kSpeckleThreads) k_speckle_local(const float *__restrict__ d, int nx, int ny, int ntx, float maxdiff,
                                                                  int *__restrict__ parent, int *__restrict__ cnt)
{
    constexpr int N = TW * TH, PPT = N / kSpeckleThreads;
    static_assert(N % kSpeckleThreads == 0 && kSpeckleThreads % 64 == 0, "whole pixels per thread, whole waves");
    constexpr int LDS = __HIP_MEMORY_SCOPE_WORKGROUP;
    __shared__ float s_d[N];
    __shared__ int s_par[N];
    __shared__ int s_cnt[N];
    const long long x0 = (long long)(blockIdx.x % (unsigned)ntx) * TW, y0 = (long long)(blockIdx.x / (unsigned)ntx) * TH;  // (x0 + TW may pass 2^31)
    for (int k = 0; k < PPT; k++) {
        const int i = threadIdx.x + k * kSpeckleThreads;
        const long long x = x0 + i % TW, y = y0 + i / TW;
        s_d[i] = (x < nx && y < ny) ? d[y * nx + x] : __builtin_nanf("");
        s_par[i] = i;
        s_cnt[i] = 0;
    }
    __syncthreads();
    // unions along the inner edges: every pixel with its right and its lower neighbour
    for (int k = 0; k < PPT; k++) {
        const int i = threadIdx.x + k * kSpeckleThreads;
        const float v = s_d[i];
        if (i % TW + 1 < TW && speckle_joined(v, s_d[i + 1], maxdiff)) speckle_union<LDS>(s_par, i, i + 1);
        if (i / TW + 1 < TH && speckle_joined(v, s_d[i + TW], maxdiff)) speckle_union<LDS>(s_par, i, i + TW);
    }
    __syncthreads();
    // flatten: every root is read before any parent is rewritten
    int root[PPT];
#pragma unroll
    for (int k = 0; k < PPT; k++) root[k] = par_find<LDS>(s_par, threadIdx.x + k * kSpeckleThreads);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PPT; k++) s_par[threadIdx.x + k * kSpeckleThreads] = root[k];
    // count per local root.  The lanes of a wave that share the first lane's root (all of them inside a smooth region) send ONE add
    // of their number, the others one add each.
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < PPT; k++) {
        const int i = threadIdx.x + k * kSpeckleThreads;
        const int key = finite_bits(s_d[i]) ? root[k] : -1;
        const int lead = __builtin_amdgcn_readfirstlane(key);
        const unsigned long long same = __ballot(key == lead);
        if (key == lead) {
            if (lead >= 0 && lane == __ffsll((long long)same) - 1) atomicAdd(&s_cnt[lead], __popcll(same));
        } else if (key >= 0) atomicAdd(&s_cnt[key], 1);
    }
    __syncthreads();
    for (int k = 0; k < PPT; k++) {
        const int i = threadIdx.x + k * kSpeckleThreads;
        const long long x = x0 + i % TW, y = y0 + i / TW;
        if (x >= nx || y >= ny) continue;
        const long long p = y * nx + x;
        const int r = s_par[i];  // (an invalid pixel is its own root, with a count of 0)
        parent[p] = (int)((y0 + r / TW) * nx + (x0 + r % TW));
        cnt[p] = r == i ? s_cnt[i] : 0;
    }
}

// One thread per pixel pair across a seam: first the (ntx - 1) vertical seams, ny pairs each, then the (nty - 1) horizontal ones,
// nx pairs each.  The unions of this kernel race with one another on `parent`; the next phase is a launch of its own.
__global__ void __launch_bounds__(kSpeckleThreads) k_speckle_seams(const float *__restrict__ d, int nx, int ny, int tw, int th, int ntx, int nty,
                                                                  float maxdiff, int *parent)
{
    long long k = (long long)blockIdx.x * kSpeckleThreads + threadIdx.x;
    const long long nv = (long long)(ntx - 1) * ny, nh = (long long)(nty - 1) * nx;
    if (k >= nv + nh) return;
    long long p, q;
    if (k < nv) {  // (x + 1 <= (ntx - 1) * tw < nx)
        const long long x = (k / ny + 1) * tw - 1, y = k % ny;
        p = y * nx + x, q = p + 1;
    } else {  // (y + 1 <= (nty - 1) * th < ny)
        k -= nv;
        const long long x = k % nx, y = (k / nx + 1) * th - 1;
        p = y * nx + x, q = p + nx;
    }
    if (speckle_joined(d[p], d[q], maxdiff)) speckle_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)p, (int)q);
}

// Every tile-local root r (cnt[r] = n > 0) finds its global root g and, if that is another pixel, adds n to cnt[g]: one atomic per
// tile-local component, never one per pixel.  ONE plane holds partial counts and totals, and they cannot be confused: adds land
// on global roots only, a global root adds nothing (g == r), so the word this thread reads as a partial -- that of a root which is
// NOT global -- is written by nobody in this launch; and k_speckle_apply, a launch of its own, reads cnt at global roots only, where
// the word is the root's own tile's count plus every add: the total.  parent[r] = g shortens the walks of the next launch; walks of
// this one that cross the word read the old parent or g, both on the way to g (relaxed atomic loads and stores).
__global__ void __launch_bounds__(kSpeckleThreads) k_speckle_count(long long npix, int *parent, int *cnt)
{
    constexpr int DEV = __HIP_MEMORY_SCOPE_AGENT;
    const long long p = (long long)blockIdx.x * kSpeckleThreads + threadIdx.x;
    if (p >= npix) return;
    const int n = cnt[p];
    if (n <= 0) return;
    if (par_load<DEV>(parent, (int)p) == (int)p) return;  // a global root: its word is the total's
    const int g = par_find<DEV>(parent, (int)p);
    __hip_atomic_fetch_add(cnt + g, n, __ATOMIC_RELAXED, DEV);
    __hip_atomic_store(parent + p, g, __ATOMIC_RELAXED, DEV);
}

// d[p] is read before out[p] is written and the labelling is finished: out may be d (no __restrict__ on either).
__global__ void __launch_bounds__(kSpeckleThreads) k_speckle_apply(const float *d, long long npix, const int *__restrict__ parent,
                                                                  const int *__restrict__ cnt, int maxsize, float *out,
                                                                  float *__restrict__ size_map)
{
    const long long p = (long long)blockIdx.x * kSpeckleThreads + threadIdx.x;
    if (p >= npix) return;
    const float v = d[p];
    const bool valid = finite_bits(v);
    int size = 0;
    if (valid) {
        int x = (int)p;
        for (int q; (q = parent[x]) != x;) x = q;
        size = cnt[x];
    }
    if (out) out[p] = (valid && size <= maxsize) ? __builtin_nanf("") : v;
    if (size_map) size_map[p] = (float)size;
}

const char *speckle_phase_name(int phase)
{
    static const char *const names[kSpecklePhases] = {"k_speckle_local", "k_speckle_seams", "k_speckle_count", "k_speckle_apply"};
    return phase >= 0 && phase < kSpecklePhases ? names[phase] : "";
}

// A table from the planner's choice to the launch: the tile's shape selects the instance of k_speckle_local, the grids are the choice's.
hipError_t launch_speckle_phase(int phase, const SpeckleParams &p, const SpeckleChoice &c, hipStream_t s)
{
    if (c.family != kSpeckleTiles || c.tw != kSpeckleTileW || c.th != kSpeckleTileH) return hipErrorInvalidValue;  // (the one instance)
    const long long npix = (long long)p.nx * p.ny;
    const dim3 block(kSpeckleThreads);
    switch (phase) {
        case kSpeckleLocal:
            hipLaunchKernelGGL((k_speckle_local<kSpeckleTileW, kSpeckleTileH>), dim3((unsigned)c.grid_local), block, 0, s, p.d, p.nx, p.ny, c.ntx,
                               p.maxdiff, p.parent, p.cnt);
            break;
        case kSpeckleSeams:
            hipLaunchKernelGGL(k_speckle_seams, dim3((unsigned)c.grid_seams), block, 0, s, p.d, p.nx, p.ny, c.tw, c.th, c.ntx, c.nty, p.maxdiff,
                               p.parent);
            break;
        case kSpeckleCount: hipLaunchKernelGGL(k_speckle_count, dim3((unsigned)c.grid_count), block, 0, s, npix, p.parent, p.cnt); break;
        case kSpeckleApply:
            hipLaunchKernelGGL(k_speckle_apply, dim3((unsigned)c.grid_apply), block, 0, s, p.d, npix, p.parent, p.cnt, p.maxsize, p.out, p.size_map);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace mgm
