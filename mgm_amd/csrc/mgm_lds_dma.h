// mgm_lds_dma.h -- the LDS-DMA and band hand-off primitives of the pass kernels that keep their memory side on loader
// waves (mgm_pass2.hip, mgm_pass_rel.hip): LDS-DMA retired by counted vmcnt waits, LDS accesses the compiler must not order
// against pending DMA, 16-byte write-through stores, and the test of a self-validating hand-off piece.  Each primitive has
// ONE copy, here, with the rule it was learned under; what only one kernel uses stays in that kernel's file.
#pragma once
#include "mgm_pass_common.h"

namespace mgm {

typedef __attribute__((address_space(3))) void *lds_vptr;
typedef const __attribute__((address_space(1))) void *glb_vptr;

// LDS-DMA (global_load_lds_dwordx4 / _dword): lane l moves 16 (4) bytes from its OWN source address -- dma16: src_lane[0 .. 15]
// -- to dst_base + 16 l (4 l): the LDS destination is a wave-uniform base + the piece size times the lane.  No VGPR round
// trip, so the compiler has nothing to wait for, and the loader retires its loads with COUNTED waits (wait_vmcnt).
template <int AUX>
__device__ __forceinline__ void dma16(const void *src_lane, void *dst_base)
{
    __builtin_amdgcn_global_load_lds((glb_vptr)src_lane, (lds_vptr)dst_base, 16, 0, AUX);
}
template <int AUX>
__device__ __forceinline__ void dma4(const void *src_lane, void *dst_base)
{
    __builtin_amdgcn_global_load_lds((glb_vptr)src_lane, (lds_vptr)dst_base, 4, 0, AUX);
}
constexpr int AUX_SC1 = 16;  // agent-scope (L1-bypassing) cache policy bit

// The counted wait: all but the newest N vector-memory instructions of this wave have completed (DMAs land in issue order),
// so N = (DMA instructions per step) x (steps kept in flight) retires exactly the step about to be read and leaves the
// rest in flight across the step barrier.
template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit counter");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// LDS accesses the compiler must not order against pending LDS-DMA itself (it would drain vmcnt): the landing of the word
// is guaranteed by the counted wait.  The reads wait for their own data (lgkmcnt) and nothing else; the write is for
// putting a validated piece back where the compute waves will read it.
__device__ __forceinline__ unsigned lds_read_u32_opaque(const unsigned *p)
{
    unsigned v;
    const unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const unsigned *)p;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
    return v;
}
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 lds_read_b128_opaque(const float *p)
{
    u32x4 v;
    const unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const float *)p;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
    return v;
}
__device__ __forceinline__ void lds_write_b128_opaque(float *p, u32x4 v)
{
    const unsigned a = (unsigned)(uintptr_t)(__attribute__((address_space(3))) float *)p;
    asm volatile("ds_write_b128 %0, %1" ::"v"(a), "v"(v) : "memory");
}

// Write-through (sc1) stores, for the band hand-off.  Use the widest piece the data allows: narrow sc1 stores are one
// fabric write each, so 4 x dword costs ~6x the time of one dwordx4 (MI355X_MICROARCH.md, "stores of each flavour"; the
// second build's hand-off learned it in round 3, and k_pass_rel's slab leaves as 16 x 16 bytes, not 64 x 4).
// Inline asm because clang has no 16-byte agent-scope store; the trailing s_nop keeps the data registers intact until the
// store has read them.  Not counted by the compiler's vmcnt bookkeeping -- compute waves issue no loads, and every wait on
// these stores is explicit.
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void st_sc1_x4(float *p, f32x4 v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st_sc1_x2(float *p, f32x2 v)
{
    asm volatile("global_store_dwordx2 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st_sc1_x1(float *p, float a)
{
    asm volatile("global_store_dword %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(a) : "memory");
}
__device__ __forceinline__ void st_sc1_x4(float *p, float a, float b, float c, float d) { st_sc1_x4(p, f32x4{a, b, c, d}); }
__device__ __forceinline__ void st_sc1_x2(float *p, float a, float b) { st_sc1_x2(p, f32x2{a, b}); }

// A self-validating hand-off piece (what is handed over is >= +0, so the last line of a band stores it with the LAUNCH's
// tag in the sign bit of every word; whatever a slot held before carries the other sign): is this piece this launch's --
// do all four sign bits equal the tag?
__device__ __forceinline__ bool hand_tagged(u32x4 v, unsigned tag)
{
    return tag ? ((v.x & v.y & v.z & v.w) >> 31) != 0u : ((v.x | v.y | v.z | v.w) >> 31) == 0u;
}

}  // namespace mgm
