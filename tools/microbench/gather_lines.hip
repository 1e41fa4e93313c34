// Gather micro-benchmark (development aid): 128-byte lines at pseudo-random places of a 2 GiB buffer, in the shapes a wave of the
// pruned winner search (k_wta_pruned, mgm_wta.hip) could ask for its chunk lines in, without any of its compute:
//   (i)   eight lanes x 16 bytes per line, eight lines per wave instruction -- the kernel's shape;
//   (ii)  32 lanes x 4 bytes per line, two lines per instruction;
//   (iii) 16 lanes x 8 bytes per line, four lines per instruction;
//   (iv)  the control: 64 lanes x 16 bytes, one KiB contiguous per instruction at a random slab.
// Each at 1, 2 and 4 independent loads in flight per lane (all issued before the first is consumed) and at 4 and 8 waves per SIMD.
// Every run reads 4 GiB; the places come from a hash of counters, never from loaded data, so nothing but the loop serialises them.
//   hipcc --offload-arch=gfx950 -O3 tools/microbench/gather_lines.hip -o gather_lines && ./gather_lines
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
template <int B> struct Piece;
template <> struct Piece<4> { using T = float; static __device__ float sum(T v) { return v; } };
template <> struct Piece<8> { using T = float2; static __device__ float sum(T v) { return v.x + v.y; } };
template <> struct Piece<16> { using T = float4; static __device__ float sum(T v) { return v.x + v.y + v.z + v.w; } };
__device__ __forceinline__ unsigned mix(unsigned x)
{
    x ^= x >> 16, x *= 0x7feb352du, x ^= x >> 15, x *= 0x846ca68bu, x ^= x >> 16;
    return x;
}
// LANES lanes read one unit of LANES * B bytes together; a wave instruction reads 64 / LANES units, ILP instructions in flight.
// `mask`: units in the buffer - 1 (a power of two), so every address stays inside it.
template <int LANES, int B, int ILP>
__global__ __launch_bounds__(256) void k_gather(const char *base, unsigned mask, int iters, float *out)
{
    constexpr int UNITS = 64 / LANES;
    using P = Piece<B>;
    const unsigned lane = threadIdx.x & 63, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const unsigned grp = lane / LANES, off = (lane % LANES) * B;
    float a = 0;
    for (int it = 0; it < iters; it++) {
        typename P::T v[ILP];
#pragma unroll
        for (int i = 0; i < ILP; i++) {
            const unsigned unit = mix(((wave * (unsigned)iters + it) * ILP + i) * UNITS + grp) & mask;
            v[i] = *reinterpret_cast<const typename P::T *>(base + (size_t)unit * (LANES * B) + off);
        }
#pragma unroll
        for (int i = 0; i < ILP; i++) a += P::sum(v[i]);
    }
    if (a == 123.456f) *out = a;
}
static hipEvent_t e0, e1;
template <int LANES, int B, int ILP>
static void run(const char *name, const char *buf, size_t bytes, float *out, int wg_per_cu, int cus)
{
    const size_t total = (size_t)4 << 30, per_instr = 64 * B;
    const int blocks = cus * wg_per_cu;
    const int iters = (int)(total / ((size_t)blocks * 4 * per_instr * ILP));
    const unsigned mask = (unsigned)(bytes / (LANES * B)) - 1u;
    float best = 1e9f;
    for (int r = 0; r < 6; r++) {  // (the first run warms up)
        (void)hipEventRecord(e0);
        hipLaunchKernelGGL((k_gather<LANES, B, ILP>), dim3(blocks), dim3(256), 0, 0, buf, mask, iters, out);
        (void)hipEventRecord(e1);
        (void)hipEventSynchronize(e1);
        float ms;
        (void)hipEventElapsedTime(&ms, e0, e1);
        if (r && ms < best) best = ms;
    }
    const double moved = (double)blocks * 4 * iters * ILP * per_instr;
    printf("%-44s %d waves/SIMD, %d in flight (%4d B per wave): %7.3f ms %8.1f GB/s %7.2f G lines/s\n", name, wg_per_cu, ILP, (int)per_instr * ILP, best,
           moved / best / 1e6, moved / 128 / best / 1e6);
}
template <int LANES, int B>
static void shape(const char *name, const char *buf, size_t bytes, float *out, int cus)
{
    for (int wg : {4, 8}) {
        run<LANES, B, 1>(name, buf, bytes, out, wg, cus);
        run<LANES, B, 2>(name, buf, bytes, out, wg, cus);
        run<LANES, B, 4>(name, buf, bytes, out, wg, cus);
    }
}
int main()
{
    const size_t bytes = (size_t)2 << 30;
    char *buf;
    float *out;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess || hipMalloc(&buf, bytes) != hipSuccess || hipMalloc(&out, 4) != hipSuccess) return 1;
    (void)hipMemset(buf, 0, bytes);
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    const int cus = prop.multiProcessorCount;
    printf("%s, %d CUs; 4 GiB read per run from a 2 GiB buffer, workgroups of 4 waves, best of 5\n", prop.name, cus);
    shape<8, 16>("(i)   8 lanes x 16 B, 8 lines / instruction", buf, bytes, out, cus);
    shape<32, 4>("(ii)  32 lanes x 4 B, 2 lines / instruction", buf, bytes, out, cus);
    shape<16, 8>("(iii) 16 lanes x 8 B, 4 lines / instruction", buf, bytes, out, cus);
    shape<64, 16>("(iv)  64 lanes x 16 B, 1 KiB slab / instruction", buf, bytes, out, cus);
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
