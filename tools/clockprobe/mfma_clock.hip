// Measures what the MFMA pipes actually deliver on this MI355X under sustained load: a bare register-resident MFMA
// loop (one wave per SIMD on every CU, like the MLP kernels), timed with HIP events, with the shader clock read from
// s_memtime (clock64) against the constant 100 MHz wall clock. Gives the DVFS-adjusted ceilings that DESIGN.md quotes
// next to the nominal peaks. Build + run:  hipcc -O3 --offload-arch=gfx950 tools/clockprobe/mfma_clock.hip -o /tmp/mfma_clock && /tmp/mfma_clock
//
// The bf16 rows compare the two MFMA shapes at equal FLOP per loop iteration (8 x 32x32x16 = 16 x 16x16x32). The "lds"
// rows re-read the A operand from LDS by ds_read_b128, one iteration ahead, at LDSR reads per iteration: 4 = the bytes
// per FLOP of the bf16x3 render kernel (3 pieces of 1 KB per 6 x 32x32x16), 8 = twice that (1 KB per 16 384 MACs).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 b8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const u32x4 lds_cu4;

constexpr int kLdsSlots = 16;                    // 1 KB fragments per wave in LDS (64 KB per workgroup)

// KIND: 0 f32_32x32x2, 1 f16_32x32x16, 2 bf16_32x32x16, 3 bf16_16x16x32
template <int KIND, int RANDOM, int LDSR = 0>
__global__ __launch_bounds__(256, 1) void probe(int iters, float* out, unsigned long long* clk) {
    constexpr int NM = KIND == 3 ? 16 : 8;       // MFMAs per iteration
    __shared__ __attribute__((aligned(16))) u32x4 smem[LDSR ? 4 * kLdsSlots * 64 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    f32x16 acc[8];
    f32x4 acc4[16];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        asm volatile("" : "+a"(acc[t]));         // one distinct register tile each (shared zeros make the allocator rotate)
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc4[t][r] = 0.f;
        asm volatile("" : "+a"(acc4[t]));
    }
    // operands: RANDOM == 0: constants (low toggle rate, the optimistic case); 1: per-lane pseudo-random values, a
    // different register pair for each of the 8 MFMAs of the loop body (data-dependent power, the realistic case)
    unsigned seed = (blockIdx.x * 256 + threadIdx.x) * 2654435761u + 12345u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return ((seed >> 8) & 0xffff) * (1.0f / 32768.0f) - 1.0f; };
    float av[8], bv[8];
    h8 hav[8], hbv[8];
    b8 bav[8], bbv[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        av[t] = RANDOM ? rnd() : 1.0f + threadIdx.x * 1e-6f;
        bv[t] = RANDOM ? rnd() : 0.5f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float x = RANDOM ? rnd() : 0.01f * i, y = RANDOM ? rnd() : 0.5f;
            hav[t][i] = (_Float16)x; hbv[t][i] = (_Float16)y; bav[t][i] = (__bf16)x; bbv[t][i] = (__bf16)y;
        }
    }
    const lds_cu4* rl = (const lds_cu4*)smem + wave * kLdsSlots * 64 + lane;
    constexpr int NF = LDSR ? LDSR : 1;
    b8 fa[NF], fb[NF];                                   // fragments of the even / odd iteration
    auto mfma = [&](int t, const b8& a) {
        if (KIND == 0) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[t], acc[t], 0, 0, 0);
        if (KIND == 1) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hav[t], hbv[t], acc[t], 0, 0, 0);
        if (KIND == 2) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bbv[t], acc[t], 0, 0, 0);
        if (KIND == 3) acc4[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bbv[t & 7], acc4[t], 0, 0, 0);
    };
    // one iteration: NM MFMAs on `cur`, the next iteration's NF fragment reads one per MFMA gap from the first on
    auto body = [&](int it, const b8 (&cur)[NF], b8 (&nxt)[NF]) {
#pragma unroll
        for (int t = 0; t < NM; ++t) {
            __builtin_amdgcn_sched_barrier(0);
            mfma(t, LDSR ? cur[t / (NM / NF)] : bav[t & 7]);
            __builtin_amdgcn_sched_barrier(0);
            if (LDSR && t < NF) nxt[t] = __builtin_bit_cast(b8, rl[(((it + 1) * NF + t) & (kLdsSlots - 1)) * 64]);
        }
    };
    if (LDSR) {
        for (int s = 0; s < kLdsSlots; ++s) {
            b8 v;
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (__bf16)(RANDOM ? rnd() : 0.01f * i);
            smem[(wave * kLdsSlots + s) * 64 + lane] = __builtin_bit_cast(u32x4, v);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NF; ++i) fa[i] = __builtin_bit_cast(b8, rl[i * 64]);
    }
    const unsigned long long c0 = clock64(), w0 = wall_clock64();
    for (int it = 0; it < iters; it += 2) {
        body(it, fa, fb);
        body(it + 1, fb, fa);
    }
    const unsigned long long c1 = clock64(), w1 = wall_clock64();
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) s += acc[t][0] + acc[t][7];
#pragma unroll
    for (int t = 0; t < 16; ++t) s += acc4[t][0] + acc4[t][3];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
    if (threadIdx.x == 0) { clk[2 * blockIdx.x] = c1 - c0; clk[2 * blockIdx.x + 1] = w1 - w0; }
}

// Launches back to back for about 2 s first (the clock settles under load), then times `reps` launches; the shader clock
// is the median over workgroups of the last launch's in-kernel stamps.
template <int KIND, int RANDOM, int LDSR = 0>
static void run(const char* name, double flop_per_mfma, int cus, int iters, int reps = 1) {
    constexpr int NM = KIND == 3 ? 16 : 8;
    float* out; unsigned long long* clk;
    hipMalloc(&out, (size_t)cus * 256 * 4);
    hipMalloc(&clk, (size_t)cus * 16);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    probe<KIND, RANDOM, LDSR><<<cus, 256>>>(iters, out, clk);          // warm-up, and its length sizes the settling run
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms1 = 0.f;
    hipEventElapsedTime(&ms1, e0, e1);
    const int settle = std::max(1, std::min(100, (int)(2000.f / std::max(ms1, 1.f))));
    for (int i = 0; i < settle; ++i) probe<KIND, RANDOM, LDSR><<<cus, 256>>>(iters, out, clk);
    hipEventRecord(e0);
    for (int i = 0; i < reps; ++i) probe<KIND, RANDOM, LDSR><<<cus, 256>>>(iters, out, clk);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    ms /= reps;
    std::vector<unsigned long long> h(2 * cus);
    hipMemcpy(h.data(), clk, (size_t)cus * 16, hipMemcpyDeviceToHost);
    std::vector<double> ghz(cus);
    for (int i = 0; i < cus; ++i) ghz[i] = (double)h[2 * i] / ((double)h[2 * i + 1] * 10.0);   // wall clock = 100 MHz = 10 ns
    std::sort(ghz.begin(), ghz.end());
    const double mfmas = (double)cus * 4 * NM * iters;
    printf("%-34s %8.3f ms  %8.1f TFLOP/s  shader clock %.3f GHz  cycles per 32k MACs per SIMD %.2f\n", name, ms,
           mfmas * flop_per_mfma / (ms * 1e-3) / 1e12, ghz[cus / 2],
           (double)h[0] / ((double)NM * iters) * (32768.0 / (flop_per_mfma / 2)));
    hipFree(out); hipFree(clk);
}

int main(int argc, char** argv) {
    int dev = 0, cus = 0;
    hipGetDevice(&dev);
    hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    printf("CUs %d\n", cus);
    const bool bf16_only = argc > 1 && argv[1][0] == 'b';        // "bf16": the shape comparison only
    const double f32 = 2.0 * 32 * 32 * 2, big = 2.0 * 32 * 32 * 16, small = 2.0 * 16 * 16 * 32;
    if (!bf16_only) {
        run<0, 0>("f32_32x32x2  constants", f32, cus, 400000);
        run<0, 1>("f32_32x32x2  random", f32, cus, 400000);
        run<1, 0>("f16_32x32x16 constants", big, cus, 800000);
        run<1, 1>("f16_32x32x16 random", big, cus, 800000);
    }
    // the two shapes alternate, so that a drift of the device clock shows up as a change between the repeats
    run<2, 0>("bf16_32x32x16 constants", big, cus, 800000, 5);
    run<3, 0>("bf16_16x16x32 constants", small, cus, 800000, 5);
    for (int rep = 0; rep < 2; ++rep) {
        run<2, 1>("bf16_32x32x16 random", big, cus, 800000, 5);
        run<3, 1>("bf16_16x16x32 random", small, cus, 800000, 5);
        run<2, 1, 4>("bf16_32x32x16 random lds 4/it", big, cus, 800000, 5);
        run<3, 1, 4>("bf16_16x16x32 random lds 4/it", small, cus, 800000, 5);
        run<2, 1, 8>("bf16_32x32x16 random lds 8/it", big, cus, 800000, 5);
        run<3, 1, 8>("bf16_16x16x32 random lds 8/it", small, cus, 800000, 5);
    }
    return 0;
}
