// Device helpers shared by the LDS-ring forward kernels (mlp_lds.hip: exact f32; mlp_x3.hip: bf16x3).
#pragma once
#include "mlp_layout.h"

namespace nerfail {

typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void glb_void_t;
typedef __attribute__((address_space(3))) const f32x4 lds_cf4;

template <int N> __device__ __forceinline__ void lds_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ f32x4 lds_read4(const float* p) { return *(lds_cf4*)p; }

// max(x, 0) as ONE integer instruction on the bit pattern (negative floats are negative integers; -0 -> +0). fmaxf costs
// two: hipcc first canonicalises an accumulator value (v_max x, x) before the IEEE-mode v_max with 0.
__device__ __forceinline__ float relu_bits(float x) {
    const int i = __float_as_int(x);
    return __int_as_float(i > 0 ? i : 0);
}

// dot product of a thin head's weights (LDS, accumulator order [OT][2][16]) with relu(x): VALU + one cross-half shuffle.
// One tile at a time (sched_barrier): left alone, hipcc reads all 128 accumulators into VGPRs first and the register
// allocator answers by spilling the positional encodings across the whole layer loop.
template <int OT, int NIN>
__device__ __forceinline__ float lds_head(const f32x16 (&x)[NIN], const float* w, int h) {
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < OT; ++t) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const f32x4 wv = lds_read4(w + (t * 2 + h) * 16 + 4 * r4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = x[t][4 * r4 + e];
                asm("" : "+v"(v));     // opaque copy: otherwise hipcc shares these ReLUs with the next layer's operand
                                       // preparation and keeps all 128 results alive in between (spills)
                s = fmaf(wv[e], relu_bits(v), s);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    return s + __shfl_xor(s, 32, 64);
}

// Three heads over the same input (rgb_linear's three rows): every accumulator register is read ONCE (round 5: three calls of
// lds_head moved each of the 64 registers to a VGPR three times - an accumulator read goes through the matrix pipe, ~13 cycles).
// Each sum is the same fma chain in the same order as lds_head's: the bits do not change.
template <int OT, int NIN>
__device__ __forceinline__ void lds_head3(const f32x16 (&x)[NIN], const float* w, int stride, int h, float (&out)[3]) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < OT; ++t) {
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const float* p = w + (t * 2 + h) * 16 + 4 * r4;
            const f32x4 w0 = lds_read4(p), w1 = lds_read4(p + stride), w2 = lds_read4(p + 2 * stride);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = x[t][4 * r4 + e];
                asm("" : "+v"(v));
                v = relu_bits(v);
                s0 = fmaf(w0[e], v, s0);
                s1 = fmaf(w1[e], v, s1);
                s2 = fmaf(w2[e], v, s2);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    out[0] = s0 + __shfl_xor(s0, 32, 64);
    out[1] = s1 + __shfl_xor(s1, 32, 64);
    out[2] = s2 + __shfl_xor(s2, 32, 64);
}

}  // namespace nerfail
