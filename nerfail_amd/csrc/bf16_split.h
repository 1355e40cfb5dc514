// The three-way bf16 split behind every "bf16x3" kernel (mlp_x3.hip, cnn_x3.hip): x = x0 + x1 + x2 + r by three
// round-to-nearest-even conversions to bf16 (8 significant bits), each difference exact in f32: |x1| <= 2^-8 |x|,
// |x2| <= 2^-16 |x|, and r = 0 whenever the pieces are normal numbers (3 x 8 bits hold the 24 of an f32). Two elements at a
// time, element 0 in the low half of the dword.
#pragma once
#include <hip/hip_runtime.h>

namespace nerfail {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// x = hi + mid + lo by round-to-nearest, two elements at a time (element 0 in the low half).
__device__ __forceinline__ unsigned cvt_bf2(float x0, float x1) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){x0, x1}, bf16x2));
}
__device__ __forceinline__ void sub_bf2(float& x0, float& x1, unsigned p) {       // x -= the bf16 pair p, exact
    x0 -= __uint_as_float(p << 16);
    x1 -= __uint_as_float(p & 0xffff0000u);
}

}  // namespace nerfail
