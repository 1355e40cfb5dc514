// K9's per-pixel arithmetic (create_gauss_w.forward, GN:169-186), shared by gauss_weight_kernel (gauss.hip) and the
// weight epilogue of the 8-NN search (knn_grid.hip): ONE definition, so the fused map is bit for bit the chain's.
#pragma once
#include "common.h"

namespace nerfail {

// d[0..7] (ascending distances of one pixel) -> w[0..7]: g_k = exp(-(d_k/c)^2 / 2), w_k = g_k / (sum g + 0.001) if sum g > 0
// else 0. One rounding per operation (explicit _rn intrinsics: no contraction, no reassociation), the sum in k = 0..7 order.
__device__ __forceinline__ void gauss_weights8(const float (&d)[8], float c, float (&w)[8]) {
    float gk[8];
    float ds = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float q = __fdiv_rn(d[k], c);
        gk[k] = expf(-__fdiv_rn(__fmul_rn(q, q), 2.0f));     // exp(-(d/c)^2 / 2)
        ds = __fadd_rn(ds, gk[k]);
    }
    const float dq = __fadd_rn(ds, 0.001f);
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = (ds > 0.f) ? __fdiv_rn(gk[k], dq) : 0.f;
}

}  // namespace nerfail
