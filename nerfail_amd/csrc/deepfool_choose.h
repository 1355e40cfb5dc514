// The second launch of a DeepFool step, deepfool.py:81-96 (= DF), as ONE device function: nerfail_deepfool_step (deepfool.hip; the
// perturbation table of the 3-D attack) and nerfail_uap2d_step (uap2d.hip; the image-plane table of the 2-D baseline) differ in
// what their norms are taken over and in what the choice is applied to, not in the choice. Record layout: include/nerfail_hip.h.
#pragma once
#include "common.h"

namespace nerfail {

// One block of 256 adds the per-workgroup partials of class k in a fixed order: every caller gets the same bits.
__device__ __forceinline__ double norms_finish_sum(const double* __restrict__ partial, long nblocks, int K, int k, double* red) {
    double v = 0.;
    for (long b = threadIdx.x; b < nblocks; b += 256) v += partial[b * K + k];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// The finish of the norm reduction (norms_finish_sum's tree for every competitor), then DF:81-96 on lane 0 in float32 and in the
// mirror's operation order: which competitor, and by how much. One workgroup of 256; red: 256 doubles, n2:
// NERFAIL_DEEPFOOL_MAX_COMPETITORS floats, both in LDS.
__device__ __forceinline__ void deepfool_choose_body(const double* __restrict__ partial, long nblocks, int K,
                                                     const nerfail_deepfool_record* __restrict__ rec, float* __restrict__ norms2,
                                                     int* __restrict__ best_out, float* __restrict__ scale_out,
                                                     int* __restrict__ trace_slot, double* red, float* n2) {
    for (int k = 0; k < K; ++k) {
        const double r = norms_finish_sum(partial, nblocks, K, k, red);
        if (threadIdx.x == 0) n2[k] = norms2[k] = (float)r;
    }
    if (threadIdx.x != 0) return;
    int best = 1, cls = -1;
    float scale = 0.f;                                                             // 0 = nothing chosen: apply leaves rot alone
    if (rec->n_comp == K) {                                                        // a record of another shape moves nothing
        if (rec->targeted) {                                                       // :92-96: competitor 0, no comparison
            const float nrm = sqrt_rn(n2[0]);
            scale = rec->fabs[0] / __fadd_rn(__fmul_rn(nrm, nrm), 1e-4f);
            cls = rec->cls[0];
        } else {
            float minv = INFINITY;
            int bi = -1;
            for (int r = 0; r < K; ++r) {
                float vr = rec->fabs[r] / __fadd_rn(sqrt_rn(n2[r]), 1e-4f);        // :82
                if (vr != vr) vr = INFINITY;
                if (vr < minv) { minv = vr; bi = r; }                              // :84's strict <: the first minimum
            }
            if (bi >= 0) {
                const float nrm = sqrt_rn(n2[bi]);
                scale = rec->fabs[bi] / __fadd_rn(__fmul_rn(nrm, nrm), 1e-4f);     // :85: the norm squared again, not norms2
                best = bi + 1;
                cls = rec->cls[bi];
            }
        }
    }
    best_out[0] = best;
    scale_out[0] = scale;
    trace_slot[0] = cls;
}

}  // namespace nerfail
