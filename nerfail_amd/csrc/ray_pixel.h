// The per-pixel ray of K1 (get_rays RH:157-166, the viewdir normalise / pack of render() RN:102-123): ONE definition behind
// ray_gen_kernel and train_batch_kernel (rays.hip) and ray_gen_list_kernel (fg_scene.hip), so their rows agree bit for bit.
#pragma once
#include "common.h"

namespace nerfail {

struct Cam {
    float fx, fy, cx, cy;
    float c2w[12];
};

// dirs = ((i-cx)/fx, -(j-cy)/fy, -1); rays_d[a] = (dirs0*R[a][0] + dirs1*R[a][1]) + dirs2*R[a][2]
// (torch.sum over 3 products, no FMA), rays_o = c2w[:,3].
__device__ __forceinline__ void pixel_ray(const Cam& c, int col, int row, float* o, float* d) {
    const float d0 = __fdiv_rn(__fsub_rn((float)col, c.cx), c.fx);
    const float d1 = -__fdiv_rn(__fsub_rn((float)row, c.cy), c.fy);
    const float d2 = -1.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p0 = __fmul_rn(d0, c.c2w[4 * a + 0]);
        const float p1 = __fmul_rn(d1, c.c2w[4 * a + 1]);
        const float p2 = __fmul_rn(d2, c.c2w[4 * a + 2]);
        d[a] = __fadd_rn(__fadd_rn(p0, p1), p2);
        o[a] = c.c2w[4 * a + 3];
    }
}

__device__ __forceinline__ void viewdir_of(const float* d, float* v) {
    const float n = sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
#pragma unroll
    for (int a = 0; a < 3; ++a) v[a] = __fdiv_rn(d[a], n);
}

__device__ __forceinline__ void store_ray(float* __restrict__ r, const float* o, const float* d, float near_, float far_) {
    float v[3];
    viewdir_of(d, v);
    r[0] = o[0]; r[1] = o[1]; r[2] = o[2];
    r[3] = d[0]; r[4] = d[1]; r[5] = d[2];
    r[6] = near_; r[7] = far_;
    r[8] = v[0]; r[9] = v[1]; r[10] = v[2];
}

static inline bool fill_cam(Cam& c, const float* K4, const float* c2w) {
    if (K4 == nullptr || c2w == nullptr) return false;
    c.fx = K4[0]; c.fy = K4[1]; c.cx = K4[2]; c.cy = K4[3];
    for (int i = 0; i < 12; ++i) c.c2w[i] = c2w[i];
    return true;
}

}  // namespace nerfail
