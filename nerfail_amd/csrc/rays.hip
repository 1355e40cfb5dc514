// K1 ray generation + packing, K2 coarse sampling.
// Replaces get_rays (run_nerf_helpers.py:157-166), the viewdir normalise / pack of render()
// (run_nerf.py:102-123) and the coarse-sample block of render_rays (run_nerf.py:357-381).
// One thread per ray (or per sample); pure streaming stores, HBM-bound and tiny next to the MLP.
// K1b: the training batch (RN:690-742, RN:744-773) - the index shuffle and rays + target colours of one batch from resident data.
#include "common.h"
#include "index_shuffle.h"
#include "ray_pixel.h"

namespace nerfail {

__global__ void get_rays_kernel(Cam c, int H, int W, float* __restrict__ rays_o, float* __restrict__ rays_d) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (long)H * W) return;
    float o[3], d[3];
    pixel_ray(c, (int)(p % W), (int)(p / W), o, d);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        rays_o[3 * p + a] = o[a];
        rays_d[3 * p + a] = d[a];
    }
}

__global__ void pack_rays_kernel(const float* __restrict__ rays_o, const float* __restrict__ rays_d, long n,
                                 float near_, float far_, float* __restrict__ rays) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float o[3] = {rays_o[3 * p], rays_o[3 * p + 1], rays_o[3 * p + 2]};
    float d[3] = {rays_d[3 * p], rays_d[3 * p + 1], rays_d[3 * p + 2]};
    store_ray(rays + NERFAIL_RAY_FLOATS * p, o, d, near_, far_);
}

__global__ void ray_gen_kernel(Cam c, int W, long pix_begin, long pix_count, float near_, float far_,
                               float* __restrict__ rays) {
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= pix_count) return;
    const long p = pix_begin + q;
    float o[3], d[3];
    pixel_ray(c, (int)(p % W), (int)(p / W), o, d);
    store_ray(rays + NERFAIL_RAY_FLOATS * q, o, d, near_, far_);
}

// out[j] = P(key, m)(first + j): one thread per element (index_shuffle.h).
__global__ void index_shuffle_kernel(uint64_t key, uint32_t m, uint32_t first, long n, int64_t* __restrict__ out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    out[j] = (int64_t)index_shuffle(key, m, first + (uint32_t)j);
}

// One training batch from resident poses and images. Population index q -> (slot, row, column) of the window; the ray is
// pixel_ray + store_ray of that pixel under the slot's pose (bit for bit ray_gen_kernel's row), the target a copy.
struct BatchArgs {
    float fx, fy, cx, cy, near_, far_;
    int H, W, row0, col0, wh, ww, view0;
    uint32_t m, first;
    uint64_t key;
    long n;
};

__global__ void train_batch_kernel(BatchArgs a, const float* __restrict__ poses, const float* __restrict__ images,
                                   const int32_t* __restrict__ view_ids, const int64_t* __restrict__ sel,
                                   float* __restrict__ rays, float* __restrict__ target, int64_t* __restrict__ sel_out) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n) return;
    const long q = (sel != nullptr) ? (long)sel[j] : (long)index_shuffle(a.key, a.m, a.first + (uint32_t)j);
    const long win = (long)a.wh * a.ww;
    const long slot = q / win;
    const int rem = (int)(q - slot * win);
    const int row = a.row0 + rem / a.ww, col = a.col0 + rem % a.ww;
    const long view = (view_ids != nullptr) ? (long)view_ids[slot] : (long)a.view0 + slot;
    Cam c;
    c.fx = a.fx; c.fy = a.fy; c.cx = a.cx; c.cy = a.cy;
#pragma unroll
    for (int i = 0; i < 12; ++i) c.c2w[i] = poses[12 * view + i];
    float o[3], d[3];
    pixel_ray(c, col, row, o, d);
    store_ray(rays + NERFAIL_RAY_FLOATS * j, o, d, a.near_, a.far_);
    if (images != nullptr) {
        const float* px = images + 3 * (((long)view * a.H + row) * a.W + col);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) target[3 * j + ch] = px[ch];
    }
    if (sel_out != nullptr) sel_out[j] = (int64_t)q;
}

// z = near*(1-t) + far*t (or the lindisp form), optional stratified jitter, pts = o + d*z.
__device__ __forceinline__ float coarse_z(float near_, float far_, float t, int lindisp) {
    if (!lindisp) return __fadd_rn(__fmul_rn(near_, __fsub_rn(1.0f, t)), __fmul_rn(far_, t));
    const float a = __fmul_rn(__fdiv_rn(1.0f, near_), __fsub_rn(1.0f, t));
    const float b = __fmul_rn(__fdiv_rn(1.0f, far_), t);
    return __fdiv_rn(1.0f, __fadd_rn(a, b));
}

__global__ void sample_coarse_kernel(const float* __restrict__ rays, long n_rays, const float* __restrict__ t_vals,
                                     int N, const float* __restrict__ t_rand, int lindisp,
                                     float* __restrict__ z_vals, float* __restrict__ pts) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_rays * N) return;
    const long r = g / N;
    const int i = (int)(g - r * N);
    const float* ray = rays + NERFAIL_RAY_FLOATS * r;
    const float near_ = ray[6], far_ = ray[7];
    float z = coarse_z(near_, far_, t_vals[i], lindisp);
    if (t_rand != nullptr) {   // RN:365-379
        const float zm = (i > 0) ? coarse_z(near_, far_, t_vals[i - 1], lindisp) : z;
        const float zp = (i < N - 1) ? coarse_z(near_, far_, t_vals[i + 1], lindisp) : z;
        const float upper = (i < N - 1) ? __fmul_rn(0.5f, __fadd_rn(zp, z)) : z;
        const float lower = (i > 0) ? __fmul_rn(0.5f, __fadd_rn(z, zm)) : z;
        z = __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), t_rand[g]));
    }
    z_vals[g] = z;
    if (pts != nullptr) {        // (NULL: the MLP kernel forms the points itself - nerfail_mlp_fwd_rays)
#pragma unroll
        for (int a = 0; a < 3; ++a) pts[3 * g + a] = mul_add_rn(ray[3 + a], z, ray[a]);
    }
}

}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_get_rays(int H, int W, const float* K4_host, const float* c2w_host, float* rays_o,
                                float* rays_d, void* stream) {
    NF_REQUIRE(H > 0 && W > 0, "H and W must be positive");
    NF_REQUIRE(rays_o != nullptr && rays_d != nullptr, "rays_o / rays_d is NULL");
    Cam c;
    NF_REQUIRE(fill_cam(c, K4_host, c2w_host), "K4_host / c2w_host is NULL");
    const long n = (long)H * W;
    get_rays_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(c, H, W, rays_o, rays_d);
    NF_LAUNCHED("get_rays_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_pack_rays(const float* rays_o, const float* rays_d, int64_t n, float near_, float far_,
                                 float* rays, void* stream) {
    NF_REQUIRE(n >= 0, "n is negative");
    if (n == 0) return NERFAIL_OK;
    NF_REQUIRE(rays_o != nullptr && rays_d != nullptr && rays != nullptr, "NULL pointer");
    pack_rays_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(rays_o, rays_d, n, near_, far_, rays);
    NF_LAUNCHED("pack_rays_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_ray_gen(int H, int W, const float* K4_host, const float* c2w_host, float near_, float far_,
                               int64_t pix_begin, int64_t pix_count, float* rays, void* stream) {
    NF_REQUIRE(H > 0 && W > 0, "H and W must be positive");
    NF_REQUIRE(pix_begin >= 0 && pix_count >= 0 && pix_begin + pix_count <= (int64_t)H * W, "pixel range outside the image");
    if (pix_count == 0) return NERFAIL_OK;
    NF_REQUIRE(rays != nullptr, "rays is NULL");
    Cam c;
    NF_REQUIRE(fill_cam(c, K4_host, c2w_host), "K4_host / c2w_host is NULL");
    ray_gen_kernel<<<dim3((unsigned)((pix_count + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(
        c, W, pix_begin, pix_count, near_, far_, rays);
    NF_LAUNCHED("ray_gen_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_index_shuffle(uint64_t key, int64_t m, int64_t first, int64_t n, int64_t* out, void* stream) {
    NF_REQUIRE(m >= 1 && m <= ((int64_t)1 << 31), "m must be in [1, 2^31]");
    NF_REQUIRE(first >= 0 && n >= 0 && first <= m && n <= m - first, "range [first, first + n) outside [0, m)");
    if (n == 0) return NERFAIL_OK;
    NF_REQUIRE(out != nullptr, "out is NULL");
    index_shuffle_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(key, (uint32_t)m, (uint32_t)first, n, out);
    NF_LAUNCHED("index_shuffle_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_train_batch(int H, int W, const float* K4_host, float near_, float far_, const float* poses, int n_img,
                                   const float* images, int row0, int col0, int wh, int ww, const int32_t* view_ids, int view0,
                                   int n_views, const int64_t* sel, uint64_t key, int64_t first, int64_t n, float* rays,
                                   float* target, int64_t* sel_out, void* stream) {
    NF_REQUIRE(H > 0 && W > 0, "H and W must be positive");
    NF_REQUIRE(row0 >= 0 && col0 >= 0 && wh >= 0 && ww >= 0 && row0 <= H && wh <= H - row0 && col0 <= W && ww <= W - col0,
               "window outside the image");
    NF_REQUIRE(n_img > 0 && n_views >= 0, "bad n_img / n_views");
    NF_REQUIRE(view_ids != nullptr || (view0 >= 0 && view0 <= n_img && n_views <= n_img - view0), "views outside [0, n_img)");
    NF_REQUIRE((int64_t)wh * ww <= ((int64_t)1 << 31), "window of more than 2^31 pixels");
    const int64_t m = (int64_t)n_views * ((int64_t)wh * ww);      // (< 2^31 * 2^31: no overflow)
    NF_REQUIRE(m >= 1 && m <= ((int64_t)1 << 31), "population n_views * wh * ww must be in [1, 2^31]");
    NF_REQUIRE(first >= 0 && n >= 0 && first <= m && n <= m - first, "batch [first, first + n) outside the population");
    if (n == 0) return NERFAIL_OK;
    NF_REQUIRE(K4_host != nullptr && poses != nullptr, "K4_host / poses is NULL");
    NF_REQUIRE(rays != nullptr, "rays is NULL");
    NF_REQUIRE(images == nullptr || target != nullptr, "target is NULL");
    BatchArgs a;
    a.fx = K4_host[0]; a.fy = K4_host[1]; a.cx = K4_host[2]; a.cy = K4_host[3];
    a.near_ = near_; a.far_ = far_;
    a.H = H; a.W = W; a.row0 = row0; a.col0 = col0; a.wh = wh; a.ww = ww; a.view0 = view0;
    a.m = (uint32_t)m; a.first = (uint32_t)first; a.key = key; a.n = n;
    train_batch_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(a, poses, images, view_ids, sel, rays,
                                                                                              target, sel_out);
    NF_LAUNCHED("train_batch_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_sample_coarse(const float* rays, int64_t n_rays, const float* t_vals, int n_samples,
                                     const float* t_rand, int lindisp, float* z_vals, float* pts, void* stream) {
    NF_REQUIRE(n_rays >= 0 && n_samples > 0, "bad n_rays / n_samples");
    if (n_rays == 0) return NERFAIL_OK;
    NF_REQUIRE(rays != nullptr && t_vals != nullptr && z_vals != nullptr, "NULL pointer");
    const long n = n_rays * n_samples;
    sample_coarse_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(
        rays, n_rays, t_vals, n_samples, t_rand, lindisp, z_vals, pts);
    NF_LAUNCHED("sample_coarse_kernel");
    return NERFAIL_OK;
}
