// ABI 15 - the per-epoch bookkeeping of the NeRFail-S loop (attack_NeRFail_S.py:278-442 = AS) on the device: epoch sums of the
// clean / attacked CE and accuracy (AS:319-344), the image loss sum (AS:329, 341), the epoch close with the best-tensor rule
// (AS:405-431), the conditional copy that keeps the best perturbation without a host decision, the beta term's gradient
// (AS:336) and the float -> uint8 conversion of the export epoch (AS:401-402). The reference takes five .item() host reads
// per batch for this; here one stats row per epoch lives on the device and the host reads one record per epoch.
//
// Sums are formed in double and kept in the float32 row as (hi, lo) pairs (hi = the sum rounded to float32, lo = the rest):
// a view count of 100 x 800 x 800 x 4 elements or a CE sum over thousands of views loses nothing on one rank, and the row can
// still travel through a float32 all-reduce (which adds the his and the los separately: the sum over ranks is then good to
// one float32 rounding of the his, ~6e-8 relative, not exact). One lane adds into the row per launch; launches on a stream are ordered: no atomics anywhere,
// every sum has a fixed order, every result is bitwise reproducible.
#include "common.h"
#include "attack_close.h"

namespace nerfail {

constexpr int kSqerrBlocks = 2048;      // partial slots = the grid cap of a streaming kernel (256 CUs x 8 workgroups)
constexpr int kSqerrViews = 16;         // view pointers per launch (passed by value)

struct OriViews {
    const void* ori[kSqerrViews];
    int nv;
};

// ---- AS:319-330: per-view CE and first-maximum argmax of both logit sets, one wave. Lane l takes views l, l + 64, ...
// (an attack batch is 8 views; the export pass a few hundred at most).
__global__ __launch_bounds__(64) void attack_logit_stats_kernel(const float* __restrict__ cla, const float* __restrict__ ori_cla, int B,
                                                                int C, int label, float* __restrict__ row) {
    const int lane = threadIdx.x;
    double ce[2] = {0.0, 0.0};
    float ok[2] = {0.f, 0.f};
    for (int b = lane; b < B; b += 64) {
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            const LogitRow r = logit_row_stats((which == 0 ? ori_cla : cla) + (long)b * C, C, label);
            ce[which] += r.ce;
            ok[which] += (r.arg == label) ? 1.f : 0.f;
        }
    }
    const double s0 = wave_sum_f64(ce[0]), s1 = wave_sum_f64(ce[1]);
    const float k0 = wave_sum(ok[0]), k1 = wave_sum(ok[1]);     // small integers: exact in any order
    if (lane == 0) {
        pair_put(row + 0, pair_get(row + 0) + s0);
        pair_put(row + 2, pair_get(row + 2) + s1);
        row[4] += k0;
        row[5] += k1;
        row[6] += (float)B;
    }
}

// ---- AS:329: sum (x_rgba - ori)^2. grid = (workgroups per view, views). Lane t of workgroup k takes pixels k * 256 + t,
// + gridDim.x * 256, ... of its view: consecutive lanes read consecutive pixels - 128 bits of x_rgba per lane (a wave reads
// 1 KB in a row), and 128 bits of a float image or 32 of a uint8 one. Each lane sums its pixels in order, in double. The
// pixel -> lane map and every order are the same whatever the image type, so the bits are.
template <bool U8>
__device__ __forceinline__ float4 load_ori_pixel(const void* base, long p) {
    if (U8) {
        const uchar4 o = reinterpret_cast<const uchar4*>(base)[p];
        return make_float4((float)o.x, (float)o.y, (float)o.z, (float)o.w);
    }
    return reinterpret_cast<const float4*>(base)[p];
}
__device__ __forceinline__ double sq4(const float4 x, const float4 o, double acc) {
    const double d0 = (double)x.x - (double)o.x, d1 = (double)x.y - (double)o.y;
    const double d2 = (double)x.z - (double)o.z, d3 = (double)x.w - (double)o.w;
    acc = fma(d0, d0, acc);
    acc = fma(d1, d1, acc);
    acc = fma(d2, d2, acc);
    acc = fma(d3, d3, acc);
    return acc;
}

template <bool U8>
__global__ __launch_bounds__(256) void img_sqerr_kernel(const float4* __restrict__ x, OriViews tab, long P, double* __restrict__ partials) {
    __shared__ double wsum[4];
    const void* ob = tab.ori[blockIdx.y];
    const float4* xv = x + (long)blockIdx.y * P;
    const long stride = (long)gridDim.x * 256;
    double acc = 0.0;
#pragma unroll 4
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += stride) acc = sq4(xv[p], load_ori_pixel<U8>(ob, p), acc);
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one workgroup: the partials in a fixed order, then the row
__global__ __launch_bounds__(256) void img_sqerr_finish_kernel(const double* __restrict__ partials, int n_partials, double count,
                                                               float* __restrict__ row) {
    __shared__ double wsum[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        pair_put(row + 7, pair_get(row + 7) + (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]));
        pair_put(row + 9, pair_get(row + 9) + count);
    }
}

// ---- the beta term of AS:336 in d loss / d x_rgba: g += scale (x - ori), one pixel (128 bits of x and g) per lane
template <bool U8>
__global__ __launch_bounds__(256) void img_sqerr_grad_add_kernel(const float4* __restrict__ x, OriViews tab, long P, float scale,
                                                                 float4* __restrict__ g) {
    const void* ob = tab.ori[blockIdx.y];                                // grid = (workgroups per view, views), as img_sqerr_kernel
    const float4* xv = x + (long)blockIdx.y * P;
    float4* gp = g + (long)blockIdx.y * P;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        const float4 o = load_ori_pixel<U8>(ob, p);
        const float4 xp = xv[p];
        float4 gv = gp[p];
        gv.x = __fadd_rn(gv.x, __fmul_rn(scale, __fsub_rn(xp.x, o.x)));
        gv.y = __fadd_rn(gv.y, __fmul_rn(scale, __fsub_rn(xp.y, o.y)));
        gv.z = __fadd_rn(gv.z, __fmul_rn(scale, __fsub_rn(xp.z, o.z)));
        gv.w = __fadd_rn(gv.w, __fmul_rn(scale, __fsub_rn(xp.w, o.w)));
        gp[p] = gv;
    }
}

// ---- AS:405-431
__global__ __launch_bounds__(64) void attack_epoch_close_kernel(const float* __restrict__ row, float* __restrict__ best, int epoch,
                                                                int targeted, float* __restrict__ record, int* __restrict__ flag) {
    if (threadIdx.x != 0) return;
    attack_epoch_close_body(row, best, epoch, targeted, false, record, flag);      // a tie goes to the later epoch
}

// ---- the best tensor of AS:426/431: copied when the close said so. The flag word is wave-uniform (one scalar load).
__global__ __launch_bounds__(256) void copy_if_kernel(const int* __restrict__ flag, const float* __restrict__ src, float* __restrict__ dst,
                                                      long n, int vec) {
    if (flag[0] == 0) return;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    long done = 0;
    if (vec) {
        const long n4 = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (long i = t; i < n4; i += stride) d4[i] = s4[i];
        done = n4 << 2;
    }
    for (long i = done + t; i < n; i += stride) dst[i] = src[i];
}

// ---- AS:401-402: what cv2.imwrite makes of a float image (to_u8, common.h).
__global__ __launch_bounds__(256) void export_u8_kernel(const float* __restrict__ src, long n, unsigned char* __restrict__ dst) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    const long n4 = n >> 2;
    const float4* s4 = reinterpret_cast<const float4*>(src);
    unsigned* d4 = reinterpret_cast<unsigned*>(dst);
    for (long i = t; i < n4; i += stride) {
        const float4 v = s4[i];
        d4[i] = to_u8(v.x) | (to_u8(v.y) << 8) | (to_u8(v.z) << 16) | (to_u8(v.w) << 24);
    }
    for (long i = (n4 << 2) + t; i < n; i += stride) dst[i] = (unsigned char)to_u8(src[i]);
}

static unsigned stream_grid(long work_items) {
    long b = (work_items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > kSqerrBlocks ? kSqerrBlocks : b));
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_abi_revision(void) { return 15; }

extern "C" int nerfail_attack_logit_stats(const float* cla, const float* ori_cla, int B, int C, int label, float* row, void* stream) {
    NF_REQUIRE(B >= 0, "B is negative");
    NF_REQUIRE(C >= 1 && C <= NERFAIL_ATTACK_MAX_CLASSES, "C must be 1..32");
    NF_REQUIRE(label >= 0 && label < C, "label must be a class index");
    if (B == 0) return NERFAIL_OK;
    NF_REQUIRE(cla != nullptr && ori_cla != nullptr && row != nullptr, "NULL pointer");
    attack_logit_stats_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(cla, ori_cla, B, C, label, row);
    NF_LAUNCHED("attack_logit_stats_kernel");
    return NERFAIL_OK;
}

extern "C" size_t nerfail_img_sqerr_scratch_bytes(void) { return (size_t)kSqerrBlocks * sizeof(double); }

static int fill_views(const void* const* ori_views_host, int v0, int n_views, OriViews* tab) {
    tab->nv = n_views - v0 < kSqerrViews ? n_views - v0 : kSqerrViews;
    for (int i = 0; i < kSqerrViews; ++i) tab->ori[i] = ori_views_host[v0 + (i < tab->nv ? i : 0)];
    return tab->nv;
}

extern "C" int nerfail_img_sqerr(const float* x_rgba, const void* const* ori_views_host, int n_views, int64_t P, int ori_is_u8,
                                 void* scratch, float* row, void* stream) {
    NF_REQUIRE(n_views >= 0 && P >= 0, "negative size");
    if ((int64_t)n_views * P == 0) return NERFAIL_OK;
    NF_REQUIRE(x_rgba != nullptr && ori_views_host != nullptr && scratch != nullptr && row != nullptr, "NULL pointer");
    NF_REQUIRE(aligned16(x_rgba) && (reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "x_rgba must be 16-byte, scratch 8-byte aligned");
    for (int v = 0; v < n_views; ++v) {
        NF_REQUIRE(ori_views_host[v] != nullptr, "a view has a NULL image");
        NF_REQUIRE((reinterpret_cast<uintptr_t>(ori_views_host[v]) & (ori_is_u8 ? 3 : 15)) == 0, "a view's image is not aligned to a pixel");
    }
    for (int v0 = 0; v0 < n_views; v0 += kSqerrViews) {
        OriViews tab;
        const int nv = fill_views(ori_views_host, v0, n_views, &tab);
        long bx = (P + 1023) / 1024;                                   // ~4 pixels per lane, at most kSqerrBlocks workgroups in all
        bx = bx > kSqerrBlocks / nv ? kSqerrBlocks / nv : (bx < 1 ? 1 : bx);
        const unsigned blocks = (unsigned)bx * (unsigned)nv;
        const dim3 grid((unsigned)bx, (unsigned)nv);
        const float4* x = (const float4*)x_rgba + (int64_t)v0 * P;
        if (ori_is_u8) img_sqerr_kernel<true><<<grid, dim3(256), 0, as_stream(stream)>>>(x, tab, (long)P, (double*)scratch);
        else img_sqerr_kernel<false><<<grid, dim3(256), 0, as_stream(stream)>>>(x, tab, (long)P, (double*)scratch);
        NF_LAUNCHED("img_sqerr_kernel");
        img_sqerr_finish_kernel<<<dim3(1), dim3(256), 0, as_stream(stream)>>>((const double*)scratch, (int)blocks, 4.0 * (double)P * (double)nv, row);
        NF_LAUNCHED("img_sqerr_finish_kernel");
    }
    return NERFAIL_OK;
}

extern "C" int nerfail_img_sqerr_grad_add(const float* x_rgba, const void* const* ori_views_host, int n_views, int64_t P,
                                          int ori_is_u8, float scale, float* g, void* stream) {
    NF_REQUIRE(n_views >= 0 && P >= 0, "negative size");
    if ((int64_t)n_views * P == 0) return NERFAIL_OK;
    NF_REQUIRE(x_rgba != nullptr && ori_views_host != nullptr && g != nullptr, "NULL pointer");
    NF_REQUIRE(aligned16(x_rgba) && aligned16(g), "x_rgba and g must be 16-byte aligned");
    for (int v = 0; v < n_views; ++v) {
        NF_REQUIRE(ori_views_host[v] != nullptr, "a view has a NULL image");
        NF_REQUIRE((reinterpret_cast<uintptr_t>(ori_views_host[v]) & (ori_is_u8 ? 3 : 15)) == 0, "a view's image is not aligned to a pixel");
    }
    for (int v0 = 0; v0 < n_views; v0 += kSqerrViews) {
        OriViews tab;
        const int nv = fill_views(ori_views_host, v0, n_views, &tab);
        long bx = (P + 255) / 256;
        bx = bx > kSqerrBlocks / nv ? kSqerrBlocks / nv : (bx < 1 ? 1 : bx);
        const dim3 grid((unsigned)bx, (unsigned)nv);
        const float4* x = (const float4*)x_rgba + (int64_t)v0 * P;
        float4* gv = (float4*)g + (int64_t)v0 * P;
        if (ori_is_u8) img_sqerr_grad_add_kernel<true><<<grid, dim3(256), 0, as_stream(stream)>>>(x, tab, (long)P, scale, gv);
        else img_sqerr_grad_add_kernel<false><<<grid, dim3(256), 0, as_stream(stream)>>>(x, tab, (long)P, scale, gv);
        NF_LAUNCHED("img_sqerr_grad_add_kernel");
    }
    return NERFAIL_OK;
}

extern "C" int nerfail_attack_epoch_close(const float* row, float* best, int epoch, int targeted, float* record, int32_t* flag,
                                          void* stream) {
    NF_REQUIRE(row != nullptr && best != nullptr && record != nullptr && flag != nullptr, "NULL pointer");
    NF_REQUIRE(epoch >= 0 && epoch < (1 << 24), "epoch must be in [0, 2^24)");
    attack_epoch_close_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(row, best, epoch, targeted != 0, record, flag);
    NF_LAUNCHED("attack_epoch_close_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_copy_if(const int32_t* flag, const float* src, float* dst, int64_t n, void* stream) {
    NF_REQUIRE(n >= 0, "n is negative");
    if (n == 0) return NERFAIL_OK;
    NF_REQUIRE(flag != nullptr && src != nullptr && dst != nullptr, "NULL pointer");
    NF_REQUIRE((reinterpret_cast<uintptr_t>(src) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0, "src and dst must be float aligned");
    const int vec = aligned16(src) && aligned16(dst);
    copy_if_kernel<<<dim3(stream_grid((long)((n + 3) / 4))), dim3(256), 0, as_stream(stream)>>>(flag, src, dst, (long)n, vec);
    NF_LAUNCHED("copy_if_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_export_u8(const float* src, int64_t n, unsigned char* dst, void* stream) {
    NF_REQUIRE(n >= 0, "n is negative");
    if (n == 0) return NERFAIL_OK;
    NF_REQUIRE(src != nullptr && dst != nullptr, "NULL pointer");
    NF_REQUIRE(aligned16(src) && (reinterpret_cast<uintptr_t>(dst) & 3) == 0, "src must be 16-byte, dst 4-byte aligned");
    export_u8_kernel<<<dim3(stream_grid((long)((n + 3) / 4))), dim3(256), 0, as_stream(stream)>>>(src, (long)n, dst);
    NF_LAUNCHED("export_u8_kernel");
    return NERFAIL_OK;
}
