// The IGSM-2D baseline (attack_IGSM_2D.py:263-416 = IG, model/GaussNet.py:340-385 = GN, MyDataset.py:235-294 = MD) on the
// device: universal_2D_net's forward up to the classifier input (white background, + r, clip, NCHW) from a resident uint8 store
// in one streaming launch, and everything after the classifier's backward (clip backward, sign step, +-epsilon clamp, the write
// back into the per-view table, IG:335-379) in another. The image-loss statistic of IG:316 and the epoch close with IG's strict
// rule (IG:407-416) complete the loop, so an epoch runs without a host read.
//
// Both big kernels are pure streams: a lane owns four consecutive pixels (16 B of a U8C4 store, 48 B of r, 48 B of planar
// output), consecutive lanes take consecutive quads, a workgroup never straddles two views (grid.y = the view of the batch,
// so idx[b] is one scalar load). No LDS, no atomics; every output element is written by one lane: the same bits on every run.
#include "common.h"
#include "attack_close.h"

namespace nerfail {
namespace {

constexpr int kU2dBlocksPerView = 512;       // x 256 lanes x 4 pixels = 524 288 pixels in flight per view before a lane loops
constexpr int kU2dSqerrBlocks = 2048;        // partial slots of nerfail_u2d_sqerr = nerfail_img_sqerr_scratch_bytes() / 8
constexpr int kU2dSqerrViews = 16;           // views per launch of the statistic (nerfail_img_sqerr's chunk)

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// 12 consecutive floats (four pixels x three channels): three 128-bit accesses when the address allows, else scalar
__device__ __forceinline__ void load12(const float* __restrict__ s, float (&v)[12]) {
    if (al16(s)) {
        const float4 a = reinterpret_cast<const float4*>(s)[0], b = reinterpret_cast<const float4*>(s)[1],
                     c = reinterpret_cast<const float4*>(s)[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = s[k];
    }
}
__device__ __forceinline__ void store12(float* __restrict__ d, const float (&v)[12]) {
    if (al16(d)) {
        reinterpret_cast<float4*>(d)[0] = make_float4(v[0], v[1], v[2], v[3]);
        reinterpret_cast<float4*>(d)[1] = make_float4(v[4], v[5], v[6], v[7]);
        reinterpret_cast<float4*>(d)[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) d[k] = v[k];
    }
}
__device__ __forceinline__ void load4(const float* __restrict__ s, float (&v)[4]) {
    if (al16(s)) {
        const float4 a = *reinterpret_cast<const float4*>(s);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
        v[0] = s[0]; v[1] = s[1]; v[2] = s[2]; v[3] = s[3];
    }
}
__device__ __forceinline__ void store4(float* __restrict__ d, float a, float b, float c, float e) {
    if (al16(d)) {
        *reinterpret_cast<float4*>(d) = make_float4(a, b, c, e);
    } else {
        d[0] = a; d[1] = b; d[2] = c; d[3] = e;
    }
}

// one pixel of a store as three floats on the white background of MD:247-255 (white_u8: nerfail_cls_batch's definition)
template <int CH>
__device__ __forceinline__ void load_pixel(const unsigned char* __restrict__ v, long p, float& o0, float& o1, float& o2) {
    if (CH == 4) {
        const unsigned w = *reinterpret_cast<const unsigned*>(v + 4 * p);
        o0 = white_u8(w, 0);
        o1 = white_u8(w, 8);
        o2 = white_u8(w, 16);
    } else {
        o0 = (float)v[3 * p];
        o1 = (float)v[3 * p + 1];
        o2 = (float)v[3 * p + 2];
    }
}

// GN:363-367 for one element: v = o + r (one rounded add), x = torch.clip(v, 0, 255) (a NaN stays), bit = 0 <= v <= 255
// (what torch.clip's backward lets through: both bounds inclusive, false for a NaN)
__device__ __forceinline__ unsigned fwd_elem(float o, float r, float& x) {
    const float v = __fadd_rn(o, r);
    x = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    return (v >= 0.f && v <= 255.f) ? 1u : 0u;
}

// torch.max / torch.min over a stacked pair (IG:373-377): a NaN on either side is the result, a tie keeps the first
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b > a ? b : a)); }
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : (b < a ? b : a)); }

// IG:343-377 for one element; g already is the gradient behind the clip
__device__ __forceinline__ float step_elem(float r, float g, float init, float a, float epsilon, int targeted) {
    const float sg = (g > 0.f) ? 1.f : ((g < 0.f) ? -1.f : 0.f);                // torch.sign: sign(+-0) = 0, sign(NaN) = 0
    const float st = __fmul_rn(a, sg);
    float q = targeted ? __fsub_rn(r, st) : __fadd_rn(r, st);
    q = nan_max(q, __fsub_rn(init, epsilon));
    q = nan_min(q, __fadd_rn(init, epsilon));
    return q;
}

// ---- GN:356-370 with MD:247-255. grid = (workgroups per view, B). The view is cut as nerfail_cls_batch cuts it: a scalar head
// up to the first wide-load boundary of the STORE, whole 4-pixel quads, a scalar tail. r and the outputs are accessed 128 bits
// wide wherever their own addresses allow (always, when P is a multiple of 4 and the bases are 16-byte aligned).
template <int F>
__global__ __launch_bounds__(256) void u2d_fwd_kernel(const unsigned char* __restrict__ images, const long long* __restrict__ idx, long N,
                                                      long P, const float* __restrict__ r, int r_shared, float* __restrict__ x_rgb,
                                                      float* __restrict__ cls_in, unsigned char* __restrict__ pass_mask) {
    constexpr int CH = (F == NERFAIL_EVAL_U8C4) ? 4 : 3;
    const int b = blockIdx.y;
    const long long i = idx[b];
    const bool bad = (i < 0 || i >= (long long)N);
    float* xo = x_rgb != nullptr ? x_rgb + (long)b * 3 * P : nullptr;
    float* co = cls_in != nullptr ? cls_in + (long)b * 3 * P : nullptr;
    unsigned char* mo = pass_mask != nullptr ? pass_mask + (long)b * P : nullptr;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    if (bad) {                                                             // views of NaN, a zero mask; neither input is touched
        for (long e = t; e < 3 * P; e += stride) {
            if (xo != nullptr) xo[e] = NAN;
            if (co != nullptr) co[e] = NAN;
        }
        if (mo != nullptr)
            for (long e = t; e < P; e += stride) mo[e] = 0;
        return;
    }
    const unsigned char* v = images + (long)i * CH * P;
    const float* rr = r + (r_shared ? 0L : (long)i * 3 * P);
    const uintptr_t a = reinterpret_cast<uintptr_t>(v);
    long head = (CH == 4) ? (long)(((16 - (a & 15)) & 15) >> 2) : (long)(a & 3);    // U8C3: (a + 3 h) % 4 == 0 <=> h == a mod 4
    head = head < P ? head : P;
    const long nq = (P - head) >> 2, tail = (P - head) & 3;
    for (long q = t; q < nq; q += stride) {
        const long p = head + 4 * q;
        float o[12];                                                       // o[3 j + c]: pixel p + j, channel c
        if (CH == 4) {
            const uint4 w = *reinterpret_cast<const uint4*>(v + 4 * p);
            const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[3 * j] = white_u8(ww[j], 0);
                o[3 * j + 1] = white_u8(ww[j], 8);
                o[3 * j + 2] = white_u8(ww[j], 16);
            }
        } else {
            const unsigned* w = reinterpret_cast<const unsigned*>(v + 3 * p);       // 12 bytes = pixels p .. p + 3
            const unsigned ww[3] = {w[0], w[1], w[2]};
#pragma unroll
            for (int k = 0; k < 12; ++k) o[k] = (float)((ww[k >> 2] >> (8 * (k & 3))) & 255u);
        }
        float rv[12], x[12];
        load12(rr + 3 * p, rv);
        unsigned m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) m |= fwd_elem(o[3 * j + c], rv[3 * j + c], x[3 * j + c]) << (8 * j + c);
        if (xo != nullptr) store12(xo + 3 * p, x);
        if (co != nullptr) {
            store4(co + p, x[0], x[3], x[6], x[9]);
            store4(co + P + p, x[1], x[4], x[7], x[10]);
            store4(co + 2 * P + p, x[2], x[5], x[8], x[11]);
        }
        if (mo != nullptr) {
            if ((reinterpret_cast<uintptr_t>(mo + p) & 3) == 0) {
                *reinterpret_cast<unsigned*>(mo + p) = m;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) mo[p + j] = (unsigned char)((m >> (8 * j)) & 255u);
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < head + tail) {                    // at most 3 + 3 pixels
        const long p = threadIdx.x < head ? (long)threadIdx.x : head + 4 * nq + ((long)threadIdx.x - head);
        float o[3], x[3];
        load_pixel<CH>(v, p, o[0], o[1], o[2]);
        unsigned m = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) m |= fwd_elem(o[c], rr[3 * p + c], x[c]) << c;
        if (xo != nullptr) { xo[3 * p] = x[0]; xo[3 * p + 1] = x[1]; xo[3 * p + 2] = x[2]; }
        if (co != nullptr) { co[p] = x[0]; co[P + p] = x[1]; co[2 * P + p] = x[2]; }
        if (mo != nullptr) mo[p] = (unsigned char)m;
    }
}

// ---- IG:335-379 in place on row idx[b] of the table. grid = (workgroups per view, B). The row is cut at ITS 16-byte
// boundaries (row i starts at float 3 P i): a scalar head of h pixels with (row + 3 h) % 4 == 0 <=> h == (row's float index) mod 4,
// whole quads, a scalar tail. The planar gradient, the mask and r_init are read 128 / 32 bits wide wherever their addresses allow.
__global__ __launch_bounds__(256) void u2d_step_kernel(float* __restrict__ r, const long long* __restrict__ idx, long N, long P,
                                                       const float* __restrict__ d, const unsigned char* __restrict__ mask,
                                                       const float* __restrict__ r_init, float a, float epsilon, int targeted) {
    const int b = blockIdx.y;
    const long long i = idx[b];
    if (i < 0 || i >= (long long)N) return;                                // the row does not exist: nothing is touched
    float* rr = r + (long)i * 3 * P;
    const float* ri = r_init != nullptr ? r_init + (long)i * 3 * P : nullptr;
    const float* db = d + (long)b * 3 * P;
    const unsigned char* mb = mask + (long)b * P;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    long head = (long)((reinterpret_cast<uintptr_t>(rr) >> 2) & 3);
    head = head < P ? head : P;
    const long nq = (P - head) >> 2, tail = (P - head) & 3;
    for (long q = t; q < nq; q += stride) {
        const long p = head + 4 * q;
        float rv[12], iv[12], out[12], g0[4], g1[4], g2[4];
        load12(rr + 3 * p, rv);
        if (ri != nullptr) {
            load12(ri + 3 * p, iv);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) iv[k] = 0.f;
        }
        load4(db + p, g0);
        load4(db + P + p, g1);
        load4(db + 2 * P + p, g2);
        unsigned m;
        if ((reinterpret_cast<uintptr_t>(mb + p) & 3) == 0) {
            m = *reinterpret_cast<const unsigned*>(mb + p);
        } else {
            m = (unsigned)mb[p] | ((unsigned)mb[p + 1] << 8) | ((unsigned)mb[p + 2] << 16) | ((unsigned)mb[p + 3] << 24);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gj[3] = {g0[j], g1[j], g2[j]};
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float g = ((m >> (8 * j + c)) & 1u) ? gj[c] : 0.f;    // torch.clip's backward: where(pass, grad, 0)
                out[3 * j + c] = step_elem(rv[3 * j + c], g, iv[3 * j + c], a, epsilon, targeted);
            }
        }
        store12(rr + 3 * p, out);
    }
    if (blockIdx.x == 0 && threadIdx.x < head + tail) {                    // at most 3 + 3 pixels
        const long p = threadIdx.x < head ? (long)threadIdx.x : head + 4 * nq + ((long)threadIdx.x - head);
        const unsigned m = mb[p];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g = ((m >> c) & 1u) ? db[(long)c * P + p] : 0.f;
            rr[3 * p + c] = step_elem(rr[3 * p + c], g, ri != nullptr ? ri[3 * p + c] : 0.f, a, epsilon, targeted);
        }
    }
}

// ---- IG:316: sum (x_rgb - o)^2, with img_sqerr_kernel's arithmetic and order (attack_stats.hip): grid = (workgroups per view,
// views); lane t of workgroup k takes pixels k * 256 + t, + gridDim.x * 256, ... of its view and sums them in order, in double;
// a workgroup its lanes; one workgroup the partials. The pixel -> lane map does not depend on the store's format, so the bits
// do not. A view whose index is out of range reads nothing and contributes NaN.
template <int F>
__global__ __launch_bounds__(256) void u2d_sqerr_kernel(const float* __restrict__ x, const unsigned char* __restrict__ images,
                                                        const long long* __restrict__ idx, long N, long P, double* __restrict__ partials) {
    constexpr int CH = (F == NERFAIL_EVAL_U8C4) ? 4 : 3;
    __shared__ double wsum[4];
    const int b = blockIdx.y;
    const long long i = idx[b];
    const bool bad = (i < 0 || i >= (long long)N);
    const float* xv = x + (long)b * 3 * P;
    const unsigned char* v = images + (bad ? 0L : (long)i * CH * P);
    const long stride = (long)gridDim.x * 256;
    double acc = 0.0;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += stride) {
        float o0 = NAN, o1 = NAN, o2 = NAN;
        if (!bad) load_pixel<CH>(v, p, o0, o1, o2);
        const double d0 = (double)xv[3 * p] - (double)o0, d1 = (double)xv[3 * p + 1] - (double)o1, d2 = (double)xv[3 * p + 2] - (double)o2;
        acc = fma(d0, d0, acc);
        acc = fma(d1, d1, acc);
        acc = fma(d2, d2, acc);
    }
    acc = wave_sum_f64(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[(long)blockIdx.y * gridDim.x + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// one workgroup: the partials in a fixed order, then the row (img_sqerr_finish_kernel's order)
__global__ __launch_bounds__(256) void u2d_sqerr_finish_kernel(const double* __restrict__ partials, int n_partials, double count,
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

// ---- IG:392-416
__global__ __launch_bounds__(64) void u2d_epoch_close_kernel(const float* __restrict__ row, float* __restrict__ best, int epoch,
                                                             int targeted, float* __restrict__ record, int* __restrict__ flag) {
    if (threadIdx.x != 0) return;
    attack_epoch_close_body(row, best, epoch, targeted, true, record, flag);              // strict: a tie keeps the earlier epoch
}

bool aligned_to(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

unsigned quad_blocks(int64_t P) {
    long bx = (long)((P / 4 + 511) / 512);                                 // ~2 quads per lane
    return (unsigned)(bx > kU2dBlocksPerView ? kU2dBlocksPerView : (bx < 1 ? 1 : bx));
}

}  // namespace
}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_u2d_revision(void) { return 1; }

extern "C" int nerfail_u2d_fwd(const void* images, int format, int64_t N, int64_t P, const int64_t* idx, int B, const float* r,
                               int r_shared, float* x_rgb, float* cls_in, unsigned char* pass_mask, void* stream) {
    NF_REQUIRE(format == NERFAIL_EVAL_U8C4 || format == NERFAIL_EVAL_U8C3, "format must be NERFAIL_EVAL_U8C4 or NERFAIL_EVAL_U8C3");
    NF_REQUIRE(N >= 0 && B >= 0, "negative size");
    NF_REQUIRE(P > 0, "P must be positive");
    NF_REQUIRE(B <= 65535, "B must be at most 65535");
    NF_REQUIRE(N <= ((int64_t)1 << 31) && P <= ((int64_t)1 << 31), "N and P must be at most 2^31");
    NF_REQUIRE(x_rgb != nullptr || cls_in != nullptr, "x_rgb and cls_in are both NULL");
    NF_REQUIRE(idx != nullptr && r != nullptr && (images != nullptr || N == 0), "NULL pointer");
    NF_REQUIRE(aligned_to(images, format == NERFAIL_EVAL_U8C4 ? 15 : 3), "the store must be 16-byte (U8C4) or 4-byte (U8C3) aligned");
    NF_REQUIRE(aligned_to(r, 3) && aligned_to(x_rgb, 3) && aligned_to(cls_in, 3) && aligned_to(idx, 7),
               "r, x_rgb and cls_in must be 4-byte, idx 8-byte aligned");
    if (B == 0) return NERFAIL_OK;
    const dim3 grid(quad_blocks(P), (unsigned)B);
    hipStream_t st = as_stream(stream);
    if (format == NERFAIL_EVAL_U8C4)
        u2d_fwd_kernel<NERFAIL_EVAL_U8C4><<<grid, dim3(256), 0, st>>>((const unsigned char*)images, (const long long*)idx, (long)N, (long)P, r,
                                                                       r_shared != 0, x_rgb, cls_in, pass_mask);
    else
        u2d_fwd_kernel<NERFAIL_EVAL_U8C3><<<grid, dim3(256), 0, st>>>((const unsigned char*)images, (const long long*)idx, (long)N, (long)P, r,
                                                                       r_shared != 0, x_rgb, cls_in, pass_mask);
    NF_LAUNCHED("u2d_fwd_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_u2d_step(float* r, int64_t N, int64_t P, const int64_t* idx, int B, const float* d_cls_in,
                                const unsigned char* pass_mask, const float* r_init, float a, float epsilon, int targeted, void* stream) {
    NF_REQUIRE(N >= 0 && B >= 0, "negative size");
    NF_REQUIRE(P > 0, "P must be positive");
    NF_REQUIRE(B <= 65535, "B must be at most 65535");
    NF_REQUIRE(N <= ((int64_t)1 << 31) && P <= ((int64_t)1 << 31), "N and P must be at most 2^31");
    NF_REQUIRE(epsilon >= 0.f, "epsilon must be >= 0 (and not NaN)");
    NF_REQUIRE(isfinite(a), "a must be finite");
    NF_REQUIRE(idx != nullptr && d_cls_in != nullptr && pass_mask != nullptr && (r != nullptr || N == 0), "NULL pointer");
    NF_REQUIRE(aligned_to(r, 3) && aligned_to(d_cls_in, 3) && aligned_to(r_init, 3) && aligned_to(idx, 7),
               "r, d_cls_in and r_init must be 4-byte, idx 8-byte aligned");
    if (B == 0) return NERFAIL_OK;
    u2d_step_kernel<<<dim3(quad_blocks(P), (unsigned)B), dim3(256), 0, as_stream(stream)>>>(r, (const long long*)idx, (long)N, (long)P,
                                                                                             d_cls_in, pass_mask, r_init, a, epsilon,
                                                                                             targeted != 0);
    NF_LAUNCHED("u2d_step_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_u2d_sqerr(const float* x_rgb, const void* images, int format, int64_t N, int64_t P, const int64_t* idx, int B,
                                 void* scratch, float* row, void* stream) {
    NF_REQUIRE(format == NERFAIL_EVAL_U8C4 || format == NERFAIL_EVAL_U8C3, "format must be NERFAIL_EVAL_U8C4 or NERFAIL_EVAL_U8C3");
    NF_REQUIRE(N >= 0 && B >= 0, "negative size");
    NF_REQUIRE(P > 0, "P must be positive");
    NF_REQUIRE(B <= 65535, "B must be at most 65535");
    NF_REQUIRE(N <= ((int64_t)1 << 31) && P <= ((int64_t)1 << 31), "N and P must be at most 2^31");
    NF_REQUIRE(scratch != nullptr, "scratch is NULL");
    NF_REQUIRE(x_rgb != nullptr && idx != nullptr && row != nullptr && (images != nullptr || N == 0), "NULL pointer");
    NF_REQUIRE(aligned_to(images, format == NERFAIL_EVAL_U8C4 ? 15 : 3), "the store must be 16-byte (U8C4) or 4-byte (U8C3) aligned");
    NF_REQUIRE(aligned_to(x_rgb, 3) && aligned_to(row, 3) && aligned_to(idx, 7) && aligned_to(scratch, 7),
               "x_rgb and row must be 4-byte, idx and scratch 8-byte aligned");
    hipStream_t st = as_stream(stream);
    for (int v0 = 0; v0 < B; v0 += kU2dSqerrViews) {
        const int nv = B - v0 < kU2dSqerrViews ? B - v0 : kU2dSqerrViews;
        long bx = (long)((P + 1023) / 1024);                               // ~4 pixels per lane, at most kU2dSqerrBlocks workgroups in all
        bx = bx > kU2dSqerrBlocks / nv ? kU2dSqerrBlocks / nv : (bx < 1 ? 1 : bx);
        const dim3 grid((unsigned)bx, (unsigned)nv);
        const float* x = x_rgb + (int64_t)v0 * 3 * P;
        const long long* ix = (const long long*)idx + v0;
        if (format == NERFAIL_EVAL_U8C4)
            u2d_sqerr_kernel<NERFAIL_EVAL_U8C4><<<grid, dim3(256), 0, st>>>(x, (const unsigned char*)images, ix, (long)N, (long)P, (double*)scratch);
        else
            u2d_sqerr_kernel<NERFAIL_EVAL_U8C3><<<grid, dim3(256), 0, st>>>(x, (const unsigned char*)images, ix, (long)N, (long)P, (double*)scratch);
        NF_LAUNCHED("u2d_sqerr_kernel");
        u2d_sqerr_finish_kernel<<<dim3(1), dim3(256), 0, st>>>((const double*)scratch, (int)(bx * nv), 3.0 * (double)P * (double)nv, row);
        NF_LAUNCHED("u2d_sqerr_finish_kernel");
    }
    return NERFAIL_OK;
}

extern "C" int nerfail_u2d_epoch_close(const float* row, float* best, int epoch, int targeted, float* record, int32_t* flag, void* stream) {
    NF_REQUIRE(row != nullptr && best != nullptr && record != nullptr && flag != nullptr, "NULL pointer");
    NF_REQUIRE(epoch >= 0 && epoch < (1 << 24), "epoch must be in [0, 2^24)");
    u2d_epoch_close_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(row, best, epoch, targeted != 0, record, flag);
    NF_LAUNCHED("u2d_epoch_close_kernel");
    return NERFAIL_OK;
}
