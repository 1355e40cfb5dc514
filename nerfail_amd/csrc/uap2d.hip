// The UAP-2D baseline (attack_UAP_2D.py:241-358 = UA, deepfool.py:10-111 with universal_2d = DF) around the classifier: one
// DeepFool step on the ONE image-plane table [P,3] every view shares, and the table's update with the +-epsilon projection of
// UA:317-319. The step's inputs are the class gradients with respect to the classifier's planar NCHW input (nerfail_cnn_bwd_data_multi,
// or autograd); the clip of GN:367 stands between that input and the table, so every gradient passes through nerfail_u2d_fwd's
// pass mask first (torch.clip's backward, where(pass, grad, 0), as u2d_step_kernel has it).
//
// nerfail_uap2d_step = norms + choose + apply, three launches with no host in between. The norms are two-stage with a fixed tree
// and double partials (deepfool_norms_kernel's shape); the choice is deepfool_choose.h's, the function nerfail_deepfool_step
// chooses with; the apply is a pure stream in u2d_step_kernel's shape: a lane owns four consecutive pixels (16 B of each
// gradient plane, 48 B of r0 / rot / r_out, 4 B of the mask), the table is cut at ITS 16-byte boundaries into a scalar head,
// whole quads and a scalar tail. No LDS beyond the reduction, no atomics; every output element is written by one lane: the same
// bits on every run.
#include "common.h"
#include "deepfool_choose.h"

namespace nerfail {
namespace {

constexpr int kUapNormBlock = 256;
constexpr int kUapNormQuads = NERFAIL_UAP2D_NORM_TERMS / 12;   // quads per lane: 4 pixels x 3 channels = 12 float32 terms each
constexpr long kUapNormPixels = (long)kUapNormBlock * kUapNormQuads * 4;   // pixels of one norm workgroup
constexpr int kUapBlocks = 512;              // x 256 lanes x 4 pixels in flight before a lane of the apply loops
constexpr size_t kUapTailBytes = 64;         // {norms2[8], best, scale} behind the partials

__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

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
// the mask bytes of pixels p .. p + 3 as one word: a 32-bit load where the address allows
__device__ __forceinline__ unsigned load_mask4(const unsigned char* __restrict__ m) {
    if ((reinterpret_cast<uintptr_t>(m) & 3) == 0) return *reinterpret_cast<const unsigned*>(m);
    return (unsigned)m[0] | ((unsigned)m[1] << 8) | ((unsigned)m[2] << 16) | ((unsigned)m[3] << 24);
}

// torch.clamp(v, lo, hi): a NaN stays
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- norms2[k-1] = sum over pixels and channels whose pass bit is set of (G_k - G_0)^2, first stage. G = [C][3][P] planar.
// Quad q = pixels 4 q .. 4 q + 3; lane t of workgroup b owns quads (b * kUapNormQuads + i) * 256 + t, i = 0 .. kUapNormQuads - 1,
// and adds their NERFAIL_UAP2D_NORM_TERMS terms per competitor in float32, in order (quad, pixel, channel; one rounded subtract,
// multiply and add per term, a cleared bit adding exactly 0 whatever the gradient holds), before it widens to double: the wave,
// then the four waves, in deepfool_norms_kernel's fixed tree. The last quad of the plane may be partial: scalar loads, pixels
// past P add 0.
template <int C>
__global__ __launch_bounds__(kUapNormBlock) void uap2d_norms_kernel(const float* __restrict__ G, long P,
                                                                    const unsigned char* __restrict__ mask,
                                                                    double* __restrict__ partial) {
    __shared__ double red[C - 1][kUapNormBlock / 64];
    float acc[C - 1];
#pragma unroll
    for (int k = 0; k < C - 1; ++k) acc[k] = 0.f;
    const long nq = (P + 3) >> 2;
#pragma unroll
    for (int i = 0; i < kUapNormQuads; ++i) {
        const long q = ((long)blockIdx.x * kUapNormQuads + i) * kUapNormBlock + threadIdx.x;
        if (q >= nq) continue;
        const long p = 4 * q;
        const bool full = p + 3 < P;
        unsigned m;
        float g0[3][4];
        if (full) {
            m = load_mask4(mask + p);
#pragma unroll
            for (int c = 0; c < 3; ++c) load4(G + (long)c * P + p, g0[c]);
        } else {
            m = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = p + j < P;
                if (in) m |= (unsigned)mask[p + j] << (8 * j);
#pragma unroll
                for (int c = 0; c < 3; ++c) g0[c][j] = in ? G[(long)c * P + p + j] : 0.f;
            }
        }
#pragma unroll
        for (int k = 1; k < C; ++k) {
            float g[3][4];
            const float* Gk = G + (long)k * 3 * P;
            if (full) {
#pragma unroll
                for (int c = 0; c < 3; ++c) load4(Gk + (long)c * P + p, g[c]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) g[c][j] = (p + j < P) ? Gk[(long)c * P + p + j] : 0.f;
            }
            float a = acc[k - 1];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float d = __fsub_rn(g[c][j], g0[c][j]);
                    const float t = ((m >> (8 * j + c)) & 1u) ? __fmul_rn(d, d) : 0.f;   // (a cleared bit of a pixel past P too)
                    a = __fadd_rn(a, t);
                }
            acc[k - 1] = a;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < C - 1; ++k) {
        double v = (double)acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[k][wv] = v;
    }
    __syncthreads();
    if (threadIdx.x < C - 1) {
        double v = 0.;
#pragma unroll
        for (int w = 0; w < kUapNormBlock / 64; ++w) v += red[threadIdx.x][w];
        partial[(long)blockIdx.x * (C - 1) + threadIdx.x] = v;
    }
}

// ---- the norm finish and DF:81-96: deepfool_choose.h, the function deepfool_choose_kernel runs
__global__ __launch_bounds__(256) void uap2d_choose_kernel(const double* __restrict__ partial, long nblocks, int K,
                                                           const nerfail_deepfool_record* __restrict__ rec, float* __restrict__ norms2,
                                                           int* __restrict__ best_out, float* __restrict__ scale_out,
                                                           int* __restrict__ trace_slot) {
    __shared__ double red[256];
    __shared__ float n2[NERFAIL_DEEPFOOL_MAX_COMPETITORS];
    deepfool_choose_body(partial, nblocks, K, rec, norms2, best_out, scale_out, trace_slot, red, n2);
}

// DF:98-101 for one element: rot' = rot + scale * masked(G_best - G_0) when something was chosen, r = clamp(r0 + overshoot rot')
__device__ __forceinline__ float apply_elem(bool move, float sc, float gb, float g0, unsigned bit, float overshoot, float r0, float& rot) {
    if (move) {
        const float d = bit ? __fsub_rn(gb, g0) : 0.f;                     // torch.clip's backward: where(pass, grad, 0)
        rot = __fadd_rn(rot, __fmul_rn(sc, d));
    }
    return clamp_keep_nan(__fadd_rn(r0, __fmul_rn(overshoot, rot)), -255.f, 255.f);
}

// ---- DF:98-101. The tables are cut at the 16-byte boundaries of rot (h pixels with (rot + 3 h) % 4 floats == 0 <=> h == rot's
// float index mod 4): a scalar head, whole quads, a scalar tail; r0 and r_out take 128-bit accesses wherever their own addresses
// allow (always, when the three tables share their alignment), the gradient planes and the mask likewise.
__global__ __launch_bounds__(256) void uap2d_apply_kernel(const float* __restrict__ G, long P, int C, const unsigned char* __restrict__ mask,
                                                          const int* __restrict__ best, const float* __restrict__ scale, float overshoot,
                                                          const float* __restrict__ r0, float* __restrict__ rot, float* __restrict__ r_out) {
    const int k = best[0];
    const float sc = scale[0];
    // scale 0 = "no class selected": rot unchanged. `best` comes from device memory: an index outside 1..C-1 must never become
    // an address.
    const bool move = sc != 0.f && k >= 1 && k < C;
    const float* Gb = G + (move ? (long)k * 3 * P : 0L);
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    long head = (long)((reinterpret_cast<uintptr_t>(rot) >> 2) & 3);
    head = head < P ? head : P;
    const long nq = (P - head) >> 2, tail = (P - head) & 3;
    for (long q = t; q < nq; q += stride) {
        const long p = head + 4 * q;
        float rv[12], iv[12], out[12], a0[3][4], ab[3][4];
        load12(rot + 3 * p, rv);
        load12(r0 + 3 * p, iv);
        unsigned m = 0;
        if (move) {
            m = load_mask4(mask + p);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                load4(G + (long)c * P + p, a0[c]);
                load4(Gb + (long)c * P + p, ab[c]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j) a0[c][j] = ab[c][j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                out[3 * j + c] = apply_elem(move, sc, ab[c][j], a0[c][j], (m >> (8 * j + c)) & 1u, overshoot, iv[3 * j + c], rv[3 * j + c]);
        if (move) store12(rot + 3 * p, rv);
        store12(r_out + 3 * p, out);
    }
    if (blockIdx.x == 0 && threadIdx.x < head + tail) {                    // at most 3 + 3 pixels
        const long p = threadIdx.x < head ? (long)threadIdx.x : head + 4 * nq + ((long)threadIdx.x - head);
        const unsigned m = move ? mask[p] : 0u;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float rr = rot[3 * p + c];
            const float gb = move ? Gb[(long)c * P + p] : 0.f, g0 = move ? G[(long)c * P + p] : 0.f;
            r_out[3 * p + c] = apply_elem(move, sc, gb, g0, (m >> c) & 1u, overshoot, r0[3 * p + c], rr);
            if (move) rot[3 * p + c] = rr;
        }
    }
}

// UA:317-319 with DF:109 for one element: dr = r_final - t, t' = t + dr, clamp(t', -epsilon, +epsilon) (torch.clamp: a NaN stays)
__device__ __forceinline__ float accumulate_elem(float t, float rf, float epsilon) {
    return clamp_keep_nan(__fadd_rn(t, __fsub_rn(rf, t)), -epsilon, epsilon);
}

// ---- UA:317-319. The table is cut at its 16-byte boundaries: a scalar head, float4 groups, a scalar tail.
__global__ __launch_bounds__(256) void uap2d_accumulate_kernel(float* __restrict__ table, const float* __restrict__ r_final, float epsilon,
                                                               long n) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    long head = (long)((4 - ((reinterpret_cast<uintptr_t>(table) >> 2) & 3)) & 3);
    head = head < n ? head : n;
    const long ng = (n - head) >> 2, tail = (n - head) & 3;
    for (long g = t; g < ng; g += stride) {
        const long e = head + 4 * g;
        const float4 tv = *reinterpret_cast<const float4*>(table + e);
        float rf[4];
        load4(r_final + e, rf);
        *reinterpret_cast<float4*>(table + e) = make_float4(accumulate_elem(tv.x, rf[0], epsilon), accumulate_elem(tv.y, rf[1], epsilon),
                                                            accumulate_elem(tv.z, rf[2], epsilon), accumulate_elem(tv.w, rf[3], epsilon));
    }
    if (blockIdx.x == 0 && threadIdx.x < head + tail) {                    // at most 3 + 3 elements
        const long e = threadIdx.x < head ? (long)threadIdx.x : head + 4 * ng + ((long)threadIdx.x - head);
        table[e] = accumulate_elem(table[e], r_final[e], epsilon);
    }
}

bool aligned_to(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

long norm_blocks(int64_t P) { return (long)((P + kUapNormPixels - 1) / kUapNormPixels); }

unsigned stream_blocks(int64_t groups) {                                   // ~2 groups of four per lane, at most kUapBlocks workgroups
    long bx = (long)((groups + 511) / 512);
    return (unsigned)(bx > kUapBlocks ? kUapBlocks : (bx < 1 ? 1 : bx));
}

size_t partial_bytes(int n_rhs, int64_t P) { return (size_t)norm_blocks(P) * (n_rhs - 1) * sizeof(double); }

}  // namespace
}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_uap2d_revision(void) { return 1; }

extern "C" size_t nerfail_uap2d_step_scratch_bytes(int n_rhs, int64_t P) {
    if (n_rhs < 2 || n_rhs > 8 || P <= 0 || P > ((int64_t)1 << 31)) return 0;
    return partial_bytes(n_rhs, P) + kUapTailBytes;
}

extern "C" int nerfail_uap2d_step(const float* grads, int n_rhs, int64_t P, const unsigned char* pass_mask,
                                  const nerfail_deepfool_record* record, void* scratch, size_t scratch_bytes, float overshoot,
                                  const float* r0, float* rot, float* r_out, int32_t* trace_slot, void* stream) {
    NF_REQUIRE(n_rhs >= 2 && n_rhs <= 8, "n_rhs must be in 2..8");
    NF_REQUIRE(P > 0 && P <= ((int64_t)1 << 31), "P must be in 1..2^31");
    NF_REQUIRE(grads && pass_mask && record && scratch && r0 && rot && r_out && trace_slot, "NULL pointer");
    NF_REQUIRE(isfinite(overshoot), "overshoot must be finite");
    NF_REQUIRE(scratch_bytes >= nerfail_uap2d_step_scratch_bytes(n_rhs, P), "scratch too small (nerfail_uap2d_step_scratch_bytes)");
    NF_REQUIRE(aligned_to(scratch, 7), "scratch must be 8-byte aligned");
    NF_REQUIRE(aligned_to(grads, 3) && aligned_to(r0, 3) && aligned_to(rot, 3) && aligned_to(r_out, 3) && aligned_to(record, 3) &&
                   aligned_to(trace_slot, 3),
               "grads, r0, rot, r_out, record and trace_slot must be 4-byte aligned");
    hipStream_t s = as_stream(stream);
    const long nb = norm_blocks(P);
    double* partial = (double*)scratch;
    float* tail = (float*)((char*)scratch + partial_bytes(n_rhs, P));
    int* best = (int*)(tail + NERFAIL_DEEPFOOL_MAX_COMPETITORS);
    float* scale = tail + NERFAIL_DEEPFOOL_MAX_COMPETITORS + 1;
    const dim3 grid((unsigned)nb), block(kUapNormBlock);
#define NF_UAP_NORMS(C) uap2d_norms_kernel<C><<<grid, block, 0, s>>>(grads, (long)P, pass_mask, partial)
    switch (n_rhs) {
        case 2: NF_UAP_NORMS(2); break;
        case 3: NF_UAP_NORMS(3); break;
        case 4: NF_UAP_NORMS(4); break;
        case 5: NF_UAP_NORMS(5); break;
        case 6: NF_UAP_NORMS(6); break;
        case 7: NF_UAP_NORMS(7); break;
        default: NF_UAP_NORMS(8); break;
    }
#undef NF_UAP_NORMS
    NF_LAUNCHED("uap2d_norms_kernel");
    uap2d_choose_kernel<<<dim3(1), dim3(256), 0, s>>>(partial, nb, n_rhs - 1, record, tail, best, scale, trace_slot);
    NF_LAUNCHED("uap2d_choose_kernel");
    uap2d_apply_kernel<<<dim3(stream_blocks(P / 4)), dim3(256), 0, s>>>(grads, (long)P, n_rhs, pass_mask, best, scale, overshoot, r0, rot,
                                                                         r_out);
    NF_LAUNCHED("uap2d_apply_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_uap2d_accumulate(float* table, const float* r_final, float epsilon, int64_t n, void* stream) {
    NF_REQUIRE(table && r_final, "NULL pointer");
    NF_REQUIRE(n > 0 && n <= 3 * ((int64_t)1 << 31), "n must be in 1..3 * 2^31");
    NF_REQUIRE(epsilon >= 0.f, "epsilon must be >= 0 (and not NaN)");
    NF_REQUIRE(aligned_to(table, 3) && aligned_to(r_final, 3), "table and r_final must be 4-byte aligned");
    uap2d_accumulate_kernel<<<dim3(stream_blocks(n / 4)), dim3(256), 0, as_stream(stream)>>>(table, r_final, epsilon, (long)n);
    NF_LAUNCHED("uap2d_accumulate_kernel");
    return NERFAIL_OK;
}
