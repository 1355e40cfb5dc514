// DeepFool step arithmetic over the perturbation table (deepfool.py:76-102 of the reference): given the class-logit
// gradients G[0..C-1] of one iteration (G[0] = original class; nerfail_gauss_bwd_csr_multi writes them as [C][n,4]),
//   K14a  norms2[k-1] = || G[k] - G[0] ||^2                      (torch.norm(grad_prime) for every competing class)
//   K14b  rot += scale * (G[best] - G[0]);  s = clamp(s0 + overshoot * rot, -255, 255) with s0's alpha channel
// replacing ~12 elementwise / reduction passes of torch over 30-245 MB each (1.8 ms of a 13 ms iteration) by two
// streaming passes. Reductions are two-stage with a fixed tree: bitwise reproducible run to run. Bound: HBM.
// DeepFool revision 1 adds what stood between them as torch launches and host reads: deepfool_gate_kernel (one wave: bump, first
// maximum, break test, |f'| of every competitor) and deepfool_choose_kernel (the norm finish, then the choice of the class and the
// scale on one lane), so that nerfail_deepfool_step is norms + choose + apply with no host in between.
#include "common.h"
#include "deepfool_choose.h"

namespace nerfail {

constexpr int kNormBlock = 256, kNormPerThread = 8;     // float4 per thread

template <int C>
__global__ __launch_bounds__(kNormBlock) void deepfool_norms_kernel(const float4* __restrict__ G, long n, double* __restrict__ partial) {
    __shared__ double red[C - 1][kNormBlock / 64];
    const long base = ((long)blockIdx.x * kNormBlock) * kNormPerThread + threadIdx.x;
    float acc[C - 1];
#pragma unroll
    for (int k = 0; k < C - 1; ++k) acc[k] = 0.f;
#pragma unroll
    for (int i = 0; i < kNormPerThread; ++i) {
        const long e = base + (long)i * kNormBlock;
        if (e < n) {
            const float4 g0 = G[e];
#pragma unroll
            for (int k = 1; k < C; ++k) {
                const float4 g = G[(long)k * n + e];
                const float dx = g.x - g0.x, dy = g.y - g0.y, dz = g.z - g0.z, dw = g.w - g0.w;
                acc[k - 1] += (dx * dx + dy * dy) + (dz * dz + dw * dw);
            }
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
        for (int w = 0; w < kNormBlock / 64; ++w) v += red[threadIdx.x][w];
        partial[(long)blockIdx.x * (C - 1) + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(256) void deepfool_norms_finish_kernel(const double* __restrict__ partial, long nblocks, int K,
                                                                    float* __restrict__ norms2) {
    __shared__ double red[256];
    for (int k = 0; k < K; ++k) {                    // one block: fixed order for every k
        const double r = norms_finish_sum(partial, nblocks, K, k, red);
        if (threadIdx.x == 0) norms2[k] = (float)r;
    }
}

// deepfool.py:53-66 and the f' of :79 / :93 for one view on one wave: lane c holds logit c. Nothing is indexed by a run-time
// value inside the wave (ballots and one shuffle): no scratch.
__global__ __launch_bounds__(64) void deepfool_gate_kernel(const float* __restrict__ cla, int C, int o, int target, float m1, float m2,
                                                           nerfail_deepfool_record* __restrict__ rec) {
    const int lane = threadIdx.x;
    const bool in = lane < C;
    const float v = in ? cla[lane] : -INFINITY;
    const bool bump = in && (target < 0 ? lane == o : lane != target);
    const float vb = bump ? __fadd_rn(v, m1) : v;                                  // :54 / :56-57
    const bool nan = __ballot(vb != vb) != 0ull;
    const float m = wave_max(vb);                                                  // (fmaxf skips a NaN: the flag above decides)
    const unsigned long long eq = __ballot(in && vb == m);
    const int arg = (nan || eq == 0ull) ? -1 : (__ffsll((long long)eq) - 1);       // the FIRST maximum (torch.max, :59)
    const bool done = arg >= 0 && (target < 0 ? arg != o : arg == target);         // :62-66; a row holding a NaN is never done
    const float vo = __shfl(vb, o, 64);
    const float f = fabsf(__fsub_rn(vb, __fadd_rn(vo, m2)));                        // |cla_b[k] - (cla_b[o] + m2)|
    const int n_comp = target < 0 ? C - 1 : 1;
    const bool comp = in && (target < 0 ? lane != o : lane == target);
    if (comp) {
        const int r = target < 0 ? (lane < o ? lane : lane - 1) : 0;
        rec->cls[r] = lane;
        rec->fabs[r] = f;
    }
    if (lane >= n_comp && lane < NERFAIL_DEEPFOOL_MAX_COMPETITORS) {               // the slots no competitor owns
        rec->cls[lane] = -1;
        rec->fabs[lane] = 0.f;
    }
    if (lane == 0) {
        rec->done = done ? 1 : 0;
        rec->argmax = arg;
        rec->n_comp = n_comp;
        rec->targeted = target < 0 ? 0 : 1;
    }
}

// The finish of the norm reduction (same tree, same bits as deepfool_norms_finish_kernel), then deepfool.py:81-96 on lane 0 in
// float32 and in the mirror's operation order: which competitor, and by how much (deepfool_choose.h: nerfail_uap2d_step chooses
// with the same function). tail = {norms2[8], best, scale}.
__global__ __launch_bounds__(256) void deepfool_choose_kernel(const double* __restrict__ partial, long nblocks, int K,
                                                              const nerfail_deepfool_record* __restrict__ rec, float* __restrict__ norms2,
                                                              int* __restrict__ best_out, float* __restrict__ scale_out,
                                                              int* __restrict__ trace_slot) {
    __shared__ double red[256];
    __shared__ float n2[NERFAIL_DEEPFOOL_MAX_COMPETITORS];
    deepfool_choose_body(partial, nblocks, K, rec, norms2, best_out, scale_out, trace_slot, red, n2);
}

__global__ __launch_bounds__(256) void deepfool_apply_kernel(const float4* __restrict__ G, long n, int C, const int* __restrict__ best,
                                                             const float* __restrict__ scale, float overshoot,
                                                             const float4* __restrict__ s0, float4* __restrict__ rot,
                                                             float4* __restrict__ s_out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const int k = best[0];
    const float sc = scale[0];
    float4 r = rot[e];
    // scale 0 = "no class selected" (all candidates inf / NaN): rot unchanged. `best` comes from device memory: an index
    // outside 1..C-1 must never become an address.
    if (sc != 0.f && k >= 1 && k < C) {
        const float4 g0 = G[e], g = G[(long)k * n + e];
        r.x += sc * (g.x - g0.x); r.y += sc * (g.y - g0.y); r.z += sc * (g.z - g0.z); r.w += sc * (g.w - g0.w);
    }
    rot[e] = r;
    const float4 s = s0[e];
    float4 o;
    o.x = fminf(fmaxf(s.x + overshoot * r.x, -255.f), 255.f);
    o.y = fminf(fmaxf(s.y + overshoot * r.y, -255.f), 255.f);
    o.z = fminf(fmaxf(s.z + overshoot * r.z, -255.f), 255.f);
    o.w = s.w;                                        // alpha unchanged (deepfool.py:100-102)
    s_out[e] = o;
}

static long norm_blocks(long n) { return (n + (long)kNormBlock * kNormPerThread - 1) / ((long)kNormBlock * kNormPerThread); }

// K14a's first stage, shared by nerfail_deepfool_norms and nerfail_deepfool_step: the same kernel, grid and partials.
static void launch_norms(const float* grads, int n_rhs, long n, double* partial, hipStream_t s) {
    const dim3 grid((unsigned)norm_blocks(n)), block(kNormBlock);
#define NF_NORMS(C) deepfool_norms_kernel<C><<<grid, block, 0, s>>>((const float4*)grads, n, partial)
    switch (n_rhs) {
        case 2: NF_NORMS(2); break;
        case 3: NF_NORMS(3); break;
        case 4: NF_NORMS(4); break;
        case 5: NF_NORMS(5); break;
        case 6: NF_NORMS(6); break;
        case 7: NF_NORMS(7); break;
        default: NF_NORMS(8); break;
    }
#undef NF_NORMS
}

constexpr size_t kStepTailBytes = 64;      // {norms2[8], best, scale} behind the partials

}  // namespace nerfail

using namespace nerfail;

extern "C" size_t nerfail_deepfool_norms_scratch_bytes(int n_rhs, int64_t n) {
    if (n_rhs < 2 || n_rhs > 8 || n <= 0) return 0;
    return (size_t)norm_blocks(n) * (n_rhs - 1) * sizeof(double);
}

extern "C" int nerfail_deepfool_norms(const float* grads, int n_rhs, int64_t n, void* scratch, size_t scratch_bytes,
                                      float* norms2, void* stream) {
    NF_REQUIRE(n_rhs >= 2 && n_rhs <= 8, "n_rhs must be in 2..8");
    NF_REQUIRE(n > 0, "n must be positive");
    NF_REQUIRE(grads && scratch && norms2, "NULL pointer");
    NF_REQUIRE(scratch_bytes >= nerfail_deepfool_norms_scratch_bytes(n_rhs, n), "scratch too small (nerfail_deepfool_norms_scratch_bytes)");
    hipStream_t s = as_stream(stream);
    const long nb = norm_blocks(n);
    double* partial = (double*)scratch;
    launch_norms(grads, n_rhs, n, partial, s);
    NF_LAUNCHED("deepfool_norms_kernel");
    deepfool_norms_finish_kernel<<<dim3(1), dim3(256), 0, s>>>(partial, nb, n_rhs - 1, norms2);
    NF_LAUNCHED("deepfool_norms_finish_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_deepfool_apply(const float* grads, int n_rhs, int64_t n, const int32_t* best, const float* scale,
                                      float overshoot, const float* spatial_init, float* rot, float* spatial_out, void* stream) {
    NF_REQUIRE(n_rhs >= 2 && n_rhs <= 8, "n_rhs must be in 2..8");
    NF_REQUIRE(n > 0, "n must be positive");
    NF_REQUIRE(grads && best && scale && spatial_init && rot && spatial_out, "NULL pointer");
    deepfool_apply_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(
        (const float4*)grads, n, n_rhs, best, scale, overshoot, (const float4*)spatial_init, (float4*)rot, (float4*)spatial_out);
    NF_LAUNCHED("deepfool_apply_kernel");
    return NERFAIL_OK;
}

// ---------------------------------------------------------------------------------- DeepFool revision 1: gate and step
extern "C" int nerfail_deepfool_revision(void) { return 1; }

extern "C" size_t nerfail_deepfool_step_scratch_bytes(int n_rhs, int64_t n) {
    const size_t nb = nerfail_deepfool_norms_scratch_bytes(n_rhs, n);
    return nb ? nb + kStepTailBytes : 0;
}

extern "C" int nerfail_deepfool_gate(const float* cla, int C, int o, int target, float m1, float m2,
                                     nerfail_deepfool_record* record, void* stream) {
    NF_REQUIRE(C >= 2 && C <= NERFAIL_DEEPFOOL_MAX_COMPETITORS, "C must be in 2..8");
    NF_REQUIRE(o >= 0 && o < C, "o must be in 0..C-1");
    NF_REQUIRE(target >= -1 && target < C, "target must be -1 (untargeted) or in 0..C-1");
    NF_REQUIRE(cla && record, "NULL pointer");
    deepfool_gate_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(cla, C, o, target, m1, m2, record);
    NF_LAUNCHED("deepfool_gate_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_deepfool_step(const float* grads, int n_rhs, int64_t n, const nerfail_deepfool_record* record, void* scratch,
                                     size_t scratch_bytes, float overshoot, const float* spatial_init, float* rot, float* spatial_out,
                                     int32_t* trace_slot, void* stream) {
    NF_REQUIRE(n_rhs >= 2 && n_rhs <= 8, "n_rhs must be in 2..8");
    NF_REQUIRE(n > 0, "n must be positive");
    NF_REQUIRE(grads && record && scratch && spatial_init && rot && spatial_out && trace_slot, "NULL pointer");
    NF_REQUIRE(scratch_bytes >= nerfail_deepfool_step_scratch_bytes(n_rhs, n), "scratch too small (nerfail_deepfool_step_scratch_bytes)");
    hipStream_t s = as_stream(stream);
    const long nb = norm_blocks(n);
    double* partial = (double*)scratch;
    float* tail = (float*)((char*)scratch + nerfail_deepfool_norms_scratch_bytes(n_rhs, n));
    int* best = (int*)(tail + NERFAIL_DEEPFOOL_MAX_COMPETITORS);
    float* scale = tail + NERFAIL_DEEPFOOL_MAX_COMPETITORS + 1;
    launch_norms(grads, n_rhs, n, partial, s);
    NF_LAUNCHED("deepfool_norms_kernel");
    deepfool_choose_kernel<<<dim3(1), dim3(256), 0, s>>>(partial, nb, n_rhs - 1, record, tail, best, scale, trace_slot);
    NF_LAUNCHED("deepfool_choose_kernel");
    deepfool_apply_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(
        (const float4*)grads, n, n_rhs, best, scale, overshoot, (const float4*)spatial_init, (float4*)rot, (float4*)spatial_out);
    NF_LAUNCHED("deepfool_apply_kernel");
    return NERFAIL_OK;
}
