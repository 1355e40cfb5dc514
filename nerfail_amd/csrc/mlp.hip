// K3 + K4: fused positional encoding + NeRF MLP forward on the exact-f32 matrix cores.
// Replaces run_network (run_nerf.py:37-51), Embedder.embed (run_nerf_helpers.py:15-50) and
// NeRF.forward (run_nerf_helpers.py:100-123); ~99 % of the render path's FLOPs.
//
// Design (CDNA4 / gfx950, wave64, v_mfma_f32_32x32x2_f32 = bit-exact f32 FMA chain):
//   * Every layer is computed TRANSPOSED: H^T[out, sample] = W[out, in] * X^T[in, sample]. The MFMA
//     A operand is a 32-row slab of W, the B operand is the activation, so the 32x32 accumulator
//     tile holds "sample on the lane, output channel on the register": lane l (h = l>>5, j = l&31)
//     owns sample j and channels c(r,h) = (r&3) + 8*(r>>2) + 4*h of the tile in registers r=0..15.
//   * That is exactly the B-operand shape of the NEXT layer (B[k][j]: lane half h supplies one k per
//     step, lane j the sample), so after bias+ReLU the accumulators feed the next layer's MFMAs
//     directly. Activations never leave the register file: no LDS, no HBM, no barriers. A wave owns
//     32 samples x all W channels (128 accumulator registers in + 128 out at W = 256, which is why
//     the kernel runs one wave per SIMD with the 512-entry unified VGPR/AGPR file).
//   * The k order a layer consumes is therefore "whatever the previous accumulator layout holds";
//     the weights are re-packed ONCE (nerfail_mlp_pack, mlp_pack.hip) into that k order and into the A-fragment
//     lane order, so each weight read is one fully coalesced 16-byte-per-lane load covering 4 MFMA
//     k-steps. The 2.4 MB image stays L2-resident; all waves stream it in the same order.
//   * Positional encoding is computed per lane in registers: MFMA step s of the encoding part needs,
//     for lane half 0 / 1, sin / cos of the SAME argument x_d*2^f: one (sin, cos) pair per step, and all bands of
//     a coordinate share ONE double-precision argument reduction (SinCosBands, common.h).
//   * alpha_linear (W->1) and rgb_linear (W/2->3) are too thin for a 32-wide MFMA tile: VALU dot
//     products on the accumulator registers + one cross-half shuffle.
// Bound: f32 MFMA (157 TFLOP/s dense on MI355X); algorithmic work 1 186 816 FLOP per sample (D8 W256).
#include <stdlib.h>
#include "mlp_layout.h"

namespace nerfail {

bool mlp_x3_covers(const MlpLayout& L, int W);                                      // mlp_x3.hip
size_t mlp_x3_bytes(const MlpLayout& L, int W);
int pack_mlp_x3(const float* packed, const MlpLayout& L, int W, void* out, hipStream_t s);
int launch_mlp_x3(const MlpArgs& a, const void* img, int W, bool fold, hipStream_t s);
size_t mlp_x3f_bytes(const MlpLayout& L, int W);                                    // the folded image (no feature layer)
size_t mlp_x3f_composed_floats(const MlpLayout& L, int W);
int pack_mlp_x3f(const float* packed, const MlpLayout& L, int W, void* out, hipStream_t s);
bool mlp_x3_raybias_covers(const MlpLayout& L, int W, int spr);                     // the folded kernel's per-ray view-bias form
int launch_mlp_x3_viewbias(const float* packed, const void* img, const MlpLayout& L, int W, const float* rays, const float* viewdirs,
                           long R, float* vb, hipStream_t s);
int launch_mlp_x3_raybias(const MlpArgs& a, const void* img, int W, float* vb, hipStream_t s);

// ------------------------------------------------------------------------------------- device side
template <int NT, bool TRAIN>
__global__ __launch_bounds__(256, 1) void nerf_mlp_fwd_kernel(MlpArgs a) {
    constexpr int OTV = NT / 2;
    const int lane = threadIdx.x & 63;
    // wave id made PROVABLY wave-uniform: tile bases then live in SGPRs and every access is scalar-base + 32-bit
    // lane offset instead of a 64-bit VGPR pair per address (which spilled hundreds of registers)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5, j = lane & 31;
    const float* __restrict__ P = a.packed;
    const MlpLayout& L = a.lay;
    const long ntiles = (a.M + 31) / 32;
    const long nrounds = (ntiles + (long)gridDim.x * 4 - 1) / ((long)gridDim.x * 4);

    for (long rnd = 0; rnd < nrounds; ++rnd) {
        const long tile = (rnd * gridDim.x + blockIdx.x) * 4 + wave;
        if (tile >= ntiles) break;     // wave-uniform; waves are fully independent (no barriers)
        const long sraw = tile * 32 + j;
        const long s = sraw < a.M ? sraw : a.M - 1;

        // ---- B operands of the encoding parts, in registers
        float emb[4 * kEmbQuads], demb[4 * kDirQuads];
        encode_sample(a, s, h, emb, demb);

        f32x16 act[NT], acc[NT];
        float* __restrict__ A = nullptr;     // this tile's activation slots (training)
        if (TRAIN) {
            A = a.acts + (size_t)tile * (train_a_slots(L.D, NT) * 1024);
            store_enc<10, 4 * kEmbQuads>(A, emb, lane);              // E0 E1: 63 channels
            store_enc<4, 4 * kDirQuads>(A + 2 * 1024, demb, lane);   // V: 27 channels
        }
        // ---- layer 0: 63 -> W
        load_bias<NT>(acc, P + L.b_off[0], h);
        mfma_scalars<NT, kEmbQuads>(acc, P + L.w_off[0], lane, emb);
        relu_to<NT>(act, acc, true);
        if (TRAIN) {
            store_tiles<NT>(A + 3 * 1024, act, lane);
            store_mask<NT>(A + train_mask_slot0(L.D, NT) * 1024, 0, mask_of<NT>(act), lane);
        }

        // ---- layers 1..D-1 (pts_linears, ReLU) and D (feature_linear, no activation)
        float alpha = 0.f;
#pragma unroll 1
        for (int l = 1; l <= L.D; ++l) {
            if (l == L.D) {   // alpha_linear on the last pts activation (RH:110)
                const float* wa = P + L.alpha_off;
                float sacc = 0.f;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const f32x4* p = reinterpret_cast<const f32x4*>(wa + (t * 2 + h) * 16);
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const f32x4 wv = p[r4];
#pragma unroll
                        for (int e = 0; e < 4; ++e) sacc = fmaf(wv[e], act[t][4 * r4 + e], sacc);
                    }
                }
                sacc += __shfl_xor(sacc, 32, 64);
                alpha = sacc + wa[NT * 32];
            }
            load_bias<NT>(acc, P + L.b_off[l], h);
            const float* w = P + L.w_off[l];
            if (l == L.skip + 1 && L.skip >= 0) {   // h = cat([input_pts, h]) (RH:106-107)
                if (TRAIN) {
                    // training: the encoding was saved to `acts`; reloading it here (instead of keeping 32 registers
                    // live across the layer loop) leaves room for the double-buffered weight stream
                    float e2[4 * kEmbQuads];
                    load_enc<10, 4 * kEmbQuads>(A, e2, lane);
                    mfma_scalars<NT, kEmbQuads>(acc, w, lane, e2);
                } else {
                    mfma_scalars<NT, kEmbQuads>(acc, w, lane, emb);
                }
                w += kEmbQuads * NT * 256;
            }
            mfma_acts<NT, NT>(acc, w, lane, act);
            relu_to<NT>(act, acc, l < L.D);
            if (TRAIN) {
                store_tiles<NT>(A + (3 + l * NT) * 1024, act, lane);   // H_{l+1} for l < D, F for l == D
                if (l < L.D) store_mask<NT>(A + train_mask_slot0(L.D, NT) * 1024, l, mask_of<NT>(act), lane);
            }
        }

        // ---- views_linears[0]: cat([feature, embedded dirs]) -> W/2, ReLU (RH:112-116)
        f32x16 hv[OTV];
        load_bias<OTV>(hv, P + L.b_off[L.D + 1], h);
        mfma_acts<OTV, NT>(hv, P + L.w_off[L.D + 1], lane, act);
        if (TRAIN) {
            float d2[4 * kDirQuads];
            load_enc<4, 4 * kDirQuads>(A + 2 * 1024, d2, lane);
            mfma_scalars<OTV, kDirQuads>(hv, P + L.w_off[L.D + 1] + NT * 4 * OTV * 256, lane, d2);
        } else {
            mfma_scalars<OTV, kDirQuads>(hv, P + L.w_off[L.D + 1] + NT * 4 * OTV * 256, lane, demb);
        }
        if (TRAIN) {
            f32x16 hvr[OTV];
            relu_to<OTV>(hvr, hv, true);
            store_tiles<OTV>(A + (3 + (L.D + 1) * NT) * 1024, hvr, lane);
            store_mask<OTV>(A + train_mask_slot0(L.D, NT) * 1024, L.D, mask_of<OTV>(hvr), lane);
        }

        // ---- rgb_linear: W/2 -> 3 (RH:118)
        const float* wr = P + L.rgb_off;
        float rgb[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float sacc = 0.f;
#pragma unroll
            for (int t = 0; t < OTV; ++t) {
                const f32x4* p = reinterpret_cast<const f32x4*>(wr + ((c * OTV + t) * 2 + h) * 16);
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const f32x4 wv = p[r4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) sacc = fmaf(wv[e], fmaxf(hv[t][4 * r4 + e], 0.f), sacc);
                }
            }
            sacc += __shfl_xor(sacc, 32, 64);
            rgb[c] = sacc + wr[3 * OTV * 32 + c];
        }
        if (h == 0 && sraw < a.M)
            reinterpret_cast<float4*>(a.raw)[sraw] = make_float4(rgb[0], rgb[1], rgb[2], alpha);
    }
}

// Inference goes to the LDS-streaming kernel (mlp_lds.hip) when it covers the shape (even depth <= 8); the training
// forward (activations saved) and the other shapes run the register-streamed kernel below. nerfail_mlp_fwd_select /
// NERFAIL_FWD_KERNEL=reg|lds force one of them (A/B timing, parity test of one against the other).
// The x3 entry points (nerfail_mlp_fwd_x3 and kin) run the bf16x3 kernel (mlp_x3.hip) under the automatic selection when it
// covers the shape; NERFAIL_FWD_KERNEL=x forces it there, =reg / =lds force the exact-f32 kernels everywhere.
static int g_fwd_select = [] {
    const char* e = getenv("NERFAIL_FWD_KERNEL");
    return e ? (e[0] == 'r' ? 1 : (e[0] == 'l' ? 2 : (e[0] == 'x' ? 3 : 0))) : 0;
}();
static bool use_lds_kernel(const MlpArgs& a) {
    if (g_fwd_select == 1) return false;
    if (g_fwd_select == 2) return true;
    return !(a.lay.D & 1) && a.lay.D <= 8;
}

static int launch_mlp(const MlpArgs& a, int W, hipStream_t s) {
    if (use_lds_kernel(a)) return launch_mlp_lds(a, W, s);
    const dim3 grid(mlp_grid_blocks((a.M + 31) / 32)), block(256);      // persistent: one 4-wave workgroup per CU
    const bool train = a.acts != nullptr;
    switch (W) {
        case 256: if (train) nerf_mlp_fwd_kernel<8, true><<<grid, block, 0, s>>>(a); else nerf_mlp_fwd_kernel<8, false><<<grid, block, 0, s>>>(a); break;
        case 128: if (train) nerf_mlp_fwd_kernel<4, true><<<grid, block, 0, s>>>(a); else nerf_mlp_fwd_kernel<4, false><<<grid, block, 0, s>>>(a); break;
        case 64: if (train) nerf_mlp_fwd_kernel<2, true><<<grid, block, 0, s>>>(a); else nerf_mlp_fwd_kernel<2, false><<<grid, block, 0, s>>>(a); break;
        default: set_error("nerfail_mlp_fwd: unsupported W"); return NERFAIL_EINVAL;
    }
    NF_LAUNCHED("nerf_mlp_fwd_kernel");
    return NERFAIL_OK;
}

// x3 entry points: the bf16x3 kernel for inference when the selection allows it and it covers the shape, else exactly
// launch_mlp. Forced ('x') on a shape it does not cover, or without an image, is an error. fold: the x3f entry points - `img`
// is the folded image and the folded kernel runs; every rule is the same.
static int launch_mlp_x3_or(const char* fn, const MlpArgs& a, const void* img, int W, bool fold, hipStream_t s) {
    if (a.acts == nullptr && (g_fwd_select == 0 || g_fwd_select == 3)) {
        if (g_fwd_select == 3 || (img != nullptr && mlp_x3_covers(a.lay, W))) {
            if (img == nullptr) { set_error("%s: NERFAIL_FWD_KERNEL=x without a bf16x3 image", fn); return NERFAIL_EINVAL; }
            return launch_mlp_x3(a, img, W, fold, s);
        }
    }
    return launch_mlp(a, W, s);
}

// The per-ray view-bias form of the folded kernel (mlp_x3.hip) serves an inference call on the folded image whose samples per
// ray are a multiple of 32, under the selection rules of the x3 entry points (not with reg / lds forced).
// nerfail_mlp_x3_raybias_select / NERFAIL_X3_RAYBIAS=0 switch it off: the plain folded kernel then runs (A/B timing, tests).
static int g_x3_raybias = [] {
    const char* e = getenv("NERFAIL_X3_RAYBIAS");
    return e && e[0] == '0' ? 0 : 1;
}();
static bool x3_raybias_runs(const MlpLayout& L, int W, int spr) {
    return g_x3_raybias && (g_fwd_select == 0 || g_fwd_select == 3) && mlp_x3_raybias_covers(L, W, spr);
}

}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_mlp_x3_raybias_select(int on) {
    const int prev = g_x3_raybias;
    if (on == 0 || on == 1) g_x3_raybias = on;
    return prev;
}

extern "C" int nerfail_mlp_fwd_select(int which) {
    const int prev = g_fwd_select;
    if (which >= 0 && which <= 3) g_fwd_select = which;
    return prev;
}

// The forward entry points differ in the form of their input only: sample points + one view direction per ray (pts), an
// already embedded batch (xemb), or packed rays + depths (rays: the points are formed inside the kernel, pts = o + d * z,
// RN:381 / :399, instead of being read from a [M,3] tensor that the sampling kernels wrote). `in0` / `in1` are the two input
// pointers of that form (xemb has one), `acts` asks for the training forward, `sel` for the bf16x3 selection with image `x3` (kX3Fold: the folded image).
enum MlpInput { kInPts, kInEmbedded, kInRays };
enum MlpSel { kF32, kX3, kX3Fold, kX3Ray };   // kX3Ray: the folded kernel's per-ray view-bias form, `vb` its per-call buffer
#define MLP_REQUIRE(cond, msg) do { if (!(cond)) { set_error("%s: %s", fn, msg); return NERFAIL_EINVAL; } } while (0)
static int mlp_fwd_entry(const char* fn, MlpInput form, const float* packed, MlpSel sel, const void* x3, int D, int W, int skip,
                         const float* in0, const float* in1, int64_t M, int spr, float* raw, float* acts, bool need_acts, void* stream,
                         float* vb = nullptr) {
    MLP_REQUIRE(M >= 0, form == kInRays ? "n_rays is negative" : "M is negative");
    MLP_REQUIRE(form == kInEmbedded || spr >= 1, "samples_per_ray must be positive");
    MlpArgs a;
    MLP_REQUIRE(make_layout(D, W, skip, a.lay), "unsupported (D, W)");
    if (form == kInRays) M *= spr;
    if (M == 0) return NERFAIL_OK;
    MLP_REQUIRE(packed != nullptr && in0 != nullptr && (form == kInEmbedded || in1 != nullptr) && raw != nullptr &&
                (!need_acts || acts != nullptr), "NULL pointer");
    a.packed = packed; a.raw = raw; a.acts = acts; a.M = M; a.spr = form == kInEmbedded ? 1 : spr;
    a.pts = form == kInPts ? in0 : nullptr; a.viewdirs = form == kInPts ? in1 : nullptr;
    a.xemb = form == kInEmbedded ? in0 : nullptr;
    a.rays = form == kInRays ? in0 : nullptr; a.z = form == kInRays ? in1 : nullptr;
    if (sel == kX3Ray) {
        MLP_REQUIRE(x3 != nullptr && vb != nullptr, "NULL pointer");
        MLP_REQUIRE(x3_raybias_runs(a.lay, W, a.spr), "the per-ray view-bias form does not serve this call (nerfail_mlp_x3f_raybias_floats returns 0)");
        return launch_mlp_x3_raybias(a, x3, W, vb, as_stream(stream));
    }
    return sel != kF32 ? launch_mlp_x3_or(fn, a, x3, W, sel == kX3Fold, as_stream(stream)) : launch_mlp(a, W, as_stream(stream));
}
#undef MLP_REQUIRE

extern "C" int nerfail_mlp_fwd(const float* packed, int D, int W, int skip, const float* pts, const float* viewdirs,
                               int64_t M, int samples_per_ray, float* raw, void* stream) {
    return mlp_fwd_entry(__func__, kInPts, packed, kF32, nullptr, D, W, skip, pts, viewdirs, M, samples_per_ray, raw, nullptr, false, stream);
}

extern "C" int nerfail_mlp_fwd_embedded(const float* packed, int D, int W, int skip, const float* x, int64_t M, float* raw,
                                        void* stream) {
    return mlp_fwd_entry(__func__, kInEmbedded, packed, kF32, nullptr, D, W, skip, x, nullptr, M, 1, raw, nullptr, false, stream);
}

extern "C" size_t nerfail_mlp_train_acts_floats(int D, int W, int64_t M) {
    MlpLayout L;
    if (!make_layout(D, W, -1, L) || M < 0) return 0;
    return (size_t)((M + 31) / 32) * make_train_layout(D, W).a_slots * 1024;   // activation tiles + ReLU bit masks
}

extern "C" int nerfail_mlp_fwd_train(const float* packed, int D, int W, int skip, const float* pts, const float* viewdirs,
                                     int64_t M, int samples_per_ray, float* raw, float* acts, void* stream) {
    return mlp_fwd_entry(__func__, kInPts, packed, kF32, nullptr, D, W, skip, pts, viewdirs, M, samples_per_ray, raw, acts, true, stream);
}

extern "C" int nerfail_mlp_fwd_rays(const float* packed, int D, int W, int skip, const float* rays, const float* z_vals,
                                    int64_t n_rays, int samples_per_ray, float* raw, float* acts, void* stream) {
    return mlp_fwd_entry(__func__, kInRays, packed, kF32, nullptr, D, W, skip, rays, z_vals, n_rays, samples_per_ray, raw, acts, false, stream);
}

// ---- bf16x3 inference (mlp_x3.hip): the weight stream split once into three bf16 planes; each entry point takes both images
extern "C" size_t nerfail_mlp_packed_x3_bytes(int D, int W, int skip) {
    MlpLayout L;
    return make_layout(D, W, skip, L) ? mlp_x3_bytes(L, W) : 0;
}

extern "C" int nerfail_mlp_pack_x3(const float* packed, int D, int W, int skip, void* out, void* stream) {
    MlpLayout L;
    NF_REQUIRE(make_layout(D, W, skip, L), "unsupported (D, W)");
    NF_REQUIRE(packed != nullptr && out != nullptr, "NULL pointer");
    return pack_mlp_x3(packed, L, W, out, as_stream(stream));
}

extern "C" int nerfail_mlp_fwd_x3(const float* packed, const void* x3, int D, int W, int skip, const float* pts,
                                  const float* viewdirs, int64_t M, int samples_per_ray, float* raw, void* stream) {
    return mlp_fwd_entry(__func__, kInPts, packed, kX3, x3, D, W, skip, pts, viewdirs, M, samples_per_ray, raw, nullptr, false, stream);
}

extern "C" int nerfail_mlp_fwd_embedded_x3(const float* packed, const void* x3, int D, int W, int skip, const float* x, int64_t M,
                                           float* raw, void* stream) {
    return mlp_fwd_entry(__func__, kInEmbedded, packed, kX3, x3, D, W, skip, x, nullptr, M, 1, raw, nullptr, false, stream);
}

extern "C" int nerfail_mlp_fwd_rays_x3(const float* packed, const void* x3, int D, int W, int skip, const float* rays,
                                       const float* z_vals, int64_t n_rays, int samples_per_ray, float* raw, float* acts, void* stream) {
    return mlp_fwd_entry(__func__, kInRays, packed, kX3, x3, D, W, skip, rays, z_vals, n_rays, samples_per_ray, raw, acts, false, stream);
}

// ---- bf16x3 inference without feature_linear: its weights composed into the views layer at pack time (mlp_x3.hip)
extern "C" size_t nerfail_mlp_packed_x3f_bytes(int D, int W, int skip) {
    MlpLayout L;
    return make_layout(D, W, skip, L) ? mlp_x3f_bytes(L, W) : 0;
}

extern "C" size_t nerfail_mlp_x3f_composed_floats(int D, int W, int skip) {
    MlpLayout L;
    return make_layout(D, W, skip, L) ? mlp_x3f_composed_floats(L, W) : 0;
}

extern "C" int nerfail_mlp_pack_x3f(const float* packed, int D, int W, int skip, void* out, void* stream) {
    MlpLayout L;
    NF_REQUIRE(make_layout(D, W, skip, L), "unsupported (D, W)");
    NF_REQUIRE(packed != nullptr && out != nullptr, "NULL pointer");
    return pack_mlp_x3f(packed, L, W, out, as_stream(stream));
}

extern "C" int nerfail_mlp_fwd_x3f(const float* packed, const void* x3f, int D, int W, int skip, const float* pts,
                                   const float* viewdirs, int64_t M, int samples_per_ray, float* raw, void* stream) {
    return mlp_fwd_entry(__func__, kInPts, packed, kX3Fold, x3f, D, W, skip, pts, viewdirs, M, samples_per_ray, raw, nullptr, false, stream);
}

extern "C" int nerfail_mlp_fwd_embedded_x3f(const float* packed, const void* x3f, int D, int W, int skip, const float* x, int64_t M,
                                            float* raw, void* stream) {
    return mlp_fwd_entry(__func__, kInEmbedded, packed, kX3Fold, x3f, D, W, skip, x, nullptr, M, 1, raw, nullptr, false, stream);
}

extern "C" int nerfail_mlp_fwd_rays_x3f(const float* packed, const void* x3f, int D, int W, int skip, const float* rays,
                                        const float* z_vals, int64_t n_rays, int samples_per_ray, float* raw, float* acts, void* stream) {
    return mlp_fwd_entry(__func__, kInRays, packed, kX3Fold, x3f, D, W, skip, rays, z_vals, n_rays, samples_per_ray, raw, acts, false, stream);
}

// ---- the folded kernel with the view-direction term computed once per ray (mlp_x3.hip: x3_viewbias_kernel, RAYBIAS)
extern "C" size_t nerfail_mlp_x3f_raybias_floats(int D, int W, int skip, int64_t n_rays, int samples_per_ray) {
    MlpLayout L;
    if (n_rays <= 0 || !make_layout(D, W, skip, L) || !x3_raybias_runs(L, W, samples_per_ray)) return 0;
    return (size_t)n_rays * (size_t)(W / 2);
}

extern "C" int nerfail_mlp_x3f_viewbias(const float* packed, const void* x3f, int D, int W, int skip, const float* rays,
                                        const float* viewdirs, int64_t n_rays, float* vb, void* stream) {
    MlpLayout L;
    NF_REQUIRE(make_layout(D, W, skip, L), "unsupported (D, W)");
    NF_REQUIRE(n_rays >= 0, "n_rays is negative");
    if (n_rays == 0) return NERFAIL_OK;
    NF_REQUIRE(packed != nullptr && x3f != nullptr && vb != nullptr && ((rays != nullptr) != (viewdirs != nullptr)),
               "NULL pointer, or both of rays and viewdirs given");
    return launch_mlp_x3_viewbias(packed, x3f, L, W, rays, viewdirs, n_rays, vb, as_stream(stream));
}

extern "C" int nerfail_mlp_fwd_x3f_raybias(const float* packed, const void* x3f, int D, int W, int skip, const float* pts,
                                           const float* viewdirs, int64_t M, int samples_per_ray, float* raw, float* vb, void* stream) {
    return mlp_fwd_entry(__func__, kInPts, packed, kX3Ray, x3f, D, W, skip, pts, viewdirs, M, samples_per_ray, raw, nullptr, false, stream, vb);
}

extern "C" int nerfail_mlp_fwd_rays_x3f_raybias(const float* packed, const void* x3f, int D, int W, int skip, const float* rays,
                                                const float* z_vals, int64_t n_rays, int samples_per_ray, float* raw, float* vb,
                                                void* stream) {
    return mlp_fwd_entry(__func__, kInRays, packed, kX3Ray, x3f, D, W, skip, rays, z_vals, n_rays, samples_per_ray, raw, nullptr, false, stream, vb);
}
