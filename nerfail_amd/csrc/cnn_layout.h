// The shapes and the two flat layouts of the MyCNN classifier (model/MyModel.py:5-52), shared by cnn.hip (pack, forward, the
// backward passes) and cls_train.hip (the optimizer step that keeps the weight image in step with the parameters): the packed
// MFMA weight image of nerfail_cnn_pack and the nn.Module-order gradient buffer of nerfail_cnn_bwd_weights. Host code only,
// apart from the constexpr shape helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>

namespace nerfail {
namespace cnn {

constexpr int kStages = 7;
constexpr int kHidden = 512;
constexpr int kFlat = 1024;
__host__ __device__ constexpr int stage_cin(int s) { return s == 0 ? 3 : (s == 1 ? 32 : (s == 2 ? 64 : (s == 3 ? 128 : (s == 6 ? 128 : 256)))); }
__host__ __device__ constexpr int stage_cout(int s) { return s == 0 ? 32 : (s == 1 ? 64 : (s == 2 ? 128 : (s == 5 ? 128 : (s == 6 ? 64 : 256)))); }

// The one per-stage table: f(std::integral_constant<int, s>) with the run-time stage index s = 0..6 as a compile-time value, so
// that a launch takes its channel counts from stage_cin(S) / stage_cout(S). Labels: NF_STAGE_LABELS("x")[s] = "x_s<s + 1>".
template <class F>
static inline int dispatch_stage(int s, F&& f) {
    switch (s) {
        case 0: return f(std::integral_constant<int, 0>());
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        default: return f(std::integral_constant<int, 6>());
    }
}
#define NF_STAGE_LABELS(p) {p "_s1", p "_s2", p "_s3", p "_s4", p "_s5", p "_s6", p "_s7"}

// ---------------------------------------------------------------------------------------------------------------- host layout
struct Dims {
    int hin[kStages + 1], win[kStages + 1];      // hin[s]: stage s input height; hin[s + 1] = its pooled output height
};

static bool dims_of(int H, int W, Dims& d) {
    if (H < 4 || W < 4 || H > 8192 || W > 8192) return false;
    d.hin[0] = H;
    d.win[0] = W;
    for (int s = 0; s < kStages; ++s) {
        if (d.hin[s] < 4 || d.win[s] < 4) return false;
        d.hin[s + 1] = (d.hin[s] - 2) / 2;
        d.win[s + 1] = (d.win[s] - 2) / 2;
    }
    return d.hin[kStages] == 4 && d.win[kStages] == 4;          // fc1 takes 4 x 4 x 64 = 1024 inputs
}

static inline size_t up4(size_t n) { return (n + 3) & ~size_t(3); }
__host__ __device__ inline int npc8(int wp) { return (wp + 7) / 8; }

// packed weight image (floats), every region 16-byte aligned
struct PackLayout {
    size_t fwd[kStages], bias[kStages], bwd[kStages], w1raw, fc1T, fc1P, b1, w2, b2, total;
};
__host__ __device__ constexpr int fwd_taps(int s) { return s == 0 ? 10 : 9; }     // stage 1: a zero 10th tap pads K to 40
__host__ __device__ constexpr int fwd_kc(int s) { return s == 0 ? 4 : stage_cin(s); }

static PackLayout pack_layout(int C) {
    PackLayout L;
    size_t o = 0;
    for (int s = 0; s < kStages; ++s) {
        L.fwd[s] = o;  o += up4((size_t)stage_cout(s) * fwd_taps(s) * fwd_kc(s));
        L.bias[s] = o; o += up4(stage_cout(s));
        L.bwd[s] = o;  o += s == 0 ? 0 : up4((size_t)stage_cin(s) * 9 * stage_cout(s));
    }
    L.w1raw = o; o += up4(32 * 3 * 9);
    L.fc1T = o; o += (size_t)kFlat * kHidden;
    L.fc1P = o; o += (size_t)kFlat * kHidden;
    L.b1 = o; o += kHidden;
    L.w2 = o; o += up4((size_t)C * kHidden);
    L.b2 = o; o += up4(C);
    L.total = o;
    return L;
}

static inline size_t act_floats(const Dims& d, int s, int B) { return (size_t)B * d.hin[s + 1] * d.win[s + 1] * stage_cout(s); }
static inline size_t mask_bytes_of(const Dims& d, int s, int B) { return (size_t)B * d.hin[s + 1] * npc8(d.win[s + 1]) * 2 * stage_cout(s); }

// ---- the bf16x3 weight image of nerfail_cnn_pack_x3 (bytes; cnn_x3.hip reads it, tests/cnn_x3_ref.py restates it).
// Stages 2..7 (s = 1..6), per stage the forward image and then the backward image, each made from the f32 image of the same
// stage and direction, which is [NC][9 taps][KC] (forward: NC = Cout, KC = Cin; backward: NC = Cin, KC = Cout, taps not flipped):
//     [KC / 16 slices][NC rows][9 taps][3 planes][16 channels] bf16
// plane 0, 1, 2 = the three pieces of the split (bf16_split.h), largest first; element (cb, n, t, p, c) is piece p of the f32
// image's (n, t, 16 cb + c). The 864 bytes (kX3RowSlots 16-byte slots) of one (slice, row) are what a lane's nine k16 steps read
// with three ds_read_b128 each (lane half h: channels 8h .. 8h + 7 of a plane), and the rows of an n-block are contiguous.
// The image does not depend on num_classes.
constexpr int kX3RowSlots = 9 * 3 * 2;
struct X3Layout {
    size_t fwd[kStages], bwd[kStages], total;                   // [0] unused: stage 1 stays exact f32
};
static inline X3Layout x3_layout() {
    X3Layout X;
    size_t o = 0;
    X.fwd[0] = X.bwd[0] = 0;
    for (int s = 1; s < kStages; ++s) {
        const size_t n = (size_t)stage_cout(s) * stage_cin(s) * 9 * 3 * 2;
        X.fwd[s] = o; o += n;
        X.bwd[s] = o; o += n;
    }
    X.total = o;
    return X;
}

// ---- one conv stage launch: the arguments of conv_stage_kernel (cnn.hip) and conv_x3_kernel (cnn_x3.hip)
struct ConvArgs {
    const float* in;           // forward: stage input (NHWC, or NCHW for MODE 1)
    const float* w;            // weight image of this stage and direction (exact kernels)
    const float* bias;         // forward
    float* out;                // forward: pooled NHWC; backward: d input NHWC
    unsigned char* mask;       // forward: argmax codes (NULL = inference)
    const float* gp;           // backward: d pooled output (NHWC)
    const float* act;          // backward: pooled output (NHWC)
    const unsigned char* gmask;// backward: argmax codes of the forward
    int hin, win, hp, wp;      // stage input and pooled output sizes
    int B;                     // backward: images of the forward (grid z = r * B + b covers the R right-hand sides)
};
// stages 2..7 (s = 1..6) on the bf16x3 image `x3` (cnn_x3.hip); Z: grid slices (B, or R * B)
int conv_fwd_stage_x3(int s, const ConvArgs& a, const void* x3, int B, hipStream_t st);
int conv_bwd_stage_x3(int s, const ConvArgs& a, const void* x3, int Z, hipStream_t st);

// ---- d_params of nerfail_cnn_bwd_weights; also the flat parameter and momentum buffers of nerfail_cnn_sgd_step
struct GradLayout {                                             // d_params (floats): nn.Module layout, state-dict order
    size_t w[kStages + 2], b[kStages + 2], total;               // 7, 8: fc1, fc2
};
static GradLayout grad_layout(int C) {
    GradLayout L;
    size_t o = 0;
    for (int s = 0; s < kStages; ++s) {
        L.w[s] = o; o += up4((size_t)stage_cout(s) * stage_cin(s) * 9);
        L.b[s] = o; o += up4(stage_cout(s));
    }
    L.w[7] = o; o += (size_t)kHidden * kFlat;
    L.b[7] = o; o += kHidden;
    L.w[8] = o; o += up4((size_t)C * kHidden);
    L.b[8] = o; o += up4(C);
    L.total = o;
    return L;
}

}  // namespace cnn
}  // namespace nerfail
