// The shapes and the two flat layouts of the MyCNN classifier (model/MyModel.py:5-52), shared by cnn.hip (pack, forward, the
// backward passes) and cls_train.hip (the optimizer step that keeps the weight image in step with the parameters): the packed
// MFMA weight image of nerfail_cnn_pack and the nn.Module-order gradient buffer of nerfail_cnn_bwd_weights. Host code only,
// apart from the constexpr shape helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace nerfail {
namespace cnn {

constexpr int kStages = 7;
constexpr int kHidden = 512;
constexpr int kFlat = 1024;
__host__ __device__ constexpr int stage_cin(int s) { return s == 0 ? 3 : (s == 1 ? 32 : (s == 2 ? 64 : (s == 3 ? 128 : (s == 6 ? 128 : 256)))); }
__host__ __device__ constexpr int stage_cout(int s) { return s == 0 ? 32 : (s == 1 ? 64 : (s == 2 ? 128 : (s == 5 ? 128 : (s == 6 ? 64 : 256)))); }

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
