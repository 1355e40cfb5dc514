// Victim training (model_train.py:107-193 = MTR, MyDataset.py:93-105 = MD) on the device: the batch a DataLoader would stack,
// gathered from a resident uint8 store by indices that never leave the GPU; the cross entropy of nn.CrossEntropyLoss() with
// per-row labels, its gradient and the running statistics of a phase; torch.optim.SGD's momentum step fused with the update of
// MyCNN's MFMA weight image; and the epoch close with the best-weights rule. The reference's loop takes two .item() host
// reads per batch, stacks 16 float images per batch on the host side and re-homes 18 tensors per step; here a step is five
// launch chains without a host read, and an epoch has one.
//
// Reproducibility: no atomics anywhere. Every output element is written by one lane; the only sum (the per-view CE of a batch)
// is formed by one lane in view order. Two runs give the same bits.
#include "common.h"
#include "cnn_layout.h"

namespace nerfail {

constexpr int kClsBlocksPerView = 128;       // 16 views x 128 = 2048 workgroups: the grid cap of a streaming kernel

// ---- MD:93-105 for B views chosen by idx. grid = (workgroups per view, B). A view of the store starts at byte ch * P * i: for
// U8C4 that is 4-byte aligned, for U8C3 not even that when P is odd. Each view is therefore cut into a scalar head (pixels up
// to the first wide-load boundary), a body of whole 4-pixel groups (one lane: 16 B of U8C4 as one 128-bit load, or the three
// dwords that hold four U8C3 pixels) and a scalar tail; consecutive lanes take consecutive groups, so a wave reads 1 KB / 768 B
// in a row. Head and tail are read pixel by pixel (dword / bytes). Nothing outside the view's own ch * P bytes is read.
// x is planar: x[b][c][p]; a lane writes four consecutive floats per channel (128-bit when that address allows).
__device__ __forceinline__ void store4(float* __restrict__ d, float a, float b, float c, float e) {
    if ((reinterpret_cast<uintptr_t>(d) & 15) == 0) {
        *reinterpret_cast<float4*>(d) = make_float4(a, b, c, e);
    } else {
        d[0] = a; d[1] = b; d[2] = c; d[3] = e;
    }
}

template <int F>
__global__ __launch_bounds__(256) void cls_batch_kernel(const unsigned char* __restrict__ images, const int* __restrict__ labels_all,
                                                        const long long* __restrict__ idx, long N, long P, float* __restrict__ x,
                                                        int* __restrict__ labels) {
    constexpr int CH = (F == NERFAIL_EVAL_U8C4) ? 4 : 3;
    const int b = blockIdx.y;
    const long long i = idx[b];
    const bool bad = (i < 0 || i >= (long long)N);
    float* xb = x + (long)b * 3 * P;
    if (blockIdx.x == 0 && threadIdx.x == 0) labels[b] = bad ? -1 : labels_all[i];
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    if (bad) {                                                             // a view of NaN; the store is not touched
        for (long e = t; e < 3 * P; e += stride) xb[e] = NAN;
        return;
    }
    const unsigned char* v = images + (long)i * CH * P;
    const uintptr_t a = reinterpret_cast<uintptr_t>(v);
    long head = (CH == 4) ? (long)(((16 - (a & 15)) & 15) >> 2) : (long)(a & 3);    // U8C3: (a + 3 h) % 4 == 0 <=> h == a mod 4
    head = head < P ? head : P;
    const long nq = (P - head) >> 2, tail = (P - head) & 3;
    for (long q = t; q < nq; q += stride) {
        const long p = head + 4 * q;
        float c0[4], c1[4], c2[4];
        if (CH == 4) {
            const uint4 w = *reinterpret_cast<const uint4*>(v + 4 * p);
            const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c0[j] = white_u8(ww[j], 0);
                c1[j] = white_u8(ww[j], 8);
                c2[j] = white_u8(ww[j], 16);
            }
        } else {
            const unsigned* w = reinterpret_cast<const unsigned*>(v + 3 * p);       // 12 bytes = pixels p .. p + 3
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
            c0[0] = (float)(w0 & 255u);         c1[0] = (float)((w0 >> 8) & 255u);  c2[0] = (float)((w0 >> 16) & 255u);
            c0[1] = (float)(w0 >> 24);          c1[1] = (float)(w1 & 255u);         c2[1] = (float)((w1 >> 8) & 255u);
            c0[2] = (float)((w1 >> 16) & 255u); c1[2] = (float)(w1 >> 24);          c2[2] = (float)(w2 & 255u);
            c0[3] = (float)((w2 >> 8) & 255u);  c1[3] = (float)((w2 >> 16) & 255u); c2[3] = (float)(w2 >> 24);
        }
        store4(xb + p, c0[0], c0[1], c0[2], c0[3]);
        store4(xb + P + p, c1[0], c1[1], c1[2], c1[3]);
        store4(xb + 2 * P + p, c2[0], c2[1], c2[2], c2[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < head + tail) {                    // at most 3 + 3 pixels
        const long p = threadIdx.x < head ? (long)threadIdx.x : head + 4 * nq + ((long)threadIdx.x - head);
        float c0, c1, c2;
        if (CH == 4) {
            const unsigned w = *reinterpret_cast<const unsigned*>(v + 4 * p);
            c0 = white_u8(w, 0);
            c1 = white_u8(w, 8);
            c2 = white_u8(w, 16);
        } else {
            c0 = (float)v[3 * p];
            c1 = (float)v[3 * p + 1];
            c2 = (float)v[3 * p + 2];
        }
        xb[p] = c0;
        xb[P + p] = c1;
        xb[2 * P + p] = c2;
    }
}

// ---- MTR:89, 150-169: one wave. Lane l takes views base + l of every block of 64 views: CE and argmax from logit_row_stats
// (the definition nerfail_attack_logit_stats and nerfail_eval_logit_stats share), the gradient of the MEAN cross entropy
// (softmax - onehot) / B evaluated in double and rounded once. Lane 0 then adds the block's CEs in view order.
__global__ __launch_bounds__(64) void cls_ce_kernel(const float* __restrict__ logits, const int* __restrict__ labels, int B, int C,
                                                    float* __restrict__ d_logits, float* __restrict__ row) {
    const int lane = threadIdx.x;
    double sum = pair_get(row + 0);
    float correct = 0.f;
    for (int base = 0; base < B; base += 64) {
        const int b = base + lane;
        double ce = 0.0;
        float ok = 0.f;
        if (b < B) {
            const int label = labels[b];
            const bool has_label = label >= 0 && label < C;
            const float* x = logits + (long)b * C;
            const LogitRow r = logit_row_stats(x, C, has_label ? label : 0);
            ce = has_label ? r.ce : (double)NAN;
            ok = (has_label && r.arg == label) ? 1.f : 0.f;
            if (d_logits != nullptr) {
                for (int c = 0; c < C; ++c) {
                    const double p = exp((double)x[c] - (double)r.m) / r.s;
                    const double d = (p - (c == label ? 1.0 : 0.0)) / (double)B;
                    d_logits[(long)b * C + c] = has_label ? (float)d : NAN;
                }
            }
        }
        const int nb = B - base < 64 ? B - base : 64;
        for (int j = 0; j < nb; ++j) sum += __shfl(ce, j, 64);             // every lane forms the same sum, in view order
        correct += wave_sum(ok);                                            // small integers: exact in any order
    }
    if (lane == 0) {
        pair_put(row + 0, sum);
        row[2] += correct;
        row[3] += (float)B;
    }
}

// ---- MTR:90, 165: torch.optim.SGD(lr, momentum) - dampening 0, no weight decay, no Nesterov - over the flat buffers in the
// nerfail_cnn_grad_floats layout, and the weight image kept in step: one thread per float of the layout updates its parameter
// and writes the new value to the one to three places of the image nerfail_cnn_pack would copy it to. The alignment floats of
// the layout and of the image are neither read nor written.
struct SgdArgs {
    cnn::GradLayout G;
    cnn::PackLayout L;
    int C, first;
    float lr, mu;
};

__global__ __launch_bounds__(256) void cnn_sgd_step_kernel(SgdArgs a, float* __restrict__ params, const float* __restrict__ grads,
                                                           float* __restrict__ mom, float* __restrict__ packed) {
    using namespace cnn;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.G.total) return;
    int layer = 0;                                                         // 0..6 conv stages, 7 fc1, 8 fc2
#pragma unroll
    for (int s = 1; s < kStages + 2; ++s) layer += (i >= a.G.w[s]) ? 1 : 0;
    const bool is_bias = i >= a.G.b[layer];
    const size_t j = i - (is_bias ? a.G.b[layer] : a.G.w[layer]);
    const int cout = layer < kStages ? stage_cout(layer) : (layer == 7 ? kHidden : a.C);
    const int fan = layer < kStages ? stage_cin(layer) * 9 : (layer == 7 ? kFlat : kHidden);
    if (j >= (is_bias ? (size_t)cout : (size_t)cout * fan)) return;      // the floats that round a region up to 4
    const float g = grads[i];
    const float buf = a.first ? g : __fadd_rn(__fmul_rn(a.mu, mom[i]), g);  // two roundings, as torch's mul_ then add_
    const float p = __fmaf_rn(-a.lr, buf, params[i]);                       // add_(buf, alpha = -lr): one rounding
    mom[i] = buf;
    params[i] = p;
    if (is_bias) {
        const size_t o = layer < kStages ? a.L.bias[layer] : (layer == 7 ? a.L.b1 : a.L.b2);
        packed[o + j] = p;
    } else if (layer < kStages) {
        const int ci = stage_cin(layer);
        const int t = (int)(j % 9), c = (int)((j / 9) % ci), o = (int)(j / ((size_t)9 * ci));
        packed[a.L.fwd[layer] + ((size_t)o * fwd_taps(layer) + t) * fwd_kc(layer) + c] = p;
        if (layer > 0) packed[a.L.bwd[layer] + ((size_t)c * 9 + t) * cout + o] = p;
        else packed[a.L.w1raw + j] = p;
    } else if (layer == 7) {
        const int o = (int)(j / kFlat), col = (int)(j % kFlat);            // col = c * 16 + yx (NCHW) -> n = yx * 64 + c (NHWC)
        const int n = (col & 15) * 64 + (col >> 4);
        packed[a.L.fc1P + (size_t)o * kFlat + n] = p;
        packed[a.L.fc1T + (size_t)n * kHidden + o] = p;
    } else {
        packed[a.L.w2 + j] = p;
    }
}

// ---- MTR:170-186
__global__ __launch_bounds__(64) void cls_epoch_close_kernel(const float* __restrict__ train_row, const float* __restrict__ val_row,
                                                             double n_train, double n_val, float* __restrict__ best, int epoch,
                                                             float* __restrict__ record, int* __restrict__ flag) {
    if (threadIdx.x != 0) return;
    const float train_loss = (float)(pair_get(train_row) / n_train), val_loss = (float)(pair_get(val_row) / n_val);
    const float train_acc = (float)((double)train_row[2] / n_train), val_acc = (float)((double)val_row[2] / n_val);
    const float best_acc = best[0], best_epoch = best[1];
    const bool take = val_acc > best_acc;                                  // strict: a tie keeps the earlier epoch; false for NaN
    if (take) {
        best[0] = val_acc;
        best[1] = (float)epoch;
    }
    flag[0] = take ? 1 : 0;
    record[0] = train_loss;
    record[1] = train_acc;
    record[2] = val_loss;
    record[3] = val_acc;
    record[4] = take ? 1.f : 0.f;
    record[5] = take ? (float)epoch : best_epoch;
    record[6] = take ? val_acc : best_acc;
    record[7] = (float)epoch;
    record[8] = train_row[2];
    record[9] = train_row[3];
    record[10] = val_row[2];
    record[11] = val_row[3];
    record[12] = record[13] = record[14] = record[15] = 0.f;
}

static bool aligned_to(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) == 0; }

}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_cls_revision(void) { return 1; }

extern "C" int nerfail_cls_batch(const void* images, int format, const int32_t* labels_all, int64_t N, int64_t P, const int64_t* idx,
                                 int B, float* x, int32_t* labels, void* stream) {
    NF_REQUIRE(format == NERFAIL_EVAL_U8C4 || format == NERFAIL_EVAL_U8C3, "format must be NERFAIL_EVAL_U8C4 or NERFAIL_EVAL_U8C3");
    NF_REQUIRE(N >= 0 && P >= 0 && B >= 0, "negative size");
    NF_REQUIRE(B <= 65535, "B must be at most 65535");
    NF_REQUIRE(N <= ((int64_t)1 << 31) && P <= ((int64_t)1 << 31), "N and P must be at most 2^31");
    if (B == 0) return NERFAIL_OK;
    NF_REQUIRE(idx != nullptr && labels != nullptr && (x != nullptr || P == 0), "NULL pointer");
    NF_REQUIRE(N == 0 || P == 0 || (images != nullptr && labels_all != nullptr), "NULL store");
    NF_REQUIRE(aligned_to(images, format == NERFAIL_EVAL_U8C4 ? 15 : 3), "the store must be 16-byte (U8C4) or 4-byte (U8C3) aligned");
    NF_REQUIRE(aligned_to(x, 3) && aligned_to(labels, 3) && aligned_to(labels_all, 3) && aligned_to(idx, 7),
               "x, labels and labels_all must be 4-byte, idx 8-byte aligned");
    long bx = (long)((P / 4 + 511) / 512);                                 // ~2 groups of 4 pixels per lane
    bx = bx > kClsBlocksPerView ? kClsBlocksPerView : (bx < 1 ? 1 : bx);
    const dim3 grid((unsigned)bx, (unsigned)B);
    hipStream_t st = as_stream(stream);
    if (format == NERFAIL_EVAL_U8C4)
        cls_batch_kernel<NERFAIL_EVAL_U8C4><<<grid, dim3(256), 0, st>>>((const unsigned char*)images, labels_all, (const long long*)idx,
                                                                         (long)N, (long)P, x, labels);
    else
        cls_batch_kernel<NERFAIL_EVAL_U8C3><<<grid, dim3(256), 0, st>>>((const unsigned char*)images, labels_all, (const long long*)idx,
                                                                         (long)N, (long)P, x, labels);
    NF_LAUNCHED("cls_batch_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_cls_ce(const float* logits, const int32_t* labels, int B, int C, float* d_logits, float* row, void* stream) {
    NF_REQUIRE(B >= 0, "B is negative");
    NF_REQUIRE(C >= 1 && C <= NERFAIL_ATTACK_MAX_CLASSES, "C must be 1..32");
    if (B == 0) return NERFAIL_OK;
    NF_REQUIRE(logits != nullptr && labels != nullptr && row != nullptr, "NULL pointer");
    NF_REQUIRE(aligned_to(logits, 3) && aligned_to(labels, 3) && aligned_to(d_logits, 3) && aligned_to(row, 3), "a buffer is not 4-byte aligned");
    cls_ce_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(logits, labels, B, C, d_logits, row);
    NF_LAUNCHED("cls_ce_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_cnn_sgd_step(float* params, const float* grads, float* momentum_buf, float* packed, int num_classes, float lr,
                                    float momentum, int first, void* stream) {
    NF_REQUIRE(num_classes >= 1 && num_classes <= 4096, "num_classes must be in 1..4096");
    NF_REQUIRE(params != nullptr && grads != nullptr && momentum_buf != nullptr && packed != nullptr, "NULL pointer");
    NF_REQUIRE(aligned_to(params, 15) && aligned_to(grads, 15) && aligned_to(momentum_buf, 15) && aligned_to(packed, 15),
               "params, grads, momentum_buf and packed must be 16-byte aligned");
    SgdArgs a;
    a.G = cnn::grad_layout(num_classes);
    a.L = cnn::pack_layout(num_classes);
    a.C = num_classes;
    a.first = first != 0;
    a.lr = lr;
    a.mu = momentum;
    cnn_sgd_step_kernel<<<dim3((unsigned)((a.G.total + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(a, params, grads, momentum_buf, packed);
    NF_LAUNCHED("cnn_sgd_step_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_cls_epoch_close(const float* train_row, const float* val_row, int64_t n_train, int64_t n_val, float* best, int epoch,
                                       float* record, int32_t* flag, void* stream) {
    NF_REQUIRE(train_row != nullptr && val_row != nullptr && best != nullptr && record != nullptr && flag != nullptr, "NULL pointer");
    NF_REQUIRE(n_train >= 1 && n_val >= 1, "the dataset lengths must be at least 1");
    NF_REQUIRE(epoch >= 0 && epoch < (1 << 24), "epoch must be in [0, 2^24)");
    cls_epoch_close_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(train_row, val_row, (double)n_train, (double)n_val, best, epoch,
                                                                        record, flag);
    NF_LAUNCHED("cls_epoch_close_kernel");
    return NERFAIL_OK;
}
