// The MyCNN victim classifier (model/MyModel.py:5-52): seven stages of 3x3 valid conv + bias + ReLU + 2x2 floor max-pool,
// 3-32-64-128-256-256-128-64 channels, then fc1 1024->512 + ReLU + fc2 512->C. Forward, the gradient with respect to the
// input, and the gradients with respect to the 18 parameters (nerfail_cnn_bwd_weights) on gfx950.
//
// Conv stages: implicit GEMM on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulate). Activations are NHWC between
// stages; stage 1 reads the module's NCHW input directly (3 channels padded to 4, K = 9 taps x 4 = 36 padded to 40).
//   forward:  M = conv pixels, ordered so that the four pixels of one 2x2 pool window are the four rows of one accumulator
//             register group of a lane (row = (reg&3) + 8 (reg>>2) + 4 (lane>>5)): the pool, its argmax and the ReLU happen in
//             registers and the un-pooled output never leaves them. N = Cout, K = (tap, Cin).
//   backward: M = stage-input pixels, N = Cin, K = (tap, Cout): a full correlation with the flipped taps. Its A operand, the
//             un-pooled ReLU-masked output gradient, is formed while it is staged into LDS: the pooled gradient goes to the
//             stored argmax position where the pooled value is not <= 0 (ATen's threshold_backward o max_pool2d_backward).
// A k-unit is 8 k-values: lane half h reads 4 consecutive channels with one ds_read_b128 for each operand, and the unit runs
// 4 MFMAs per (m-tile, n-tile) pair. No atomics: every output element is written by one lane, sums run in a fixed order.
// Stage 1's backward (N = 3) and the FC head are small VALU kernels.
// The workgroup tile, the A-row map, the epilogue, the pool-mask rules (gate, gmask_addr) and the launch grid live in cnn_tile.h,
// which the bf16x3 kernel (cnn_x3.hip) includes as well; the per-stage launch tables are dispatch_stage (cnn_layout.h) over
// stage_cin / stage_cout. On the host one chain (bwd_data_chain) runs the backward-data pass for every entry point.
//
// Multi-RHS backward (nerfail_cnn_bwd_data_multi): R gradients of ONE forward. The backward kernels run one grid slice per
// (r, b): slice g = r * B + b indexes every gradient buffer (d logits, gp, out, d x), image b = g % B indexes what the
// forward kept (act, gmask, hidden). R = 1 is the single backward; the order of every sum does not depend on R.
//
// Weight gradients (nerfail_cnn_bwd_weights): dW[co][ci][tap] = sum over conv pixels p of G[p][co] X[p + tap][ci], the third
// implicit GEMM on the same MFMA: M = Cout, N = (tap, Cin), and the contraction runs over the conv pixels of the batch. G is
// the un-pooled gated gradient stage_grad() forms, X the stage input. Both LDS tiles are [pixel][channel], as the other two
// directions keep them, and NO transposed copy is made: a lane's A element is (m = lane % 32, k = lane / 32) = (channel,
// pixel), so the 32 lanes of a half-wave read 32 CONSECUTIVE CHANNELS of one pixel with one ds_read_b32 (bank-conflict
// free), half-wave h the pixel next to it; the same for B at the pixel shifted by the tap. A wave owns one 32 x 32 (Cout, Cin)
// block with all nine taps (9 accumulators = 144 registers): ten LDS reads feed nine MFMAs. The pixel range is split over
// workgroups in whole 4 x 16 tiles of the FULL (hin - 2) x (win - 2) conv grid (rows and columns the floor pool dropped are
// zeros in G; a tile pixel past the grid gets B = 0 and positions outside the image are zeros in X: never a read outside
// either, and exactly ATen's set of products, so a NaN in X shows in the same taps); every workgroup writes its partial
// [Cout][tap][Cin] slab to scratch and reduce_slabs_kernel adds the slabs in a fixed order (blocks of 16). No float atomics:
// every output is written by one lane, the slab count depends on the shapes only, two runs give the same bits.
// Stage 1 (Cin = 3, NCHW input) is an MFMA tile as well: M = 32 = Cout, N = (ci, tap) = 27 padded to 32 with zero B values,
// one wave per two rows of an 8 x 32 pixel tile, the four waves' accumulators added in LDS in wave order.
// Bias gradients: the sum of the gated pooled gradient over the pooled cells (db_kernel), through the same slabs. FC head:
// VALU kernels, one thread per output, the batch summed in order; dW1's columns come out in PyTorch's c * 16 + y * 4 + x.
#include "common.h"
#include "cnn_tile.h"

namespace nerfail {
namespace cnn {

// ---------------------------------------------------------------------------------------------------------------- pack
// One thread per element of the image; the source index is recomputed from the destination's.

__global__ void pack_conv_fwd_kernel(const float* __restrict__ w, float* __restrict__ dst, int cout, int cin, int taps, int kc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // dst [cout][taps][kc]
    if (i >= cout * taps * kc) return;
    const int c = i % kc, t = (i / kc) % taps, o = i / (kc * taps);
    dst[i] = (c < cin && t < 9) ? w[(o * cin + c) * 9 + t] : 0.f;
}

__global__ void pack_conv_bwd_kernel(const float* __restrict__ w, float* __restrict__ dst, int cout, int cin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;          // dst [cin][9][cout] (tap not flipped: the A offsets flip it)
    if (i >= cout * cin * 9) return;
    const int o = i % cout, t = (i / cout) % 9, c = i / (cout * 9);
    dst[i] = w[(o * cin + c) * 9 + t];
}

__global__ void pack_copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// fc1 [512][1024] with columns in PyTorch's NCHW flatten order (c*16 + y*4 + x) -> NHWC order ((y*4 + x)*64 + c):
// fc1T [1024 nhwc][512] (forward, coalesced over outputs) and fc1P [512][1024 nhwc] (backward, coalesced over inputs)
__global__ void pack_fc1_kernel(const float* __restrict__ w, float* __restrict__ fc1T, float* __restrict__ fc1P) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kFlat * kHidden) return;
    const int o = i / kFlat, j = i % kFlat;                       // j: NHWC flat index
    const int c = j % 64, yx = j / 64;
    const float v = w[o * kFlat + c * 16 + yx];
    fc1P[o * kFlat + j] = v;
    fc1T[j * kHidden + o] = v;
}

// ---------------------------------------------------------------------------------------------------------------- conv stage
// MODE, the workgroup's tile, the A-row map, the epilogue and the pool-mask rules: cnn_tile.h, shared with cnn_x3.hip.
// KC: channels of the K dimension (forward: Cin, backward: Cout); NC: channels of the N dimension (forward: Cout, backward:
// Cin); NT: 32-wide n-tiles per wave; CC: K channels staged per LDS round.
// (ConvArgs: cnn_layout.h)

// Stage one CC-channel slice of the un-pooled, ReLU-masked output gradient at conv positions (gy0 + r, gx0 + c) into LDS
// (row stride XS floats); positions outside [0, 2 hp) x [0, 2 wp) get 0 (rows and columns the floor pool dropped, halo).
// gp is read at gradient slice g, act and gmask at image b.
template <int KC, int CC, int TH, int TW, int XS, int NTHR = 256>
__device__ __forceinline__ void stage_grad(float* xs, const float* __restrict__ gp, const float* __restrict__ act,
                                           const unsigned char* __restrict__ gmask, int g, int b, int hp, int wp, int gy0,
                                           int gx0, int c0) {
    const int n8 = npc8(wp);
    for (int idx = threadIdx.x; idx < TH * TW * (CC / 4); idx += NTHR) {
        const int q4 = idx % (CC / 4), p = idx / (CC / 4);
        const int oy = gy0 + p / TW, ox = gx0 + p % TW;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (oy >= 0 && ox >= 0 && oy < 2 * hp && ox < 2 * wp) {
            const int pr = oy >> 1, pc = ox >> 1;
            const unsigned q = (unsigned)(((oy & 1) << 1) | (ox & 1));
            const size_t cell = ((size_t)b * hp + pr) * wp + pc, gcell = ((size_t)g * hp + pr) * wp + pc;
            const int ch = c0 + 4 * q4;
            const float4 gv = *reinterpret_cast<const float4*>(gp + gcell * KC + ch);
            const float4 av = *reinterpret_cast<const float4*>(act + cell * KC + ch);
            const unsigned mk = *reinterpret_cast<const unsigned*>(gmask_addr(gmask, b, hp, n8, pr, pc, KC, ch));
            const int sh = gate_shift(pc);                      // (one byte per channel: channel j's code at bit 8 j + sh)
            v.x = gate(gv.x, av.x, mk, sh, q);
            v.y = gate(gv.y, av.y, mk, 8 + sh, q);
            v.z = gate(gv.z, av.z, mk, 16 + sh, q);
            v.w = gate(gv.w, av.w, mk, 24 + sh, q);
        }
        *reinterpret_cast<float4*>(xs + p * XS + 4 * q4) = v;
    }
}

template <int MODE, int KC, int NC, int NT, int CC>
__global__ __launch_bounds__(256) void conv_stage_kernel(ConvArgs a) {
    constexpr int TH = Geo<MODE>::TH, TW = Geo<MODE>::TW;
    constexpr int TAPS = MODE == 1 ? 10 : 9;
    constexpr int XS = CC + 4, WS = TAPS * CC + 4;              // LDS row strides (floats), padded against bank conflicts
    constexpr int ZERO_PIX = TH * TW;                           // an all-zero pixel: stage 1's padding tap reads it
    constexpr int UNITS = MODE == 1 ? 5 : 9 * (CC / 8);
    static_assert(KC % CC == 0 && (MODE == 1 ? CC == 4 : CC % 8 == 0), "channel chunking");
    static_assert(NC % (NT * 32) == 0, "n tiles");
    __shared__ __attribute__((aligned(16))) float xs[(TH * TW + 1) * XS];
    __shared__ __attribute__((aligned(16))) float ws[NT * 32 * WS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const int g = blockIdx.z, b = MODE == 2 ? g % a.B : g;      // gradient slice / image (forward: the same)
    const int n0 = blockIdx.y * NT * 32;
    int ty0, tx0, gy0, gx0;
    tile_origin<MODE>(a, ty0, tx0, gy0, gx0);
    int abase[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) abase[mt] = a_row_pixel<MODE>(wave, n, mt);
    // (lane & 31 is both the A row m and the B column n of this lane)

    f32x16 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;

    if (MODE == 1 && tid < XS) xs[ZERO_PIX * XS + tid] = 0.f;

    for (int c0 = 0; c0 < KC; c0 += CC) {
        __syncthreads();
        // ---- A tile
        if (MODE == 0) {
            for (int idx = tid; idx < TH * TW * (CC / 4); idx += 256) {
                const int q4 = idx % (CC / 4), p = idx / (CC / 4);
                const int gy = gy0 + p / TW, gx = gx0 + p % TW;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy < a.hin && gx < a.win)
                    v = *reinterpret_cast<const float4*>(a.in + (((size_t)b * a.hin + gy) * a.win + gx) * KC + c0 + 4 * q4);
                *reinterpret_cast<float4*>(xs + p * XS + 4 * q4) = v;
            }
        } else if (MODE == 1) {
            const size_t plane = (size_t)a.hin * a.win;
            for (int p = tid; p < TH * TW; p += 256) {
                const int gy = gy0 + p / TW, gx = gx0 + p % TW;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (gy < a.hin && gx < a.win) {
                    const float* src = a.in + (size_t)b * 3 * plane + (size_t)gy * a.win + gx;
                    v.x = src[0];
                    v.y = src[plane];
                    v.z = src[2 * plane];
                }
                *reinterpret_cast<float4*>(xs + p * XS) = v;
            }
        } else {
            stage_grad<KC, CC, TH, TW, XS>(xs, a.gp, a.act, a.gmask, g, b, a.hp, a.wp, gy0, gx0, c0);
        }
        // ---- B tile: ws[n][tap * CC + c] = w[(n0 + n)][tap][c0 + c]
        for (int idx = tid; idx < NT * 32 * TAPS * (CC / 4); idx += 256) {
            const int q4 = idx % (CC / 4), t = (idx / (CC / 4)) % TAPS, r = idx / ((CC / 4) * TAPS);
            const float4 v = *reinterpret_cast<const float4*>(a.w + ((size_t)(n0 + r) * TAPS + t) * KC + c0 + 4 * q4);
            *reinterpret_cast<float4*>(ws + r * WS + t * CC + 4 * q4) = v;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < UNITS; ++u) {
            int aidx[2], bofs, ch;
            if (MODE == 1) {                                    // unit u: taps 2u (lane half 0) and 2u + 1 (half 1), 4 channels
                const int t = 2 * u + h;
                ch = 0;
                bofs = t * CC;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) aidx[mt] = t < 9 ? abase[mt] + tap_ofs(MODE, t, TW) : ZERO_PIX;
            } else {                                            // unit u: one tap, channels 8j + 4h .. + 3
                const int t = u / (CC / 8);
                ch = (u % (CC / 8)) * 8 + 4 * h;
                bofs = t * CC + ch;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) aidx[mt] = abase[mt] + tap_ofs(MODE, t, TW);
            }
            float4 av[2], bv[NT];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) av[mt] = *reinterpret_cast<const float4*>(xs + aidx[mt] * XS + ch);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = *reinterpret_cast<const float4*>(ws + (nt * 32 + n) * WS + bofs);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const float x = s == 0 ? av[mt].x : s == 1 ? av[mt].y : s == 2 ? av[mt].z : av[mt].w;
                        const float y = s == 0 ? bv[nt].x : s == 1 ? bv[nt].y : s == 2 ? bv[nt].z : bv[nt].w;
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc[mt][nt], 0, 0, 0);
                    }
        }
    }

    epilogue<MODE, NC, NT>(acc, a, g, b, n0, ty0, tx0, wave, n, h);
}

// Stage 1 backward-data (N = 3 input channels: too narrow for a 32-wide MFMA tile): one thread per input pixel of a 16 x 16
// tile, the masked output gradient of the 18 x 18 footprint x 32 channels in LDS, weights read wave-uniformly. Writes NCHW.
__global__ __launch_bounds__(256) void conv1_bwd_kernel(const float* __restrict__ w1raw, const float* __restrict__ gp,
                                                        const float* __restrict__ act, const unsigned char* __restrict__ gmask,
                                                        float* __restrict__ dx, int hin, int win, int hp, int wp, int B) {
    constexpr int TH = 18, TW = 18, CC = 32, XS = CC + 4;
    __shared__ __attribute__((aligned(16))) float xs[TH * TW * XS];
    const int nx = (win + 15) / 16;
    const int ty0 = (blockIdx.x / nx) * 16, tx0 = (blockIdx.x % nx) * 16, gs = blockIdx.z, b = gs % B;
    stage_grad<32, CC, TH, TW, XS>(xs, gp, act, gmask, gs, b, hp, wp, ty0 - 2, tx0 - 2, 0);
    __syncthreads();
    const int ly = threadIdx.x / 16, lx = threadIdx.x % 16;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int ky = t / 3, kx = t % 3;
        const float* g = xs + ((ly + 2 - ky) * TW + lx + 2 - kx) * XS;
#pragma unroll 4
        for (int c4 = 0; c4 < CC; c4 += 4) {
            const float4 v = *reinterpret_cast<const float4*>(g + c4);
            const float gg[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* wc = w1raw + (c4 + j) * 27 + t;   // [co][ci][tap]
                s0 = fmaf(gg[j], wc[0], s0);
                s1 = fmaf(gg[j], wc[9], s1);
                s2 = fmaf(gg[j], wc[18], s2);
            }
        }
    }
    const int y = ty0 + ly, x = tx0 + lx;
    if (y < hin && x < win) {
        const size_t plane = (size_t)hin * win, o = (size_t)gs * 3 * plane + (size_t)y * win + x;
        dx[o] = s0;
        dx[o + plane] = s1;
        dx[o + 2 * plane] = s2;
    }
}

// ---------------------------------------------------------------------------------------------------------------- FC head
// One workgroup of 512 threads per image: hidden = relu(fc1 x + b1) (saved for the backward), logits = fc2 hidden + b2.
__global__ __launch_bounds__(512) void fc_fwd_kernel(const float* __restrict__ x, const float* __restrict__ fc1T,
                                                     const float* __restrict__ b1, const float* __restrict__ w2,
                                                     const float* __restrict__ b2, int C, float* __restrict__ hidden,
                                                     float* __restrict__ logits) {
    __shared__ float xv[kFlat];
    __shared__ float hv[kHidden];
    const int b = blockIdx.x, o = threadIdx.x;
    xv[o] = x[(size_t)b * kFlat + o];
    xv[o + kHidden] = x[(size_t)b * kFlat + o + kHidden];
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < kFlat; ++i) s = fmaf(fc1T[(size_t)i * kHidden + o], xv[i], s);
    s += b1[o];
    s = s < 0.f ? 0.f : s;
    hidden[(size_t)b * kHidden + o] = s;
    hv[o] = s;
    __syncthreads();
    const int lane = o & 63, wave = o >> 6;
    for (int c = wave; c < C; c += kHidden / 64) {
        float p = 0.f;
        for (int i = lane; i < kHidden; i += 64) p = fmaf(hv[i], w2[(size_t)c * kHidden + i], p);
        p = wave_sum(p);
        if (lane == 0) logits[(size_t)b * C + c] = p + b2[c];
    }
}

// d hidden = (fc2^T d logits) gated by hidden > 0 (NaN passes, as threshold_backward), d x = fc1^T d hidden in NHWC order.
// One workgroup per gradient slice g = r * B + b: d logits and d x at g, hidden at image b.
__global__ __launch_bounds__(1024) void fc_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ hidden,
                                                      const float* __restrict__ fc1P, const float* __restrict__ w2, int C, int B,
                                                      float* __restrict__ dx) {
    __shared__ float dh[kHidden];
    const int g = blockIdx.x, b = g % B, t = threadIdx.x;
    if (t < kHidden) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = fmaf(dlogits[(size_t)g * C + c], w2[(size_t)c * kHidden + t], s);
        dh[t] = hidden[(size_t)b * kHidden + t] <= 0.f ? 0.f : s;
    }
    __syncthreads();
    float s = 0.f;
    for (int o = 0; o < kHidden; ++o) s = fmaf(fc1P[(size_t)o * kFlat + t], dh[o], s);
    dx[(size_t)g * kFlat + t] = s;
}

// ---------------------------------------------------------------------------------------------------------------- launches
template <int MODE, int KC, int NC, int NT, int CC>
static int launch_conv(const ConvArgs& a, int Z, hipStream_t st, const char* name) {   // Z: grid slices (B, or R * B)
    conv_stage_kernel<MODE, KC, NC, NT, CC><<<conv_grid<MODE, NC, NT>(a, Z), dim3(256), 0, st>>>(a);
    NF_LAUNCHED(name);
    return 0;
}

constexpr int kConvCC = 16;                                     // K channels per LDS round (stage 1's forward: its 4 padded ones)

static int conv_fwd_stage(int s, const ConvArgs& a, int B, hipStream_t st) {
    static const char* const name[kStages] = NF_STAGE_LABELS("cnn_conv_fwd");
    return dispatch_stage(s, [&](auto S) {
        constexpr int KC = fwd_kc(S), NC = stage_cout(S);
        return launch_conv<S == 0 ? 1 : 0, KC, NC, conv_nt(NC), S == 0 ? KC : kConvCC>(a, B, st, name[S]);
    });
}

static int conv_bwd_stage(int s, const ConvArgs& a, int Z, hipStream_t st) {   // s >= 1: KC = Cout, NC = Cin
    static const char* const name[kStages] = NF_STAGE_LABELS("cnn_conv_bwd");
    return dispatch_stage(s, [&](auto S) {
        if constexpr (S == 0) return NERFAIL_EINVAL;            // (stage 1's backward is conv1_bwd_kernel)
        else return launch_conv<2, stage_cout(S), stage_cin(S), conv_nt(stage_cin(S)), kConvCC>(a, Z, st, name[S]);
    });
}

static size_t workspace_floats(const Dims& d, int B) {
    size_t n = 0;
    for (int s = 0; s < kStages; ++s) n += act_floats(d, s, B);
    return n + (size_t)B * kHidden;
}


// ---------------------------------------------------------------------------------------------------------------- weight gradients
// Stages >= 2: a tile is 4 x 16 conv pixels (k-steps of two pixels side by side: lane half h takes pixel 2 j + h), stage 1:
// 8 x 32. A slab is `tps` consecutive tiles of the (image, tile row, tile column) order; the last slab may be shorter.
constexpr int kDwTH = 4, kDwTW = 16, kDw1TH = 8, kDw1TW = 32;
constexpr int kDwWorkgroups = 1024;                             // slabs x channel blocks aimed at per stage
constexpr size_t kDwPartFloats = (size_t)16 << 20;              // cap of the partial-slab region (64 MB)
constexpr int kDwWM = 2;                                        // waves over Cout, waves over Cin: a workgroup's channel block
constexpr int dw_wn(int cin) { return cin >= 64 ? 2 : 1; }

struct DwArgs {
    const float* in;           // stage input: NHWC [B, hin, win, Cin], stage 1: the module's NCHW input
    const float* gp;           // d pooled output of the stage (NHWC)
    const float* act;          // pooled output (NHWC)
    const unsigned char* gmask;
    float* part;               // partial slabs
    int hin, win, hp, wp;
    int ntx, nty, ntiles, tps; // tiles per image row / column, tiles of the batch, tiles per slab
};

// KC = Cout (M), NC = Cin (N, times nine taps); WM x WN waves, wave (wm, wn) owns Cout block co0 + 32 wm, Cin block ci0 + 32 wn.
// part: [slab][Cout][tap][Cin].
template <int KC, int NC, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void conv_dw_kernel(DwArgs a) {
    constexpr int NTHR = 64 * WM * WN, MCH = 32 * WM, NCH = 32 * WN, TH = kDwTH, TW = kDwTW, XH = TH + 2, XW = TW + 2;
    constexpr int GS = MCH + 4, XS = NCH + 4;                   // LDS row strides (floats): 16-byte rows, half-waves 4 banks apart
    static_assert(KC % MCH == 0 && NC % NCH == 0, "channel blocks");
    __shared__ __attribute__((aligned(16))) float gs[TH * TW * GS];
    __shared__ __attribute__((aligned(16))) float xt[XH * XW * XS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5, wm = wave % WM, wn = wave / WM;
    const int co0 = (blockIdx.y % (KC / MCH)) * MCH, ci0 = (blockIdx.y / (KC / MCH)) * NCH;
    const int slab = blockIdx.x;

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    const int t0 = slab * a.tps, t1 = min(t0 + a.tps, a.ntiles);
    for (int t = t0; t < t1; ++t) {
        const int per = a.nty * a.ntx, b = t / per, r = t % per;
        const int gy0 = (r / a.ntx) * TH, gx0 = (r % a.ntx) * TW;
        __syncthreads();
        stage_grad<KC, MCH, TH, TW, GS, NTHR>(gs, a.gp, a.act, a.gmask, b, b, a.hp, a.wp, gy0, gx0, co0);
        for (int idx = tid; idx < XH * XW * (NCH / 4); idx += NTHR) {
            const int q4 = idx % (NCH / 4), p = idx / (NCH / 4);
            const int gy = gy0 + p / XW, gx = gx0 + p % XW;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy < a.hin && gx < a.win)
                v = *reinterpret_cast<const float4*>(a.in + (((size_t)b * a.hin + gy) * a.win + gx) * NC + ci0 + 4 * q4);
            *reinterpret_cast<float4*>(xt + p * XS + 4 * q4) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int py = 0; py < TH; ++py) {                       // (one row per trip: the unrolled tile keeps 120 operands live)
            const float* ga = gs + (py * TW + h) * GS + wm * 32 + n;
            const float* xa = xt + (py * XW + h) * XS + wn * 32 + n;
            const bool rowok = gy0 + py < a.hin - 2;
#pragma unroll
            for (int j = 0; j < TW / 2; ++j) {
                // a pixel past the conv grid contributes no product at all (G is 0 there, but 0 x NaN would not be)
                const bool ok = rowok && gx0 + 2 * j + h < a.win - 2;
                const float av = ga[2 * j * GS];
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) {
                    const float bv = xa[((tap / 3) * XW + tap % 3 + 2 * j) * XS];
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ok ? bv : 0.f, acc[tap], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int co = co0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            a.part[(((size_t)slab * KC + co) * 9 + tap) * NC + ci0 + wn * 32 + n] = acc[tap][i];
        }
}

// Stage 1: M = 32 output channels, N = 27 (ci, tap) columns padded to 32 (B = 0 there), wave w takes rows 2w, 2w + 1 of the
// 8 x 32 tile. part: [slab][32 co][32 n], n = ci * 9 + tap (conv1.weight's own order).
__global__ __launch_bounds__(256) void conv1_dw_kernel(DwArgs a) {
    constexpr int TH = kDw1TH, TW = kDw1TW, XH = TH + 2, XW = TW + 2, XP = XH * XW, GS = 36;
    __shared__ __attribute__((aligned(16))) float gs[TH * TW * GS];
    __shared__ float xt[3 * XP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 31, h = lane >> 5;
    const bool live = n < 27;
    const int bofs = live ? (n / 9) * XP + ((n % 9) / 3) * XW + n % 3 : 0;
    const int slab = blockIdx.x;
    const size_t plane = (size_t)a.hin * a.win;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

    const int t0 = slab * a.tps, t1 = min(t0 + a.tps, a.ntiles);
    for (int t = t0; t < t1; ++t) {
        const int per = a.nty * a.ntx, b = t / per, r = t % per;
        const int gy0 = (r / a.ntx) * TH, gx0 = (r % a.ntx) * TW;
        __syncthreads();
        stage_grad<32, 32, TH, TW, GS>(gs, a.gp, a.act, a.gmask, b, b, a.hp, a.wp, gy0, gx0, 0);
        for (int idx = tid; idx < 3 * XP; idx += 256) {
            const int c = idx / XP, p = idx % XP;
            const int gy = gy0 + p / XW, gx = gx0 + p % XW;
            xt[idx] = (gy < a.hin && gx < a.win) ? a.in[((size_t)b * 3 + c) * plane + (size_t)gy * a.win + gx] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TW; ++j) {                          // 64 pixels of the wave's two rows, two per k-step
            const int py = 2 * wave + (2 * j) / TW, px = (2 * j) % TW + h;
            const float av = gs[(py * TW + px) * GS + n];
            const bool ok = live && gy0 + py < a.hin - 2 && gx0 + px < a.win - 2;   // (past the conv grid: no product)
            const float bv = ok ? xt[bofs + py * XW + px] : 0.f;
            acc[j & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j & 1], 0, 0, 0);
        }
    }
    __syncthreads();                                            // gs becomes [4 waves][32 co][32 n]
#pragma unroll
    for (int i = 0; i < 16; ++i) gs[(wave * 32 + (i & 3) + 8 * (i >> 2) + 4 * h) * 32 + n] = acc[0][i] + acc[1][i];
    __syncthreads();
    for (int idx = tid; idx < 1024; idx += 256)
        a.part[(size_t)slab * 1024 + idx] = ((gs[idx] + gs[1024 + idx]) + gs[2048 + idx]) + gs[3072 + idx];
}

// db: the gated pooled gradient (act <= 0 -> 0, NaN passes) summed over `cps` pooled cells per workgroup. part: [slab][C].
template <int C>
__global__ __launch_bounds__(256) void db_kernel(const float* __restrict__ gp, const float* __restrict__ act,
                                                 float* __restrict__ part, size_t cells, int cps) {
    constexpr int Q = C / 4, L = 256 / Q;
    __shared__ __attribute__((aligned(16))) float red[L * C];
    const int q = threadIdx.x % Q, l = threadIdx.x / Q;
    const size_t c0 = (size_t)blockIdx.x * cps, c1 = min(c0 + (size_t)cps, cells);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t cell = c0 + l; cell < c1; cell += L) {
        const float4 gv = *reinterpret_cast<const float4*>(gp + cell * C + 4 * q);
        const float4 av = *reinterpret_cast<const float4*>(act + cell * C + 4 * q);
        s.x += av.x <= 0.f ? 0.f : gv.x;
        s.y += av.y <= 0.f ? 0.f : gv.y;
        s.z += av.z <= 0.f ? 0.f : gv.z;
        s.w += av.w <= 0.f ? 0.f : gv.w;
    }
    *reinterpret_cast<float4*>(red + l * C + 4 * q) = s;
    __syncthreads();
    if (threadIdx.x < C) {
        float t = 0.f;
        for (int k = 0; k < L; ++k) t += red[k * C + threadIdx.x];
        part[(size_t)blockIdx.x * C + threadIdx.x] = t;
    }
}

// dst = the S slabs added in a fixed order, sixteen at a time. One thread per slab element i < n.
// mode 0: dst[i]; mode 1: slab [Cout][tap][NC] -> dst [Cout][NC][tap]; mode 2: slab [32][32] -> dst [32][27].
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ part, int S, int n, int NC, int mode,
                                                           float* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float total = 0.f;
    for (int s0 = 0; s0 < S; s0 += 16) {
        float g = 0.f;
        const int s1 = min(s0 + 16, S);
        for (int s = s0; s < s1; ++s) g += part[(size_t)s * n + i];
        total += g;
    }
    if (mode == 0) {
        dst[i] = total;
    } else if (mode == 1) {
        const int ci = i % NC, t = (i / NC) % 9, co = i / (9 * NC);
        dst[((size_t)co * NC + ci) * 9 + t] = total;
    } else if (i % 32 < 27) {
        dst[(i / 32) * 27 + i % 32] = total;
    }
}

// d hidden [B][512] = (fc2^T d logits) gated by hidden > 0 (NaN passes): fc_bwd_kernel's first half, kept.
__global__ __launch_bounds__(512) void fc_dh_kernel(const float* __restrict__ dlogits, const float* __restrict__ hidden,
                                                    const float* __restrict__ w2, int C, float* __restrict__ dh) {
    const int b = blockIdx.x, t = threadIdx.x;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = fmaf(dlogits[(size_t)b * C + c], w2[(size_t)c * kHidden + t], s);
    dh[(size_t)b * kHidden + t] = hidden[(size_t)b * kHidden + t] <= 0.f ? 0.f : s;
}

// fc1.weight [512][1024] (column c * 16 + yx reads the NHWC stage-7 output at yx * 64 + c: pack_fc1_kernel's permutation
// inverted), fc1.bias, fc2.weight [C][512], fc2.bias: one thread per output, the batch summed in order.
__global__ __launch_bounds__(256) void fc_dw_kernel(const float* __restrict__ dlogits, const float* __restrict__ hidden,
                                                    const float* __restrict__ dh, const float* __restrict__ x7, int B, int C,
                                                    float* __restrict__ dW1, float* __restrict__ db1, float* __restrict__ dW2,
                                                    float* __restrict__ db2) {
    const int n1 = kHidden * kFlat, n2 = C * kHidden;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    float s = 0.f;
    if (i < n1) {
        const int o = i / kFlat, col = i % kFlat, j = (col % 16) * 64 + col / 16;
        for (int b = 0; b < B; ++b) s = fmaf(dh[(size_t)b * kHidden + o], x7[(size_t)b * kFlat + j], s);
        dW1[i] = s;
    } else if ((i -= n1) < kHidden) {
        for (int b = 0; b < B; ++b) s += dh[(size_t)b * kHidden + i];
        db1[i] = s;
    } else if ((i -= kHidden) < n2) {
        const int c = i / kHidden, u = i % kHidden;
        for (int b = 0; b < B; ++b) s = fmaf(dlogits[(size_t)b * C + c], hidden[(size_t)b * kHidden + u], s);
        dW2[i] = s;
    } else if ((i -= n2) < C) {
        for (int b = 0; b < B; ++b) s += dlogits[(size_t)b * C + i];
        db2[i] = s;
    }
}

// ---- host side of the weight gradients
struct DwPlan {
    int ntx, nty, ntiles, tps, slabs, ny;                       // ny: channel blocks (grid y)
    size_t out;                                                 // floats of one slab
    int db_cps, db_slabs;
};
static DwPlan dw_plan(const Dims& d, int s, int B) {
    DwPlan p;
    const int th = s == 0 ? kDw1TH : kDwTH, tw = s == 0 ? kDw1TW : kDwTW;
    p.nty = (d.hin[s] - 2 + th - 1) / th;
    p.ntx = (d.win[s] - 2 + tw - 1) / tw;
    p.ntiles = B * p.nty * p.ntx;
    p.ny = s == 0 ? 1 : (stage_cout(s) / (32 * kDwWM)) * (stage_cin(s) / (32 * dw_wn(stage_cin(s))));
    p.out = s == 0 ? 1024 : (size_t)stage_cout(s) * 9 * stage_cin(s);
    size_t want = (size_t)(kDwWorkgroups + p.ny - 1) / p.ny;
    if (want > kDwPartFloats / p.out) want = kDwPartFloats / p.out;
    if (want > (size_t)p.ntiles) want = (size_t)p.ntiles;
    if (want < 1) want = 1;
    p.tps = (int)((p.ntiles + want - 1) / want);
    p.slabs = (p.ntiles + p.tps - 1) / p.tps;
    const size_t cells = (size_t)B * d.hin[s + 1] * d.win[s + 1];
    p.db_cps = (int)((cells + 255) / 256);
    p.db_slabs = (int)((cells + p.db_cps - 1) / p.db_cps);
    return p;
}

struct DwScratch {                                              // scratch of nerfail_cnn_bwd_weights (floats)
    size_t gpool[kStages], dh, part, total;
};
static DwScratch dw_scratch(const Dims& d, int B) {
    DwScratch L;
    size_t o = 0, m = 0;
    for (int s = 0; s < kStages; ++s) {
        L.gpool[s] = o; o += up4(act_floats(d, s, B));
        const DwPlan p = dw_plan(d, s, B);
        const size_t a = (size_t)p.slabs * p.out, c = (size_t)p.db_slabs * stage_cout(s);
        m = a > m ? a : m;
        m = c > m ? c : m;
    }
    L.dh = o; o += up4((size_t)B * kHidden);
    L.part = o; o += up4(m);
    L.total = o;
    return L;
}

static int conv_dw_stage(int s, const DwArgs& a, const DwPlan& p, hipStream_t st) {
    static const char* const name[kStages] = NF_STAGE_LABELS("cnn_conv_dw");
    return dispatch_stage(s, [&](auto S) {
        constexpr int WN = dw_wn(stage_cin(S));
        if constexpr (S == 0) conv1_dw_kernel<<<dim3((unsigned)p.slabs), dim3(256), 0, st>>>(a);
        else conv_dw_kernel<stage_cout(S), stage_cin(S), kDwWM, WN><<<dim3((unsigned)p.slabs, (unsigned)p.ny), dim3(64 * kDwWM * WN), 0, st>>>(a);
        NF_LAUNCHED(name[S]);
        return 0;
    });
}

static int db_stage(int s, const float* gp, const float* act, float* part, size_t cells, const DwPlan& p, hipStream_t st) {
    return dispatch_stage(s, [&](auto S) {
        db_kernel<stage_cout(S)><<<dim3((unsigned)p.db_slabs), dim3(256), 0, st>>>(gp, act, part, cells, p.db_cps);
        NF_LAUNCHED("cnn_db");
        return 0;
    });
}

static int reduce_slabs(const float* part, int S, size_t n, int NC, int mode, float* dst, hipStream_t st) {
    reduce_slabs_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(part, S, (int)n, NC, mode, dst);
    NF_LAUNCHED("cnn_reduce_slabs");
    return 0;
}

}  // namespace cnn
}  // namespace nerfail

using namespace nerfail;
using namespace nerfail::cnn;

extern "C" size_t nerfail_cnn_packed_floats(int num_classes) {
    if (num_classes < 1 || num_classes > 4096) return 0;
    return pack_layout(num_classes).total;
}

extern "C" int nerfail_cnn_pack(const float* const* params_host, int num_classes, float* packed, void* stream) {
    NF_REQUIRE(num_classes >= 1 && num_classes <= 4096, "num_classes must be in 1..4096");
    NF_REQUIRE(params_host != nullptr && packed != nullptr, "params_host or packed is NULL");
    for (int i = 0; i < 16; ++i) NF_REQUIRE(params_host[i] != nullptr, "a parameter pointer is NULL");
    const PackLayout L = pack_layout(num_classes);
    hipStream_t st = as_stream(stream);
    const int T = 256;
    for (int s = 0; s < kStages; ++s) {
        const float* w = params_host[2 * s];
        const float* bias = params_host[2 * s + 1];
        const int co = stage_cout(s), ci = stage_cin(s);
        int n = co * fwd_taps(s) * fwd_kc(s);
        pack_conv_fwd_kernel<<<dim3((n + T - 1) / T), dim3(T), 0, st>>>(w, packed + L.fwd[s], co, ci, fwd_taps(s), fwd_kc(s));
        NF_LAUNCHED("cnn_pack_conv_fwd");
        pack_copy_kernel<<<dim3((co + T - 1) / T), dim3(T), 0, st>>>(bias, packed + L.bias[s], co);
        NF_LAUNCHED("cnn_pack_copy");
        if (s > 0) {
            n = co * ci * 9;
            pack_conv_bwd_kernel<<<dim3((n + T - 1) / T), dim3(T), 0, st>>>(w, packed + L.bwd[s], co, ci);
            NF_LAUNCHED("cnn_pack_conv_bwd");
        } else {
            pack_copy_kernel<<<dim3((32 * 27 + T - 1) / T), dim3(T), 0, st>>>(w, packed + L.w1raw, 32 * 27);
            NF_LAUNCHED("cnn_pack_copy");
        }
    }
    pack_fc1_kernel<<<dim3(kFlat * kHidden / T), dim3(T), 0, st>>>(params_host[14], packed + L.fc1T, packed + L.fc1P);
    NF_LAUNCHED("cnn_pack_fc1");
    pack_copy_kernel<<<dim3(kHidden / T), dim3(T), 0, st>>>(params_host[15], packed + L.b1, kHidden);
    NF_LAUNCHED("cnn_pack_copy");
    const int n2 = num_classes * kHidden;
    pack_copy_kernel<<<dim3((n2 + T - 1) / T), dim3(T), 0, st>>>(params_host[16], packed + L.w2, n2);
    NF_LAUNCHED("cnn_pack_copy");
    pack_copy_kernel<<<dim3((num_classes + T - 1) / T), dim3(T), 0, st>>>(params_host[17], packed + L.b2, num_classes);
    NF_LAUNCHED("cnn_pack_copy");
    return 0;
}

extern "C" size_t nerfail_cnn_workspace_bytes(int B, int H, int W, int C) {
    Dims d;
    if (B < 1 || B > 65535 || C < 1 || C > 4096 || !dims_of(H, W, d)) return 0;
    return workspace_floats(d, B) * sizeof(float);
}

extern "C" size_t nerfail_cnn_mask_bytes(int B, int H, int W) {
    Dims d;
    if (B < 1 || B > 65535 || !dims_of(H, W, d)) return 0;
    size_t n = 0;
    for (int s = 0; s < kStages; ++s) n += mask_bytes_of(d, s, B);
    return n;
}

extern "C" size_t nerfail_cnn_bwd_scratch_bytes(int B, int H, int W) {
    Dims d;
    if (B < 1 || B > 65535 || !dims_of(H, W, d)) return 0;
    return (act_floats(d, 0, B) + act_floats(d, 1, B)) * sizeof(float);
}

// The forward launch chain (arguments already validated). x3 = NULL: the exact kernels; else stages 2..7 on the bf16x3 image.
static int fwd_launch(const float* packed, const void* x3, int num_classes, const float* x, int B, const Dims& d, float* workspace,
                      unsigned char* masks, float* logits, void* stream) {
    const PackLayout L = pack_layout(num_classes);
    hipStream_t st = as_stream(stream);
    const float* in = x;
    float* act = workspace;
    unsigned char* mk = masks;
    for (int s = 0; s < kStages; ++s) {
        ConvArgs a = {};
        a.in = in;
        a.w = packed + L.fwd[s];
        a.bias = packed + L.bias[s];
        a.out = act;
        a.mask = mk;
        a.hin = d.hin[s];
        a.win = d.win[s];
        a.hp = d.hin[s + 1];
        a.wp = d.win[s + 1];
        int rc = (x3 && s >= 1) ? conv_fwd_stage_x3(s, a, x3, B, st) : conv_fwd_stage(s, a, B, st);
        if (rc) return rc;
        in = act;
        act += act_floats(d, s, B);
        if (mk) mk += mask_bytes_of(d, s, B);
    }
    fc_fwd_kernel<<<dim3(B), dim3(kHidden), 0, st>>>(in, packed + L.fc1T, packed + L.b1, packed + L.w2, packed + L.b2, num_classes,
                                                     act, logits);
    NF_LAUNCHED("cnn_fc_fwd");
    return 0;
}

// True when R right-hand sides of a B-image forward fit the grid's z dimension (R * B <= 65535).
static bool multi_ok(int R, int B) { return R >= 1 && B >= 1 && R <= 65535 && B <= 65535 && (long long)R * B <= 65535; }

template <class... P>
static bool all_set(const P*... p) { return (... && (p != nullptr)); }

// The refusals every forward and backward entry point shares, in this order: num_classes, the batch (BATCH = B, or RB for the
// multi backward), H x W (fills the caller's Dims `d`), then the pointers of the entry point (`names` lists them for the message).
#define NF_CNN_BATCH_B NF_REQUIRE(B >= 1 && B <= 65535, "B must be in 1..65535")
#define NF_CNN_BATCH_RB \
    NF_REQUIRE(multi_ok(R, B), "R and B must be >= 1 with R * B <= 65535 (one grid slice per right-hand side and image)")
#define NF_CNN_CHECKS(BATCH, d, names, ...)                                                                            \
    NF_REQUIRE(num_classes >= 1 && num_classes <= 4096, "num_classes must be in 1..4096");                             \
    NF_CNN_BATCH_##BATCH;                                                                                              \
    NF_REQUIRE(dims_of(H, W, d), "unsupported H x W: the seventh stage must be 4 x 4 (fc1 takes 1024 inputs)");        \
    NF_REQUIRE(all_set(__VA_ARGS__), names " is NULL")

extern "C" int nerfail_cnn_fwd(const float* packed, int num_classes, const float* x, int B, int H, int W, float* workspace,
                               unsigned char* masks, float* logits, void* stream) {
    Dims d;
    NF_CNN_CHECKS(B, d, "packed, x, workspace or logits", packed, x, workspace, logits);
    return fwd_launch(packed, nullptr, num_classes, x, B, d, workspace, masks, logits, stream);
}

extern "C" int nerfail_cnn_fwd_x3(const float* packed, const void* packed_x3, int num_classes, const float* x, int B, int H, int W,
                                  float* workspace, unsigned char* masks, float* logits, void* stream) {
    Dims d;
    NF_CNN_CHECKS(B, d, "packed, x, workspace or logits", packed, x, workspace, logits);
    NF_REQUIRE(packed_x3 != nullptr, "packed_x3 is NULL");
    return fwd_launch(packed, packed_x3, num_classes, x, B, d, workspace, masks, logits, stream);
}

extern "C" size_t nerfail_cnn_bwd_multi_scratch_bytes(int R, int B, int H, int W) {
    Dims d;
    if (!multi_ok(R, B) || !dims_of(H, W, d)) return 0;
    return (act_floats(d, 0, R * B) + act_floats(d, 1, R * B)) * sizeof(float);
}

// What a forward of B images kept, per stage: its pooled outputs and pool masks in the workspace's and masks' order, then the
// FC head's hidden layer.
struct FwdView {
    const float* acts[kStages];
    const unsigned char* mks[kStages];
    const float* hidden;
};
static FwdView fwd_view(const float* workspace, const unsigned char* masks, const Dims& d, int B) {
    FwdView v;
    for (int s = 0; s < kStages; ++s) {
        v.acts[s] = workspace;
        v.mks[s] = masks;
        workspace += act_floats(d, s, B);
        masks += mask_bytes_of(d, s, B);
    }
    v.hidden = workspace;
    return v;
}

// The backward-data chain for Z = R * B gradient slices of one B-image forward (arguments already validated): the FC head,
// stages 7..2 (x3 = NULL: the exact kernels; else on the bf16x3 image) and stage 1 (d_x = NULL: not wanted). gp[s]: where the
// gradient of stage s's pooled output lives (Z slices); every caller's layout runs the same kernels, grids and arguments.
static int bwd_data_chain(const float* packed, const void* x3, int num_classes, const FwdView& v, const float* d_logits, int Z, int B,
                          const Dims& d, float* const* gp, float* d_x, hipStream_t st) {
    const PackLayout L = pack_layout(num_classes);
    fc_bwd_kernel<<<dim3(Z), dim3(kFlat), 0, st>>>(d_logits, v.hidden, packed + L.fc1P, packed + L.w2, num_classes, B, gp[6]);
    NF_LAUNCHED("cnn_fc_bwd");
    for (int s = kStages - 1; s >= 1; --s) {
        ConvArgs a = {};
        a.w = packed + L.bwd[s];
        a.out = gp[s - 1];                        // d (stage s input) = d (stage s-1 output)
        a.gp = gp[s];
        a.act = v.acts[s];
        a.gmask = v.mks[s];
        a.hin = d.hin[s];
        a.win = d.win[s];
        a.hp = d.hin[s + 1];
        a.wp = d.win[s + 1];
        a.B = B;
        int rc = x3 ? conv_bwd_stage_x3(s, a, x3, Z, st) : conv_bwd_stage(s, a, Z, st);
        if (rc) return rc;
    }
    if (d_x) {
        const int H = d.hin[0], W = d.win[0];
        const unsigned tiles = (unsigned)(((W + 15) / 16) * ((H + 15) / 16));
        conv1_bwd_kernel<<<dim3(tiles, 1, Z), dim3(256), 0, st>>>(packed + L.w1raw, gp[0], v.acts[0], v.mks[0], d_x, H, W, d.hin[1],
                                                                 d.win[1], B);
        NF_LAUNCHED("cnn_conv1_bwd");
    }
    return 0;
}

// nerfail_cnn_bwd_data[_multi][_x3]: R right-hand sides of one B-image forward, the gradients in a ping-pong pair of scratch.
static int bwd_data_launch(const float* packed, const void* x3, int num_classes, const float* workspace, const unsigned char* masks,
                           const float* d_logits, int R, int B, const Dims& d, float* scratch, float* d_x, void* stream) {
    const int Z = R * B;                                         // gradient slices: the grid's z (FC head: x) dimension
    float* const odd = scratch + act_floats(d, 0, Z);            // stage outputs 5, 3, 1; scratch itself: 6, 4, 2, 0
    float* const gp[kStages] = {scratch, odd, scratch, odd, scratch, odd, scratch};
    return bwd_data_chain(packed, x3, num_classes, fwd_view(workspace, masks, d, B), d_logits, Z, B, d, gp, d_x, as_stream(stream));
}

// The single backward is the R = 1 case: the same kernels, the same grid, the same bits.
extern "C" int nerfail_cnn_bwd_data(const float* packed, int num_classes, const float* workspace, const unsigned char* masks,
                                    const float* d_logits, int B, int H, int W, float* scratch, float* d_x, void* stream) {
    Dims d;
    NF_CNN_CHECKS(B, d, "packed, workspace, masks, d_logits, scratch or d_x", packed, workspace, masks, d_logits, scratch, d_x);
    return bwd_data_launch(packed, nullptr, num_classes, workspace, masks, d_logits, 1, B, d, scratch, d_x, stream);
}

extern "C" int nerfail_cnn_bwd_data_multi(const float* packed, int num_classes, const float* workspace, const unsigned char* masks,
                                          const float* d_logits, int R, int B, int H, int W, float* scratch, float* d_x,
                                          void* stream) {
    Dims d;
    NF_CNN_CHECKS(RB, d, "packed, workspace, masks, d_logits, scratch or d_x", packed, workspace, masks, d_logits, scratch, d_x);
    return bwd_data_launch(packed, nullptr, num_classes, workspace, masks, d_logits, R, B, d, scratch, d_x, stream);
}

// The bf16x3 forms: the same refusals, the same buffers and size functions; stages 7..2 run on the bf16x3 image (cnn_x3.hip),
// the FC head and stage 1 on the exact kernels above.
extern "C" int nerfail_cnn_bwd_data_x3(const float* packed, const void* packed_x3, int num_classes, const float* workspace,
                                       const unsigned char* masks, const float* d_logits, int B, int H, int W, float* scratch,
                                       float* d_x, void* stream) {
    Dims d;
    NF_CNN_CHECKS(B, d, "packed, packed_x3, workspace, masks, d_logits, scratch or d_x", packed, packed_x3, workspace, masks, d_logits,
                  scratch, d_x);
    return bwd_data_launch(packed, packed_x3, num_classes, workspace, masks, d_logits, 1, B, d, scratch, d_x, stream);
}

extern "C" int nerfail_cnn_bwd_data_multi_x3(const float* packed, const void* packed_x3, int num_classes, const float* workspace,
                                             const unsigned char* masks, const float* d_logits, int R, int B, int H, int W,
                                             float* scratch, float* d_x, void* stream) {
    Dims d;
    NF_CNN_CHECKS(RB, d, "packed, packed_x3, workspace, masks, d_logits, scratch or d_x", packed, packed_x3, workspace, masks, d_logits,
                  scratch, d_x);
    return bwd_data_launch(packed, packed_x3, num_classes, workspace, masks, d_logits, R, B, d, scratch, d_x, stream);
}

// ---------------------------------------------------------------------------------------------------------------- weight gradients
extern "C" size_t nerfail_cnn_grad_floats(int num_classes) {
    if (num_classes < 1 || num_classes > 4096) return 0;
    return grad_layout(num_classes).total;
}

extern "C" size_t nerfail_cnn_bwd_weights_scratch_bytes(int B, int H, int W, int num_classes) {
    Dims d;
    if (B < 1 || B > 65535 || num_classes < 1 || num_classes > 4096 || !dims_of(H, W, d)) return 0;
    return dw_scratch(d, B).total * sizeof(float);
}

// bwd_data_chain with every stage's pooled gradient kept in its own region (d_x as nerfail_cnn_bwd_data's, or NULL), then
// the FC head's and every stage's weight and bias gradient.
extern "C" int nerfail_cnn_bwd_weights(const float* packed, int num_classes, const float* x, const float* workspace,
                                       const unsigned char* masks, const float* d_logits, int B, int H, int W, float* scratch,
                                       float* d_params, float* d_x, void* stream) {
    Dims d;
    NF_CNN_CHECKS(B, d, "packed, x, workspace, masks, d_logits, scratch or d_params", packed, x, workspace, masks, d_logits, scratch,
                  d_params);
    const PackLayout L = pack_layout(num_classes);
    const GradLayout G = grad_layout(num_classes);
    const DwScratch S = dw_scratch(d, B);
    hipStream_t st = as_stream(stream);
    const FwdView v = fwd_view(workspace, masks, d, B);
    float* gpool[kStages];
    for (int s = 0; s < kStages; ++s) gpool[s] = scratch + S.gpool[s];
    float* dh = scratch + S.dh;
    float* part = scratch + S.part;

    int rc = bwd_data_chain(packed, nullptr, num_classes, v, d_logits, B, B, d, gpool, d_x, st);
    if (rc) return rc;

    // ---- FC head
    fc_dh_kernel<<<dim3(B), dim3(kHidden), 0, st>>>(d_logits, v.hidden, packed + L.w2, num_classes, dh);
    NF_LAUNCHED("cnn_fc_dh");
    const size_t nfc = (size_t)kHidden * kFlat + kHidden + (size_t)num_classes * kHidden + num_classes;
    fc_dw_kernel<<<dim3((unsigned)((nfc + 255) / 256)), dim3(256), 0, st>>>(d_logits, v.hidden, dh, v.acts[6], B, num_classes,
                                                                           d_params + G.w[7], d_params + G.b[7],
                                                                           d_params + G.w[8], d_params + G.b[8]);
    NF_LAUNCHED("cnn_fc_dw");

    // ---- conv stages: partial slabs, then their fixed-order sum (the slab region is reused, stream order keeps it safe)
    for (int s = 0; s < kStages; ++s) {
        const DwPlan pl = dw_plan(d, s, B);
        DwArgs a = {};
        a.in = s == 0 ? x : v.acts[s - 1];
        a.gp = gpool[s];
        a.act = v.acts[s];
        a.gmask = v.mks[s];
        a.part = part;
        a.hin = d.hin[s];
        a.win = d.win[s];
        a.hp = d.hin[s + 1];
        a.wp = d.win[s + 1];
        a.ntx = pl.ntx;
        a.nty = pl.nty;
        a.ntiles = pl.ntiles;
        a.tps = pl.tps;
        rc = conv_dw_stage(s, a, pl, st);
        if (rc) return rc;
        rc = reduce_slabs(part, pl.slabs, pl.out, stage_cin(s), s == 0 ? 2 : 1, d_params + G.w[s], st);
        if (rc) return rc;
        rc = db_stage(s, gpool[s], v.acts[s], part, (size_t)B * a.hp * a.wp, pl, st);
        if (rc) return rc;
        rc = reduce_slabs(part, pl.db_slabs, stage_cout(s), 0, 0, d_params + G.b[s], st);
        if (rc) return rc;
    }
    return 0;
}
