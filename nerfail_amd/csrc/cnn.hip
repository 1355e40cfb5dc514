// The MyCNN victim classifier (model/MyModel.py:5-52): seven stages of 3x3 valid conv + bias + ReLU + 2x2 floor max-pool,
// 3-32-64-128-256-256-128-64 channels, then fc1 1024->512 + ReLU + fc2 512->C. Forward and the gradient with respect to the
// input (weights frozen) on gfx950.
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
//
// Multi-RHS backward (nerfail_cnn_bwd_data_multi): R gradients of ONE forward. The backward kernels run one grid slice per
// (r, b): slice g = r * B + b indexes every gradient buffer (d logits, gp, out, d x), image b = g % B indexes what the
// forward kept (act, gmask, hidden). R = 1 is the single backward; the order of every sum does not depend on R.
#include "common.h"

namespace nerfail {
namespace cnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

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

static size_t act_floats(const Dims& d, int s, int B) { return (size_t)B * d.hin[s + 1] * d.win[s + 1] * stage_cout(s); }
static size_t mask_bytes_of(const Dims& d, int s, int B) { return (size_t)B * d.hin[s + 1] * npc8(d.win[s + 1]) * 2 * stage_cout(s); }

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
// MODE 0: forward, NHWC input.  MODE 1: forward, stage 1 (NCHW input, 3 channels padded to 4).  MODE 2: backward-data.
// KC: channels of the K dimension (forward: Cin, backward: Cout); NC: channels of the N dimension (forward: Cout, backward:
// Cin); NT: 32-wide n-tiles per wave; CC: K channels staged per LDS round.
// Workgroup: 4 waves, each 2 m-tiles x NT n-tiles. Forward: 8 x 8 pooled cells (wave w: pooled rows 2w, 2w+1; an m-tile is one
// pooled row of 8 cells = 2 x 16 conv pixels). Backward: 8 rows x 32 columns of stage-input pixels (an m-tile is 32 pixels of
// one row).
struct ConvArgs {
    const float* in;           // forward: stage input (NHWC, or NCHW for MODE 1)
    const float* w;            // weight image of this stage and direction
    const float* bias;         // forward
    float* out;                // forward: pooled NHWC; backward: d input NHWC
    unsigned char* mask;       // forward: argmax codes (NULL = inference)
    const float* gp;           // backward: d pooled output (NHWC)
    const float* act;          // backward: pooled output (NHWC)
    const unsigned char* gmask;// backward: argmax codes of the forward
    int hin, win, hp, wp;      // stage input and pooled output sizes
    int B;                     // backward: images of the forward (grid z = r * B + b covers the R right-hand sides)
};

template <int MODE>
struct Geo {
    static constexpr int TH = MODE == 2 ? 10 : 18;
    static constexpr int TW = MODE == 2 ? 34 : 18;
};

__device__ __forceinline__ int tap_ofs(int mode, int tap, int tw) {
    const int ky = tap / 3, kx = tap % 3;
    return mode == 2 ? -(ky * tw + kx) : ky * tw + kx;
}

// Stage one CC-channel slice of the un-pooled, ReLU-masked output gradient at conv positions (gy0 + r, gx0 + c) into LDS
// (row stride XS floats); positions outside [0, 2 hp) x [0, 2 wp) get 0 (rows and columns the floor pool dropped, halo).
// gp is read at gradient slice g, act and gmask at image b.
template <int KC, int CC, int TH, int TW, int XS>
__device__ __forceinline__ void stage_grad(float* xs, const float* __restrict__ gp, const float* __restrict__ act,
                                           const unsigned char* __restrict__ gmask, int g, int b, int hp, int wp, int gy0,
                                           int gx0, int c0) {
    const int n8 = npc8(wp);
    for (int idx = threadIdx.x; idx < TH * TW * (CC / 4); idx += 256) {
        const int q4 = idx % (CC / 4), p = idx / (CC / 4);
        const int oy = gy0 + p / TW, ox = gx0 + p % TW;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (oy >= 0 && ox >= 0 && oy < 2 * hp && ox < 2 * wp) {
            const int pr = oy >> 1, pc = ox >> 1, q = ((oy & 1) << 1) | (ox & 1);
            const size_t cell = ((size_t)b * hp + pr) * wp + pc, gcell = ((size_t)g * hp + pr) * wp + pc;
            const int ch = c0 + 4 * q4;
            const float4 gv = *reinterpret_cast<const float4*>(gp + gcell * KC + ch);
            const float4 av = *reinterpret_cast<const float4*>(act + cell * KC + ch);
            const unsigned mk = *reinterpret_cast<const unsigned*>(
                gmask + ((((size_t)b * hp + pr) * n8 + (pc >> 3)) * 2 + (pc & 1)) * KC + ch);
            const int sh = 2 * ((pc & 7) >> 1);
            v.x = (((mk >> sh) & 3u) == (unsigned)q && !(av.x <= 0.f)) ? gv.x : 0.f;
            v.y = (((mk >> (8 + sh)) & 3u) == (unsigned)q && !(av.y <= 0.f)) ? gv.y : 0.f;
            v.z = (((mk >> (16 + sh)) & 3u) == (unsigned)q && !(av.z <= 0.f)) ? gv.z : 0.f;
            v.w = (((mk >> (24 + sh)) & 3u) == (unsigned)q && !(av.w <= 0.f)) ? gv.w : 0.f;
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
    int ty0, tx0, gy0, gx0;                                     // tile origin: output units / LDS tile in global coordinates
    if (MODE == 2) {
        const int nx = (a.win + 31) / 32;
        ty0 = (blockIdx.x / nx) * 8;
        tx0 = (blockIdx.x % nx) * 32;
        gy0 = ty0 - 2;
        gx0 = tx0 - 2;
    } else {
        const int nx = (a.wp + 7) / 8;
        ty0 = (blockIdx.x / nx) * 8;                            // pooled
        tx0 = (blockIdx.x % nx) * 8;
        gy0 = 2 * ty0;
        gx0 = 2 * tx0;
    }
    // LDS pixel of this lane's A row for tap (0,0), per m-tile
    int abase[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        if (MODE == 2) {
            abase[mt] = (2 * wave + mt + 2) * TW + lane % 32 + 2;
        } else {
            const int cell = n >> 2, q = n & 3;
            abase[mt] = (2 * (2 * wave + mt) + (q >> 1)) * TW + 2 * cell + (q & 1);
        }
    }
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

    // ---- epilogue
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int co = n0 + nt * 32 + n;
            if (MODE == 2) {
                const int y = ty0 + 2 * wave + mt;
                if (y < a.hin) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int x = tx0 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        if (x < a.win) a.out[(((size_t)g * a.hin + y) * a.win + x) * NC + co] = acc[mt][nt][i];
                    }
                }
            } else {
                const int pr = ty0 + 2 * wave + mt;
                if (pr < a.hp) {
                    const float bias = a.bias[co];
                    unsigned code = 0;
#pragma unroll
                    for (int w4 = 0; w4 < 4; ++w4) {
                        float best = -INFINITY;
                        int bi = 0;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {           // window position j = (dy, dx) row-major; ATen's rule: first max, NaN wins
                            float v = acc[mt][nt][4 * w4 + j] + bias;
                            v = v < 0.f ? 0.f : v;              // ReLU (NaN stays NaN)
                            if (v > best || __builtin_isnan(v)) {
                                best = v;
                                bi = j;
                            }
                        }
                        code |= (unsigned)bi << (2 * w4);
                        const int pc = tx0 + 2 * w4 + h;
                        if (pc < a.wp) a.out[(((size_t)b * a.hp + pr) * a.wp + pc) * NC + co] = best;
                    }
                    if (a.mask)
                        a.mask[((((size_t)b * a.hp + pr) * npc8(a.wp) + (tx0 >> 3)) * 2 + h) * NC + co] = (unsigned char)code;
                }
            }
        }
    }
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
    unsigned tiles;
    if (MODE == 2) tiles = (unsigned)(((a.win + 31) / 32) * ((a.hin + 7) / 8));
    else tiles = (unsigned)(((a.wp + 7) / 8) * ((a.hp + 7) / 8));
    conv_stage_kernel<MODE, KC, NC, NT, CC><<<dim3(tiles, NC / (NT * 32), Z), dim3(256), 0, st>>>(a);
    NF_LAUNCHED(name);
    return 0;
}

static int conv_fwd_stage(int s, const ConvArgs& a, int B, hipStream_t st) {
    switch (s) {
        case 0: return launch_conv<1, 4, 32, 1, 4>(a, B, st, "cnn_conv_fwd_s1");
        case 1: return launch_conv<0, 32, 64, 2, 16>(a, B, st, "cnn_conv_fwd_s2");
        case 2: return launch_conv<0, 64, 128, 2, 16>(a, B, st, "cnn_conv_fwd_s3");
        case 3: return launch_conv<0, 128, 256, 2, 16>(a, B, st, "cnn_conv_fwd_s4");
        case 4: return launch_conv<0, 256, 256, 2, 16>(a, B, st, "cnn_conv_fwd_s5");
        case 5: return launch_conv<0, 256, 128, 2, 16>(a, B, st, "cnn_conv_fwd_s6");
        default: return launch_conv<0, 128, 64, 2, 16>(a, B, st, "cnn_conv_fwd_s7");
    }
}

static int conv_bwd_stage(int s, const ConvArgs& a, int Z, hipStream_t st) {   // s >= 1: KC = Cout, NC = Cin
    switch (s) {
        case 1: return launch_conv<2, 64, 32, 1, 16>(a, Z, st, "cnn_conv_bwd_s2");
        case 2: return launch_conv<2, 128, 64, 2, 16>(a, Z, st, "cnn_conv_bwd_s3");
        case 3: return launch_conv<2, 256, 128, 2, 16>(a, Z, st, "cnn_conv_bwd_s4");
        case 4: return launch_conv<2, 256, 256, 2, 16>(a, Z, st, "cnn_conv_bwd_s5");
        case 5: return launch_conv<2, 128, 256, 2, 16>(a, Z, st, "cnn_conv_bwd_s6");
        default: return launch_conv<2, 64, 128, 2, 16>(a, Z, st, "cnn_conv_bwd_s7");
    }
}

static size_t workspace_floats(const Dims& d, int B) {
    size_t n = 0;
    for (int s = 0; s < kStages; ++s) n += act_floats(d, s, B);
    return n + (size_t)B * kHidden;
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

extern "C" int nerfail_cnn_fwd(const float* packed, int num_classes, const float* x, int B, int H, int W, float* workspace,
                               unsigned char* masks, float* logits, void* stream) {
    Dims d;
    NF_REQUIRE(num_classes >= 1 && num_classes <= 4096, "num_classes must be in 1..4096");
    NF_REQUIRE(B >= 1 && B <= 65535, "B must be in 1..65535");
    NF_REQUIRE(dims_of(H, W, d), "unsupported H x W: the seventh stage must be 4 x 4 (fc1 takes 1024 inputs)");
    NF_REQUIRE(packed != nullptr && x != nullptr && workspace != nullptr && logits != nullptr,
               "packed, x, workspace or logits is NULL");
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
        int rc = conv_fwd_stage(s, a, B, st);
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

extern "C" size_t nerfail_cnn_bwd_multi_scratch_bytes(int R, int B, int H, int W) {
    Dims d;
    if (!multi_ok(R, B) || !dims_of(H, W, d)) return 0;
    return (act_floats(d, 0, R * B) + act_floats(d, 1, R * B)) * sizeof(float);
}

// The backward launch chain for R right-hand sides of one B-image forward (arguments already validated).
static int bwd_data_launch(const float* packed, int num_classes, const float* workspace, const unsigned char* masks,
                           const float* d_logits, int R, int B, int H, int W, const Dims& d, float* scratch, float* d_x,
                           void* stream) {
    const PackLayout L = pack_layout(num_classes);
    hipStream_t st = as_stream(stream);
    const int Z = R * B;                                         // gradient slices: the grid's z (FC head: x) dimension
    const float* acts[kStages];
    const unsigned char* mks[kStages];
    const float* p = workspace;
    const unsigned char* q = masks;
    for (int s = 0; s < kStages; ++s) {                          // what the forward kept: B images
        acts[s] = p;
        mks[s] = q;
        p += act_floats(d, s, B);
        q += mask_bytes_of(d, s, B);
    }
    float* bufs[2] = {scratch, scratch + act_floats(d, 0, Z)};   // [0] holds stage outputs 6, 4, 2, 0; [1] stage outputs 5, 3, 1
    fc_bwd_kernel<<<dim3(Z), dim3(kFlat), 0, st>>>(d_logits, p, packed + L.fc1P, packed + L.w2, num_classes, B, bufs[0]);
    NF_LAUNCHED("cnn_fc_bwd");
    for (int s = kStages - 1; s >= 1; --s) {
        ConvArgs a = {};
        a.w = packed + L.bwd[s];
        a.out = bufs[(s + 1) & 1];                // d (stage s input) = d (stage s-1 output)
        a.gp = bufs[s & 1];
        a.act = acts[s];
        a.gmask = mks[s];
        a.hin = d.hin[s];
        a.win = d.win[s];
        a.hp = d.hin[s + 1];
        a.wp = d.win[s + 1];
        a.B = B;
        int rc = conv_bwd_stage(s, a, Z, st);
        if (rc) return rc;
    }
    const unsigned tiles = (unsigned)(((W + 15) / 16) * ((H + 15) / 16));
    conv1_bwd_kernel<<<dim3(tiles, 1, Z), dim3(256), 0, st>>>(packed + L.w1raw, bufs[0], acts[0], mks[0], d_x, H, W, d.hin[1],
                                                             d.win[1], B);
    NF_LAUNCHED("cnn_conv1_bwd");
    return 0;
}

// The single backward is the R = 1 case: the same kernels, the same grid, the same bits.
extern "C" int nerfail_cnn_bwd_data(const float* packed, int num_classes, const float* workspace, const unsigned char* masks,
                                    const float* d_logits, int B, int H, int W, float* scratch, float* d_x, void* stream) {
    Dims d;
    NF_REQUIRE(num_classes >= 1 && num_classes <= 4096, "num_classes must be in 1..4096");
    NF_REQUIRE(B >= 1 && B <= 65535, "B must be in 1..65535");
    NF_REQUIRE(dims_of(H, W, d), "unsupported H x W: the seventh stage must be 4 x 4 (fc1 takes 1024 inputs)");
    NF_REQUIRE(packed != nullptr && workspace != nullptr && masks != nullptr && d_logits != nullptr && scratch != nullptr &&
                   d_x != nullptr, "packed, workspace, masks, d_logits, scratch or d_x is NULL");
    return bwd_data_launch(packed, num_classes, workspace, masks, d_logits, 1, B, H, W, d, scratch, d_x, stream);
}

extern "C" int nerfail_cnn_bwd_data_multi(const float* packed, int num_classes, const float* workspace, const unsigned char* masks,
                                          const float* d_logits, int R, int B, int H, int W, float* scratch, float* d_x,
                                          void* stream) {
    Dims d;
    NF_REQUIRE(num_classes >= 1 && num_classes <= 4096, "num_classes must be in 1..4096");
    NF_REQUIRE(multi_ok(R, B), "R and B must be >= 1 with R * B <= 65535 (one grid slice per right-hand side and image)");
    NF_REQUIRE(dims_of(H, W, d), "unsupported H x W: the seventh stage must be 4 x 4 (fc1 takes 1024 inputs)");
    NF_REQUIRE(packed != nullptr && workspace != nullptr && masks != nullptr && d_logits != nullptr && scratch != nullptr &&
                   d_x != nullptr, "packed, workspace, masks, d_logits, scratch or d_x is NULL");
    return bwd_data_launch(packed, num_classes, workspace, masks, d_logits, R, B, H, W, d, scratch, d_x, stream);
}
