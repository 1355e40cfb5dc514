// The MyCNN victim's conv stages 2..7 on the bf16 matrix cores ("bf16x3"): forward and backward-data with every f32 product
// computed as six bf16 products, f32-accurate, opt-in (MyCNN(precision='bf16x3')). Stage 1, the FC head and every weight
// gradient stay on the exact kernels of cnn.hip, called as they are.
//
// Arithmetic. Both operands are split by round-to-nearest into three bf16 pieces (bf16_split.h): x = x0 + x1 + x2 with
// |x1| <= 2^-8 |x|, |x2| <= 2^-16 |x|, each difference exact in f32 (nothing is left over while the pieces are normal). Of the
// nine piece products the six a1b1, a0b2, a2b0, a0b1, a1b0, a0b0 are kept and issued in that order (smallest first) into the
// ONE f32 accumulator of an output element, k16 step after k16 step (tap-major inside a 16-channel slice, slices in ascending
// order): a bf16 x bf16 product is exact in f32, and what is dropped (a1b2 + a2b1 + a2b2) is at most 2^-23 |a||b| per product
// in the worst case (both operands at a rounding tie twice) and about 2^-26 |a||b| on average: below the f32 rounding of the sum.
// No float atomics, every output is written by one lane, two runs give the same bits. bf16 has the f32 exponent range: no
// pre-scale. A NaN operand is NaN in all three pieces, so NaN shows where the exact kernel shows it; +-Inf (and a finite
// value that rounds to a bf16 Inf, |x| >= 2^128 (1 - 2^-9)) becomes NaN, because Inf - Inf happens in the split.
//
// Kernel: an implicit GEMM on v_mfma_f32_32x32x16_bf16 over the workgroup tile of cnn_tile.h, which it shares with the exact
// conv_stage_kernel (cnn.hip): the tile geometry and origin, the A-row map, the accumulator-register-to-row map and the epilogue
// on it (ReLU, 2 x 2 pool, first-maximum / NaN-wins argmax code, mask byte), the gate of the un-pooled gradient and the launch
// grid are the functions there, not copies. What is this file's own: the staging, the LDS layout, the k-loop. A k16 step is the
// 16 channels of one tap of a 16-channel slice: lane half h holds channels 8h .. 8h+7, one ds_read_b128 per operand and plane.
//   * B operand: the bf16x3 image (nerfail_cnn_pack_x3, split ONCE on the device from the f32 image; layout in cnn_layout.h):
//     the [n-block][9 taps][3 planes][16 channels] block of a slice is contiguous there and is copied to LDS as it is.
//   * A operand: split WHILE it is staged, once per tile element and slice (forward: the input tile; backward: the gated
//     un-pooled gradient: gate() of cnn_tile.h, as stage_grad in cnn.hip), then read by 9 taps and NT n-tiles.
//   * Staging: single-buffered LDS behind two barriers per slice, with the global loads of slice c + 1 (A and B, raw, in
//     registers) issued before the MFMAs of slice c: the L2 latency lies under 216 MFMAs, what stays exposed per slice is the
//     split (VALU) and the LDS writes. LDS: A 18 x 18 (10 x 34) pixels x 112 bytes (3 planes x 32 + 16 pad: an odd number of
//     16-byte slots per pixel), B 64 rows x 880 bytes (864 + 16 pad, odd as well: the 16 lanes of a ds_read_b128 group fall on
//     16 different slots): 36 288 (38 080) + 56 320 bytes, one workgroup per CU, one wave per SIMD.
#include "common.h"
#include "cnn_tile.h"
#include "bf16_split.h"

namespace nerfail {
namespace cnn {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kX3PixBytes = 112;                                // LDS bytes of one A pixel: [3 planes][16 bf16] + 16
constexpr int kX3RowBytes = kX3RowSlots * 16 + 16;              // LDS bytes of one B row: [9 taps][3 planes][16 bf16] + 16

// 8 f32 -> the three bf16 planes (4 dwords each)
__device__ __forceinline__ void split8(const float (&x)[8], u32x4& hi, u32x4& mid, u32x4& lo) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float a = x[2 * k], b = x[2 * k + 1];
        hi[k] = cvt_bf2(a, b);
        sub_bf2(a, b, hi[k]);
        mid[k] = cvt_bf2(a, b);
        sub_bf2(a, b, mid[k]);
        lo[k] = cvt_bf2(a, b);
    }
}

// ---------------------------------------------------------------------------------------------------------------- pack
// One thread per (slice cb, row n, tap t, channel half): src is the f32 image of the stage and direction, [NC][9][KC].
__global__ void pack_x3_conv_kernel(const float* __restrict__ src, u32x4* __restrict__ dst, int NC, int KC) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NC * 9 * (KC / 8)) return;
    const int hf = i & 1, t = (i >> 1) % 9, n = ((i >> 1) / 9) % NC, cb = (i >> 1) / (9 * NC);
    const float* p = src + ((size_t)n * 9 + t) * KC + 16 * cb + 8 * hf;
    const float4 q0 = *reinterpret_cast<const float4*>(p), q1 = *reinterpret_cast<const float4*>(p + 4);
    const float x[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
    u32x4 hi, mid, lo;
    split8(x, hi, mid, lo);
    u32x4* o = dst + (((size_t)cb * NC + n) * 9 + t) * 6 + hf;   // [plane][2 halves] of 16 bytes
    o[0] = hi;
    o[2] = mid;
    o[4] = lo;
}

// ---------------------------------------------------------------------------------------------------------------- conv stage
// MODE 0: forward (stages 2..7, NHWC input).  MODE 2: backward-data (cnn_tile.h). KC: channels of the K dimension (forward: Cin,
// backward: Cout), NC: of the N dimension, NT: 32-wide n-tiles per wave (conv_nt); the slice is 16 channels.
template <int MODE, int KC, int NC, int NT>
struct StageX3 {
    static constexpr int TH = Geo<MODE>::TH, TW = Geo<MODE>::TW;
    static constexpr int AITEMS = TH * TW * 2;                  // (pixel, channel half) items of the A tile
    static constexpr int AIT = (AITEMS + 255) / 256;
    static constexpr int BUNITS = NT * 32 * kX3RowSlots;        // 16-byte units of the B tile
    static constexpr int BIT = (BUNITS + 255) / 256;
    static constexpr int XBYTES = TH * TW * kX3PixBytes, WBYTES = NT * 32 * kX3RowBytes;

    // what one thread holds of the next slice between its global loads and its LDS writes
    struct Regs {
        float4 v[AIT][2];                                       // forward: the input; backward: d pooled output
        float4 act[MODE == 2 ? AIT : 1][2];                     // backward: pooled output
        u32x2 mk[MODE == 2 ? AIT : 1];                          // backward: argmax codes of the 8 channels
        u32x4 w[BIT];
    };

    // pixel p of the tile -> is it inside, and where (forward: input pixel; backward: pooled cell and window position)
    static __device__ __forceinline__ void load(Regs& r, const ConvArgs& a, const u32x4* __restrict__ wimg, int tid, int g, int b,
                                                int gy0, int gx0, int n0, int cb) {
#pragma unroll
        for (int it = 0; it < AIT; ++it) {
            const int idx = tid + 256 * it;
            const int hf = idx & 1, p = idx >> 1;
            const int ch = 16 * cb + 8 * hf;
            r.v[it][0] = r.v[it][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (MODE == 2) {
                r.act[it][0] = r.act[it][1] = make_float4(0.f, 0.f, 0.f, 0.f);
                r.mk[it] = (u32x2){0u, 0u};
            }
            if (idx < AITEMS) {
                if (MODE == 0) {
                    const int gy = gy0 + p / TW, gx = gx0 + p % TW;
                    if (gy < a.hin && gx < a.win) {
                        const float* src = a.in + (((size_t)b * a.hin + gy) * a.win + gx) * KC + ch;
                        r.v[it][0] = *reinterpret_cast<const float4*>(src);
                        r.v[it][1] = *reinterpret_cast<const float4*>(src + 4);
                    }
                } else {
                    const int oy = gy0 + p / TW, ox = gx0 + p % TW;
                    if (oy >= 0 && ox >= 0 && oy < 2 * a.hp && ox < 2 * a.wp) {
                        const int pr = oy >> 1, pc = ox >> 1;
                        const size_t cell = ((size_t)b * a.hp + pr) * a.wp + pc, gcell = ((size_t)g * a.hp + pr) * a.wp + pc;
                        const float* gs = a.gp + gcell * KC + ch;
                        const float* as = a.act + cell * KC + ch;
                        r.v[it][0] = *reinterpret_cast<const float4*>(gs);
                        r.v[it][1] = *reinterpret_cast<const float4*>(gs + 4);
                        r.act[it][0] = *reinterpret_cast<const float4*>(as);
                        r.act[it][1] = *reinterpret_cast<const float4*>(as + 4);
                        r.mk[it] = *reinterpret_cast<const u32x2*>(gmask_addr(a.gmask, b, a.hp, npc8(a.wp), pr, pc, KC, ch));
                    }
                }
            }
        }
        const u32x4* wsrc = wimg + ((size_t)cb * NC + n0) * kX3RowSlots;
#pragma unroll
        for (int it = 0; it < BIT; ++it) {
            const int u = tid + 256 * it;
            r.w[it] = (u32x4){0u, 0u, 0u, 0u};
            if (u < BUNITS) r.w[it] = wsrc[u];
        }
    }

    static __device__ __forceinline__ void store(const Regs& r, const ConvArgs& a, char* xs, char* ws, int tid, int gy0, int gx0) {
#pragma unroll
        for (int it = 0; it < AIT; ++it) {
            const int idx = tid + 256 * it;
            const int hf = idx & 1, p = idx >> 1;
            float x[8] = {r.v[it][0].x, r.v[it][0].y, r.v[it][0].z, r.v[it][0].w, r.v[it][1].x, r.v[it][1].y, r.v[it][1].z, r.v[it][1].w};
            if (MODE == 2) {
                const int oy = gy0 + p / TW, ox = gx0 + p % TW;
                const unsigned q = (unsigned)(((oy & 1) << 1) | (ox & 1));
                const int sh = gate_shift(ox >> 1);
                const float av[8] = {r.act[it][0].x, r.act[it][0].y, r.act[it][0].z, r.act[it][0].w,
                                     r.act[it][1].x, r.act[it][1].y, r.act[it][1].z, r.act[it][1].w};
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = gate(x[j], av[j], r.mk[it][j >> 2], 8 * (j & 3) + sh, q);
            }
            u32x4 hi, mid, lo;
            split8(x, hi, mid, lo);
            if (idx < AITEMS) {
                u32x4* o = reinterpret_cast<u32x4*>(xs + p * kX3PixBytes + hf * 16);
                o[0] = hi;
                o[2] = mid;
                o[4] = lo;
            }
        }
#pragma unroll
        for (int it = 0; it < BIT; ++it) {
            const int u = tid + 256 * it;
            if (u < BUNITS) *reinterpret_cast<u32x4*>(ws + (u / kX3RowSlots) * kX3RowBytes + (u % kX3RowSlots) * 16) = r.w[it];
        }
    }
};

__device__ __forceinline__ void mfma_bf(f32x16& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

template <int MODE, int KC, int NC, int NT>
__global__ __launch_bounds__(256) void conv_x3_kernel(ConvArgs a, const u32x4* __restrict__ wimg) {
    typedef StageX3<MODE, KC, NC, NT> S;
    constexpr int TW = S::TW;
    static_assert(KC % 16 == 0 && NC % (NT * 32) == 0, "channel chunking");
    __shared__ __attribute__((aligned(16))) char xs[S::XBYTES];
    __shared__ __attribute__((aligned(16))) char ws[S::WBYTES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = lane & 31, h = lane >> 5;
    const int g = blockIdx.z, b = MODE == 2 ? g % a.B : g;
    const int n0 = blockIdx.y * NT * 32;
    int ty0, tx0, gy0, gx0;
    tile_origin<MODE>(a, ty0, tx0, gy0, gx0);
    int abase[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) abase[mt] = a_row_pixel<MODE>(wave, n, mt);

    f32x16 acc[2][NT];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[mt][nt][i] = 0.f;

    typename S::Regs regs;
    S::load(regs, a, wimg, tid, g, b, gy0, gx0, n0, 0);
#pragma unroll 1
    for (int cb = 0; cb < KC / 16; ++cb) {
        __syncthreads();                                        // the MFMAs of the slice before have read their operands
        S::store(regs, a, xs, ws, tid, gy0, gx0);
        __syncthreads();
        if (cb + 1 < KC / 16) S::load(regs, a, wimg, tid, g, b, gy0, gx0, n0, cb + 1);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int tofs = tap_ofs(MODE, t, TW);
            u32x4 av[2][3], bv[NT][3];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    av[mt][p] = *reinterpret_cast<const u32x4*>(xs + (abase[mt] + tofs) * kX3PixBytes + p * 32 + h * 16);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    bv[nt][p] = *reinterpret_cast<const u32x4*>(ws + (nt * 32 + n) * kX3RowBytes + (t * 3 + p) * 32 + h * 16);
            // a1b1, a0b2, a2b0, a0b1, a1b0, a0b0: smallest first, the (m-tile, n-tile) pairs interleaved
            constexpr int PA[6] = {1, 0, 2, 0, 1, 0}, PB[6] = {1, 2, 0, 1, 0, 0};
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) mfma_bf(acc[mt][nt], av[mt][PA[k]], bv[nt][PB[k]]);
        }
    }

    epilogue<MODE, NC, NT>(acc, a, g, b, n0, ty0, tx0, wave, n, h);
}

template <int MODE, int KC, int NC, int NT>
static int launch_x3(const ConvArgs& a, const void* img, int Z, hipStream_t st, const char* name) {
    conv_x3_kernel<MODE, KC, NC, NT><<<conv_grid<MODE, NC, NT>(a, Z), dim3(256), 0, st>>>(a, static_cast<const u32x4*>(img));
    NF_LAUNCHED(name);
    return 0;
}

// s = 1..6 (stages 2..7): stage 1 has no bf16x3 kernel
#define NF_X3_STAGE_CHECKS NF_REQUIRE(s >= 1 && s < kStages && x3 != nullptr, "stage index outside 1..6, or the bf16x3 image is NULL")

int conv_fwd_stage_x3(int s, const ConvArgs& a, const void* x3, int B, hipStream_t st) {
    static const char* const name[kStages] = NF_STAGE_LABELS("cnn_x3_conv_fwd");
    NF_X3_STAGE_CHECKS;
    const void* img = static_cast<const char*>(x3) + x3_layout().fwd[s];
    return dispatch_stage(s, [&](auto S) {
        if constexpr (S == 0) return NERFAIL_EINVAL;
        else return launch_x3<0, stage_cin(S), stage_cout(S), conv_nt(stage_cout(S))>(a, img, B, st, name[S]);
    });
}

int conv_bwd_stage_x3(int s, const ConvArgs& a, const void* x3, int Z, hipStream_t st) {   // KC = Cout, NC = Cin
    static const char* const name[kStages] = NF_STAGE_LABELS("cnn_x3_conv_bwd");
    NF_X3_STAGE_CHECKS;
    const void* img = static_cast<const char*>(x3) + x3_layout().bwd[s];
    return dispatch_stage(s, [&](auto S) {
        if constexpr (S == 0) return NERFAIL_EINVAL;
        else return launch_x3<2, stage_cout(S), stage_cin(S), conv_nt(stage_cin(S))>(a, img, Z, st, name[S]);
    });
}

}  // namespace cnn
}  // namespace nerfail

using namespace nerfail;
using namespace nerfail::cnn;

extern "C" int nerfail_cnn_x3_revision(void) { return 1; }

extern "C" size_t nerfail_cnn_x3_packed_bytes(int num_classes) {
    if (num_classes < 1 || num_classes > 4096) return 0;
    return x3_layout().total;
}

extern "C" int nerfail_cnn_pack_x3(const float* packed, int num_classes, void* packed_x3, void* stream) {
    NF_REQUIRE(num_classes >= 1 && num_classes <= 4096, "num_classes must be in 1..4096");
    NF_REQUIRE(packed != nullptr && packed_x3 != nullptr, "packed or packed_x3 is NULL");
    const PackLayout L = pack_layout(num_classes);
    const X3Layout X = x3_layout();
    hipStream_t st = as_stream(stream);
    for (int s = 1; s < kStages; ++s) {
        const int co = stage_cout(s), ci = stage_cin(s), n = co * ci * 9 / 8;
        pack_x3_conv_kernel<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(
            packed + L.fwd[s], reinterpret_cast<u32x4*>(static_cast<char*>(packed_x3) + X.fwd[s]), co, ci);
        NF_LAUNCHED("cnn_pack_x3");
        pack_x3_conv_kernel<<<dim3((n + 255) / 256), dim3(256), 0, st>>>(
            packed + L.bwd[s], reinterpret_cast<u32x4*>(static_cast<char*>(packed_x3) + X.bwd[s]), ci, co);
        NF_LAUNCHED("cnn_pack_x3");
    }
    return 0;
}
