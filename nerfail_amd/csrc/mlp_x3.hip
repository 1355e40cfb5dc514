// K3 + K4, inference form on the bf16 matrix cores: fused positional encoding + NeRF MLP forward with every f32 product
// computed as six bf16 products ("bf16x3"), f32-accurate (run_nerf.py:37-51, run_nerf_helpers.py:15-50, :100-123).
//
// Arithmetic. Every f32 operand is split by round-to-nearest into three bf16 pieces, x = x0 + x1 + x2 + r with
// |x1| <= 2^-9 |x|, |x2| <= 2^-18 |x|, |r| <= 2^-27 |x| (each difference is exact in f32). Of the nine piece products the
// six a1b1, a0b2, a2b0, a0b1, a1b0, a0b0 are kept, smallest first, into the one f32 accumulator: a bf16 x bf16 product
// is exact in f32, and what is dropped (a1b2 + a2b1 + a2b2 and the residuals) adds up to about 2^-26 |a||b|, below one
// f32 rounding. The result is f32-accurate, not bitwise that of the exact-f32 kernel (mlp_lds.hip) - any reordering of
// an f32 sum differs in the last bits as well. bf16 has the f32 exponent range: no pre-scale, no weight-range limit.
// Cost per 32x32x16 f32-equivalent: 6 v_mfma_f32_32x32x16_bf16 (6 x 32 cycles) against 8 v_mfma_f32_32x32x2_f32 (8 x 64).
//
// Structure: that of nerf_mlp_fwd_lds_kernel (mlp_lds.hip) - one wave per SIMD, 32 samples x all channels per wave, every
// layer transposed (the 32x32 accumulator tile of one layer is the B operand of the next), the weight stream shared by
// the 4 waves of a workgroup through an LDS-DMA ring with one barrier per group, running across layer boundaries; biases
// and the thin alpha / rgb heads in a constant LDS area (f32, computed exactly as there); encoding in the kernel.
//   * A operand: the bf16x3 image (nerfail_mlp_pack_x3, split ONCE on the device from the f32 image), laid out per layer as
//     [k16 step][out tile][plane][lane][8 bf16]: one 1 KB piece = the fragment of one (step, tile, plane).
//   * B operand: registers 8s'..8s'+7 of an accumulator tile are the k order of one 32x32x16 step (the pack puts the
//     weights in that order). The ReLU is applied lazily where an operand is consumed; each k16 chunk is split ONCE, one
//     step ahead, and serves all 8 out tiles (4 in the views layer).
//   * one "tile-step" = the 6 MFMAs of one (k16 step, out tile) with its 3 pieces; ring group = 8 tile-steps = 24 pieces,
//     4 groups in the ring (96 KB). Fragments are read two tile-steps ahead, so the group boundary sits at the group's
//     second-to-last tile-step (both remaining tile-steps' fragments are in registers when the slot is released).
#include "mlp_lds.h"

namespace nerfail {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const u32x4 lds_cu4;
typedef __attribute__((address_space(3))) const f32x2 lds_cf2;

struct X3Cfg {
    static constexpr int NT = 8;                 // W = 256 only
    static constexpr int GP = 24;                // pieces per ring group: 8 tile-steps x 3 planes
    static constexpr int S = 4;                  // groups in the ring
    static constexpr int RP = GP * S;            // ring pieces (96 KB)
    static constexpr int GPW = GP / 4;           // LDS-DMAs per wave and group
    static constexpr int SPG = GP / 3;           // tile-steps per group
    static constexpr int kSync = SPG - 2;        // position of the boundary tile-step inside its group
    static constexpr int kMaxDepth = 8;
    static constexpr int kAlphaFloats = (NT * 32 + 4 + kPiece - 1) / kPiece * kPiece;
    static constexpr int kRgbFloats = (3 * (NT / 2) * 32 + 4 + kPiece - 1) / kPiece * kPiece;
    static constexpr int kConstMax = (kMaxDepth + 2) * kPiece + kAlphaFloats + kRgbFloats;   // as LdsCfg<8> (mlp_lds.hip)
    static constexpr int kParkQuads = kEmbQuads + kDirQuads;
    static constexpr int kParkFloats = 4 * 64 * 4 * kParkQuads;
    static_assert((S - 2) * GPW <= 63, "vmcnt is a 6-bit counter");
    static_assert(GPW <= 8, "dma() covers 8 pieces per wave and group");
};

// x3 image offsets (in pieces) of every layer's stream part; false when the x3 kernel does not cover the shape
struct X3Layout {
    unsigned off[NERFAIL_MAX_DEPTH + 2];
    unsigned pieces;
};
static inline bool make_x3_layout(const MlpLayout& L, int W, X3Layout& X) {
    if (W != 256 || (L.D & 1) || L.D > X3Cfg::kMaxDepth) return false;
    unsigned off = 0;
    for (int l = 0; l <= L.D + 1; ++l) {
        const unsigned OT = (l == L.D + 1) ? L.NT / 2 : L.NT;
        const unsigned quads = L.w_count[l] / (OT * kPiece);
        if (quads & 1) return false;
        X.off[l] = off;
        off += quads / 2 * OT * 3;
    }
    X.pieces = off;
    return off % X3Cfg::GP == 0;
}

// x = hi + mid + lo (+ |r| <= 2^-27 |x|) by round-to-nearest, two elements at a time (element 0 in the low half).
__device__ __forceinline__ unsigned cvt_bf2(float x0, float x1) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2){x0, x1}, bf16x2));
}
__device__ __forceinline__ void sub_bf2(float& x0, float& x1, unsigned p) {       // x -= the bf16 pair p, exact
    x0 -= __uint_as_float(p << 16);
    x1 -= __uint_as_float(p & 0xffff0000u);
}

// ---- the bf16x3 image from the f32 image: one thread per (layer step, tile, lane), 8 weights -> 3 x 16 bytes
struct X3PackArgs {
    MlpLayout L;
    X3Layout X;
};
__global__ void pack_x3_kernel(const float* __restrict__ packed, X3PackArgs p, u32x4* __restrict__ img) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long ts = g >> 6;                                        // tile-step in the stream
    const int lane = (int)(g & 63);
    if (ts * 3 >= p.X.pieces) return;
    int l = 0;
    while (l < p.L.D + 1 && ts * 3 >= p.X.off[l + 1]) ++l;
    const int OT = (l == p.L.D + 1) ? p.L.NT / 2 : p.L.NT;
    const long r = ts - p.X.off[l] / 3;
    const int s = (int)(r / OT), t = (int)(r % OT);
    const float* w = packed + p.L.w_off[l] + lane * 4;
    const f32x4 q0 = *reinterpret_cast<const f32x4*>(w + ((2 * s) * OT + t) * kPiece);
    const f32x4 q1 = *reinterpret_cast<const f32x4*>(w + ((2 * s + 1) * OT + t) * kPiece);
    float x[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
    u32x4 hi, mid, lo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float a = x[2 * k], b = x[2 * k + 1];
        hi[k] = cvt_bf2(a, b);
        sub_bf2(a, b, hi[k]);
        mid[k] = cvt_bf2(a, b);
        sub_bf2(a, b, mid[k]);
        lo[k] = cvt_bf2(a, b);
    }
    u32x4* o = img + (p.X.off[l] + (long)r * 3) * 64 + lane;
    o[0] = hi;
    o[64] = mid;
    o[128] = lo;
}

// ---- the weight ring of one workgroup (the x3 counterpart of WRing in mlp_lds.hip; every member but f1 / f2 is
// wave-uniform). Refill interval: the SPG tile-steps from one boundary tile-step (inclusive) to the next; DMA P of the
// interval is issued behind the first MFMA of its P-th tile-step (P < GPW), the boundary's own right after the barrier.
// Boundary i + 1 needs group i + 1 landed; its DMAs are older than the two younger groups' 2 * GPW -> vmcnt(2 * GPW).
struct X3Ring {
    using C = X3Cfg;
    __amdgpu_buffer_rsrc_t rsrc;     // the x3 image as a raw buffer (reads past its end return 0, never fault)
    int voff;                        // lane * 16
    float* ring;                     // LDS ring base
    const float* rl;                 // ring + lane * 4
    int total;                       // stream length in pieces (multiple of GP)
    int src, slot, rd, wave;         // next group's first source piece, its ring group, next ring piece to read
    u32x4 f1[3], f2[3];              // fragments of the next two tile-steps

    template <int I>
    __device__ __forceinline__ void dma_at() const {
        constexpr int B4 = I / 4;                                  // one base per block of 4 pieces (12-bit immediate)
        const int first = wave * C::GPW + 4 * B4;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)(ring + (slot * C::GP + first) * kPiece), 16, voff,
                                                 (src + first) * (kPiece * 4), (I % 4) * kPiece * 4, 0);
    }
    __device__ __forceinline__ void dma(int i) const {             // i is a constant after unrolling
        switch (i) {
            case 0: dma_at<0>(); break;   case 1: dma_at<1>(); break;   case 2: dma_at<2>(); break;   case 3: dma_at<3>(); break;
            case 4: dma_at<4>(); break;   case 5: dma_at<5>(); break;   case 6: dma_at<6>(); break;   case 7: dma_at<7>(); break;
            default: break;
        }
    }
    __device__ __forceinline__ void group_issued() {
        src += C::GP;
        if (src >= total) src = 0;
        slot = (slot + 1 == C::S) ? 0 : slot + 1;
    }
    __device__ __forceinline__ void boundary() const {
        lds_wait_vmcnt<(C::S - 2) * C::GPW>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    __device__ __forceinline__ u32x4 frag(int p) const { return *(lds_cu4*)(rl + (rd + p) * kPiece); }
    __device__ __forceinline__ void advance() {
        rd += 3;
        if (rd >= C::RP) rd = 0;
    }
    // S-1 groups issued, group 0 readable; then the state right behind a boundary tile-step that sat two tile-steps before
    // the stream's first: DMAs 0 and 1 of group S-1 issued, the fragments of tile-steps 0 and 1 read
    __device__ __forceinline__ void start() {
#pragma unroll
        for (int g = 0; g < C::S - 1; ++g) {
#pragma unroll
            for (int i = 0; i < C::GPW; ++i) dma(i);
            group_issued();
        }
        boundary();
        dma(0);
        dma(1);
#pragma unroll
        for (int p = 0; p < 3; ++p) f1[p] = frag(p);
        advance();
#pragma unroll
        for (int p = 0; p < 3; ++p) f2[p] = frag(p);
        advance();
    }
};

__device__ __forceinline__ void mfma_x3(f32x16& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// One tile-step at stream position POS (mod SPG, a constant after unrolling): the six MFMAs of out tile `acc`, smallest
// product first, each with ONE piece of side work in its shadow: MFMA 0 the refill DMA, MFMAs 1..3 a fragment read of the
// tile-step two ahead, side(k) behind MFMA k (operand preparation, bias tiles).
template <class Side>
__device__ __forceinline__ void x3_step(X3Ring& st, const int POS, f32x16& acc, const u32x4 (&b)[3], Side side) {
    using C = X3Cfg;
    const int P = (POS - C::kSync + C::SPG) % C::SPG;              // position in the refill interval
    u32x4 a[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) { a[p] = st.f1[p]; st.f1[p] = st.f2[p]; }
    if (P == 0) st.boundary();
    __builtin_amdgcn_sched_barrier(0);
    mfma_x3(acc, a[1], b[1]);
    __builtin_amdgcn_sched_barrier(0);
    if (P < C::GPW) st.dma(P);
    side(0);
    __builtin_amdgcn_sched_barrier(0);
    mfma_x3(acc, a[0], b[2]);
    __builtin_amdgcn_sched_barrier(0);
    st.f2[1] = st.frag(1);
    side(1);
    __builtin_amdgcn_sched_barrier(0);
    mfma_x3(acc, a[2], b[0]);
    __builtin_amdgcn_sched_barrier(0);
    st.f2[0] = st.frag(0);
    side(2);
    __builtin_amdgcn_sched_barrier(0);
    mfma_x3(acc, a[0], b[1]);
    __builtin_amdgcn_sched_barrier(0);
    st.f2[2] = st.frag(2);
    st.advance();
    side(3);
    __builtin_amdgcn_sched_barrier(0);
    mfma_x3(acc, a[1], b[0]);
    __builtin_amdgcn_sched_barrier(0);
    side(4);
    __builtin_amdgcn_sched_barrier(0);
    mfma_x3(acc, a[0], b[0]);
    __builtin_amdgcn_sched_barrier(0);
    side(5);
    if (P == C::SPG - 1) st.group_issued();
    __builtin_amdgcn_sched_barrier(0);
}

// One part of a layer: NS k16 steps over OT out tiles (NS * OT a whole number of ring groups, so every part starts at
// stream position 0 mod SPG). bsrc(s, p, x): elements 2p, 2p+1 of step s's B operand as f32 (lazy ReLU / parked encoding).
// Step s+1's operand is split during step s: pair p behind MFMAs 1, 3, 4, 5 of tile-step p (load; hi; mid; lo). Step 0's
// cannot be early (its source is the layer before). hook(s, t): behind MFMA 2 of tile-step t of step s.
template <int OT, int NS, class BSrc, class Hook>
__device__ __forceinline__ void x3_part(X3Ring& st, f32x16 (&out)[X3Cfg::NT], BSrc bsrc, Hook hook) {
    static_assert((NS * OT) % X3Cfg::SPG == 0 && OT >= 4, "a part is a whole number of ring groups; 4 pairs per step");
    u32x4 b[3];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        float x[2];
        bsrc(0, p, x);
        b[0][p] = cvt_bf2(x[0], x[1]);
        sub_bf2(x[0], x[1], b[0][p]);
        b[1][p] = cvt_bf2(x[0], x[1]);
        sub_bf2(x[0], x[1], b[1][p]);
        b[2][p] = cvt_bf2(x[0], x[1]);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        u32x4 bn[3];
        float xs[4][2];
#pragma unroll
        for (int t = 0; t < OT; ++t) {
            auto side = [&](int k) {
                if (s + 1 < NS && t < 4) {
                    if (k == 1) bsrc(s + 1, t, xs[t]);
                    if (k == 3) { bn[0][t] = cvt_bf2(xs[t][0], xs[t][1]); sub_bf2(xs[t][0], xs[t][1], bn[0][t]); }
                    if (k == 4) { bn[1][t] = cvt_bf2(xs[t][0], xs[t][1]); sub_bf2(xs[t][0], xs[t][1], bn[1][t]); }
                    if (k == 5) bn[2][t] = cvt_bf2(xs[t][0], xs[t][1]);
                }
                if (k == 2) hook(s, t);
            };
            x3_step(st, (s * OT + t) % X3Cfg::SPG, out[t], b, side);
        }
        if (s + 1 < NS) {
#pragma unroll
            for (int p = 0; p < 3; ++p) b[p] = bn[p];
        }
    }
}

template <int NT, int SKIP>
__global__ __launch_bounds__(256, 1) void nerf_mlp_fwd_x3_kernel(MlpArgs a, const void* img, int img_pieces) {
    static_assert(NT == X3Cfg::NT, "W = 256 only");
    using C = X3Cfg;
    constexpr int OTV = NT / 2;
    // ONE object (see nerf_mlp_fwd_lds_kernel): ring first, then constants, then the parked encoding operands
    __shared__ __attribute__((aligned(16))) float smem[C::RP * kPiece + C::kConstMax + C::kParkFloats];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, j = lane & 31;
    const MlpLayout& L = a.lay;
    float* const ring0 = smem;
    float* const cst = smem + C::RP * kPiece;
    float* const park = cst + C::kConstMax + wave * (64 * 4 * C::kParkQuads) + lane * 4;
    {   // constant area: biases (one piece per layer), alpha head, rgb head - from the f32 image
        const int n = (int)(L.total - L.b_off[0]);
        const float* __restrict__ g = a.packed + L.b_off[0];
        for (int i = tid * 4; i < n; i += 1024) *reinterpret_cast<f32x4*>(cst + i) = *reinterpret_cast<const f32x4*>(g + i);
    }
    __syncthreads();
    const float* const c_alpha = cst + (L.alpha_off - L.b_off[0]);
    const float* const c_rgb = cst + (L.rgb_off - L.b_off[0]);

    X3Ring st;
    st.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(img), 0, img_pieces * (kPiece * 4), 0x00020000);
    st.voff = lane * 16; st.ring = ring0; st.rl = ring0 + lane * 4;
    st.total = img_pieces; st.src = 0; st.slot = 0; st.rd = 0; st.wave = wave;
    st.start();

    f32x16 P[NT], Q[NT];
    auto bias_tile = [&](f32x16 (&dst)[NT], int l, int t) {             // dst[t] = bias of layer l, tile t (f32, in AGPRs)
        const float* p = cst + l * kPiece + (t * 2 + h) * 16;
        const f32x4 v0 = lds_read4(p), v1 = lds_read4(p + 4), v2 = lds_read4(p + 8), v3 = lds_read4(p + 12);
        dst[t] = (f32x16){v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3],
                          v2[0], v2[1], v2[2], v2[3], v3[0], v3[1], v3[2], v3[3]};
        asm volatile("" : "+a"(dst[t]));
    };
#pragma unroll
    for (int t = 0; t < NT; ++t) bias_tile(P, 0, t);                    // later rounds: written during the views layer

    const int ntiles = (int)((a.M + 31) / 32);
    const int nrounds = (int)((ntiles + (long)gridDim.x * 4 - 1) / ((long)gridDim.x * 4));
    for (int rnd = 0; rnd < nrounds; ++rnd) {
        // every wave walks the whole stream every round; one without a tile of its own recomputes the last tile, stores nothing
        const int tile_own = (int)(((long)rnd * gridDim.x + blockIdx.x) * 4 + wave);
        const int tile = tile_own < ntiles ? tile_own : ntiles - 1;
        int jj = j;
        asm volatile("" : "+v"(jj));
        const long sraw = (long)tile * 32 + jj;
        const long s = sraw < a.M ? sraw : a.M - 1;
        {
            float emb[4 * kEmbQuads], demb[4 * kDirQuads];
            int hh = h;
            asm volatile("" : "+v"(hh));
            encode_sample(a, s, hh, emb, demb);
#pragma unroll
            for (int k = 0; k < kEmbQuads; ++k)
                *reinterpret_cast<f32x4*>(park + k * 256) = (f32x4){emb[4 * k], emb[4 * k + 1], emb[4 * k + 2], emb[4 * k + 3]};
#pragma unroll
            for (int k = 0; k < kDirQuads; ++k)
                *reinterpret_cast<f32x4*>(park + (kEmbQuads + k) * 256) =
                    (f32x4){demb[4 * k], demb[4 * k + 1], demb[4 * k + 2], demb[4 * k + 3]};
        }
        // k16 step s of a parked encoding: parked quads 2s, 2s+1 (f32 k-steps 8s .. 8s+7)
        auto b_park = [&](int q0) {
            return [=](int s, int p, float (&x)[2]) {
                const f32x2 v = *(lds_cf2*)(park + (q0 + 2 * s + (p >> 1)) * 256 + 2 * (p & 1));
                x[0] = v[0];
                x[1] = v[1];
            };
        };
        auto no_hook = [](int, int) {};
        // layer 0: 63 -> W into P (its bias is already there); Q (dead) receives the bias of layer 1 meanwhile
        x3_part<NT, kEmbQuads / 2>(st, P, b_park(0), [&](int s, int t) { if (t == 4 || t == 6) bias_tile(Q, 1, 2 * s + (t - 4) / 2); });

        float alpha = 0.f;
        auto layer = [&](f32x16 (&in)[NT], f32x16 (&out)[NT], int l, bool may_skip, bool may_be_last) __attribute__((always_inline)) {
            if (may_be_last && l == L.D) alpha = lds_head<NT>(in, c_alpha, h) + c_alpha[NT * 32];   // alpha_linear on relu(h)
            if (may_skip && l == L.skip + 1) x3_part<NT, kEmbQuads / 2>(st, out, b_park(0), no_hook);   // cat([input_pts, h])
            // input tile k is last read by the split of step 2k+1 (during step 2k): dead from step 2k+2 on
            x3_part<NT, 2 * NT>(st, out,
                [&](int s, int p, float (&x)[2]) {
                    x[0] = relu_bits(in[s >> 1][8 * (s & 1) + 2 * p]);
                    x[1] = relu_bits(in[s >> 1][8 * (s & 1) + 2 * p + 1]);
                },
                [&](int s, int t) { if (t == 4 && (s & 1) == 0 && s > 0) bias_tile(in, l + 1, s / 2 - 1); });
            bias_tile(in, l + 1, NT - 1);
        };
#pragma unroll 1
        for (int l = 1; l < L.D; l += 2) {                                  // D is even (host check): whole pairs
            layer(P, Q, l, SKIP == 1, false);
            layer(Q, P, l + 1, SKIP == 2, true);
        }
        // views_linears[0]: cat([feature, embedded dirs]) -> W/2 into Q's first tiles (no activation on the feature);
        // P receives the bias of the NEXT tile's layer 0 as its tiles die
        x3_part<OTV, 2 * NT>(st, Q,
            [&](int s, int p, float (&x)[2]) {
                x[0] = P[s >> 1][8 * (s & 1) + 2 * p];
                x[1] = P[s >> 1][8 * (s & 1) + 2 * p + 1];
            },
            [&](int s, int t) { if (t == 3 && (s & 1) == 0 && s > 0) bias_tile(P, 0, s / 2 - 1); });
        bias_tile(P, 0, NT - 1);
        x3_part<OTV, kDirQuads / 2>(st, Q, b_park(kEmbQuads), no_hook);
        float rgb[3];                                                       // rgb_linear: W/2 -> 3
        lds_head3<OTV>(Q, c_rgb, OTV * 32, h, rgb);
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[c] += c_rgb[3 * OTV * 32 + c];
        int je = j;
        asm volatile("" : "+v"(je));
        const long sout = (long)tile * 32 + je;
        if (h == 0 && sout < a.M && tile_own < ntiles)
            reinterpret_cast<float4*>(a.raw)[sout] = make_float4(rgb[0], rgb[1], rgb[2], alpha);
    }
    lds_wait_vmcnt<0>();       // no LDS-DMA may be in flight when the workgroup's LDS is released
}

bool mlp_x3_covers(const MlpLayout& L, int W) {
    X3Layout X;
    return make_x3_layout(L, W, X) && L.total - L.b_off[0] <= (unsigned)X3Cfg::kConstMax;
}

size_t mlp_x3_bytes(const MlpLayout& L, int W) {
    X3Layout X;
    return mlp_x3_covers(L, W) && make_x3_layout(L, W, X) ? (size_t)X.pieces * kPiece * 4 : 0;
}

int pack_mlp_x3(const float* packed, const MlpLayout& L, int W, void* out, hipStream_t s) {
    X3PackArgs p;
    p.L = L;
    if (!mlp_x3_covers(L, W) || !make_x3_layout(L, W, p.X)) { set_error("nerfail_mlp_pack_x3: shape not covered (W = 256, even D <= 8)"); return NERFAIL_EINVAL; }
    const long threads = (long)p.X.pieces / 3 * 64;
    pack_x3_kernel<<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(packed, p, reinterpret_cast<u32x4*>(out));
    NF_LAUNCHED("pack_x3_kernel");
    return NERFAIL_OK;
}

int launch_mlp_x3(const MlpArgs& a, const void* img, int W, hipStream_t s) {
    X3Layout X;
    if (!mlp_x3_covers(a.lay, W) || !make_x3_layout(a.lay, W, X)) { set_error("nerf_mlp_fwd_x3_kernel: shape not covered (W = 256, even D <= 8)"); return NERFAIL_EINVAL; }
    if (a.M >= (1L << 36)) { set_error("nerfail_mlp_fwd: M must be below 2^36 samples per call"); return NERFAIL_EINVAL; }
    const long ntiles = (a.M + 31) / 32;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
    }
    long blocks = (ntiles + 3) / 4;
    if (blocks > cus) blocks = cus;      // persistent: one 4-wave workgroup per CU, one wave per SIMD
    const dim3 grid((unsigned)blocks), block(256);
    const int skip_layer = a.lay.skip >= 0 ? a.lay.skip + 1 : -1;
    if (skip_layer < 0) nerf_mlp_fwd_x3_kernel<8, 0><<<grid, block, 0, s>>>(a, img, (int)X.pieces);
    else if (skip_layer & 1) nerf_mlp_fwd_x3_kernel<8, 1><<<grid, block, 0, s>>>(a, img, (int)X.pieces);
    else nerf_mlp_fwd_x3_kernel<8, 2><<<grid, block, 0, s>>>(a, img, (int)X.pieces);
    NF_LAUNCHED("nerf_mlp_fwd_x3_kernel");
    return NERFAIL_OK;
}

}  // namespace nerfail
