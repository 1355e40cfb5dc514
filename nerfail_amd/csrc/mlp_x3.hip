// K3 + K4, inference form on the bf16 matrix cores: fused positional encoding + NeRF MLP forward with every f32 product
// computed as six bf16 products ("bf16x3"), f32-accurate (run_nerf.py:37-51, run_nerf_helpers.py:15-50, :100-123).
//
// Arithmetic. Every f32 operand is split by round-to-nearest into three bf16 pieces, x = x0 + x1 + x2 + r with
// |x1| <= 2^-9 |x|, |x2| <= 2^-18 |x|, |r| <= 2^-27 |x| (each difference is exact in f32). Of the nine piece products the
// six a1b1, a0b2, a2b0, a0b1, a1b0, a0b0 are kept, smallest first, into the one f32 accumulator: a bf16 x bf16 product
// is exact in f32, and what is dropped (a1b2 + a2b1 + a2b2 and the residuals) adds up to about 2^-26 |a||b|, below one
// f32 rounding. The result is f32-accurate, not bitwise that of the exact-f32 kernel (mlp_lds.hip) - any reordering of
// an f32 sum differs in the last bits as well. bf16 has the f32 exponent range: no pre-scale, no weight-range limit.
// Cost per 32x32x16 f32-equivalent: 12 v_mfma_f32_16x16x32_bf16 (12 x 16 cycles) against 8 v_mfma_f32_32x32x2_f32 (8 x 64).
// The 16x16x32 shape takes the cycles per FLOP of the 32x32x16 one, but the chip holds a higher clock under it on random
// operands re-read from LDS (tools/clockprobe/mfma_clock.hip: 1.09x the FLOP/s at this kernel's LDS bytes per FLOP).
//
// Structure: that of nerf_mlp_fwd_lds_kernel (mlp_lds.hip) - one wave per SIMD, 32 samples x all channels per wave, every
// layer transposed (the accumulator tiles of one layer are the B operand of the next), the weight stream shared by the 4
// waves of a workgroup through an LDS-DMA ring with one barrier per group, running across layer boundaries; biases and
// the thin alpha / rgb heads in a constant LDS area (f32, computed exactly as there); encoding in the kernel.
//   * accumulators: per 16-row out tile two 16x16 tiles, one per sample half n (samples 16n + (lane & 15)); lane group
//     g = lane >> 4 holds rows 4g .. 4g+3 of both. 16 out tiles x 2 halves x 4 registers = 128 per activation array.
//   * A operand: the bf16x3 image (nerfail_mlp_pack_x3, split ONCE on the device from the f32 image), laid out per layer as
//     [k32 step][16-row out tile][plane][lane][8 bf16]: one 1 KB piece = the fragment of one (step, tile, plane); lane l
//     holds row l & 15 of the tile and k positions 8(l >> 4) .. +7 of the step.
//   * B operand: element j of lane group g in k32 step u is channel 32u + 4g + (j & 3) + 16(j >> 2), i.e. registers 0..3 of
//     out tiles 2u and 2u+1 of the layer before - no lane movement (the pack permutes the weights' k index to match). The
//     ReLU is applied lazily where an operand is consumed; each k32 step is split ONCE, one step ahead, and serves all 16
//     out tiles (8 in the views layer).
//   * one "tile-step" = the 12 MFMAs of one (k32 step, out tile): 6 products x 2 sample halves, with its 3 pieces; ring
//     group = 8 tile-steps = 24 pieces, 4 groups in the ring (96 KB). Fragments are read two tile-steps ahead, so the group
//     boundary sits at the group's second-to-last tile-step (both remaining tile-steps' fragments are in registers when
//     the slot is released).
#include "mlp_lds.h"
#include "bf16_split.h"

namespace nerfail {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const u32x4 lds_cu4;
typedef __attribute__((address_space(3))) const f32x2 lds_cf2;

struct X3Cfg {
    static constexpr int NT = 8;                 // W = 256 only (32-row tiles of the f32 image)
    static constexpr int OT = 2 * NT;            // 16-row out tiles
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
    // RAYBIAS form: no direction operands are parked; instead one 512-byte row of the per-ray view bias per wave
    static constexpr int kRowFloats = 16 * NT;   // W / 2 channels
    static constexpr int kParkFloatsRB = 4 * kRowFloats + 4 * 64 * 4 * kEmbQuads;
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
        if (quads & 3) return false;
        X.off[l] = off;
        off += quads / 4 * (2 * OT) * 3;                           // [k32 step][16-row out tile][plane]
    }
    X.pieces = off;
    return off % X3Cfg::GP == 0;
}
// The folded image (nerfail_mlp_pack_x3f): feature_linear and the hidden part of views_linears[0] composed into ONE 256 -> 128
// part (no activation lies between them), so layer D has no stream of its own: off[D] == off[D + 1], one 128-tile-step layer
// (16 ring groups) shorter. Behind the stream: the constant area as the f32 image has it (bias piece D, feature_linear's there
// and unused here, = the composed bias bc: the hooks of layer D - 1 hand piece D to the views layer's output tiles), then the composed f32 block - Wc [W/2][W] row-major, bc [W/2] zero-padded to a piece.
static inline bool make_x3f_layout(const MlpLayout& L, int W, X3Layout& X) {
    if (!make_x3_layout(L, W, X)) return false;
    const unsigned feature = X.off[L.D + 1] - X.off[L.D];
    X.off[L.D + 1] = X.off[L.D];
    X.pieces -= feature;
    return X.pieces % X3Cfg::GP == 0;
}
__host__ __device__ inline unsigned x3f_const_floats(const MlpLayout& L) { return L.total - L.b_off[0]; }
static inline unsigned x3f_composed_floats(const MlpLayout& L) { return (unsigned)(L.NT / 2 * 32) * (L.NT * 32) + kPiece; }

// (cvt_bf2 / sub_bf2, the three-way split: bf16_split.h)

// ---- the bf16x3 image from the f32 image: one thread per (layer step, tile, lane), 8 weights -> 3 x 16 bytes.
// The f32 image holds layer l as [quad Q][32-row tile][lane32][4]: weight (row i, k-step 4Q + e) of half h at lane32
// i + 32h, element e; for a hidden part, (Q, e, h) is channel 32(Q / 4) + acc_channel(4(Q % 4) + e, h). Element j of lane
// group g in k32 step u is (Q, e, h) = (4u + (g >> 1) + 2(j >> 2), j & 3, g & 1): channel 32u + 4g + (j & 3) + 16(j >> 2).
// The encoding parts (whole k32 steps too) take the same map; the kernel's parked-operand reader follows it.
struct X3PackArgs {
    MlpLayout L;
    X3Layout X;
};
// FOLD: the hidden part of the views layer is split from the composed Wc (compose_x3f_kernel) instead of the f32 image
template <bool FOLD>
__global__ void pack_x3_kernel(const float* __restrict__ packed, X3PackArgs p, u32x4* __restrict__ img, const float* __restrict__ wc) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long ts = g >> 6;                                        // tile-step in the stream
    const int lane = (int)(g & 63);
    if (ts * 3 >= p.X.pieces) return;
    int l = 0;
    while (l < p.L.D + 1 && ts * 3 >= p.X.off[l + 1]) ++l;
    const int OT32 = (l == p.L.D + 1) ? p.L.NT / 2 : p.L.NT, OT16 = 2 * OT32;
    const long r = ts - p.X.off[l] / 3;
    const int u = (int)(r / OT16), t = (int)(r % OT16);
    const int row = 16 * t + (lane & 15), lg = lane >> 4;          // out channel; lane group
    const int q = 4 * u + (lg >> 1);
    const float* w = packed + p.L.w_off[l] + (row >> 5) * kPiece + ((row & 31) + 32 * (lg & 1)) * 4;
    const f32x4 q0 = *reinterpret_cast<const f32x4*>(w + (q * OT32) * kPiece);
    const f32x4 q1 = *reinterpret_cast<const f32x4*>(w + ((q + 2) * OT32) * kPiece);
    float x[8] = {q0[0], q0[1], q0[2], q0[3], q1[0], q1[1], q1[2], q1[3]};
    if (FOLD && l == p.L.D + 1 && u < p.L.NT) {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = wc[row * (32 * p.L.NT) + 32 * u + 4 * lg + (j & 3) + 16 * (j >> 2)];
    }
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

// ---- the composed views layer of the folded image. h2 = relu(Wv[:, :W] (Wf h + bf) + Wv[:, W:] dirs + bv) has no activation
// between feature_linear and views_linears[0]: Wc = Wv[:, :W] Wf and bc = Wv[:, :W] bf + bv, by a FIXED rule - the sum over
// m = 0, 1, ..., W-1 in this order, in double from 0 (a product of two f32 values is exact in double: fused or not, the order
// alone fixes the bits), bv added last, rounded once to f32. Everything is read from the f32 image through the forward column
// map and its inverse (mlp_layout.h): column c of a hidden part is k-step hidden_step(c) of lane half hidden_half(c), and a
// bias piece holds channel c at bias_index(c).
// weight (row i, hidden column c) of layer l (OT32 32-row out tiles) in the f32 image
// weight (row i, k-step s of lane half h) of layer l (OT32 32-row out tiles) in the f32 image
__device__ __forceinline__ float x3f_weight_at(const float* __restrict__ packed, const MlpLayout& L, int l, int OT32, int i, int s, int h) {
    return packed[L.w_off[l] + ((s >> 2) * OT32 + (i >> 5)) * kPiece + ((i & 31) + 32 * h) * 4 + (s & 3)];
}
__device__ __forceinline__ float x3f_weight(const float* __restrict__ packed, const MlpLayout& L, int l, int OT32, int i, int c) {
    return x3f_weight_at(packed, L, l, OT32, i, hidden_step(c), hidden_half(c));
}
// threads [0, W/2 * W): Wc; then one per float of the constant area (bias piece D receives bc, zero behind it); then the bc piece
__global__ void compose_x3f_kernel(const float* __restrict__ packed, MlpLayout L, float* __restrict__ cst, float* __restrict__ comp) {
    const int W = 32 * L.NT, WV = W / 2, D = L.D;
    const int nconst = (int)x3f_const_floats(L);
    int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t < WV * W) {
        const int i = t / W, j = t % W;
        double acc = 0.;
        for (int m = 0; m < W; ++m)
            acc += (double)x3f_weight(packed, L, D + 1, L.NT / 2, i, m) * (double)x3f_weight(packed, L, D, L.NT, m, j);
        comp[t] = (float)acc;
        return;
    }
    t -= WV * W;
    if (t >= nconst + kPiece) return;
    const int pos = t < nconst ? t % kPiece : t - nconst;              // position in a bias piece / index in the bc piece
    const bool in_bias = t < nconst && t / kPiece == D;
    if (t < nconst && !in_bias) { cst[t] = packed[L.b_off[0] + t]; return; }
    // bias order -> channel: the inverse of bias_index
    const int ch = in_bias ? 32 * (pos >> 5) + acc_channel(pos & 15, (pos >> 4) & 1) : pos;
    float v = 0.f;
    if (ch < WV && pos < (in_bias ? W : WV)) {
        double acc = 0.;
        for (int m = 0; m < W; ++m)
            acc += (double)x3f_weight(packed, L, D + 1, L.NT / 2, ch, m) * (double)packed[L.b_off[D] + bias_index(m)];
        acc += (double)packed[L.b_off[D + 1] + bias_index(ch)];
        v = (float)acc;
    }
    (t < nconst ? cst[t] : comp[WV * W + pos]) = v;
}

// ---- the per-ray view bias of the RAYBIAS kernel. The direction columns of the views layer meet the same 27 encoded channels
// for every sample of a ray: vb[r][i] = bc[i] + sum_m Wv[i][W + m] enc(d_r)[m] is computed once per ray, by a FIXED rule in the
// style of compose_x3f_kernel - start from the composed f32 bc[i] (bias piece D of the folded image's constant area), add the
// terms m = 0, 1, ..., 26 in this order in double (each product is exact there), round once to f32. enc(d) is encode_dir, the
// code the MLP kernels run; the weight columns come from the f32 image through the forward column map. Row r is stored in bias
// piece order (channel i at bias_index(i)): the MLP kernel's bias hooks read it with the addressing of a bias piece.
// One workgroup = kVbRays rays: threads 2r + h encode lane half h of ray r into LDS (channel order), then thread (half, i) adds
// up channel i for 16 of the rays, its 27 weights in registers. dirs: `rays` [R,11] (the view direction at floats 8..10) or,
// when that is NULL, `viewdirs` [R,3].
constexpr int kVbRays = 32;
__global__ __launch_bounds__(256) void x3_viewbias_kernel(const float* __restrict__ packed, MlpLayout L, const float* __restrict__ cst,
                                                          const float* __restrict__ rays, const float* __restrict__ viewdirs, long R,
                                                          float* __restrict__ vb) {
    __shared__ float enc[kVbRays][kDirCh + 1];
    const int WV = 16 * L.NT, D = L.D;                                     // 2 * WV threads (host)
    const int t = (int)threadIdx.x;
    const long r0 = (long)blockIdx.x * kVbRays;
    if (t < 2 * kVbRays) {
        const int h = t & 1;
        const long r = r0 + (t >> 1) < R ? r0 + (t >> 1) : R - 1;
        const float* d = rays != nullptr ? rays + NERFAIL_RAY_FLOATS * r + 8 : viewdirs + 3 * r;
        float demb[4 * kDirQuads];
        encode_dir(d[0], d[1], d[2], h, demb);
#pragma unroll
        for (int s = 0; s < 4 * kDirQuads; ++s) {
            const int c = enc_channel(s, h, 4);
            if (c >= 0) enc[t >> 1][c] = demb[s];
        }
    }
    const int i = t % WV, half = t / WV;
    float w[kDirCh];
#pragma unroll
    for (int m = 0; m < kDirCh; ++m) {
        w[m] = 0.f;
#pragma unroll
        for (int s = 0; s < 4 * kDirQuads; ++s)
#pragma unroll
            for (int h = 0; h < 2; ++h)                                    // the k-step and lane half that multiply column W + m
                if (weight_column(-1, 0, 2 * WV, L.NT, 16 * L.NT + s, h) == 2 * WV + m)
                    w[m] = x3f_weight_at(packed, L, D + 1, L.NT / 2, i, 16 * L.NT + s, h);
    }
    const float bc = cst[D * kPiece + bias_index(i)];
    __syncthreads();
    for (int rr = half * (kVbRays / 2); rr < (half + 1) * (kVbRays / 2) && r0 + rr < R; ++rr) {
        double acc = (double)bc;
#pragma unroll
        for (int m = 0; m < kDirCh; ++m) acc += (double)w[m] * (double)enc[rr][m];
        vb[(r0 + rr) * WV + bias_index(i)] = (float)acc;
    }
}

// ---- the weight ring of one workgroup (the x3 counterpart of WRing in mlp_lds.hip; every member but f1 / f2 / voff / rl / rdp
// is wave-uniform). Refill interval: the SPG tile-steps from one boundary tile-step (inclusive) to the next; DMA P of the
// interval is issued behind the first MFMA of its P-th tile-step (P < GPW), the boundary's own behind its MFMA 4.
// Boundary i + 1 needs group i + 1 landed; its DMAs are older than the two younger groups' 2 * GPW -> vmcnt(2 * GPW).
// Bookkeeping in BYTES, by increments (no multiply or shift per DMA): `fill` and `srcb` carry the per-wave part
// wave * GPW pieces from the start; a DMA takes both as they are, pieces 0..3 and 4..5 of a wave through the 12-bit
// immediate (srcb steps over the first four pieces once, between DMA 3 and DMA 4; the LDS side is one add into m0). The
// slot being filled is always the group read before the current one: fill = ring + rd (old) + wave part, so the ring
// needs ONE wrap-around (rd's). Every update is one or two scalar instructions pinned (opaque copy) into an MFMA gap that
// has room for them (x3_step).
typedef __attribute__((address_space(3))) char lds_char_t;
typedef __attribute__((address_space(3))) const char lds_cchar_t;
struct X3Ring {
    using C = X3Cfg;
    static constexpr int kPB = kPiece * 4;                           // bytes of a piece
    static constexpr int kGB = C::GP * kPB;                          // bytes of a ring group
    __amdgpu_buffer_rsrc_t rsrc;     // the x3 image as a raw buffer (reads past its end return 0, never fault)
    int voff;                        // lane * 16
    lds_char_t* ring;                // LDS ring base
    lds_cchar_t* rl;                 // ring + lane * 16
    lds_cchar_t* rdp;                // rl + rd: the fragment reads' address (one per group, constant offsets)
    lds_char_t* fill;                // this wave's first piece of the ring group being filled
    int woff;                        // wave * GPW pieces
    int src_end;                     // stream length + woff
    int srcb;                        // source offset of this wave's next DMA block (pieces 0..3, then 4..)
    int rd;                          // offset in the ring of the group read next
    u32x4 f1[3], f2[3];              // fragments of the next two tile-steps

    template <int I>
    __device__ __forceinline__ void dma_at() const {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)(fill + (I / 4) * 4 * kPB), 16, voff, srcb, (I % 4) * kPB, 0);
    }
    __device__ __forceinline__ void dma(int i) const {             // i is a constant after unrolling
        switch (i) {
            case 0: dma_at<0>(); break;   case 1: dma_at<1>(); break;   case 2: dma_at<2>(); break;   case 3: dma_at<3>(); break;
            case 4: dma_at<4>(); break;   case 5: dma_at<5>(); break;   case 6: dma_at<6>(); break;   case 7: dma_at<7>(); break;
            default: break;
        }
    }
    // srcb: + 4 pieces between DMA 3 and DMA 4, the rest of a group behind the last DMA, then the wrap to the stream's start
    __device__ __forceinline__ void src_mid() { srcb += 4 * kPB; asm volatile("" : "+s"(srcb)); }
    __device__ __forceinline__ void src_step() { srcb += kGB - 4 * kPB; asm volatile("" : "+s"(srcb)); }
    __device__ __forceinline__ void src_wrap() { srcb = srcb == src_end ? woff : srcb; asm volatile("" : "+s"(srcb)); }
    // behind the last fragment read of a group: its slot is the next to be filled, the group after it the next to be read
    __device__ __forceinline__ void rd_step() {
        fill = ring + rd + woff;
        rd += kGB;
        asm volatile("" : "+s"(fill), "+s"(rd));
    }
    __device__ __forceinline__ void rd_wrap() { rd = rd == C::RP * kPB ? 0 : rd; asm volatile("" : "+s"(rd)); }
    __device__ __forceinline__ void rd_apply() { rdp = rl + rd; asm volatile("" : "+v"(rdp)); }
    __device__ __forceinline__ void boundary() const {
        lds_wait_vmcnt<(C::S - 2) * C::GPW>();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    // The ring's share of the gap behind MFMA k of the tile-step at position P of the refill interval. Gaps 4, 7 and 9 carry
    // one instruction of the operand split at most (x3_part), gap 0 one load.
    __device__ __forceinline__ void side(int P, int k) {
        if (P == 0 ? k == 4 : (P < C::GPW && k == 0)) dma(P);      // the boundary's gap 0 holds the wait and the barrier
        if (P == 3 && k == 4) src_mid();
        if (P == C::GPW && k == 4) src_step();
        if (P == C::GPW && k == 7) src_wrap();
        if (P == C::SPG - 1 && k == 4) rd_step();                  // the last fragment read of the group was behind MFMA 3
        if (P == C::SPG - 1 && k == 7) rd_wrap();
        if (P == C::SPG - 1 && k == 9) rd_apply();
    }
    // plane p of the tile-step at position POS (mod SPG) of the group read next: a constant offset from one address per group
    __device__ __forceinline__ u32x4 frag(int POS, int p) const { return *(lds_cu4*)(rdp + (3 * POS + p) * kPB); }
    // S-1 groups issued, group 0 readable; then the state right behind a boundary tile-step that sat two tile-steps before
    // the stream's first: DMAs 0 and 1 of group S-1 issued, the fragments of tile-steps 0 and 1 read
    __device__ __forceinline__ void start(float* ring0, int lane, int wave, int total) {
        static_assert(C::GPW > 4 && C::GPW <= 8 && C::GPW < C::SPG - 1, "side(): two DMA blocks per wave, bookkeeping behind the last DMA");
        voff = lane * 16;
        ring = (lds_char_t*)ring0;
        rl = ring + lane * 16;
        woff = wave * C::GPW * kPB;
        src_end = total * kPB + woff;
        srcb = woff;
        fill = ring + woff;
#pragma unroll
        for (int g = 0; g < C::S - 1; ++g) {
#pragma unroll
            for (int i = 0; i < C::GPW; ++i) {
                if (i == 4) src_mid();
                dma(i);
            }
            src_step();
            src_wrap();
            fill += kGB;
        }
        rd = 0;
        rdp = rl;
        boundary();
        dma(0);
        dma(1);
#pragma unroll
        for (int p = 0; p < 3; ++p) f1[p] = frag(0, p);
#pragma unroll
        for (int p = 0; p < 3; ++p) f2[p] = frag(1, p);
    }
};

__device__ __forceinline__ void mfma_x3(f32x4& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// Index of channel 16t + 4g + i (i = 0..3) in a bias piece or thin head, stored in the 32x32 accumulator order [OT][2][16]
// of the f32 image: the four rows of lane group g in out tile t are four consecutive floats, at x3_lane_off(g) +
// x3_tile_off(t). Callers add the lane part once, so that the tile part folds into the ds_read offsets.
__device__ __forceinline__ int x3_lane_off(int g) { return 16 * (g & 1) + 4 * (g >> 1); }
__device__ __forceinline__ int x3_tile_off(int t) { return 32 * (t >> 1) + 8 * (t & 1); }

// Thin heads on relu(x) in the 16x16 layout (the counterparts of lds_head / lds_head3): per sample half, a VALU dot
// product over the lane's 4 rows of every tile, then the sum over the 4 lane groups (xor 16, xor 32). One tile at a time.
// w: the head's weights + x3_lane_off(g).
template <int OT, int NIN>
__device__ __forceinline__ void x3_head(const f32x4 (&x)[NIN][2], const float* w, float (&out)[2]) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int t = 0; t < OT; ++t) {
        const f32x4 wv = lds_read4(w + x3_tile_off(t));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float v0 = x[t][0][e], v1 = x[t][1][e];
            asm("" : "+v"(v0), "+v"(v1));     // opaque copies (see lds_head)
            s0 = fmaf(wv[e], relu_bits(v0), s0);
            s1 = fmaf(wv[e], relu_bits(v1), s1);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    s0 += __shfl_xor(s0, 16, 64);
    s1 += __shfl_xor(s1, 16, 64);
    out[0] = s0 + __shfl_xor(s0, 32, 64);
    out[1] = s1 + __shfl_xor(s1, 32, 64);
}
template <int OT, int NIN>
__device__ __forceinline__ void x3_head3(const f32x4 (&x)[NIN][2], const float* w, int stride, float (&out)[2][3]) {
    float s[2][3] = {};
#pragma unroll
    for (int t = 0; t < OT; ++t) {
        const float* p = w + x3_tile_off(t);
        const f32x4 w0 = lds_read4(p), w1 = lds_read4(p + stride), w2 = lds_read4(p + 2 * stride);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                float v = x[t][n][e];
                asm("" : "+v"(v));
                v = relu_bits(v);
                s[n][0] = fmaf(w0[e], v, s[n][0]);
                s[n][1] = fmaf(w1[e], v, s[n][1]);
                s[n][2] = fmaf(w2[e], v, s[n][2]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = s[n][c] + __shfl_xor(s[n][c], 16, 64);
            out[n][c] = v + __shfl_xor(v, 32, 64);
        }
}

// One tile-step at stream position POS (mod SPG, a constant after unrolling): the twelve MFMAs of out tile `acc`, product
// by product smallest first, each for both sample halves (MFMA k = product k / 2, half k % 2). A 16x16x32 MFMA leaves 8 of
// its 16 cycles for vector issue: the budget of a gap is three instructions of any kind (tools/mfma_gaps.py). Behind MFMA
// k: in the boundary tile-step's gap 0 the wait and the barrier (the refill DMA and the fragment reads behind them are the
// first to touch the new group and the released slot; MFMA 0 itself runs on fragments read two tile-steps before), then
// side(k) (operand preparation, bias tiles), the ring's bookkeeping (X3Ring::side), and behind MFMAs 1..3 a fragment read of
// the tile-step two ahead (an LDS load issued by side(0) or side(1) is older than those reads: waiting for it does not
// wait for them).
template <class Side>
__device__ __forceinline__ void x3_step(X3Ring& st, const int POS, f32x4 (&acc)[2], const u32x4 (&b)[2][3], Side side) {
    using C = X3Cfg;
    const int P = (POS - C::kSync + C::SPG) % C::SPG;              // position in the refill interval
    const int AHEAD = (POS + 2) % C::SPG;
    static_assert((C::SPG - 1 + C::kSync + 2) % C::SPG == C::SPG - 1, "the group's last fragments are read at P = SPG - 1");
    u32x4 a[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) { a[p] = st.f1[p]; st.f1[p] = st.f2[p]; }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const int pr = k >> 1, n = k & 1;                          // a1b1, a0b2, a2b0, a0b1, a1b0, a0b0
        const int pa = pr == 0 || pr == 4 ? 1 : pr == 2 ? 2 : 0;
        const int pb = pr == 0 || pr == 3 ? 1 : pr == 1 ? 2 : 0;
        __builtin_amdgcn_sched_barrier(0);
        mfma_x3(acc[n], a[pa], b[n][pb]);
        __builtin_amdgcn_sched_barrier(0);
        if (P == 0 && k == 0) st.boundary();
        side(k);
        st.side(P, k);
        if (k == 1) st.f2[1] = st.frag(AHEAD, 1);
        if (k == 2) st.f2[0] = st.frag(AHEAD, 0);
        if (k == 3) st.f2[2] = st.frag(AHEAD, 2);
    }
    __builtin_amdgcn_sched_barrier(0);
}

// One part of a layer: NS k32 steps over OT out tiles (NS * OT a whole number of ring groups, so every part starts at
// stream position 0 mod SPG). ld(s, n, p, e): element 2p + e of step s's B operand for sample half n as f32 (an
// accumulator register, relu'd here when RELU, or a parked encoding value). Step s+1's operand is split during step s:
// pair (n, p) = (t / 4, t % 4) in tile-step t < 8, at most two instructions per gap - load 0, load 1 behind MFMAs 0, 1;
// ReLU behind 2, 3; then hi; extract hi; subtract; mid; extract mid; subtract; lo behind 4..10. Step 0's cannot be early
// (its source is the layer before). hook(s, t, k): behind MFMA k of tile-step t of step s (bias tiles: gaps the split leaves room in).
template <int OT, int NS, bool RELU, class Ld, class Hook>
__device__ __forceinline__ void x3_part(X3Ring& st, f32x4 (&out)[X3Cfg::OT][2], Ld ld, Hook hook) {
    static_assert((NS * OT) % X3Cfg::SPG == 0 && OT >= 8, "a part is a whole number of ring groups; 8 pairs per step");
    auto act = [](float v) { return RELU ? relu_bits(v) : v; };
    auto bf2_f32 = [](unsigned q) { return (f32x2){__uint_as_float(q << 16), __uint_as_float(q & 0xffff0000u)}; };
    u32x4 b[2][3];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            f32x2 x = {act(ld(0, n, p, 0)), act(ld(0, n, p, 1))};
            b[n][0][p] = cvt_bf2(x[0], x[1]);
            x -= bf2_f32(b[n][0][p]);
            b[n][1][p] = cvt_bf2(x[0], x[1]);
            x -= bf2_f32(b[n][1][p]);
            b[n][2][p] = cvt_bf2(x[0], x[1]);
        }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        u32x4 bn[2][3];
        f32x2 xs[8], es[8];
#pragma unroll
        for (int t = 0; t < OT; ++t) {
            auto side = [&](int k) {
                if (s + 1 < NS && t < 8) {
                    const int n = t >> 2, p = t & 3;
                    if (k == 0) xs[t][0] = ld(s + 1, n, p, 0);
                    if (k == 1) xs[t][1] = ld(s + 1, n, p, 1);
                    if (RELU && k == 2) xs[t][0] = relu_bits(xs[t][0]);
                    if (RELU && k == 3) xs[t][1] = relu_bits(xs[t][1]);
                    if (k == 4) bn[n][0][p] = cvt_bf2(xs[t][0], xs[t][1]);
                    if (k == 5) es[t] = bf2_f32(bn[n][0][p]);
                    if (k == 6) xs[t] -= es[t];
                    if (k == 7) bn[n][1][p] = cvt_bf2(xs[t][0], xs[t][1]);
                    if (k == 8) es[t] = bf2_f32(bn[n][1][p]);
                    if (k == 9) xs[t] -= es[t];
                    if (k == 10) bn[n][2][p] = cvt_bf2(xs[t][0], xs[t][1]);
                }
                hook(s, t, k);
            };
            x3_step(st, (s * OT + t) % X3Cfg::SPG, out[t], b, side);
        }
        if (s + 1 < NS) {
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int p = 0; p < 3; ++p) b[n][p] = bn[n][p];
        }
    }
}

// FOLD: `img` is the folded image (make_x3f_layout) - no feature layer; the views layer reads relu(h) directly, and the
// constant area comes from behind the image's stream instead of the f32 image.
//
// RAYBIAS (FOLD only; a call whose 32-sample tiles each lie inside one ray: samples_per_ray % 32 == 0): the direction part of the
// views layer is the same 128-vector for every sample of a ray, so it is not computed here at all. `vb` [rays][W/2] holds
// bc + Wv[:, W:] enc(d) per ray in bias piece order (x3_viewbias_kernel); a tile's row takes the place of bias piece D, which the
// hooks of layer D - 1 hand to the views layer's output tiles. No direction encoding, no parked direction operands, no
// direction part: the stream ends one ring group earlier (that part is the image's last group).
// One kernel text: the last argument is X3RayBias in the RAYBIAS form and an empty struct in the plain forms, whose
// instructions are then those of a kernel without it (a shared __device__ body behind two kernels is not: the plain forms come
// out with another register allocation).
struct X3NoRayBias {};
struct X3RayBias { const float* vb; };
template <int NT, int SKIP, bool FOLD, class RB>
__global__ __launch_bounds__(256, 1) void nerf_mlp_fwd_x3_kernel(MlpArgs a, const void* img, int img_pieces, RB rb) {
    constexpr bool RAYBIAS = !__is_same(RB, X3NoRayBias);
    const float* vb = nullptr;
    if constexpr (RAYBIAS) vb = rb.vb;
    static_assert(NT == X3Cfg::NT, "W = 256 only");
    static_assert(FOLD || !RAYBIAS, "the per-ray view bias replaces the COMPOSED bias bc");
    using C = X3Cfg;
    constexpr int OT = C::OT, OTV = OT / 2;
    constexpr int kParkQ = RAYBIAS ? kEmbQuads : C::kParkQuads;         // parked quads per wave
    // ONE object (see nerf_mlp_fwd_lds_kernel): ring first, then constants, then (RAYBIAS) the four waves' view-bias rows,
    // then the parked encoding operands
    __shared__ __attribute__((aligned(16))) float smem[C::RP * kPiece + C::kConstMax + (RAYBIAS ? C::kParkFloatsRB : C::kParkFloats)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = lane >> 5, j = lane & 31;                             // the encoding's (half, sample) of this lane
    const int g = lane >> 4, c = lane & 15;                             // lane group, sample in a 16-sample half
    const MlpLayout& L = a.lay;
    float* const ring0 = smem;
    float* const cst = smem + C::RP * kPiece;
    float* const park_w = cst + C::kConstMax + (RAYBIAS ? 4 * C::kRowFloats : 0) + wave * (64 * 4 * kParkQ);
    float* const park = park_w + lane * 4;
    // the parked operand of (half n, lane group g) is the encoding lane 16n + c + 32(g & 1) wrote (pack_x3_kernel's k map)
    const float* const park_rd = park_w + (c + 32 * (g & 1)) * 4 + (g >> 1) * 256;
    {   // constant area: biases (one piece per layer), alpha head, rgb head - from the f32 image
        const int n = (int)(L.total - L.b_off[0]);
        const float* __restrict__ gm = FOLD ? static_cast<const float*>(img) + (long)img_pieces * kPiece : a.packed + L.b_off[0];
        for (int i = tid * 4; i < n; i += 1024) *reinterpret_cast<f32x4*>(cst + i) = *reinterpret_cast<const f32x4*>(gm + i);
    }
    __syncthreads();
    const float* const c_alpha = cst + (L.alpha_off - L.b_off[0]);
    const float* const c_rgb = cst + (L.rgb_off - L.b_off[0]);
    int lane_off = x3_lane_off(g);
    asm volatile("" : "+v"(lane_off));                                   // added once: the tile parts stay immediates
    const float* const cst_g = cst + lane_off;
    // the heads' weights + the lane part. RAYBIAS: formed from cst_g where a head runs (the offset opaque: not hoisted), so
    // that neither lane_off nor the two sums are lane registers live across the round (<8,2> has none to spare)
    auto head_w = [&](unsigned off) {
        int o = (int)(off - L.b_off[0]);
        asm volatile("" : "+s"(o));
        return cst_g + o;
    };

    X3Ring st;
    st.rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(img), 0, img_pieces * (kPiece * 4), 0x00020000);
    st.start(ring0, lane, wave, RAYBIAS ? img_pieces - C::GP : img_pieces);   // RAYBIAS: the direction group is never streamed
    // RAYBIAS: this wave's row slot, in floats from cst (wave-uniform), and the tiles of a ray
    int row_off = C::kConstMax + wave * C::kRowFloats;
    const int tpr = a.spr >> 5;

    f32x4 P[OT][2], Q[OT][2];
    // dst[i] = bias of layer l, tile i (f32, in AGPRs), as side work of two tile-steps: the LDS read into the first sample
    // half behind MFMA 10 of tile-step t0, the four register copies into the second behind MFMAs 5, 6, 8, 9 of tile-step
    // t0 + 1 (when the read has landed: a copy right behind it would wait for it). Those gaps are empty in tile-steps 8..15
    // of a step, where the layers' bias tiles sit, and hold two split instructions at most below (the views layer's);
    // X3Ring::side uses gaps 0, 4, 7, 9 and shares gap 9 only in the interval's last tile-step (t = 5 mod 8: no bias copy).
    // (bias_tile_at: the piece given by its offset in floats from cst - a bias piece, or a view-bias row slot)
    auto bias_tile_at = [&](f32x4 (&dst)[OT][2], int off, int i, int t0, int t, int k) {
        if (t == t0 && k == 10) {
            dst[i][0] = lds_read4(cst_g + off + x3_tile_off(i));
        }
        if (t == t0 + 1 && k == 11) {
            dst[i][1] = dst[i][0];
            asm volatile("" : "+a"(dst[i][1]));
        }
    };
    auto bias_tile = [&](f32x4 (&dst)[OT][2], int l, int i, int t0, int t, int k) { bias_tile_at(dst, l * kPiece, i, t0, t, k); };
    // (outside the stream: a whole tile at once)
    auto bias_tile_now = [&](f32x4 (&dst)[OT][2], int l, int i) {
        dst[i][0] = lds_read4(cst_g + l * kPiece + x3_tile_off(i));
        dst[i][1] = dst[i][0];
        asm volatile("" : "+a"(dst[i][0]), "+a"(dst[i][1]));
    };
#pragma unroll
    for (int t = 0; t < OT; ++t) bias_tile_now(P, 0, t);                    // later rounds: written during the views layer

    const int ntiles = (int)((a.M + 31) / 32);
    const int nrounds = (int)((ntiles + (long)gridDim.x * 4 - 1) / ((long)gridDim.x * 4));
    for (int rnd = 0; rnd < nrounds; ++rnd) {
        // every wave walks the whole stream every round; one without a tile of its own recomputes the last tile, stores nothing
        const int tile_own = (int)(((long)rnd * gridDim.x + blockIdx.x) * 4 + wave);
        const int tile = tile_own < ntiles ? tile_own : ntiles - 1;
        int jj = j;
        asm volatile("" : "+v"(jj));
        const long sraw = (long)tile * 32 + jj;
        const long s = RAYBIAS || sraw < a.M ? sraw : a.M - 1;              // RAYBIAS: M is a multiple of 32, no partial tile
        if constexpr (RAYBIAS) {
            // The tile's view-bias row (ray tile / tpr, wave-uniform), 512 bytes, by ONE LDS-DMA of lanes 0..31 into this wave's
            // slot. It joins the ring's vmcnt queue as an entry OLDER than every ring DMA of this round: a boundary lets at
            // most (S - 2) * GPW younger DMAs stay in flight, and the wave issues GPW per ring group, so the round's THIRD
            // boundary (lds_wait_vmcnt in X3Ring::boundary) has seen the row land. Its first reader is a hook of layer D - 1,
            // behind layer 0's four groups at the least; writer and readers are this wave alone, no barrier is involved. The
            // slot's last reads of the round before (the same hooks) were waited for by every boundary since (lgkmcnt(0)).
            int tp = tpr;
            asm volatile("" : "+s"(tp));                                 // opaque per round, as spr below
            const int row = __builtin_amdgcn_readfirstlane(tile / tp);
            const __amdgpu_buffer_rsrc_t rrow = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<float*>(vb) + (long)row * C::kRowFloats, 0, C::kRowFloats * 4, 0x00020000);
            if (lane < 32) __builtin_amdgcn_raw_ptr_buffer_load_lds(rrow, (lds_void_t*)(cst + row_off), 16, st.voff, 0, 0, 0);
        }
        {
            float emb[4 * kEmbQuads], demb[4 * kDirQuads];
            int hh = h;
            asm volatile("" : "+v"(hh));
            if constexpr (FOLD) {       // spr opaque per round: its reciprocal (s / spr) is then formed here, not kept live (a spill)
                MlpArgs ar = a;
                asm volatile("" : "+s"(ar.spr));
                if constexpr (RAYBIAS) encode_sample_pts(ar, s, hh, emb); else encode_sample(ar, s, hh, emb, demb);
            } else {
                encode_sample(a, s, hh, emb, demb);
            }
#pragma unroll
            for (int k = 0; k < kEmbQuads; ++k)
                *reinterpret_cast<f32x4*>(park + k * 256) = (f32x4){emb[4 * k], emb[4 * k + 1], emb[4 * k + 2], emb[4 * k + 3]};
            if constexpr (!RAYBIAS) {
#pragma unroll
            for (int k = 0; k < kDirQuads; ++k)
                *reinterpret_cast<f32x4*>(park + (kEmbQuads + k) * 256) =
                    (f32x4){demb[4 * k], demb[4 * k + 1], demb[4 * k + 2], demb[4 * k + 3]};
            }
        }
        // k32 step u of a parked encoding from quad q0 on: element 2p + e is k-step 4Q + 2(p & 1) + e of quad
        // Q = q0 + 4u + (g >> 1) + 2(p >> 1)
        auto b_park = [&](int q0) {
            return [=](int u, int n, int p, int e) {
                return *(__attribute__((address_space(3))) const float*)(park_rd + n * 64 + (q0 + 4 * u + 2 * (p >> 1)) * 256 + 2 * (p & 1) + e);
            };
        };
        // element 2p + e of k32 step u: register 2(p & 1) + e of tile 2u + (p >> 1)
        auto b_acc = [](const f32x4 (&in)[OT][2]) {
            return [&in](int u, int n, int p, int e) { return in[2 * u + (p >> 1)][n][2 * (p & 1) + e]; };
        };
        auto no_hook = [](int, int, int) {};
        // layer 0: 63 -> W into P (its bias is already there); Q (dead) receives the bias of layer 1 meanwhile
        x3_part<OT, kEmbQuads / 4, false>(st, P, b_park(0), [&](int u, int t, int k) {     // tile 8u + i: tile-steps 7 + i, 8 + i
            for (int i = 0; i < 8; ++i) bias_tile(Q, 1, 8 * u + i, 7 + i, t, k);
        });

        float alpha[2] = {0.f, 0.f};
        auto layer = [&](f32x4 (&in)[OT][2], f32x4 (&out)[OT][2], int l, bool may_skip, bool may_be_last) __attribute__((always_inline)) {
            if (!FOLD && may_be_last && l == L.D) {                                  // alpha_linear on relu(h)
                x3_head<OT>(in, c_alpha + lane_off, alpha);
                alpha[0] += c_alpha[NT * 32];
                alpha[1] += c_alpha[NT * 32];
            }
            if (may_skip && l == L.skip + 1) x3_part<OT, kEmbQuads / 4, false>(st, out, b_park(0), no_hook);   // cat([input_pts, h])
            // input tiles 2u, 2u+1 are last read by the split of step u (during step u-1): dead from step u on
            int lb = l + 1;                                                 // the bias piece handed to the dying input tiles
            if constexpr (RAYBIAS) {
                // as an offset from cst: layer D - 1 hands on the tile's view-bias row instead of piece D. (The row is half a
                // piece: the upper tiles read what lies behind it, inside the LDS object, and are rewritten with layer 0's
                // bias during the views layer before anything reads them - as piece D's zero half is in the plain form.)
                // The select is two scalar instructions the compiler does not see into: written as `lb == L.D ? row_off : ...`
                // the <8,0> and <8,2> instantiations spill some 1500 VGPRs.
                lb *= kPiece;
                asm volatile("s_cmp_eq_u32 %1, %2\n\ts_cselect_b32 %0, %3, %0" : "+s"(lb) : "s"(l + 1), "s"(L.D), "s"(row_off) : "scc");
                x3_part<OT, NT, true>(st, out, b_acc(in), [&](int u, int t, int k) {
                    if (u > 0) { bias_tile_at(in, lb, 2 * u - 2, 8, t, k); bias_tile_at(in, lb, 2 * u - 1, 9, t, k); }
                    if (u == NT - 1) { bias_tile_at(in, lb, 2 * u, 10, t, k); bias_tile_at(in, lb, 2 * u + 1, 11, t, k); }
                });
            } else {
            if constexpr (FOLD) asm volatile("" : "+s"(lb));                // kept scalar: as a VGPR induction address it spills
            x3_part<OT, NT, true>(st, out, b_acc(in), [&](int u, int t, int k) {
                if (u > 0) { bias_tile(in, lb, 2 * u - 2, 8, t, k); bias_tile(in, lb, 2 * u - 1, 9, t, k); }
                if (u == NT - 1) { bias_tile(in, lb, 2 * u, 10, t, k); bias_tile(in, lb, 2 * u + 1, 11, t, k); }
            });
            }
            if (FOLD && may_be_last && l == L.D - 1) {                      // folded: `out` is the last pts activation
                if constexpr (RAYBIAS) x3_head<OT>(out, head_w(L.alpha_off), alpha);
                else x3_head<OT>(out, c_alpha + lane_off, alpha);
                alpha[0] += c_alpha[NT * 32];
                alpha[1] += c_alpha[NT * 32];
            }
        };
#pragma unroll 1
        for (int l = 1; l < L.D; l += 2) {                                  // D is even (host check): whole pairs
            layer(P, Q, l, SKIP == 1, FOLD);
            if (!FOLD || l + 1 < L.D) layer(Q, P, l + 1, SKIP == 2, !FOLD);     // FOLD: no layer D (wave-uniform)
        }
        float rgb[2][3];                                                    // rgb_linear: W/2 -> 3
        if constexpr (FOLD) {
            // h = relu(Q) is the last pts activation (one 256-wide layer fewer: the arrays have swapped roles). The composed
            // views layer goes into P's first tiles, which hold its bias bc (piece D, written by layer D - 1 as they died);
            // P's other tiles, dead, receive their half of the NEXT tile's layer 0 bias, the first half follows the head.
            // (alpha_linear ran on relu(Q) behind layer D - 1, inside the loop: behind the loop the kernel spills VGPRs)
            x3_part<OTV, NT, true>(st, P, b_acc(Q), [&](int u, int t, int k) { bias_tile(P, 0, OTV + u, 2, t, k); });
            if constexpr (!RAYBIAS) x3_part<OTV, kDirQuads / 4, false>(st, P, b_park(kEmbQuads), no_hook);   // RAYBIAS: in the bias
            if constexpr (RAYBIAS) x3_head3<OTV>(P, head_w(L.rgb_off), OTV * 16, rgb);
            else x3_head3<OTV>(P, c_rgb + lane_off, OTV * 16, rgb);
#pragma unroll
            for (int t = 0; t < OTV; ++t) bias_tile_now(P, 0, t);
        } else {
        // views_linears[0]: cat([feature, embedded dirs]) -> W/2 into Q's first tiles (no activation on the feature);
        // P receives the bias of the NEXT tile's layer 0 as its tiles die
        x3_part<OTV, NT, false>(st, Q, b_acc(P), [&](int u, int t, int k) {
            if (u > 0) { bias_tile(P, 0, 2 * u - 2, 2, t, k); bias_tile(P, 0, 2 * u - 1, 3, t, k); }
            if (u == NT - 1) { bias_tile(P, 0, 2 * u, 4, t, k); bias_tile(P, 0, 2 * u + 1, 5, t, k); }
        });
        x3_part<OTV, kDirQuads / 4, false>(st, Q, b_park(kEmbQuads), no_hook);
        x3_head3<OTV>(Q, c_rgb + lane_off, OTV * 16, rgb);
        }
        // lane group n < 2 stores sample half n
        const int n = g & 1;
        int je = 16 * n + c;
        asm volatile("" : "+v"(je));
        const long sout = (long)tile * 32 + je;
        if (g < 2 && (RAYBIAS || sout < a.M) && tile_own < ntiles)
            reinterpret_cast<float4*>(a.raw)[sout] = make_float4((n ? rgb[1][0] : rgb[0][0]) + c_rgb[3 * OTV * 16 + 0],
                                                                 (n ? rgb[1][1] : rgb[0][1]) + c_rgb[3 * OTV * 16 + 1],
                                                                 (n ? rgb[1][2] : rgb[0][2]) + c_rgb[3 * OTV * 16 + 2],
                                                                 n ? alpha[1] : alpha[0]);
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

size_t mlp_x3f_composed_floats(const MlpLayout& L, int W) { return mlp_x3_covers(L, W) ? x3f_composed_floats(L) : 0; }

size_t mlp_x3f_bytes(const MlpLayout& L, int W) {
    X3Layout X;
    if (!mlp_x3_covers(L, W) || !make_x3f_layout(L, W, X)) return 0;
    return ((size_t)X.pieces * kPiece + x3f_const_floats(L) + x3f_composed_floats(L)) * 4;
}

int pack_mlp_x3(const float* packed, const MlpLayout& L, int W, void* out, hipStream_t s) {
    X3PackArgs p;
    p.L = L;
    if (!mlp_x3_covers(L, W) || !make_x3_layout(L, W, p.X)) { set_error("nerfail_mlp_pack_x3: shape not covered (W = 256, even D <= 8)"); return NERFAIL_EINVAL; }
    const long threads = (long)p.X.pieces / 3 * 64;
    pack_x3_kernel<false><<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(packed, p, reinterpret_cast<u32x4*>(out), nullptr);
    NF_LAUNCHED("pack_x3_kernel");
    return NERFAIL_OK;
}

int pack_mlp_x3f(const float* packed, const MlpLayout& L, int W, void* out, hipStream_t s) {
    X3PackArgs p;
    p.L = L;
    if (!mlp_x3_covers(L, W) || !make_x3f_layout(L, W, p.X)) { set_error("nerfail_mlp_pack_x3f: shape not covered (W = 256, even D <= 8)"); return NERFAIL_EINVAL; }
    float* const cst = static_cast<float*>(out) + (size_t)p.X.pieces * kPiece;
    float* const comp = cst + x3f_const_floats(L);
    const long cthreads = (long)(W / 2) * W + x3f_const_floats(L) + kPiece;
    compose_x3f_kernel<<<dim3((unsigned)((cthreads + 255) / 256)), dim3(256), 0, s>>>(packed, L, cst, comp);
    NF_LAUNCHED("compose_x3f_kernel");
    const long threads = (long)p.X.pieces / 3 * 64;
    pack_x3_kernel<true><<<dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s>>>(packed, p, reinterpret_cast<u32x4*>(out), comp);
    NF_LAUNCHED("pack_x3_kernel");
    return NERFAIL_OK;
}

template <bool FOLD>
static void launch_x3(const MlpArgs& a, const void* img, int pieces, hipStream_t s) {
    const dim3 grid(mlp_grid_blocks((a.M + 31) / 32)), block(256);      // persistent: one 4-wave workgroup per CU
    const int skip_layer = a.lay.skip >= 0 ? a.lay.skip + 1 : -1;
    if (skip_layer < 0) nerf_mlp_fwd_x3_kernel<8, 0, FOLD, X3NoRayBias><<<grid, block, 0, s>>>(a, img, pieces, X3NoRayBias());
    else if (skip_layer & 1) nerf_mlp_fwd_x3_kernel<8, 1, FOLD, X3NoRayBias><<<grid, block, 0, s>>>(a, img, pieces, X3NoRayBias());
    else nerf_mlp_fwd_x3_kernel<8, 2, FOLD, X3NoRayBias><<<grid, block, 0, s>>>(a, img, pieces, X3NoRayBias());
}

// fold: `img` is the folded image of nerfail_mlp_pack_x3f
int launch_mlp_x3(const MlpArgs& a, const void* img, int W, bool fold, hipStream_t s) {
    X3Layout X;
    if (!mlp_x3_covers(a.lay, W) || !(fold ? make_x3f_layout(a.lay, W, X) : make_x3_layout(a.lay, W, X))) { set_error("nerf_mlp_fwd_x3_kernel: shape not covered (W = 256, even D <= 8)"); return NERFAIL_EINVAL; }
    if (a.M >= (1L << 36)) { set_error("nerfail_mlp_fwd: M must be below 2^36 samples per call"); return NERFAIL_EINVAL; }
    if (fold) launch_x3<true>(a, img, (int)X.pieces, s);
    else launch_x3<false>(a, img, (int)X.pieces, s);
    NF_LAUNCHED("nerf_mlp_fwd_x3_kernel");
    return NERFAIL_OK;
}

// ---- the RAYBIAS form: the folded image, whole 32-sample tiles inside one ray
bool mlp_x3_raybias_covers(const MlpLayout& L, int W, int spr) {
    X3Layout X;
    return mlp_x3_covers(L, W) && make_x3f_layout(L, W, X) && X.pieces > (unsigned)(X3Cfg::S * X3Cfg::GP) && spr > 0 && spr % 32 == 0;
}

// vb [R][W/2] from the directions of `rays` [R,11] or, when that is NULL, `viewdirs` [R,3]; `img` is the folded image
int launch_mlp_x3_viewbias(const float* packed, const void* img, const MlpLayout& L, int W, const float* rays, const float* viewdirs,
                           long R, float* vb, hipStream_t s) {
    X3Layout X;
    if (!mlp_x3_covers(L, W) || !make_x3f_layout(L, W, X)) { set_error("x3_viewbias_kernel: shape not covered (W = 256, even D <= 8)"); return NERFAIL_EINVAL; }
    if (R <= 0) return NERFAIL_OK;
    if ((R + kVbRays - 1) / kVbRays > 0x7fffffffL) { set_error("x3_viewbias_kernel: too many rays"); return NERFAIL_EINVAL; }
    const float* cst = static_cast<const float*>(img) + (size_t)X.pieces * kPiece;
    x3_viewbias_kernel<<<dim3((unsigned)((R + kVbRays - 1) / kVbRays)), dim3(W), 0, s>>>(packed, L, cst, rays, viewdirs, R, vb);
    NF_LAUNCHED("x3_viewbias_kernel");
    return NERFAIL_OK;
}

// the view bias of the call's rays into `vb`, then the RAYBIAS kernel
int launch_mlp_x3_raybias(const MlpArgs& a, const void* img, int W, float* vb, hipStream_t s) {
    X3Layout X;
    if (!mlp_x3_raybias_covers(a.lay, W, a.spr) || !make_x3f_layout(a.lay, W, X) || a.M % a.spr != 0 || a.xemb != nullptr) {
        set_error("nerf_mlp_fwd_x3_kernel (RAYBIAS): needs the folded image of a covered shape (W = 256, even D <= 8), rays or points with view directions, and samples_per_ray a multiple of 32");
        return NERFAIL_EINVAL;
    }
    if (a.M >= (1L << 36)) { set_error("nerfail_mlp_fwd: M must be below 2^36 samples per call"); return NERFAIL_EINVAL; }
    const int rc = launch_mlp_x3_viewbias(a.packed, img, a.lay, W, a.rays, a.viewdirs, a.M / a.spr, vb, s);
    if (rc != NERFAIL_OK) return rc;
    const dim3 grid(mlp_grid_blocks((a.M + 31) / 32)), block(256);      // persistent: one 4-wave workgroup per CU
    const int skip_layer = a.lay.skip >= 0 ? a.lay.skip + 1 : -1;
    const X3RayBias rb = {vb};
    if (skip_layer < 0) nerf_mlp_fwd_x3_kernel<8, 0, true, X3RayBias><<<grid, block, 0, s>>>(a, img, (int)X.pieces, rb);
    else if (skip_layer & 1) nerf_mlp_fwd_x3_kernel<8, 1, true, X3RayBias><<<grid, block, 0, s>>>(a, img, (int)X.pieces, rb);
    else nerf_mlp_fwd_x3_kernel<8, 2, true, X3RayBias><<<grid, block, 0, s>>>(a, img, (int)X.pieces, rb);
    NF_LAUNCHED("nerf_mlp_fwd_x3_kernel (RAYBIAS)");
    return NERFAIL_OK;
}

}  // namespace nerfail
