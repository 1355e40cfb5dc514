// poison revision 1 - the hand-off from an attack's export epoch to the retrain stage (README "retrain"; load_blender.py = LB,
// run_nerf.py = RN), in one pass over the float export: the uint8 image nerfail_export_u8 would write AND the float32 training
// target the file path makes of that image (PNG -> imageio -> LB:65's float64 divide -> RN:587-588's white composite), both
// straight into the slots of two resident stores. What the reference does through the disk, bit for bit, without it.
//
// The conversion q -> (float)((double)q / 255.0) comes from a 256-entry table every workgroup builds with the divide itself
// (256 lanes, one entry each): one definition, no constant to keep in step. The composite is three separately rounded float32
// operations, as numpy evaluates a[..., :3] * a[..., -1:] + (1. - a[..., -1:]).
#include <algorithm>
#include <vector>

#include "common.h"

namespace nerfail {

constexpr int kPoisonViews = 16;        // (view, slot) pairs per launch, passed by value
constexpr int kPoisonBlocks = 2048;     // grid cap of a streaming kernel (256 CUs x 8 workgroups)

struct PoisonSlots {
    int slot[kPoisonViews];
    int nb;
};

// LB:65 for one byte.
__device__ __forceinline__ float unit_of_u8(unsigned q) { return (float)((double)q / 255.0); }

// RN:588: c * a + (1 - a), every operation rounded on its own.
__device__ __forceinline__ float on_white(float c, float a) { return __fadd_rn(__fmul_rn(c, a), __fsub_rn(1.f, a)); }

struct Rgb {
    float r, g, b;
};

// One BGRA pixel: the dword of adv_u8 (B in the low byte, as cv2 stores it) and the RGB target.
__device__ __forceinline__ unsigned pixel4(const float4 v, const float* __restrict__ lut, Rgb* t) {
    const unsigned qb = to_u8(v.x), qg = to_u8(v.y), qr = to_u8(v.z), qa = to_u8(v.w);
    const float a = lut[qa];
    t->r = on_white(lut[qr], a);
    t->g = on_white(lut[qg], a);
    t->b = on_white(lut[qb], a);
    return qb | (qg << 8) | (qr << 16) | (qa << 24);
}

// x [nb,P,4] float32 BGRA -> adv [slot][P,4] uint8, tgt [slot][P,3] float32 RGB. blockIdx.y = the view of this launch.
// wide: the bases of both stores are 16-byte aligned; a view then takes the wide path when slot * P is a multiple of 4.
__global__ __launch_bounds__(256) void export_train_views4_kernel(const float4* __restrict__ x, PoisonSlots tab, long P,
                                                                  unsigned char* __restrict__ adv, float* __restrict__ tgt, int wide) {
    __shared__ float lut[256];
    lut[threadIdx.x] = unit_of_u8(threadIdx.x);
    __syncthreads();
    const int b = blockIdx.y;
    const long slot = tab.slot[b];
    const float4* src = x + (long)b * P;
    unsigned* a_out = reinterpret_cast<unsigned*>(adv) + slot * P;          // one dword per pixel: always 4-byte aligned
    float* t_out = tgt + slot * P * 3;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    long done = 0;
    if (wide && ((slot * P) & 3) == 0) {
        const long n4 = P >> 2;
        uint4* a4 = reinterpret_cast<uint4*>(a_out);
        float4* t4 = reinterpret_cast<float4*>(t_out);
        for (long i = t; i < n4; i += stride) {
            Rgb c0, c1, c2, c3;
            uint4 q;
            q.x = pixel4(src[4 * i + 0], lut, &c0);
            q.y = pixel4(src[4 * i + 1], lut, &c1);
            q.z = pixel4(src[4 * i + 2], lut, &c2);
            q.w = pixel4(src[4 * i + 3], lut, &c3);
            a4[i] = q;
            t4[3 * i + 0] = make_float4(c0.r, c0.g, c0.b, c1.r);
            t4[3 * i + 1] = make_float4(c1.g, c1.b, c2.r, c2.g);
            t4[3 * i + 2] = make_float4(c2.b, c3.r, c3.g, c3.b);
        }
        done = n4 << 2;
    }
    for (long p = done + t; p < P; p += stride) {
        Rgb c;
        a_out[p] = pixel4(src[p], lut, &c);
        t_out[3 * p + 0] = c.r;
        t_out[3 * p + 1] = c.g;
        t_out[3 * p + 2] = c.b;
    }
}

// x [nb,P,3] float32 BGR -> adv [slot][P,3] uint8, tgt [slot][P,3] float32 RGB (RN:587: a 3-channel image is taken as it is).
// wide: the bases of x and of both stores are 16-byte aligned; a view takes the wide path when b0 + b and slot, times P, are
// multiples of 4 (12 floats in, 12 bytes and 12 floats out per lane).
__global__ __launch_bounds__(256) void export_train_views3_kernel(const float* __restrict__ x, long b0, PoisonSlots tab, long P,
                                                                  unsigned char* __restrict__ adv, float* __restrict__ tgt, int wide) {
    __shared__ float lut[256];
    lut[threadIdx.x] = unit_of_u8(threadIdx.x);
    __syncthreads();
    const long b = b0 + blockIdx.y;
    const long slot = tab.slot[blockIdx.y];
    const float* src = x + b * P * 3;
    unsigned char* a_out = adv + slot * P * 3;
    float* t_out = tgt + slot * P * 3;
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    long done = 0;
    if (wide && ((b * P) & 3) == 0 && ((slot * P) & 3) == 0) {
        const long n4 = P >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        unsigned* a3 = reinterpret_cast<unsigned*>(a_out);
        float4* t4 = reinterpret_cast<float4*>(t_out);
        for (long i = t; i < n4; i += stride) {
            const float4 v0 = s4[3 * i + 0], v1 = s4[3 * i + 1], v2 = s4[3 * i + 2];     // b g r b | g r b g | r b g r
            const unsigned q0 = to_u8(v0.x), q1 = to_u8(v0.y), q2 = to_u8(v0.z), q3 = to_u8(v0.w);
            const unsigned q4 = to_u8(v1.x), q5 = to_u8(v1.y), q6 = to_u8(v1.z), q7 = to_u8(v1.w);
            const unsigned q8 = to_u8(v2.x), q9 = to_u8(v2.y), q10 = to_u8(v2.z), q11 = to_u8(v2.w);
            a3[3 * i + 0] = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
            a3[3 * i + 1] = q4 | (q5 << 8) | (q6 << 16) | (q7 << 24);
            a3[3 * i + 2] = q8 | (q9 << 8) | (q10 << 16) | (q11 << 24);
            t4[3 * i + 0] = make_float4(lut[q2], lut[q1], lut[q0], lut[q5]);
            t4[3 * i + 1] = make_float4(lut[q4], lut[q3], lut[q8], lut[q7]);
            t4[3 * i + 2] = make_float4(lut[q6], lut[q11], lut[q10], lut[q9]);
        }
        done = n4 << 2;
    }
    for (long p = done + t; p < P; p += stride) {
        const unsigned qb = to_u8(src[3 * p + 0]), qg = to_u8(src[3 * p + 1]), qr = to_u8(src[3 * p + 2]);
        a_out[3 * p + 0] = (unsigned char)qb;
        a_out[3 * p + 1] = (unsigned char)qg;
        a_out[3 * p + 2] = (unsigned char)qr;
        t_out[3 * p + 0] = lut[qr];
        t_out[3 * p + 1] = lut[qg];
        t_out[3 * p + 2] = lut[qb];
    }
}

static bool poison_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_poison_revision(void) { return 1; }

extern "C" int nerfail_export_train_views(const float* x, int channels, int B, int64_t P, const int32_t* slots_host, int64_t n_slots,
                                          unsigned char* adv_u8, float* target, void* stream) {
    NF_REQUIRE(channels == 3 || channels == 4, "channels must be 3 (BGR) or 4 (BGRA)");
    NF_REQUIRE(B >= 0 && B <= 65535, "B must be in 0..65535");
    NF_REQUIRE(P >= 1 && P <= ((int64_t)1 << 31), "P must be in 1..2^31");
    NF_REQUIRE(n_slots >= 1 && n_slots <= ((int64_t)1 << 31) - 1, "n_slots must be in 1..2^31-1");
    if (B == 0) return NERFAIL_OK;
    NF_REQUIRE(x != nullptr && slots_host != nullptr && adv_u8 != nullptr && target != nullptr, "NULL pointer");
    NF_REQUIRE(channels == 3 ? poison_aligned(x, 4) : poison_aligned(x, 16),
               "x must be 16-byte aligned (4 channels) or 4-byte aligned (3 channels)");
    NF_REQUIRE(poison_aligned(adv_u8, 4) && poison_aligned(target, 4), "adv_u8 and target must be 4-byte aligned");
    for (int b = 0; b < B; ++b) NF_REQUIRE(slots_host[b] >= 0 && (int64_t)slots_host[b] < n_slots, "a slot is outside 0..n_slots-1");
    {
        std::vector<int32_t> sorted(slots_host, slots_host + B);
        std::sort(sorted.begin(), sorted.end());
        NF_REQUIRE(std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end(), "the slots of one call must be distinct");
    }
    const int stores_wide = poison_aligned(adv_u8, 16) && poison_aligned(target, 16);
    const long quads = (long)((P + 3) / 4);
    for (int b0 = 0; b0 < B; b0 += kPoisonViews) {
        PoisonSlots tab;
        tab.nb = B - b0 < kPoisonViews ? B - b0 : kPoisonViews;
        for (int i = 0; i < kPoisonViews; ++i) tab.slot[i] = slots_host[b0 + (i < tab.nb ? i : 0)];
        long bx = (quads + 255) / 256;
        bx = bx > kPoisonBlocks / tab.nb ? kPoisonBlocks / tab.nb : (bx < 1 ? 1 : bx);
        const dim3 grid((unsigned)bx, (unsigned)tab.nb);
        if (channels == 4) {
            export_train_views4_kernel<<<grid, dim3(256), 0, as_stream(stream)>>>(reinterpret_cast<const float4*>(x) + (int64_t)b0 * P, tab,
                                                                                   (long)P, adv_u8, target, stores_wide);
            NF_LAUNCHED("export_train_views4_kernel");
        } else {
            export_train_views3_kernel<<<grid, dim3(256), 0, as_stream(stream)>>>(x, (long)b0, tab, (long)P, adv_u8, target,
                                                                                   stores_wide && poison_aligned(x, 16));
            NF_LAUNCHED("export_train_views3_kernel");
        }
    }
    return NERFAIL_OK;
}
