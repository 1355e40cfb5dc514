// What conv_stage_kernel (cnn.hip, exact f32) and conv_x3_kernel (cnn_x3.hip, bf16x3) share: the workgroup's tile, the map from
// accumulator registers to output rows, the epilogue on it, the pool-mask convention and the launch grid. Each kernel keeps its
// own operand staging, LDS layout and k-loop. Because both families write and read the pool masks through the code below, a
// workspace and masks of one family's forward can be handed to the other family's backward.
//
// MODE 0: forward, NHWC input.  MODE 1: forward, stage 1 (NCHW input; exact kernel only).  MODE 2: backward-data.
// Workgroup: 4 waves, each 2 m-tiles x NT n-tiles of 32 x 32. Forward: 8 x 8 pooled cells (wave w: pooled rows 2w, 2w+1; an
// m-tile is one pooled row of 8 cells = 2 x 16 conv pixels, ordered so that the four pixels of one 2x2 pool window are the four
// rows of one accumulator register group of a lane: row = (reg&3) + 8 (reg>>2) + 4 (lane>>5)). Backward: 8 rows x 32 columns of
// stage-input pixels (an m-tile is 32 pixels of one row).
#pragma once
#include "cnn_layout.h"

namespace nerfail {
namespace cnn {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int MODE>
struct Geo {                                                    // the LDS tile of the A operand, in pixels
    static constexpr int TH = MODE == 2 ? 10 : 18;
    static constexpr int TW = MODE == 2 ? 34 : 18;
};

constexpr int conv_nt(int NC) { return NC >= 64 ? 2 : 1; }     // 32-wide n-tiles per wave, forward and backward

// grid of one conv stage launch; Z: grid slices (B, or R * B)
template <int MODE, int NC, int NT>
static inline dim3 conv_grid(const ConvArgs& a, int Z) {
    const int tiles = MODE == 2 ? ((a.win + 31) / 32) * ((a.hin + 7) / 8) : ((a.wp + 7) / 8) * ((a.hp + 7) / 8);
    return dim3((unsigned)tiles, NC / (NT * 32), Z);
}

// tile origin: (ty0, tx0) in output units (forward: pooled cells), (gy0, gx0) the LDS tile's first pixel in global coordinates
template <int MODE>
__device__ __forceinline__ void tile_origin(const ConvArgs& a, int& ty0, int& tx0, int& gy0, int& gx0) {
    if (MODE == 2) {
        const int nx = (a.win + 31) / 32;
        ty0 = (blockIdx.x / nx) * 8;
        tx0 = (blockIdx.x % nx) * 32;
        gy0 = ty0 - 2;
        gx0 = tx0 - 2;
    } else {
        const int nx = (a.wp + 7) / 8;
        ty0 = (blockIdx.x / nx) * 8;
        tx0 = (blockIdx.x % nx) * 8;
        gy0 = 2 * ty0;
        gx0 = 2 * tx0;
    }
}

// LDS pixel of this lane's A row (m = n = lane & 31) of m-tile mt for tap (0,0); tap_ofs() moves it to the other taps
template <int MODE>
__device__ __forceinline__ int a_row_pixel(int wave, int n, int mt) {
    constexpr int TW = Geo<MODE>::TW;
    if (MODE == 2) return (2 * wave + mt + 2) * TW + n + 2;
    const int cell = n >> 2, q = n & 3;
    return (2 * (2 * wave + mt) + (q >> 1)) * TW + 2 * cell + (q & 1);
}

__device__ __forceinline__ int tap_ofs(int mode, int tap, int tw) {
    const int ky = tap / 3, kx = tap % 3;
    return mode == 2 ? -(ky * tw + kx) : ky * tw + kx;
}

// ---- the pool masks. One byte holds the 2-bit argmax codes (window position (dy, dx) row-major) of channel ch in the four
// pooled cells pc = 8 c8 + 2 w4 + half, w4 = 0..3 (code w4 at bits 2 w4): [image][pooled row][c8][half][channel].
// gmask_addr: the byte of pooled cell (pr, pc) and channel ch; n8 = npc8(wp), C channels.
__device__ __forceinline__ const unsigned char* gmask_addr(const unsigned char* gmask, int b, int hp, int n8, int pr, int pc, int C, int ch) {
    return gmask + ((((size_t)b * hp + pr) * n8 + (pc >> 3)) * 2 + (pc & 1)) * C + ch;
}
__device__ __forceinline__ int gate_shift(int pc) { return 2 * ((pc & 7) >> 1); }   // bit position of cell pc's code in its byte

// The un-pooled, ReLU-masked gradient at window position q of a pooled cell: the pooled gradient gv goes to the stored argmax
// position where the pooled value av is not <= 0 (ATen's threshold_backward o max_pool2d_backward). mk >> sh: the cell's code.
__device__ __forceinline__ float gate(float gv, float av, unsigned mk, int sh, unsigned q) {
    return (((mk >> sh) & 3u) == q && !(av <= 0.f)) ? gv : 0.f;
}

// ---- epilogue. Backward: scatter the accumulators to d input. Forward: bias + ReLU + 2x2 pool, argmax code, mask byte.
template <int MODE, int NC, int NT>
__device__ __forceinline__ void epilogue(const f32x16 (&acc)[2][NT], const ConvArgs a, int g, int b, int n0, int ty0, int tx0,
                                         int wave, int n, int h) {
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
                    if (a.mask)                                 // (gmask_addr's byte for the cells pc = tx0 + 2 w4 + h)
                        a.mask[((((size_t)b * a.hp + pr) * npc8(a.wp) + (tx0 >> 3)) * 2 + h) * NC + co] = (unsigned char)code;
                }
            }
        }
    }
}

}  // namespace cnn
}  // namespace nerfail
