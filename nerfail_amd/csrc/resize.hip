// resize revision 1 - the stage in front of a stock victim classifier (GaussNet.py = GN:121-157, model_test.py = MT:283-290):
// white background, NHWC -> NCHW and aten's antialiased bilinear resize as ONE kernel, and its exact adjoint as another. The
// arithmetic is the definition in include/nerfail_hip.h ("classifier-input resize"), restated in numpy by tests/resize_ref.py:
// tables in double rounded once to float32, then separately rounded float32 products and sums in a fixed order. No atomics, no
// global scratch: the intermediate of the two passes lives in LDS.
//
// Forward: a workgroup owns toy x tox outputs of one view, three channels. Its source window [wy][wx] goes to LDS planar
// (row stride odd: a column of it is conflict-free; nine loads per lane in flight), the horizontal pass gives lanes to window rows,
// three channel sums per lane - the output column, its
// start, count and weights are wave-uniform and sit in scalar registers - and the vertical pass gives lanes to output columns, so
// the planar store is coalesced. Adjoint: a workgroup owns ty x tx source pixels, stages the transposed weights of its rows and
// columns and the alpha test once, then loops over the R right-hand sides: g window -> LDS, vertical pass LDS -> LDS, horizontal
// pass LDS -> registers -> one 16-byte store per pixel (layout 0).
#include <vector>

#include "common.h"

namespace nerfail {

constexpr int kResizeTaps = NERFAIL_RESIZE_MAX_TAPS;
constexpr int kResizeLds = 80 * 1024;       // per workgroup: two of them share a CU's 160 KiB
constexpr int kResizeThreads = 256;
constexpr int kResizeBatch = 9;           // source loads a lane keeps in flight: 2 x 9 x 256 lanes cover the 49 x 92 window of 800 -> 299

// ---------------------------------------------------------------------------------------------------------------- host tables
struct HostAxis {
    int n_in = 0, n_out = 0, kmax = 0;
    bool ok = false;
    std::vector<int32_t> start, count, ostart, ocount;
    std::vector<float> w;                   // [n_out][kTaps]
};

static void axis_span(double scale, double support, int n_in, int i, int* start, int* count) {
    const double c = scale * ((double)i + 0.5);
    int s = (int)(c - support + 0.5);
    s = s > 0 ? s : 0;
    int e = (int)(c + support + 0.5);
    e = e < n_in ? e : n_in;
    *start = s;
    *count = e - s;
}

// The definition, in double. ok = false: a count or an inverted count above kResizeTaps, or an inverted range with a hole.
static void build_axis(int n_in, int n_out, HostAxis* a) {
    a->n_in = n_in;
    a->n_out = n_out;
    a->kmax = 0;
    a->ok = false;
    a->start.assign(n_out, 0);
    a->count.assign(n_out, 0);
    a->w.assign((size_t)n_out * kResizeTaps, 0.f);
    a->ostart.assign(n_in, -1);
    a->ocount.assign(n_in, 0);
    const double scale = (double)n_in / (double)n_out;
    const double support = scale >= 1.0 ? scale : 1.0;
    const double inv = scale >= 1.0 ? 1.0 / scale : 1.0;
    for (int i = 0; i < n_out; ++i) {
        int s, n;
        axis_span(scale, support, n_in, i, &s, &n);
        if (n < 1 || n > kResizeTaps) return;
        a->start[i] = s;
        a->count[i] = n;
        a->kmax = n > a->kmax ? n : a->kmax;
        const double c = scale * ((double)i + 0.5);
        double wk[kResizeTaps], total = 0.0;
        for (int k = 0; k < n; ++k) {
            const double x = ((double)(k + s) - c + 0.5) * inv;
            const double v = 1.0 - fabs(x);
            wk[k] = v > 0.0 ? v : 0.0;
            total += wk[k];
        }
        for (int k = 0; k < n; ++k) a->w[(size_t)i * kResizeTaps + k] = (float)(wk[k] / total);
        for (int j = s; j < s + n; ++j) {
            if (a->ocount[j] == 0) a->ostart[j] = i;
            else if (a->ostart[j] + a->ocount[j] != i) return;          // not contiguous
            if (++a->ocount[j] > kResizeTaps) return;
        }
    }
    for (int j = 0; j < n_in; ++j)
        if (a->ocount[j] < 1) return;                                    // not covered
    a->ok = true;
}

// The launch functions size their tiles from the host tables: a few (n_in, n_out) pairs are kept per thread.
// `keep`: a table of the same call that must not be the one replaced.
static const HostAxis* host_axis(int n_in, int n_out, const HostAxis* keep = nullptr) {
    constexpr int kSlots = 4;
    static thread_local HostAxis cache[kSlots];
    static thread_local int next = 0;
    for (int i = 0; i < kSlots; ++i)
        if (cache[i].n_in == n_in && cache[i].n_out == n_out) return &cache[i];
    if (&cache[next] == keep) next = (next + 1) % kSlots;
    HostAxis* a = &cache[next];
    next = (next + 1) % kSlots;
    build_axis(n_in, n_out, a);
    return a;
}

// Largest source window of a tile of `tile` outputs, and largest output window of a tile of `tile` inputs.
static int max_window(const std::vector<int32_t>& start, const std::vector<int32_t>& count, int n, int tile) {
    int m = 1;
    for (int i0 = 0; i0 < n; i0 += tile) {
        const int i1 = (i0 + tile < n ? i0 + tile : n) - 1;
        const int span = start[i1] + count[i1] - start[i0];
        m = span > m ? span : m;
    }
    return m;
}

struct ResizePlan {
    int t0, t1;         // tile: rows, columns (outputs for the forward, source pixels for the adjoint)
    int w0, w1;         // largest window: rows, columns
    int stride;         // LDS row stride of the window, odd
    size_t lds;         // bytes
};

static size_t fwd_lds(int toy, int tox, int wy, int stride) {
    return sizeof(float) * ((size_t)3 * wy * stride + (size_t)3 * wy * (tox + 1));
}
static size_t bwd_lds(int ty, int tx, int gh, int stride) {
    // g window, tmp, transposed weights of the rows and of the columns, per-row and per-column ranges, the alpha test
    return sizeof(float) * ((size_t)3 * gh * stride + (size_t)3 * ty * stride + (size_t)kResizeTaps * (ty + tx) + 2 * (size_t)(ty + tx) +
                            (size_t)ty * tx);
}

static ResizePlan plan_fwd(const HostAxis* ay, const HostAxis* ax) {
    static const int ladder[][2] = {{16, 32}, {8, 32}, {8, 16}, {4, 16}, {4, 8}, {2, 8}};
    ResizePlan p{};
    for (const auto& t : ladder) {
        p.t0 = t[0];
        p.t1 = t[1];
        p.w0 = max_window(ay->start, ay->count, ay->n_out, p.t0);
        p.w1 = max_window(ax->start, ax->count, ax->n_out, p.t1);
        p.stride = p.w1 | 1;
        p.lds = fwd_lds(p.t0, p.t1, p.w0, p.stride);
        if (p.lds <= (size_t)kResizeLds) break;
    }
    return p;
}

static ResizePlan plan_bwd(const HostAxis* ay, const HostAxis* ax) {
    static const int ladder[][2] = {{16, 64}, {8, 64}, {8, 32}, {4, 32}, {4, 16}, {2, 16}, {2, 8}, {1, 8}};
    ResizePlan p{};
    for (const auto& t : ladder) {
        p.t0 = t[0];
        p.t1 = t[1];
        p.w0 = max_window(ay->ostart, ay->ocount, ay->n_in, p.t0);
        p.w1 = max_window(ax->ostart, ax->ocount, ax->n_in, p.t1);
        p.stride = p.w1 | 1;
        p.lds = bwd_lds(p.t0, p.t1, p.w0, p.stride);
        if (p.lds <= (size_t)kResizeLds) break;
    }
    return p;
}

// ---------------------------------------------------------------------------------------------------------------- kernels
struct AxisDev {
    const int* start;
    const int* count;
    const float* w;
    const int* ostart;
    const int* ocount;
    int n_in, n_out, kmax;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The window of the tile [i0, i0 + n) of an axis: first = start[i0], size = start[last] + count[last] - first, kept inside
// [0, limit) and at most `cap` long whatever the tables hold.
__device__ __forceinline__ void tile_window(const int* __restrict__ start, const int* __restrict__ count, int i0, int n, int limit,
                                            int cap, int* first, int* size) {
    const int f = clampi(start[i0], 0, limit - 1);
    const int e = start[i0 + n - 1] + count[i0 + n - 1];
    const int room = limit - f < cap ? limit - f : cap;
    *first = f;
    *size = clampi(e - f, 1, room);
}

// out [B,3,oh,ow] from src (LAYOUT 0: [B,H,W,4], white where alpha > 0 is false; LAYOUT 1: [B,3,H,W]).
// LDS: s [3 * wy][stride] the source window, t [3 * wy][tox + 1] the horizontal pass.
template <int LAYOUT>
__global__ __launch_bounds__(kResizeThreads) void cls_input_resize_fwd_kernel(const float* __restrict__ src, int H, int W, int oh, int ow,
                                                                              AxisDev ay, AxisDev ax, int toy, int tox, int wymax,
                                                                              int wxmax, int stride, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.z, oy0 = blockIdx.y * toy, ox0 = blockIdx.x * tox;
    const int ny = oh - oy0 < toy ? oh - oy0 : toy, nx = ow - ox0 < tox ? ow - ox0 : tox;
    int y0, wy, x0, wx;
    tile_window(ay.start, ay.count, oy0, ny, H, wymax, &y0, &wy);
    tile_window(ax.start, ax.count, ox0, nx, W, wxmax, &x0, &wx);
    float* s = lds;
    float* t = lds + 3 * wymax * stride;
    const int tp = tox + 1;
    const int rows = 3 * wy;                                     // r = ch * wy + row

    if (LAYOUT == 0) {
        // kResizeBatch loads in flight per lane before the first goes to LDS: a lane's loads do not wait for one another
        const float4* src4 = reinterpret_cast<const float4*>(src) + ((long)b * H + y0) * W + x0;
        const int n = wy * wx;
        for (int p0 = tid; p0 < n; p0 += kResizeThreads * kResizeBatch) {
            float4 v[kResizeBatch];
            int at[kResizeBatch];
#pragma unroll
            for (int u = 0; u < kResizeBatch; ++u) {
                const int p = p0 + u * kResizeThreads;
                const int pc = p < n ? p : n - 1;                // past the end: re-read the last pixel, store nothing
                const int row = pc / wx, col = pc - row * wx;
                v[u] = src4[(long)row * W + col];
                at[u] = p < n ? row * stride + col : -1;
            }
#pragma unroll
            for (int u = 0; u < kResizeBatch; ++u) {
                if (at[u] >= 0) {
                    const bool on = v[u].w > 0.f;
                    s[at[u]] = on ? v[u].x : 255.f;
                    s[wy * stride + at[u]] = on ? v[u].y : 255.f;
                    s[2 * wy * stride + at[u]] = on ? v[u].z : 255.f;
                }
            }
        }
    } else {
        const float* base = src + (long)b * 3 * H * W;
        const int n = rows * wx;
        for (int p0 = tid; p0 < n; p0 += kResizeThreads * kResizeBatch) {
            float v[kResizeBatch];
            int at[kResizeBatch];
#pragma unroll
            for (int u = 0; u < kResizeBatch; ++u) {
                const int p = p0 + u * kResizeThreads;
                const int pc = p < n ? p : n - 1;
                const int r = pc / wx, col = pc - r * wx;
                const int ch = r / wy, row = r - ch * wy;
                v[u] = base[((long)ch * H + y0 + row) * W + x0 + col];
                at[u] = p < n ? r * stride + col : -1;
            }
#pragma unroll
            for (int u = 0; u < kResizeBatch; ++u)
                if (at[u] >= 0) s[at[u]] = v[u];
        }
    }
    __syncthreads();

    // horizontal pass: one output column per wave and step, lanes over the window's rows; a lane carries the three channels of
    // its row as three independent sums, so an LDS read's latency is shared by three chains
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int cs = wy * stride, ct = wy * tp;                    // channel strides of s and t
    for (int oxl = wave; oxl < nx; oxl += kResizeThreads / 64) {
        const int ox = ox0 + oxl;
        const int xs = clampi(ax.start[ox] - x0, 0, wx - 1);
        int cnt = ax.count[ox] < ax.kmax ? ax.count[ox] : ax.kmax;
        cnt = clampi(cnt, 1, wx - xs);
        const float* __restrict__ wr = ax.w + (long)ox * ax.kmax;
        for (int row = lane; row < wy; row += 64) {
            const float* v = s + row * stride + xs;
            const float w0 = wr[0];
            float a0 = __fmul_rn(w0, v[0]), a1 = __fmul_rn(w0, v[cs]), a2 = __fmul_rn(w0, v[2 * cs]);
            for (int k = 1; k < cnt; ++k) {
                const float wk = wr[k];
                a0 = __fadd_rn(a0, __fmul_rn(wk, v[k]));
                a1 = __fadd_rn(a1, __fmul_rn(wk, v[cs + k]));
                a2 = __fadd_rn(a2, __fmul_rn(wk, v[2 * cs + k]));
            }
            float* o = t + row * tp + oxl;
            o[0] = a0;
            o[ct] = a1;
            o[2 * ct] = a2;
        }
    }
    __syncthreads();

    // vertical pass: lanes over output columns, again the three channels of an output per lane
    for (int idx = tid; idx < ny * nx; idx += kResizeThreads) {
        const int oyl = idx / nx, oxl = idx - oyl * nx;
        const int oy = oy0 + oyl;
        const int ys = clampi(ay.start[oy] - y0, 0, wy - 1);
        int cnt = ay.count[oy] < ay.kmax ? ay.count[oy] : ay.kmax;
        cnt = clampi(cnt, 1, wy - ys);
        const float* __restrict__ wr = ay.w + (long)oy * ay.kmax;
        const float* v = t + ys * tp + oxl;
        const float w0 = wr[0];
        float a0 = __fmul_rn(w0, v[0]), a1 = __fmul_rn(w0, v[ct]), a2 = __fmul_rn(w0, v[2 * ct]);
        for (int k = 1; k < cnt; ++k) {
            const float wk = wr[k];
            a0 = __fadd_rn(a0, __fmul_rn(wk, v[k * tp]));
            a1 = __fadd_rn(a1, __fmul_rn(wk, v[ct + k * tp]));
            a2 = __fadd_rn(a2, __fmul_rn(wk, v[2 * ct + k * tp]));
        }
        float* o = out + (((long)b * 3) * oh + oy) * ow + ox0 + oxl;
        o[0] = a0;
        o[(long)oh * ow] = a1;
        o[2 * (long)oh * ow] = a2;
    }
}

// gsrc (LAYOUT 0: [R,B,H,W,4]; LAYOUT 1: [R,B,3,H,W]) from g [R,B,3,oh,ow].
// LDS: gs [3 * gh][stride] the g window, tmp [3 * ty][stride] the vertical pass, awy [taps][ty] and awx [taps][tx] the weights of
// every (source row / column, j-th output of its inverted range), ry / rx the ranges (first output relative to the window,
// count), on [ty * tx] the alpha test.
template <int LAYOUT>
__global__ __launch_bounds__(kResizeThreads) void cls_input_resize_bwd_kernel(const float* __restrict__ g, int R, const float* __restrict__ src,
                                                                              int B, int H, int W, int oh, int ow, AxisDev ay, AxisDev ax,
                                                                              int ty, int tx, int ghmax, int gwmax, int stride,
                                                                              float* __restrict__ gsrc) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int b = blockIdx.z, y0 = blockIdx.y * ty, x0 = blockIdx.x * tx;
    const int ny = H - y0 < ty ? H - y0 : ty, nx = W - x0 < tx ? W - x0 : tx;
    int goy0, gh, gox0, gw;
    tile_window(ay.ostart, ay.ocount, y0, ny, oh, ghmax, &goy0, &gh);
    tile_window(ax.ostart, ax.ocount, x0, nx, ow, gwmax, &gox0, &gw);
    float* gs = lds;
    float* tmp = gs + 3 * ghmax * stride;
    float* awy = tmp + 3 * ty * stride;
    float* awx = awy + kResizeTaps * ty;
    int* ry = reinterpret_cast<int*>(awx + kResizeTaps * tx);   // [2][ty]
    int* rx = ry + 2 * ty;                                       // [2][tx]
    float* on = reinterpret_cast<float*>(rx + 2 * tx);           // [ty * tx]

    // once per workgroup: ranges, transposed weights, the alpha test
    for (int i = tid; i < ny + nx; i += kResizeThreads) {
        const bool isy = i < ny;
        const int l = isy ? i : i - ny;
        const AxisDev& a = isy ? ay : ax;
        const int j = (isy ? y0 : x0) + l;
        const int first = isy ? goy0 : gox0, size = isy ? gh : gw;
        const int os = clampi(a.ostart[j] - first, 0, size - 1);
        const int oc = clampi(a.ocount[j], 1, (size - os) < kResizeTaps ? (size - os) : kResizeTaps);
        int* rr = isy ? ry : rx;
        const int n = isy ? ty : tx;
        rr[l] = os;
        rr[n + l] = oc;
        float* aw = isy ? awy : awx;
        for (int q = 0; q < oc; ++q) {
            const int o = first + os + q;                        // < a.n_out by the clamps above
            const int k = j - a.start[o];
            const int c = a.count[o] < a.kmax ? a.count[o] : a.kmax;
            aw[q * n + l] = (k >= 0 && k < c) ? a.w[(long)o * a.kmax + k] : 0.f;
        }
    }
    if (LAYOUT == 0) {
        const float* alpha = src + ((((long)b * H + y0) * W + x0) * 4 + 3);
        for (int p = tid; p < ny * nx; p += kResizeThreads) {
            const int yl = p / nx, xl = p - yl * nx;
            on[p] = alpha[((long)yl * W + xl) * 4] > 0.f ? 1.f : 0.f;
        }
    }
    __syncthreads();

    for (int r = 0; r < R; ++r) {
        const float* gr = g + ((long)r * B + b) * 3 * oh * ow;
        for (int p = tid; p < 3 * gh * gw; p += kResizeThreads) {
            const int q = p / gw, col = p - q * gw;
            const int ch = q / gh, row = q - ch * gh;
            gs[q * stride + col] = gr[((long)ch * oh + goy0 + row) * ow + gox0 + col];
        }
        __syncthreads();
        // vertical pass: tmp[ch][yl][col] over the outputs of source row yl, ascending
        for (int idx = tid; idx < 3 * ny * gw; idx += kResizeThreads) {
            const int q = idx / gw, col = idx - q * gw;
            const int ch = q / ny, yl = q - ch * ny;
            const int os = ry[yl], oc = ry[ty + yl];
            const float* v = gs + (ch * gh + os) * stride + col;
            float acc = __fmul_rn(awy[yl], v[0]);
            for (int j = 1; j < oc; ++j) acc = __fadd_rn(acc, __fmul_rn(awy[j * ty + yl], v[j * stride]));
            tmp[q * stride + col] = acc;
        }
        __syncthreads();
        // horizontal pass: one source pixel per lane and step, three channels
        for (int p = tid; p < ny * nx; p += kResizeThreads) {
            const int yl = p / nx, xl = p - yl * nx;
            const int os = rx[xl], oc = rx[tx + xl];
            const float* v = tmp + yl * stride + os;
            const int cs = ny * stride;                          // channel stride of tmp
            const float w0 = awx[xl];
            float a0 = __fmul_rn(w0, v[0]), a1 = __fmul_rn(w0, v[cs]), a2 = __fmul_rn(w0, v[2 * cs]);
            for (int j = 1; j < oc; ++j) {
                const float wj = awx[j * tx + xl];
                a0 = __fadd_rn(a0, __fmul_rn(wj, v[j]));
                a1 = __fadd_rn(a1, __fmul_rn(wj, v[cs + j]));
                a2 = __fadd_rn(a2, __fmul_rn(wj, v[2 * cs + j]));
            }
            const int y = y0 + yl, x = x0 + xl;
            if (LAYOUT == 0) {
                const bool keep = on[p] != 0.f;
                reinterpret_cast<float4*>(gsrc)[(((long)r * B + b) * H + y) * W + x] =
                    make_float4(keep ? a0 : 0.f, keep ? a1 : 0.f, keep ? a2 : 0.f, 0.f);
            } else {
                float* o = gsrc + ((((long)r * B + b) * 3) * H + y) * W + x;
                o[0] = a0;
                o[(long)H * W] = a1;
                o[2 * (long)H * W] = a2;
            }
        }
        // the next r writes gs (read by nobody after the barrier above) and then, behind its own barrier, tmp
    }
}

static bool resize_aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static AxisDev axis_dev(const nerfail_resize_axis* a) {
    AxisDev d;
    d.start = a->start;
    d.count = a->count;
    d.w = a->w;
    d.ostart = a->ostart;
    d.ocount = a->ocount;
    d.n_in = a->n_in;
    d.n_out = a->n_out;
    d.kmax = a->kmax;
    return d;
}

template <typename K>
static int allow_lds(K kernel, const char* name) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kResizeLds);
    return e == hipSuccess ? NERFAIL_OK : hip_fail(e, name);
}

}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_resize_revision(void) { return 1; }

extern "C" int nerfail_resize_aa_kmax(int n_in, int n_out) {
    if (n_in < 1 || n_out < 1) return 0;
    const double scale = (double)n_in / (double)n_out;
    const double support = scale >= 1.0 ? scale : 1.0;
    int kmax = 0;
    for (int i = 0; i < n_out; ++i) {
        int s, n;
        axis_span(scale, support, n_in, i, &s, &n);
        kmax = n > kmax ? n : kmax;
    }
    return kmax;
}

extern "C" int nerfail_resize_aa_table(int n_in, int n_out, int32_t* start, int32_t* count, float* w, int kmax, int32_t* ostart,
                                       int32_t* ocount) {
    NF_REQUIRE(n_in >= 1 && n_out >= 1, "n_in and n_out must be >= 1");
    NF_REQUIRE(start != nullptr && count != nullptr && w != nullptr && ostart != nullptr && ocount != nullptr, "NULL pointer");
    HostAxis a;
    build_axis(n_in, n_out, &a);
    NF_REQUIRE(a.ok, "an output takes, or an input feeds, more than 16 taps (or the inverted ranges have a hole)");
    NF_REQUIRE(kmax >= a.kmax, "kmax is below the axis' largest count (nerfail_resize_aa_kmax)");
    for (int i = 0; i < n_out; ++i) {
        start[i] = a.start[i];
        count[i] = a.count[i];
        for (int k = 0; k < kmax; ++k) w[(size_t)i * kmax + k] = k < kResizeTaps ? a.w[(size_t)i * kResizeTaps + k] : 0.f;
    }
    for (int j = 0; j < n_in; ++j) {
        ostart[j] = a.ostart[j];
        ocount[j] = a.ocount[j];
    }
    return NERFAIL_OK;
}

extern "C" int nerfail_resize_tiles(int H, int W, int oh, int ow, int32_t* fwd_tile, int32_t* bwd_tile) {
    NF_REQUIRE(H >= 1 && W >= 1 && oh >= 1 && ow >= 1, "H, W, oh and ow must be >= 1");
    NF_REQUIRE(fwd_tile != nullptr && bwd_tile != nullptr, "NULL pointer");
    const HostAxis* ay = host_axis(H, oh);
    const HostAxis* ax = host_axis(W, ow, ay);
    NF_REQUIRE(ay->ok && ax->ok, "an axis takes more than 16 taps");
    const ResizePlan f = plan_fwd(ay, ax), r = plan_bwd(ay, ax);
    fwd_tile[0] = f.t0;
    fwd_tile[1] = f.t1;
    bwd_tile[0] = r.t0;
    bwd_tile[1] = r.t1;
    return NERFAIL_OK;
}

// What both launch functions refuse; on NERFAIL_OK *hy / *hx are the host tables of the two axes.
static int resize_check(const char* who, const void* in, const void* outp, int layout, int B, int H, int W, int oh, int ow,
                        const nerfail_resize_axis* ty, const nerfail_resize_axis* tx, bool in_is_image, const HostAxis** hy,
                        const HostAxis** hx) {
#define RS_REQUIRE(cond, msg)                          \
    do {                                               \
        if (!(cond)) {                                 \
            ::nerfail::set_error("%s: %s", who, msg);  \
            return NERFAIL_EINVAL;                     \
        }                                              \
    } while (0)
    RS_REQUIRE(layout == 0 || layout == 1, "layout must be 0 ([B,H,W,4], white background) or 1 ([B,3,H,W])");
    RS_REQUIRE(B >= 1 && B <= 65535, "B must be in 1..65535");
    RS_REQUIRE(H >= 1 && W >= 1 && oh >= 1 && ow >= 1, "H, W, oh and ow must be >= 1");
    RS_REQUIRE(in != nullptr && outp != nullptr && ty != nullptr && tx != nullptr, "NULL pointer");
    for (const nerfail_resize_axis* a : {ty, tx})
        RS_REQUIRE(a->start != nullptr && a->count != nullptr && a->w != nullptr && a->ostart != nullptr && a->ocount != nullptr,
                   "NULL table pointer");
    RS_REQUIRE(ty->n_in == H && ty->n_out == oh && tx->n_in == W && tx->n_out == ow, "ty / tx are not the tables of H -> oh / W -> ow");
    RS_REQUIRE(ty->kmax >= 1 && ty->kmax <= kResizeTaps && tx->kmax >= 1 && tx->kmax <= kResizeTaps, "kmax must be in 1..16");
    *hy = host_axis(H, oh);
    *hx = host_axis(W, ow, *hy);
    RS_REQUIRE((*hy)->ok && (*hx)->ok, "an axis takes more than 16 taps");
    RS_REQUIRE(ty->kmax >= (*hy)->kmax && tx->kmax >= (*hx)->kmax, "kmax is below the axis' largest count");
    // the image side: src of the forward, gsrc of the adjoint; the planar side: out of the forward, g of the adjoint
    const void* image = in_is_image ? in : outp;
    const void* planar = in_is_image ? outp : in;
    RS_REQUIRE(resize_aligned(image, layout == 0 ? 16 : 4), "the image must be 16-byte aligned (layout 0) or 4-byte aligned (layout 1)");
    RS_REQUIRE(resize_aligned(planar, 4), "the resized tensor must be 4-byte aligned");
    return NERFAIL_OK;
#undef RS_REQUIRE
}

extern "C" int nerfail_cls_input_resize_fwd(const float* src, int layout, int B, int H, int W, int oh, int ow,
                                            const nerfail_resize_axis* ty, const nerfail_resize_axis* tx, float* out, void* stream) {
    const HostAxis *hy, *hx;
    const int rc = resize_check(__func__, src, out, layout, B, H, W, oh, ow, ty, tx, true, &hy, &hx);
    if (rc != NERFAIL_OK) return rc;
    const ResizePlan p = plan_fwd(hy, hx);
    NF_REQUIRE(p.lds <= (size_t)kResizeLds, "no tile fits the LDS");
    const dim3 grid((unsigned)((ow + p.t1 - 1) / p.t1), (unsigned)((oh + p.t0 - 1) / p.t0), (unsigned)B);
    NF_REQUIRE(grid.y <= 65535, "oh / tile rows must be <= 65535");
    {   // every call: the attribute belongs to the current device, and the call is a cheap host-side one
        const int e = layout == 0 ? allow_lds(cls_input_resize_fwd_kernel<0>, "cls_input_resize_fwd_kernel")
                                  : allow_lds(cls_input_resize_fwd_kernel<1>, "cls_input_resize_fwd_kernel");
        if (e != NERFAIL_OK) return e;
    }
    const AxisDev ay = axis_dev(ty), ax = axis_dev(tx);
    if (layout == 0)
        cls_input_resize_fwd_kernel<0><<<grid, dim3(kResizeThreads), p.lds, as_stream(stream)>>>(src, H, W, oh, ow, ay, ax, p.t0, p.t1, p.w0,
                                                                                                  p.w1, p.stride, out);
    else
        cls_input_resize_fwd_kernel<1><<<grid, dim3(kResizeThreads), p.lds, as_stream(stream)>>>(src, H, W, oh, ow, ay, ax, p.t0, p.t1, p.w0,
                                                                                                  p.w1, p.stride, out);
    NF_LAUNCHED("cls_input_resize_fwd_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_cls_input_resize_bwd(const float* g, int R, const float* src, int layout, int B, int H, int W, int oh, int ow,
                                            const nerfail_resize_axis* ty, const nerfail_resize_axis* tx, float* gsrc, void* stream) {
    NF_REQUIRE(R >= 1 && R <= 8, "R must be in 1..8");
    const HostAxis *hy, *hx;
    const int rc = resize_check(__func__, g, gsrc, layout, B, H, W, oh, ow, ty, tx, false, &hy, &hx);
    if (rc != NERFAIL_OK) return rc;
    NF_REQUIRE(layout != 0 || (src != nullptr && resize_aligned(src, 16)), "layout 0 needs src (16-byte aligned) for the alpha test");
    const ResizePlan p = plan_bwd(hy, hx);
    NF_REQUIRE(p.lds <= (size_t)kResizeLds, "no tile fits the LDS");
    const dim3 grid((unsigned)((W + p.t1 - 1) / p.t1), (unsigned)((H + p.t0 - 1) / p.t0), (unsigned)B);
    NF_REQUIRE(grid.y <= 65535, "H / tile rows must be <= 65535");
    {   // every call: the attribute belongs to the current device, and the call is a cheap host-side one
        const int e = layout == 0 ? allow_lds(cls_input_resize_bwd_kernel<0>, "cls_input_resize_bwd_kernel")
                                  : allow_lds(cls_input_resize_bwd_kernel<1>, "cls_input_resize_bwd_kernel");
        if (e != NERFAIL_OK) return e;
    }
    const AxisDev ay = axis_dev(ty), ax = axis_dev(tx);
    if (layout == 0)
        cls_input_resize_bwd_kernel<0><<<grid, dim3(kResizeThreads), p.lds, as_stream(stream)>>>(g, R, src, B, H, W, oh, ow, ay, ax, p.t0, p.t1,
                                                                                                  p.w0, p.w1, p.stride, gsrc);
    else
        cls_input_resize_bwd_kernel<1><<<grid, dim3(kResizeThreads), p.lds, as_stream(stream)>>>(g, R, src, B, H, W, oh, ow, ay, ax, p.t0, p.t1,
                                                                                                  p.w0, p.w1, p.stride, gsrc);
    NF_LAUNCHED("cls_input_resize_bwd_kernel");
    return NERFAIL_OK;
}
