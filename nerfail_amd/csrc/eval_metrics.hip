// Attack evaluation (model_test.py:226-348 = MT, MyDataset.py:93-113 = MD) on the device: what test_for_inception measures
// between every attacked view and its original - eps max / min / avg, the L2 and L0 distance, PSNR - plus the classifier's
// input tensor, the prediction and cross entropy of every view, and the set-level record the report is printed from. The
// reference makes ~15 full-image torch ops and a dozen host reads per view on the CPU; here ONE pass over an (attacked,
// original) pair yields the five distances and the NCHW classifier input, and a one-lane fold keeps the running record on the
// device: an evaluation of any number of views has one host read, at its end.
//
// Reproducibility (the rule of img_sqerr_kernel): no atomics anywhere. The element -> lane map and every order of summation
// depend on the element count of a view only - not on the storage format of either side, not on the other views of the launch,
// not on the run. A view's row is therefore the same bits as uint8 or float32 holding the same values, alone or in a batch.
#include "common.h"

namespace nerfail {

constexpr int kEvalViews = 16;               // view pairs per launch (pointer table passed by value)
constexpr int kEvalBlocksPerView = 128;      // 16 views x 128 = 2048 workgroups: the grid cap of a streaming kernel
constexpr int kEvalPartial = 5;              // max, min, sum, sum of squares, non-zero count
constexpr double kPsnrIdentical = 361.20199909921956;      // 20 log10(255 / DBL_EPSILON): get_psnr of two equal images (MT:36-39)
constexpr int kEvalUnit = 3;                 // elements per lane and step: the three channels of one pixel

struct EvalViews {
    const void* a[kEvalViews];
    const void* o[kEvalViews];
};

// The elements 3 u .. 3 u + ne - 1 of one side after the white background of MT:237-254 (4-channel formats: rgb where
// alpha > 0, else 255; a NaN alpha fails the comparison and gives white). Image formats: unit u = pixel u, ne = 3. Consecutive
// lanes take consecutive units, so a wave reads one contiguous piece of the image per instruction: 1 KB of F32C4 (128 bits per
// lane), 256 B of U8C4 (one dword per lane), 192 B of U8C3. A U8C3 pixel starts at byte 3 u: the lane loads the two aligned
// dwords that hold it and shifts, unless the second dword would reach to or beyond byte `bytes` = 3 P of the view - then (the
// last pixels of a view only) byte loads. Nothing at or beyond element ne is read; v[ne..] is left 0.
template <int F>
__device__ __forceinline__ void load_unit(const void* __restrict__ base, long u, int ne, long bytes, float v[kEvalUnit]) {
    v[0] = v[1] = v[2] = 0.f;
    if (F == NERFAIL_EVAL_U8C4) {
        const unsigned w = reinterpret_cast<const unsigned*>(base)[u];
        v[0] = white_u8(w, 0);
        v[1] = white_u8(w, 8);
        v[2] = white_u8(w, 16);
    } else if (F == NERFAIL_EVAL_F32C4) {
        const float4 p = reinterpret_cast<const float4*>(base)[u];
        const bool keep = p.w > 0.f;
        v[0] = keep ? p.x : 255.f;
        v[1] = keep ? p.y : 255.f;
        v[2] = keep ? p.z : 255.f;
    } else if (F == NERFAIL_EVAL_U8C3) {
        const long b = 3 * u, word = b >> 2;
        if (4 * word + 8 <= bytes) {
            const unsigned* w = reinterpret_cast<const unsigned*>(base) + word;
            const unsigned long long both = ((unsigned long long)w[1] << 32) | (unsigned long long)w[0];
            const unsigned px = (unsigned)(both >> (8 * (int)(b & 3)));
            v[0] = (float)(px & 255u);
            v[1] = (float)((px >> 8) & 255u);
            v[2] = (float)((px >> 16) & 255u);
        } else {
            const unsigned char* c = reinterpret_cast<const unsigned char*>(base) + b;
            v[0] = (float)c[0];
            v[1] = (float)c[1];
            v[2] = (float)c[2];
        }
    } else {                                                               // FLAT: three consecutive elements, fewer at the end
        const float* f = reinterpret_cast<const float*>(base) + 3 * u;
#pragma unroll
        for (int j = 0; j < kEvalUnit; ++j)
            if (j < ne) v[j] = f[j];
    }
}

// grid = (workgroups per view, views). Lane t of workgroup k takes units k * 256 + t, + gridDim.x * 256, ... of its view and
// folds their elements in order; E = the view's element count (3 P, or n for FLAT).
template <int FA, int FO>
__global__ __launch_bounds__(256) void eval_view_metrics_kernel(EvalViews tab, long E, long P, double* __restrict__ partials,
                                                                float* __restrict__ cla_in) {
    __shared__ double w_s[4], w_s2[4], w_nz[4];
    __shared__ float w_mx[4], w_mn[4];
    __shared__ int w_nan[4];
    const void* ab = tab.a[blockIdx.y];
    const void* ob = tab.o[blockIdx.y];
    float* cla = cla_in ? cla_in + (long)blockIdx.y * 3 * P : nullptr;
    const long units = (E + kEvalUnit - 1) / kEvalUnit;
    const long stride = (long)gridDim.x * 256;
    float mx = -INFINITY, mn = INFINITY;
    double s = 0.0, s2 = 0.0;
    int nz = 0;
    bool nan = false;
#pragma unroll 4
    for (long u = (long)blockIdx.x * 256 + threadIdx.x; u < units; u += stride) {
        const long left = E - u * kEvalUnit;
        const int ne = (FA != NERFAIL_EVAL_FLAT || left >= kEvalUnit) ? kEvalUnit : (int)left;
        float a[kEvalUnit], o[kEvalUnit];
        load_unit<FA>(ab, u, ne, E, a);                                   // E = 3 P = the bytes of a U8C3 view
        load_unit<FO>(ob, u, ne, E, o);
#pragma unroll
        for (int j = 0; j < kEvalUnit; ++j) {
            if (j < ne) {
                const float d = fabsf(__fsub_rn(a[j], o[j]));
                const double dd = (double)d;
                nan = nan || (d != d);
                mx = fmaxf(mx, d);
                mn = fminf(mn, d);
                s += dd;
                s2 = fma(dd, dd, s2);
                nz += (d != 0.f) ? 1 : 0;                                  // a NaN counts, as torch.count_nonzero counts it
            }
        }
        if (FA != NERFAIL_EVAL_FLAT && cla != nullptr) {                   // planar: consecutive lanes, consecutive floats
            cla[u] = a[0];
            cla[P + u] = a[1];
            cla[2 * P + u] = a[2];
        }
    }
    mx = wave_max(mx);
    mn = wave_min(mn);
    s = wave_sum_f64(s);
    s2 = wave_sum_f64(s2);
    const double nzw = wave_sum_f64((double)nz);                           // integers below 2^53: exact in any order
    const int any_nan = __any(nan ? 1 : 0);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        w_mx[w] = mx;
        w_mn[w] = mn;
        w_s[w] = s;
        w_s2[w] = s2;
        w_nz[w] = nzw;
        w_nan[w] = any_nan;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* p = partials + ((long)blockIdx.y * gridDim.x + blockIdx.x) * kEvalPartial;
        const bool bn = (w_nan[0] | w_nan[1] | w_nan[2] | w_nan[3]) != 0;
        p[0] = bn ? (double)NAN : (double)fmaxf(fmaxf(w_mx[0], w_mx[1]), fmaxf(w_mx[2], w_mx[3]));
        p[1] = bn ? (double)NAN : (double)fminf(fminf(w_mn[0], w_mn[1]), fminf(w_mn[2], w_mn[3]));
        p[2] = ((w_s[0] + w_s[1]) + w_s[2]) + w_s[3];
        p[3] = ((w_s2[0] + w_s2[1]) + w_s2[2]) + w_s2[3];
        p[4] = ((w_nz[0] + w_nz[1]) + w_nz[2]) + w_nz[3];
    }
}

// one wave per view: its workgroups' partials in a fixed order -> the row {max, min, sum, sum of squares, non-zero, elements}
__global__ __launch_bounds__(64) void eval_view_finish_kernel(const double* __restrict__ partials, int per_view, double elements,
                                                              double* __restrict__ rows) {
    const double* p = partials + (long)blockIdx.x * per_view * kEvalPartial;
    double mx = -INFINITY, mn = INFINITY, s = 0.0, s2 = 0.0, nz = 0.0;
    bool nan = false;
    for (int i = threadIdx.x; i < per_view; i += 64) {
        const double pm = p[i * kEvalPartial];
        nan = nan || (pm != pm);
        mx = fmax(mx, pm);
        mn = fmin(mn, p[i * kEvalPartial + 1]);
        s += p[i * kEvalPartial + 2];
        s2 += p[i * kEvalPartial + 3];
        nz += p[i * kEvalPartial + 4];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mx = fmax(mx, __shfl_xor(mx, o, 64));
        mn = fmin(mn, __shfl_xor(mn, o, 64));
    }
    s = wave_sum_f64(s);
    s2 = wave_sum_f64(s2);
    nz = wave_sum_f64(nz);
    const bool any_nan = __any(nan ? 1 : 0) != 0;
    if (threadIdx.x == 0) {
        double* r = rows + (long)blockIdx.x * NERFAIL_EVAL_VIEW_DOUBLES;
        r[0] = any_nan ? (double)NAN : mx;
        r[1] = any_nan ? (double)NAN : mn;
        r[2] = s;
        r[3] = s2;
        r[4] = nz;
        r[5] = elements;
    }
}

// ---- MT:292-295: the prediction and the CE of every view, one wave; lane l takes views l, l + 64, ...
__global__ __launch_bounds__(64) void eval_logit_stats_kernel(const float* __restrict__ logits, int B, int C, int label,
                                                              int* __restrict__ pred, double* __restrict__ ce) {
    for (int b = threadIdx.x; b < B; b += 64) {
        const LogitRow r = logit_row_stats(logits + (long)b * C, C, label);
        pred[b] = r.arg;
        ce[b] = r.ce;
    }
}

// max / min that keep a NaN once they have seen one (torch.max / torch.min of MT:269-271 do)
__device__ __forceinline__ double nan_max(double m, double v) { return (m != m || v != v) ? (double)NAN : fmax(m, v); }
__device__ __forceinline__ double nan_min(double m, double v) { return (m != m || v != v) ? (double)NAN : fmin(m, v); }

// ---- MT:268-278, 298-299, 341-348: one lane folds a batch into the set record. record[0] (views so far) == 0 marks the first
// batch: the minima and maxima are then taken from the first view instead of from the zeroed record.
__global__ __launch_bounds__(64) void eval_fold_kernel(const double* __restrict__ rows, const int* __restrict__ pred,
                                                       const double* __restrict__ ce, int B, int C, double* __restrict__ rec) {
    if (threadIdx.x != 0) return;
    double views = rec[0];
    double e_max = rec[1], e_min = rec[2], e_avg = rec[3], l2 = rec[4], l0 = rec[5];
    double p_min = rec[6], p_max = rec[7], p_sum = rec[8], ce_sum = rec[9], none = rec[10], elems = rec[11];
    for (int b = 0; b < B; ++b) {
        const double* r = rows + (long)b * NERFAIL_EVAL_VIEW_DOUBLES;
        const double n = r[5];
        const double rmse = sqrt(r[3] / n);
        const double psnr = rmse == 0.0 ? kPsnrIdentical : 20.0 * log10(255.0 / rmse);      // get_psnr, MT:36-39
        const bool first = (views == 0.0);
        e_max = first ? r[0] : nan_max(e_max, r[0]);
        e_min = first ? r[1] : nan_min(e_min, r[1]);
        p_max = first ? psnr : nan_max(p_max, psnr);
        p_min = first ? psnr : nan_min(p_min, psnr);
        e_avg += r[2] / n;
        l2 += sqrt(r[3]);
        l0 += r[4];
        p_sum += psnr;
        ce_sum += ce[b];
        elems += n;
        const int k = pred[b];
        if (k >= 0 && k < C) rec[16 + k] += 1.0;
        else none += 1.0;
        views += 1.0;
    }
    rec[0] = views;
    rec[1] = e_max;
    rec[2] = e_min;
    rec[3] = e_avg;
    rec[4] = l2;
    rec[5] = l0;
    rec[6] = p_min;
    rec[7] = p_max;
    rec[8] = p_sum;
    rec[9] = ce_sum;
    rec[10] = none;
    rec[11] = elems;
}

static bool eval_format_ok(int f) { return f >= NERFAIL_EVAL_U8C4 && f <= NERFAIL_EVAL_FLAT; }
static uintptr_t eval_align_mask(int f) { return f == NERFAIL_EVAL_F32C4 ? 15 : 3; }

template <int FA, int FO>
static void launch_view_metrics(dim3 grid, hipStream_t st, const EvalViews& tab, long E, long P, double* partials, float* cla) {
    eval_view_metrics_kernel<FA, FO><<<grid, dim3(256), 0, st>>>(tab, E, P, partials, cla);
}

}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_eval_revision(void) { return 1; }

extern "C" size_t nerfail_eval_scratch_bytes(void) {
    return (size_t)kEvalViews * kEvalBlocksPerView * kEvalPartial * sizeof(double);
}

extern "C" int nerfail_eval_view_metrics(const void* const* a_views_host, int a_format, const void* const* o_views_host, int o_format,
                                         int n_views, int64_t P, void* scratch, double* rows, float* cla_in, void* stream) {
    NF_REQUIRE(n_views >= 0 && P >= 0, "negative size");
    NF_REQUIRE(eval_format_ok(a_format) && eval_format_ok(o_format), "unknown image format");
    NF_REQUIRE((a_format == NERFAIL_EVAL_FLAT) == (o_format == NERFAIL_EVAL_FLAT), "FLAT pairs only with FLAT");
    NF_REQUIRE(cla_in == nullptr || a_format != NERFAIL_EVAL_FLAT, "cla_in is not available for FLAT");
    if ((int64_t)n_views * P == 0) return NERFAIL_OK;
    NF_REQUIRE(a_views_host != nullptr && o_views_host != nullptr && scratch != nullptr && rows != nullptr, "NULL pointer");
    NF_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0 && (reinterpret_cast<uintptr_t>(rows) & 7) == 0,
               "scratch and rows must be 8-byte aligned");
    NF_REQUIRE((reinterpret_cast<uintptr_t>(cla_in) & 3) == 0, "cla_in is not 4-byte aligned");
    for (int v = 0; v < n_views; ++v) {
        NF_REQUIRE(a_views_host[v] != nullptr && o_views_host[v] != nullptr, "a view has a NULL image");
        NF_REQUIRE((reinterpret_cast<uintptr_t>(a_views_host[v]) & eval_align_mask(a_format)) == 0,
                   "an attacked view is not aligned for its format (U8C4, U8C3, FLAT: 4 bytes; F32C4: 16)");
        NF_REQUIRE((reinterpret_cast<uintptr_t>(o_views_host[v]) & eval_align_mask(o_format)) == 0,
                   "an original view is not aligned for its format (U8C4, U8C3, FLAT: 4 bytes; F32C4: 16)");
    }
    const long E = a_format == NERFAIL_EVAL_FLAT ? (long)P : 3 * (long)P;
    const long units = (E + kEvalUnit - 1) / kEvalUnit;
    long bx = (units + 1023) / 1024;                                       // >= 4 pixels per lane; a function of the view size alone
    bx = bx > kEvalBlocksPerView ? kEvalBlocksPerView : (bx < 1 ? 1 : bx);
    hipStream_t st = as_stream(stream);
    for (int v0 = 0; v0 < n_views; v0 += kEvalViews) {
        EvalViews tab;
        const int nv = n_views - v0 < kEvalViews ? n_views - v0 : kEvalViews;
        for (int i = 0; i < kEvalViews; ++i) {
            tab.a[i] = a_views_host[v0 + (i < nv ? i : 0)];
            tab.o[i] = o_views_host[v0 + (i < nv ? i : 0)];
        }
        const dim3 grid((unsigned)bx, (unsigned)nv);
        double* partials = (double*)scratch;
        float* cla = cla_in ? cla_in + (int64_t)v0 * 3 * P : nullptr;
#define NF_EVAL_CASE(FA, FO)                                                          \
    if (a_format == FA && o_format == FO) launch_view_metrics<FA, FO>(grid, st, tab, E, (long)P, partials, cla)
        NF_EVAL_CASE(NERFAIL_EVAL_U8C4, NERFAIL_EVAL_U8C4);
        NF_EVAL_CASE(NERFAIL_EVAL_U8C4, NERFAIL_EVAL_U8C3);
        NF_EVAL_CASE(NERFAIL_EVAL_U8C4, NERFAIL_EVAL_F32C4);
        NF_EVAL_CASE(NERFAIL_EVAL_U8C3, NERFAIL_EVAL_U8C4);
        NF_EVAL_CASE(NERFAIL_EVAL_U8C3, NERFAIL_EVAL_U8C3);
        NF_EVAL_CASE(NERFAIL_EVAL_U8C3, NERFAIL_EVAL_F32C4);
        NF_EVAL_CASE(NERFAIL_EVAL_F32C4, NERFAIL_EVAL_U8C4);
        NF_EVAL_CASE(NERFAIL_EVAL_F32C4, NERFAIL_EVAL_U8C3);
        NF_EVAL_CASE(NERFAIL_EVAL_F32C4, NERFAIL_EVAL_F32C4);
        NF_EVAL_CASE(NERFAIL_EVAL_FLAT, NERFAIL_EVAL_FLAT);
#undef NF_EVAL_CASE
        NF_LAUNCHED("eval_view_metrics_kernel");
        eval_view_finish_kernel<<<dim3((unsigned)nv), dim3(64), 0, st>>>(partials, (int)bx, (double)E,
                                                                         rows + (int64_t)v0 * NERFAIL_EVAL_VIEW_DOUBLES);
        NF_LAUNCHED("eval_view_finish_kernel");
    }
    return NERFAIL_OK;
}

extern "C" int nerfail_eval_logit_stats(const float* logits, int B, int C, int label, int32_t* pred, double* ce, void* stream) {
    NF_REQUIRE(B >= 0, "B is negative");
    NF_REQUIRE(C >= 1 && C <= NERFAIL_ATTACK_MAX_CLASSES, "C must be 1..32");
    NF_REQUIRE(label >= 0 && label < C, "label must be a class index");
    if (B == 0) return NERFAIL_OK;
    NF_REQUIRE(logits != nullptr && pred != nullptr && ce != nullptr, "NULL pointer");
    NF_REQUIRE((reinterpret_cast<uintptr_t>(ce) & 7) == 0, "ce must be 8-byte aligned");
    eval_logit_stats_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(logits, B, C, label, pred, ce);
    NF_LAUNCHED("eval_logit_stats_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_eval_fold(const double* rows, const int32_t* pred, const double* ce, int B, int C, double* record, void* stream) {
    NF_REQUIRE(B >= 0, "B is negative");
    NF_REQUIRE(C >= 1 && C <= NERFAIL_ATTACK_MAX_CLASSES, "C must be 1..32");
    if (B == 0) return NERFAIL_OK;
    NF_REQUIRE(rows != nullptr && pred != nullptr && ce != nullptr && record != nullptr, "NULL pointer");
    NF_REQUIRE((reinterpret_cast<uintptr_t>(rows) & 7) == 0 && (reinterpret_cast<uintptr_t>(ce) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(record) & 7) == 0, "rows, ce and record must be 8-byte aligned");
    eval_fold_kernel<<<dim3(1), dim3(64), 0, as_stream(stream)>>>(rows, pred, ce, B, C, record);
    NF_LAUNCHED("eval_fold_kernel");
    return NERFAIL_OK;
}
