// Foreground-only scene maps (fg revision 1): the pixels of a view that the attacks read - alpha > 0 in its registered BGRA image,
// gauss_net's rule (gauss.hip) - as a list, rays for that list, and the 8-NN search with K9's epilogue over that list.
//   nerfail_fg_pixel_list            ordered stream compaction of one uint8 BGRA view: three streaming launches, no atomics
//   nerfail_ray_gen_list             ray_gen_kernel's row (ray_pixel.h) for pixel pix[j]
//   nerfail_knn8_grid_weights_list   the [2,P,8] map zeroed, then knn8_grid_kernel's list instantiation scatters row j to pix[j]
// Everything here is HBM-bound streaming; the search itself is knn_grid.hip's kernel (knn_grid_list.h).
#include "common.h"
#include "ray_pixel.h"
#include "knn_grid_list.h"

namespace nerfail {

constexpr int kFgBlock = 256;                 // pixels per workgroup of the count and write kernels: one per thread, 4 waves

static inline size_t fg_al256(size_t v) { return (v + 255) & ~(size_t)255; }
static inline long fg_blocks(int64_t n_pixels) { return (long)((n_pixels + kFgBlock - 1) / kFgBlock); }

// alpha of pixel p as a flag (p >= n: 0). One 4-byte load per lane, a wave reads 256 consecutive bytes.
__device__ __forceinline__ bool fg_flag(const uint32_t* __restrict__ bgra, long p, long n) {
    return p < n && (bgra[p] >> 24) > 0u;     // little endian: byte 3 is A
}

// Pass 1: foreground pixels per workgroup. Ballot and popcount per wave, the four wave counts added through LDS.
__global__ __launch_bounds__(kFgBlock) void fg_count_kernel(const uint32_t* __restrict__ bgra, long n, int32_t* __restrict__ counts) {
    __shared__ int wave_n[kFgBlock / kWave];
    const long p = (long)blockIdx.x * kFgBlock + threadIdx.x;
    const unsigned long long m = __ballot(fg_flag(bgra, p, n));
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
}

// Pass 2: exclusive scan of the workgroup counts in place, one workgroup; *total = n. Thread t owns the contiguous run
// [t * per, (t + 1) * per): its sum, a scan of the 256 sums (wave scan, then the 4 wave totals), then the run again.
__global__ __launch_bounds__(256) void fg_scan_kernel(int32_t* __restrict__ counts, long nb, int32_t* __restrict__ total) {
    __shared__ int wave_tot[4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long per = (nb + 255) / 256;
    const long b = min((long)t * per, nb), e = min(b + per, nb);
    int sum = 0;
    for (long i = b; i < e; ++i) sum += counts[i];
    int inc = sum;                                        // inclusive scan across the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wave_tot[wv] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; ++w) base += wave_tot[w];
    int run = base + inc - sum;                           // exclusive prefix of this thread's run
    for (long i = b; i < e; ++i) {
        const int c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (t == 255) *total = base + inc;
}

// Pass 3: the write. The same ballots as pass 1; a set lane's slot is its workgroup's offset + the waves before it + the set
// lanes below it in its wave: ascending pixel order whatever the device schedules.
__global__ __launch_bounds__(kFgBlock) void fg_write_kernel(const uint32_t* __restrict__ bgra, long n, const int32_t* __restrict__ offsets,
                                                            int32_t* __restrict__ list) {
    __shared__ int wave_n[kFgBlock / kWave];
    const long p = (long)blockIdx.x * kFgBlock + threadIdx.x;
    const bool f = fg_flag(bgra, p, n);
    const unsigned long long m = __ballot(f);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wave_n[wv] = __popcll(m);
    __syncthreads();
    if (!f) return;
    int at = offsets[blockIdx.x];
    for (int w = 0; w < wv; ++w) at += wave_n[w];
    at += __popcll(m & ((1ull << lane) - 1ull));
    list[at] = (int32_t)p;
}

__global__ void ray_gen_list_kernel(Cam c, int W, const int32_t* __restrict__ pix, long n, float near_, float far_,
                                    float* __restrict__ rays) {
    const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long p = (long)pix[j];
    float o[3], d[3];
    pixel_ray(c, (int)(p % W), (int)(p / W), o, d);       // ray_gen_kernel's two calls for pixel p
    store_ray(rays + NERFAIL_RAY_FLOATS * j, o, d, near_, far_);
}

// +0 over n16 16-byte words: the [2,P,8] map before the scatter (64 bytes per pixel: 41 MB per 800 x 800 view).
__global__ __launch_bounds__(256) void fg_zero_kernel(float4* __restrict__ out, long n16) {
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) out[i] = z;
}

}  // namespace nerfail

using namespace nerfail;

extern "C" int nerfail_fg_revision(void) { return 1; }

extern "C" size_t nerfail_fg_pixel_list_workspace_bytes(int64_t n_pixels) {
    if (n_pixels <= 0 || n_pixels >= ((int64_t)1 << 31)) return 0;
    return fg_al256((size_t)fg_blocks(n_pixels) * sizeof(int32_t));
}

extern "C" int nerfail_fg_pixel_list(const uint8_t* bgra, int64_t n_pixels, int32_t* list, int32_t* count, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    NF_REQUIRE(n_pixels > 0 && n_pixels < ((int64_t)1 << 31), "n_pixels must be in [1, 2^31)");
    NF_REQUIRE(bgra != nullptr && list != nullptr && count != nullptr, "NULL pointer");
    NF_REQUIRE(((reinterpret_cast<uintptr_t>(bgra) | reinterpret_cast<uintptr_t>(list) | reinterpret_cast<uintptr_t>(count)) & 3) == 0,
               "bgra / list / count must be 4-byte aligned");
    NF_REQUIRE(workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0 &&
                   workspace_bytes >= nerfail_fg_pixel_list_workspace_bytes(n_pixels),
               "workspace too small (nerfail_fg_pixel_list_workspace_bytes)");
    hipStream_t s = as_stream(stream);
    const long nb = fg_blocks(n_pixels);
    const uint32_t* px = reinterpret_cast<const uint32_t*>(bgra);
    int32_t* counts = reinterpret_cast<int32_t*>(workspace);
    fg_count_kernel<<<dim3((unsigned)nb), dim3(kFgBlock), 0, s>>>(px, n_pixels, counts);
    NF_LAUNCHED("fg_count_kernel");
    fg_scan_kernel<<<dim3(1), dim3(256), 0, s>>>(counts, nb, count);
    NF_LAUNCHED("fg_scan_kernel");
    fg_write_kernel<<<dim3((unsigned)nb), dim3(kFgBlock), 0, s>>>(px, n_pixels, counts, list);
    NF_LAUNCHED("fg_write_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_ray_gen_list(int H, int W, const float* K4_host, const float* c2w_host, float near_, float far_,
                                    const int32_t* pix, int64_t n, float* rays, void* stream) {
    NF_REQUIRE(H > 0 && W > 0 && (int64_t)H * W < ((int64_t)1 << 31), "H and W must be positive, H * W below 2^31");
    NF_REQUIRE(n >= 0, "n is negative");
    if (n == 0) return NERFAIL_OK;
    NF_REQUIRE(pix != nullptr && rays != nullptr, "pix / rays is NULL");
    Cam c;
    NF_REQUIRE(fill_cam(c, K4_host, c2w_host), "K4_host / c2w_host is NULL");
    NF_REQUIRE((n + 255) / 256 < ((int64_t)1 << 31), "too many pixels for one launch");
    ray_gen_list_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream)>>>(c, W, pix, n, near_, far_, rays);
    NF_LAUNCHED("ray_gen_list_kernel");
    return NERFAIL_OK;
}

extern "C" int nerfail_knn8_grid_weights_list(const float* queries, int64_t n, const int32_t* pix, int64_t n_pixels, int64_t n_points,
                                              float c, float* weight_and_index, double* sum_d2, const void* grid_workspace,
                                              size_t grid_workspace_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    NF_REQUIRE(n_pixels > 0 && n_pixels < ((int64_t)1 << 31), "n_pixels must be in [1, 2^31)");
    NF_REQUIRE(n >= 0 && n <= n_pixels, "n must be in [0, n_pixels]");
    NF_REQUIRE(n_points >= NERFAIL_KNN && n_points < (1 << 24), "bad n_points");
    NF_REQUIRE(c > 0.f, "c must be positive");
    NF_REQUIRE(weight_and_index != nullptr && (n == 0 || (queries != nullptr && pix != nullptr)), "NULL pointer");
    NF_REQUIRE((reinterpret_cast<uintptr_t>(weight_and_index) & 15) == 0, "weight_and_index must be 16-byte aligned");
    NF_REQUIRE((reinterpret_cast<uintptr_t>(sum_d2) & 7) == 0, "sum_d2 must be 8-byte aligned");
    NF_REQUIRE(n == 0 || sum_d2 == nullptr ||
                   (workspace != nullptr && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 &&
                    workspace_bytes >= nerfail_knn8_grid_weights_workspace_bytes(n)),
               "workspace too small (nerfail_knn8_grid_weights_workspace_bytes)");
    const int rc = knn8_grid_list_check(n, n_points, grid_workspace, grid_workspace_bytes);
    if (rc != NERFAIL_OK) return rc;
    hipStream_t s = as_stream(stream);
    const long n16 = (long)n_pixels * 4;                      // 2 planes x 8 floats = 4 float4 per pixel
    const long zb = (n16 + 255) / 256;
    fg_zero_kernel<<<dim3((unsigned)(zb < 4096 ? zb : 4096)), dim3(256), 0, s>>>(reinterpret_cast<float4*>(weight_and_index), n16);
    NF_LAUNCHED("fg_zero_kernel");
    return knn8_grid_weights_list_launch(queries, n, pix, n_pixels, n_points, c, weight_and_index, sum_d2, grid_workspace,
                                         grid_workspace_bytes, workspace, s);
}
