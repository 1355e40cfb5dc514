// The f32 weight images of the fused NeRF MLP, packed from the nn.Linear tensors: the forward image (MlpLayout: A fragments in
// the k order weight_column() states, bias pieces, alpha / rgb heads) and the transposed image of the backward-data pass
// (MlpLayoutT). One kernel: a table of jobs passed by value, a block row (blockIdx.y) per job, grid-striding over the job's
// elements. nerfail_mlp_pack fills in the forward layers and the heads, nerfail_mlp_pack_T the transposed layers,
// nerfail_mlp_pack_train (once per network and training step) all of them.
// The fp16 hi/lo images are packed in mlp_f16.hip (from the same maps and the same layer table, mlp_layout.h), the bf16x3 image
// is split on the device from the forward image (mlp_x3.hip).
#include "mlp_layout.h"

namespace nerfail {

struct PackJob { MlpLayerDesc d; int total; unsigned w_off, b_off; };      // total = elements of the layer's weight image
struct PackHeads { const float* aw; const float* ab; const float* rw; const float* rb; unsigned alpha_off, rgb_off; };
struct PackJobs {
    int NT, nF, nH, nT;                      // jobs in blockIdx.y order: nF forward layers, nH (0 | 1) heads, nT transposed layers
    PackHeads h;
    PackJob f[NERFAIL_MAX_DEPTH + 2], t[NERFAIL_MAX_DEPTH + 2];
};

// element g of a forward layer: bias image [OT][2][16] and A fragments [quad q][out-tile][lane][e] of k-step 4q + e
__device__ __forceinline__ void pack_fwd_element(const PackJob& j, int NT, int g, float* __restrict__ packed) {
    const MlpLayerDesc& d = j.d;
    if (g < d.OT * 32) {
        const int ch = 32 * (g / 32) + acc_channel(g & 15, (g / 16) & 1);
        packed[j.b_off + g] = (ch < d.out_f) ? d.b[ch] : 0.f;
    }
    if (g >= j.total) return;
    const int e = g & 3, lane = (g >> 2) & 63, rest = g >> 8;
    const int row = 32 * (rest % d.OT) + (lane & 31);
    const int col = weight_column(d.emb0, d.h0, d.dir0, NT, 4 * (rest / d.OT) + e, lane >> 5);
    packed[j.w_off + g] = (row < d.out_f && col >= 0) ? d.w[(long)row * d.in_f + col] : 0.f;
}

// element g of the heads: alpha image [NT][2][16] + bias, rgb image [3][OTV][2][16] + 3 biases
__device__ __forceinline__ void pack_heads_element(const PackHeads& h, int NT, int g, float* __restrict__ packed) {
    const int OTV = NT / 2;
    float* __restrict__ aq = packed + h.alpha_off;
    float* __restrict__ rq = packed + h.rgb_off;
    if (g < NT * 32) {
        aq[g] = h.aw[32 * (g / 32) + acc_channel(g & 15, (g / 16) & 1)];
    } else if (g < NT * 32 + 4) {
        aq[g] = (g == NT * 32) ? h.ab[0] : 0.f;
    }
    if (g < 3 * OTV * 32) {
        const int c = g / (OTV * 32), rem = g % (OTV * 32);
        rq[g] = h.rw[c * (16 * NT) + 32 * (rem / 32) + acc_channel(rem & 15, (rem / 16) & 1)];
    } else if (g < 3 * OTV * 32 + 4) {
        const int c = g - 3 * OTV * 32;
        rq[g] = (c < 3) ? h.rb[c] : 0.f;
    }
}

// element g of a transposed layer, [quad q][in-tile t][lane (i = l&31 -> input channel 32t + i, h = l>>5)][e]:
// W[out channel of k-step 4q + e in half h][h0 + 32t + i]
__device__ __forceinline__ void pack_T_element(const PackJob& j, int NT, int g, float* __restrict__ packedT) {
    const MlpLayerDesc& d = j.d;
    const int e = g & 3, lane = (g >> 2) & 63, rest = g >> 8;
    const int o = hidden_channel(4 * (rest / NT) + e, lane >> 5);
    const int i = 32 * (rest % NT) + (lane & 31);
    packedT[j.w_off + g] = (o < d.out_f) ? d.w[(long)o * d.in_f + d.h0 + i] : 0.f;
}

__global__ void pack_kernel(PackJobs t, float* __restrict__ packed, float* __restrict__ packedT) {
    const int job = blockIdx.y, NT = t.NT;
    const int stride = gridDim.x * blockDim.x, g0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (job < t.nF) {
        const PackJob& j = t.f[job];
        const int n = j.total > j.d.OT * 32 ? j.total : j.d.OT * 32;
        for (int g = g0; g < n; g += stride) pack_fwd_element(j, NT, g, packed);
    } else if (job < t.nF + t.nH) {
        for (int g = g0; g < NT * 32 + 4 || g < 3 * (NT / 2) * 32 + 4; g += stride) pack_heads_element(t.h, NT, g, packed);
    } else {
        const PackJob& j = t.t[job - t.nF - t.nH];
        for (int g = g0; g < j.total; g += stride) pack_T_element(j, NT, g, packedT);
    }
}

static int launch_pack(const PackJobs& t, float* packed, float* packedT, void* stream) {
    pack_kernel<<<dim3(32, (unsigned)(t.nF + t.nH + t.nT)), dim3(256), 0, as_stream(stream)>>>(t, packed, packedT);
    NF_LAUNCHED("pack_kernel");
    return NERFAIL_OK;
}

}  // namespace nerfail

using namespace nerfail;

extern "C" size_t nerfail_mlp_packed_floats(int D, int W, int skip) {
    MlpLayout L;
    return make_layout(D, W, skip, L) ? (size_t)L.total : 0;
}

extern "C" size_t nerfail_mlp_packed_T_floats(int D, int W, int skip) {
    MlpLayout L;
    if (!make_layout(D, W, skip, L)) return 0;
    MlpLayoutT T;
    make_layout_T(D, L.NT, T);
    return (size_t)T.total;
}

// the forward jobs (layers + heads) of a complete parameter set
static int fill_pack_table(const nerfail_mlp_params* p, MlpLayout& L, PackJobs& t) {
    NF_REQUIRE(p->input_ch == kPtsCh && p->input_ch_views == kDirCh, "only multires=10 / multires_views=4 (63 + 27 channels)");
    NF_REQUIRE(make_layout(p->D, p->W, p->skip, L), "unsupported (D, W): W in {64,128,256}, 2 <= D <= 16");
    for (int i = 0; i < p->D; ++i) NF_REQUIRE(p->pts_w[i] != nullptr && p->pts_b[i] != nullptr, "pts_linears pointer is NULL");
    NF_REQUIRE(p->views_w && p->views_b && p->feature_w && p->feature_b && p->alpha_w && p->alpha_b && p->rgb_w && p->rgb_b,
               "head pointer is NULL");
    t.NT = L.NT; t.nF = p->D + 2; t.nH = 1; t.nT = 0;
    for (int l = 0; l <= p->D + 1; ++l) t.f[l] = {mlp_layer(p, L, l), (int)L.w_count[l], L.w_off[l], L.b_off[l]};
    t.h = {p->alpha_w, p->alpha_b, p->rgb_w, p->rgb_b, L.alpha_off, L.rgb_off};
    return NERFAIL_OK;
}

// the transposed jobs: layers 1 .. D+1 (layer 0 has no hidden input), each at its place in the backward pass's stream
static void fill_pack_table_T(const nerfail_mlp_params* p, const MlpLayout& L, PackJobs& t) {
    MlpLayoutT T;
    make_layout_T(L.D, L.NT, T);
    t.NT = L.NT; t.nT = L.D + 1;
    for (int l = 1; l <= L.D + 1; ++l) {
        const MlpLayerDesc d = mlp_layer(p, L, l);
        t.t[l - 1] = {d, d.OT * 4 * L.NT * 256, T.w_off[l], 0u};
    }
}

extern "C" int nerfail_mlp_pack(const nerfail_mlp_params* p, float* packed, void* stream) {
    NF_REQUIRE(p != nullptr && packed != nullptr, "NULL pointer");
    MlpLayout L;
    PackJobs t;
    const int rc = fill_pack_table(p, L, t);
    return rc != NERFAIL_OK ? rc : launch_pack(t, packed, nullptr, stream);
}

extern "C" int nerfail_mlp_pack_T(const nerfail_mlp_params* p, float* packedT, void* stream) {
    NF_REQUIRE(p != nullptr && packedT != nullptr, "NULL pointer");
    MlpLayout L;
    NF_REQUIRE(make_layout(p->D, p->W, p->skip, L), "unsupported (D, W)");
    PackJobs t;
    t.nF = 0; t.nH = 0;
    fill_pack_table_T(p, L, t);
    for (int l = 1; l <= L.D + 1; ++l) NF_REQUIRE(t.t[l - 1].d.w != nullptr, mlp_layer_null_msg(L, l));
    return launch_pack(t, nullptr, packedT, stream);
}

extern "C" int nerfail_mlp_pack_train(const nerfail_mlp_params* p, float* packed, float* packedT, void* stream) {
    NF_REQUIRE(p != nullptr && packed != nullptr && packedT != nullptr, "NULL pointer");
    MlpLayout L;
    PackJobs t;
    const int rc = fill_pack_table(p, L, t);
    if (rc != NERFAIL_OK) return rc;
    fill_pack_table_T(p, L, t);
    return launch_pack(t, packed, packedT, stream);
}
