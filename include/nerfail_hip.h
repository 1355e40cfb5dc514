/*
 * nerfail_hip.h - C ABI of libnerfail_hip.so: the MI355X (gfx950) implementation of the NeRFail
 * render-and-attack hot path.
 *
 * The reference (jiang-wenxiang/NeRFail) is pure Python/PyTorch and has no FFI of its own; its
 * boundary is a set of Python call signatures. Each entry point below names the reference
 * function (file:line, relative to the reference root) whose arithmetic it replaces; the Python
 * mirror of those signatures lives in nerfail_amd/ and binds this library with ctypes
 * (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 *   RN = Create_spatial_point_set/nerf_pytorch/run_nerf.py      RH = .../run_nerf_helpers.py
 *   NC = Create_spatial_point_set/nerf_to_coord.py              CI = .../create_index_and_dist.py
 *   GN = model/GaussNet.py    AS = attack_NeRFail_S.py          DW = tools/dist_to_weight.py
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer to float32 unless the parameter name ends in `_host`.
 *     Buffers are dense, row-major, 16-byte aligned (hipMalloc / torch allocations are).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream). Calls only enqueue
 *     work; they never synchronise and never allocate.
 *   - Inputs are borrowed and never written; outputs are fully overwritten unless stated.
 *   - Return value: 0 on success, otherwise a NERFAIL_E* code; nerfail_last_error() then returns a
 *     thread-local message (argument name or HIP error string).
 *   - All arithmetic is IEEE float32 (the MLP uses the exact-f32 MFMA v_mfma_f32_32x32x2_f32).
 */
#ifndef NERFAIL_HIP_H
#define NERFAIL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NERFAIL_ABI_VERSION 14

#define NERFAIL_OK 0
#define NERFAIL_EINVAL 1   /* bad argument (null pointer, size, unsupported shape) */
#define NERFAIL_EHIP 2     /* a HIP runtime call or kernel launch failed           */
#define NERFAIL_ENODEV 3   /* no gfx950 device visible                             */

#define NERFAIL_RAY_FLOATS 11      /* o(3) d(3) near far viewdir(3): RN:116-123      */
#define NERFAIL_KNN 8              /* top_number, CI:46                              */
#define NERFAIL_MAX_DEPTH 16

int nerfail_abi_version(void);
const char* nerfail_last_error(void);
/* name of the device the library will launch on ("gfx950..." expected); NERFAIL_ENODEV if none */
int nerfail_device_name(char* buf_host, size_t buf_len);

/* ------------------------------------------------------------------ rays (K1) ------------- */

/* get_rays, RH:157-166. K4_host = {fx, fy, cx, cy} (K[0][0], K[1][1], K[0][2], K[1][2]),
 * c2w_host = 12 floats, row-major [3,4]. Writes rays_o, rays_d as [H,W,3]. */
int nerfail_get_rays(int H, int W, const float* K4_host, const float* c2w_host,
                     float* rays_o, float* rays_d, void* stream);

/* Ray packing of render(), RN:102-123 (use_viewdirs=True, ndc=False): viewdirs = d/|d|;
 * rays[n, 11] = o, d, near, far, viewdirs. */
int nerfail_pack_rays(const float* rays_o, const float* rays_d, int64_t n, float near_, float far_,
                      float* rays, void* stream);

/* get_rays + pack for the pixel range [pix_begin, pix_begin+pix_count) of an H x W image
 * (row-major pixel index = row*W + col): the per-rank unit when a view is sharded. */
int nerfail_ray_gen(int H, int W, const float* K4_host, const float* c2w_host, float near_, float far_,
                    int64_t pix_begin, int64_t pix_count, float* rays, void* stream);

/* ABI 13. The training batch (K1b): which rays a step trains on, and those rays, from resident data.
 *
 * nerfail_index_shuffle: out[j] = P(key, m)(first + j), j < n, where P(key, m) is a bijection of [0, m) evaluated per
 * element - no memory, no sort: a balanced Feistel network (6 rounds, murmur3's 32-bit finaliser as round function) over
 * the smallest even bit width covering m - 1, cycle-walked back into [0, m). The definition is the __host__ __device__
 * function index_shuffle() of csrc/index_shuffle.h; tests/batch_ref.py restates it. Requires 1 <= m <= 2^31, first >= 0,
 * n >= 0, first + n <= m. The first n values of a permutation are n distinct indices - what RN:768
 * (np.random.choice(H*W, N_rand, replace=False)) draws; successive ranges of one permutation are the batches of an epoch -
 * what RN:704 / RN:733-742 take from a shuffled copy of every training ray. Same distribution as the reference's draws,
 * not the same bits. */
int nerfail_index_shuffle(uint64_t key, int64_t m, int64_t first, int64_t n, int64_t* out, void* stream);

/* Packed rays and target colours of one training batch, RN:733-735 (use_batching) and RN:746-773 (one image, optional
 * precrop window RN:754-761), from resident data: poses[n_img,12] (row-major [3,4] c2w per image), images[n_img,H,W,3]
 * (NULL: no targets are written). The population is n_views view slots times the window (row0, col0, wh, ww) of the image:
 * index q in [0, m), m = n_views*wh*ww, is slot q / (wh*ww), row row0 + (q % (wh*ww)) / ww, column col0 + q % ww.
 * Slot s shows image view_ids[s] (int32 [n_views]), or view0 + s when view_ids is NULL.
 * The batch is sel[n] (int64 population indices), or, when sel is NULL, q_j = P(key, m)(first + j) computed in the kernel.
 * Writes rays[n,11] - row j bit for bit the row nerfail_ray_gen writes for that pixel and pose -, target[n,3] (copies of the
 * pixels; untouched when images is NULL) and, unless NULL, sel_out[n] = q_j.
 * Validated: the window lies inside the image, 1 <= m <= 2^31, 0 <= first, n <= m - first (both modes), view0 .. view0 +
 * n_views inside [0, n_img) when view_ids is NULL, NULL pointers. The VALUES of view_ids (< n_img) and sel (< m) are the
 * caller's contract, as index maps are elsewhere in this ABI. */
int nerfail_train_batch(int H, int W, const float* K4_host, float near_, float far_, const float* poses, int n_img,
                        const float* images, int row0, int col0, int wh, int ww, const int32_t* view_ids, int view0,
                        int n_views, const int64_t* sel, uint64_t key, int64_t first, int64_t n, float* rays,
                        float* target, int64_t* sel_out, void* stream);

/* ------------------------------------------------------------------ sampling (K2, K6) ----- */

/* Coarse samples of render_rays, RN:357-381. t_vals[N] = torch.linspace(0,1,N) (host computes it so
 * the bits are the reference's); t_rand[R,N] = stratified draws in [0,1) or NULL (perturb == 0).
 * Writes z_vals[R,N] and pts[R,N,3] = o + d*z. */
int nerfail_sample_coarse(const float* rays, int64_t n_rays, const float* t_vals, int n_samples,
                          const float* t_rand, int lindisp, float* z_vals, float* pts, void* stream);

/* sample_pdf, RH:200-243: bins[R,nb], weights[R,nb-1] -> samples[R,n]. u[R,n] explicit uniform draws
 * (u_is_row != 0: one row u[n] shared by all rays, e.g. torch.linspace(0,1,n) for det=True). */
int nerfail_sample_pdf(const float* bins, const float* weights, int64_t n_rays, int n_bins,
                       const float* u, int u_is_row, int n_samples, float* samples, void* stream);

/* Hierarchical step of render_rays, RN:392-397 + RN:412, fused: z_mid, sample_pdf on weights[...,1:-1],
 * sort(cat(z_vals, z_samples)), pts = o + d*z, z_std = std(z_samples, unbiased=False).
 * z_coarse[R,Nc], weights[R,Nc] -> z_samples[R,Nf] (may be NULL), z_fine[R,Nc+Nf], pts[R,Nc+Nf,3], z_std[R]. */
int nerfail_sample_fine(const float* rays, int64_t n_rays, const float* z_coarse, const float* weights,
                        int n_coarse, const float* u, int u_is_row, int n_fine,
                        float* z_samples, float* z_fine, float* pts, float* z_std, void* stream);

/* ------------------------------------------------------------------ MLP (K3 + K4) --------- */

/* Embedder.embed, RH:15-50 (log-sampled bands, include_input): x[M,3] -> out[M, 3 + 6*multires] =
 * [x, sin(x*2^0), cos(x*2^0), ..., sin(x*2^(L-1)), cos(x*2^(L-1))]. Standalone form of the encoding;
 * the render path never calls it (nerfail_mlp_fwd computes the encoding in registers). */
int nerfail_embed(const float* x, int64_t M, int multires, float* out, void* stream);

/* nn.Linear tensors of one NeRF (RH:83-98), weight layout [out, in] row-major as in the state_dict. */
typedef struct nerfail_mlp_params {
    int32_t D, W;                 /* netdepth, netwidth: (8,256) or (4,64); W % 32 == 0, W <= 256 */
    int32_t input_ch;             /* 63 (multires 10)                                              */
    int32_t input_ch_views;       /* 27 (multires_views 4)                                         */
    int32_t skip;                 /* layer index after which [input_pts, h] is concatenated (4), -1 = none */
    int32_t reserved;
    const float* pts_w[NERFAIL_MAX_DEPTH];   /* pts_linears.i.weight */
    const float* pts_b[NERFAIL_MAX_DEPTH];   /* pts_linears.i.bias   */
    const float* views_w;  const float* views_b;      /* views_linears.0  [W/2, W+27] */
    const float* feature_w; const float* feature_b;   /* feature_linear   [W, W]      */
    const float* alpha_w;  const float* alpha_b;      /* alpha_linear     [1, W]      */
    const float* rgb_w;    const float* rgb_b;        /* rgb_linear       [3, W/2]    */
} nerfail_mlp_params;

/* Number of floats of the MFMA-fragment-ordered weight image for a (D, W, skip) network; 0 if unsupported. */
size_t nerfail_mlp_packed_floats(int D, int W, int skip);
/* Re-pack the nn.Linear tensors into that image (device to device; call again after weights change). */
int nerfail_mlp_pack(const nerfail_mlp_params* params_host, float* packed, void* stream);

/* run_network, RN:37-51 (+ Embedder RH:15-50, NeRF.forward RH:100-123), fused: positional encoding of
 * pts (L=10) and of the per-ray viewdir (L=4) is computed in registers and never written to memory.
 * pts[M,3]; viewdirs[n_rays,3] with sample m using row m / samples_per_ray; raw[M,4] = rgb(3), sigma(1). */
int nerfail_mlp_fwd(const float* packed, int D, int W, int skip, const float* pts, const float* viewdirs,
                    int64_t M, int samples_per_ray, float* raw, void* stream);

/* Which kernel serves nerfail_mlp_fwd / nerfail_mlp_fwd_embedded: 0 = automatic (default: the LDS-streaming kernel for
 * even depths <= 8, else the register-streamed one), 1 = register-streamed (mlp.hip), 2 = LDS-streaming (mlp_lds.hip;
 * shapes it does not cover return NERFAIL_EINVAL). Both compute the same f32 FMA chains in the same order; the switch
 * exists for A/B timing and for the parity test of one against the other. 3 = the bf16x3 kernel (mlp_x3.hip) for the x3
 * entry points below (an error where it does not cover the shape; the other entry points select automatically). Under 0 the
 * x3 entry points use it wherever it covers the shape. Initial value from NERFAIL_FWD_KERNEL=reg|lds|x (read once).
 * Process-wide; returns the previous value. */
int nerfail_mlp_fwd_select(int which);

/* Which kernel serves nerfail_mlp_bwd_data / nerfail_mlp_bwd_data2: 0 = automatic (default: the LDS-ring kernel for W = 256 and
 * even depths <= 8, else the register-streamed one), 1 = register-streamed (mlp_bwd.hip), 2 = LDS ring (mlp_lds.hip; shapes it
 * does not cover return NERFAIL_EINVAL). Both store the same bits; the switch exists for A/B timing and for the parity test of
 * one against the other. Initial value from NERFAIL_BWD_KERNEL=reg|lds (read once). Process-wide; returns the previous value. */
int nerfail_mlp_bwd_select(int which);

/* NeRF.forward on an already embedded batch x[M, 63+27] (RH:100-123 as a standalone call). */
int nerfail_mlp_fwd_embedded(const float* packed, int D, int W, int skip, const float* x, int64_t M,
                             float* raw, void* stream);

/* ---- bf16x3 inference: same contracts as nerfail_mlp_fwd / _fwd_embedded / _fwd_rays, f32-accurate, not bitwise ----------
 * Every f32 product as six bf16 products (hi/mid/lo round-to-nearest split of both operands, the three smallest cross terms
 * dropped: about 2^-26 |a||b| per product). Covers W = 256 at even depths <= 8 (nerfail_mlp_packed_x3_bytes returns 0 for
 * other shapes). `x3`: nerfail_mlp_packed_x3_bytes() bytes, filled on the device by nerfail_mlp_pack_x3 from the f32 image
 * `packed`, which the kernel still reads for the biases and heads. The entry points run the bf16x3 kernel under the
 * automatic selection when x3 is non-NULL and the shape is covered (and, for _rays, acts is NULL); otherwise exactly the
 * path of the f32 entry point. */
size_t nerfail_mlp_packed_x3_bytes(int D, int W, int skip);
int nerfail_mlp_pack_x3(const float* packed, int D, int W, int skip, void* x3, void* stream);
int nerfail_mlp_fwd_x3(const float* packed, const void* x3, int D, int W, int skip, const float* pts, const float* viewdirs,
                       int64_t M, int samples_per_ray, float* raw, void* stream);
int nerfail_mlp_fwd_embedded_x3(const float* packed, const void* x3, int D, int W, int skip, const float* x, int64_t M,
                                float* raw, void* stream);
int nerfail_mlp_fwd_rays_x3(const float* packed, const void* x3, int D, int W, int skip, const float* rays,
                            const float* z_vals, int64_t n_rays, int samples_per_ray, float* raw, float* acts, void* stream);

/* ABI 12. The same kernel without feature_linear: no activation lies between feature_linear and views_linears[0], so
 * Wc = Wv[:, :W] Wf and bc = Wv[:, :W] bf + bv are composed ONCE per weight set (nerfail_mlp_pack_x3f, on the device, from
 * the f32 image: each sum over m = 0..W-1 in this order in double, bv added last, rounded once to f32, then Wc split
 * into bf16 planes like every weight) and the 256 -> 256 layer, 11 % of the kernel's MFMAs, leaves the hot path. The folded
 * image `x3f` is separate from `x3`: the stream of layers 0..D-1 as there, ONE views layer (Wc, then the direction columns),
 * the constant area of the f32 image with bias piece D = bc (zero behind it), and last the composed f32 block of
 * nerfail_mlp_x3f_composed_floats() floats - Wc [W/2][W] row-major, then bc [W/2] zero-padded to 256 floats. A caller
 * checks that block for inf / NaN (weights so large that the product leaves f32) and, if it finds any, keeps using the
 * unfolded entry points above. Same shapes, same selection rules and same fall-backs as the x3 entry points (forced reg /
 * lds: the exact kernels; shapes not covered: nerfail_mlp_packed_x3f_bytes returns 0 and the f32 path runs); f32-accurate,
 * not bitwise the unfolded kernel's results. */
size_t nerfail_mlp_packed_x3f_bytes(int D, int W, int skip);
size_t nerfail_mlp_x3f_composed_floats(int D, int W, int skip);
int nerfail_mlp_pack_x3f(const float* packed, int D, int W, int skip, void* x3f, void* stream);
int nerfail_mlp_fwd_x3f(const float* packed, const void* x3f, int D, int W, int skip, const float* pts, const float* viewdirs,
                        int64_t M, int samples_per_ray, float* raw, void* stream);
int nerfail_mlp_fwd_embedded_x3f(const float* packed, const void* x3f, int D, int W, int skip, const float* x, int64_t M,
                                 float* raw, void* stream);
int nerfail_mlp_fwd_rays_x3f(const float* packed, const void* x3f, int D, int W, int skip, const float* rays,
                             const float* z_vals, int64_t n_rays, int samples_per_ray, float* raw, float* acts, void* stream);

/* The folded kernel with the view-direction term computed once per RAY (additions only: version and revision words unchanged; a
 * library without them fails the loader's symbol check). When samples_per_ray is a multiple of 32 every 32-sample tile lies
 * inside one ray, and Wv[:, W:] enc(d) is one W/2-vector per ray. nerfail_mlp_x3f_viewbias writes
 *     vb[r][bias_index(i)] = float( bc[i] + sum_{m = 0..26} Wv[i][W + m] * enc(d_r)[m] )
 * - from the composed f32 bc[i] of the folded image, the terms added in this order in double (each product exact), rounded
 * once; enc(d) the direction encoding of every MLP kernel (x, y, z, then per band sin(3), cos(3)); row r in the kernels' bias
 * piece order (mlp_layout.h) - for the directions of `rays` [n_rays,11] or (exactly one of the two non-NULL) `viewdirs`
 * [n_rays,3]. The _raybias entry points run it into `vb` and then the folded kernel in a form that neither encodes directions
 * nor runs the direction part: a tile's row replaces the composed bias. raw[..., 3] is bitwise that of the plain folded
 * kernel; raw[..., :3] is f32-accurate, not bitwise. `vb`: nerfail_mlp_x3f_raybias_floats() floats, a temporary of the call.
 * That function returns 0 when the form does not serve the call - samples_per_ray not a multiple of 32, a shape the folded
 * image does not cover, reg / lds forced (NERFAIL_FWD_KERNEL), or the form switched off (NERFAIL_X3_RAYBIAS=0, read once;
 * nerfail_mlp_x3_raybias_select(0 | 1) sets it and returns the previous value, any other argument only queries): the caller
 * then uses nerfail_mlp_fwd[_rays]_x3f, and the _raybias entry points refuse the call. Inference only. */
size_t nerfail_mlp_x3f_raybias_floats(int D, int W, int skip, int64_t n_rays, int samples_per_ray);
int nerfail_mlp_x3_raybias_select(int on);
int nerfail_mlp_x3f_viewbias(const float* packed, const void* x3f, int D, int W, int skip, const float* rays, const float* viewdirs,
                             int64_t n_rays, float* vb, void* stream);
int nerfail_mlp_fwd_x3f_raybias(const float* packed, const void* x3f, int D, int W, int skip, const float* pts, const float* viewdirs,
                                int64_t M, int samples_per_ray, float* raw, float* vb, void* stream);
int nerfail_mlp_fwd_rays_x3f_raybias(const float* packed, const void* x3f, int D, int W, int skip, const float* rays,
                                     const float* z_vals, int64_t n_rays, int samples_per_ray, float* raw, float* vb, void* stream);

/* ---- split-precision ("f16x3") forward: same contract as nerfail_mlp_fwd, fp32-equivalent results --------
 * Every product a*w is evaluated as a_hi*w_hi + a_hi*w_lo + a_lo*w_hi on the fp16 matrix cores with fp32
 * accumulation (a_hi = fp16(a), a_lo = fp16(a - a_hi); weights pre-scaled by 2^10 inside the image). Opt-in: the
 * default path is the exact-f32 kernel. `image`: nerfail_mlp_f16_image_bytes() bytes, filled by
 * nerfail_mlp_pack_f16 from the nn.Linear tensors; `packed` is the f32 image of nerfail_mlp_pack (biases, heads). */
size_t nerfail_mlp_f16_image_bytes(int D, int W, int skip);
int nerfail_mlp_pack_f16(const nerfail_mlp_params* params_host, void* image, void* stream);
int nerfail_mlp_fwd_f16(const float* packed, const void* image, int D, int W, int skip, const float* pts,
                        const float* viewdirs, int64_t M, int samples_per_ray, float* raw, void* stream);
/* Same, additionally saving the fp32 activation tiles exactly like nerfail_mlp_fwd_train (the backward kernels
 * consume them unchanged). */
int nerfail_mlp_fwd_f16_train(const float* packed, const void* image, int D, int W, int skip, const float* pts,
                              const float* viewdirs, int64_t M, int samples_per_ray, float* raw, float* acts,
                              void* stream);

/* Split-precision backward-data: same contract as nerfail_mlp_bwd_data with the transposed fp16 image. */
size_t nerfail_mlp_f16_image_T_bytes(int D, int W, int skip);
int nerfail_mlp_pack_f16_T(const nerfail_mlp_params* params_host, void* imageT, void* stream);
int nerfail_mlp_bwd_data_f16(const float* packed, const void* imageT, int D, int W, int skip, const float* d_raw,
                             const float* acts, int64_t M, float* dz, void* stream);

/* ---- training step (RN:776-801): forward that saves activations, backward-data, weight gradients -------- */

/* Floats of the activation / gradient scratch of one pass over M samples (0 = unsupported shape). */
size_t nerfail_mlp_train_acts_floats(int D, int W, int64_t M);
size_t nerfail_mlp_train_dz_floats(int D, int W, int64_t M);
/* nerfail_mlp_fwd that additionally writes every layer's activation to `acts` (register-fragment layout). */
int nerfail_mlp_fwd_train(const float* packed, int D, int W, int skip, const float* pts, const float* viewdirs,
                          int64_t M, int samples_per_ray, float* raw, float* acts, void* stream);
/* The north-star form of nerfail_mlp_fwd / nerfail_mlp_fwd_train: the sample points are formed INSIDE the kernel from the
 * packed rays [n_rays,11] and the depths z_vals [n_rays, samples_per_ray] - pts = o + d * z with the reference's rounding
 * (RN:381, :399) - so the [M,3] point tensor is never written or read (nerfail_sample_coarse / nerfail_sample_fine accept
 * pts = NULL, nerfail_composite forms pts_max from the ray when pts is NULL). acts: NULL, or the training forward's
 * activation buffer (nerfail_mlp_train_acts_floats). Same bits as the pts form. */
int nerfail_mlp_fwd_rays(const float* packed, int D, int W, int skip, const float* rays, const float* z_vals,
                         int64_t n_rays, int samples_per_ray, float* raw, float* acts, void* stream);
/* Transposed weight image for the backward-data pass (re-pack after every optimizer step). */
size_t nerfail_mlp_packed_T_floats(int D, int W, int skip);
int nerfail_mlp_pack_T(const nerfail_mlp_params* params_host, float* packedT, void* stream);
/* nerfail_mlp_pack + nerfail_mlp_pack_T in ONE launch (the training loop re-packs both after every optimizer step). */
int nerfail_mlp_pack_train(const nerfail_mlp_params* params_host, float* packed, float* packedT, void* stream);
/* d_raw[M,4] -> gradient w.r.t. every layer's pre-activation (`dz`, fragment layout). */
int nerfail_mlp_bwd_data(const float* packed, const float* packedT, int D, int W, int skip, const float* d_raw,
                         const float* acts, int64_t M, float* dz, void* stream);
/* The same for TWO networks of one architecture in ONE launch (the coarse and the fine network of a training step:
 * independent, RN:394): d_raw / acts / dz hold the M0 samples (tiles) of network 0 followed by the M1 of network 1;
 * M0 must be a multiple of 32 when M1 > 0. */
int nerfail_mlp_bwd_data2(const float* packed0, const float* packedT0, int64_t M0, const float* packed1,
                          const float* packedT1, int64_t M1, int D, int W, int skip, const float* d_raw,
                          const float* acts, float* dz, void* stream);
/* Parameter gradients of ONE or TWO networks of the same architecture in one launch (RN:791; the coarse and the
 * fine network of a training step are independent because RN:394 detaches z_samples). `acts` / `dz` hold the tiles
 * of network 0 (M0 samples) followed by those of network 1 (M1 samples; M1 = 0: one network, then M0 need not be a
 * multiple of 32). gradsN hold DEVICE pointers shaped like the nn.Linear tensors (same struct as the weights).
 * flags: NERFAIL_DW_ACCUMULATE adds to the gradient tensors (+=), otherwise they are overwritten;
 *        NERFAIL_DW_BF16X3 converts the operands in registers to bf16 hi/lo pairs, 3 bf16 MFMAs per product block
 *        (fp32 accumulation, fp32 exponent range, ~1.5e-5 relative per product: a gradient-grade opt-in mode).
 * W = 256: LDS-staged kernel, NO float atomics - every workgroup writes its partial block to `scratch`
 * (nerfail_mlp_bwd_weights_scratch_bytes) and a second kernel adds the partials in workgroup order, so the result is
 * bitwise reproducible. Other widths (and NERFAIL_DW_KERNEL=reg): register-fed kernel with float atomics, no scratch.
 * D <= 10 (the descriptor table of both kernels): a deeper network is refused with NERFAIL_EINVAL before anything is launched,
 * the gradient tensors keep what they held. */
#define NERFAIL_DW_BF16X3 1
#define NERFAIL_DW_ACCUMULATE 2
size_t nerfail_mlp_bwd_weights_scratch_bytes(int D, int W, int skip, int64_t M0, int64_t M1, int flags);
int nerfail_mlp_bwd_weights(int D, int W, int skip, const float* acts, const float* dz, int64_t M0,
                            const nerfail_mlp_params* grads0, int64_t M1, const nerfail_mlp_params* grads1, int flags,
                            void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ compositing (K5, K7) -- */

/* raw2outputs, RN:262-305, one wavefront per ray with a wave-level exclusive product scan.
 * raw[R,N,4], z_vals[R,N], rays (packed [R,11]; d is read from it), noise[R,N] already scaled by
 * raw_noise_std or NULL. Outputs rgb_map[R,3], disp_map[R], acc_map[R], weights[R,N], depth_map[R];
 * if pts_max[R,3] is non-NULL also NC:418-423 (first argmax of weights -> point): gathered from pts[R,N,3], or - pts
 * NULL - formed from the ray and its depth (o + d * z, the same bits). */
int nerfail_composite(const float* raw, const float* z_vals, const float* rays, const float* noise,
                      int64_t n_rays, int n_samples, int white_bkgd,
                      float* rgb_map, float* disp_map, float* acc_map, float* weights, float* depth_map,
                      const float* pts, float* pts_max, void* stream);

/* Which kernel serves nerfail_composite: 0 = automatic (default: two rays per wave when n_samples is a multiple of 32, else
 * one ray per wave), 1 = one ray per wave everywhere. The two forms add a ray's sums in different orders (last bits). The
 * initial value is read ONCE from NERFAIL_COMPOSITE_KERNEL ("1"); the switch exists for A/B timing and for the parity test of
 * one form against the other. Process-wide; returns the previous value. */
int nerfail_composite_select(int which);

/* Backward of raw2outputs (autograd of RN:262-305, what loss.backward() at RN:791 needs): given the upstream
 * gradients of rgb_map[R,3], disp_map[R], acc_map[R], depth_map[R], weights[R,N] (each may be NULL = zero)
 * writes d_raw[R,N,4]. z_vals / rays_d receive no gradient (z_samples is detached, RN:394). */
int nerfail_composite_bwd(const float* raw, const float* z_vals, const float* rays, const float* noise,
                          int64_t n_rays, int n_samples, int white_bkgd, const float* g_rgb_map,
                          const float* g_disp_map, const float* g_acc_map, const float* g_depth_map,
                          const float* g_weights, float* d_raw, void* stream);

/* ------------------------------------------------------------------ 8-NN build (K8) ------- */

/* create_index_and_dist core, CI:126-145, exact: for each query the 8 smallest keys
 * (d2, index) with d2 = ((dx*dx + dy*dy) + dz*dz) in float32 without FMA; dist = sqrt(d2).
 * queries[Nq,3], points[M,3] (M < 2^24 so indices are exact in float32, as on disk CI:148-163).
 * dist[Nq,8] ascending; idx_f32[Nq,8] (may be NULL) and idx_i32[Nq,8] (may be NULL). */
int nerfail_knn8(const float* queries, int64_t n_queries, const float* points, int64_t n_points,
                 float* dist, float* idx_f32, int32_t* idx_i32, void* stream);

/* Same result, bit for bit, through a uniform grid (cell sort + shell expansion with a conservative termination
 * bound): ~1000x less work than the brute-force scan at 1.92 M points. workspace: scratch of
 * nerfail_knn8_grid_workspace_bytes(n_points) bytes (0 = unsupported size). */
size_t nerfail_knn8_grid_workspace_bytes(int64_t n_points);
int nerfail_knn8_grid(const float* queries, int64_t n_queries, const float* points, int64_t n_points,
                      float* dist, float* idx_f32, int32_t* idx_i32, void* workspace, size_t workspace_bytes,
                      void* stream);
/* The two halves of nerfail_knn8_grid: the grid of a point set is built ONCE into `workspace` (CI:57-61 stacks the base
 * views of a scene once) and searched for every view of the scene (CI:110-163: 400 of them) - same results, the build's
 * ~1 ms per view saved. The workspace must not be modified between build and search. */
int nerfail_knn8_grid_build(const float* points, int64_t n_points, void* workspace, size_t workspace_bytes, void* stream);
int nerfail_knn8_grid_search(const float* queries, int64_t n_queries, int64_t n_points, float* dist, float* idx_f32,
                             int32_t* idx_i32, const void* workspace, size_t workspace_bytes, void* stream);
/* The same search for the [height, width, 3] point image of ONE VIEW (pts_max, NC:418-423 -> CI:126): results in the same
 * row-major [height*width, 8] layout, but a wave searches an 8 x 8 pixel tile instead of 64 consecutive pixels of a row -
 * neighbouring pixels' points lie within a fraction of a grid cell, the 64 searches share their candidates. */
/* (all grid searches: dist / idx_f32 / idx_i32 must be 16-byte aligned - a query's eight results leave as two 16-byte stores) */
int nerfail_knn8_grid_search_view(const float* queries, int height, int width, int64_t n_points, float* dist, float* idx_f32,
                                  int32_t* idx_i32, const void* workspace, size_t workspace_bytes, void* stream);
/* Work counters of the grid search (measurement aid, off by default): while `stats` (two device uint64, zeroed by the caller)
 * is set, every search adds [0] the distances it computed (summed over queries) and [1] the queries answered by the
 * wave-cooperative search (all of a coherent wave's; the leftovers of the per-lane shell walk otherwise). NULL switches the
 * counters off again. Process-wide, not stream-ordered with other threads' searches. */
int nerfail_knn8_grid_stats(unsigned long long* stats);

/* ------------------------------------------------------------------ gauss path (K9-K12) --- */

/* create_gauss_w.forward, GN:169-186 (driver DW:82-97): dist_and_index[B,2,P,8] -> out[B,2,P,8]
 * (weight, index) with g = exp(-(d/c)^2/2), w = g/(sum g + 0.001) if sum g > 0 else 0. P = H*W. */
int nerfail_gauss_weight(const float* dist_and_index, int64_t B, int64_t P, float c, float* out, void* stream);

/* gauss_get_img.forward's hot part, GN:309-319: x_rgba[n,4] from an already gathered r[n,4] (gauss_get_r's output, GN:224-268)
 * and ori_img[n,4] (float BGRA): rgb = ori_rgb + r_rgb * (r_a/255) where ori_a > 0 else 0, a = ori_a. Unlike gauss_net's
 * composite (nerfail_gauss_fwd) there is neither an epsilon clip nor a [0,255] clip. x_rgba may alias nothing. */
int nerfail_gauss_compose(const float* ori_img, const float* r, int64_t n_pixels, float* x_rgba, void* stream);

/* gauss_net.forward hot part, GN:53-119. spatial[Ns,4] (BGRA, 0..255), weight_and_index[B,2,P,8],
 * ori_img[B,P,4] float. epsilon < 0 means None (no clip). Writes x[B,P,4], x_rgba[B,P,4];
 * eps_minmax (2 floats, may be NULL) is UPDATED with the running min / max of x_rgb*alpha (GN:89-103):
 * eps_minmax[0] = min(old, new_min), eps_minmax[1] = max(old, new_max). */
int nerfail_gauss_fwd(const float* spatial, int64_t Ns, const float* weight_and_index, const float* ori_img,
                      int64_t B, int64_t P, float epsilon, float* x, float* x_rgba, float* eps_minmax,
                      void* stream);

/* The same over views that are addressed ONE BY ONE (host table of n_views entries; all pointers device memory): the
 * device-resident maps of the attack loop, kept per view id instead of re-uploaded per iteration (MyDataset.py:199-204
 * hands out a freshly loaded 41 MB map per view and step). ori_is_u8: ori_img entries are uint8 [P,4] BGRA as cv2.imread
 * delivers them (MyDataset.py:200), else float32 [P,4]. x may be NULL (GN:83's tensor is not needed by the attack step);
 * aux_alpha [n_views*P] / aux_mask [n_views*P] (both or neither) receive alpha = x_3 / 255 and the 3-bit mask "channel c
 * passes its gradient" - all nerfail_gauss_bwd_views_rgb needs. Outputs are indexed [view][pixel] like a batch tensor. */
typedef struct nerfail_view_fwd {
    const float* weight_and_index;  /* [2,P,8] float32: weights, then indices (as float) */
    const void* ori_img;            /* [P,4] uint8 or float32 */
} nerfail_view_fwd;
int nerfail_gauss_fwd_views(const float* spatial, int64_t Ns, const nerfail_view_fwd* views, int n_views, int64_t P,
                            int ori_is_u8, float epsilon, float* x, float* x_rgba, float* aux_alpha, unsigned char* aux_mask,
                            float* eps_minmax, void* stream);

/* Backward of the above (autograd of GN:63-119): grad_spatial[Ns,4] += d/ds( sum(x*grad_x) +
 * sum(x_rgba*grad_x_rgba) ). grad_x / grad_x_rgba may be NULL (treated as zero). x is the forward's
 * saved output. grad_spatial is ACCUMULATED into (zero it first for a fresh gradient) with float atomics. */
int nerfail_gauss_bwd(const float* weight_and_index, const float* ori_img, const float* x,
                      const float* grad_x, const float* grad_x_rgba, int64_t Ns, int64_t B, int64_t P,
                      float epsilon, float* grad_spatial, void* stream);

/* Deterministic form of the same backward. The index map of a view is static, so its inverse (for each
 * row of the perturbation table, the contributions (view b, pixel p, neighbour k) that gather from it, in
 * ascending (b*P+p)*8+k order) is built once and reused by every attack epoch:
 *   row_ptr[Ns+1] int32, contrib[B*P*8] int32 (contribution id), w_sorted[B*P*8] (its weight).
 * workspace: nerfail_gauss_csr_workspace_bytes() bytes of scratch (0 = sizes unsupported). */
/* Content fingerprint of n_items equally sized device buffers laid out back to back (32-bit words): out[2i] = sum of the
 * words, out[2i+1] = sum of word * (1 + position mod 65521), modulo 2^64. Host code keys per-view inverted indices on it
 * when a view's map arrives as an anonymous tensor (MyDataset.py:199-204 + DataLoader: a fresh tensor per iteration). */
int nerfail_fingerprint(const void* data, int64_t words_per_item, int64_t n_items, uint64_t* out, void* stream);
size_t nerfail_gauss_csr_workspace_bytes(int64_t Ns, int64_t B, int64_t P);
/* row_of [B*P*8] int32: the destination row of every entry of the row-sorted list (contrib / w_sorted are in that order);
 * entries of weight 0 are sorted behind row_ptr[Ns] and never visited. */
int nerfail_gauss_csr_build(const float* weight_and_index, int64_t Ns, int64_t B, int64_t P, int32_t* row_ptr,
                            int32_t* contrib, float* w_sorted, int32_t* row_of, void* workspace, size_t workspace_bytes,
                            void* stream);
/* floats of scratch the two backward calls below need (per-pixel gradients + partial-row records); 0 = bad arguments */
size_t nerfail_gauss_bwd_scratch_floats(int64_t B, int64_t P, int n_rhs);
/* grad_spatial[Ns,4] = (accumulate ? grad_spatial : 0) + segmented reduction of w_e * (per-pixel gradient) over the
 * row-sorted entries: no atomics, fixed summation order, bitwise reproducible. */
int nerfail_gauss_bwd_csr(const float* ori_img, const float* x, const float* grad_x, const float* grad_x_rgba,
                          const int32_t* row_ptr, const int32_t* contrib, const float* w_sorted, const int32_t* row_of,
                          int64_t Ns, int64_t B, int64_t P, float epsilon, float* scratch, int accumulate,
                          float* grad_spatial, void* stream);

/* The compact form of ONE view's index, from the arrays of nerfail_gauss_csr_build with B = 1:
 *   pos[Ns]            ordinal of row j among the view's non-empty rows, -1 for an empty row;
 *   packed[e]          pixel * 2 + (1 if entry e starts a row), for the first min(entry_capacity, row_ptr[Ns]) entries;
 *   chunk_ord[c]       ordinal of the row of entry 512 c (one int per 512 entries: nerfail_gauss_view_chunks(n) ints);
 *   n_rows[0] (device) number of non-empty rows.
 * With w_sorted that is everything the backward reads: 8 bytes per entry + 4 Ns. */
size_t nerfail_gauss_view_pack_workspace_bytes(int64_t Ns);
int64_t nerfail_gauss_view_chunks(int64_t n_entries);
int nerfail_gauss_view_pack(const int32_t* row_ptr, const int32_t* row_of, const int32_t* contrib, int64_t Ns,
                            int64_t entry_capacity, int32_t* pos, int32_t* packed, int32_t* chunk_ord, int32_t* n_rows,
                            void* workspace, size_t workspace_bytes, void* stream);

/* One view's inverted index in compact form (nerfail_gauss_view_pack). All pointers are device memory; the counts are
 * host values (read back once when the index is built). `packed` and `w_sorted` are read 16 bytes per lane at multiples of 8
 * entries: keep them 16-byte aligned (any allocator does; a slice starting at an odd entry still works, slower). */
typedef struct nerfail_view_index {
    const int32_t* packed;     /* [n_entries] pixel * 2 + row-start flag, entries sorted by destination row             */
    const float* w_sorted;     /* [n_entries] the entry's Gaussian weight                                               */
    const int32_t* chunk_ord;  /* [nerfail_gauss_view_chunks(n_entries)] row ordinal of every 512th entry               */
    const int32_t* pos;        /* [Ns]        ordinal of a row, -1 if the view has no entry for it                      */
    int64_t n_entries;         /* entries with non-zero weight (= row_ptr[Ns] of the csr build)                         */
    int64_t n_rows;            /* non-empty rows                                                                        */
} nerfail_view_index;
/* The backward of a BATCH of views through their per-view indices (host table of n_views structs): per-pixel gradients of
 * the whole batch in one pass; every view's entries reduced to that view's own row sums (all views in one launch, no
 * shared destination); the views' sums added row by row IN VIEW ORDER. No atomics, every order fixed: bitwise
 * reproducible. ori_img / x / grad_* are [n_views*P, 4]; grad_spatial [Ns,4] is overwritten. A view's map is static, so
 * its index is built once whatever batches it later appears in (the reference's DataLoader shuffles, AS:222-231).
 * scratch: nerfail_gauss_bwd_views_scratch_floats(views, n_views, P, 1) floats (0 = bad arguments). */
size_t nerfail_gauss_bwd_views_scratch_floats(const nerfail_view_index* views, int n_views, int64_t P, int n_rhs);
int nerfail_gauss_bwd_views(const float* ori_img, const float* x, const float* grad_x, const float* grad_x_rgba,
                            const nerfail_view_index* views, int n_views, int64_t Ns, int64_t P, float epsilon,
                            float* scratch, float* grad_spatial, void* stream);
/* The rgb-gradient-only form for the NeRFail-S step (AS:357-392 never reads the alpha channel's gradient): upstream
 * gradient w.r.t. x_rgba only, per-pixel chain from nerfail_gauss_fwd_views' aux outputs (5 bytes per pixel instead of
 * x and ori), result as grad_rgb [Ns,3] - the buffer the perturbation-gradient all-reduce moves. Same sums, same order
 * as nerfail_gauss_bwd_views: the three channels are bitwise equal to its rgb channels. Same scratch size. */
int nerfail_gauss_bwd_views_rgb(const float* aux_alpha, const unsigned char* aux_mask, const float* grad_x_rgba,
                                const nerfail_view_index* views, int n_views, int64_t Ns, int64_t P, float* scratch,
                                float* grad_rgb, void* stream);
/* ABI 7 (round 6). The same backward with the NeRFail-S sign step (AS:352-392 = nerfail_igsm_step_rgb) as the epilogue of its last
 * launch: spatial_out[j] = step(spatial[j], d CE / d spatial_rgb[j], spatial_init[j]) - for a 1-rank run, where the gradient is
 * not all-reduced, it is then neither written nor read back (23 MB each way) and one launch goes. grad_rgb: NULL, or [Ns,3] to
 * receive the gradient as well (required when n_views > 16: the running sum between launches). Same sums in the same order as
 * nerfail_gauss_bwd_views_rgb + nerfail_igsm_step_rgb: bit-identical spatial_out. spatial_out must not alias an input. */
int nerfail_gauss_bwd_views_rgb_step(const float* aux_alpha, const unsigned char* aux_mask, const float* grad_x_rgba,
                                     const nerfail_view_index* views, int n_views, int64_t Ns, int64_t P, float* scratch,
                                     float* grad_rgb, const float* spatial, const float* spatial_init, float a, float epsilon,
                                     int targeted, float* spatial_out, void* stream);
/* ONE view, n_rhs (1..8) upstream gradients at once - the class-logit gradients of one DeepFool iteration (deepfool.py:
 * 66-96 takes them one autograd.grad call at a time). grad_x_rgba: [n_rhs][P,4]; grad_spatial: [n_rhs][Ns,4],
 * overwritten. Sums run in the same order as nerfail_gauss_bwd_views, so each right-hand side gets bitwise the result of
 * a single call. scratch: nerfail_gauss_bwd_views_scratch_floats(view, 1, P, n_rhs) floats. */
int nerfail_gauss_bwd_view_multi(const float* ori_img, const float* x, const float* grad_x_rgba, int n_rhs,
                                 const nerfail_view_index* view, int64_t Ns, int64_t P, float epsilon, float* scratch,
                                 float* grad_spatial, void* stream);

/* The same backward for n_rhs (1..8) upstream gradients at once - the class-logit gradients of one DeepFool iteration
 * (deepfool.py:66-96 takes them one autograd.grad call at a time). grad_x_rgba: [n_rhs][B*P,4]; grad_spatial:
 * [n_rhs][Ns,4], overwritten. Sums run in the same order as nerfail_gauss_bwd_csr, so each right-hand side gets bitwise
 * the result of a single call. */
int nerfail_gauss_bwd_csr_multi(const float* ori_img, const float* x, const float* grad_x_rgba, int n_rhs,
                                const int32_t* row_ptr, const int32_t* contrib, const float* w_sorted, const int32_t* row_of,
                                int64_t Ns, int64_t B, int64_t P, float epsilon, float* scratch, float* grad_spatial,
                                void* stream);

/* K14 - DeepFool step arithmetic over the perturbation table (deepfool.py:76-102). grads = [n_rhs][n,4] as written by
 * nerfail_gauss_bwd_csr_multi, slice 0 = original class.
 *   norms:  norms2[k-1] = ||grads[k] - grads[0]||^2 (torch.norm(grad_prime)**2), k = 1..n_rhs-1; two-stage reduction with a
 *           fixed tree (bitwise reproducible); scratch: nerfail_deepfool_norms_scratch_bytes() bytes.
 *   apply:  rot += scale[0] * (grads[best[0]] - grads[0]) (skipped when scale[0] == 0);
 *           spatial_out = clamp(spatial_init + overshoot * rot, -255, 255), alpha channel copied from spatial_init.
 *           best (int32, 1..n_rhs-1) and scale are DEVICE scalars: no host round trip between choosing the class and
 *           applying it. rot is updated in place; spatial_out may alias nothing else. */
size_t nerfail_deepfool_norms_scratch_bytes(int n_rhs, int64_t n);
int nerfail_deepfool_norms(const float* grads, int n_rhs, int64_t n, void* scratch, size_t scratch_bytes, float* norms2,
                           void* stream);
int nerfail_deepfool_apply(const float* grads, int n_rhs, int64_t n, const int32_t* best, const float* scale,
                           float overshoot, const float* spatial_init, float* rot, float* spatial_out, void* stream);

/* NeRFail-S sign step, AS:352-392: rgb <- rgb -/+ a*sign(grad) where alpha > 0 else 0, clamped to
 * init +- epsilon; alpha channel copied. spatial/grad/spatial_init/out are [n,4]; out may alias spatial. */
int nerfail_igsm_step(const float* spatial, const float* grad, const float* spatial_init, int64_t n,
                      float a, float epsilon, int targeted, float* out, void* stream);
/* The same with the gradient as [n,3] (rgb only, nerfail_gauss_bwd_views_rgb's output). */
int nerfail_igsm_step_rgb(const float* spatial, const float* grad_rgb, const float* spatial_init, int64_t n, float a,
                          float epsilon, int targeted, float* out, void* stream);

/* K13 - one optimizer step of the NeRF training loop for ALL parameter tensors in one launch. Replaces
 * optimizer.step() of torch.optim.Adam(params, lr, betas=(0.9, 0.999)) (run_nerf.py:207, :792): no weight decay, no
 * amsgrad. Same fp32 operation order as torch's CPU kernels (bit-exact but for rare 1-ulp differences, fixture g13):
 *   m <- fma(1-beta1, g - m, m);  v <- fma((1-beta2) g, g, beta2 v);
 *   p <- p + (-step_size m) / (sqrt(v) / bias_correction2_sqrt + eps)
 * step_size = lr / (1 - beta1^t) and bias_correction2_sqrt = sqrt(1 - beta2^t) are computed by the caller in double
 * (per tensor: torch keeps one step counter per parameter). `tensors` is a HOST array, copied at enqueue. */
typedef struct nerfail_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
    float step_size;
    float bias_correction2_sqrt;
} nerfail_adam_tensor;
int nerfail_adam_step(const nerfail_adam_tensor* tensors, int n_tensors, double beta1, double beta2, double eps,
                      void* stream);

/* img2mse of the training loss (RH:9, RN:781-789): loss[0] = mean((x - y)^2) over n values by a fixed-order tree, and - when
 * dx is not NULL - dx[i] = 2 (x[i] - y[i]) / n, the gradient of that mean (one launch instead of ~9 torch kernels). */
int nerfail_mse(const float* x, const float* y, int64_t n, float* loss, float* dx, void* stream);

/* One rank's share of that loss in a data-parallel step (ABI 14): x and y hold n of the n_total >= n values of the global
 * batch; loss[0] = sum((x - y)^2) * (1 / n_total) and dx[i] = 2 (x[i] - y[i]) * (1 / n_total). The shares of all ranks add up
 * to the global mean, the parameter gradients they drive to its gradient. nerfail_mse is the n_total = n case of the same
 * kernel (same fixed-order tree: bit for bit the ABI 13 result). */
int nerfail_mse_part(const float* x, const float* y, int64_t n, int64_t n_total, float* loss, float* dx, void* stream);

/* ------------------------------------------------------------------ NeRFail-S epoch statistics (ABI 15) -- */

/* ABI 15 only ADDS the entry points of this section; no existing entry point, struct or default changes, so NERFAIL_ABI_VERSION
 * (the compatibility word callers compare) stays 14 and the additions are announced by nerfail_abi_revision() = 15.
 *
 * The per-epoch bookkeeping of the NeRFail-S loop (AS:319-344, 405-431) on the device, so that the loop never waits for the
 * GPU between epoch ends. Everything accumulates into one STATS ROW of NERFAIL_ATTACK_ROW_FLOATS float32 that the caller
 * zeroes at the start of an epoch. Sums are kept as (hi, lo) float32 pairs whose exact sum is the double-precision running
 * value (counts of views are plain float32, exact up to 2^24 views). A row can travel through a float32 all-reduce, which adds
 * his and los separately: the sum over ranks is then good to one float32 rounding of the his (~6e-8 relative), no longer exact:
 *   [0,1] sum of per-view CE(ori_cla)      [2,3] sum of per-view CE(cla)        [4] views with argmax(ori_cla) == label
 *   [5] views with argmax(cla) == label    [6] views                            [7,8] sum (x_rgba - ori)^2
 *   [9,10] number of elements in that sum  [11..15] unused, left alone
 * One lane adds into the row per launch (plain loads and stores, no atomics): launches on one stream are ordered. */
#define NERFAIL_ATTACK_ROW_FLOATS 16
#define NERFAIL_ATTACK_MAX_CLASSES 32
int nerfail_abi_revision(void);

/* AS:319-330, 339, 344. cla, ori_cla: [B,C] logits, 1 <= C <= 32, 0 <= label < C. Per view: CE = log-sum-exp with the maximum
 * subtracted, minus the label's logit (evaluated in double from the float32 logits); argmax = the FIRST maximum; a row that
 * holds a NaN never counts as correct (its CE is NaN and makes the epoch's mean NaN, as in the reference). Adds, in this
 * order: sum CE(ori_cla), sum CE(cla), correct(ori_cla), correct(cla), B. The views are summed in a fixed order. */
int nerfail_attack_logit_stats(const float* cla, const float* ori_cla, int B, int C, int label, float* row, void* stream);

/* AS:329, 341: sum over [n_views,P,4] of (x_rgba - ori)^2 into row[7,8], and the element count 4 P n_views into row[9,10].
 * x_rgba is dense [n_views,P,4]; ori_views_host is a HOST array of n_views device pointers, each to one view's [P,4] image,
 * float32 or (ori_is_u8) uint8 - resident views keep uint8. Differences and squares are formed in double; each lane sums
 * its pixels (consecutive lanes take consecutive pixels), each workgroup its lanes, one workgroup the per-workgroup partials, all in a fixed order: no float atomics, the
 * same bits on every run, and the same bits for a float32 and a uint8 image holding the same values. scratch:
 * nerfail_img_sqerr_scratch_bytes() bytes (the partials), contents unspecified on return. */
size_t nerfail_img_sqerr_scratch_bytes(void);
int nerfail_img_sqerr(const float* x_rgba, const void* const* ori_views_host, int n_views, int64_t P, int ori_is_u8,
                      void* scratch, float* row, void* stream);

/* The beta term of AS:336 carried into d loss / d x_rgba: g[v,p,c] += scale * (x_rgba[v,p,c] - ori[v][p,c]) (float32: one
 * subtraction, one product, one sum per element). For beta * mean((x_rgba - ori)^2) over a batch of B views the caller
 * passes scale = 2 beta / (4 P B). g is dense [n_views,P,4] like x_rgba. */
int nerfail_img_sqerr_grad_add(const float* x_rgba, const void* const* ori_views_host, int n_views, int64_t P, int ori_is_u8,
                               float scale, float* g, void* stream);

/* AS:405-431 on one workgroup. From the row: test loss = row[0,1] / views, attack loss = row[2,3] / views, the accuracies
 * row[4] / views and row[5] / views, image loss = row[7,8] / row[9,10] (= AS:411's value: every view has the same 4 P
 * elements). best: float32 [4] = {best attack accuracy, its attack loss, its epoch, unused}; the caller initialises it to
 * {10000, 0, -1, 0} untargeted and {0, 0, -1, 0} targeted (AS:270-276). The epoch is taken when its attack accuracy is <= the
 * best (untargeted) or >= the best (targeted) - a tie goes to the later epoch; then best is updated and *flag = 1, else
 * *flag = 0. A NaN accuracy (an epoch without views) is never taken. record: float32 [NERFAIL_ATTACK_ROW_FLOATS] =
 *   {test loss, test acc, attack loss, attack acc, image loss, views, taken, best epoch, best acc, best loss, epoch,
 *    correct(ori_cla), correct(cla), 0, 0, 0}. The row is not written. */
int nerfail_attack_epoch_close(const float* row, float* best, int epoch, int targeted, float* record, int32_t* flag,
                               void* stream);

/* dst[0..n) = src[0..n) if *flag != 0, else nothing is written (the best tensor of AS:426/431 without a host decision).
 * Every workgroup reads the same flag word, written by an EARLIER launch on the stream. 128-bit copies when both pointers are
 * 16-byte aligned. src and dst must not overlap. */
int nerfail_copy_if(const int32_t* flag, const float* src, float* dst, int64_t n, void* stream);

/* float32 -> uint8 as cv2.imwrite stores a float image (AS:401-402): clamp to [0, 255], round half to even; NaN -> 0. */
int nerfail_export_u8(const float* src, int64_t n, unsigned char* dst, void* stream);

/* ------------------------------------------------------------------ Attack evaluation (eval revision 1) -- */

/* What test_for_inception (model_test.py = MT, MyDataset.py = MD) measures after an attack, on the device: the distances between
 * every attacked view and its original (MT:256-266), each view's prediction and cross entropy (MT:292-295) and the set-level
 * record the report is made from (MT:268-278, 298-299, 341-348, 355-399). Like the section above this one only ADDS entry points:
 * NERFAIL_ABI_VERSION stays 14, nerfail_abi_revision() stays 15, and the additions are announced by nerfail_eval_revision() = 1.
 *
 * Image formats of one side of an (attacked, original) pair; P = pixels of a view:
 *   U8C4   [P,4] uint8    what cv2.imread(..., IMREAD_UNCHANGED) returns for an RGBA PNG         base 4-byte aligned
 *   U8C3   [P,3] uint8    a 3-channel file, e.g. a rendered view                                  base 4-byte aligned
 *   F32C4  [P,4] float32  x_rgba of gauss_net, unrounded                                          base 16-byte aligned
 *   FLAT   [P] float32    P elements without alpha logic (an image that already is a classifier  base 4-byte aligned
 *                         input, e.g. after a resize); pairs only with FLAT
 * 4-channel sides get the white background of MT:237-254 / MD:98-105: rgb where alpha > 0, else 255 (a NaN alpha gives white).
 * The channel order is left as stored. A view then has n = 3 P elements (FLAT: n = P). */
#define NERFAIL_EVAL_U8C4 0
#define NERFAIL_EVAL_U8C3 1
#define NERFAIL_EVAL_F32C4 2
#define NERFAIL_EVAL_FLAT 3
#define NERFAIL_EVAL_VIEW_DOUBLES 6
#define NERFAIL_EVAL_RECORD_DOUBLES (16 + NERFAIL_ATTACK_MAX_CLASSES)
int nerfail_eval_revision(void);

/* MT:256-266 for n_views pairs. a_views_host / o_views_host: HOST arrays of n_views device pointers, one image each (resident
 * views are separate allocations); at most 16 pairs travel per launch, the function loops. Per element d = |a - o| is formed in
 * float32 (one rounded subtraction, as the reference's float tensors). rows: float64 [n_views, 6] =
 *   {max d, min d, sum d, sum d^2, count(d != 0), n}
 * with the sums formed in double. A NaN element makes max, min and both sums of ITS view NaN and counts as non-zero.
 * Two stages without atomics: per-workgroup partials in scratch (nerfail_eval_scratch_bytes() bytes, contents unspecified on
 * return), then one wave per view adds them in a fixed order. The element -> lane map and every order depend on n alone: the
 * same bits on every run, for every format holding the same values, and whatever other views share the launch.
 * cla_in (optional, NULL to skip; not with FLAT): float32 [n_views, 3, P], the attacked view after the white background as a
 * planar (NCHW) image - what MyCNN consumes - written in the same pass. No byte at or beyond the end of a view is read.
 * A wrong alignment, an unknown format, FLAT paired with another format or cla_in with FLAT is NERFAIL_EINVAL before any launch;
 * n_views == 0 or P == 0 is a no-op. */
size_t nerfail_eval_scratch_bytes(void);
int nerfail_eval_view_metrics(const void* const* a_views_host, int a_format, const void* const* o_views_host, int o_format,
                              int n_views, int64_t P, void* scratch, double* rows, float* cla_in, void* stream);

/* MT:292-295. logits [B,C] float32, 1 <= C <= 32, 0 <= label < C -> pred int32 [B], ce float64 [B], with the definitions of
 * nerfail_attack_logit_stats (one shared device function): the FIRST maximum is the prediction; CE = log-sum-exp with the maximum
 * subtracted, minus the label's logit, in double. A row that holds a NaN predicts -1 and has CE = NaN. */
int nerfail_eval_logit_stats(const float* logits, int B, int C, int label, int32_t* pred, double* ce, void* stream);

/* MT:268-278, 298-299, 341-348: folds the rows, predictions and CEs of a batch of B views into the set record, float64
 * [NERFAIL_EVAL_RECORD_DOUBLES], which the caller zeroes before the first batch. One lane, plain loads and stores: batches
 * accumulate in stream order.
 *   [0] views so far     [1] e max = max of the views' maxima     [2] e min = min of the views' minima
 *   [3] sum of the views' means (sum d / n)       [4] sum of sqrt(sum d^2)       [5] sum of the non-zero counts
 *   [6] PSNR min         [7] PSNR max             [8] PSNR sum                   [9] CE sum
 *   [10] views without a prediction (pred outside 0..C-1)         [11] sum of n  [12..15] unused, left alone
 *   [16 + k] views predicted as class k
 * PSNR of a view = 20 log10(255 / rmse), rmse = sqrt(sum d^2 / n), rmse == 0 replaced by DBL_EPSILON (get_psnr, MT:26-39):
 * two equal images have PSNR 361.20199909921956, stored as that constant.
 * record[0] == 0 marks the first view: [1], [2], [6], [7] are then SET from it, not compared with the zeroed record. A NaN that
 * enters a maximum or minimum stays (torch.max / torch.min). The report divides [3], [4], [5], [8], [9] by [0] on the host. */
int nerfail_eval_fold(const double* rows, const int32_t* pred, const double* ce, int B, int C, double* record, void* stream);

/* ------------------------------------------------------------------ victim training (cls revision 1) -- */

/* The first stage of the reference's pipeline, model_train.py:107-193 (= MTR; MyDataset.py = MD), on the device: the batch a
 * DataLoader would stack, the cross entropy of nn.CrossEntropyLoss() with one label per row, torch.optim.SGD's momentum step
 * fused with the update of MyCNN's weight image, and the epoch close. Like the two sections before it this one only ADDS entry
 * points: NERFAIL_ABI_VERSION stays 14, nerfail_abi_revision() stays 15, nerfail_eval_revision() stays 1, and the additions are
 * announced by nerfail_cls_revision() = 1. No allocation, no synchronisation, no float atomics; the same bits on every run. */
int nerfail_cls_revision(void);

/* MTR:121-123 with MD:93-105: B views of a resident store, chosen by indices that live on the DEVICE (what
 * nerfail_index_shuffle writes). images: dense uint8 [N,P,4] (NERFAIL_EVAL_U8C4: BGRA as cv2 reads an RGBA PNG; base 16-byte
 * aligned) or [N,P,3] (NERFAIL_EVAL_U8C3; base 4-byte aligned); labels_all int32 [N]; idx int64 [B].
 *   x       float32 [B,3,P] planar (NCHW), channel order as stored; four-channel views on the white background of MD:98-105:
 *           rgb where alpha > 0, else 255.
 *   labels  int32 [B] = labels_all[idx[b]].
 * An index outside 0..N-1 writes a view of NaN and the label -1 and reads nothing of the store. A view is read with wide loads
 * (16 bytes per lane for U8C4, the three dwords of four pixels for U8C3) between a scalar head and tail: view i of a U8C3
 * store starts at byte 3 P i, which is not 4-byte aligned when P is odd. No byte outside the indexed views, and none at or
 * beyond the end of the store, is read. B <= 65535; B == 0 is a no-op. */
int nerfail_cls_batch(const void* images, int format, const int32_t* labels_all, int64_t N, int64_t P, const int64_t* idx, int B,
                      float* x, int32_t* labels, void* stream);

/* MTR:89, 150-169. logits [B,C] float32, 1 <= C <= 32; labels int32 [B]. Per row the CE and the prediction are those of
 * nerfail_attack_logit_stats / nerfail_eval_logit_stats (one shared device function: the FIRST maximum; log-sum-exp with the
 * maximum subtracted, minus the label's logit, in double); a row that holds a NaN, or whose label is outside 0..C-1, is never
 * correct and has CE NaN.
 *   d_logits  [B,C] or NULL (the validation phase): (softmax - onehot) / B, the gradient of nn.CrossEntropyLoss()'s mean
 *             (MTR:89, 164), evaluated in double and rounded once to float32; NaN for a row without a valid label.
 *   row       the phase's stats row, NERFAIL_ATTACK_ROW_FLOATS float32 the caller zeroes per phase; this call adds
 *             [0,1] the sum of the per-view CE as a (hi, lo) pair   [2] correct views   [3] views (B)   [4..15] left alone.
 * One lane adds the B CEs to the running sum in view order, with plain loads and stores: batches accumulate in stream order.
 * The sum of per-view CE is what MTR:168 means by loss.item() * inputs.size(0): exact here, where the reference rounds the
 * batch mean to float32 once and multiplies it back. */
int nerfail_cls_ce(const float* logits, const int32_t* labels, int B, int C, float* d_logits, float* row, void* stream);

/* MTR:90, 165: one step of torch.optim.SGD(lr, momentum) - dampening 0, no weight decay, no Nesterov - on MyCNN, and the weight
 * image kept in step, in ONE launch. params, grads, momentum_buf: nerfail_cnn_grad_floats(num_classes) floats each, in the
 * layout nerfail_cnn_bwd_weights writes d_params in; packed: the image of nerfail_cnn_pack. lr and momentum are float32.
 *   first != 0:  buf <- g                         (the step that creates torch's momentum buffer)
 *   else:        buf <- fl(fl(mu * buf) + g)      (two roundings: buf.mul_(mu).add_(g))
 *   then:        p <- fma(-lr, buf, p)            (one rounding: p.add_(buf, alpha = -lr))
 * which is, bit for bit, what torch's CPU kernels compute. On return packed is bit for bit what nerfail_cnn_pack makes from the
 * updated parameters: every updated float is written to its one to three places in the image by the lane that updated it. The
 * floats that round a region up to a multiple of 4, in either layout, and the zero tap and channel of stage 1's forward
 * weights are neither read nor written. All four buffers 16-byte aligned, none NULL. */
int nerfail_cnn_sgd_step(float* params, const float* grads, float* momentum_buf, float* packed, int num_classes, float lr,
                         float momentum, int first, void* stream);

/* MTR:170-186 on one lane. train_row, val_row: the two phases' stats rows; n_train, n_val >= 1: the DATASET lengths - losses
 * and accuracies divide by len(dataset), not by the views seen, so the views a drop_last loader skips count as wrong and as
 * loss 0, as in the reference (MTR:170-171). best: float32 [2] = {best validation accuracy, its epoch}, initialised by the
 * caller to {0, -1} (MTR:92). The epoch is taken exactly when its validation accuracy is > the best (MTR:181): a tie keeps the
 * earlier epoch, a NaN is never taken; then best is updated and *flag = 1, else *flag = 0 - the best weights are one
 * nerfail_copy_if(flag, params, best_params, n) away. Accuracies are compared as float32 (equal counts give equal floats).
 * record: float32 [NERFAIL_ATTACK_ROW_FLOATS] = {train loss, train acc, val loss, val acc, taken, best epoch, best acc, epoch,
 * train correct, train views, val correct, val views, 0, 0, 0, 0}. The rows are not written. */
int nerfail_cls_epoch_close(const float* train_row, const float* val_row, int64_t n_train, int64_t n_val, float* best, int epoch,
                            float* record, int32_t* flag, void* stream);

/* ------------------------------------------------------------------ DeepFool gate and step (deepfool revision 1) -- */

/* One DeepFool iteration of the universal attack (deepfool.py:53-105 = DF) without a torch op between the classifier and the
 * table: the break test and the margins f' on one wave, then the norms, the choice of the competing class and the update of
 * the table in one call. Like the three sections before it this one only ADDS entry points: NERFAIL_ABI_VERSION stays 14,
 * nerfail_abi_revision() stays 15, nerfail_eval_revision() and nerfail_cls_revision() stay 1, and the additions are announced
 * by nerfail_deepfool_revision() = 1. nerfail_deepfool_norms and nerfail_deepfool_apply are unchanged. No allocation, no
 * synchronisation, no atomics; the same bits on every run.
 *
 * The record one iteration's gate leaves for its step and for the host: 80 bytes of device memory, written with plain stores.
 * The host reads the first two words (one copy of 8 bytes per iteration: the loop's only wait). */
#define NERFAIL_DEEPFOOL_MAX_COMPETITORS 8
typedef struct nerfail_deepfool_record {
    int32_t done;      /* 1: the loop breaks before this iteration's step (DF:62-66); 0 also for a row that holds a NaN */
    int32_t argmax;    /* first maximum of the bumped logits (DF:59); -1 when the row holds a NaN */
    int32_t n_comp;    /* competitors: C - 1 untargeted (every k != o, ascending), 1 targeted ([target]) */
    int32_t targeted;  /* 0 / 1 */
    int32_t cls[NERFAIL_DEEPFOOL_MAX_COMPETITORS];   /* competitor r's class id; -1 from n_comp on */
    float fabs[NERFAIL_DEEPFOOL_MAX_COMPETITORS];    /* |f'| of competitor r (DF:79 / :93), from the BUMPED logits; 0 from n_comp on */
} nerfail_deepfool_record;
int nerfail_deepfool_revision(void);

/* DF:53-66 and the f' of DF:79 / :93 for one view, on one wave. cla: the [1,C] float32 logits of this iteration, 2 <= C <= 8;
 * o: the clean argmax, 0..C-1; target: -1 untargeted, else 0..C-1. Float32, in the reference's order:
 *   cla_b[c] = cla[c] + m1 for c == o (untargeted) or for every c != target (targeted), else cla[c]
 *   argmax   = the FIRST maximum of cla_b;   done = argmax != o (untargeted) / argmax == target (targeted)
 *   fabs[r]  = |cla_b[k_r] - (cla_b[o] + m2)| for the competitors k_r (the in-place bump of DF:54-57 makes the reference read
 *              the bumped values too)
 * A row holding a NaN (after the bump) has argmax -1 and is never done. Anything else is NERFAIL_EINVAL before the launch. */
int nerfail_deepfool_gate(const float* cla, int C, int o, int target, float m1, float m2, nerfail_deepfool_record* record,
                          void* stream);

/* DF:68-105 once the gradients exist. grads = [n_rhs][n,4], slice 0 the original class, slice r + 1 competitor r of the
 * record; n_rhs = record->n_comp + 1. Three launches: nerfail_deepfool_norms' first stage; one workgroup that finishes the
 * norms (the same fixed tree, the same bits as nerfail_deepfool_norms) and chooses; nerfail_deepfool_apply's kernel. The
 * choice, float32, one rounding per operation, no fused multiply-add:
 *   nrm_r = sqrt(norms2_r);   value_r = fabs[r] / (nrm_r + 1e-4f), a NaN counting as +inf;   best = the FIRST minimum (the
 *   strict < of DF:84; nothing is chosen when every value is +inf);   scale = fabs[best] / (nrm_best * nrm_best + 1e-4f) - the
 *   norm squared again, as DF:85 does, not norms2;   targeted: competitor 0 without a comparison (DF:92-96).
 * Nothing chosen: scale = 0, rot is left alone, *trace_slot = -1; else *trace_slot = cls[best]. A record whose n_comp is not
 * n_rhs - 1 chooses nothing: what the device read never becomes an address outside slices 1..n_rhs-1. Then
 *   rot += scale * (grads[best + 1] - grads[0]);   spatial_out = clamp(spatial_init + overshoot * rot, -255, 255), alpha
 *   channel copied from spatial_init (DF:98-105).
 * scratch: nerfail_deepfool_step_scratch_bytes(n_rhs, n) bytes, 8-byte aligned (0 for n_rhs outside 2..8 or n <= 0): the
 * partials, then {norms2[8], best, scale}; contents unspecified on return. trace_slot: a device int32 - the caller points it
 * at slot loop_i of a trace array. rot is updated in place; spatial_out may alias nothing else. */
size_t nerfail_deepfool_step_scratch_bytes(int n_rhs, int64_t n);
int nerfail_deepfool_step(const float* grads, int n_rhs, int64_t n, const nerfail_deepfool_record* record, void* scratch,
                          size_t scratch_bytes, float overshoot, const float* spatial_init, float* rot, float* spatial_out,
                          int32_t* trace_slot, void* stream);

/* ------------------------------------------------------------------ scene maps (scene revision 1) -- */

/* The 8-NN search with create_gauss_w as its epilogue: a view's point image straight to the [2,P,8] (weight, index) map the
 * attacks differentiate through (CI:126-163 + DW:82-97 in one launch, no [2,P,8] distance tensor in between). Like the four
 * sections before it this one only ADDS entry points: NERFAIL_ABI_VERSION stays 14, nerfail_abi_revision() stays 15, the eval,
 * cls and deepfool revisions stay 1, and the additions are announced by nerfail_scene_revision() = 1. nerfail_knn8_grid_search[_view]
 * and nerfail_gauss_weight are unchanged. No allocation, no synchronisation, no float atomics; the same bits on every run.
 *
 * weight_and_index[2, n_queries, 8] (16-byte aligned): plane 0 the weights, plane 1 the indices as float32 - bit for bit what
 * nerfail_knn8_grid_search[_view] followed by nerfail_gauss_weight(c) writes: d_k = sqrt(d2_k), g_k = exp(-(d_k/c)^2 / 2),
 * w_k = g_k / (sum g + 0.001) if sum g > 0 else 0, the sum in k = 0..7 order.
 * sum_d2 (a device double, may be NULL): the sum over all 8 * n_queries distances of the float32 product d * d (torch.square of
 * DW:92), added up in double in a fixed order - one partial per workgroup in `workspace`, then a one-wave fold.
 * grid_workspace: a grid built by nerfail_knn8_grid_build for n_points points (a count that contradicts the build this process
 * made in that workspace is NERFAIL_EINVAL). workspace: nerfail_knn8_grid_weights_workspace_bytes(n_queries) bytes, 8-byte
 * aligned (0 for n_queries <= 0); contents unspecified on return. c > 0. */
int nerfail_scene_revision(void);
size_t nerfail_knn8_grid_weights_workspace_bytes(int64_t n_queries);
int nerfail_knn8_grid_weights_view(const float* queries, int height, int width, int64_t n_points, float c, float* weight_and_index,
                                   double* sum_d2, const void* grid_workspace, size_t grid_workspace_bytes, void* workspace,
                                   size_t workspace_bytes, void* stream);
int nerfail_knn8_grid_weights(const float* queries, int64_t n_queries, int64_t n_points, float c, float* weight_and_index,
                              double* sum_d2, const void* grid_workspace, size_t grid_workspace_bytes, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ 2-D baseline (u2d revision 1) -- */

/* The IGSM-2D baseline (attack_IGSM_2D.py:263-416 = IG; model/GaussNet.py:340-385 = GN; MyDataset.py:235-294 = MD) around the
 * classifier: universal_2D_net's forward up to the classifier input in one streaming launch, and clip backward, sign step,
 * +-epsilon clamp and the write back into the per-view table in another. Like the five sections before it this one only ADDS
 * entry points: NERFAIL_ABI_VERSION stays 14, nerfail_abi_revision() stays 15, the eval, cls, deepfool and scene revisions stay 1,
 * and the additions are announced by nerfail_u2d_revision() = 1. No allocation, no synchronisation, no float atomics; the same
 * bits on every run. */
int nerfail_u2d_revision(void);

/* GN:356-370 with MD:247-255 for B views of a resident store, chosen by indices that live on the DEVICE. images: dense uint8
 * [N,P,4] (NERFAIL_EVAL_U8C4; base 16-byte aligned) or [N,P,3] (NERFAIL_EVAL_U8C3; base 4-byte aligned), as for
 * nerfail_cls_batch; idx int64 [B]; r float32 [N,P,3], view b using row idx[b] - or, with r_shared != 0, ONE [P,3] plane that
 * every view uses (the broadcast of GN:359-363). Per element, float32:
 *   o = the original on the white background of MD:247-255: rgb where alpha > 0, else 255 (nerfail_cls_batch's device function;
 *       a U8C3 store is taken as is);   v = o + r (one rounded add);   x = min(max(v, 0), 255), a NaN stays a NaN (torch.clip).
 * Outputs, each may be NULL but not both x_rgb and cls_in:
 *   x_rgb      float32 [B,P,3]  the attacked image (GN:367)
 *   cls_in     float32 [B,3,P]  the same values planar: the NCHW tensor of GN:369, channel order as stored
 *   pass_mask  uint8 [B,P]      bit c set when 0 <= v_c <= 255: where torch.clip's backward lets the gradient through (both
 *                               bounds inclusive; never for a NaN)
 * An index outside 0..N-1 writes views of NaN and a zero mask and reads nothing of either input. A lane owns four consecutive
 * pixels (one 16-byte load of a U8C4 store, three of r, three 16-byte stores into the planes) between a scalar head and tail,
 * as nerfail_cls_batch cuts a view; no byte outside the indexed views (and rows of r) is read. P >= 1; B <= 65535; B == 0 is a
 * no-op. r, x_rgb and cls_in 4-byte aligned (128-bit accesses are used wherever an address allows). */
int nerfail_u2d_fwd(const void* images, int format, int64_t N, int64_t P, const int64_t* idx, int B, const float* r, int r_shared,
                    float* x_rgb, float* cls_in, unsigned char* pass_mask, void* stream);

/* IG:335-379 in ONE launch, in place on rows idx[b] of the table r [N,P,3]. d_cls_in: float32 [B,3,P], the gradient of the loss
 * with respect to nerfail_u2d_fwd's cls_in; pass_mask: that call's mask. r_init: [N,P,3], or NULL for the zero table IG:250-252
 * starts from (the same bits as a tensor of zeros, without its N P 12 bytes). Per element, float32, one rounding per operation:
 *   g  = d where the mask bit is set, else 0 (torch.clip's backward)
 *   r' = r - a * sign(g) when targeted, else r + a * sign(g)         (torch.sign: sign(+-0) = 0, sign(NaN) = 0; IG:343-352)
 *   r' = max(r', init - epsilon);   r' = min(r', init + epsilon)     (in this order; a NaN on either side stays, IG:370-377)
 * The indices of one call must be distinct (the caller guarantees it: two workgroups would otherwise update one row). A row
 * whose index is outside 0..N-1 is skipped; no other row is read or written. epsilon >= 0 and a finite, else NERFAIL_EINVAL.
 * P >= 1; B <= 65535; B == 0 is a no-op. */
int nerfail_u2d_step(float* r, int64_t N, int64_t P, const int64_t* idx, int B, const float* d_cls_in,
                     const unsigned char* pass_mask, const float* r_init, float a, float epsilon, int targeted, void* stream);

/* IG:316, the image-loss statistic: adds the sum over [B,P,3] of (x_rgb - o)^2 into row[7,8] and the element count 3 P B into
 * row[9,10] of a NERFAIL_ATTACK_ROW_FLOATS stats row; o as in nerfail_u2d_fwd, from rows idx[b] of the store. The arithmetic and
 * the fixed summation order are nerfail_img_sqerr's: differences and squares in double, each lane its pixels in order, each
 * workgroup its lanes, one workgroup the partials; no atomics, the same bits on every run and for a U8C4 and a U8C3 store
 * holding the same values. A view whose index is outside 0..N-1 reads nothing and makes the sum NaN. scratch:
 * nerfail_img_sqerr_scratch_bytes() bytes, 8-byte aligned, contents unspecified on return. */
int nerfail_u2d_sqerr(const float* x_rgb, const void* images, int format, int64_t N, int64_t P, const int64_t* idx, int B,
                      void* scratch, float* row, void* stream);

/* IG:392-416: nerfail_attack_epoch_close with IG's STRICT rule - the epoch is taken only when its attack accuracy is < the best
 * so far (> when targeted; IG:408, 413): a tie keeps the earlier epoch. Row, best ({10000, 0, -1, 0} untargeted, {0, 0, -1, 0}
 * targeted, IG:255-261) and record layouts are those of nerfail_attack_epoch_close; one device function serves both. */
int nerfail_u2d_epoch_close(const float* row, float* best, int epoch, int targeted, float* record, int32_t* flag, void* stream);

/* ------------------------------------------------------------------ 2-D universal baseline (uap2d revision 1) -- */

/* The UAP-2D baseline (attack_UAP_2D.py:241-358 = UA; deepfool.py:10-111 with universal_2d = DF) around the classifier: one
 * DeepFool step on the ONE image-plane table [P,3] that every view shares (UA:219, GN:359-363), and the table's update with
 * the +-epsilon projection of UA:317-319. Like the six sections before it this one only ADDS entry points: NERFAIL_ABI_VERSION
 * stays 14, nerfail_abi_revision() stays 15, the eval, cls, deepfool, scene and u2d revisions stay 1, and the additions are
 * announced by nerfail_uap2d_revision() = 1. nerfail_deepfool_step chooses with the same device function as before (its bits
 * are unchanged). No allocation, no synchronisation, no atomics; the same bits on every run. */
int nerfail_uap2d_revision(void);

/* Float32 terms a lane of the norm kernel adds per competitor before it widens to double: two quads of four pixels, three
 * channels each. One norm workgroup (256 lanes) covers 256 * NERFAIL_UAP2D_NORM_TERMS / 3 = 2048 pixels. */
#define NERFAIL_UAP2D_NORM_TERMS 24

/* DF:68-102 with universal_2d once the gradients exist. grads = [n_rhs][3][P] planar float32, d logit / d classifier input
 * (nerfail_u2d_fwd's cls_in) of ONE view: row 0 the clean class o, row r + 1 competitor r of the record - what
 * nerfail_cnn_bwd_data_multi returns for one-hot rows, or n_rhs autograd.grad calls. pass_mask: uint8 [P], nerfail_u2d_fwd's
 * three bits per pixel of the forward the gradients belong to. r0, rot, r_out: float32 [P,3] interleaved (the table at the
 * call's start, the accumulated direction, the table the next forward runs on). Three launches, no host in between:
 *   norms   norms2[k-1] = sum over pixels p and channels c whose bit c of pass_mask[p] is set of (G_k - G_0)^2. A cleared bit
 *           contributes exactly 0 whatever the gradient holds there, a NaN included (torch.clip's backward, where(pass, grad, 0)).
 *           Pixels are taken in quads of four; lane t of workgroup b owns quads (2 b + i) * 256 + t, i = 0, 1, and adds their
 *           NERFAIL_UAP2D_NORM_TERMS terms in float32 in the order (quad, pixel, channel) - per term one rounded subtract, one
 *           rounded multiply, one rounded add, no fused multiply-add - then widens to double: the 64 lanes of a wave by
 *           butterfly, the four waves in order, one partial per workgroup and competitor in scratch.
 *   choose  one workgroup adds the partials in a fixed tree, rounds each norm to float32 once, and chooses exactly as
 *           nerfail_deepfool_step does (one device function; see there): first minimum, a NaN never chosen, competitor 0 when
 *           targeted. Nothing chosen: scale = 0, *trace_slot = -1; else *trace_slot = cls[best]. A record whose n_comp is not
 *           n_rhs - 1 chooses nothing.
 *   apply   per element, float32, one rounding per operation, no fused multiply-add:
 *             d = G_best - G_0 where the bit is set, else 0;   rot += scale * d;
 *             r_out = clamp(r0 + overshoot * rot, -255, 255) on all three channels (no alpha restore: DF:104), a NaN stays.
 *           scale == 0 or best outside 1..n_rhs-1 leaves rot alone and still writes r_out. A lane owns four consecutive pixels
 *           between a scalar head and tail cut at the 16-byte boundaries of rot; 128-bit accesses of the gradient planes and of
 *           r0 / rot / r_out, a 32-bit one of the mask, wherever an address allows.
 * scratch: nerfail_uap2d_step_scratch_bytes(n_rhs, P) bytes, 8-byte aligned (0 for n_rhs outside 2..8 or P outside 1..2^31):
 * the partials, then {norms2[8], best, scale}; contents unspecified on return, except that the caller may read norms2 there.
 * overshoot finite; every float pointer 4-byte aligned; rot is updated in place; r_out aliases nothing else. Anything else is
 * NERFAIL_EINVAL before the first launch. */
size_t nerfail_uap2d_step_scratch_bytes(int n_rhs, int64_t P);
int nerfail_uap2d_step(const float* grads, int n_rhs, int64_t P, const unsigned char* pass_mask,
                       const nerfail_deepfool_record* record, void* scratch, size_t scratch_bytes, float overshoot,
                       const float* r0, float* rot, float* r_out, int32_t* trace_slot, void* stream);

/* UA:317-319 with DF:109 in one stream, in place on the n = 3 P floats of the table; r_final: the table DeepFool ended on (its
 * r_out), the table itself being DeepFool's r0. Per element, float32, one rounding per operation:
 *   dr = r_final - t;   t' = t + dr;   table = clamp(t', -epsilon, +epsilon), a NaN stays (torch.clamp).
 * epsilon >= 0 (not NaN), 1 <= n <= 3 * 2^31, both pointers 4-byte aligned, else NERFAIL_EINVAL. */
int nerfail_uap2d_accumulate(float* table, const float* r_final, float epsilon, int64_t n, void* stream);

/* ------------------------------------------------------------------ poisoned retrain hand-off (poison revision 1) -- */

/* The hand-off from an attack's export epoch to the NeRF that is retrained on the attacked views (README "retrain";
 * load_blender.py = LB, run_nerf.py = RN), without the disk: the reference writes PNGs (AS:401-402), decodes them (LB:62-65) and
 * composites them on white (RN:587-588); here one pass over the float export fills a resident uint8 store and a resident float32
 * target store. Like the seven sections before it this one only ADDS entry points: NERFAIL_ABI_VERSION stays 14,
 * nerfail_abi_revision() stays 15, the eval, cls, deepfool, scene, u2d and uap2d revisions stay 1, and the additions are announced
 * by nerfail_poison_revision() = 1. nerfail_export_u8 is unchanged and rounds with the same device function. No allocation, no
 * synchronisation, no atomics, plain vector stores; the same bits on every run. */
int nerfail_poison_revision(void);

/* x: the export of B views, float32 [B,P,4] in BGRA order (x_rgba of NeRFail-S / NeRFail; 16-byte aligned) or [B,P,3] in BGR order
 * (x_rgb of IGSM-2D / UAP-2D; 4-byte aligned), `channels` saying which. slots_host: a HOST array of B slot numbers, each in
 * 0..n_slots-1, distinct within the call; view b goes to slot slots_host[b] of both stores:
 *   adv_u8  uint8 [n_slots,P,channels]  q = rintf(min(max(v, 0), 255)) per element (NaN -> 0), channel order as given: bit for bit
 *                                       what nerfail_export_u8 writes for the view, i.e. what cv2.imread(..., IMREAD_UNCHANGED)
 *                                       returns for the PNG cv2.imwrite makes of it.
 *   target  float32 [n_slots,P,3]       in RGB order, bit for bit what the file path makes of that uint8 image: every byte becomes
 *                                       u = (float)((double)q / 255.0) (LB:65: a float64 divide, then the cast); a 4-channel pixel is
 *                                       composited on white as fadd_rn(fmul_rn(u_c, u_a), fsub_rn(1.f, u_a)) (RN:588: three float32
 *                                       roundings, no fused multiply-add); a 3-channel pixel is taken as it is (RN:587).
 * Slots that no view of the call names are neither read nor written. A lane owns four consecutive pixels (16-byte loads and
 * stores) where a view's place in the stores allows it - both store bases 16-byte aligned and slot * P a multiple of 4 (for 3
 * channels also x 16-byte aligned and b * P a multiple of 4) - with a scalar tail; any other view is written pixel by pixel.
 * At most 16 views travel per launch, the function loops. Refused with NERFAIL_EINVAL before any launch: channels other than 3 or
 * 4, B outside 0..65535, P outside 1..2^31, n_slots < 1, a NULL pointer, a slot outside 0..n_slots-1, a slot named twice, x not
 * aligned as above, adv_u8 or target not 4-byte aligned. B == 0 is a no-op. */
int nerfail_export_train_views(const float* x, int channels, int B, int64_t P, const int32_t* slots_host, int64_t n_slots,
                               unsigned char* adv_u8, float* target, void* stream);

/* ------------------------------------------------------------------ classifier-input resize (resize revision 1) -- */

/* The stage in front of a stock victim classifier (GaussNet.py:121-157, model_test.py:283-290): white background, NHWC -> NCHW and
 * the antialiased bilinear resize to the classifier's side (299; 224 for vit_b_16), as one kernel with an exact adjoint. Like the
 * eight sections before it this one only ADDS entry points: NERFAIL_ABI_VERSION stays 14, nerfail_abi_revision() stays 15, the eval,
 * cls, deepfool, scene, u2d, uap2d and poison revisions stay 1, and the additions are announced by nerfail_resize_revision() = 1.
 * The arithmetic is fixed down to the order of the float32 operations (tests/resize_ref.py restates it in numpy):
 *
 *   axis table, n_in -> n_out, in double: scale = n_in / n_out; support = scale >= 1 ? scale : 1; inv = scale >= 1 ? 1 / scale : 1;
 *     output i: c = scale * (i + 0.5); start = max(0, (int)(c - support + 0.5)); count = min(n_in, (int)(c + support + 0.5)) - start;
 *     w[k] = max(0, 1 - |(k + start - c + 0.5) * inv|) for k = 0..count-1, divided by their sum (added in that order), then rounded
 *     ONCE to float32: aten's _upsample_bilinear2d_aa with align_corners = false.
 *   inverted table: input j is covered by the outputs ostart[j] .. ostart[j] + ocount[j] - 1 (those whose [start, start + count)
 *     holds j): one contiguous, non-empty range.
 *   forward, per channel, every product and every sum rounded to float32 on its own (no fused multiply-add):
 *     t[y][ox]    = w_x[ox][0] * v[y][xs]  (+ w_x[ox][k] * v[y][xs + k], k = 1..count-1, in that order), xs = start_x[ox];
 *     out[oy][ox] = w_y[oy][0] * t[ys][ox] (+ w_y[oy][k] * t[ys + k][ox], k = 1..count-1, in that order), ys = start_y[oy].
 *   adjoint: tmp[y][ox] = sum over oy ascending in the inverted range of y of w_y[oy][y - ys] * g[oy][ox];
 *            gx[y][x]   = sum over ox ascending in the inverted range of x of w_x[ox][x - xs] * tmp[y][ox];
 *     the first product starts each sum, as in the forward.
 * No allocation on the device, no synchronisation, no atomics, no global scratch; the same bits on every run. */
int nerfail_resize_revision(void);

#define NERFAIL_RESIZE_MAX_TAPS 16

/* Pure host functions. nerfail_resize_aa_kmax: the largest count of the axis n_in -> n_out (the row length of w), or 0 when n_in or
 * n_out < 1. nerfail_resize_aa_table fills caller-owned HOST arrays: start[n_out], count[n_out], w[n_out][kmax] (a row's floats
 * from count on are +0), ostart[n_in], ocount[n_in]. NERFAIL_EINVAL, with nothing promised about the arrays: n_in or n_out < 1,
 * a NULL array, kmax below the axis' largest count, any count or ocount above NERFAIL_RESIZE_MAX_TAPS (a scale above ~7.5, or
 * below ~1/7.5), or an inverted range that would not be contiguous and non-empty. */
int nerfail_resize_aa_kmax(int n_in, int n_out);
int nerfail_resize_aa_table(int n_in, int n_out, int32_t* start, int32_t* count, float* w, int kmax, int32_t* ostart,
                            int32_t* ocount);

/* One axis' tables on the DEVICE, exactly what nerfail_resize_aa_table wrote (the struct itself lives on the host). */
typedef struct nerfail_resize_axis {
    const int32_t* start;    /* [n_out] */
    const int32_t* count;    /* [n_out] */
    const float* w;          /* [n_out][kmax] */
    const int32_t* ostart;   /* [n_in] */
    const int32_t* ocount;   /* [n_in] */
    int32_t n_in, n_out, kmax, reserved;
} nerfail_resize_axis;

/* The tiles the two kernels take for H x W -> oh x ow: fwd_tile = {output rows, output columns} of a forward workgroup, bwd_tile =
 * {source rows, source columns} of an adjoint workgroup. The largest of a fixed ladder (forward 16 x 32 down to 2 x 8, adjoint
 * 16 x 64 down to 1 x 8) whose source (gradient) window, intermediate and staged weights fit 80 KiB of LDS, so two workgroups share
 * a CU's 160 KiB. NERFAIL_EINVAL when an axis' table is refused or a pointer is NULL. */
int nerfail_resize_tiles(int H, int W, int oh, int ow, int32_t* fwd_tile, int32_t* bwd_tile);

/* Source value v: layout 0 = src float32 [B,H,W,4] (x_rgba; 16-byte aligned), v = a > 0 ? c : 255 for the first three channels c of
 * a pixel with fourth channel a (a = 0, -0, negative, NaN: 255, as torch.where(a > 0, c, 255)); layout 1 = src float32 [B,3,H,W],
 * taken as it is. out: float32 [B,3,oh,ow], every element written. One workgroup owns an output tile of one view, all three
 * channels: the source window goes to LDS once (layout 0: one 16-byte load per pixel, the background rule applied on the way in),
 * the horizontal pass runs LDS -> LDS, the vertical pass LDS -> registers, the store is coalesced along ox; weights are read from
 * the tables. Whatever the tables hold, no global access leaves src [B,H,W,*] or out [B,3,oh,ow]; the VALUES are the definition's
 * only for tables written by nerfail_resize_aa_table for H -> oh (ty) and W -> ow (tx).
 * Refused with NERFAIL_EINVAL before a launch: a NULL pointer (src, out, ty, tx or a table pointer), layout other than 0 or 1,
 * B outside 1..65535, H, W, oh or ow < 1, ty / tx not of H -> oh / W -> ow (n_in, n_out), kmax outside 1..16 or below the axis'
 * largest count, an axis nerfail_resize_aa_table refuses, src not aligned (16 bytes for layout 0, else 4), out not 4-byte aligned. */
int nerfail_cls_input_resize_fwd(const float* src, int layout, int B, int H, int W, int oh, int ow, const nerfail_resize_axis* ty,
                                 const nerfail_resize_axis* tx, float* out, void* stream);

/* The adjoint for R right-hand sides of one forward: g float32 [R,B,3,oh,ow] -> gsrc. Layout 0: gsrc [R,B,H,W,4] (16-byte aligned),
 * the first three channels a > 0 ? gx : +0 with a the fourth channel of src (the forward's input, needed for nothing else), the
 * fourth channel 0 - what autograd gives through torch.where. Layout 1: gsrc [R,B,3,H,W]; src is not read and may be NULL. Every
 * element of gsrc is written. One workgroup owns a source tile of one view and loops over r: the g window is staged in LDS, the
 * vertical pass runs LDS -> LDS, the horizontal pass LDS -> registers, layout 0 stores 16 bytes per pixel. Slice r is, bit for
 * bit, what the call returns for g[r] alone (R = 1). Refused with NERFAIL_EINVAL before a launch: everything the forward refuses
 * (g and gsrc in the places of src and out), R outside 1..8, layout 0 with a NULL src. */
int nerfail_cls_input_resize_bwd(const float* g, int R, const float* src, int layout, int B, int H, int W, int oh, int ow,
                                 const nerfail_resize_axis* ty, const nerfail_resize_axis* tx, float* gsrc, void* stream);

/* ------------------------------------------------------------------ foreground-only scene maps (fg revision 1) -- */

/* Scene maps over the pixels the attacks read. gauss_net writes 0 to x_rgba and takes no gradient wherever the view's registered
 * BGRA image has alpha <= 0, so a view's map matters only on its FOREGROUND, the pixels with alpha > 0: these entry points list
 * them, make rays for the list and search for the list. Like the nine sections before it this one only ADDS entry points:
 * NERFAIL_ABI_VERSION stays 14, nerfail_abi_revision() stays 15, every other revision stays 1, and the additions are announced by
 * nerfail_fg_revision() = 1. nerfail_ray_gen and nerfail_knn8_grid_weights[_view] are unchanged. No allocation on the device, no
 * synchronisation, no float atomics; the same bits on every run.
 *
 * nerfail_fg_pixel_list: bgra = one uint8 BGRA view of n_pixels pixels (4-byte aligned; 1 <= n_pixels < 2^31). Writes
 * list[0..n) = the indices row * W + col of the pixels with A > 0, strictly ascending, and *count = n, both on the device (list
 * holds n_pixels int32; elements from n on are not written). An ordered stream compaction in three launches - ballot and popcount
 * per wave into one count per workgroup, an exclusive scan of the counts, the write - whose order does not depend on scheduling.
 * workspace: nerfail_fg_pixel_list_workspace_bytes(n_pixels) bytes (0 for a count outside the range), 4-byte aligned; contents
 * unspecified on return.
 *
 * nerfail_ray_gen_list: rays[n,11]; row j is bit for bit the row nerfail_ray_gen writes for pixel pix[j] of the H x W view (one
 * device function behind both). n = 0 is valid and launches nothing. H * W < 2^31.
 *
 * nerfail_knn8_grid_weights_list: nerfail_knn8_grid_weights over the n compact queries (64 consecutive queries per wave), with
 * query j's weights and indices written to row pix[j] of the two planes of weight_and_index[2, n_pixels, 8] (16-byte aligned). The
 * same call first zeroes ALL of weight_and_index on the same stream (+0: weight 0, index 0), so every row not named by pix is zero
 * bits. A listed row is bit for bit the row nerfail_knn8_grid_weights[_view] writes for that query. sum_d2 (device double, may be
 * NULL): the fixed-order double fold over the 8 n listed distances only. n = 0 is valid: the map is all zero, *sum_d2 = 0, no search
 * is launched (queries, pix and workspace may then be NULL). workspace: nerfail_knn8_grid_weights_workspace_bytes(n) bytes, 8-byte
 * aligned, needed when sum_d2 is given. The VALUES of pix are the caller's contract (distinct, in [0, n_pixels) - a list made by
 * nerfail_fg_pixel_list); a value outside [0, n_pixels) stores nothing. Refused with NERFAIL_EINVAL before any launch: n_pixels
 * outside [1, 2^31), n outside [0, n_pixels], n_points outside [8, 2^24), c not > 0, a NULL or misaligned pointer, a workspace or
 * grid workspace that is too small, a point count that contradicts the grid built in grid_workspace. */
int nerfail_fg_revision(void);
size_t nerfail_fg_pixel_list_workspace_bytes(int64_t n_pixels);
int nerfail_fg_pixel_list(const uint8_t* bgra, int64_t n_pixels, int32_t* list, int32_t* count, void* workspace,
                          size_t workspace_bytes, void* stream);
int nerfail_ray_gen_list(int H, int W, const float* K4_host, const float* c2w_host, float near_, float far_, const int32_t* pix,
                         int64_t n, float* rays, void* stream);
int nerfail_knn8_grid_weights_list(const float* queries, int64_t n, const int32_t* pix, int64_t n_pixels, int64_t n_points, float c,
                                   float* weight_and_index, double* sum_d2, const void* grid_workspace, size_t grid_workspace_bytes,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ victim classifier (MyCNN) -- */

/* The MyCNN classifier of model/MyModel.py:5-52 (ABI 9): seven stages of 3x3 valid conv + bias + ReLU + 2x2 floor max-pool
 * (3-32-64-128-256-256-128-64 channels), fc1 1024->512 + ReLU, fc2 512->num_classes. Input x: [B,3,H,W] float32 NCHW;
 * H and W must make the seventh stage 4 x 4 (766..893). Conv stages run on v_mfma_f32_32x32x2_f32; no atomics, results are
 * bitwise reproducible.
 *   pack:       params_host = HOST array of the 18 DEVICE parameter pointers in state_dict order (conv1.weight, conv1.bias,
 *               ..., conv7.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias) -> packed (nerfail_cnn_packed_floats floats).
 *   fwd:        logits [B,num_classes]; workspace (nerfail_cnn_workspace_bytes): every stage's pooled NHWC output and the FC
 *               hidden layer, kept for the backward; masks (nerfail_cnn_mask_bytes): 2-bit pool argmax codes, or NULL for
 *               inference only.
 *   bwd_data:   d_x [B,3,H,W] (NCHW) from d_logits [B,num_classes], the forward's workspace and masks (weights frozen);
 *               scratch: nerfail_cnn_bwd_scratch_bytes bytes. Inputs are not written: callable any number of times.
 * The size helpers return 0 for unsupported shapes.
 *
 * Buffer contract (what tests/cnn_ref.py decodes; all buffers are plain caller-owned memory). Stage s = 0..6 has input
 * hin x win (stage 0: H x W), Cout_s = 32, 64, 128, 256, 256, 128, 64 output channels and a pooled output of
 * hp x wp = (hin - 2) / 2 x (win - 2) / 2 (floor), which is the next stage's input.
 *   workspace:  stage s = 0..6 pooled output [B, hp_s, wp_s, Cout_s] (NHWC) float32, the stages back to back, then
 *               hidden [B, 512] (fc1's output after the ReLU). fwd writes every element.
 *   masks:      per stage [B, hp][ceil(wp / 8)][2][Cout] bytes, the stages back to back. The byte at
 *               (b, pr, pc >> 3, pc & 1, ch) holds, at bits 2 * ((pc & 7) >> 1) and the one above, the window position
 *               2 * dy + dx of pooled cell (pr, pc): the first maximum of the window wins, a NaN wins over any number (the
 *               last NaN of a window). fwd writes every byte; the cells of a byte beyond wp are unspecified and never read.
 *               bwd_data routes the gradient of a cell to the coded position unless the cell's workspace value is <= 0
 *               (NaN passes), and gates d hidden where hidden <= 0.
 *   scratch:    of bwd_data; contents unspecified on return.
 *   packed:     regions in this order, each rounded up to 4 floats (the round-up's contents unspecified): per stage
 *               s = 0..6 the forward weights [Cout][tap][Cin] (tap = 3 ky + kx; stage 0: [32][10 taps][4 channels], the
 *               tenth tap and the fourth channel exactly 0), the bias [Cout], and for s >= 1 the backward weights
 *               [Cin][tap][Cout] (taps not flipped); then conv1.weight as it is [32][3][9]; fc1T [1024][512] and fc1P
 *               [512][1024], fc1.weight with its 1024 columns reordered from c * 16 + y * 4 + x to (y * 4 + x) * 64 + c
 *               (NHWC), transposed and not; fc1.bias [512]; fc2.weight [num_classes][512]; fc2.bias [num_classes]. */
size_t nerfail_cnn_packed_floats(int num_classes);
int nerfail_cnn_pack(const float* const* params_host, int num_classes, float* packed, void* stream);
size_t nerfail_cnn_workspace_bytes(int B, int H, int W, int num_classes);
size_t nerfail_cnn_mask_bytes(int B, int H, int W);
size_t nerfail_cnn_bwd_scratch_bytes(int B, int H, int W);
int nerfail_cnn_fwd(const float* packed, int num_classes, const float* x, int B, int H, int W, float* workspace,
                    unsigned char* masks, float* logits, void* stream);
int nerfail_cnn_bwd_data(const float* packed, int num_classes, const float* workspace, const unsigned char* masks,
                         const float* d_logits, int B, int H, int W, float* scratch, float* d_x, void* stream);

/* ABI 10. bwd_data for R right-hand sides of ONE forward in one launch chain (DeepFool: the input gradients of up to 8 class
 * logits of one view, where a batch-1 backward leaves most of the chip idle in the late stages). Slice r of d_x is, bit for
 * bit, what nerfail_cnn_bwd_data returns for d_logits[r] with the same workspace and masks: the kernels are the same, run
 * with one grid slice per (r, b), and no sum changes its order. nerfail_cnn_bwd_data is the R = 1 case.
 *   R >= 1 and R * B <= 65535 (the grid's z dimension carries r * B + b); anything else is NERFAIL_EINVAL, and
 *   nerfail_cnn_bwd_multi_scratch_bytes returns 0 for it as for an unsupported H x W.
 * Buffer contract for R > 1 - what is indexed by the image b of the forward and what by the gradient slice r * B + b:
 *   by b (B images, read only, exactly what nerfail_cnn_fwd wrote for B images):
 *               workspace (every stage's pooled output, the FC hidden layer) and masks (pool argmax codes);
 *   by r * B + b (R * B slices):
 *               d_logits [R,B,num_classes] (read only), d_x [R,B,3,H,W] (every element written), and scratch
 *               (nerfail_cnn_bwd_multi_scratch_bytes(R, B, H, W) bytes = R x the single backward's; every stage's gradient
 *               lives there as [R * B, h, w, C] NHWC; contents unspecified on return).
 * No allocation, no synchronisation, no atomics; inputs are never written, so the call may be repeated. */
size_t nerfail_cnn_bwd_multi_scratch_bytes(int R, int B, int H, int W);
int nerfail_cnn_bwd_data_multi(const float* packed, int num_classes, const float* workspace, const unsigned char* masks,
                               const float* d_logits /* [R,B,num_classes] */, int R, int B, int H, int W, float* scratch,
                               float* d_x /* [R,B,3,H,W] */, void* stream);

/* ABI 11. Weight gradients: everything a training step of the classifier needs from one backward pass. Runs
 * nerfail_cnn_bwd_data's chain (the same kernels, grids and arguments) keeping every stage's pooled gradient, then forms the
 * gradient of all 18 parameters. Conv stages: dW[co][ci][ky][kx] = sum over b and conv pixels (y, x) of
 * G[b,y,x,co] X[b,y+ky,x+kx,ci] and db[co] = sum G[b,y,x,co], with G the un-pooled gradient (the pooled gradient at the coded
 * window position unless the cell's workspace value is <= 0; NaN passes) and X the stage input, on v_mfma_f32_32x32x2_f32
 * (exact f32 products, f32 accumulate). The pixel range is split over workgroups into partial slabs that a second kernel adds
 * in a fixed order: no float atomics, every output written by one lane, two calls give the same bits.
 *   x:          the forward's input [B,3,H,W] (stage 1's dW reads it); workspace, masks: what nerfail_cnn_fwd wrote (masks
 *               kept); d_logits [B,num_classes]. None of them is written.
 *   d_x:        [B,3,H,W] or NULL. When given, bit for bit what nerfail_cnn_bwd_data writes for the same inputs.
 *   d_params:   nerfail_cnn_grad_floats(num_classes) floats, nn.Module layout in state-dict order, each region starting on a
 *               multiple of 4 floats (16 bytes): conv1.weight [32][3][3][3], conv1.bias [32], ..., conv7.weight [64][128][3][3],
 *               conv7.bias [64], fc1.weight [512][1024] (columns c * 16 + y * 4 + x, PyTorch's flatten order), fc1.bias [512],
 *               fc2.weight [num_classes][512], fc2.bias [num_classes]. Every parameter's floats are overwritten (nothing is
 *               accumulated); the floats that round a region up to a multiple of 4 are never written.
 *   scratch:    nerfail_cnn_bwd_weights_scratch_bytes(B, H, W, num_classes) bytes, any contents on entry. On return, as
 *               floats: for s = 0..6 back to back the gradient with respect to stage s's POOLED output,
 *               [B, hp_s, wp_s, Cout_s] NHWC (the layout and sizes of the workspace's stage outputs; stage 6's is fc1's input
 *               gradient), then d hidden [B, 512] (gated: 0 where hidden <= 0), then the partial slabs (contents
 *               unspecified). Every element of the seven gradients and of d hidden is written.
 * The size helpers return 0 for unsupported arguments. No allocation, no synchronisation; callable any number of times. */
size_t nerfail_cnn_grad_floats(int num_classes);
size_t nerfail_cnn_bwd_weights_scratch_bytes(int B, int H, int W, int num_classes);
int nerfail_cnn_bwd_weights(const float* packed, int num_classes, const float* x, const float* workspace,
                            const unsigned char* masks, const float* d_logits, int B, int H, int W, float* scratch,
                            float* d_params, float* d_x /* or NULL */, void* stream);

/* bf16x3: a second, opt-in arithmetic for the victim's conv stages 2..7, forward and backward-data, on
 * v_mfma_f32_32x32x16_bf16 (csrc/cnn_x3.hip). Only ADDS entry points: NERFAIL_ABI_VERSION stays 14, nerfail_abi_revision() stays
 * 15, every other revision stays 1, and the additions are announced by nerfail_cnn_x3_revision() = 1. The exact entry points
 * above, their kernels and their bits are unchanged.
 * Arithmetic: both operands of every product are split by three round-to-nearest-even conversions to bf16 (8 significant
 * bits), x = x0 + x1 + x2 with |x1| <= 2^-8 |x|, |x2| <= 2^-16 |x| and each subtraction exact in f32; nothing is left over
 * while the pieces are normal numbers. Of the nine piece products the six a1b1, a0b2, a2b0, a0b1, a1b0, a0b0 are kept and issued
 * in that order (smallest first) into ONE f32 accumulator per output element, one step of 16 channels (k16) after another in a
 * fixed order (the nine taps of a 16-channel slice, the slices ascending). A bf16 x bf16 product is exact in f32; what is
 * dropped (a1b2 + a2b1 + a2b2) is at most 2^-23 |a||b| per product in the worst case, about 2^-26 |a||b| on average, per
 * product. The results are f32-accurate, not bitwise those of the exact kernels. No float atomics, every output is written by
 * one lane, two calls give the same bits.
 * Special values: bf16 has the f32 exponent range, so nothing is pre-scaled. A NaN is NaN in all three pieces: NaN inputs give
 * NaN at the positions where the exact kernels give NaN. +-Inf (and a finite |x| >= 2^128 (1 - 2^-9), which rounds to a bf16
 * Inf) becomes NaN, because Inf - Inf happens in the split.
 * Scope: stage 1 in both directions, the FC head in both directions and every weight gradient stay on the exact kernels, called
 * as they are: the x3 forward's stage-1 output and mask codes are bit for bit the exact forward's. Activations and gradients
 * stay f32 in global memory: workspace, masks, scratch and d_x have exactly the contracts, sizes and size functions of
 * nerfail_cnn_fwd / nerfail_cnn_bwd_data / nerfail_cnn_bwd_data_multi, so what an x3 forward wrote can be consumed by either
 * backward family and vice versa. The refusals are the exact entry points' (shapes, NULL pointers, R * B <= 65535); slice r of
 * nerfail_cnn_bwd_data_multi_x3 is bit for bit nerfail_cnn_bwd_data_x3 of row r.
 *   packed_x3:  nerfail_cnn_x3_packed_bytes(num_classes) bytes (0 for an unsupported num_classes; the size does not depend on
 *               it otherwise), 16-byte aligned, made by nerfail_cnn_pack_x3 from `packed` on the device. For stage s = 1..6,
 *               back to back, the forward image and then the backward image, each the split of the same region of `packed`
 *               (forward [Cout][tap][Cin], backward [Cin][tap][Cout], written [NC][9][KC] here):
 *                   [KC / 16 slices][NC rows][9 taps][3 planes][16 channels] bf16,
 *               plane p = piece p of the split (largest first), channel c of slice cb = K-channel 16 cb + c.
 *   Every x3 call takes `packed` as well (bias, stage 1, the FC head). */
int nerfail_cnn_x3_revision(void);
size_t nerfail_cnn_x3_packed_bytes(int num_classes);
int nerfail_cnn_pack_x3(const float* packed, int num_classes, void* packed_x3, void* stream);
int nerfail_cnn_fwd_x3(const float* packed, const void* packed_x3, int num_classes, const float* x, int B, int H, int W,
                       float* workspace, unsigned char* masks, float* logits, void* stream);
int nerfail_cnn_bwd_data_x3(const float* packed, const void* packed_x3, int num_classes, const float* workspace,
                            const unsigned char* masks, const float* d_logits, int B, int H, int W, float* scratch, float* d_x,
                            void* stream);
int nerfail_cnn_bwd_data_multi_x3(const float* packed, const void* packed_x3, int num_classes, const float* workspace,
                                  const unsigned char* masks, const float* d_logits /* [R,B,num_classes] */, int R, int B, int H,
                                  int W, float* scratch, float* d_x /* [R,B,3,H,W] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFAIL_HIP_H */
