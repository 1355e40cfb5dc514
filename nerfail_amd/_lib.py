"""ctypes binding of libnerfail_hip.so (the C ABI declared in include/nerfail_hip.h).

There is NO CPU fallback anywhere in this package: if the library is missing, or a tensor is not a
contiguous float32 HIP tensor, the call raises. PyTorch is used for device memory and streams only.
"""
import ctypes
import os

import torch  # noqa: F401  (must be imported first: libnerfail_hip.so binds to torch's libamdhip64.so.7)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NERFAIL_HIP_LIB') or os.path.join(_HERE, 'lib', 'libnerfail_hip.so')   # override: A/B builds (tools/ablate.py)

ABI_VERSION = 14
ABI_REVISION = 15                        # additions since ABI_VERSION (nerfail_abi_revision): the NeRFail-S epoch statistics
EVAL_REVISION = 1                        # nerfail_eval_revision: the attack-evaluation entry points (model_test)
CLS_REVISION = 1                         # nerfail_cls_revision: the victim-training entry points (model_train)
DEEPFOOL_REVISION = 1                    # nerfail_deepfool_revision: the DeepFool gate and step (deepfool.deepfool_native)
SCENE_REVISION = 1                       # nerfail_scene_revision: the 8-NN search with the Gaussian weights as its epilogue (scene)
U2D_REVISION = 1                         # nerfail_u2d_revision: the IGSM-2D baseline's forward, step and statistics (attack.igsm_2d)
UAP2D_REVISION = 1                       # nerfail_uap2d_revision: the UAP-2D baseline's DeepFool step and projection (attack.uap_2d)
POISON_REVISION = 1                      # nerfail_poison_revision: the export -> training-target hand-off (retrain.PoisonedTrainSet)
RESIZE_REVISION = 1                      # nerfail_resize_revision: the classifier-input resize and its adjoint (_resize.classifier_input)
CNN_X3_REVISION = 1                      # nerfail_cnn_x3_revision: the bf16x3 arithmetic of the MyCNN victim (MyCNN(precision='bf16x3'))
FG_REVISION = 1                          # nerfail_fg_revision: pixel list, list rays and list search of foreground-only scene maps (scene)
RESIZE_MAX_TAPS = 16                     # NERFAIL_RESIZE_MAX_TAPS
UAP2D_NORM_TERMS = 24                   # NERFAIL_UAP2D_NORM_TERMS: float32 terms per lane of nerfail_uap2d_step's norms
DEEPFOOL_MAX_COMPETITORS = 8             # NERFAIL_DEEPFOOL_MAX_COMPETITORS
DEEPFOOL_RECORD_WORDS = 4 + 2 * DEEPFOOL_MAX_COMPETITORS    # struct nerfail_deepfool_record as 32-bit words
EVAL_U8C4, EVAL_U8C3, EVAL_F32C4, EVAL_FLAT = 0, 1, 2, 3    # NERFAIL_EVAL_*: image formats of nerfail_eval_view_metrics
EVAL_VIEW_DOUBLES = 6                    # NERFAIL_EVAL_VIEW_DOUBLES: one view's row
EVAL_RECORD_DOUBLES = 16 + 32            # NERFAIL_EVAL_RECORD_DOUBLES: the set record of nerfail_eval_fold
ATTACK_ROW_FLOATS = 16                   # NERFAIL_ATTACK_ROW_FLOATS: the stats row and the epoch record of attack.nerfail_s
MAX_DEPTH = 16
DW_BF16X3, DW_ACCUMULATE = 1, 2          # flags of nerfail_mlp_bwd_weights
RAY_FLOATS = 11

c_f = ctypes.c_float
c_i = ctypes.c_int
c_i64 = ctypes.c_int64
c_u64 = ctypes.c_uint64
c_p = ctypes.c_void_p


class NerfailError(RuntimeError):
    """A libnerfail_hip call returned a NERFAIL_E* code."""


class MlpParams(ctypes.Structure):
    """struct nerfail_mlp_params (include/nerfail_hip.h)."""
    _fields_ = [('D', ctypes.c_int32), ('W', ctypes.c_int32), ('input_ch', ctypes.c_int32),
                ('input_ch_views', ctypes.c_int32), ('skip', ctypes.c_int32), ('reserved', ctypes.c_int32),
                ('pts_w', c_p * MAX_DEPTH), ('pts_b', c_p * MAX_DEPTH),
                ('views_w', c_p), ('views_b', c_p), ('feature_w', c_p), ('feature_b', c_p),
                ('alpha_w', c_p), ('alpha_b', c_p), ('rgb_w', c_p), ('rgb_b', c_p)]


def mlp_params(D, W, input_ch, input_ch_views, skip, tensors, keep):
    """struct nerfail_mlp_params over `tensors`: 2 D + 8 of them in _train.ordered_params order - the parameters of a network,
    or the buffers that receive their gradients. With a list `keep`, every tensor that is not contiguous float32 is copied and
    all of them are appended to `keep`: the caller holds that list until the launch reading the struct has been enqueued,
    or the copies are freed under it. keep=None takes the pointers of the tensors as they are (outputs, where a copy would
    swallow the result: the caller passes contiguous float32 and keeps them alive itself)."""
    if keep is not None:
        tensors = [f32c(t) for t in tensors]
        keep += tensors
    ptrs = [t.data_ptr() for t in tensors]
    if len(ptrs) != 2 * D + 8:
        raise ValueError('nerfail_mlp_params: D = %d takes %d tensors (got %d)' % (D, 2 * D + 8, len(ptrs)))
    mp = MlpParams()
    mp.D, mp.W, mp.input_ch, mp.input_ch_views, mp.skip = D, W, input_ch, input_ch_views, skip
    for i in range(D):
        mp.pts_w[i], mp.pts_b[i] = ptrs[2 * i], ptrs[2 * i + 1]
    (mp.views_w, mp.views_b, mp.feature_w, mp.feature_b, mp.alpha_w, mp.alpha_b, mp.rgb_w, mp.rgb_b) = ptrs[2 * D:]
    return mp


# name -> (restype, argtypes); every symbol include/nerfail_hip.h declares
SIGNATURES = {
    'nerfail_abi_version': (c_i, []),
    'nerfail_last_error': (ctypes.c_char_p, []),
    'nerfail_device_name': (c_i, [ctypes.c_char_p, ctypes.c_size_t]),
    'nerfail_get_rays': (c_i, [c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    'nerfail_pack_rays': (c_i, [c_p, c_p, c_i64, c_f, c_f, c_p, c_p]),
    'nerfail_ray_gen': (c_i, [c_i, c_i, c_p, c_p, c_f, c_f, c_i64, c_i64, c_p, c_p]),
    'nerfail_index_shuffle': (c_i, [c_u64, c_i64, c_i64, c_i64, c_p, c_p]),
    'nerfail_train_batch': (c_i, [c_i, c_i, c_p, c_f, c_f, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_u64, c_i64, c_i64,
                                  c_p, c_p, c_p, c_p]),
    'nerfail_sample_coarse': (c_i, [c_p, c_i64, c_p, c_i, c_p, c_i, c_p, c_p, c_p]),
    'nerfail_sample_pdf': (c_i, [c_p, c_p, c_i64, c_i, c_p, c_i, c_i, c_p, c_p]),
    'nerfail_sample_fine': (c_i, [c_p, c_i64, c_p, c_p, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p]),
    'nerfail_embed': (c_i, [c_p, c_i64, c_i, c_p, c_p]),
    'nerfail_mlp_packed_floats': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_mlp_pack': (c_i, [ctypes.POINTER(MlpParams), c_p, c_p]),
    'nerfail_mlp_fwd': (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p]),
    'nerfail_mlp_fwd_rays': (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p, c_p]),
    'nerfail_mlp_fwd_select': (c_i, [c_i]),
    'nerfail_mlp_bwd_select': (c_i, [c_i]),
    'nerfail_mlp_fwd_embedded': (c_i, [c_p, c_i, c_i, c_i, c_p, c_i64, c_p, c_p]),
    'nerfail_mlp_packed_x3_bytes': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_mlp_pack_x3': (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    'nerfail_mlp_fwd_x3': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p]),
    'nerfail_mlp_fwd_embedded_x3': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_i64, c_p, c_p]),
    'nerfail_mlp_fwd_rays_x3': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p, c_p]),
    'nerfail_mlp_packed_x3f_bytes': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_mlp_x3f_composed_floats': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_mlp_pack_x3f': (c_i, [c_p, c_i, c_i, c_i, c_p, c_p]),
    'nerfail_mlp_fwd_x3f': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p]),
    'nerfail_mlp_fwd_embedded_x3f': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_i64, c_p, c_p]),
    'nerfail_mlp_fwd_rays_x3f': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p, c_p]),
    'nerfail_mlp_x3f_raybias_floats': (ctypes.c_size_t, [c_i, c_i, c_i, c_i64, c_i]),
    'nerfail_mlp_x3_raybias_select': (c_i, [c_i]),
    'nerfail_mlp_x3f_viewbias': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_p, c_p]),
    'nerfail_mlp_fwd_x3f_raybias': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p, c_p]),
    'nerfail_mlp_fwd_rays_x3f_raybias': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p, c_p]),
    'nerfail_mlp_f16_image_bytes': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_mlp_pack_f16': (c_i, [ctypes.POINTER(MlpParams), c_p, c_p]),
    'nerfail_mlp_fwd_f16': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p]),
    'nerfail_mlp_fwd_f16_train': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p, c_p]),
    'nerfail_mlp_f16_image_T_bytes': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_mlp_pack_f16_T': (c_i, [ctypes.POINTER(MlpParams), c_p, c_p]),
    'nerfail_mlp_bwd_data_f16': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_p, c_p]),
    'nerfail_mlp_train_acts_floats': (ctypes.c_size_t, [c_i, c_i, c_i64]),
    'nerfail_mlp_train_dz_floats': (ctypes.c_size_t, [c_i, c_i, c_i64]),
    'nerfail_mlp_fwd_train': (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_i, c_p, c_p, c_p]),
    'nerfail_mlp_packed_T_floats': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_mlp_pack_T': (c_i, [ctypes.POINTER(MlpParams), c_p, c_p]),
    'nerfail_mlp_pack_train': (c_i, [ctypes.POINTER(MlpParams), c_p, c_p, c_p]),
    'nerfail_mlp_bwd_data': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i64, c_p, c_p]),
    'nerfail_mlp_bwd_data2': (c_i, [c_p, c_p, c_i64, c_p, c_p, c_i64, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    'nerfail_mlp_bwd_weights_scratch_bytes': (ctypes.c_size_t, [c_i, c_i, c_i, c_i64, c_i64, c_i]),
    'nerfail_mlp_bwd_weights': (c_i, [c_i, c_i, c_i, c_p, c_p, c_i64, ctypes.POINTER(MlpParams), c_i64, ctypes.POINTER(MlpParams),
                                      c_i, c_p, ctypes.c_size_t, c_p]),
    'nerfail_composite': (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    'nerfail_composite_select': (c_i, [c_i]),
    'nerfail_composite_bwd': (c_i, [c_p, c_p, c_p, c_p, c_i64, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    'nerfail_knn8': (c_i, [c_p, c_i64, c_p, c_i64, c_p, c_p, c_p, c_p]),
    'nerfail_knn8_grid_workspace_bytes': (ctypes.c_size_t, [c_i64]),
    'nerfail_knn8_grid': (c_i, [c_p, c_i64, c_p, c_i64, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    'nerfail_knn8_grid_build': (c_i, [c_p, c_i64, c_p, ctypes.c_size_t, c_p]),
    'nerfail_knn8_grid_stats': (c_i, [c_p]),
    'nerfail_knn8_grid_search': (c_i, [c_p, c_i64, c_i64, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    'nerfail_knn8_grid_search_view': (c_i, [c_p, c_i, c_i, c_i64, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    'nerfail_gauss_weight': (c_i, [c_p, c_i64, c_i64, c_f, c_p, c_p]),
    'nerfail_gauss_compose': (c_i, [c_p, c_p, c_i64, c_p, c_p]),
    'nerfail_gauss_fwd': (c_i, [c_p, c_i64, c_p, c_p, c_i64, c_i64, c_f, c_p, c_p, c_p, c_p]),
    'nerfail_gauss_bwd': (c_i, [c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_f, c_p, c_p]),
    'nerfail_gauss_fwd_views': (c_i, [c_p, c_i64, c_p, c_i, c_i64, c_i, c_f, c_p, c_p, c_p, c_p, c_p, c_p]),
    'nerfail_gauss_bwd_views_rgb': (c_i, [c_p, c_p, c_p, c_p, c_i, c_i64, c_i64, c_p, c_p, c_p]),
    'nerfail_igsm_step_rgb': (c_i, [c_p, c_p, c_p, c_i64, c_f, c_f, c_i, c_p, c_p]),
    'nerfail_gauss_bwd_views_rgb_step': (c_i, [c_p, c_p, c_p, c_p, c_i, c_i64, c_i64, c_p, c_p, c_p, c_p, c_f, c_f, c_i, c_p, c_p]),
    'nerfail_fingerprint': (c_i, [c_p, c_i64, c_i64, c_p, c_p]),
    'nerfail_gauss_csr_workspace_bytes': (ctypes.c_size_t, [c_i64, c_i64, c_i64]),
    'nerfail_gauss_csr_build': (c_i, [c_p, c_i64, c_i64, c_i64, c_p, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    'nerfail_gauss_bwd_scratch_floats': (ctypes.c_size_t, [c_i64, c_i64, c_i]),
    'nerfail_gauss_view_pack_workspace_bytes': (ctypes.c_size_t, [c_i64]),
    'nerfail_gauss_view_chunks': (c_i64, [c_i64]),
    'nerfail_gauss_view_pack': (c_i, [c_p, c_p, c_p, c_i64, c_i64, c_p, c_p, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    'nerfail_gauss_bwd_view_multi': (c_i, [c_p, c_p, c_p, c_i, c_p, c_i64, c_i64, c_f, c_p, c_p, c_p]),
    'nerfail_gauss_bwd_views_scratch_floats': (ctypes.c_size_t, [c_p, c_i, c_i64, c_i]),
    'nerfail_gauss_bwd_csr': (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_f, c_p, c_i, c_p, c_p]),
    'nerfail_gauss_bwd_views': (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i64, c_i64, c_f, c_p, c_p, c_p]),
    'nerfail_gauss_bwd_csr_multi': (c_i, [c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_f, c_p, c_p, c_p]),
    'nerfail_deepfool_norms_scratch_bytes': (ctypes.c_size_t, [c_i, c_i64]),
    'nerfail_deepfool_norms': (c_i, [c_p, c_i, c_i64, c_p, ctypes.c_size_t, c_p, c_p]),
    'nerfail_deepfool_apply': (c_i, [c_p, c_i, c_i64, c_p, c_p, c_f, c_p, c_p, c_p, c_p]),
    'nerfail_igsm_step': (c_i, [c_p, c_p, c_p, c_i64, c_f, c_f, c_i, c_p, c_p]),
    'nerfail_adam_step': (c_i, [c_p, c_i, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_p]),
    'nerfail_mse': (c_i, [c_p, c_p, c_i64, c_p, c_p, c_p]),
    'nerfail_mse_part': (c_i, [c_p, c_p, c_i64, c_i64, c_p, c_p, c_p]),
    'nerfail_abi_revision': (c_i, []),
    'nerfail_attack_logit_stats': (c_i, [c_p, c_p, c_i, c_i, c_i, c_p, c_p]),
    'nerfail_img_sqerr_scratch_bytes': (ctypes.c_size_t, []),
    'nerfail_img_sqerr': (c_i, [c_p, c_p, c_i, c_i64, c_i, c_p, c_p, c_p]),
    'nerfail_img_sqerr_grad_add': (c_i, [c_p, c_p, c_i, c_i64, c_i, c_f, c_p, c_p]),
    'nerfail_attack_epoch_close': (c_i, [c_p, c_p, c_i, c_i, c_p, c_p, c_p]),
    'nerfail_copy_if': (c_i, [c_p, c_p, c_p, c_i64, c_p]),
    'nerfail_export_u8': (c_i, [c_p, c_i64, c_p, c_p]),
    'nerfail_eval_revision': (c_i, []),
    'nerfail_eval_scratch_bytes': (ctypes.c_size_t, []),
    'nerfail_eval_view_metrics': (c_i, [c_p, c_i, c_p, c_i, c_i, c_i64, c_p, c_p, c_p, c_p]),
    'nerfail_eval_logit_stats': (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    'nerfail_eval_fold': (c_i, [c_p, c_p, c_p, c_i, c_i, c_p, c_p]),
    'nerfail_cls_revision': (c_i, []),
    'nerfail_cls_batch': (c_i, [c_p, c_i, c_p, c_i64, c_i64, c_p, c_i, c_p, c_p, c_p]),
    'nerfail_cls_ce': (c_i, [c_p, c_p, c_i, c_i, c_p, c_p, c_p]),
    'nerfail_cnn_sgd_step': (c_i, [c_p, c_p, c_p, c_p, c_i, c_f, c_f, c_i, c_p]),
    'nerfail_cls_epoch_close': (c_i, [c_p, c_p, c_i64, c_i64, c_p, c_i, c_p, c_p, c_p]),
    'nerfail_deepfool_revision': (c_i, []),
    'nerfail_deepfool_gate': (c_i, [c_p, c_i, c_i, c_i, c_f, c_f, c_p, c_p]),
    'nerfail_deepfool_step_scratch_bytes': (ctypes.c_size_t, [c_i, c_i64]),
    'nerfail_deepfool_step': (c_i, [c_p, c_i, c_i64, c_p, c_p, ctypes.c_size_t, c_f, c_p, c_p, c_p, c_p, c_p]),
    'nerfail_scene_revision': (c_i, []),
    'nerfail_knn8_grid_weights_workspace_bytes': (ctypes.c_size_t, [c_i64]),
    'nerfail_knn8_grid_weights_view': (c_i, [c_p, c_i, c_i, c_i64, c_f, c_p, c_p, c_p, ctypes.c_size_t, c_p, ctypes.c_size_t, c_p]),
    'nerfail_knn8_grid_weights': (c_i, [c_p, c_i64, c_i64, c_f, c_p, c_p, c_p, ctypes.c_size_t, c_p, ctypes.c_size_t, c_p]),
    'nerfail_u2d_revision': (c_i, []),
    'nerfail_u2d_fwd': (c_i, [c_p, c_i, c_i64, c_i64, c_p, c_i, c_p, c_i, c_p, c_p, c_p, c_p]),
    'nerfail_u2d_step': (c_i, [c_p, c_i64, c_i64, c_p, c_i, c_p, c_p, c_p, c_f, c_f, c_i, c_p]),
    'nerfail_u2d_sqerr': (c_i, [c_p, c_p, c_i, c_i64, c_i64, c_p, c_i, c_p, c_p, c_p]),
    'nerfail_u2d_epoch_close': (c_i, [c_p, c_p, c_i, c_i, c_p, c_p, c_p]),
    'nerfail_uap2d_revision': (c_i, []),
    'nerfail_uap2d_step_scratch_bytes': (ctypes.c_size_t, [c_i, c_i64]),
    'nerfail_uap2d_step': (c_i, [c_p, c_i, c_i64, c_p, c_p, c_p, ctypes.c_size_t, c_f, c_p, c_p, c_p, c_p, c_p]),
    'nerfail_uap2d_accumulate': (c_i, [c_p, c_p, c_f, c_i64, c_p]),
    'nerfail_poison_revision': (c_i, []),
    'nerfail_export_train_views': (c_i, [c_p, c_i, c_i, c_i64, c_p, c_i64, c_p, c_p, c_p]),
    'nerfail_resize_revision': (c_i, []),
    'nerfail_resize_aa_kmax': (c_i, [c_i, c_i]),
    'nerfail_resize_aa_table': (c_i, [c_i, c_i, c_p, c_p, c_p, c_i, c_p, c_p]),
    'nerfail_resize_tiles': (c_i, [c_i, c_i, c_i, c_i, c_p, c_p]),
    'nerfail_cls_input_resize_fwd': (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    'nerfail_cls_input_resize_bwd': (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    'nerfail_fg_revision': (c_i, []),
    'nerfail_fg_pixel_list_workspace_bytes': (ctypes.c_size_t, [c_i64]),
    'nerfail_fg_pixel_list': (c_i, [c_p, c_i64, c_p, c_p, c_p, ctypes.c_size_t, c_p]),
    'nerfail_ray_gen_list': (c_i, [c_i, c_i, c_p, c_p, c_f, c_f, c_p, c_i64, c_p, c_p]),
    'nerfail_knn8_grid_weights_list': (c_i, [c_p, c_i64, c_p, c_i64, c_i64, c_f, c_p, c_p, c_p, ctypes.c_size_t, c_p, ctypes.c_size_t, c_p]),
    'nerfail_cnn_packed_floats': (ctypes.c_size_t, [c_i]),
    'nerfail_cnn_pack': (c_i, [c_p, c_i, c_p, c_p]),
    'nerfail_cnn_workspace_bytes': (ctypes.c_size_t, [c_i, c_i, c_i, c_i]),
    'nerfail_cnn_mask_bytes': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_cnn_bwd_scratch_bytes': (ctypes.c_size_t, [c_i, c_i, c_i]),
    'nerfail_cnn_fwd': (c_i, [c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    'nerfail_cnn_bwd_data': (c_i, [c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    'nerfail_cnn_bwd_multi_scratch_bytes': (ctypes.c_size_t, [c_i, c_i, c_i, c_i]),
    'nerfail_cnn_bwd_data_multi': (c_i, [c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p]),
    'nerfail_cnn_grad_floats': (ctypes.c_size_t, [c_i]),
    'nerfail_cnn_bwd_weights_scratch_bytes': (ctypes.c_size_t, [c_i, c_i, c_i, c_i]),
    'nerfail_cnn_bwd_weights': (c_i, [c_p, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    'nerfail_cnn_x3_revision': (c_i, []),
    'nerfail_cnn_x3_packed_bytes': (ctypes.c_size_t, [c_i]),
    'nerfail_cnn_pack_x3': (c_i, [c_p, c_i, c_p, c_p]),
    'nerfail_cnn_fwd_x3': (c_i, [c_p, c_p, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p]),
    'nerfail_cnn_bwd_data_x3': (c_i, [c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_p]),
    'nerfail_cnn_bwd_data_multi_x3': (c_i, [c_p, c_p, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p, c_p, c_p]),
}



class ViewIndexStruct(ctypes.Structure):
    """struct nerfail_view_index (include/nerfail_hip.h)"""
    _fields_ = [('packed', c_p), ('w_sorted', c_p), ('chunk_ord', c_p), ('pos', c_p), ('n_entries', c_i64), ('n_rows', c_i64)]


class ViewFwdStruct(ctypes.Structure):
    """struct nerfail_view_fwd (include/nerfail_hip.h)"""
    _fields_ = [('weight_and_index', c_p), ('ori_img', c_p)]


class ResizeAxisStruct(ctypes.Structure):
    """struct nerfail_resize_axis (include/nerfail_hip.h)"""
    _fields_ = [('start', c_p), ('count', c_p), ('w', c_p), ('ostart', c_p), ('ocount', c_p),
                ('n_in', ctypes.c_int32), ('n_out', ctypes.c_int32), ('kmax', ctypes.c_int32), ('reserved', ctypes.c_int32)]


class AdamTensor(ctypes.Structure):
    """struct nerfail_adam_tensor (include/nerfail_hip.h)"""
    _fields_ = [('param', c_p), ('grad', c_p), ('exp_avg', c_p), ('exp_avg_sq', c_p), ('numel', c_i64),
                ('step_size', c_f), ('bias_correction2_sqrt', c_f)]


_lib = None


def load():
    """Load the library once; raise (never fall back) when it is absent or has the wrong ABI."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError('nerfail_amd: %s is missing - build it with `python -m nerfail_amd.build` '
                           '(hipcc, gfx950). There is no CPU fallback.' % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = the .so is stale: rebuild
        fn.restype = res
        fn.argtypes = args
    v = lib.nerfail_abi_version()
    if v != ABI_VERSION or lib.nerfail_abi_revision() != ABI_REVISION:
        raise RuntimeError('nerfail_amd: ABI version %d revision %d, expected %d / %d - rebuild the library'
                           % (v, lib.nerfail_abi_revision(), ABI_VERSION, ABI_REVISION))
    if lib.nerfail_eval_revision() != EVAL_REVISION:
        raise RuntimeError('nerfail_amd: attack-evaluation revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_eval_revision(), EVAL_REVISION))
    if lib.nerfail_cls_revision() != CLS_REVISION:
        raise RuntimeError('nerfail_amd: victim-training revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_cls_revision(), CLS_REVISION))
    if lib.nerfail_deepfool_revision() != DEEPFOOL_REVISION:
        raise RuntimeError('nerfail_amd: DeepFool revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_deepfool_revision(), DEEPFOOL_REVISION))
    if lib.nerfail_scene_revision() != SCENE_REVISION:
        raise RuntimeError('nerfail_amd: scene-maps revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_scene_revision(), SCENE_REVISION))
    if lib.nerfail_u2d_revision() != U2D_REVISION:
        raise RuntimeError('nerfail_amd: 2-D baseline revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_u2d_revision(), U2D_REVISION))
    if lib.nerfail_uap2d_revision() != UAP2D_REVISION:
        raise RuntimeError('nerfail_amd: 2-D universal baseline revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_uap2d_revision(), UAP2D_REVISION))
    if lib.nerfail_poison_revision() != POISON_REVISION:
        raise RuntimeError('nerfail_amd: poisoned-retrain revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_poison_revision(), POISON_REVISION))
    if lib.nerfail_resize_revision() != RESIZE_REVISION:
        raise RuntimeError('nerfail_amd: classifier-input resize revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_resize_revision(), RESIZE_REVISION))
    if lib.nerfail_fg_revision() != FG_REVISION:
        raise RuntimeError('nerfail_amd: foreground scene-maps revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_fg_revision(), FG_REVISION))
    if lib.nerfail_cnn_x3_revision() != CNN_X3_REVISION:
        raise RuntimeError('nerfail_amd: bf16x3 victim revision %d, expected %d - rebuild the library'
                           % (lib.nerfail_cnn_x3_revision(), CNN_X3_REVISION))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().nerfail_last_error().decode('utf-8', 'replace')
        raise NerfailError('libnerfail_hip error %d: %s' % (rc, msg))


def dev(t, name='tensor'):
    """Pointer of a dense float32 HIP tensor; anything else is an error (no silent copies / fallbacks)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s is on %s: nerfail_amd runs on the MI355X only (no CPU path)' % (name, t.device))
    if t.dtype not in (torch.float32, torch.int32, torch.uint8, torch.int64):
        raise TypeError('%s must be float32 (got %s)' % (name, t.dtype))
    if not t.is_contiguous():
        raise ValueError('%s must be contiguous' % name)
    return c_p(t.data_ptr())


def host_floats(values):
    arr = (c_f * len(values))(*[float(v) for v in values])
    return arr


def stream():
    return c_p(torch.cuda.current_stream().cuda_stream)


def f32c(t, device=None):
    """Detached contiguous float32 view/copy of t on `device` (the reference's .float() / .to(device))."""
    t = t.detach()
    if device is not None and t.device != device:
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def device_name():
    buf = ctypes.create_string_buffer(256)
    check(load().nerfail_device_name(buf, 256))
    return buf.value.decode()
