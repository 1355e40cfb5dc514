"""The file path of the retrain hand-off, in numpy: what the reference makes of an attack's float export on its way to the NeRF's
training targets. cv2.imwrite's conversion (attack_loop_ref.export_u8 = np.rint(np.clip(x, 0, 255))), the PNG (lossless), imageio's
decode (RGBA / RGB order), LB:65's float64 divide with the float32 cast, and RN:587-588 through the mirror's training_images.
tests/test_retrain_paths.py pins this chain to fixture g30; the GPU tests compare nerfail_export_train_views against it bitwise."""
import numpy as np


def to_file_order(adv_u8):
    """uint8 [...,4] BGRA or [...,3] BGR (cv2's order, what the export holds) -> the PNG's own RGBA / RGB order."""
    return adv_u8[..., [2, 1, 0, 3]] if adv_u8.shape[-1] == 4 else adv_u8[..., ::-1]


def targets_of_u8(adv_u8):
    """float32 [n,H,W,3] RGB: load_blender_data(train_dir=...)'s train images of the PNGs holding adv_u8 [n,H,W,C] (cv2 order),
    through training_images(white_bkgd=True)."""
    from nerfail_amd.load_blender import training_images
    imgs = (np.array(to_file_order(adv_u8)) / 255.).astype(np.float32)            # LB:65
    return training_images([imgs, imgs[:0]], True, train_dir='adv')             # RN:573-596; no val / test views behind them


def targets_of_export(x):
    """(adv_u8, targets) of a float export x [n,H,W,C]."""
    from attack_loop_ref import export_u8
    q = export_u8(x)                                                            # np.rint(np.clip(x, 0, 255)), NaN -> 0
    return q, targets_of_u8(q)
