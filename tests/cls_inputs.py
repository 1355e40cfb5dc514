"""Seeded inputs of the victim-training tests (tests/test_cls_train_ref.py, tests/test_hip_cls_*.py,
tests/golden/make_golden_cls_train.py): BGRA uint8 views as cv2 reads the classification set's PNGs, regenerated from seeds on
both sides so that fixture g26 stores seeds, orders and results instead of 19 MB of images. Weights come from
cnn_inputs.state_dict."""
import numpy as np

H = W = 766                     # the smallest input MyCNN accepts (a 4 x 4 seventh stage)
NUM_CLASSES = 8
TRAIN_LABELS = (1, 6, 1, 3, 6)  # 5 train views, 3 val views at batch 2: each phase drops one view
VAL_LABELS = (6, 1, 3)


def view(seed, label, H=H, W=W):
    """uint8 [H,W,4] BGRA: an ellipse (alpha 255) whose colours depend on the class, on a transparent background whose rgb
    bytes are garbage - the white background of MD:98-105 must come from alpha alone."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = H * rs.uniform(0.45, 0.55), W * rs.uniform(0.45, 0.55)
    ry, rx = H * rs.uniform(0.25, 0.35), W * rs.uniform(0.25, 0.35)
    inside = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
    img = rs.randint(0, 255, size=(H, W, 4)).astype(np.uint8)           # garbage, never 255 everywhere
    img[..., 3] = 0
    for c in range(3):
        level = 40 + 25 * ((label * (c + 2)) % 8)
        period = 12.0 + 9.0 * ((label + 3 * c) % 5)
        tex = level + 30 * np.sin(x / period + c) * np.cos(y / period) + rs.normal(scale=6.0, size=(H, W))
        img[..., c][inside] = np.clip(np.round(tex), 0, 255).astype(np.uint8)[inside]
    img[..., 3][inside] = 255
    return img


def views(seed, labels, H=H, W=W):
    """(uint8 [N,H,W,4], int32 [N]) for a list of labels; view k is drawn from seed + k."""
    return np.stack([view(seed + k, lb, H, W) for k, lb in enumerate(labels)]), np.asarray(labels, np.int32)


def white_nchw(store):
    """float32 [N,3,H,W]: MD:93-105 of a uint8 [N,H,W,4|3] store (rgb where alpha > 0, else 255; channel order as stored)."""
    a = np.asarray(store).astype(np.float32)
    if a.shape[-1] == 4:
        a = np.where(a[..., 3:4] > 0, a[..., :3], np.float32(255))
    return np.ascontiguousarray(np.moveaxis(a, -1, 1))
