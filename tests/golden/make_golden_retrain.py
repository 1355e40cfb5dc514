#!/usr/bin/env python3
"""Fixture g30: the reference's load_blender_data(train_dir=...) (load_blender.py:37-110 = LB) RUN on two toy scenes whose
attacked train views are what an attack's export epoch writes.

Run in the build container only (it imports the reference through make_golden.py, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_retrain.py

As for g18, `imageio` is absent: its imread is backed by PIL for this call (PNG decoding is lossless, so every decoder returns
the same uint8 array). Only DATA is written.

  full_*   a 256 x 256 scene with ONE attacked train view, an RGBA PNG whose red channel is the row, whose green and blue channels
           are two other bijections of the row (255 - row, (7 row + 13) mod 256: a swapped channel cannot hide) and whose alpha is
           the column: every (colour byte, alpha byte) pair occurs in every channel. val and test hold one view of 32 x 32 blocks each.
  rgb_*    write_toy_scene's 12 x 12 scene (seed 30) whose three attacked train views are 3-channel PNGs (what IGSM-2D and UAP-2D
           export): LB:65 keeps three channels, RN:587 then takes them as they are. g18 does not cover this case.

Stored per scene: the JSON texts, the raw uint8 images of every file (`raw_*`: RGBA or RGB, the PNG's own channel order) and the
arrays the reference returned: `train_imgs` (float32 [n,H,W,C]), `rest_imgs` (val + test), poses, hwf, i_split."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (stubs the I/O-only packages and puts the reference on sys.path)
import synth  # noqa: E402  (tests/)
from test_load_blender import write_toy_scene  # noqa: E402  (tests/)


def exhaustive_rgba():
    row = np.arange(256, dtype=np.int64)[:, None] * np.ones((1, 256), np.int64)
    col = np.arange(256, dtype=np.int64)[None, :] * np.ones((256, 1), np.int64)
    return np.stack([row, 255 - row, (7 * row + 13) % 256, col], -1).astype(np.uint8)


def smooth_rgba(k):
    y, x = np.mgrid[0:256, 0:256] // 32                                   # 32 x 32 blocks of one colour: the fixture stays small
    return np.stack([(31 * x + k) % 256, (29 * y + 2 * k) % 256, (17 * (x + y)) % 256, np.where((x + y + k) % 2 == 0, 255, 0)], -1).astype(np.uint8)


def write_full_scene(root):
    from PIL import Image
    raw = {'train': exhaustive_rgba()[None] // 2 + 17, 'val': smooth_rgba(1)[None], 'test': smooth_rgba(2)[None]}   # (train: never read)
    for split, imgs in raw.items():
        os.makedirs(os.path.join(root, split))
        frames = []
        for i, img in enumerate(imgs):
            Image.fromarray(img, 'RGBA').save(os.path.join(root, split, 'r_%d.png' % i))
            pose = synth.pose_spherical(40. * i + {'train': 0., 'val': 13., 'test': 27.}[split], -30., 4.)
            frames.append({'file_path': './%s/r_%d' % (split, i), 'rotation': 0.1, 'transform_matrix': pose.tolist()})
        json.dump({'camera_angle_x': synth.LEGO_CAMERA_ANGLE_X, 'frames': frames}, open(os.path.join(root, 'transforms_%s.json' % split), 'w'))
    return raw


def record(out, tag, root, raw, adv_raw, adv_mode, LB):
    from PIL import Image
    for split in ('train', 'val', 'test'):
        out['%s_raw_%s' % (tag, split)] = raw[split]
        out['%s_json_%s' % (tag, split)] = np.frombuffer(open(os.path.join(root, 'transforms_%s.json' % split), 'rb').read(), np.uint8)
    adv = root + '_adv'
    os.makedirs(adv)
    for i, img in enumerate(adv_raw):
        Image.fromarray(img, adv_mode).save(os.path.join(adv, 'r_%d.png' % i))
    out[tag + '_raw_adv'] = adv_raw
    (t_imgs, rest), poses, _, hwf, i_split = LB.load_blender_data(root, train_dir=adv)
    assert t_imgs.dtype == np.float32 and t_imgs.shape == adv_raw.shape, (t_imgs.dtype, t_imgs.shape)
    out.update({tag + '_train_imgs': t_imgs, tag + '_rest_imgs': rest, tag + '_poses': poses, tag + '_hwf': np.array(hwf, np.float64),
                tag + '_i_split': np.concatenate(i_split), tag + '_i_split_sizes': np.array([len(s) for s in i_split])})


def g30():
    from PIL import Image
    sys.modules['imageio'].imread = lambda path: np.asarray(Image.open(path))
    import load_blender as LB  # noqa: E402  (reference)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'full')
        raw = write_full_scene(root)
        record(out, 'full', root, raw, exhaustive_rgba()[None], 'RGBA', LB)
        root = os.path.join(tmp, 'rgb')
        raw = write_toy_scene(root, H=12, W=12, n=(3, 2, 2), seed=30)
        adv_rgb = np.random.RandomState(31).randint(0, 256, size=(3, 12, 12, 3)).astype(np.uint8)
        adv_rgb[0, 0, :6] = np.array([0, 1, 127, 128, 254, 255], np.uint8)[:, None]
        record(out, 'rgb', root, raw, adv_rgb, 'RGB', LB)
    MG.save('g30_train_dir', **out)


if __name__ == '__main__':
    g30()
