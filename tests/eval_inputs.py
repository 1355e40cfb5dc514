"""Seeded inputs of the attack-evaluation tests (fixture g25, tests/golden/make_golden_eval.py; tests/test_eval_ref.py;
tests/test_hip_eval.py): pairs of (original, attacked) views as cv2.imread(..., IMREAD_UNCHANGED) returns RGBA PNGs - uint8
[S,S,4] in cv2's channel order - regenerated from seeds on both sides, so that the fixture stores seeds and results only."""
import numpy as np

import cnn_inputs as CI


def view_pairs(image_seeds, pert_seed, side, bound, identical, hidden):
    """(originals, attacked), each a list of uint8 [side,side,4] images.

    Original i: cnn_inputs.cold_tail_image(image_seeds[i]) - its textured object opaque, the white background transparent with
    rgb 0 under it, as the nerf_synthetic renders store it. Attacked i: the original plus an integer perturbation in
    [-bound, bound] on the opaque pixels, clipped to [0, 255], alpha untouched. View `identical` is left as its original (the
    rmse == 0 branch of get_psnr); in view `hidden` the perturbation also writes the rgb of the transparent pixels and leaves
    their alpha at 0: the file differs there, the image on white does not."""
    rs = np.random.RandomState(pert_seed)
    originals, attacked = [], []
    for i, seed in enumerate(image_seeds):
        img = CI.cold_tail_image(int(seed), side, side)[0]                    # [3,S,S], 255 outside the object
        opaque = (img != 255.0).any(0)
        ori = np.zeros((side, side, 4), np.uint8)
        ori[..., :3] = np.where(opaque[..., None], img.transpose(1, 2, 0), 0.0).astype(np.uint8)
        ori[..., 3] = np.where(opaque, 255, 0)
        pert = rs.randint(-bound, bound + 1, size=(side, side, 3))
        att = ori.copy()
        if i != identical:
            where = np.ones_like(opaque) if i == hidden else opaque
            att[..., :3] = np.where(where[..., None], np.clip(ori[..., :3].astype(np.int64) + pert, 0, 255), ori[..., :3]).astype(np.uint8)
        originals.append(ori)
        attacked.append(att)
    return originals, attacked
