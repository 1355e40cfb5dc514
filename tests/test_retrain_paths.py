"""CPU: the host side of the retrain stage. attack_output_dir returns the literal folder names of the reference's
transfer_files.get_test_dir_after_nerf_attack (typed here from its string expressions), and they are the folders test_for_inception
asks for; the mirror's load_blender_data(train_dir=...) and training_images reproduce what the REFERENCE returned for two scenes of
attacked train views (fixture g30, tests/golden/make_golden_retrain.py) - the exhaustive (colour, alpha) image and the 3-channel
PNGs g18 does not cover - and tests/poison_ref.py, the numpy chain the GPU tests compare the hand-off kernel against, is pinned to
the same fixture."""
import inspect
import os

import numpy as np
import pytest

import poison_ref as PR

STEPS = {0: 'attack', 1: 'nerf', 2: 'defense', 3: 'nerf_defense'}
KW = dict(scene_name='mic', model_name='inception', now_class_idx=6, attack_epochs=50, print_a=4, print_e=16, target_class_idx=5,
          base_mask_image_number=7, m1=8, m2=100)
TAILS = {'NeRFail': 'NeRFail_7P_50_to_5_e_16_m_8_100', 'NeRFail_S': 'NeRFail_S_7P_50_to_5_e_16_a_4', 'IGSM_2D': 'IGSM_2D_50_to_5_e_16_a_4',
         'Universal_2D': 'Universal_2D_50_to_5_e_16_m_8_100', 'No_attack': 'no_attack'}


@pytest.mark.parametrize('step', [0, 1, 2, 3])
@pytest.mark.parametrize('method', ['NeRFail', 'NeRFail_S', 'IGSM_2D', 'Universal_2D', 'No_attack', 'IGSM', 'Universal'])
def test_attack_output_dir_returns_the_reference_strings(method, step):
    from nerfail_amd.retrain import attack_output_dir
    got = attack_output_dir(method_name=method, step=step, **KW)
    if method == 'No_attack' and step == 0:
        assert got is None
        return
    tail = TAILS[{'IGSM': 'NeRFail_S', 'Universal': 'NeRFail'}.get(method, method)]
    assert got == './output/inception/' + STEPS[step] + '/mic/' + tail


def test_attack_output_dir_defaults_and_unknown_methods():
    from nerfail_amd.retrain import attack_output_dir
    assert attack_output_dir() == './output/vgg16/attack/lego/NeRFail_3P_100_to_n_e_32_m_0_0'
    assert attack_output_dir(step=1, method_name='IGSM') == './output/vgg16/nerf/lego/NeRFail_S_3P_100_to_n_e_32_a_2'
    assert attack_output_dir(method_name=None) is None and attack_output_dir(method_name='something else') is None
    sig = [(p.name, p.default) for p in inspect.signature(attack_output_dir).parameters.values()]
    assert sig == [('scene_name', 'lego'), ('model_name', 'vgg16'), ('now_class_idx', 10), ('attack_epochs', 100), ('print_a', 2),
                   ('print_e', 32), ('target_class_idx', 'n'), ('base_mask_image_number', 3), ('m1', 0), ('m2', 0),
                   ('method_name', 'NeRFail'), ('step', 0), ('something_need_log', None)]


class _Captured(Exception):
    pass


@pytest.mark.parametrize('step', [0, 1, 2, 3])
@pytest.mark.parametrize('method', ['NeRFail', 'NeRFail_S', 'IGSM_2D', 'Universal_2D', 'No_attack', 'IGSM', 'Universal'])
def test_attack_output_dir_is_the_folder_test_for_inception_reads(monkeypatch, method, step):
    """model_test.test_for_inception builds its folder inline (MT:104-128); attack_output_dir states the rows once more. The two are
    held together here: test_for_inception is run up to the point where it lists its folder (no GPU, no weights: the device, the
    model and the checkpoint are stood in for), and the folder it asks for must be attack_output_dir's plus the set name."""
    import torch
    from nerfail_amd import model_test as MT
    from nerfail_amd.retrain import attack_output_dir
    asked = []

    def listing(directory):
        asked.append(directory)
        raise _Captured()
    monkeypatch.setattr(MT, '_cuda', lambda: torch.device('cpu'))
    monkeypatch.setattr(MT, '_build_model', lambda name, n: torch.nn.Identity())
    monkeypatch.setattr(MT.torch, 'load', lambda *a, **k: {})
    monkeypatch.setattr(MT, '_indexed_files', listing)
    with pytest.raises(_Captured):
        MT.test_for_inception(setname='val', method_name=method, step=step, **KW)
    mine = attack_output_dir(method_name=method, step=step, **KW)
    if method == 'No_attack' and step == 0:
        assert mine is None and asked == ['./data/nerf_synthetic/mic/val']
    else:
        assert asked == [mine + '/val']


def _rebuild(g, tag, root, mode):
    from PIL import Image
    for split in ('train', 'val', 'test'):
        os.makedirs(os.path.join(root, split))
        open(os.path.join(root, 'transforms_%s.json' % split), 'wb').write(g['%s_json_%s' % (tag, split)].tobytes())
        for i, img in enumerate(g['%s_raw_%s' % (tag, split)]):
            Image.fromarray(img, 'RGBA').save(os.path.join(root, split, 'r_%d.png' % i))
    adv = root + '_adv'
    os.makedirs(adv)
    for i, img in enumerate(g[tag + '_raw_adv']):
        Image.fromarray(img, mode).save(os.path.join(adv, 'r_%d.png' % i))
    return adv


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (a.dtype, b.dtype, a.shape, b.shape)


@pytest.fixture(scope='module')
def g30():
    return np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g30_train_dir.npz'))


@pytest.mark.parametrize('tag, mode, channels', [('full', 'RGBA', 4), ('rgb', 'RGB', 3)])
def test_mirror_reproduces_the_reference_on_attacked_train_views(tmp_path, g30, tag, mode, channels):
    from nerfail_amd.load_blender import load_blender_data, training_images
    g = g30
    root = str(tmp_path / tag)
    adv = _rebuild(g, tag, root, mode)
    (t_imgs, rest), poses, _, hwf, i_split = load_blender_data(root, train_dir=adv)
    _same(t_imgs, g[tag + '_train_imgs']); _same(rest, g[tag + '_rest_imgs']); _same(poses, g[tag + '_poses'])
    _same(np.array(hwf, np.float64), g[tag + '_hwf']); _same(np.concatenate(i_split), g[tag + '_i_split'])
    assert [len(s) for s in i_split] == list(g[tag + '_i_split_sizes']) and t_imgs.shape[-1] == channels
    imgs = training_images([t_imgs, rest], white_bkgd=True, train_dir=adv)
    n = t_imgs.shape[0]
    assert imgs.dtype == np.float32 and imgs.shape == (n + rest.shape[0],) + t_imgs.shape[1:3] + (3,)
    # RN:587-588 on the reference's own arrays, operation by operation in float32
    t = g[tag + '_train_imgs']
    if channels == 4:
        want = (t[..., :3] * t[..., 3:]).astype(np.float32) + (np.float32(1.) - t[..., 3:])
    else:
        want = t
    _same(imgs[:n], want)
    # ... and the numpy chain of the GPU tests, from the raw bytes in cv2's order, lands on the same bits
    raw = g[tag + '_raw_adv']
    cv2_order = raw[..., [2, 1, 0, 3]] if channels == 4 else raw[..., ::-1]
    _same(PR.targets_of_u8(np.ascontiguousarray(cv2_order)), want)


def test_exhaustive_image_covers_every_pair(g30):
    """Every (colour byte, alpha byte) pair occurs in every colour channel of the full scene's attacked view, and LB:65 is the
    float64 divide: q / 255 in double, rounded once to float32."""
    raw = g30['full_raw_adv'][0]
    for c in range(3):
        assert len(set(zip(raw[..., c].reshape(-1).tolist(), raw[..., 3].reshape(-1).tolist()))) == 65536
    _same(g30['full_train_imgs'][0], (raw.astype(np.float64) / 255.0).astype(np.float32))
    # the shortcuts differ from the reference arithmetic: a test on this image tells them apart
    q = np.arange(256)
    assert np.count_nonzero((q.astype(np.float32) * np.float32(1. / 255.)) != (q / 255.).astype(np.float32)) > 0


def test_unsupported_targets_raise_clearly():
    from nerfail_amd.retrain import PoisonedTrainSet
    with pytest.raises(NotImplementedError, match='white_bkgd=False'):
        PoisonedTrainSet([0, 1], 4, 4, 4, white_bkgd=False)
    with pytest.raises(NotImplementedError, match='half_res'):
        PoisonedTrainSet([0, 1], 4, 4, 4, half_res=True)
    with pytest.raises(ValueError, match='channels'):
        PoisonedTrainSet([0, 1], 4, 4, 5)
    with pytest.raises(ValueError, match='each once'):
        PoisonedTrainSet([0, 0], 4, 4, 4)
