"""How often the Python layer packs a weight image, counted at the C ABI: the cache rules of nerfail_amd/_images.py on the
real networks. A slip here costs a launch per call or per optimizer step and changes no result, so no parity test sees it.

`nerfail_amd._lib._lib` is replaced, for one test, by a proxy around the loaded library that counts the calls of every
symbol beginning `nerfail_mlp_pack` (the packers and their size queries) and forwards everything else. Written against the
public names only (run_network, NeRF.forward, _mlp_rays, x3_image, mlp_fwd_train, mlp_backward) and first run on the
commit before the caches were unified: every count below is that commit's."""
import collections

import pytest
import torch

import synth
from hiputil import T, hip_nerf

SMALL, SHIPPED = (2, 64), (8, 256)          # (D, W) with skips=[4]: (2, 64, -1) has no bf16x3 image, (8, 256, 4) has both
R, N = 2, 32                                # M = 64 samples per forward
PACKERS = ('nerfail_mlp_pack', 'nerfail_mlp_pack_T', 'nerfail_mlp_pack_train', 'nerfail_mlp_pack_x3', 'nerfail_mlp_pack_x3f',
           'nerfail_mlp_pack_f16', 'nerfail_mlp_pack_f16_T')


class CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('nerfail_mlp_pack'):
            return fn

        def counted(*args):
            self.calls[name] += 1
            return fn(*args)
        return counted

    def packs(self):
        return {k: self.calls[k] for k in PACKERS if self.calls[k]}


@pytest.fixture
def lib(monkeypatch):
    from nerfail_amd import _lib
    proxy = CountingLib(_lib.load())
    monkeypatch.setattr(_lib, '_lib', proxy)
    return proxy


def inputs():
    rays = T(synth.ray_batch(R, seed=5))
    z = torch.linspace(2., 6., N, device=rays.device).expand(R, N).contiguous()
    pts = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).contiguous()
    return rays, z, pts, rays[:, 8:11].contiguous()


def four_inferences(net):
    """Two run_network calls on points, one NeRF.forward on an embedded batch, one _mlp_rays."""
    from nerfail_amd import run_nerf as RN
    rays, z, pts, vd = inputs()
    e, ed = RN.Embedder(10), RN.Embedder(4)
    with torch.no_grad():
        RN.run_network(pts, vd, net, e, ed)
        RN.run_network(pts, vd, net, e, ed)
        net(torch.cat([e(pts.reshape(-1, 3)), ed(vd[:, None].expand(R, N, 3).reshape(-1, 3))], -1))
        RN._mlp_rays(net, rays, z)


@pytest.mark.gpu
@pytest.mark.parametrize('D,W', [SHIPPED, SMALL], ids=['D8_W256_skip4', 'D2_W64_noskip'])
def test_inference_packs_once_per_weight_version(D, W, lib):
    _, net = hip_nerf(D, W, seed=3)
    want = {'nerfail_mlp_pack': 1, 'nerfail_mlp_pack_x3f': 1} if (D, W) == SHIPPED else {'nerfail_mlp_pack': 1}
    four_inferences(net)
    print('packs after four inferences:', dict(lib.calls))
    assert lib.packs() == want
    # a shape without a bf16x3 image caches its None: one size query per image and weight version, not one per call
    assert lib.calls['nerfail_mlp_packed_x3f_bytes'] == 1
    assert lib.calls['nerfail_mlp_packed_x3_bytes'] == (0 if (D, W) == SHIPPED else 1)
    with torch.no_grad():
        net.alpha_linear.bias.add_(0.)                         # one in-place write: every image once more
    four_inferences(net)
    print('packs after an in-place write and four more:', dict(lib.calls))
    assert lib.packs() == {k: 2 * v for k, v in want.items()}
    assert lib.calls['nerfail_mlp_packed_x3f_bytes'] == 2


@pytest.mark.gpu
def test_non_finite_fold_falls_back_and_is_cached(lib):
    """feature_linear and views_linears[0] finite, their product not: the folded image is refused once per weight version
    (one host synchronisation) and the unfolded one is split once."""
    _, net = hip_nerf(*SHIPPED, seed=3)
    with torch.no_grad():
        net.feature_linear.weight.mul_(1e25)
        net.views_linears[0].weight.mul_(1e25)
    assert bool(torch.isfinite(net.feature_linear.weight).all() and torch.isfinite(net.views_linears[0].weight).all())
    four_inferences(net)
    four_inferences(net)
    print('packs with a non-finite composed block:', dict(lib.calls))
    assert lib.packs() == {'nerfail_mlp_pack': 1, 'nerfail_mlp_pack_x3f': 1, 'nerfail_mlp_pack_x3': 1}
    fold, img = net.x3_image()
    assert fold is False and img is not None
    assert lib.packs() == {'nerfail_mlp_pack': 1, 'nerfail_mlp_pack_x3f': 1, 'nerfail_mlp_pack_x3': 1}


def train_step(net, opt):
    from nerfail_amd import _train
    _, _, pts, vd = inputs()
    raw, acts = _train.mlp_fwd_train(net, pts, vd)
    grads = _train._zero_grads(net)
    _train.mlp_backward(net, torch.ones_like(raw), acts, grads, accumulate=True)
    for p, g in zip(_train.ordered_params(net), grads):
        p.grad = g
    opt.step()


# precision -> packer counts after one forward + backward, the parent commit's (printed by this test there): the f32 step
# packs both images in one launch; the split-precision step skips the joint pack, packs the f32 image alone (the kernels
# read their biases and heads from it) and the two fp16 images, each once
TRAIN_PACKS = {'f32': {'nerfail_mlp_pack_train': 1},
               'f16x3': {'nerfail_mlp_pack': 1, 'nerfail_mlp_pack_f16': 1, 'nerfail_mlp_pack_f16_T': 1}}


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
def test_training_step_packs_once_per_weight_version(precision, lib):
    from nerfail_amd.optim import Adam
    _, net = hip_nerf(*SMALL, seed=4, requires_grad=True, precision=precision)
    opt = Adam(list(net.parameters()), lr=5e-4, betas=(0.9, 0.999))
    want = TRAIN_PACKS[precision]
    train_step(net, opt)
    print('packs after one %s training step:' % precision, dict(lib.calls))
    assert lib.packs() == want
    train_step(net, opt)                                       # the optimizer step moved the weights: each once more
    print('packs after two %s training steps:' % precision, dict(lib.calls))
    assert lib.packs() == {k: 2 * v for k, v in want.items()}
