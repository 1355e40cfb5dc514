"""What the data-parallel training tests share (tests/test_hip_train_shard.py in one process, tests/mgpu/train_rank.py and
train_nccl1.py as ranks): the toy scene of 4 views of 8 x 8, the args of a short train() run, one shard of fixture g7's
training step written into a gradient arena, and the bound tests/test_hip_train.py::test_training_step_gradients holds that
step to."""
import os
import types

import numpy as np
import torch

import synth
from hiputil import T, hip_nerf

NEAR, FAR = 2., 6.
H = W = 8
N_VIEWS = 4
STEPS = 3
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
G7_TAGS = (('small', 4, 64), ('full', 8, 256))


def scene(seed=0):
    rs = np.random.RandomState(seed)
    images = rs.uniform(size=(N_VIEWS, H, W, 3)).astype(np.float32)
    poses = np.stack([synth.pose_spherical(40. * i, -30., 4.) for i in range(N_VIEWS)])
    focal = .5 * W / np.tan(.5 * synth.LEGO_CAMERA_ANGLE_X)
    return images, poses, [H, W, focal], np.array([[focal, 0, 0.5 * W], [0, focal, 0.5 * H], [0, 0, 1]])


def create_args(basedir, **kw):
    """args of RN.create_nerf + train.train: D4 W64 coarse + fine, 16 + 16 samples, deterministic draws (perturb 0, no noise)."""
    a = dict(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=16, N_samples=16, netdepth=4, netwidth=64,
             netdepth_fine=4, netwidth_fine=64, netchunk=65536, lrate=5e-4, basedir=basedir, expname='toy', ft_path=None,
             no_reload=False, perturb=0., white_bkgd=True, raw_noise_std=0., dataset_type='blender', no_ndc=False, lindisp=False,
             N_rand=32, no_batching=True, lrate_decay=250, i_print=1, i_weights=10 ** 9, precrop_iters=0, precrop_frac=.5,
             chunk=1024 * 32)
    a.update(kw)
    return types.SimpleNamespace(**a)


def nudge_density(kw):
    with torch.no_grad():                  # (a fresh NeRF has no density: the nudge the other toy training tests use)
        for net in (kw['network_fn'], kw['network_fine']):
            net.alpha_linear.bias += 0.5


def flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors]).cpu().numpy()


def g7():
    return dict(np.load(os.path.join(GOLDEN, 'g7_train_grads.npz')))


def g7_nets(D, W_):
    return hip_nerf(D, W_, 31, requires_grad=True)[1], hip_nerf(D, W_, 32, requires_grad=True)[1]


def g7_shard_step(g, tag, coarse, fine, lo, hi, arena=None):
    """Rows [lo, hi) of fixture g7's step `tag` - its rays, targets and draws - with the loss divided by the WHOLE step's
    count, gradients into `arena` (None: wherever autograd puts them). Returns (loss share, fine image loss share)."""
    from nerfail_amd import run_nerf as RN
    R = g[tag + '_rays'].shape[0]
    for p in list(coarse.parameters()) + list(fine.parameters()):
        p.grad = None
    r = RN.render_rays(T(g[tag + '_rays'][lo:hi]), coarse, None, 64, retraw=True, N_importance=128, network_fine=fine, white_bkgd=True,
                       perturb=1., t_rand=T(g[tag + '_t_rand'][lo:hi]), u=T(g[tag + '_u'][lo:hi]), grad_arena=arena)
    target = T(g[tag + '_target'][lo:hi])
    n_total = None if (lo, hi) == (0, R) and arena is None else 3 * R
    img = RN.img2mse(r['rgb_map'], target, n_total)
    loss = img + RN.img2mse(r['rgb0'], target, n_total)
    loss.backward()
    if arena is not None:
        arena.put_tail(loss, img)
    return loss.detach(), img.detach()


def arena_named(arena, buf):
    """{(net index, parameter name): gradient array} of an arena image `buf` (numpy, P + 2 floats)."""
    from nerfail_amd._train import ordered_params
    out = {}
    for k, net in enumerate(arena.nets):
        names = {id(p): n for n, p in net.named_parameters()}
        for p, off in zip(ordered_params(net), arena.offsets[k]):
            out[(k, names[id(p)])] = buf[off:off + p.numel()].reshape(tuple(p.shape))
    return out


def g7_worst_ratio(g, tag, grads):
    """max over all parameters of (L2 error against the reference's fp32 gradient) / (2 x the reference's own fp32-vs-fp64 L2
    distance + 2e-6): test_training_step_gradients' measure. `grads`: {(0 | 1, name): array}."""
    worst, lines = 0., []
    for (k, name), got in sorted(grads.items()):
        nm = ('coarse', 'fine')[k]
        ref = g['%s_%s_grad_%s' % (tag, nm, name)].astype(np.float64)
        e = float(np.linalg.norm(got.astype(np.float64) - ref) / max(np.linalg.norm(ref), 1e-30))
        bound = 2 * float(g['%s_%s_referr_%s' % (tag, nm, name)]) + 2e-6
        worst = max(worst, e / bound)
        lines.append('%-6s %-26s err %.2e  bound %.2e' % (nm, name, e, bound))
    return worst, lines
