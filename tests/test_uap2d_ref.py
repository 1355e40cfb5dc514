"""CPU: tests/uap2d_ref.py - the numpy restatement of the UAP-2D loop and of the three kernels behind it - and the package's
deepfool.deepfool_2d (stock torch, on the CPU, through GaussNet.universal_2D_net) against fixture g29, the reference's own run
(tests/golden/make_golden_uap2d.py): every discrete decision equal - the epochs the loop went through, the skipped visits,
iter_k, the class chosen in every iteration, the counts, the taken flags -, losses within twice the fixture's own
float32-to-float64 spread, tables, best tensor and exported images within uap2d_ref.g29_bound."""
import numpy as np
import pytest
import torch

import igsm2d_ref as IR
import uap2d_ref as UR

TAGS = ('untargeted', 'targeted')


@pytest.fixture(scope='module')
def g(golden):
    return golden('g29_uap2d')


@pytest.fixture(scope='module')
def images(g):
    return UR.g29_images(int(g['seed']), g['tints'], g['extra_tints'])


def test_the_fixture_meets_its_own_conditions(g):
    """What the generator asserted, visible from the stored data: both kinds of run, a skip, a completed and a capped call, a
    strict tie, a jump to the export epoch, best != last, elements on +-epsilon."""
    assert [str(t) for t in g['tags']] == list(TAGS) and g['targeted'].tolist() == [0, 1]
    cap, last = int(g['shape'][5]), int(g['shape'][4]) - 1
    skipped = completed = capped = tie = jumped = differ = on_eps = False
    for i, tag in enumerate(TAGS):
        v, p = g[tag + '_visits'], g[tag + '_passes']
        att = v[p[:, 0] < last]
        skipped |= bool((att[..., 1] == 1).any())
        completed |= bool(((att[..., 1] == 0) & (att[..., 2] < cap)).any())
        capped |= bool((att[..., 2] == cap).any())
        best = 0. if g['targeted'][i] else 10000.
        for acc, taken in p[:, [6, 7]]:
            tie |= acc == best and not taken
            best = acc if taken else best
        jumped |= bool(((p[:, 1] == last) & (p[:, 0] < last - 1)).any())
        t_last = g[tag + '_tables'][np.nonzero(p[:, 0] < last)[0][-1]]
        differ |= not np.array_equal(t_last, g[tag + '_best'])
        on_eps |= bool((np.abs(t_last) == np.float32(g['epsilon'][i])).any())
    assert skipped and completed and capped and tie and jumped and differ and on_eps


@pytest.mark.parametrize('i', (0, 1))
def test_restated_loop_reproduces_g29(g, images, i):
    tag = TAGS[i]
    out = UR.run_loop(images, g['cls_w'], **UR.g29_args(g, i))
    assert out['cleared'] > 0                                              # pass-mask bits were cleared in DeepFool's forwards
    assert out['iters_so_far'] == g[tag + '_iters_so_far'].tolist()
    UR.g29_check(g, tag, out['passes'], out['visits'], out['tables'], out['best'], out['export'])
    assert out['last'] is out['best'] or np.array_equal(out['last'], out['tables'][-1])


@pytest.mark.parametrize('i', (0, 1))
def test_deepfool_2d_on_the_cpu_reproduces_g29(g, images, i):
    """The restated loop with nerfail_amd.deepfool.deepfool_2d in DeepFool's place: universal_2D_net and the stand-in
    classifier in torch, float32, on the CPU."""
    from nerfail_amd import deepfool as DF
    from nerfail_amd.GaussNet import universal_2D_net
    tag = TAGS[i]
    w = torch.from_numpy(g['cls_w'])

    class Cls(torch.nn.Module):
        def forward(self, x):
            return (torch.nn.functional.adaptive_avg_pool2d(x.double(), 4).reshape(x.shape[0], -1) @ w.double().t()).float()
    net = universal_2D_net('cpu', 0.02, Cls(), 'vit_b_16')

    def deepfool(table, image, w_, num_classes, max_iter, target, overshoot, m1, m2):
        ori = torch.from_numpy(IR.white(image)[None])
        dr, k, o, arg, r = DF.deepfool_2d((torch.from_numpy(np.array(table, np.float32)), ori), None, net, num_classes, max_iter,
                                          None if target < 0 else target, overshoot, m1, m2)
        assert torch.equal(dr, r - torch.from_numpy(np.asarray(table, np.float32))) and not r.requires_grad
        return r.numpy(), k, None, 0
    out = UR.run_loop(images, g['cls_w'], deepfool=deepfool, **UR.g29_args(g, i))
    UR.g29_check(g, tag, out['passes'], out['visits'], out['tables'], out['best'], out['export'])


def test_deepfool_2d_honours_max_iter_zero_and_the_deprecated_switch(g, images):
    from nerfail_amd import deepfool as DF
    from nerfail_amd.GaussNet import universal_2D_net
    w = torch.from_numpy(g['cls_w'])
    net = universal_2D_net('cpu', 0.02, lambda x: torch.nn.functional.adaptive_avg_pool2d(x, 4).reshape(x.shape[0], -1) @ w.t(), 'vit_b_16')
    table = torch.zeros((224, 224, 3))
    ori = torch.from_numpy(IR.white(images[1])[None])
    dr, k, o, arg, r = DF.deepfool_2d((table, ori), None, net, max_iter=0)
    assert k == 0 and not dr.any() and int(o) == int(arg) == 1 and torch.equal(r, table)
    with pytest.raises(NotImplementedError):
        DF.deepfool((table, ori), None, net, universal_2d=True)
