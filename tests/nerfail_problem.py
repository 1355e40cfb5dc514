"""Fixture g27 (tests/golden/make_golden_nerfail.py) as data for the CPU restatement test and as inputs of attack.nerfail /
deepfool.deepfool_native for the GPU tests. The fixture files travel with the tests, the reference does not."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
TAGS = ('untargeted', 'targeted', 'm2_raise', 'bisect', 'one_by_one')
# columns of a pass record (`passes`)
EPOCH, NEXT_EPOCH, M1_PASS, M1, M2, VIEWS, TEST_LOSS, TEST_ACC, ATTACK_LOSS, ATTACK_ACC, TAKEN, RAISES, TEST_CORRECT, ATTACK_CORRECT = range(14)


def load():
    g = dict(np.load(os.path.join(GOLDEN, 'g27_nerfail.npz')))
    g['runs'] = {}
    for tag in TAGS:
        g['runs'][tag] = dict(np.load(os.path.join(GOLDEN, 'g27_nerfail_%s.npz' % tag)))
    return g


def run_args(g, tag):
    """(targeted, label, m1, m2, m2_max_limit)"""
    i = list(g['tags']).index(tag)
    return bool(g['targeted'][i]), int(g['label'][i]), int(g['m1'][i]), int(g['m2'][i]), int(g['m2_limit'][i])


def shape(g):
    """P, H, W, C, epochs, views, export views, df_max_iter"""
    return [int(v) for v in g['shape']]


def draws(g, tag):
    """{pass number: view indices} of the runs whose loader draws differ from pass to pass (else {}: all twelve views)."""
    pre = 'draws_%s_' % tag
    return {int(k[len(pre):]): [int(v) for v in g[k]] for k in g if isinstance(k, str) and k.startswith(pre)}


def pass_views(g, tag, n_pass):
    return draws(g, tag).get(n_pass, list(range(shape(g)[5])))


def wi_of(g):
    return np.stack([g['w'], g['idx_u16'].astype(np.float32)], 1)       # [views, 2, H, W, 8]


def setup(g, dev, view_ids=True):
    """(net, s0, the dataset's views - twelve and the one only `bisect` draws -, export views) on `dev`: batch-1 items
    (weight_and_index, ori_img[, view id])."""
    import torch
    from nerfail_amd.GaussNet import gauss_net
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                      # noqa: E731
    w = T(g['cls_w'])

    class Cls(torch.nn.Module):
        def forward(self, x):
            # evaluated in float64 and rounded once, as the fixture's generator evaluates it (PoolCls64): order-independent logits
            return (torch.nn.functional.adaptive_avg_pool2d(x.double(), 4).reshape(x.shape[0], -1) @ w.double().t()).float()
    net = gauss_net(dev, 0.02, Cls(), 'my_model', epsilon=None)
    wi, ori = T(wi_of(g)), T(g['ori'].astype(np.float32))
    n_export = shape(g)[6]
    items = [(wi[v:v + 1].contiguous(), ori[v:v + 1].contiguous()) + ((('g27', v),) if view_ids else ()) for v in range(wi.shape[0])]
    return net, T(g['s0']), items, items[:n_export]


def run(g, tag, dev, native=None, view_ids=True, on_export=None, log=None):
    from nerfail_amd.attack import nerfail
    targeted, label, m1, m2, limit = run_args(g, tag)
    net, s0, items, export = setup(g, dev, view_ids)
    P, H, W, C, epochs, _, _, df_max_iter = shape(g)
    views = lambda n_pass: [items[v] for v in pass_views(g, tag, n_pass)]              # noqa: E731
    return nerfail(net, s0, views, label, epochs, m1=m1, m2=m2, targeted=targeted, df_max_iter=df_max_iter, overshoot=float(g['overshoot']),
                   num_classes=C, m2_max_limit=limit, export_views=export, on_export=on_export, log=log, native=native), (net, s0, items, export)
