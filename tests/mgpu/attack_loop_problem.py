"""Fixture g24 as inputs of attack.nerfail_s: shared by tests/test_hip_attack_loop.py and the rank script
tests/mgpu/attack_loop_rank.py (GPU only; the fixture file travels with the tests, the reference does not)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden', 'g24_attack_loop.npz')
TAGS = ('untargeted', 'targeted', 'beta')


def load():
    return dict(np.load(GOLDEN))


def run_args(g, tag):
    i = list(g['tags']).index(tag)
    return bool(g['targeted'][i]), float(g['beta'][i]), int(g['label'][i])


def setup(g, dev, view_ids=False, ori_u8=False):
    """(net, s0, attack batches, export batches) on `dev`. view_ids: name the views ('g24', 0..7)."""
    from nerfail_amd.GaussNet import gauss_net
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                      # noqa: E731
    w = T(g['cls_w'])

    class Cls(torch.nn.Module):
        def forward(self, x):
            # evaluated in float64 and rounded once, as the fixture's generator evaluates it (PoolCls64 there): the float32 logits
            # then do not depend on the summation order of the library or the device
            return (torch.nn.functional.adaptive_avg_pool2d(x.double(), 4).reshape(x.shape[0], -1) @ w.double().t()).float()
    net = gauss_net(dev, 0.02, Cls(), 'my_model', epsilon=None)
    wi, ori = T(g['wi']), T(g['ori'].astype(np.uint8) if ori_u8 else g['ori'])

    def cut(sizes):
        out, v0 = [], 0
        for B in [int(b) for b in sizes]:
            b = (wi[v0:v0 + B].contiguous(), ori[v0:v0 + B].contiguous())
            out.append(b + ([('g24', v) for v in range(v0, v0 + B)],) if view_ids else b)
            v0 += B
        return out
    return net, T(g['s0']), cut(g['train_batches']), cut(g['export_batches'])


def run(g, tag, dev, view_ids=False, group=None, on_export=None, epochs=None, log=None):
    from nerfail_amd.attack import nerfail_s
    targeted, beta, label = run_args(g, tag)
    net, s0, train, export = setup(g, dev, view_ids)
    res = nerfail_s(net, s0, train, label, int(g['shape'][4]) if epochs is None else epochs, float(g['a']), float(g['epsilon']), targeted, beta,
                    export_batches=export, on_export=on_export, log=log, group=group)
    return res, (net, s0, train, export)
