"""-m gpu: torch.library.opcheck (schema, fake tensor, autograd registration, AOT dispatch) on the two 2-D baseline ops,
torch.ops.nerfail_mi.u2d_fwd and u2d_step, and their values through the op handles against tests/igsm2d_ref.py."""
import numpy as np
import pytest
import torch

import igsm2d_ref as IR
from hiputil import N, dev

pytestmark = pytest.mark.gpu
TESTS = ('test_schema', 'test_faketensor', 'test_autograd_registration', 'test_aot_dispatch_dynamic')


def _inputs():
    rs = np.random.RandomState(4)
    images = rs.randint(0, 256, size=(5, 9, 13, 4)).astype(np.uint8)
    images[..., 3] = rs.randint(0, 2, size=(5, 9, 13)) * 255
    r = rs.uniform(-300, 300, size=(5, 9, 13, 3)).astype(np.float32)
    return images, r, [3, 0, 4]


def test_opcheck():
    import nerfail_amd.ops as O
    assert O.U2D_OPS == ('u2d_fwd', 'u2d_step')
    images, r, idx = _inputs()
    st, rt, ix = torch.from_numpy(images).to(dev()), torch.from_numpy(r).to(dev()), torch.tensor(idx, device=dev())
    for want in ((True, True, True), (False, True, False)):
        res = torch.library.opcheck(torch.ops.nerfail_mi.u2d_fwd.default, (st, ix, rt) + want, test_utils=TESTS)
        assert all(v == 'SUCCESS' for v in res.values()), res
    res = torch.library.opcheck(torch.ops.nerfail_mi.u2d_fwd.default, (st, ix, rt[0].contiguous(), True, True, True), test_utils=TESTS)
    assert all(v == 'SUCCESS' for v in res.values()), res
    _, cls_in, mask = O.u2d_fwd(st, ix, rt, False, True, True)
    d = torch.randn_like(cls_in)
    for init in (None, torch.zeros_like(rt)):
        res = torch.library.opcheck(torch.ops.nerfail_mi.u2d_step.default, (rt.clone(), ix, d, mask, init, 2., 32., False), test_utils=TESTS)
        assert all(v == 'SUCCESS' for v in res.values()), res


def test_op_values():
    import nerfail_amd.ops as O
    images, r, idx = _inputs()
    st, rt, ix = torch.from_numpy(images).to(dev()), torch.from_numpy(r).to(dev()), torch.tensor(idx, device=dev())
    x, c, m = O.u2d_fwd(st, ix, rt, True, True, True)
    wx, wc, wm = IR.u2d_fwd(images.reshape(5, -1, 4), idx, r.reshape(5, -1, 3))
    assert tuple(x.shape) == (3, 9, 13, 3) and tuple(c.shape) == (3, 3, 9, 13) and tuple(m.shape) == (3, 9, 13)
    assert np.array_equal(N(x).reshape(wx.shape), wx) and np.array_equal(N(c).reshape(wc.shape), wc) and np.array_equal(N(m).reshape(wm.shape), wm)
    x0, c0, m0 = O.u2d_fwd(st, ix, rt, False, True, False)
    assert x0.numel() == 0 and m0.numel() == 0 and torch.equal(c0, c)
    d = torch.randn_like(c)
    table = rt.clone()
    O.u2d_step(table, ix, d, m, None, 2., 32., True)
    want = IR.u2d_step(r.reshape(5, -1, 3), idx, N(d).reshape(3, 3, -1), wm, None, 2., 32., True)
    assert np.array_equal(N(table).reshape(want.shape), want)
    with pytest.raises(ValueError):
        O.u2d_fwd(st, ix, rt, False, False, True)
    with pytest.raises(ValueError):
        O.u2d_step(table, ix, d[:2].contiguous(), m, None, 2., 32., True)
