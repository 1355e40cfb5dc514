"""-m gpu: attack._ExportBuffers.to_host on its own - the one way every export epoch (nerfail_s / nerfail, igsm_2d, uap_2d) takes
its float images to the host as uint8. Against the numpy restatement of nerfail_export_u8's contract (include/nerfail_hip.h):
clamp to [0, 255], round half to even, NaN -> 0. Exact equality, at the smallest shapes at which the staging can go wrong: 105
floats (no multiple of 4, so the next slot would start misaligned without the padding), three images of two sizes in one call,
and a source that starts 4-byte but not 16-byte aligned (a row range of a table)."""
import numpy as np
import pytest
import torch

from hiputil import dev

pytestmark = pytest.mark.gpu

SPECIAL = [-3., -0.25, 0., 0.5, 1.5, 2.5, 254.5, 255., 255.5, 300., float('nan'), float('inf'), float('-inf')]


def source(shape, seed):
    """Random values on both sides of [0, 255], every special value at the front and again in the last elements (the tail the
    128-bit loop leaves over)."""
    rng = np.random.RandomState(seed)
    v = rng.uniform(-40., 300., size=int(np.prod(shape))).astype(np.float32)
    v[::7] = np.floor(v[::7]) + 0.5                                        # more exact halves, even and odd below them
    v[:len(SPECIAL)] = SPECIAL
    v[-len(SPECIAL):] = SPECIAL[::-1]
    return v.reshape(shape)


def expected(v):
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(v), 0., np.rint(np.clip(v, 0., 255.))).astype(np.uint8)


def pinned_arrays(bufs):
    return [t.numpy() for entry in bufs.bufs.values() for t in entry if isinstance(t, torch.Tensor) and t.is_pinned()]


def test_three_images_then_a_misaligned_row_range():
    from nerfail_amd import attack
    bufs = attack._ExportBuffers()
    host = [source((1, 5, 7, 3), 1), source((5, 7, 3), 2), source((2, 5, 7, 4), 3)]
    first = bufs.to_host(*[torch.from_numpy(h).to(dev()) for h in host])
    want = [expected(h) for h in host]
    assert len(first) == 3
    for got, w in zip(first, want):
        assert got.dtype == np.uint8 and got.shape == w.shape
        assert np.array_equal(got, w)
    assert len(pinned_arrays(bufs)) == 1
    for i, got in enumerate(first):
        assert not any(np.shares_memory(got, p) for p in pinned_arrays(bufs))
        assert not any(np.shares_memory(got, other) for other in first[i + 1:])
    n_bufs = len(bufs.bufs)

    table_host = source((3, 5, 7, 3), 4)
    table = torch.from_numpy(table_host).to(dev())
    rows = table[1:2]
    assert table.data_ptr() % 16 == 0 and rows.data_ptr() % 16 == 4      # 420 bytes in
    host2 = [table_host[1:2], source((5, 7, 3), 5), source((2, 5, 7, 4), 6)]
    second = bufs.to_host(rows, *[torch.from_numpy(h).to(dev()) for h in host2[1:]])
    for got, h in zip(second, host2):
        assert got.shape == h.shape and np.array_equal(got, expected(h))
    assert np.array_equal(table.cpu().numpy(), table_host, equal_nan=True)             # the source is only read
    assert len(bufs.bufs) == n_bufs                                        # the same sizes: the same buffers
    for got, w in zip(first, want):                                        # ... which the first call's arrays do not alias
        assert np.array_equal(got, w)
    assert any(not np.array_equal(a, b) for a, b in zip(first, second))
