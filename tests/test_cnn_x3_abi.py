"""CPU: the bf16x3 entry points of the MyCNN victim exist with the documented signatures, their host-side refusals fire before any
launch, and the module-level switch validates. The GPU side is tests/test_hip_cnn_x3_kernels.py / _product.py."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

NEW = ('nerfail_cnn_x3_revision', 'nerfail_cnn_x3_packed_bytes', 'nerfail_cnn_pack_x3', 'nerfail_cnn_fwd_x3', 'nerfail_cnn_bwd_data_x3',
       'nerfail_cnn_bwd_data_multi_x3')


def _decl(name):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read(), flags=re.S)
    m = re.search(r'\b(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)\s*;' % name, text)
    assert m, name
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(',')]


def test_symbols_and_signatures():
    from nerfail_amd import _lib
    lib = _lib.load()
    c_i, c_p = ctypes.c_int, ctypes.c_void_p
    for n in NEW:
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert _lib.SIGNATURES['nerfail_cnn_x3_packed_bytes'] == (ctypes.c_size_t, [c_i])
    assert _lib.SIGNATURES['nerfail_cnn_pack_x3'] == (c_i, [c_p, c_i, c_p, c_p])
    # the exact entry points' parameter lists plus packed_x3 (behind packed)
    for exact, x3 in (('nerfail_cnn_fwd', 'nerfail_cnn_fwd_x3'), ('nerfail_cnn_bwd_data', 'nerfail_cnn_bwd_data_x3'),
                      ('nerfail_cnn_bwd_data_multi', 'nerfail_cnn_bwd_data_multi_x3')):
        res, args = _lib.SIGNATURES[exact]
        assert _lib.SIGNATURES[x3] == (res, args[:1] + [c_p] + args[1:]), x3
        (r0, a0), (r1, a1) = _decl(exact), _decl(x3)
        assert r0 == r1 == 'int' and a1[0] == a0[0] and a1[2:] == a0[1:], (a0, a1)
        assert re.fullmatch(r'const void\s*\*\s*packed_x3', a1[1]), a1[1]


def test_revision_words():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_cnn_x3_revision() == 1 == _lib.CNN_X3_REVISION
    assert lib.nerfail_abi_version() == 14 == _lib.ABI_VERSION and lib.nerfail_abi_revision() == 15 == _lib.ABI_REVISION


def test_sizes_and_refusals_without_a_device():
    import cnn_x3_ref as X
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_cnn_x3_packed_bytes(8) == lib.nerfail_cnn_x3_packed_bytes(24) == X.x3_bytes()
    assert lib.nerfail_cnn_x3_packed_bytes(0) == 0 and lib.nerfail_cnn_x3_packed_bytes(4097) == 0
    p = ctypes.c_void_p(16)                       # never dereferenced: every call below is refused on the host
    assert lib.nerfail_cnn_pack_x3(None, 8, p, None) == 1 and lib.nerfail_cnn_pack_x3(p, 8, None, None) == 1
    assert lib.nerfail_cnn_pack_x3(p, 0, p, None) == 1
    assert lib.nerfail_cnn_fwd_x3(p, p, 8, p, 1, 700, 800, p, p, p, None) == 1
    assert b'unsupported H x W' in lib.nerfail_last_error()
    assert lib.nerfail_cnn_fwd_x3(p, None, 8, p, 1, 800, 800, p, p, p, None) == 1
    assert b'packed_x3' in lib.nerfail_last_error()
    assert lib.nerfail_cnn_fwd_x3(p, p, 8, None, 1, 800, 800, p, p, p, None) == 1
    assert lib.nerfail_cnn_fwd_x3(p, p, 8, p, 0, 800, 800, p, p, p, None) == 1
    assert lib.nerfail_cnn_fwd_x3(p, p, 5000, p, 1, 800, 800, p, p, p, None) == 1
    assert lib.nerfail_cnn_bwd_data_x3(p, None, 8, p, p, p, 1, 800, 800, p, p, None) == 1
    assert lib.nerfail_cnn_bwd_data_x3(p, p, 8, p, None, p, 1, 800, 800, p, p, None) == 1
    assert lib.nerfail_cnn_bwd_data_x3(p, p, 8, p, p, p, 1, 765, 800, p, p, None) == 1
    for R, B in ((0, 1), (1, 0), (65536, 1), (256, 256), (-1, 1)):
        assert lib.nerfail_cnn_bwd_data_multi_x3(p, p, 8, p, p, p, R, B, 800, 800, p, p, None) == 1, (R, B)
        assert b'R * B <= 65535' in lib.nerfail_last_error()
    assert lib.nerfail_cnn_bwd_data_multi_x3(p, None, 8, p, p, p, 8, 1, 800, 800, p, p, None) == 1
    assert lib.nerfail_cnn_bwd_data_multi_x3(p, p, 8, p, p, p, 8, 1, 700, 800, p, p, None) == 1


def test_ops_are_listed():
    import nerfail_amd.ops as O
    assert O.CNN_X3_OPS == ('cnn_pack_x3', 'cnn_fwd_x3', 'cnn_bwd_data_x3', 'cnn_bwd_data_multi_x3')
    assert O.CNN_OPS == ('cnn_fwd', 'cnn_bwd_data', 'cnn_bwd_data_multi', 'cnn_bwd_weights')
    for n in O.CNN_X3_OPS:
        assert hasattr(torch.ops.nerfail_mi, n), n


def test_precision_is_validated():
    from nerfail_amd.MyModel import MyCNN
    assert MyCNN(8).precision == 'f32' and MyCNN(8, precision='bf16x3').precision == 'bf16x3'
    assert MyCNN(8, False, 'bf16x3').precision == 'bf16x3'
    for bad in ('bf16', 'f16x3', None, 3):
        with pytest.raises(ValueError, match='precision'):
            MyCNN(8, precision=bad)
    m = MyCNN(8)
    m.precision = 'bf16x3'
    assert m.precision == 'bf16x3'
    with pytest.raises(ValueError, match='precision'):
        m.precision = 'fp32'
    assert m.precision == 'bf16x3'
    assert sorted(MyCNN(8, precision='bf16x3').state_dict()) == sorted(MyCNN(8).state_dict())   # the switch is no tensor


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it is on the GPU: reaches the checks of MyCNN.forward that come before any launch."""
    @property
    def is_cuda(self):
        return True


@pytest.mark.parametrize('trainable', [False, True])
def test_training_is_refused(trainable):
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(8, trainable=trainable, precision='bf16x3')            # parameters require grad, grad mode is on
    x = torch.zeros(1, 3, 800, 800).as_subclass(_OnDevice)
    with pytest.raises(RuntimeError, match='training path is exact f32 only'):
        m(x)
    m.precision = 'f32'
    if not trainable:                                                # the default module's own refusal is unchanged
        with pytest.raises(RuntimeError, match='trainable=True'):
            m(x)
