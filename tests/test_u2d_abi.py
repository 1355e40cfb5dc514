"""CPU-side checks of the C ABI section "2-D baseline (u2d revision 1)": header, binding and library agree on the five new
prototypes, the revision words stand, and every documented refusal answers NERFAIL_EINVAL before a launch (without a GPU a
launch would answer NERFAIL_EHIP instead)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ('nerfail_u2d_revision', 'nerfail_u2d_fwd', 'nerfail_u2d_step', 'nerfail_u2d_sqerr', 'nerfail_u2d_epoch_close')
CTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _prototypes():
    text = open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(nerfail_u2d_[a-z_]+)\s*\(([^)]*)\)\s*;', text):
        types = []
        for a in [a.strip() for a in args.split(',')]:
            if a == 'void':
                continue
            types.append(ctypes.c_void_p if '*' in a else CTYPE[a.split()[-2]])
        out[name] = (CTYPE[ret], types)
    return out


def test_header_binding_and_library_agree():
    from nerfail_amd import _lib
    lib = _lib.load()
    protos = _prototypes()
    assert sorted(protos) == sorted(NEW)
    for name in NEW:
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == protos[name], (name, _lib.SIGNATURES[name], protos[name])


def test_revision_words():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_abi_version() == 14 == _lib.ABI_VERSION
    assert lib.nerfail_abi_revision() == 15 == _lib.ABI_REVISION
    assert lib.nerfail_eval_revision() == lib.nerfail_cls_revision() == lib.nerfail_deepfool_revision() == lib.nerfail_scene_revision() == 1
    assert lib.nerfail_u2d_revision() == 1 == _lib.U2D_REVISION


P_IMG, P_IDX, P_R, P_X, P_C, P_M, P_D, P_ROW, P_SCR = (0x10000 * k for k in range(1, 10))      # never dereferenced: refused first
U8C4, U8C3 = 0, 1


def _fwd(lib, images=P_IMG, fmt=U8C4, N=7, P=64, idx=P_IDX, B=2, r=P_R, shared=0, x=P_X, c=P_C, m=P_M):
    return lib.nerfail_u2d_fwd(images, fmt, N, P, idx, B, r, shared, x, c, m, None)


def _step(lib, r=P_R, N=7, P=64, idx=P_IDX, B=2, d=P_D, m=P_M, init=None, a=2., eps=32., targeted=0):
    return lib.nerfail_u2d_step(r, N, P, idx, B, d, m, init, a, eps, targeted, None)


def _sqerr(lib, x=P_X, images=P_IMG, fmt=U8C4, N=7, P=64, idx=P_IDX, B=2, scratch=P_SCR, row=P_ROW):
    return lib.nerfail_u2d_sqerr(x, images, fmt, N, P, idx, B, scratch, row, None)


@pytest.mark.parametrize('what, call', [
    ('fwd: images NULL', lambda l: _fwd(l, images=None)),
    ('fwd: idx NULL', lambda l: _fwd(l, idx=None)),
    ('fwd: r NULL', lambda l: _fwd(l, r=None)),
    ('fwd: both outputs NULL', lambda l: _fwd(l, x=None, c=None)),
    ('fwd: bad format', lambda l: _fwd(l, fmt=2)),
    ('fwd: negative format', lambda l: _fwd(l, fmt=-1)),
    ('fwd: P == 0', lambda l: _fwd(l, P=0)),
    ('fwd: P < 0', lambda l: _fwd(l, P=-3)),
    ('fwd: B > 65535', lambda l: _fwd(l, B=65536)),
    ('fwd: misaligned U8C4 base', lambda l: _fwd(l, images=P_IMG + 4)),
    ('fwd: misaligned U8C3 base', lambda l: _fwd(l, fmt=U8C3, images=P_IMG + 2)),
    ('step: r NULL', lambda l: _step(l, r=None)),
    ('step: idx NULL', lambda l: _step(l, idx=None)),
    ('step: d_cls_in NULL', lambda l: _step(l, d=None)),
    ('step: pass_mask NULL', lambda l: _step(l, m=None)),
    ('step: P == 0', lambda l: _step(l, P=0)),
    ('step: B > 65535', lambda l: _step(l, B=65536)),
    ('step: negative epsilon', lambda l: _step(l, eps=-1.)),
    ('step: NaN epsilon', lambda l: _step(l, eps=float('nan'))),
    ('step: infinite a', lambda l: _step(l, a=float('inf'))),
    ('step: NaN a', lambda l: _step(l, a=float('nan'))),
    ('sqerr: x_rgb NULL', lambda l: _sqerr(l, x=None)),
    ('sqerr: images NULL', lambda l: _sqerr(l, images=None)),
    ('sqerr: idx NULL', lambda l: _sqerr(l, idx=None)),
    ('sqerr: row NULL', lambda l: _sqerr(l, row=None)),
    ('sqerr: scratch NULL', lambda l: _sqerr(l, scratch=None)),
    ('sqerr: bad format', lambda l: _sqerr(l, fmt=3)),
    ('sqerr: P == 0', lambda l: _sqerr(l, P=0)),
    ('sqerr: B > 65535', lambda l: _sqerr(l, B=65536)),
    ('sqerr: misaligned U8C4 base', lambda l: _sqerr(l, images=P_IMG + 8)),
    ('close: row NULL', lambda l: l.nerfail_u2d_epoch_close(None, P_X, 0, 0, P_R, P_M, None)),
    ('close: flag NULL', lambda l: l.nerfail_u2d_epoch_close(P_ROW, P_X, 0, 0, P_R, None, None)),
    ('close: negative epoch', lambda l: l.nerfail_u2d_epoch_close(P_ROW, P_X, -1, 0, P_R, P_M, None)),
])
def test_refusals_answer_before_a_launch(what, call):
    from nerfail_amd import _lib
    lib = _lib.load()
    assert call(lib) == 1, what                                          # NERFAIL_EINVAL
    assert b'nerfail_u2d_' in lib.nerfail_last_error(), what


def test_empty_batches_are_no_ops():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert _fwd(lib, B=0) == 0 and _step(lib, B=0) == 0 and _sqerr(lib, B=0) == 0
