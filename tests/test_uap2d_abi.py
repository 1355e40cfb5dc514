"""CPU-side checks of the C ABI section "2-D universal baseline (uap2d revision 1)": header, binding and library agree on the
four new prototypes, the revision words stand, and every documented refusal answers NERFAIL_EINVAL before a launch (without a
GPU a launch would answer NERFAIL_EHIP instead)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ('nerfail_uap2d_revision', 'nerfail_uap2d_step_scratch_bytes', 'nerfail_uap2d_step', 'nerfail_uap2d_accumulate')
CTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read(), flags=re.S)


def _prototypes():
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(nerfail_uap2d_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _header()):
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
    assert len(protos['nerfail_uap2d_step'][1]) == 13 and len(protos['nerfail_uap2d_accumulate'][1]) == 5
    terms = int(re.search(r'#define\s+NERFAIL_UAP2D_NORM_TERMS\s+(\d+)', _header()).group(1))
    assert terms == _lib.UAP2D_NORM_TERMS and terms % 12 == 0              # whole quads of four pixels x three channels


def test_revision_words():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_uap2d_revision() == 1 == _lib.UAP2D_REVISION
    assert lib.nerfail_abi_version() == 14 == _lib.ABI_VERSION
    assert lib.nerfail_abi_revision() == 15 == _lib.ABI_REVISION
    assert (lib.nerfail_eval_revision() == lib.nerfail_cls_revision() == lib.nerfail_deepfool_revision() == lib.nerfail_scene_revision()
            == lib.nerfail_u2d_revision() == 1)


def test_scratch_bytes():
    from nerfail_amd import _lib
    lib = _lib.load()
    per_group = 256 * _lib.UAP2D_NORM_TERMS // 3                          # pixels of one norm workgroup
    tail = 64                                                             # {norms2[8], best, scale}
    for n_rhs in (2, 3, 8):
        assert lib.nerfail_uap2d_step_scratch_bytes(n_rhs, 1) == 8 * (n_rhs - 1) + tail
        assert lib.nerfail_uap2d_step_scratch_bytes(n_rhs, per_group) == 8 * (n_rhs - 1) + tail
        assert lib.nerfail_uap2d_step_scratch_bytes(n_rhs, per_group + 1) == 16 * (n_rhs - 1) + tail
    for n_rhs, P in ((1, 64), (9, 64), (3, 0), (3, -1), (3, 2 ** 31 + 1)):
        assert lib.nerfail_uap2d_step_scratch_bytes(n_rhs, P) == 0, (n_rhs, P)
    assert lib.nerfail_uap2d_step_scratch_bytes(8, 2 ** 31) == 8 * 7 * (2 ** 31 // per_group) + tail


P_G, P_M, P_REC, P_SCR, P_R0, P_ROT, P_OUT, P_TR, P_T = (0x10000 * k for k in range(1, 10))     # never dereferenced: refused first
BIG = 1 << 20


def _step(lib, g=P_G, n_rhs=3, P=64, m=P_M, rec=P_REC, scr=P_SCR, nb=BIG, overshoot=0.02, r0=P_R0, rot=P_ROT, out=P_OUT, tr=P_TR):
    return lib.nerfail_uap2d_step(g, n_rhs, P, m, rec, scr, nb, overshoot, r0, rot, out, tr, None)


def _acc(lib, t=P_T, rf=P_R0, eps=8., n=192):
    return lib.nerfail_uap2d_accumulate(t, rf, eps, n, None)


@pytest.mark.parametrize('what, call', [
    ('step: grads NULL', lambda l: _step(l, g=None)),
    ('step: pass_mask NULL', lambda l: _step(l, m=None)),
    ('step: record NULL', lambda l: _step(l, rec=None)),
    ('step: scratch NULL', lambda l: _step(l, scr=None)),
    ('step: r0 NULL', lambda l: _step(l, r0=None)),
    ('step: rot NULL', lambda l: _step(l, rot=None)),
    ('step: r_out NULL', lambda l: _step(l, out=None)),
    ('step: trace_slot NULL', lambda l: _step(l, tr=None)),
    ('step: n_rhs 1', lambda l: _step(l, n_rhs=1)),
    ('step: n_rhs 9', lambda l: _step(l, n_rhs=9)),
    ('step: P == 0', lambda l: _step(l, P=0)),
    ('step: P < 0', lambda l: _step(l, P=-5)),
    ('step: P > 2^31', lambda l: _step(l, P=2 ** 31 + 1, nb=1 << 40)),
    ('step: scratch too small', lambda l: _step(l, nb=8 * 2 + 63)),
    ('step: scratch not 8-byte aligned', lambda l: _step(l, scr=P_SCR + 4)),
    ('step: grads not 4-byte aligned', lambda l: _step(l, g=P_G + 2)),
    ('step: r0 not 4-byte aligned', lambda l: _step(l, r0=P_R0 + 1)),
    ('step: rot not 4-byte aligned', lambda l: _step(l, rot=P_ROT + 2)),
    ('step: r_out not 4-byte aligned', lambda l: _step(l, out=P_OUT + 3)),
    ('step: infinite overshoot', lambda l: _step(l, overshoot=float('inf'))),
    ('step: NaN overshoot', lambda l: _step(l, overshoot=float('nan'))),
    ('accumulate: table NULL', lambda l: _acc(l, t=None)),
    ('accumulate: r_final NULL', lambda l: _acc(l, rf=None)),
    ('accumulate: n == 0', lambda l: _acc(l, n=0)),
    ('accumulate: n < 0', lambda l: _acc(l, n=-3)),
    ('accumulate: n > 3 * 2^31', lambda l: _acc(l, n=3 * 2 ** 31 + 1)),
    ('accumulate: negative epsilon', lambda l: _acc(l, eps=-1.)),
    ('accumulate: NaN epsilon', lambda l: _acc(l, eps=float('nan'))),
    ('accumulate: table not 4-byte aligned', lambda l: _acc(l, t=P_T + 2)),
    ('accumulate: r_final not 4-byte aligned', lambda l: _acc(l, rf=P_R0 + 1)),
])
def test_refusals_answer_before_a_launch(what, call):
    from nerfail_amd import _lib
    lib = _lib.load()
    assert call(lib) == 1, what                                          # NERFAIL_EINVAL
    assert b'nerfail_uap2d_' in lib.nerfail_last_error(), what


def test_the_choice_has_one_definition():
    """deepfool.hip and uap2d.hip both choose through csrc/deepfool_choose.h; neither restates DF:81-96."""
    csrc = os.path.join(ROOT, 'nerfail_amd', 'csrc')
    for name in ('deepfool.hip', 'uap2d.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "deepfool_choose.h"' in text and 'deepfool_choose_body(' in text, name
        assert 'minv' not in text, name
    assert open(os.path.join(csrc, 'deepfool_choose.h')).read().count('if (vr < minv)') == 1
