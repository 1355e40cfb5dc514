"""CPU-side checks of the C ABI section "poisoned retrain hand-off (poison revision 1)": header, binding and library agree on the
two new prototypes, the revision words stand, every documented refusal answers NERFAIL_EINVAL before a launch (without a GPU a
launch would answer NERFAIL_EHIP instead), and the rounding to uint8 has one definition."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = ('nerfail_poison_revision', 'nerfail_export_train_views')
CTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read(), flags=re.S)


def _prototypes():
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(nerfail_poison_[a-z0-9_]+|nerfail_export_train_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _header()):
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
    assert len(protos['nerfail_export_train_views'][1]) == 9


def test_revision_words():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_poison_revision() == 1 == _lib.POISON_REVISION
    assert lib.nerfail_abi_version() == 14 == _lib.ABI_VERSION
    assert lib.nerfail_abi_revision() == 15 == _lib.ABI_REVISION
    assert (lib.nerfail_eval_revision() == lib.nerfail_cls_revision() == lib.nerfail_deepfool_revision() == lib.nerfail_scene_revision()
            == lib.nerfail_u2d_revision() == lib.nerfail_uap2d_revision() == 1)


P_X, P_ADV, P_TGT = 0x10000, 0x20000, 0x30000                             # never dereferenced: refused first


def _call(lib, x=P_X, channels=4, B=3, P=35, slots=(4, 0, 2), n_slots=5, adv=P_ADV, tgt=P_TGT):
    tab = None if slots is None else (ctypes.c_int32 * len(slots))(*slots)
    return lib.nerfail_export_train_views(x, channels, B, P, tab, n_slots, adv, tgt, None)


@pytest.mark.parametrize('what, kw', [
    ('x NULL', dict(x=None)),
    ('slots NULL', dict(slots=None)),
    ('adv_u8 NULL', dict(adv=None)),
    ('target NULL', dict(tgt=None)),
    ('channels 2', dict(channels=2)),
    ('channels 5', dict(channels=5)),
    ('B < 0', dict(B=-1)),
    ('B > 65535', dict(B=65536)),
    ('P == 0', dict(P=0)),
    ('P > 2^31', dict(P=2 ** 31 + 1)),
    ('n_slots == 0', dict(n_slots=0)),
    ('slot == n_slots', dict(slots=(4, 5, 2))),
    ('slot < 0', dict(slots=(4, -1, 2))),
    ('a slot twice', dict(slots=(4, 0, 4))),
    ('4-channel x only 4-byte aligned', dict(x=P_X + 4)),
    ('4-channel x only 8-byte aligned', dict(x=P_X + 8)),
    ('3-channel x not 4-byte aligned', dict(x=P_X + 2, channels=3)),
    ('adv_u8 not 4-byte aligned', dict(adv=P_ADV + 2)),
    ('target not 4-byte aligned', dict(tgt=P_TGT + 1)),
])
def test_refusals_answer_before_a_launch(what, kw):
    from nerfail_amd import _lib
    lib = _lib.load()
    assert _call(lib, **kw) == 1, what                                    # NERFAIL_EINVAL
    assert b'nerfail_export_train_views' in lib.nerfail_last_error(), what


def test_no_views_is_a_no_op():
    from nerfail_amd import _lib
    assert _call(_lib.load(), B=0, slots=()) == 0


def test_the_rounding_has_one_definition():
    """nerfail_export_u8 and nerfail_export_train_views round through common.h's to_u8; neither source restates it, and the
    target's arithmetic is the divide and three separately rounded operations - no reciprocal, no fused multiply-add."""
    csrc = os.path.join(ROOT, 'nerfail_amd', 'csrc')
    define = '__device__ __forceinline__ unsigned to_u8(float v)'
    assert open(os.path.join(csrc, 'common.h')).read().count(define) == 1
    for name in ('attack_stats.hip', 'poison.hip'):
        text = open(os.path.join(csrc, name)).read()
        assert 'to_u8(' in text and define not in text and 'rintf' not in text, name
    poison = open(os.path.join(csrc, 'poison.hip')).read()
    assert '(float)((double)q / 255.0)' in poison and '__fadd_rn(__fmul_rn(c, a), __fsub_rn(1.f, a))' in poison
    assert 'fmaf' not in poison and '1.f / 255' not in poison and 'atomic' not in poison.lower()
