"""CPU-side checks of the DeepFool gate / step boundary (deepfool revision 1): header, binding and library agree on the entry
points and the revision word, the host-side refusals answer as documented, and attack.nerfail refuses what it cannot run."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _header():
    return open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read()


def test_header_binding_and_library_agree():
    from nerfail_amd import _lib
    lib = _lib.load()
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    for name in ('nerfail_deepfool_revision', 'nerfail_deepfool_gate', 'nerfail_deepfool_step', 'nerfail_deepfool_step_scratch_bytes'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.nerfail_deepfool_revision() == _lib.DEEPFOOL_REVISION == 1
    assert lib.nerfail_abi_version() == _lib.ABI_VERSION == 14 and lib.nerfail_abi_revision() == _lib.ABI_REVISION == 15
    assert int(re.search(r'#define NERFAIL_ABI_VERSION (\d+)', text).group(1)) == 14
    assert int(re.search(r'#define NERFAIL_DEEPFOOL_MAX_COMPETITORS (\d+)', text).group(1)) == _lib.DEEPFOOL_MAX_COMPETITORS == 8
    # the record: four words, then the class ids, then |f'|
    body = re.search(r'typedef struct nerfail_deepfool_record \{(.*?)\} nerfail_deepfool_record;', text, flags=re.S).group(1)
    assert re.findall(r'(?:int32_t|float) (\w+)', body) == ['done', 'argmax', 'n_comp', 'targeted', 'cls', 'fabs']
    assert _lib.DEEPFOOL_RECORD_WORDS == 4 + 2 * 8
    # argument lists as the header declares them
    gate = re.search(r'int nerfail_deepfool_gate\((.*?)\);', text, flags=re.S).group(1)
    step = re.search(r'int nerfail_deepfool_step\((.*?)\);', text, flags=re.S).group(1)
    assert len(gate.split(',')) == len(_lib.SIGNATURES['nerfail_deepfool_gate'][1]) == 8
    assert len(step.split(',')) == len(_lib.SIGNATURES['nerfail_deepfool_step'][1]) == 12


def test_refusals_without_gpu():
    from nerfail_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)          # a non-NULL pointer that is never dereferenced: every call below is refused before a launch
    n = 1440
    assert lib.nerfail_deepfool_step_scratch_bytes(8, n) == lib.nerfail_deepfool_norms_scratch_bytes(8, n) + 64
    assert lib.nerfail_deepfool_step_scratch_bytes(3, 3072) == 2 * 2 * 8 + 64
    for bad in ((1, n), (9, n), (8, 0), (8, -5)):
        assert lib.nerfail_deepfool_step_scratch_bytes(*bad) == 0
    big = lib.nerfail_deepfool_step_scratch_bytes(8, n)

    def step(n_rhs=8, n_=n, grads=one, record=one, scratch=one, nbytes=big, s0=one, rot=one, out=one, trace=one):
        return lib.nerfail_deepfool_step(grads, n_rhs, n_, record, scratch, nbytes, 0.02, s0, rot, out, trace, None)
    for kw, word in ((dict(n_rhs=1), b'2..8'), (dict(n_rhs=9), b'2..8'), (dict(n_=0), b'positive'), (dict(n_=-1), b'positive'),
                     (dict(grads=None), b'NULL'), (dict(record=None), b'NULL'), (dict(scratch=None), b'NULL'), (dict(s0=None), b'NULL'),
                     (dict(rot=None), b'NULL'), (dict(out=None), b'NULL'), (dict(trace=None), b'NULL'),
                     (dict(nbytes=big - 1), b'scratch too small'), (dict(nbytes=0), b'scratch too small')):
        assert step(**kw) == 1, kw
        msg = lib.nerfail_last_error()
        assert b'nerfail_deepfool_step' in msg and word in msg, (kw, msg)

    def gate(C=8, o=0, target=-1, cla=one, record=one):
        return lib.nerfail_deepfool_gate(cla, C, o, target, 1.0, 30.0, record, None)
    for kw, word in ((dict(C=1), b'2..8'), (dict(C=9), b'2..8'), (dict(o=-1), b'0..C-1'), (dict(o=8), b'0..C-1'), (dict(C=2, o=2), b'0..C-1'),
                     (dict(target=-2), b'target'), (dict(target=8), b'target'), (dict(cla=None), b'NULL'), (dict(record=None), b'NULL')):
        assert gate(**kw) == 1, kw
        msg = lib.nerfail_last_error()
        assert b'nerfail_deepfool_gate' in msg and word in msg, (kw, msg)
    with pytest.raises(_lib.NerfailError):
        _lib.check(gate(C=0))


def test_nerfail_refuses_bad_epochs_and_more_than_one_rank(monkeypatch):
    from nerfail_amd import attack, sharding
    with pytest.raises(ValueError, match='epochs'):
        attack.nerfail(None, None, [], 0, 0)
    with pytest.raises(ValueError, match='epochs'):
        attack.nerfail(None, None, [], 0, -3)
    with pytest.raises(ValueError, match='export'):                   # (refused before anything touches the device)
        attack.nerfail(None, None, [('w', 'i')], 0, 4, export_views=[])
    with pytest.raises(ValueError, match='export'):
        attack.nerfail(None, None, [], 0, 4)
    monkeypatch.setattr(sharding, 'world_and_rank', lambda group=None: (2, 0))
    with pytest.raises(ValueError, match='rank'):
        attack.nerfail(None, None, [('w', 'i')], 0, 4)


def test_native_signature_extends_the_mirror():
    import inspect
    from nerfail_amd import deepfool
    a = list(inspect.signature(deepfool.deepfool).parameters.values())
    b = list(inspect.signature(deepfool.deepfool_native).parameters.values())
    assert [(p.name, p.default) for p in b[:len(a)]] == [(p.name, p.default) for p in a]
    assert [(p.name, p.default) for p in b[len(a):]] == [('view_ids', None)]
