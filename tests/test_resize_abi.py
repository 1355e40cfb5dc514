"""CPU-side checks of the C ABI section "classifier-input resize (resize revision 1)": header, binding and library agree on the new
prototypes, the revision words stand, nerfail_resize_aa_table writes exactly tests/resize_ref.py's tables, and every documented
refusal of the two launch entry points answers NERFAIL_EINVAL before a launch (without a GPU a launch would answer NERFAIL_EHIP)."""
import ctypes
import os
import re

import numpy as np
import pytest

import resize_ref as RR
from conftest import ROOT

NEW = ('nerfail_resize_revision', 'nerfail_resize_aa_kmax', 'nerfail_resize_aa_table', 'nerfail_resize_tiles',
       'nerfail_cls_input_resize_fwd', 'nerfail_cls_input_resize_bwd')
CTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}
AXES = [(800, 299), (800, 224), (37, 16), (53, 16), (20, 29), (23, 29), (16, 16), (5, 3), (7, 3), (299, 299), (300, 299), (3, 8)]
REFUSED = [(800, 64), (3, 40)]


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read(), flags=re.S)


def _prototypes():
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(nerfail_resize_[a-z0-9_]+|nerfail_cls_input_resize_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _header()):
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
    assert len(protos['nerfail_cls_input_resize_fwd'][1]) == 11 and len(protos['nerfail_cls_input_resize_bwd'][1]) == 13
    fields = re.search(r'typedef struct nerfail_resize_axis \{(.*?)\}', _header(), flags=re.S).group(1)
    names = re.findall(r'(\w+)\s*[;,]', fields)
    assert names == [f[0] for f in _lib.ResizeAxisStruct._fields_]
    assert ctypes.sizeof(_lib.ResizeAxisStruct) == 5 * 8 + 4 * 4
    assert '#define NERFAIL_RESIZE_MAX_TAPS 16' in _header() and _lib.RESIZE_MAX_TAPS == 16 == RR.MAX_TAPS


def test_revision_words():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_resize_revision() == 1 == _lib.RESIZE_REVISION
    assert lib.nerfail_abi_version() == 14 == _lib.ABI_VERSION
    assert lib.nerfail_abi_revision() == 15 == _lib.ABI_REVISION
    assert (lib.nerfail_eval_revision() == lib.nerfail_cls_revision() == lib.nerfail_deepfool_revision() == lib.nerfail_scene_revision()
            == lib.nerfail_u2d_revision() == lib.nerfail_uap2d_revision() == lib.nerfail_poison_revision() == 1)


def _c_table(n_in, n_out, kmax=None):
    from nerfail_amd import _lib
    lib = _lib.load()
    k = lib.nerfail_resize_aa_kmax(n_in, n_out) if kmax is None else kmax
    start, count = np.full(n_out, -7, np.int32), np.full(n_out, -7, np.int32)
    w = np.full((n_out, max(k, 1)), -7, np.float32)
    ostart, ocount = np.full(n_in, -7, np.int32), np.full(n_in, -7, np.int32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    rc = lib.nerfail_resize_aa_table(n_in, n_out, P(start), P(count), P(w), k, P(ostart), P(ocount))
    return rc, dict(start=start, count=count, w=w, ostart=ostart, ocount=ocount, kmax=k)


@pytest.mark.parametrize('n_in, n_out', AXES)
def test_the_table_builder_writes_the_definitions_tables(n_in, n_out):
    rc, got = _c_table(n_in, n_out)
    want = RR.axis_table(n_in, n_out)
    assert rc == 0 and not want['refused'] and got['kmax'] == want['kmax']
    for k in ('start', 'count', 'ostart', 'ocount'):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got['w'].view(np.int32), want['w'].view(np.int32))          # float32 weights, bit for bit
    rc, wide = _c_table(n_in, n_out, kmax=want['kmax'] + 2)                             # a wider row: the same floats, then +0
    assert rc == 0 and np.array_equal(wide['w'][:, :want['kmax']], want['w']) and not wide['w'][:, want['kmax']:].any()


@pytest.mark.parametrize('n_in, n_out', REFUSED)
def test_the_table_builder_refuses_more_than_16_taps(n_in, n_out):
    from nerfail_amd import _lib
    assert RR.axis_table(n_in, n_out)['refused']
    rc, _ = _c_table(n_in, n_out, kmax=64)
    assert rc == 1 and b'nerfail_resize_aa_table' in _lib.load().nerfail_last_error()


def test_the_table_builder_refuses_bad_arguments():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert lib.nerfail_resize_aa_kmax(0, 5) == 0 and lib.nerfail_resize_aa_kmax(5, 0) == 0 and lib.nerfail_resize_aa_kmax(800, 299) == 6
    assert _c_table(37, 16, kmax=2)[0] == 1                                            # below the largest count
    buf = (ctypes.c_int32 * 64)()
    assert lib.nerfail_resize_aa_table(0, 4, buf, buf, buf, 4, buf, buf) == 1
    assert lib.nerfail_resize_aa_table(4, 0, buf, buf, buf, 4, buf, buf) == 1
    assert lib.nerfail_resize_aa_table(5, 3, None, buf, buf, 4, buf, buf) == 1
    f, b = (ctypes.c_int32 * 2)(), (ctypes.c_int32 * 2)()
    assert lib.nerfail_resize_tiles(800, 800, 299, 299, f, b) == 0 and list(f) == [16, 32] and list(b) == [16, 64]
    assert lib.nerfail_resize_tiles(800, 800, 64, 64, f, b) == 1 and lib.nerfail_resize_tiles(800, 800, 299, 299, None, b) == 1


FAKE = 0x10000                                                                         # never dereferenced: refused first


def _axis(n_in, n_out, kmax=None, null=None):
    from nerfail_amd import _lib
    st = _lib.ResizeAxisStruct()
    st.start, st.count, st.w, st.ostart, st.ocount = FAKE, FAKE + 0x1000, FAKE + 0x2000, FAKE + 0x3000, FAKE + 0x4000
    if null:
        setattr(st, null, None)
    st.n_in, st.n_out = n_in, n_out
    st.kmax = _lib.load().nerfail_resize_aa_kmax(n_in, n_out) if kmax is None else kmax
    return st


def _launch(which, src=FAKE * 2, out=FAKE * 3, g=FAKE * 4, layout=0, R=1, B=2, H=37, W=53, oh=16, ow=16, ty=None, tx=None, no_ty=False):
    from nerfail_amd import _lib
    lib = _lib.load()
    ty = _axis(H, oh) if ty is None else ty
    tx = _axis(W, ow) if tx is None else tx
    ty_ref = None if no_ty else ctypes.byref(ty)
    if which == 'fwd':
        return lib.nerfail_cls_input_resize_fwd(src, layout, B, H, W, oh, ow, ty_ref, ctypes.byref(tx), out, None)
    return lib.nerfail_cls_input_resize_bwd(g, R, src, layout, B, H, W, oh, ow, ty_ref, ctypes.byref(tx), out, None)


COMMON = [
    ('out NULL', dict(out=None)),
    ('ty NULL', dict(no_ty=True)),
    ('a table pointer NULL', dict(tx=lambda: _axis(53, 16, null='w'))),
    ('an inverted table pointer NULL', dict(ty=lambda: _axis(37, 16, null='ocount'))),
    ('layout 2', dict(layout=2)),
    ('layout -1', dict(layout=-1)),
    ('B = 0', dict(B=0)),
    ('B = 65536', dict(B=65536)),
    ('H = 0', dict(H=0)),
    ('ow = 0', dict(ow=0)),
    ('ty of another shape', dict(ty=lambda: _axis(38, 16))),
    ('tx of another shape', dict(tx=lambda: _axis(53, 17))),
    ('kmax 0', dict(tx=lambda: _axis(53, 16, kmax=0))),
    ('kmax 17', dict(ty=lambda: _axis(37, 16, kmax=17))),
    ('kmax below the largest count', dict(ty=lambda: _axis(37, 16, kmax=3))),
    ('more than 16 taps', dict(H=800, oh=64)),
    ('inverted count above 16', dict(W=3, ow=40)),
    ('out not 4-byte aligned', dict(out=FAKE * 3 + 2)),
]


def _kw(kw):
    return {k: (v() if callable(v) else v) for k, v in kw.items()}


@pytest.mark.parametrize('what, kw', COMMON + [('src NULL', dict(src=None)), ('layout 0 src only 8-byte aligned', dict(src=FAKE * 2 + 8)),
                                               ('layout 1 src not 4-byte aligned', dict(src=FAKE * 2 + 2, layout=1))])
def test_forward_refusals_answer_before_a_launch(what, kw):
    from nerfail_amd import _lib
    assert _launch('fwd', **_kw(kw)) == 1, what                                        # NERFAIL_EINVAL
    assert b'nerfail_cls_input_resize_fwd' in _lib.load().nerfail_last_error(), what


@pytest.mark.parametrize('what, kw', COMMON + [('g NULL', dict(g=None)), ('R = 0', dict(R=0)), ('R = 9', dict(R=9)), ('R = -1', dict(R=-1)),
                                               ('layout 0 with a NULL src', dict(src=None)),
                                               ('layout 0 gsrc only 8-byte aligned', dict(out=FAKE * 3 + 8)),
                                               ('layout 0 src only 4-byte aligned', dict(src=FAKE * 2 + 4))])
def test_adjoint_refusals_answer_before_a_launch(what, kw):
    from nerfail_amd import _lib
    assert _launch('bwd', **_kw(kw)) == 1, what
    assert b'nerfail_cls_input_resize_bwd' in _lib.load().nerfail_last_error(), what


def test_the_source_keeps_the_definitions_arithmetic():
    """Separately rounded products and sums, no fused multiply-add, no atomics; weights come from the tables."""
    text = open(os.path.join(ROOT, 'nerfail_amd', 'csrc', 'resize.hip')).read()
    assert '__fadd_rn(acc, __fmul_rn(' in text and 'fmaf' not in text and 'atomic' not in text.lower().replace('no atomics', '')
    from nerfail_amd import build
    assert '-ffp-contract=off' in build.CFLAGS and 'resize.hip' not in build.FILE_FLAGS
