"""CPU-side checks of the scene-maps boundary (scene revision 1): header, binding and library agree on the entry points and
their argument lists, the revision words stand as documented, and the host-side refusals answer before any launch."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ('nerfail_scene_revision', 'nerfail_knn8_grid_weights_workspace_bytes', 'nerfail_knn8_grid_weights_view', 'nerfail_knn8_grid_weights')
CTYPE = {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nerfail_hip.h')).read(), flags=re.S)


def _prototype(text, name):
    """(restype, argtypes) of `name` as the header declares it; every pointer is a c_void_p in the binding."""
    res, args = re.search(r'(\w[\w\s\*]*?)\b%s\s*\((.*?)\)\s*;' % name, text, flags=re.S).groups()
    out = []
    for a in [a.strip() for a in args.split(',')]:
        if a == 'void':
            continue
        typ = re.sub(r'\bconst\b', '', a).strip()
        typ = typ[:typ.rindex(re.search(r'(\w+)$', typ).group(1))].strip()        # drop the parameter's name
        out.append(ctypes.c_void_p if typ.endswith('*') else CTYPE[typ])
    return CTYPE[res.strip()], out


def test_header_binding_and_library_agree():
    from nerfail_amd import _lib
    lib = _lib.load()
    text = _header()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == _prototype(text, name), name
    assert len(_lib.SIGNATURES['nerfail_knn8_grid_weights_view'][1]) == 12 and len(_lib.SIGNATURES['nerfail_knn8_grid_weights'][1]) == 11
    assert lib.nerfail_scene_revision() == _lib.SCENE_REVISION == 1
    assert lib.nerfail_abi_version() == _lib.ABI_VERSION == 14 and lib.nerfail_abi_revision() == _lib.ABI_REVISION == 15
    assert int(re.search(r'#define NERFAIL_ABI_VERSION (\d+)', text).group(1)) == 14


def test_the_parser_reads_a_known_prototype():
    from nerfail_amd import _lib
    assert _prototype(_header(), 'nerfail_knn8_grid_search_view') == _lib.SIGNATURES['nerfail_knn8_grid_search_view']
    assert _prototype(_header(), 'nerfail_gauss_weight') == _lib.SIGNATURES['nerfail_gauss_weight']


def test_workspace_size_and_refusals_without_gpu():
    from nerfail_amd import _lib
    lib = _lib.load()
    size = lib.nerfail_knn8_grid_weights_workspace_bytes
    assert size(0) == 0 and size(-3) == 0
    assert size(1) == 256 and size(640000) == 640000 and size(640001) % 256 == 0
    for H, W in ((1, 999), (999, 1), (9, 130), (37, 53), (800, 800), (8, 8)):      # one double per 8 x 8 tile always fits
        assert size(H * W) >= 8 * ((H + 7) // 8) * ((W + 7) // 8), (H, W)
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(260)          # never dereferenced: every call below is refused before a launch
    M, H, W = 12288, 37, 53
    gbytes, wbytes = lib.nerfail_knn8_grid_workspace_bytes(M), size(H * W)

    def view(q=one, h=H, w=W, m=M, c=0.02, out=one, d2=one, grid=one, gb=gbytes, ws=one, wb=wbytes):
        return lib.nerfail_knn8_grid_weights_view(q, h, w, m, c, out, d2, grid, gb, ws, wb, None)

    def flat(q=one, n=H * W, m=M, c=0.02, out=one, d2=one, grid=one, gb=gbytes, ws=one, wb=wbytes):
        return lib.nerfail_knn8_grid_weights(q, n, m, c, out, d2, grid, gb, ws, wb, None)
    cases = ((dict(c=0.0), b'c must be positive'), (dict(c=-0.02), b'c must be positive'), (dict(c=float('nan')), b'c must be positive'),
             (dict(out=odd), b'16-byte aligned'), (dict(out=None), b'NULL'), (dict(q=None), b'NULL'),
             (dict(wb=wbytes - 1), b'workspace too small'), (dict(ws=None), b'workspace too small'),
             (dict(gb=gbytes - 1), b'grid workspace too small'), (dict(grid=None), b'grid workspace too small'),
             (dict(m=7), b'n_points'), (dict(m=1 << 24), b'n_points'), (dict(d2=odd), b'sum_d2'))
    for call in (view, flat):
        for kw, word in cases:
            assert call(**kw) == 1, kw
            msg = lib.nerfail_last_error()
            assert b'grid_weights' in msg and word in msg, (kw, msg)
    for kw, word in ((dict(h=0), b'view size'), (dict(w=-1), b'view size')):
        assert view(**kw) == 1 and word in lib.nerfail_last_error(), kw
    assert flat(n=0) == 1 and b'n_queries' in lib.nerfail_last_error()
    # a view one pixel high needs one slot per 8 pixels: the size helper gives that, a smaller buffer is refused
    assert view(h=1, w=H * W, wb=8 * ((H * W + 7) // 8) - 8) == 1 and b'workspace too small' in lib.nerfail_last_error()
