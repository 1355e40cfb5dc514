"""CPU-side checks of the foreground-only scene-map boundary (fg revision 1): header, binding and library agree on the entry
points, the other revision words stand as they were, the size helper and the host-side refusals answer before any launch, and
build_scene_maps' opt-in keyword refuses a view without an image before it touches a device."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NAMES = ('nerfail_fg_revision', 'nerfail_fg_pixel_list_workspace_bytes', 'nerfail_fg_pixel_list', 'nerfail_ray_gen_list',
         'nerfail_knn8_grid_weights_list')
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
    assert _prototype(text, 'nerfail_ray_gen') == _lib.SIGNATURES['nerfail_ray_gen']              # the parser reads a known one
    assert len(_lib.SIGNATURES['nerfail_knn8_grid_weights_list'][1]) == 13 and len(_lib.SIGNATURES['nerfail_ray_gen_list'][1]) == 10
    assert lib.nerfail_fg_revision() == _lib.FG_REVISION == 1
    assert lib.nerfail_abi_version() == _lib.ABI_VERSION == 14 and lib.nerfail_abi_revision() == _lib.ABI_REVISION == 15
    assert int(re.search(r'#define NERFAIL_ABI_VERSION (\d+)', text).group(1)) == 14
    for rev in ('eval', 'cls', 'deepfool', 'scene', 'u2d', 'uap2d', 'poison', 'resize'):
        assert getattr(lib, 'nerfail_%s_revision' % rev)() == 1, rev


def test_foreground_only_is_opt_in_and_needs_every_image():
    from nerfail_amd import scene
    p = inspect.signature(scene.build_scene_maps).parameters['foreground_only']
    assert p.default is False
    assert 'rendered' in scene.SceneMaps.__init__.__code__.co_varnames
    poses = {'test': np.zeros((2, 4, 4), np.float32), 'train': np.zeros((1, 4, 4), np.float32)}
    img = np.zeros((2, 4, 4, 4), np.uint8)

    def boom(*a, **k):
        raise AssertionError('a device was touched')
    saved = scene._cuda
    scene._cuda = boom
    try:
        for images in (None, {'test': img}, {'test': img[:1], 'train': img[:1]}, {'test': [img[0], None], 'train': img[:1]}):
            with pytest.raises(ValueError, match='every view needs its image'):
                scene.build_scene_maps({}, poses, [4, 4, 1.], None, [0], images=images, foreground_only=True)
        with pytest.raises(ValueError, match='every view needs its image'):                  # one array of poses = the test split
            scene.build_scene_maps({}, poses['test'], [4, 4, 1.], None, [0], foreground_only=True)
    finally:
        scene._cuda = saved


def test_sizes_and_refusals_without_gpu():
    from nerfail_amd import _lib
    lib = _lib.load()
    size = lib.nerfail_fg_pixel_list_workspace_bytes
    assert size(0) == 0 and size(-1) == 0 and size(1 << 31) == 0
    assert size(1) == 256 and size(640000) == 10240 and size(640000) >= 4 * ((640000 + 255) // 256)
    for P in (1, 255, 256, 257, 851, 90000, (1 << 31) - 1):          # one int32 per 256 pixels always fits
        assert size(P) >= 4 * ((P + 255) // 256) and size(P) % 256 == 0, P
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)           # never dereferenced: every call below is refused before a launch

    def plist(img=one, P=851, lst=one, cnt=one, ws=one, wb=None):
        return lib.nerfail_fg_pixel_list(img, P, lst, cnt, ws, size(851) if wb is None else wb, None)
    for kw, word in ((dict(P=0), b'n_pixels'), (dict(P=1 << 31), b'n_pixels'), (dict(img=None), b'NULL'), (dict(lst=None), b'NULL'),
                     (dict(cnt=None), b'NULL'), (dict(img=odd), b'4-byte aligned'), (dict(lst=odd), b'4-byte aligned'),
                     (dict(ws=None), b'workspace too small'), (dict(wb=size(851) - 1), b'workspace too small'), (dict(ws=odd), b'workspace too small')):
        assert plist(**kw) == 1, kw
        msg = lib.nerfail_last_error()
        assert b'nerfail_fg_pixel_list' in msg and word in msg, (kw, msg)

    k4, c2w = _lib.host_floats([50., 50., 20., 20.]), _lib.host_floats([0.] * 12)

    def rays(H=37, W=23, K=k4, c=c2w, pix=one, n=5, out=one):
        return lib.nerfail_ray_gen_list(H, W, K, c, 2., 6., pix, n, out, None)
    assert rays(n=0, pix=None, out=None) == 0                         # an empty list is valid and launches nothing
    for kw, word in ((dict(H=0), b'H and W'), (dict(W=-1), b'H and W'), (dict(H=1 << 16, W=1 << 15), b'H and W'), (dict(n=-1), b'negative'),
                     (dict(pix=None), b'NULL'), (dict(out=None), b'NULL'), (dict(K=None), b'NULL'), (dict(c=None), b'NULL')):
        assert rays(**kw) == 1, kw
        msg = lib.nerfail_last_error()
        assert b'nerfail_ray_gen_list' in msg and word in msg, (kw, msg)

    M, P, n = 12288, 1600, 707
    gbytes, wbytes = lib.nerfail_knn8_grid_workspace_bytes(M), lib.nerfail_knn8_grid_weights_workspace_bytes(n)

    def search(q=one, n=n, pix=one, P=P, m=M, c=0.02, out=one, d2=one, grid=one, gb=gbytes, ws=one, wb=wbytes):
        return lib.nerfail_knn8_grid_weights_list(q, n, pix, P, m, c, out, d2, grid, gb, ws, wb, None)
    cases = ((dict(c=0.0), b'c must be positive'), (dict(c=float('nan')), b'c must be positive'), (dict(out=odd), b'16-byte aligned'),
             (dict(out=None), b'NULL'), (dict(q=None), b'NULL'), (dict(pix=None), b'NULL'), (dict(n=-1), b'n must be'),
             (dict(n=P + 1), b'n must be'), (dict(P=0), b'n_pixels'), (dict(P=1 << 31), b'n_pixels'),
             (dict(wb=wbytes - 1), b'workspace too small'), (dict(ws=None), b'workspace too small'),
             (dict(gb=gbytes - 1), b'grid workspace too small'), (dict(grid=None), b'grid workspace too small'),
             (dict(m=7), b'n_points'), (dict(m=1 << 24), b'n_points'), (dict(d2=ctypes.c_void_p(260)), b'sum_d2'))
    for kw, word in cases:
        assert search(**kw) == 1, kw
        msg = lib.nerfail_last_error()
        assert word in msg, (kw, msg)
