"""CPU side of the multi-right-hand-side MyCNN backward (ABI 10): the size helper and the refusals of
nerfail_cnn_bwd_data_multi are pure host code, checked before any launch. The GPU side is tests/test_hip_cnn_multi.py."""
import ctypes


def test_multi_scratch_bytes_and_refusals_without_gpu():
    from nerfail_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 10
    one = lib.nerfail_cnn_bwd_scratch_bytes(1, 800, 800)
    assert one == 4 * (399 * 399 * 32 + 198 * 198 * 64)                  # the first two stages' pooled outputs, one image
    # R x the single backward's scratch: every gradient buffer holds R * B slices
    for R, B in ((1, 1), (8, 1), (3, 2), (9, 1), (2, 8), (65535, 1), (255, 257)):
        assert lib.nerfail_cnn_bwd_multi_scratch_bytes(R, B, 800, 800) == R * lib.nerfail_cnn_bwd_scratch_bytes(B, 800, 800), (R, B)
    assert lib.nerfail_cnn_bwd_multi_scratch_bytes(3, 2, 766, 893) == 3 * lib.nerfail_cnn_bwd_scratch_bytes(2, 766, 893)
    # 0 for R = 0, negative counts, R * B beyond the grid's z dimension (also where the int product would wrap), bad sizes
    for R, B in ((0, 1), (1, 0), (-1, 1), (65536, 1), (1, 65536), (256, 256), (65535, 2), (65535, 65535), (1 << 30, 4)):
        assert lib.nerfail_cnn_bwd_multi_scratch_bytes(R, B, 800, 800) == 0, (R, B)
    assert lib.nerfail_cnn_bwd_multi_scratch_bytes(8, 1, 700, 800) == 0
    # the call refuses the same counts before it touches a pointer
    p = ctypes.c_void_p(64)                                              # never dereferenced: refused first
    for R, B in ((0, 1), (65536, 1), (256, 256), (65535, 65535)):
        assert lib.nerfail_cnn_bwd_data_multi(p, 24, p, p, p, R, B, 800, 800, p, p, None) == 1, (R, B)
        assert b'R * B' in lib.nerfail_last_error()
    assert lib.nerfail_cnn_bwd_data_multi(p, 24, p, p, p, 8, 1, 700, 800, p, p, None) == 1
    assert b'unsupported H x W' in lib.nerfail_last_error()
    assert lib.nerfail_cnn_bwd_data_multi(None, 24, None, None, None, 8, 1, 800, 800, None, None, None) == 1
    assert b'NULL' in lib.nerfail_last_error()
    assert lib.nerfail_cnn_bwd_data(None, 24, None, None, None, 1, 800, 800, None, None, None) == 1
    assert b'nerfail_cnn_bwd_data:' in lib.nerfail_last_error()


def test_op_is_registered_with_a_fake():
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode
    import nerfail_amd.ops as O
    assert 'cnn_bwd_data_multi' in O.CNN_OPS
    with FakeTensorMode():
        z = torch.empty((4,))
        out = torch.ops.nerfail_mi.cnn_bwd_data_multi(z, z, torch.empty((4,), dtype=torch.uint8), torch.empty((8, 1, 24)), 800, 800)
    assert tuple(out.shape) == (8, 1, 3, 800, 800)
