"""The six MLP weight images, looked at directly: every byte each packer writes is pinned against digests recorded from
the commit BEFORE the packers were unified (one column map, one layer table, csrc/mlp_pack.hip), so that a slip in a
packer shows here, bit for bit, and not as a parity failure far downstream.

Every image is packed through the C ABI into a buffer pre-filled with a byte pattern: an element a packer stops (or
starts) writing changes the digest. The f32 forward image has bytes nobody writes (the rest of a bias piece, the end
padding of the weight stream); the same image packed over two different patterns tells which, and the images the Python
API allocates itself (torch.empty) are compared on the written bytes only.

test_hip_mlp_images.json was made by running this module as a script (`python tests/test_hip_mlp_images.py`) on an
MI355X with NERFAIL_HIP_LIB pointing at a library built from that parent commit - never from the tree under test."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

DIGESTS = os.path.splitext(os.path.abspath(__file__))[0] + '.json'
# (D, W, skip), the smallest that reach every branch of the column maps: no skip, NT = 2, one views tile | the encoding
# re-enters at layer 2 | odd depth, encoding at layer 1 | the shipped shape (the only one with a bf16x3 image)
SHAPES = [(2, 64, -1), (4, 64, 1), (3, 128, 0), (8, 256, 4)]
PLANTED = (0.0, -0.0, 1e-30, -59.5)                              # inside the fp16-split range |w| < 60
SEED = 20261017
FILL = 0xA5


def shape_id(s):
    return 'D%d_W%d_skip%d' % s


def make_net(shape, seed=SEED):
    """NeRF of `shape` on the GPU; every tensor f32 standard_normal * 0.5 with PLANTED at fixed positions."""
    from nerfail_amd.run_nerf_helpers import NeRF
    D, W, skip = shape
    net = NeRF(D=D, W=W, input_ch=63, input_ch_views=27, output_ch=5, skips=[skip] if skip >= 0 else [], use_viewdirs=True)
    rng = np.random.default_rng(seed)
    sd = {}
    for k, v in net.state_dict().items():
        a = (rng.standard_normal(tuple(v.shape)) * 0.5).astype(np.float32)
        flat, n = a.reshape(-1), a.size
        for i, p in enumerate(PLANTED):
            flat[(i * (n - 1)) // 3] = p
        sd[k] = torch.from_numpy(a)
    net.load_state_dict(sd)
    net.requires_grad_(False)
    return net.to(torch.device('cuda:0'))


class Packer:
    """The pack entry points of one network, through ctypes, into buffers the caller pre-fills."""

    def __init__(self, net):
        from nerfail_amd import _lib, _train
        self.L, self.lib, self.net = _lib, _lib.load(), net
        self.keep = []
        self.mp = net._mlp_params(self.keep)
        self.keep += [_lib.f32c(p) for p in _train.ordered_params(net)]
        self.mpT = _train._grads_struct(net, self.keep[-len(_train.ordered_params(net)):])
        a = (net.D, net.W, net._skip())
        lib = self.lib
        self.size = {'f32': 4 * lib.nerfail_mlp_packed_floats(*a), 'f32_T': 4 * lib.nerfail_mlp_packed_T_floats(*a),
                     'f16': lib.nerfail_mlp_f16_image_bytes(*a), 'f16_T': lib.nerfail_mlp_f16_image_T_bytes(*a),
                     'x3': lib.nerfail_mlp_packed_x3_bytes(*a)}
        assert all(self.size[k] > 0 for k in ('f32', 'f32_T', 'f16', 'f16_T')), self.size

    def buffers(self, fill=FILL):
        return {k: torch.full((n,), fill, dtype=torch.uint8, device='cuda:0') for k, n in self.size.items() if n}

    def pack(self, bufs, train=False):
        """Fills `bufs` in place; train=True: both f32 images from the one training launch."""
        L, lib, net, st = self.L, self.lib, self.net, self.L.stream()
        if train:
            L.check(lib.nerfail_mlp_pack_train(self.mp, L.dev(bufs['f32']), L.dev(bufs['f32_T']), st))
        else:
            L.check(lib.nerfail_mlp_pack(self.mp, L.dev(bufs['f32']), st))
            L.check(lib.nerfail_mlp_pack_T(self.mpT, L.dev(bufs['f32_T']), st))
        L.check(lib.nerfail_mlp_pack_f16(self.mp, L.dev(bufs['f16']), st))
        L.check(lib.nerfail_mlp_pack_f16_T(self.mpT, L.dev(bufs['f16_T']), st))
        if 'x3' in bufs:
            L.check(lib.nerfail_mlp_pack_x3(L.dev(bufs['f32']), net.D, net.W, net._skip(), L.dev(bufs['x3']), st))
        return bufs


def images(shape, fill=FILL, train=False):
    p = Packer(make_net(shape))
    return p.pack(p.buffers(fill), train)


def digests(bufs):
    return {k: hashlib.sha256(v.cpu().numpy().tobytes()).hexdigest() for k, v in bufs.items()}


def same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


@pytest.fixture(scope='module')
def packed():
    """name -> images of every shape, packed once over FILL and shared (read-only) by the tests."""
    return {shape_id(s): images(s) for s in SHAPES}


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_images_match_parent_digests(shape, packed):
    want = json.load(open(DIGESTS))[shape_id(shape)]
    got = digests(packed[shape_id(shape)])
    assert ('x3' in got) == (shape == (8, 256, 4))             # the bf16x3 image exists for the shipped shape only
    assert got == want


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_python_api_images(shape, packed):
    """net.packed() & co. allocate their own (uninitialised) buffers: equal to the pinned images on every written byte."""
    from nerfail_amd import _train
    ref = packed[shape_id(shape)]
    other = images(shape, fill=FILL ^ 0xFF)['f32']
    written = ref['f32'] == other                                       # unwritten bytes keep the two patterns
    assert 0 < int((~written).sum()) < written.numel() // 2
    net = make_net(shape)
    f32 = net.packed().view(torch.uint8)
    assert torch.equal(f32[written], ref['f32'][written])
    assert torch.equal(_train.packed_T(net).view(torch.uint8), ref['f32_T'])
    assert torch.equal(net.packed_f16(), ref['f16'])
    assert torch.equal(_train.packed_f16_T(net), ref['f16_T'])
    x3 = net.packed_x3()
    assert (x3 is None) == ('x3' not in ref)
    if x3 is not None:
        assert torch.equal(x3, ref['x3'])
    # the folded image against nerfail_mlp_pack_x3f called directly. The packer writes every byte, but it copies the bias
    # pieces and heads of the f32 image with their unwritten bytes: two direct packs, each from an f32 image and into a
    # buffer of one pattern, tell which bytes the weights decide - all but some of that copied block
    x3f = net.packed_x3f()
    assert (x3f is None) == (shape != (8, 256, 4))
    if x3f is not None:
        from nerfail_amd import _lib
        lib, a = _lib.load(), (net.D, net.W, net._skip())
        n, composed = lib.nerfail_mlp_packed_x3f_bytes(*a), 4 * lib.nerfail_mlp_x3f_composed_floats(*a)
        consts = 4 * ((net.D + 2) * net.W + 512 + 512)                  # bias pieces, alpha head, rgb head (mlp_layout.h)
        direct = []
        for fill, src in ((FILL, ref['f32']), (FILL ^ 0xFF, other)):
            direct.append(torch.full((n,), fill, dtype=torch.uint8, device='cuda:0'))
            _lib.check(lib.nerfail_mlp_pack_x3f(_lib.dev(src), *a, _lib.dev(direct[-1]), _lib.stream()))
        decided = direct[0] == direct[1]
        assert bool(decided[:n - composed - consts].all()) and bool(decided[n - composed:].all())
        assert x3f.dtype == torch.uint8 and x3f.numel() == n and torch.equal(x3f[decided], direct[0][decided])
    # the one training launch on a fresh, identically initialised net: the same pair
    both, bothT = _train.packed_both(make_net(shape))
    assert torch.equal(both.view(torch.uint8)[written], f32[written])
    assert torch.equal(bothT.view(torch.uint8), ref['f32_T'])


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES, ids=shape_id)
def test_pack_train_equals_the_two_packers(shape, packed):
    """nerfail_mlp_pack_train into pre-filled buffers == (nerfail_mlp_pack, nerfail_mlp_pack_T), unwritten bytes included."""
    assert same(images(shape, train=True), packed[shape_id(shape)])


@pytest.mark.gpu
def test_launches_are_independent(packed):
    """Packing twice into the same buffers, and A, B, A through the table-driven kernels, changes nothing."""
    A, B = SHAPES[1], SHAPES[3]
    pa = Packer(make_net(A))
    bufs = pa.pack(pa.buffers())
    first = {k: v.clone() for k, v in bufs.items()}
    assert same(first, packed[shape_id(A)])
    assert same(pa.pack(bufs), first)                                   # twice into the same buffers
    pb = Packer(make_net(B))
    assert same(pb.pack(pb.buffers()), packed[shape_id(B)])
    assert same(pa.pack(pa.buffers()), first)                           # A after B
    assert same(pa.pack(pa.buffers(), train=True), first)


if __name__ == '__main__':
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(json.dumps({shape_id(s): digests(images(s)) for s in SHAPES}, indent=1, sort_keys=True))
