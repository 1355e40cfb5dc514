"""numpy restatement of the bf16x3 arithmetic of the MyCNN victim (nerfail_amd/csrc/bf16_split.h, cnn_x3.hip) and of the
bf16x3 weight image (include/nerfail_hip.h, nerfail_cnn_pack_x3; layout in csrc/cnn_layout.h). numpy only, no GPU:
tests/test_cnn_x3_ref.py pins its properties, tests/test_hip_cnn_x3_kernels.py holds the device image to it bit for bit."""
import numpy as np

import cnn_ref as R

# the tiles of conv_x3_kernel: those of the exact kernel (forward 8 x 8 pooled cells, backward 8 rows x 32 columns of stage
# input), so cnn_ref.size_coverage names every residue that matters; the cases of the x3 GPU tests
CASES = [(767, 767, 1, 'c'), (783, 785, 1, 'n'), (766, 893, 3, 'cnc')]


def bf16_rne(x):
    """f32 -> the nearest bf16 (ties to even on the upper 16 bits), returned as f32; NaN -> NaN."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32)
    return np.where(np.isnan(x), np.float32(np.nan), r.view(np.float32))


def split3(x):
    """The three pieces [3, ...] (f32 values whose lower 16 bits are 0) of x = x0 + x1 + x2 + r: each piece is the bf16
    nearest to what is left, each subtraction is exact in f32."""
    rest = np.ascontiguousarray(x, np.float32)
    out = []
    with np.errstate(invalid='ignore', over='ignore'):
        for _ in range(3):
            p = bf16_rne(rest)
            out.append(p)
            rest = (rest - p).astype(np.float32)
    return np.stack(out)


def bf16_bits(p):
    """uint16 bit patterns of pieces made by bf16_rne."""
    return (np.ascontiguousarray(p, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _regions(C):
    """{(s, 'fwd' | 'bwd'): (offset, NC, KC)} of stages s = 1..6 in the f32 image of cnn_ref.pack_image."""
    out, o = {}, 0

    def up4(n):
        return (n + 3) // 4 * 4
    for s in range(R.STAGES):
        ci, co = R.CHANS[s], R.CHANS[s + 1]
        nf = co * 10 * 4 if s == 0 else co * 9 * ci
        if s > 0:
            out[(s, 'fwd')] = (o, co, ci)
        o += up4(nf) + up4(co)
        if s > 0:
            out[(s, 'bwd')] = (o, ci, co)
            o += up4(ci * 9 * co)
    return out


def x3_image(sd, C):
    """The bf16x3 image as uint8 bytes, from the f32 image: for s = 1..6 the forward then the backward image, each
    [KC / 16 slices][NC rows][9 taps][3 planes][16 channels] bf16 of the f32 region [NC][9][KC]."""
    img, _ = R.pack_image(sd, C)
    parts = []
    for s in range(1, R.STAGES):
        for d in ('fwd', 'bwd'):
            o, NC, KC = _regions(C)[(s, d)]
            w = img[o:o + NC * 9 * KC].reshape(NC, 9, KC)
            bits = bf16_bits(split3(w)).reshape(3, NC, 9, KC // 16, 16)
            parts.append(np.ascontiguousarray(np.transpose(bits, (3, 1, 2, 0, 4))).reshape(-1))
    return np.concatenate(parts).view(np.uint8)


def x3_bytes():
    return sum(2 * R.CHANS[s] * R.CHANS[s + 1] * 9 * 3 * 2 for s in range(1, R.STAGES))
