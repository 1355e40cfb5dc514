"""Seeded inputs of the MyCNN victim tests (tests/test_hip_cnn.py, tests/golden/make_golden_cnn.py): weights in the
reference's state_dict order and 800x800 cold-tail-like images, regenerated from seeds on both sides so that the fixture
stores seeds and checksums instead of the tensors."""
import numpy as np

CHANS = (3, 32, 64, 128, 256, 256, 128, 64)


def param_shapes(num_classes=24):
    """(name, shape) of MyCNN's parameters in state_dict order (model/MyModel.py:5-52)."""
    out = []
    for i in range(7):
        out += [('conv%d.weight' % (i + 1), (CHANS[i + 1], CHANS[i], 3, 3)), ('conv%d.bias' % (i + 1), (CHANS[i + 1],))]
    return out + [('fc1.weight', (512, 1024)), ('fc1.bias', (512,)), ('fc2.weight', (num_classes, 512)), ('fc2.bias', (num_classes,))]


def state_dict(seed, num_classes=24):
    """Weights uniform in +-1/sqrt(fan_in) of their layer, drawn in state_dict order from RandomState(seed)."""
    rs = np.random.RandomState(seed)
    sd = {}
    fan_in = 1
    for name, shape in param_shapes(num_classes):
        if name.endswith('weight'):
            fan_in = int(np.prod(shape[1:]))
        bound = 1.0 / np.sqrt(fan_in)
        sd[name] = rs.uniform(-bound, bound, size=shape).astype(np.float32)
    return sd


def cold_tail_image(seed, H=800, W=800):
    """[3,H,W] float32, integer valued: white (255) background - equal pool windows everywhere - and a textured object,
    an ellipse of colour gradients + noise, as gauss_net hands the classifier (white where alpha == 0, GN:121-157)."""
    rs = np.random.RandomState(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cy, cx = H * rs.uniform(0.4, 0.6), W * rs.uniform(0.4, 0.6)
    ry, rx = H * rs.uniform(0.2, 0.3), W * rs.uniform(0.2, 0.3)
    inside = ((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1.0
    img = np.full((3, H, W), 255.0)
    for c in range(3):
        base = 128 + 80 * np.sin(x / rs.uniform(20, 60) + rs.uniform(0, 6)) * np.cos(y / rs.uniform(20, 60))
        tex = np.clip(np.round(base + rs.normal(scale=20.0, size=(H, W))), 0, 255)
        img[c][inside] = tex[inside]
    return img.astype(np.float32), (int(cy), int(cx - rx))      # image, a point on the object's left edge


def edge_crop(g, edge, size=64):
    """size x size crop of a [3,H,W] gradient around the object edge point."""
    y0 = min(max(edge[0] - size // 2, 0), g.shape[1] - size)
    x0 = min(max(edge[1] - size // 2, 0), g.shape[2] - size)
    return g[:, y0:y0 + size, x0:x0 + size]


def block_sums(g, block=16):
    C, H, W = g.shape
    return g[:, :H // block * block, :W // block * block].reshape(C, H // block, block, W // block, block).sum((2, 4))


def summaries(g, edge):
    """(edge crop, 16x16 block sums, global L2 norm) of one image's input gradient, in float64."""
    g = np.asarray(g, np.float64)
    return edge_crop(g, edge), block_sums(g), np.sqrt((g * g).sum())
