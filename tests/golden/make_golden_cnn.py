"""Generate tests/golden/g23_mycnn.npz by RUNNING THE REFERENCE's classifier (model/MyModel.py) on CPU.

Run in the build container only (needs the reference checkout; NERFAIL_REFERENCE overrides its location):
    python tests/golden/make_golden_cnn.py
The reference MyCNN is imported as make_golden.py imports the reference's modules; weights and the two 800x800 images come
from tests/cnn_inputs.py (seeds), so the fixture holds seeds, checksums and results only: logits and the CE(label 4) input
gradient summaries, each in float32 and float64 (the reference's own rounding spread)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get('NERFAIL_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)

import cnn_inputs as CI  # noqa: E402
from model.MyModel import MyCNN  # noqa: E402  (reference)

WEIGHT_SEED, IMAGE_SEEDS, LABEL = 23, (2301, 2302), 4


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    sd = CI.state_dict(WEIGHT_SEED)
    m = MyCNN(24)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    m.eval()
    imgs, edges = zip(*[CI.cold_tail_image(s) for s in IMAGE_SEEDS])
    x = np.stack(imgs)
    out = {'keys': np.array(list(m.state_dict().keys())),
           'shapes': np.array([list(v.shape) + [0] * (4 - v.dim()) for v in m.state_dict().values()], np.int64),
           'weight_seed': np.int64(WEIGHT_SEED), 'image_seeds': np.array(IMAGE_SEEDS, np.int64), 'label': np.int64(LABEL),
           'weight_sums': np.array([float(np.asarray(sd[k], np.float64).sum()) for k in sd]),
           'image_sums': np.array([float(np.asarray(i, np.float64).sum()) for i in imgs]), 'edges': np.array(edges, np.int64)}
    for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
        mm = m.to(dt)
        xt = torch.from_numpy(x).to(dt).requires_grad_(True)
        logits = mm(xt)
        loss = torch.nn.functional.cross_entropy(logits, torch.full((len(imgs),), LABEL), reduction='sum')
        loss.backward()
        g = xt.grad.detach().double().numpy()
        out['logits_' + tag] = logits.detach().double().numpy()
        crops, blocks, norms = zip(*[CI.summaries(g[i], edges[i]) for i in range(len(imgs))])
        out['crop_' + tag], out['blocks_' + tag], out['norm_' + tag] = np.stack(crops), np.stack(blocks), np.array(norms)
        print(tag, 'logits', out['logits_' + tag][:, :4], 'grad norms', out['norm_' + tag])
    for k in ('logits', 'crop', 'blocks', 'norm'):
        a, b = out[k + '_f32'], out[k + '_f64']
        print('%-7s fp32-vs-fp64 rel L2 %.2e' % (k, np.linalg.norm(a - b) / np.linalg.norm(b)))
    path = os.path.join(ROOT, 'tests', 'golden', 'g23_mycnn.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
