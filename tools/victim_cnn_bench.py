"""Native (nerfail_amd.MyModel.MyCNN, csrc/cnn.hip) vs stock PyTorch (MIOpen) MyCNN victim, in one session on one GPU:
forward and forward + input backward at B = 8, 800x800; the NeRFail-S end-to-end iteration and the DeepFool inner loop with
each victim (the legs of bench_sections.attack_bench). Prints one JSON object. Usage: python tools/victim_cnn_bench.py [--out F]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_sections as BS  # noqa: E402

BS._heavy_imports()

FWD_GFLOP = 20.78            # one 800x800 image, forward (2 x 10.39 G MAC)
PEAK_TF = 157.3              # f32 MFMA


def timed(fn, reps=10, blocks=5):
    fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(blocks):
        t = time.time()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        per.append((time.time() - t) / reps)
    return float(np.median(per))


def native_victim(stock):
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(8)
    sd = dict(zip([k for k in m.state_dict()], stock.state_dict().values()))
    m.load_state_dict(sd, strict=True)
    return m.to(stock[0].weight.device).requires_grad_(False).eval()


def classifier_legs(dev, victims, B=8):
    x0 = torch.rand((B, 3, BS.H, BS.W), device=dev) * 255
    out = {}
    for name, v in victims.items():
        def fwd():
            with torch.no_grad():
                v(x0)

        def fwd_bwd():
            x = x0.clone().requires_grad_(True)
            v(x)[:, 4].sum().backward()
        for leg, fn, gflop in (('forward', fwd, FWD_GFLOP * B), ('forward_input_backward', fwd_bwd, 2 * FWD_GFLOP * B)):
            dt = timed(fn)
            out['%s_%s' % (name, leg)] = {'ms': dt * 1e3, 'tflops': gflop / dt / 1e3, 'frac_f32_mfma_peak': gflop / dt / 1e3 / PEAK_TF}
    return out


def attack_legs(dev, victims, iters=5):
    from nerfail_amd.GaussNet import gauss_net
    from nerfail_amd.attack import nerfail_s_step
    from nerfail_amd.deepfool import deepfool
    wi, ori, s_init = BS._attack_inputs(dev, 8, seed=0)
    ori_u8 = ori.to(torch.uint8)
    label = torch.tensor(4, device=dev)
    ids = [('victim-bench', b) for b in range(8)]
    out = {}
    for name, v in victims.items():
        net = gauss_net(dev, 0.02, v, 'my_model', epsilon=None)
        net.cache_ori_cla = None
        s = [s_init.clone()]

        def step():
            s[0] = nerfail_s_step(net, s[0], s_init, wi, ori_u8, label, 2.0, 32.0, False, view_ids=ids)[0]
        dt = timed(step, reps=iters)
        out['%s_nerfail_s_end_to_end' % name] = {'ms_per_iter': dt * 1e3, 'iters_per_sec': 1 / dt,
                                                 'note': 'default settings, views named by id (original logits cached)'}
        net.cache_ori_cla = False
        deepfool((s_init, wi[:1], ori[:1]), 1.0, net, num_classes=8, max_iter=2, m1=1e6, m2=30)
        torch.cuda.synchronize()
        runs = []
        for _ in range(3):
            t = time.time()
            _, n_it, _, _, _ = deepfool((s_init, wi[:1], ori[:1]), 1.0, net, num_classes=8, max_iter=6, m1=1e6, m2=30)
            torch.cuda.synchronize()
            runs.append((time.time() - t) / max(n_it, 1))
        dt = float(np.median(runs))
        out['%s_deepfool_inner_loop' % name] = {'ms_per_iter': dt * 1e3, 'iters_per_sec': 1 / dt}
    return out


def main():
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    stock = BS.victim_cnn(8).to(dev).requires_grad_(False).eval()
    victims = {'miopen': stock, 'native': native_victim(stock)}
    res = {'device': torch.cuda.get_device_name(0), 'batch': 8, 'size': [BS.H, BS.W]}
    res.update(classifier_legs(dev, victims))
    if '--classifier-only' not in sys.argv:
        res.update(attack_legs(dev, victims))
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
