"""Native (nerfail_amd.MyModel.MyCNN, csrc/cnn.hip) vs stock PyTorch (MIOpen) MyCNN victim, in one session on one GPU:
forward and forward + input backward at B = 8, 800x800; the NeRFail-S end-to-end iteration and the DeepFool inner loop with
each victim (the legs of bench_sections.attack_bench). Prints one JSON object. Usage: python tools/victim_cnn_bench.py [--out F]

--multi: only the legs of the multi-right-hand-side backward (nerfail_cnn_bwd_data_multi), three rounds with the arms
alternated inside each round: the native backward of 8 one-hot rows of one 800x800 forward as eight cnn_bwd_data calls and as
one cnn_bwd_data_multi call, the single backward at B = 8 beside them (the same MFMA work), and the DeepFool inner loop with
the MIOpen victim, the native victim forced to one backward per class (batched_classifier_backward = False) and the native
victim on the automatic setting.

--train: one model_train.py-shaped step (forward, cross-entropy, backward, torch.optim.SGD(lr=1e-3, momentum=0.9) step) at
B = 16 and B = 8, 800x800: MyCNN(8, trainable=True) (nerfail_cnn_bwd_weights) against the stock module on MIOpen, arms
alternated, three rounds. The number that matters is the ratio to the stock module in the same session.

--x3: the bf16x3 victim (MyCNN(8, precision='bf16x3'), csrc/cnn_x3.hip) against the exact native victim, the same weights, in
one session: forward at B = 8, forward + input backward at B = 8, the R = 8, B = 1 multi backward, and the NeRFail-S end-to-end
step. Per arm: HIP events around one call, 5 warm-up calls, then 20 timed calls with the two victims ALTERNATED call by call;
the median, and max - min as the spread. `faster_beyond_spread` says whether exact - x3 exceeds the sum of the two spreads."""
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


def deepfool_ms_per_iter(net, inputs):
    from nerfail_amd.deepfool import deepfool
    runs = []
    for _ in range(3):
        t = time.time()
        _, n_it, _, _, _ = deepfool(inputs, 1.0, net, num_classes=8, max_iter=6, m1=1e6, m2=30)
        torch.cuda.synchronize()
        runs.append((time.time() - t) / max(n_it, 1))
    return float(np.median(runs)) * 1e3


def multi_legs(dev, victims, rounds=3):
    """The arms of the multi-RHS backward, alternated inside each of `rounds` rounds; per arm the list of per-round values."""
    import nerfail_amd.ops as O
    from nerfail_amd.GaussNet import gauss_net
    from nerfail_amd.deepfool import deepfool
    m = victims['native']
    H, W = BS.H, BS.W
    x = torch.rand((8, 3, H, W), device=dev) * 255
    _, ws1, mk1 = O.cnn_fwd(m.packed(), x[:1].contiguous(), 8, True)
    _, ws8, mk8 = O.cnn_fwd(m.packed(), x, 8, True)
    eye = torch.eye(8, device=dev).reshape(8, 1, 8).contiguous()
    rows = [eye[k].contiguous() for k in range(8)]
    d8 = torch.eye(8, device=dev)

    def eight_single():
        for k in range(8):
            O.cnn_bwd_data(m.packed(), ws1, mk1, rows[k], H, W)

    def one_multi():
        O.cnn_bwd_data_multi(m.packed(), ws1, mk1, eye, H, W)

    def single_b8():
        O.cnn_bwd_data(m.packed(), ws8, mk8, d8, H, W)
    wi, ori, s_init = BS._attack_inputs(dev, 1, seed=0)
    inputs = (s_init, wi[:1], ori[:1])
    nets = {}
    for name, victim, mode in (('miopen', victims['miopen'], None), ('native_per_class', m, False), ('native_auto', m, None)):
        net = gauss_net(dev, 0.02, victim, 'my_model', epsilon=None)
        net.cache_ori_cla = False
        net.batched_classifier_backward = mode
        deepfool(inputs, 1.0, net, num_classes=8, max_iter=2, m1=1e6, m2=30)        # warm-up of every shape
        nets[name] = net
    torch.cuda.synchronize()
    out = {'backward_b1_8rhs_eight_cnn_bwd_data_ms': [], 'backward_b1_8rhs_one_cnn_bwd_data_multi_ms': [],
           'backward_b8_single_cnn_bwd_data_ms': []}
    out.update({'deepfool_inner_loop_%s_ms_per_iter' % k: [] for k in nets})
    for _ in range(rounds):
        out['backward_b1_8rhs_eight_cnn_bwd_data_ms'].append(timed(eight_single) * 1e3)
        out['backward_b1_8rhs_one_cnn_bwd_data_multi_ms'].append(timed(one_multi) * 1e3)
        out['backward_b8_single_cnn_bwd_data_ms'].append(timed(single_b8) * 1e3)
        for k, net in nets.items():
            out['deepfool_inner_loop_%s_ms_per_iter' % k].append(deepfool_ms_per_iter(net, inputs))
    out['ranges'] = {k: [min(v), max(v)] for k, v in out.items()}
    out['note'] = ('per arm: one value per round, arms alternated inside a round; backward legs: median of 5 blocks of 10 calls, '
                   'backward only, from one kept forward; deepfool legs: median of 3 runs of <= 6 iterations, one view')
    return out


def train_legs(dev, stock, rounds=3):
    from nerfail_amd.MyModel import MyCNN
    import torch.nn.functional as F
    native = MyCNN(8, trainable=True)
    native.load_state_dict(dict(zip(native.state_dict(), stock.state_dict().values())), strict=True)
    arms = {'miopen': stock.requires_grad_(True).train(), 'native': native.to(dev).train()}
    opts = {k: torch.optim.SGD(v.parameters(), lr=1e-3, momentum=0.9) for k, v in arms.items()}
    out = {}
    for B in (16, 8):
        x = torch.rand((B, 3, BS.H, BS.W), device=dev) * 255
        y = torch.randint(0, 8, (B,), device=dev)

        def step(k):
            opts[k].zero_grad()
            F.cross_entropy(arms[k](x), y).backward()
            opts[k].step()
        for k in arms:
            out['train_step_b%d_%s_ms' % (B, k)] = []
        for _ in range(rounds):
            for k in arms:
                out['train_step_b%d_%s_ms' % (B, k)].append(timed(lambda: step(k), reps=3, blocks=3) * 1e3)
        a, b = out['train_step_b%d_native_ms' % B], out['train_step_b%d_miopen_ms' % B]
        out['train_step_b%d_native_over_miopen' % B] = float(np.median(a) / np.median(b))
    out['note'] = 'per arm: one value per round, arms alternated inside a round; each value the median of 3 blocks of 3 steps'
    return out


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternated(arms, warm=5, n=20):
    """{arm: {'median_ms', 'spread_ms' (max - min), 'samples_ms'}}: every arm warmed, then n rounds of one call per arm."""
    for _ in range(warm):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(n):
        for k, fn in arms.items():
            t[k].append(event_ms(fn))
    return {k: {'median_ms': float(np.median(v)), 'spread_ms': float(max(v) - min(v)), 'samples_ms': [round(x, 4) for x in v]}
            for k, v in t.items()}


def x3_legs(dev, stock):
    from nerfail_amd.GaussNet import gauss_net
    from nerfail_amd.MyModel import MyCNN
    from nerfail_amd.attack import nerfail_s_step
    victims = {'exact': native_victim(stock)}
    x3 = MyCNN(8, precision='bf16x3')
    x3.load_state_dict(victims['exact'].state_dict(), strict=True)
    victims['bf16x3'] = x3.to(dev).requires_grad_(False).eval()
    H, W = BS.H, BS.W
    x8 = torch.rand((8, 3, H, W), device=dev) * 255
    eye = torch.eye(8, device=dev).reshape(8, 1, 8).contiguous()
    out = {}

    def fwd(v):
        def f():
            with torch.no_grad():
                v(x8)
        return f

    def fwd_bwd(v):
        def f():
            x = x8.clone().requires_grad_(True)
            v(x)[:, 4].sum().backward()
        return f

    def multi(v):
        _, ws, mk = v.forward_masks(x8[:1].contiguous())
        return lambda: v.backward_data(ws, mk, eye, H, W)
    wi, ori, s_init = BS._attack_inputs(dev, 8, seed=0)
    ori_u8 = ori.to(torch.uint8)
    label = torch.tensor(4, device=dev)
    ids = [('victim-bench', b) for b in range(8)]

    def step(v):
        net = gauss_net(dev, 0.02, v, 'my_model', epsilon=None)
        s = [s_init.clone()]

        def f():
            s[0] = nerfail_s_step(net, s[0], s_init, wi, ori_u8, label, 2.0, 32.0, False, view_ids=ids)[0]
        return f
    for leg, make in (('forward_b8', fwd), ('forward_input_backward_b8', fwd_bwd), ('multi_backward_r8_b1', multi),
                      ('nerfail_s_end_to_end_b8', step)):
        r = alternated({k: make(v) for k, v in victims.items()})
        e, b = r['exact'], r['bf16x3']
        out[leg] = {'exact': e, 'bf16x3': b, 'exact_over_bf16x3': e['median_ms'] / b['median_ms'],
                    'faster_beyond_spread': bool(e['median_ms'] - b['median_ms'] > e['spread_ms'] + b['spread_ms'])}
    for k in ('exact', 'bf16x3'):
        out['nerfail_s_end_to_end_b8'][k]['iters_per_sec'] = 1e3 / out['nerfail_s_end_to_end_b8'][k]['median_ms']
    with torch.no_grad():                                       # faster and different is not faster: the two victims' logits
        a, b = victims['exact'](x8).double(), victims['bf16x3'](x8).double()
    out['logits_rel_l2_bf16x3_vs_exact'] = float((a - b).norm() / a.norm())
    out['note'] = ('HIP events around one call; 5 warm-up calls per arm, then 20 rounds of one call per arm (arms alternated); '
                   'median and max - min per arm; the same weights in both victims')
    return out


def main():
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    stock = BS.victim_cnn(8).to(dev).requires_grad_(False).eval()
    victims = {'miopen': stock, 'native': native_victim(stock)}
    res = {'device': torch.cuda.get_device_name(0), 'batch': 8, 'size': [BS.H, BS.W]}
    if '--x3' in sys.argv:
        res.update(x3_legs(dev, stock))
    elif '--train' in sys.argv:
        res['batch'] = [16, 8]
        res.update(train_legs(dev, stock))
    elif '--multi' in sys.argv:
        res.update(multi_legs(dev, victims))
    else:
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
