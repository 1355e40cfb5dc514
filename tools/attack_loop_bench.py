"""The NeRFail-S loops in one session at cfg5's shape: 800x800, P = 3 (1.92 M table rows), `--views` (default 100) resident
views named by id, batches of 8 with a 4-view tail, the stand-in 800x800 victim CNN, beta = 0. Three arms, alternated
`--rounds` times (default 3), each run `--epochs` (default 2) attack epochs:

  a  the AS:278-431 loop as a user writes it by hand over the step's parts (attack_forward, CE, backward, fused gather
     backward + sign step - what nerfail_s_step runs on one rank), with the reference's five .item() reads per batch
     (AS:325-344), the epoch means and the best-tensor rule decided on the host;
  b  attack.nerfail_s (statistics, rule and best tensor on the device, one host read per epoch). Its export epoch is given
     no batches (export_batches=[]), so that the run is the same attack steps as the other arms and is divided by the same
     number of steps; everything nerfail_s adds to them - per-batch statistics kernels, epoch close, conditional copy, the
     read per epoch - is inside the time;
  c  attack.nerfail_s_loop, the loop without any statistics - the figure b is held against: b must not be slower than c by
     more than c's own run-to-run spread in this session.

Per arm and run: wall ms per batch step (device synchronised before and after the run). No speed-up is claimed in advance;
the numbers and their spread are the result. Also times nerfail_img_sqerr alone at this shape (8 views, uint8 images). Prints one
JSON object; --out F also writes it to F."""
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

BATCH, LABEL, A, EPS = 8, 4, 2., 32.


def opt_arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def scene(dev, n_views):
    from nerfail_amd.GaussNet import gauss_net, register_view
    wi, ori, s_init = BS._attack_inputs(dev, n_views, seed=40)
    Ns = s_init.numel() // 4
    ori8 = ori.to(torch.uint8)
    for v in range(n_views):
        register_view(('bench', v), Ns, weight_and_index=wi[v], ori_img=ori8[v])          # resident: map, uint8 image, inverted index
    del wi
    torch.manual_seed(0)
    victim = BS.victim_cnn(8).to(dev).requires_grad_(False).eval()
    net = gauss_net(dev, 0.02, victim, 'my_model', epsilon=None)
    batches = [(None, None, [('bench', v) for v in range(b, min(b + BATCH, n_views))]) for b in range(0, n_views, BATCH)]
    return net, s_init, batches


def hand_written(net, s_init, batches, epochs, targeted=False):
    """AS:278-431 by hand, five host reads per batch."""
    from nerfail_amd.GaussNet import hot_backward_rgb_step
    criterion = torch.nn.CrossEntropyLoss()
    mse = torch.nn.MSELoss()
    lab = torch.tensor(LABEL, device=s_init.device)
    s, best, best_acc = s_init, s_init.clone(), (0 if targeted else 10000)
    n_views = sum(len(b[2]) for b in batches)
    for epoch in range(epochs):
        running_loss = attack_loss = attack_img_loss = 0.0
        running_corrects = attack_corrects = 0
        for wi, ori, vids in batches:
            xr, cla, ori_cla, views, aux = net.attack_forward(s, wi, ori, vids)
            lab_r = lab.broadcast_to([cla.shape[0]])
            B = cla.shape[0]
            running_loss += criterion(ori_cla, lab_r).item() * B                          # AS:325
            running_corrects += torch.sum(torch.max(ori_cla, 1)[1] == lab_r).item()     # AS:326 (read at AS:406)
            ae_loss = criterion(cla, lab_r)
            attack_loss += ae_loss.item() * B                                             # AS:339
            attack_img_loss += mse(xr.detach(), views.ori_float()).item() * B             # AS:341
            attack_corrects += torch.sum(torch.max(cla, 1)[1] == lab_r).item()           # AS:344
            ae_loss.backward()
            s = hot_backward_rgb_step(aux, xr.grad, views, s, s_init, A, EPS, targeted).view(s_init.shape)
        acc = attack_corrects / n_views
        net.epsilon_3d_zero()
        if (acc >= best_acc) if targeted else (acc <= best_acc):                          # AS:422-431
            best_acc, best = acc, s.clone().detach()
    return best


def sqerr_alone(dev, vids, s_init, calls=50):
    """nerfail_img_sqerr on one 8-view batch (float x_rgba, resident uint8 images), `calls` launches between two events."""
    from nerfail_amd import _lib
    from nerfail_amd.GaussNet import resolve_views
    views = resolve_views(s_init, None, None, vids)
    x = torch.rand((views.B, views.H, views.W, 4), device=dev) * 255.
    lib = _lib.load()
    row = torch.zeros(_lib.ATTACK_ROW_FLOATS, device=dev)
    scratch = torch.empty(lib.nerfail_img_sqerr_scratch_bytes() // 8, dtype=torch.float64, device=dev)
    table = (_lib.c_p * views.B)(*[o.data_ptr() for o in views.ori])

    def call():
        _lib.check(lib.nerfail_img_sqerr(_lib.dev(x), table, views.B, views.P, int(views.ori_u8), _lib.c_p(scratch.data_ptr()), _lib.dev(row),
                                         _lib.stream()))
    for _ in range(5):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        call()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / calls
    nbytes = views.B * views.P * (16 + (4 if views.ori_u8 else 16))
    return {'us_per_call': us, 'bytes_per_call': nbytes, 'GBps': nbytes / us * 1e-3,
            'note': 'two launches per call (partials + finish); the same %d MB are read by every call and fit the 256 MB last-level '
                    'cache, so this is not an HBM figure' % (nbytes // 1000000)}


def timed(fn, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def main():
    from nerfail_amd.attack import nerfail_s, nerfail_s_loop
    n_views, epochs, rounds = opt_arg('--views', 100), opt_arg('--epochs', 2), opt_arg('--rounds', 3)
    dev = torch.device('cuda:0')
    net, s_init, batches = scene(dev, n_views)
    steps = epochs * len(batches)
    lab = torch.tensor(LABEL, device=dev)
    arms = {'a_hand_written_five_item_reads': (lambda: hand_written(net, s_init, batches, epochs), steps),
            'b_nerfail_s': (lambda: nerfail_s(net, s_init, batches, LABEL, epochs + 1, A, EPS, False, 0., export_batches=[], log=None), steps),
            'c_nerfail_s_loop': (lambda: nerfail_s_loop(net, s_init, s_init, batches, lab, epochs, A, EPS, False), steps)}
    for fn, _ in arms.values():                                     # warm-up of every arm: MIOpen plans, logit cache, allocator
        fn()
    runs = {k: [] for k in arms}
    for r in range(rounds):
        for k, (fn, n) in arms.items():
            runs[k].append(timed(fn, n))
            print('round %d %s %.3f ms per batch step' % (r, k, runs[k][-1]), file=sys.stderr, flush=True)
    res = {'device': torch.cuda.get_device_name(0), 'rounds': rounds, 'epochs_per_run': epochs,
           'shape': '800x800, P=3, %d resident views, batches of %d (tail %d), stand-in victim CNN, beta 0' % (n_views, BATCH, len(batches[-1][2]))}
    for k in arms:
        res[k] = {'ms_per_batch_step': runs[k], 'median': float(np.median(runs[k])), 'spread': float(max(runs[k]) - min(runs[k]))}
    res['img_sqerr_alone'] = sqerr_alone(dev, batches[0][2], s_init)
    a, b, c = (res[k]['median'] for k in arms)
    res['a_over_b'] = a / b
    res['b_minus_c_ms'] = b - c
    res['b_not_slower_than_c_beyond_its_spread'] = bool(b - c <= res['c_nerfail_s_loop']['spread'])
    res['note'] = ('wall ms per batch step of a whole run, device synchronised before and after; arms alternated inside a round; every arm '
                   'runs the same attack steps (arm b with an empty export epoch); spread = max - min over the rounds')
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
