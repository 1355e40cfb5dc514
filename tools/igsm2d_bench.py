"""attack.igsm_2d against the loop the reference writes, and its two streaming kernels against the chip, in one session at the
reference's shape: 800x800 BGRA views, batches of 4, the native MyCNN victim with 8 classes. Event-timed, median of `--reps`
(default 20) after `--warmup` (default 5), the arms alternated call by call, max - min of each arm reported as its spread.

  1  one attack step of attack.igsm_2d per 4-view batch, on both classifier paths (native=True: cnn_fwd, cls_ce, cnn_bwd_data
     between the two u2d launches, no autograd graph; native=False: autograd through the same MyCNN). A call with 1 + K attack
     epochs minus a call with 1 attack epoch, over K = 4: what a call pays once (the clean logits, the export pass, allocations)
     is not in it; what every epoch pays (the close, the conditional copy of the best table, the host read of the record) is.
  2  the literal IG:289-379 loop body on the same module and device, in stock torch ops with the reference's seven .item()
     reads: universal_2D_net's forward (GN:356-385), CrossEntropyLoss twice, MSELoss, backward, sign, the two cat + max / min
     pairs, the index-put into the table. The dataset's item (MD:247-255, the white-background uint8 image) is prepared outside
     the timed region, as a DataLoader would have it ready.
  3  nerfail_u2d_fwd and nerfail_u2d_step alone over 40 views (a 307 MB table, 102 MB of images: larger than the 256 MB
     last-level cache), with the compulsory bytes of include/nerfail_hip.h per pixel and the achieved bytes per second.

No ratio is claimed in advance. Prints one JSON object; --out F also writes it to F (profiles/<round>_igsm2d_bench.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

H = W = 800
BATCH, K, CLASSES, LABEL, STREAM_VIEWS = 4, 4, 8, 4, 40


def opt_arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms, reps, warmup):
    """{name: [ms per rep]}: every rep runs each arm once, in turn."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    runs = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            runs[k].append(event_ms(fn))
    return runs


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'spread_ms': float(max(ms) - min(ms))}


def views(n, dev, seed=0):
    """uint8 BGRA [n,800,800,4]: random colours, alpha 255 inside a centred disc of radius 300."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    img = torch.randint(0, 256, (n, H, W, 4), dtype=torch.uint8, generator=g)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    inside = ((yy - H / 2 + .5) ** 2 + (xx - W / 2 + .5) ** 2) <= 300. ** 2
    img[..., 3] = torch.where(inside, 255, 0).to(torch.uint8)
    return img.to(dev)


def literal_step(net, table_all, init_all, index, ori_img, lab, a, epsilon, targeted):
    """IG:289-379 for one batch, as the reference writes it (beta = 0, IG:69)."""
    criterion, img_rgba_loss = torch.nn.CrossEntropyLoss(), torch.nn.MSELoss()
    t = table_all[index, :, :, :]
    t_init = init_all[index, :, :, :]
    t = t.clone().detach().requires_grad_(True)
    x, r, cla, ori_f, ori_cla = net(t, ori_img)
    lab_r = lab.broadcast_to([ori_cla.size()[0], ])
    loss = criterion(ori_cla, lab_r)
    _, preds = torch.max(ori_cla, 1)
    running_loss = loss.item() * len(ori_f)
    running_corrects = torch.sum(preds == lab_r)
    ae_loss = criterion(cla, lab_r)
    img_pixel_loss = img_rgba_loss(r, ori_f)
    _, ae_preds = torch.max(cla, 1)
    total_loss = (1 * ae_loss) + (0 * img_pixel_loss)
    stats = (ae_loss.item() * len(ori_f), (1 * ae_loss.item()) * len(ori_f), img_pixel_loss.item() * len(ori_f),
             (0 * img_pixel_loss.item()) * len(ori_f), total_loss.item() * len(ori_f), torch.sum(ae_preds == lab_r))
    total_loss.backward(retain_graph=True)
    if targeted:
        t2 = t - a * torch.sign(t.grad.data)
    else:
        t2 = t + a * torch.sign(t.grad.data)
    t_max, t_min = t_init + epsilon, t_init - epsilon
    t2 = torch.max(torch.cat([t2.unsqueeze(0), t_min.unsqueeze(0)], 0), dim=0)[0]
    t2 = torch.min(torch.cat([t2.unsqueeze(0), t_max.unsqueeze(0)], 0), dim=0)[0]
    table_all[index, :, :, :] = t2.clone().detach()
    return running_loss, running_corrects, stats


def main():
    from nerfail_amd import _lib
    from nerfail_amd.attack import igsm_2d
    from nerfail_amd.GaussNet import universal_2D_net
    from nerfail_amd.MyModel import MyCNN
    reps, warmup = opt_arg('--reps', 20), opt_arg('--warmup', 5)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    victim = MyCNN(CLASSES).to(dev).requires_grad_(False).eval()
    images = views(BATCH, dev)
    res = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'warmup': warmup,
           'shape': '%dx%d BGRA, batches of %d, native MyCNN (%d classes)' % (H, W, BATCH, CLASSES)}

    # ---- 1 + 2: the attack step, three ways
    net = universal_2D_net(dev, 0.02, victim, 'my_model')
    table_all = torch.zeros((BATCH, H, W, 3), device=dev)
    init_all = table_all.clone()
    index = torch.arange(BATCH, device=dev)
    ori_img = torch.where(images[..., 3:4] > 0, images[..., :3], torch.ones_like(images[..., :3]) * 255)      # MD:247-255
    lab = torch.tensor(LABEL, device=dev)
    arms = {}
    for name, native in (('native', True), ('general', False)):
        for ep in (1, 1 + K):
            arms['%s_%d' % (name, ep)] = lambda native=native, ep=ep: igsm_2d(victim, 'my_model', images, LABEL, ep + 1, 2., 32., False, BATCH,
                                                                              log=None, native=native)
    arms['literal'] = lambda: literal_step(net, table_all, init_all, index, ori_img, lab, 2., 32., False)
    runs = alternate(arms, reps, warmup)
    step = {k: summary(v) for k, v in runs.items()}
    for name in ('native', 'general'):
        step['%s_step' % name] = summary([(b - a) / K for a, b in zip(runs['%s_1' % name], runs['%s_%d' % (name, 1 + K)])])
    res['attack_step'] = step
    lit, nat, gen = step['literal'], step['native_step'], step['general_step']
    res['literal_over_native'] = lit['median_ms'] / nat['median_ms']
    res['literal_over_general'] = lit['median_ms'] / gen['median_ms']
    res['native_faster_than_literal_beyond_its_spread'] = bool(lit['median_ms'] - nat['median_ms'] > lit['spread_ms'])

    # ---- 3: the two streams alone, over more than the last-level cache holds
    del arms, runs, net, table_all, init_all
    torch.cuda.empty_cache()
    lib = _lib.load()
    big = views(STREAM_VIEWS, dev, seed=1)
    P = H * W
    table = (torch.rand((STREAM_VIEWS, H, W, 3), device=dev) - 0.5) * 64.
    ix = torch.arange(STREAM_VIEWS, dtype=torch.int64, device=dev)
    x_rgb = torch.empty((STREAM_VIEWS, H, W, 3), device=dev)
    cls_in = torch.empty((STREAM_VIEWS, 3, H, W), device=dev)
    mask = torch.empty((STREAM_VIEWS, H, W), dtype=torch.uint8, device=dev)
    d = torch.randn((STREAM_VIEWS, 3, H, W), device=dev)
    p = lambda t: _lib.c_p(t.data_ptr())                                   # noqa: E731

    def fwd(with_x):
        _lib.check(lib.nerfail_u2d_fwd(p(big), _lib.EVAL_U8C4, STREAM_VIEWS, P, p(ix), STREAM_VIEWS, p(table), 0, p(x_rgb) if with_x else None,
                                       p(cls_in), p(mask), _lib.stream()))

    def stp():
        _lib.check(lib.nerfail_u2d_step(p(table), STREAM_VIEWS, P, p(ix), STREAM_VIEWS, p(d), p(mask), None, 2., 32., 0, _lib.stream()))
    fwd(True)
    runs = alternate({'u2d_fwd': lambda: fwd(False), 'u2d_fwd_with_x_rgb': lambda: fwd(True), 'u2d_step': stp}, reps, warmup)
    per_pixel = {'u2d_fwd': 4 + 12 + 12 + 1, 'u2d_fwd_with_x_rgb': 4 + 12 + 12 + 1 + 12, 'u2d_step': 12 + 1 + 12 + 12}
    streams = {}
    for k, v in runs.items():
        s = summary(v)
        nbytes = per_pixel[k] * P * STREAM_VIEWS
        s.update(bytes_per_pixel=per_pixel[k], bytes=nbytes, TB_per_s=nbytes / (s['median_ms'] * 1e-3) / 1e12)
        s['of_6.3_TB_per_s'] = s['TB_per_s'] / 6.3
        streams[k] = s
    res['streams'] = streams
    res['streams_shape'] = '%d views of %dx%d: table %.0f MB, images %.0f MB' % (STREAM_VIEWS, H, W, table.numel() * 4 / 1e6, big.numel() / 1e6)
    res['note'] = ('HIP events around each call, device idle before it; the arms alternate call by call; a step is (call with 5 attack '
                   'epochs - call with 1) / 4 of the same rep; spread = max - min over the reps; 6.3 TB/s is what a streaming kernel '
                   'reaches on this chip (README)')
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
