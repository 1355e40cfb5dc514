#!/usr/bin/env python3
"""Attack evaluation (nerfail_amd.model_test.evaluate_views) against the same measurement written with stock torch ops.

    python tools/eval_bench.py [--out FILE]

Shape: 8 resident uint8 BGRA views of 800x800 (the originals), 8 float32 [800,800,4] attacked images (x_rgba of gauss_net, not
rounded), the native MyCNN with 8 classes. Arm `fused`: evaluate_views - one nerfail_eval_view_metrics pass per batch (distances
and the classifier input), MyCNN, nerfail_eval_logit_stats, nerfail_eval_fold, one host read of the record. Arm `stock`:
model_test.py:237-299 as a user would port it to the device - per view the white background with torch.where, abs / max / sum /
min / dist / count_nonzero, get_psnr, the same MyCNN, CrossEntropyLoss, and the reference's host reads (.item(), int(preds),
rmse == 0). Both arms are timed with events over the whole evaluation, median of 20 after 5 warm-up runs.

`metrics_kernel`: nerfail_eval_view_metrics alone (both launches) on the same shape, cycling through 4 sets of images (656 MB
in all) so that no call finds its images in the 256 MB last-level cache: bytes moved / time is an HBM figure, set against the
6.3 TB/s a streaming kernel achieves and the compositing scan's 0.65-0.69 of the 8 TB/s peak. Prints one
JSON line."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

VIEWS, SIDE, LABEL, CLASSES, WARMUP, RUNS = 8, 800, 4, 8, 5, 20


def inputs(dev, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:SIDE, 0:SIDE]
    inside = ((yy - SIDE / 2) ** 2 + (xx - SIDE / 2) ** 2) <= (0.375 * SIDE) ** 2
    ori = rs.randint(0, 256, size=(VIEWS, SIDE, SIDE, 4)).astype(np.uint8)
    ori[..., 3] = np.where(inside, 255, 0)[None]
    att = ori.astype(np.float32)
    att[..., :3] += rs.uniform(-32, 32, size=att[..., :3].shape).astype(np.float32) * inside[None, ..., None]
    return torch.from_numpy(att).to(dev), [torch.from_numpy(o).to(dev) for o in ori]


def stock(model, attacked, originals, label, dev):
    """MT:226-348 on the device, batch size 1, with the reference's host reads."""
    from nerfail_amd.model_test import get_psnr
    criterion = torch.nn.CrossEntropyLoss()
    labels = torch.tensor([label], device=dev)
    e, hist = None, {}
    running_loss, running_corrects = 0.0, 0
    with torch.no_grad():
        for a, o in zip(attacked, originals):
            inputs_ = a.transpose(1, 2).transpose(0, 1).unsqueeze(0)
            ori_img = o.to(torch.float).transpose(1, 2).transpose(0, 1).unsqueeze(0)
            inputs_ = torch.where(inputs_[:, 3:4].broadcast_to(1, 3, SIDE, SIDE) > 0, inputs_[:, :3], torch.ones_like(inputs_[:, :3]) * 255)
            ori_img = torch.where(ori_img[:, 3:4].broadcast_to(1, 3, SIDE, SIDE) > 0, ori_img[:, :3], torch.ones_like(ori_img[:, :3]) * 255)
            dist_mask = torch.abs(inputs_ - ori_img)
            e_max, e_min = torch.max(dist_mask), torch.min(dist_mask)
            e_avg = torch.sum(dist_mask) / dist_mask.numel()
            d_l2 = torch.dist(inputs_, ori_img, p=2)
            d_l0 = torch.count_nonzero(dist_mask)
            psnr = get_psnr(inputs_, ori_img)
            if e is None:
                e = {"e_max": e_max, "e_avg": e_avg, "e_min": e_min, "d_l2": d_l2, "d_l0": d_l0, "psnr_list": [psnr]}
            else:
                e["e_max"] = torch.max(torch.stack([e["e_max"], e_max]))
                e["e_avg"] += e_avg
                e["e_min"] = torch.min(torch.stack([e["e_min"], e_min]))
                e["d_l2"] += d_l2
                e["d_l0"] += d_l0
                e["psnr_list"].append(psnr)
            outputs = model(inputs_.contiguous())
            loss = criterion(outputs, labels)
            _, preds = torch.max(outputs, 1)
            running_loss += loss.item()
            running_corrects += torch.sum(preds == labels.data)
            hist[str(int(preds))] = hist.get(str(int(preds)), 0) + 1
    n = len(attacked)
    return {"e min": float(e["e_min"]), "e avg": float(e["e_avg"] / n), "e max": float(e["e_max"]), "d l2 norm": float(e["d_l2"] / n),
            "d l0 norm": float(e["d_l0"] / n), "psnr min": min(e["psnr_list"]), "psnr max": max(e["psnr_list"]),
            "psnr avg": sum(e["psnr_list"]) / n, "loss": running_loss / n, "acc": float(running_corrects) / n, "hist": hist}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def arm(fn):
    for _ in range(WARMUP):
        fn()
    ms = [event_ms(fn) for _ in range(RUNS)]
    return {'ms_median': float(np.median(ms)), 'ms_min': float(min(ms)), 'ms_max': float(max(ms))}


def metrics_kernel(dev):
    from nerfail_amd import _lib
    lib = _lib.load()
    sets = [inputs(dev, 100 + i) for i in range(4)]
    P = SIDE * SIDE
    scratch = torch.empty(lib.nerfail_eval_scratch_bytes() // 8, dtype=torch.float64, device=dev)
    rows = torch.empty((VIEWS, 6), dtype=torch.float64, device=dev)
    cla = [torch.empty((VIEWS, 3, P), dtype=torch.float32, device=dev) for _ in sets]
    tabs = [((_lib.c_p * VIEWS)(*[a[v].data_ptr() for v in range(VIEWS)]), (_lib.c_p * VIEWS)(*[o.data_ptr() for o in os_]))
            for a, os_ in sets]

    def call(i):
        _lib.check(lib.nerfail_eval_view_metrics(tabs[i][0], _lib.EVAL_F32C4, tabs[i][1], _lib.EVAL_U8C4, VIEWS, P, _lib.c_p(scratch.data_ptr()),
                                                 _lib.c_p(rows.data_ptr()), _lib.c_p(cla[i].data_ptr()), _lib.stream()))
    for i in range(8):
        call(i % 4)
    calls = 40
    ms = []
    for _ in range(RUNS):
        ms.append(event_ms(lambda: [call(i % 4) for i in range(calls)]) / calls)
    us = float(np.median(ms)) * 1e3
    nbytes = VIEWS * P * (16 + 4 + 12)
    return {'us_per_call': us, 'bytes_per_call': nbytes, 'GBps': nbytes / us * 1e-3, 'of_hbm_peak_8TBps': nbytes / us * 1e-3 / 8000.,
            'of_achievable_6p3TBps': nbytes / us * 1e-3 / 6300.,
            'note': 'both launches (partials + finish); reads 16 B + 4 B and writes 12 B per pixel; 4 image sets in rotation, 656 MB, so '
                    'no call is served from the 256 MB last-level cache'}


def main():
    import cnn_inputs as CI
    from nerfail_amd import model_test as MT
    from nerfail_amd.MyModel import MyCNN
    dev = torch.device('cuda:0')
    m = MyCNN(CLASSES)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(31, CLASSES).items()})
    m = m.to(dev).requires_grad_(False).eval()
    attacked, originals = inputs(dev, 0)
    a_list = list(attacked.unbind(0))
    fused = MT.evaluate_views(m, 'my_model', a_list, originals, LABEL, num_classes=CLASSES)
    st = stock(m, a_list, originals, LABEL, dev)
    agree = {k: (fused[k], st[k]) for k in ('e min', 'e avg', 'e max', 'd l2 norm', 'd l0 norm', 'psnr min', 'psnr max', 'psnr avg', 'loss', 'acc')}
    for k, (f, s) in agree.items():
        assert math.isclose(f, s, rel_tol=1e-4, abs_tol=1e-6), (k, f, s)          # the two arms measure the same thing
    res = {'device': torch.cuda.get_device_name(0), 'shape': '%d views %dx%d, attacked float32 RGBA, originals resident uint8 BGRA, native MyCNN(%d)'
           % (VIEWS, SIDE, SIDE, CLASSES), 'warmup': WARMUP, 'runs': RUNS,
           'command': 'python tools/eval_bench.py', 'commit': subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True,
                                                                              text=True).stdout.strip() or os.environ.get('NERFAIL_COMMIT', 'unknown')}
    res['fused'] = arm(lambda: MT.evaluate_views(m, 'my_model', a_list, originals, LABEL, num_classes=CLASSES))
    res['stock'] = arm(lambda: stock(m, a_list, originals, LABEL, dev))
    res['stock_over_fused'] = res['stock']['ms_median'] / res['fused']['ms_median']
    cnn = arm(lambda: m(torch.empty((VIEWS, 3, SIDE, SIDE), device=dev).fill_(128.)))
    res['mycnn_forward_alone_8_views'] = cnn
    res['metrics_kernel'] = metrics_kernel(dev)
    res['values_fused_vs_stock'] = agree
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
