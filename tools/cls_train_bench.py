#!/usr/bin/env python3
"""Victim training: ms per step of nerfail_amd.model_train.train_classifier against the literal loop of model_train.py:121-169
on the same trainable native MyCNN, the same device, the same session.

    python tools/cls_train_bench.py [--out FILE]

Shape: batch 16, 800x800 BGRA views, 8 classes (model_train.py's own configuration). Arm `product`: train_classifier on a
resident uint8 store - cls_batch, cnn_fwd, cls_ce, cnn_bwd_weights, MyCNN.sgd_step; no autograd graph, no host read inside the
epoch. Arm `literal`: MTR:121-169 as written - a DataLoader(shuffle=True, drop_last=True) over per-view float tensors on the
device (what MySimpleDataset(device='cuda') of the reference holds), optimizer.zero_grad(), the module's autograd forward,
nn.CrossEntropyLoss, torch.max, loss.backward(), torch.optim.SGD(lr=0.001, momentum=0.9).step(), loss.item() and the
running_corrects sum.

Both arms mark the start of every step with a device event; a step's time is the distance to the next mark, so it contains
everything between two steps (the batch assembly, the optimizer, the host waits). 5 warm-up steps, then the median of 20.
Every arm runs in a child process of its own under its own time limit, twice, alternating (product, literal, product,
literal): the distance between the two runs of ONE arm is the run-to-run spread a difference between the arms has to exceed
(other people's work shares the host). The step is ~1 TFLOP of convolution in both arms; what the product loop removes is
launches and host waits, not FLOPs - expect a small difference. Prints one JSON line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BATCH, SIDE, CLASSES, WARMUP, RUNS = 16, 800, 8, 5, 20
STEPS = WARMUP + RUNS + 1                     # marks: one more than intervals
CHILD_TIMEOUT = 300


def make_store(dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(20)
    n = STEPS * BATCH
    store = torch.randint(0, 256, (n, SIDE, SIDE, 4), dtype=torch.uint8, device=dev, generator=g)
    yy, xx = torch.meshgrid(torch.arange(SIDE, device=dev), torch.arange(SIDE, device=dev), indexing='ij')
    inside = ((yy - SIDE / 2) ** 2 + (xx - SIDE / 2) ** 2) <= (0.375 * SIDE) ** 2
    store[..., 3] = torch.where(inside, 255, 0).to(torch.uint8)[None]
    labels = torch.randint(0, CLASSES, (n,), dtype=torch.int32, device=dev, generator=g)
    return store, labels


def model(dev):
    import torch
    import cnn_inputs as CI
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(CLASSES, trainable=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(31, CLASSES).items()})
    return m.to(dev)


def intervals(marks):
    import numpy as np
    import torch
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])][WARMUP:WARMUP + RUNS]
    assert len(ms) == RUNS, len(ms)
    return {'ms_median': float(np.median(ms)), 'ms_min': float(min(ms)), 'ms_max': float(max(ms))}


def mark(marks):
    import torch
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    marks.append(e)


def product(dev):
    import torch
    from nerfail_amd import model_train as MT
    store, labels = make_store(dev)

    class Set:
        def __len__(self):
            return self.store.shape[0]
    train, val = Set(), Set()
    train.store, train.labels = store, labels
    val.store, val.labels = store[:BATCH], labels[:BATCH]
    marks = []

    class Marked(MT._Native):
        def train_step(self, x, lb, row):
            super().train_step(x, lb, row)
            mark(marks)                          # the end of a step = the start of the next one's batch assembly
    MT._Native = Marked
    m = model(dev)
    MT.train_classifier(m, train, val, num_classes=CLASSES, epochs=1, batch_size=BATCH, log=lambda s: None)
    return intervals(marks)


def literal(dev):
    import torch
    from torch import nn, optim
    store, labels = make_store(dev)
    f = store.to(torch.float32)
    views = [torch.where(v[..., 3:4] > 0, v[..., :3], torch.full_like(v[..., :3], 255.)).permute(2, 0, 1).contiguous() for v in f]   # MD:93-105
    del f
    host_labels = labels.tolist()

    class Views(torch.utils.data.Dataset):
        def __len__(self):
            return len(views)

        def __getitem__(self, i):
            return views[i], host_labels[i]
    loader = torch.utils.data.DataLoader(Views(), batch_size=BATCH, shuffle=True, num_workers=0, drop_last=True)
    m = model(dev)
    m.train()
    criterion = nn.CrossEntropyLoss()
    optimizer = optim.SGD(m.parameters(), lr=0.001, momentum=0.9)
    running_loss, running_corrects = 0.0, 0
    marks = []
    for inputs, lb in loader:                                            # MTR:121-169
        inputs = inputs.to(dev)
        lb = lb.to(dev)
        optimizer.zero_grad()
        with torch.set_grad_enabled(True):
            outputs = m(inputs)
            loss = criterion(outputs, lb)
            _, preds = torch.max(outputs, 1)
            loss.backward()
            optimizer.step()
        running_loss += loss.item() * inputs.size(0)
        running_corrects += torch.sum(preds == lb.data)
        mark(marks)
    return intervals(marks)


def child(which):
    import torch
    dev = torch.device('cuda:0')
    res = {'product': product, 'literal': literal}[which](dev)
    res['device'] = torch.cuda.get_device_name(0)
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    if '--child' in sys.argv:
        return child(sys.argv[sys.argv.index('--child') + 1])
    runs = {'product': [], 'literal': []}
    device = None
    for which in ('product', 'literal', 'product', 'literal'):          # alternating; each under its own time limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', which], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit('%s arm failed with status %d; nothing more is started' % (which, r.returncode))
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])
        device = out.pop('device')
        runs[which].append(out)
        print(which, out, file=sys.stderr, flush=True)
    med = {k: [r['ms_median'] for r in v] for k, v in runs.items()}
    mean = {k: sum(v) / len(v) for k, v in med.items()}
    spread = max(abs(v[0] - v[1]) / min(v) for v in med.values())
    res = {'device': device, 'shape': 'batch %d, %dx%d BGRA uint8 views, native trainable MyCNN(%d), SGD lr 0.001 momentum 0.9' % (BATCH, SIDE, SIDE, CLASSES),
           'warmup_steps': WARMUP, 'timed_steps': RUNS, 'command': 'python tools/cls_train_bench.py',
           'commit': subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip()
           or os.environ.get('NERFAIL_COMMIT', 'unknown'),
           'product': runs['product'], 'literal': runs['literal'], 'ms_per_step_product': mean['product'], 'ms_per_step_literal': mean['literal'],
           'literal_over_product': mean['literal'] / mean['product'], 'run_to_run_spread': spread,
           'spread_note': 'largest relative distance between the two runs of one arm (same code, same session, alternating with the other arm)',
           'product_not_slower_beyond_spread': bool(mean['product'] <= mean['literal'] * (1 + spread))}
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
