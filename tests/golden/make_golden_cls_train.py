"""Generate tests/golden/g26_cls_train.npz by RUNNING model_train.py:107-193's own calls on the reference's MyCNN, on the CPU.

Run in the build container only (needs the reference checkout; NERFAIL_REFERENCE overrides its location):
    python tests/golden/make_golden_cls_train.py [first_seed]
The reference's MySimpleDataset needs cv2 and torchvision, which the build container lacks, so the dataset is a list of the
tensors MD:93-105 builds (tests/cls_inputs.py: seeded BGRA views, white background from alpha) and the loop below issues
MTR's calls on it: nn.CrossEntropyLoss(), optim.SGD(lr=0.001, momentum=0.9), DataLoader(shuffle=True, drop_last=True) with a
seeded generator, running_loss += loss.item() * B, the division by len(dataset), the strict best rule, the save epochs.
The fixture holds seeds, each epoch's index order, every batch's logits, the per-epoch records and summaries of the
parameters - of a float32 and a float64 run (the reference's own rounding spread).

766 x 766, 8 classes, 5 train and 3 val views at batch 2 (each phase drops one view and still divides by 5 and 3), 3 epochs,
save_model_epochs = 2. A seed is accepted only if the two runs agree on every prediction, every evaluated view's top-two logit
margin is >= 1e-3 in both, and the best epoch is neither the first nor decided by a tie."""
import copy
import os
import sys

import numpy as np
import torch
from torch import nn, optim

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get('NERFAIL_REFERENCE', '/root/reference')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, REF)

import cnn_inputs as CI  # noqa: E402
import cls_inputs as XI  # noqa: E402
from model.MyModel import MyCNN  # noqa: E402  (reference)

EPOCHS, BATCH, SAVE_EPOCHS, LR, MOMENTUM = 3, 2, 2, 0.001, 0.9


class Views(torch.utils.data.Dataset):
    def __init__(self, x, labels):
        self.x, self.labels = x, [int(v) for v in labels]

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, i):
        return self.x[i], self.labels[i], i


def run(seed, dtype, train, val):
    """MTR:89-193 on the tensors of MD:93-105."""
    sd = CI.state_dict(seed, XI.NUM_CLASSES)
    model = MyCNN(XI.NUM_CLASSES)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.to(dtype)
    sets = {'train': Views(torch.from_numpy(XI.white_nchw(train[0])).to(dtype), train[1]),
            'val': Views(torch.from_numpy(XI.white_nchw(val[0])).to(dtype), val[1])}
    gens = {p: torch.Generator().manual_seed(seed * 2 + k) for k, p in enumerate(('train', 'val'))}
    loaders = {p: torch.utils.data.DataLoader(sets[p], batch_size=BATCH, shuffle=True, num_workers=0, drop_last=True, generator=gens[p])
               for p in ('train', 'val')}
    criterion = nn.CrossEntropyLoss()
    optimizer = optim.SGD(model.parameters(), lr=LR, momentum=MOMENTUM)
    best_wts, best_acc, best_epoch = copy.deepcopy(model.state_dict()), 0.0, -1
    out = {'order_train': [], 'order_val': [], 'logits_train': [], 'logits_val': [], 'loss': [], 'acc': [], 'taken': [],
           'batch_loss_train': [], 'batch_loss_val': [], 'saved': [], 'saved_sums': []}
    for epoch in range(EPOCHS):
        rec_loss, rec_acc = [], []
        for phase in ('train', 'val'):
            model.train() if phase == 'train' else model.eval()
            running_loss, running_corrects = 0.0, 0
            order, logits, losses = [], [], []
            for inputs, labels, idx in loaders[phase]:
                optimizer.zero_grad()
                with torch.set_grad_enabled(phase == 'train'):
                    outputs = model(inputs)
                    loss = criterion(outputs, labels)
                    _, preds = torch.max(outputs, 1)
                    if phase == 'train':
                        loss.backward()
                        optimizer.step()
                running_loss += loss.item() * inputs.size(0)
                running_corrects += torch.sum(preds == labels.data)
                order += idx.tolist()
                logits.append(outputs.detach().double().numpy())
                losses.append(loss.item())
            epoch_loss = running_loss / len(loaders[phase].dataset)
            epoch_acc = running_corrects.double() / len(loaders[phase].dataset)
            print('  %s %s Loss: %.4f Acc: %.4f' % (dtype, phase, epoch_loss, epoch_acc), flush=True)
            out['order_' + phase].append(order)
            out['logits_' + phase].append(np.stack(logits))
            out['batch_loss_' + phase].append(losses)
            rec_loss.append(epoch_loss)
            rec_acc.append(float(epoch_acc))
            if phase == 'val' and (epoch + 1) % SAVE_EPOCHS == 0:
                out['saved'].append(epoch + 1)
                out['saved_sums'].append([float(v.double().sum()) for v in model.state_dict().values()])
            took = phase == 'val' and bool(epoch_acc > best_acc)
            if took:
                best_acc, best_epoch = float(epoch_acc), epoch
                best_wts = copy.deepcopy(model.state_dict())
            if phase == 'val':
                out['taken'].append(int(took))
        out['loss'].append(rec_loss)
        out['acc'].append(rec_acc)
    out['final_sums'] = [float(v.double().sum()) for v in model.state_dict().values()]
    out['final_norms'] = [float(v.double().norm()) for v in model.state_dict().values()]
    model.load_state_dict(best_wts)
    out['best_sums'] = [float(v.double().sum()) for v in model.state_dict().values()]
    out['best_acc'], out['best_epoch'] = best_acc, best_epoch
    return {k: np.asarray(v) for k, v in out.items()}


def margins(logits):
    s = np.sort(logits.reshape(-1, logits.shape[-1]), axis=1)
    return float((s[:, -1] - s[:, -2]).min())


def acceptable(r, why):
    accs = r['acc'][:, 1]
    # "not decided by a tie": no other epoch reaches the best accuracy, so > and >= name the same best epoch
    ok = (r['best_epoch'] > 0 and np.isfinite(r['loss']).all() and int((accs == r['best_acc']).sum()) == 1
          and min(margins(r['logits_train']), margins(r['logits_val'])) >= 1e-3)
    if not ok:
        print('  rejected (%s): best epoch %d, val acc %s, margins %.2e %.2e' % (why, r['best_epoch'], accs, margins(r['logits_train']),
                                                                                margins(r['logits_val'])), flush=True)
    return ok


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 2600
    while True:
        print('seed', seed, flush=True)
        train, val = XI.views(seed * 10, XI.TRAIN_LABELS), XI.views(seed * 10 + 5, XI.VAL_LABELS)
        r32 = run(seed, torch.float32, train, val)
        if acceptable(r32, 'fp32'):
            r64 = run(seed, torch.float64, train, val)
            same = all(np.array_equal(r32['logits_' + p].argmax(-1), r64['logits_' + p].argmax(-1)) for p in ('train', 'val'))
            if same and acceptable(r64, 'fp64') and np.array_equal(r32['taken'], r64['taken']):
                break
            print('  rejected: fp32 and fp64 disagree', flush=True)
        seed += 1
    assert np.array_equal(r32['order_train'], r64['order_train']) and np.array_equal(r32['order_val'], r64['order_val'])
    out = {'seed': np.int64(seed), 'epochs': np.int64(EPOCHS), 'batch': np.int64(BATCH), 'save_model_epochs': np.int64(SAVE_EPOCHS),
           'lr': np.float64(LR), 'momentum': np.float64(MOMENTUM), 'train_labels': np.asarray(XI.TRAIN_LABELS, np.int32),
           'val_labels': np.asarray(XI.VAL_LABELS, np.int32), 'order_train': r32['order_train'].astype(np.int64),
           'order_val': r32['order_val'].astype(np.int64), 'keys': np.array([k for k, _ in CI.param_shapes(XI.NUM_CLASSES)]),
           'image_sums': np.array([float(train[0].astype(np.float64).sum()), float(val[0].astype(np.float64).sum())])}
    for tag, r in (('f32', r32), ('f64', r64)):
        for k in ('logits_train', 'logits_val', 'loss', 'acc', 'taken', 'batch_loss_train', 'batch_loss_val', 'saved', 'saved_sums',
                  'final_sums', 'final_norms', 'best_sums', 'best_acc', 'best_epoch'):
            out['%s_%s' % (k, tag)] = r[k]
    print('loss fp32', r32['loss'].tolist(), '\nloss fp64', r64['loss'].tolist(), '\n|fp32 - fp64|', np.abs(r32['loss'] - r64['loss']).tolist())
    path = os.path.join(ROOT, 'tests', 'golden', 'g26_cls_train.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
