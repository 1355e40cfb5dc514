"""model_train.py:107-193 (= MTR) as a product loop: train the victim classifier that every later stage loads
(model/weights/<model_name>_<num_classes>_best.pth), on the device.

    from nerfail_amd.MyDataset import MySimpleDataset
    from nerfail_amd.model_train import train_classifier
    sets = {x: MySimpleDataset(data_dir, x, class_names_file, _3_channels=True, device='cuda') for x in ['train', 'val']}
    records, best_acc = train_classifier(MyCNN(8, trainable=True).cuda(), sets['train'], sets['val'], weights_dir='model/weights')

For a trainable native MyCNN a training step makes no autograd graph and waits for nothing on the host:
    ops.cls_batch         the batch, gathered from the resident uint8 store by indices that live on the device
    ops.cnn_fwd           the forward, keeping its pool masks
    ops.cls_ce            per-view CE and predictions into the phase's stats row; d loss / d logits of the mean CE
    ops.cnn_bwd_weights_into   the flat gradient of all 18 parameters, into a buffer reused every step
    MyCNN.sgd_step        torch.optim.SGD's momentum step and the weight image, one launch
and an epoch ends with ops.cls_epoch_close (MTR:170-186) and ops.copy_if, which keeps the best weights without a host
decision. The epoch's record is read once, for the two log lines of MTR:173. Any other nn.Module takes the same batches through
stock autograd and torch.optim.SGD; its statistics still come from ops.cls_ce.

Kept from the reference: both phases are shuffled and drop their last partial batch, yet losses and accuracies divide by
len(dataset) (MTR:102, 170-171); the best epoch needs a strictly higher validation accuracy (MTR:181).
Not kept: torch's shuffle order (the default order is nerfail_index_shuffle's, keyed on (seed, epoch, phase); `order` takes an
explicit one). Documented deviation: getModel (model/GetModel.py:44-49) hands "my_model" a Resize([299, 299]) because its second
`if` is not an `elif`; on 299 x 299 MyCNN's seventh stage is empty, so the reference as written cannot train it. "my_model"
is not resized here - as GN:147-148 and model_test treat it, and as fc1's 1024 inputs require."""
import os

import torch

from . import _lib
from . import _resize
from . import ops

RECORD_FIELDS = ('train_loss', 'train_acc', 'val_loss', 'val_acc', 'taken', 'best_epoch', 'best_acc', 'epoch', 'train_correct',
                 'train_views', 'val_correct', 'val_views')
PHASES = ('train', 'val')


def _read_record(record):
    """THE host read of an epoch: its record, one device-to-host copy."""
    v = record.cpu().tolist()
    d = dict(zip(RECORD_FIELDS, v))
    for k in ('taken', 'best_epoch', 'epoch', 'train_correct', 'train_views', 'val_correct', 'val_views'):
        d[k] = int(d[k])
    return d


def resize_to(model_name):
    """The input size of a classifier by its name (model/GetModel.py:44-49, with "my_model" left alone: see the module text)."""
    if model_name == 'my_model':
        return None
    return 224 if model_name == 'vit_b_16' else 299


def shuffle_key(seed, epoch, phase):
    """The nerfail_index_shuffle key of one phase of one epoch."""
    return ops.as_op_key((int(seed) << 32) ^ (int(epoch) << 1) ^ int(phase))


def _is_native(model):
    from .MyModel import MyCNN
    return isinstance(model, MyCNN) and model.trainable


def _store_of(dataset):
    store, labels = getattr(dataset, 'store', None), getattr(dataset, 'labels', None)
    if store is None or labels is None or not store.is_cuda:
        raise RuntimeError('train_classifier: the dataset must be resident on the device (MySimpleDataset(..., device="cuda"): '
                           'a uint8 `store` and int32 `labels`); nerfail_amd runs on the MI355X only (no CPU path)')
    return store, labels


def _phase_order(dataset, seed, epoch, phase, order):
    n = len(dataset)
    store, _ = _store_of(dataset)
    if order is not None:
        idx = torch.as_tensor(order(epoch, PHASES[phase]), dtype=torch.int64).to(store.device)
        if idx.dim() != 1:
            raise ValueError('order(epoch, phase) must return a 1-D index tensor')
        return idx
    return ops.index_shuffle(store, shuffle_key(seed, epoch, phase), n, 0, n)


class _Native:
    """The step of a flattened trainable MyCNN: no autograd graph, no host read."""

    def __init__(self, model, lr, momentum):
        self.model, self.lr, self.momentum = model, lr, momentum
        self.flat = model.flatten_parameters()
        self.momentum_buf = torch.zeros_like(self.flat)
        self.d_params = torch.zeros_like(self.flat)      # reused every step; its alignment floats are never written
        self.scratch, self.steps = None, 0

    def train_step(self, x, labels, row):
        m = self.model
        with torch.no_grad():
            logits, ws, masks = ops.cnn_fwd(m.packed(), x, m.num_classes, True)
            d_logits = ops.cls_ce(logits, labels, row, True)
            need = ops.cnn_bwd_weights_scratch_floats(x.shape[0], x.shape[2], x.shape[3], m.num_classes)
            if self.scratch is None or self.scratch.numel() < need:
                self.scratch = torch.empty((need,), dtype=torch.float32, device=x.device)
            ops.cnn_bwd_weights_into(m.packed(), x, ws, masks, d_logits, self.scratch, self.d_params)
            m.sgd_step(self.d_params, self.momentum_buf, self.lr, self.momentum, self.steps == 0)
        self.steps += 1

    def eval_step(self, x, labels, row):
        m = self.model
        with torch.no_grad():
            logits, _, _ = ops.cnn_fwd(m.packed(), x, m.num_classes, False)
            ops.cls_ce(logits, labels, row, False)

    def parameters_flat(self):
        return self.flat

    def load_flat(self, flat):
        with torch.no_grad():
            self.flat.copy_(flat)                       # an in-place write through the base: tell the views' caches
            for p in self.model._params():
                torch.autograd.graph.increment_version(p)


class _Stock:
    """Any other nn.Module: the same batches through stock autograd and torch.optim.SGD (MTR:140-165)."""

    def __init__(self, model, model_name, lr, momentum):
        self.model, self.size, self.lr, self.momentum, self.opt = model, resize_to(model_name), lr, momentum, None

    def _inputs(self, x):
        return x if self.size is None else _resize.resize(x, self.size)

    def train_step(self, x, labels, row):
        if self.opt is None:
            self.opt = torch.optim.SGD(self.model.parameters(), lr=self.lr, momentum=self.momentum)     # MTR:90
        self.opt.zero_grad()
        out = self.model(self._inputs(x))
        target = labels.long()
        if isinstance(out, tuple):                      # MTR:148-152: the auxiliary classifier of a model in train mode
            out, aux = out[0], out[1]
            loss = torch.nn.functional.cross_entropy(out, target) + 0.4 * torch.nn.functional.cross_entropy(aux, target)
        else:
            loss = torch.nn.functional.cross_entropy(out, target)
        loss.backward()
        self.opt.step()
        ops.cls_ce(_lib.f32c(out), labels, row, False)

    def eval_step(self, x, labels, row):
        with torch.no_grad():
            out = self.model(self._inputs(x))
        ops.cls_ce(_lib.f32c(out[0] if isinstance(out, tuple) else out), labels, row, False)

    def parameters_flat(self):
        return torch.cat([t.detach().reshape(-1).float() for t in self.model.state_dict().values()])

    def load_flat(self, flat):
        o = 0
        with torch.no_grad():
            for t in self.model.state_dict().values():
                t.copy_(flat[o:o + t.numel()].view(t.shape).to(t.dtype))
                o += t.numel()


def _stepper(model, model_name, lr, momentum):
    return _Native(model, lr, momentum) if _is_native(model) else _Stock(model, model_name, lr, momentum)


def _run_phase(step, dataset, idx, batch_size, row, train):
    store, labels_all = _store_of(dataset)
    fn = step.train_step if train else step.eval_step
    for first in range(0, idx.numel() - batch_size + 1, batch_size):       # drop_last=True (MTR:102)
        x, labels = ops.cls_batch(store, labels_all, idx[first:first + batch_size])
        fn(x, labels, row)


def _save(model, path):
    torch.save({k: v.detach().clone() for k, v in model.state_dict().items()}, path)


def train_classifier(model, train_set, val_set, *, model_name="my_model", num_classes=8, epochs=200, batch_size=16, lr=0.001,
                     momentum=0.9, save_model_epochs=50, weights_dir=None, seed=0, order=None, log=print):
    """MTR:107-193. Returns (records, best_acc): one dict of RECORD_FIELDS per epoch, and the best validation accuracy.
    `order(epoch, phase)` (phase = 'train' | 'val') may return the epoch's index order instead of the keyed shuffle. With
    `weights_dir`, <model_name>_<num_classes>_%03d.pth is written every `save_model_epochs` epochs and, at the end, the best
    weights are loaded into the model (MTR:192) and saved as <model_name>_<num_classes>_best.pth; both load into the
    reference's module with strict=True."""
    if batch_size < 1 or epochs < 0 or save_model_epochs < 1:
        raise ValueError('train_classifier: batch_size and save_model_epochs must be at least 1, epochs at least 0')
    sets = (train_set, val_set)
    dev = _store_of(train_set)[0].device
    step = _stepper(model, model_name, lr, momentum)
    n = _lib.ATTACK_ROW_FLOATS
    rows = torch.zeros((max(epochs, 1), 2, n), dtype=torch.float32, device=dev)
    recs = torch.zeros((max(epochs, 1), n), dtype=torch.float32, device=dev)
    best = torch.tensor([0., -1.], dtype=torch.float32).to(dev)            # MTR:92
    flag = torch.zeros((1,), dtype=torch.int32, device=dev)
    best_flat = step.parameters_flat().clone()                             # MTR:91
    if weights_dir is not None:
        os.makedirs(weights_dir, exist_ok=True)
    stem = '%s_%d' % (model_name, num_classes)
    records = []
    for epoch in range(epochs):
        log('Epoch {}/{}'.format(epoch + 1, epochs))
        log('*' * 10)
        for phase in (0, 1):
            model.train() if phase == 0 else model.eval()
            idx = _phase_order(sets[phase], seed, epoch, phase, order)
            _run_phase(step, sets[phase], idx, batch_size, rows[epoch, phase], phase == 0)
        ops.cls_epoch_close(rows[epoch, 0], rows[epoch, 1], len(train_set), len(val_set), best, epoch, recs[epoch], flag)
        if weights_dir is not None and (epoch + 1) % save_model_epochs == 0:                       # MTR:177-179
            _save(model, os.path.join(weights_dir, stem + '_%03d.pth' % (epoch + 1)))
        ops.copy_if(flag, step.parameters_flat(), best_flat)               # MTR:181-183
        r = _read_record(recs[epoch])
        log('{} Loss: {:.4f} Acc: {:.4f}'.format('train', r['train_loss'], r['train_acc']))
        log('{} Loss: {:.4f} Acc: {:.4f}'.format('val', r['val_loss'], r['val_acc']))
        records.append(r)
    best_acc = records[-1]['best_acc'] if records else 0.0
    log('Best val Acc: {:4f}'.format(best_acc))
    if weights_dir is not None:
        step.load_flat(best_flat)                                          # MTR:192
        _save(model, os.path.join(weights_dir, stem + '_best.pth'))
    return records, best_acc


def evaluate_classifier(model, dataset, *, model_name="my_model", batch_size=16, seed=0, order=None):
    """The validation phase alone (MTR:115, 157-171): {'loss', 'acc', 'correct', 'views'} of `model` on `dataset`, shuffled and
    with drop_last as there, divided by len(dataset)."""
    store, _ = _store_of(dataset)
    step = _Stock(model, model_name, 0.0, 0.0)                              # evaluation only: the module's own forward
    row = torch.zeros((_lib.ATTACK_ROW_FLOATS,), dtype=torch.float32, device=store.device)
    was_training = model.training
    model.eval()
    _run_phase(step, dataset, _phase_order(dataset, seed, 0, 1, order), batch_size, row, False)
    model.train(was_training)
    v = row.cpu().tolist()
    n = max(len(dataset), 1)
    return {'loss': (v[0] + v[1]) / n, 'acc': v[2] / n, 'correct': int(v[2]), 'views': int(v[3])}
