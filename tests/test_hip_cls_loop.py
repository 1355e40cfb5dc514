"""-m gpu: nerfail_amd.model_train.train_classifier - against a hand-written loop over the same five ops (bitwise), against the
reference's own run (fixture g26, tests/golden/make_golden_cls_train.py), on the stock fallback path, and MySimpleDataset on a
directory of small PNGs."""
import os

import numpy as np
import pytest
import torch

import cls_inputs as XI
import cls_train_ref as R
import cnn_inputs as CI

pytestmark = pytest.mark.gpu

# Test 6's loss bound: 2 x |fp32 - fp64 of the reference| + FLOOR of the reference's fp64 value. The HIP-to-fp64 distance of the
# per-epoch losses was measured on the MI355X BEFORE the floor was chosen (this file's test, printing and not yet asserting):
#   epoch 1  train 1.5e-7  val 8.8e-7     (the reference's own fp32 run: 2.1e-7, 1.7e-5)
#   epoch 2  train 3.5e-8  val 1.3e-7     (1.4e-4, 7.4e-4)
#   epoch 3  train 2.7e-5  val 3.5e-5     (3.0e-3, 4.4e-3: by now a pool window routed differently has moved the weights)
# The distance is taken where no routing flip has been amplified by later steps yet, the first epoch: 8.8e-7. The floor is four
# times that, 3.5e-6 - 2.9e-6 of the smallest loss, far below the cap of 1e-4 of the loss, the project's literal bound elsewhere.
MEASURED_HIP_TO_F64 = 8.8e-7
FLOOR_ABS = 4 * MEASURED_HIP_TO_F64
FLOOR_CAP_REL = 1e-4


def _dev():
    return torch.device('cuda:0')


class Resident:
    """What train_classifier needs of a dataset: a resident uint8 store, int32 labels, a length."""

    def __init__(self, store, labels):
        self.store, self.labels = torch.from_numpy(store).to(_dev()), torch.from_numpy(labels).to(_dev())

    def __len__(self):
        return self.store.shape[0]


def native(seed, trainable=True):
    from nerfail_amd.MyModel import MyCNN
    m = MyCNN(XI.NUM_CLASSES, trainable=trainable)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CI.state_dict(seed, XI.NUM_CLASSES).items()}, strict=True)
    return m.to(_dev())


@pytest.fixture(scope='module')
def problem(golden):
    g = golden('g26_cls_train')
    seed = int(g['seed'])
    train, val = XI.views(seed * 10, XI.TRAIN_LABELS), XI.views(seed * 10 + 5, XI.VAL_LABELS)
    assert [float(train[0].astype(np.float64).sum()), float(val[0].astype(np.float64).sum())] == g['image_sums'].tolist()
    return g, seed, Resident(*train), Resident(*val)


def order_of(g):
    return lambda epoch, phase: torch.from_numpy(g['order_' + phase][epoch])


@pytest.fixture(scope='module')
def product_run(problem, tmp_path_factory):
    """ONE run of train_classifier on g26's problem and recorded orders, shared by the tests below."""
    from nerfail_amd import model_train as MT
    g, seed, train, val = problem
    out = tmp_path_factory.mktemp('weights')
    made, reads, lines = [], [], []

    class Spy(MT._Native):
        def __init__(self, *a):
            super().__init__(*a)
            made.append(self)

    read = MT._read_record

    def counted(rec):
        reads.append(1)
        return read(rec)
    MT._Native, MT._read_record = Spy, counted
    try:
        m = native(seed)
        records, best_acc = MT.train_classifier(m, train, val, num_classes=XI.NUM_CLASSES, epochs=int(g['epochs']), batch_size=int(g['batch']),
                                                lr=float(g['lr']), momentum=float(g['momentum']),
                                                save_model_epochs=int(g['save_model_epochs']), weights_dir=str(out), order=order_of(g),
                                                log=lines.append)
    finally:
        MT._Native, MT._read_record = Spy.__mro__[1], read
    step = made[0]
    return dict(model=m, records=records, best_acc=best_acc, momentum=step.momentum_buf.clone(), dir=str(out), reads=len(reads),
                lines=lines)


def hand_loop(problem):
    """The same five ops, one by one, with the bookkeeping on the host."""
    from nerfail_amd import ops as O
    g, seed, train, val = problem
    E, bs, C = int(g['epochs']), int(g['batch']), XI.NUM_CLASSES
    m = native(seed)
    flat = m.flatten_parameters()
    packed = m.packed()
    buf = torch.zeros_like(flat)
    best, best_flat, records, steps = np.array([0, -1], np.float32), flat.clone(), [], 0
    saved = {}
    for e in range(E):
        rows = []
        for phase, ds in (('train', train), ('val', val)):
            row = torch.zeros(16, device=_dev())
            idx = torch.from_numpy(g['order_' + phase][e]).to(_dev())
            for first in range(0, idx.numel() - bs + 1, bs):
                x, lb = O.cls_batch(ds.store, ds.labels, idx[first:first + bs])
                with torch.no_grad():
                    logits, ws, masks = O.cnn_fwd(packed, x, C, phase == 'train')
                    d = O.cls_ce(logits, lb, row, phase == 'train')
                    if phase == 'train':
                        dp, _ = O.cnn_bwd_weights(packed, x, ws, masks, d, False)
                        O.cnn_sgd_step(flat, dp, buf, packed, C, float(g['lr']), float(g['momentum']), steps == 0)
                        steps += 1
            rows.append(row.cpu().numpy())
        rec, take = R.epoch_close(rows[0], rows[1], len(train), len(val), best, e)
        if (e + 1) % int(g['save_model_epochs']) == 0:
            saved[e + 1] = flat.clone()
        if take:
            best_flat = flat.clone()
        records.append(rec)
    return flat, buf, np.stack(records), best, best_flat, saved


def record_array(records):
    from nerfail_amd.model_train import RECORD_FIELDS
    return np.array([[r[k] for k in RECORD_FIELDS] for r in records], np.float32)


def stock_module():
    """A stock-torch module of the reference's layout (model/MyModel.py:5-52: the same submodule names and shapes)."""
    class Stock(torch.nn.Module):
        def __init__(self):
            super().__init__()
            for i in range(7):
                setattr(self, 'conv%d' % (i + 1), torch.nn.Conv2d(CI.CHANS[i], CI.CHANS[i + 1], 3))
                setattr(self, 'max_pool%d' % (i + 1), torch.nn.MaxPool2d(2))
            self.fc1, self.fc2 = torch.nn.Linear(1024, 512), torch.nn.Linear(512, XI.NUM_CLASSES)
    return Stock()


# ------------------------------------------------------------------------------------------------------------ 5. against its pieces
def test_loop_is_bitwise_its_own_pieces(problem, product_run):
    from nerfail_amd import ops as O
    g = problem[0]
    flat, buf, records, best, best_flat, saved = hand_loop(problem)
    got = record_array(product_run['records'])
    assert np.array_equal(got.view(np.int32), records[:, :12].view(np.int32)), (got, records[:, :12])
    assert torch.equal(product_run['momentum'], buf)
    assert product_run['best_acc'] == float(best[0]) and product_run['records'][-1]['best_epoch'] == int(best[1])
    # MTR:192: the model ends with the BEST weights; the last epoch's are in the numbered checkpoint only when it is a save epoch
    layout, _ = O.cnn_grad_layout(XI.NUM_CLASSES)
    m = product_run['model']
    for (o, sh), (k, v) in zip(layout, m.state_dict().items()):
        assert torch.equal(v.reshape(-1), best_flat[o:o + v.numel()]), k
    assert product_run['reads'] == int(g['epochs'])                                # ONE record read per epoch, nothing else
    lines = product_run['lines']
    assert lines[0] == 'Epoch 1/3' and lines[1] == '*' * 10 and lines[2:4] == R.log_lines(records[0])
    assert lines[-1] == 'Best val Acc: {:4f}'.format(float(best[0]))
    # both checkpoint files load into a stock-torch module of the reference's layout with strict=True
    names = sorted(os.listdir(product_run['dir']))
    assert names == ['my_model_8_%03d.pth' % e for e in R.save_epochs(int(g['epochs']), int(g['save_model_epochs']))] + ['my_model_8_best.pth']
    for name, want in (('my_model_8_002.pth', saved[2]), ('my_model_8_best.pth', best_flat)):
        sd = torch.load(os.path.join(product_run['dir'], name), map_location='cpu')
        stock = stock_module()
        stock.load_state_dict(sd, strict=True)
        assert all(v.is_contiguous() and v.untyped_storage().nbytes() == v.numel() * 4 for v in sd.values())   # no 7.5 MB per tensor
        for (o, sh), (k, v) in zip(layout, stock.state_dict().items()):
            assert torch.equal(v.reshape(-1), want[o:o + v.numel()].cpu()), (name, k)


def test_no_host_read_inside_an_epoch(problem, monkeypatch):
    """One epoch with every Tensor.cpu / .item / .tolist / .numpy counted: the only device-to-host copy is the record read."""
    from nerfail_amd import model_train as MT
    g, seed, train, val = problem
    calls = []
    for name in ('cpu', 'item', 'tolist', 'numpy', '__bool__', '__float__', '__int__'):
        orig = getattr(torch.Tensor, name)

        def spy(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                calls.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, spy)
    dev_orders = {(e, p): torch.from_numpy(g['order_' + p][e]).to(_dev()) for e in range(1) for p in ('train', 'val')}
    calls.clear()
    MT.train_classifier(native(seed), train, val, num_classes=XI.NUM_CLASSES, epochs=1, batch_size=int(g['batch']),
                        order=lambda e, p: dev_orders[(e, p)], log=lambda s: None)
    assert calls == ['cpu'], calls


# ------------------------------------------------------------------------------------------------------------ 6. against the reference
def test_loop_against_the_reference(problem, product_run):
    """Every prediction-derived number equal; every per-epoch loss within 2 x |fp32 - fp64 of the reference| + floor of the
    reference's fp64 value. Measured on the MI355X before the floor was chosen: see MEASURED_HIP_TO_F64 above and DESIGN.md."""
    g = problem[0]
    rec = record_array(product_run['records'])
    for tag in ('f32', 'f64'):
        assert np.array_equal(rec[:, 1], g['acc_' + tag][:, 0].astype(np.float32))
        assert np.array_equal(rec[:, 3], g['acc_' + tag][:, 1].astype(np.float32))
        assert rec[:, 4].astype(int).tolist() == g['taken_' + tag].tolist()
        assert int(rec[-1, 5]) == int(g['best_epoch_' + tag]) and rec[-1, 6] == np.float32(g['best_acc_' + tag])
    f32, f64 = g['loss_f32'], g['loss_f64']
    got = rec[:, [0, 2]].astype(np.float64)
    floor = np.minimum(FLOOR_ABS, FLOOR_CAP_REL * np.abs(f64))
    bound = 2 * np.abs(f32 - f64) + floor
    err = np.abs(got - f64)
    for e in range(len(got)):
        print('epoch %d  train/val loss HIP %s  fp64 %s  |HIP - fp64| %s  |fp32 - fp64| %s  bound %s'
              % (e + 1, got[e], f64[e], err[e], np.abs(f32 - f64)[e], bound[e]))
    assert (err <= bound).all(), (err, bound)


# ------------------------------------------------------------------------------------------------------------ 7. fallback path
def test_stock_module_takes_the_same_batches(problem):
    from nerfail_amd import model_train as MT
    g, seed, train, val = problem
    torch.manual_seed(0)
    tiny = torch.nn.Sequential(torch.nn.AdaptiveAvgPool2d(4), torch.nn.Flatten(), torch.nn.Linear(48, XI.NUM_CLASSES)).to(_dev())
    with torch.no_grad():
        tiny[2].weight.mul_(0.01)
    seen = []
    tiny.register_forward_hook(lambda mod, inp, out: seen.append((tuple(inp[0].shape), out.detach().double().cpu(), mod.training)))
    w0 = tiny[2].weight.detach().clone()
    assert MT.resize_to('tiny') == 299 and MT.resize_to('vit_b_16') == 224 and MT.resize_to('my_model') is None
    records, _ = MT.train_classifier(tiny, train, val, model_name='tiny', num_classes=XI.NUM_CLASSES, epochs=1, batch_size=2,
                                     order=order_of(g), log=lambda s: None)
    assert [s[0] for s in seen] == [(2, 3, 299, 299)] * 3 and [s[2] for s in seen] == [True, True, False]     # two steps, one val batch
    assert not torch.equal(tiny[2].weight.detach(), w0)
    labels = {'train': g['train_labels'], 'val': g['val_labels']}
    r = records[0]
    for phase, outs, n in (('train', seen[:2], 5), ('val', seen[2:], 3)):
        y = torch.from_numpy(labels[phase][g['order_' + phase][0][:2 * len(outs)]]).long().view(len(outs), 2)
        ce = sum(torch.nn.functional.cross_entropy(o[1], yy, reduction='sum').item() for o, yy in zip(outs, y))
        correct = sum(int((o[1].argmax(1) == yy).sum()) for o, yy in zip(outs, y))
        assert abs(r[phase + '_loss'] - ce / n) <= 2.0 ** -23 * abs(ce / n) + 1e-12           # float64 CE, the record's float32
        assert r[phase + '_correct'] == correct and r[phase + '_views'] == 2 * len(outs)
        assert r[phase + '_acc'] == float(np.float32(correct / n))


def test_evaluate_classifier_is_the_val_phase(problem, product_run):
    from nerfail_amd import model_train as MT
    g, seed, train, val = problem
    m = native(seed)
    out = MT.evaluate_classifier(m, val, batch_size=2, order=lambda e, p: torch.from_numpy(g['order_val'][0]))
    assert not m._is_flat()                                                        # evaluation leaves the module as it was
    first = MT.train_classifier(native(seed), train, val, num_classes=8, epochs=0, log=lambda s: None)
    assert first == ([], 0.0)
    assert out['views'] == 2 and 0 <= out['correct'] <= 2 and np.isfinite(out['loss'])
    frozen = native(seed, trainable=False).requires_grad_(False)
    again = MT.evaluate_classifier(frozen, val, batch_size=2, order=lambda e, p: torch.from_numpy(g['order_val'][0]))
    assert again == out


# ------------------------------------------------------------------------------------------------------------ MySimpleDataset
def test_my_simple_dataset_on_a_directory(tmp_path):
    from PIL import Image
    from nerfail_amd.MyDataset import MySimpleDataset, find_classes
    rs = np.random.RandomState(0)
    made = {}
    for cls, count in (('chair', 2), ('lego', 3)):
        for set_name in ('train', 'val'):
            d = tmp_path / cls / set_name
            d.mkdir(parents=True)
            for i in range(count):
                a = rs.randint(0, 255, size=(6, 9, 4)).astype(np.uint8)
                a[..., 3] = rs.randint(0, 2, size=(6, 9)) * 255
                Image.fromarray(a, 'RGBA').save(d / ('r_%d.png' % i))
                made[(cls, set_name, i)] = a[..., [2, 1, 0, 3]]                    # cv2 order: BGRA
            Image.fromarray(a, 'RGBA').save(d / 'r_0_depth_0001.png')               # three parts: filtered (MD:82)
            Image.fromarray(a, 'RGBA').save(d / 'ori_7.png')                       # "ori": filtered
    names = tmp_path / 'class_names.txt'
    ds = MySimpleDataset(str(tmp_path), 'train', str(names), _3_channels=True, resize_frame=True, resize_frame_size=None, device='cuda')
    assert find_classes(str(tmp_path))[0] == ['chair', 'lego'] and names.read_text() == '0 -- chair\n1 -- lego\n'
    assert len(ds) == 5 and ds.indices == [0, 1, 2, 3, 4] and ds.labels.tolist() == [0, 0, 1, 1, 1]
    assert ds.store.dtype == torch.uint8 and tuple(ds.store.shape) == (5, 6, 9, 4) and ds.store.is_cuda
    for idx, key in ((0, ('chair', 'train', 0)), (1, ('chair', 'train', 1)), (2, ('lego', 'train', 0)), (4, ('lego', 'train', 2))):
        x, label = ds[idx]
        assert label == (0 if key[0] == 'chair' else 1) and x.dtype == torch.float32 and tuple(x.shape) == (3, 6, 9)
        assert np.array_equal(x.cpu().numpy(), XI.white_nchw(made[key][None])[0])
    for kw, what in ((dict(load_later=True), 'load_later'), (dict(ori_img_from={0: 'x'}), 'ori_img_from'), (dict(_3_channels=False), '_3_channels')):
        args = dict(_3_channels=True, device='cuda')
        args.update(kw)
        with pytest.raises(NotImplementedError, match=what):
            MySimpleDataset(str(tmp_path), 'train', **args)
    Image.fromarray(np.zeros((5, 9, 4), np.uint8), 'RGBA').save(tmp_path / 'lego' / 'val' / 'r_3.png')
    with pytest.raises(ValueError, match='differ'):
        MySimpleDataset(str(tmp_path), 'val', _3_channels=True, device='cuda')
