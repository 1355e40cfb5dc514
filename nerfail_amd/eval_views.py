"""model_test.evaluate_record / evaluate_views with one more keyword, `native_resize=False`: when True and the model is resized
for (any model_name but "my_model"), both resizes go through _resize.resize_native - csrc/resize.hip's kernel, fixed-order float32
arithmetic, the same bits on every run - instead of _resize.resize. With the default the calls ARE model_test's. model_test.py
itself keeps its text; everything else (view formats, metrics, fold, report) is its code, used from here."""
import torch

from . import _lib, ops
from . import model_test as MT
from ._resize import resize_native


def evaluate_record(model, model_name, attacked, originals, label, batch=8, num_classes=8, resize_to=None, native_resize=False):
    """model_test.evaluate_record; native_resize=True: its resized branch with resize_native in the place of resize."""
    if not native_resize or model_name == "my_model":
        return MT.evaluate_record(model, model_name, attacked, originals, label, batch, num_classes, resize_to)
    if not 1 <= num_classes <= 32 or not 0 <= label < num_classes:
        raise ValueError('num_classes must be 1..32 and label a class index')
    dev = MT._cuda()
    a_views, a_fmt, hw = MT._views(attacked, dev)
    o_views, o_fmt, hw_o = MT._views(originals, dev)
    if len(a_views) != len(o_views) or hw != hw_o:
        raise ValueError('attacked and originals must hold the same number of views of one size')
    size = resize_to or (224 if model_name == "vit_b_16" else 299)
    record = torch.zeros(_lib.EVAL_RECORD_DOUBLES, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for b0 in range(0, len(a_views), batch):
            a, o = a_views[b0:b0 + batch], o_views[b0:b0 + batch]
            _, a3 = ops.eval_view_metrics(a, a_fmt, a, a_fmt, True)
            _, o3 = ops.eval_view_metrics(o, o_fmt, o, o_fmt, True)
            cla_in = resize_native(a3.view(len(a), 3, hw[0], hw[1]), size)
            o3 = resize_native(o3.view(len(a), 3, hw[0], hw[1]), size)
            rows, _ = ops.eval_view_metrics(MT._flat(cla_in), _lib.EVAL_FLAT, MT._flat(o3), _lib.EVAL_FLAT, False)
            logits = model(cla_in)
            if logits.dim() != 2 or logits.shape[1] != num_classes:
                raise ValueError('the classifier returned %s, expected [B,%d]' % (tuple(logits.shape), num_classes))
            pred, ce = ops.eval_logit_stats(logits, label)
            ops.eval_fold(rows, pred, ce, num_classes, record)
    return record


def evaluate_views(model, model_name, attacked, originals, label, batch=8, num_classes=8, resize_to=None, native_resize=False):
    """model_test.evaluate_views over the evaluate_record above: report()'s dict, the record read once."""
    record = evaluate_record(model, model_name, attacked, originals, label, batch, num_classes, resize_to, native_resize)
    return MT.report(record.cpu().numpy(), label, num_classes)
