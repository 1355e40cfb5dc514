"""Mirror of model_test.py (reference = MT): what an attack is judged by - the attack success rate and where the wrong
predictions went, eps min / avg / max, the L2 and L0 distance and PSNR min / max / avg between every attacked view and its
original - measured on the device.

The reference runs this stage on the CPU, one view at a time, with ~15 full-image torch ops and a dozen host reads per view
(MT:226-348). Here one pass of nerfail_eval_view_metrics over a batch of (attacked, original) pairs yields the five distances
and the classifier's NCHW input, nerfail_eval_logit_stats the predictions and cross entropies, and nerfail_eval_fold keeps the
set's running record on the device (include/nerfail_hip.h, "Attack evaluation"): no host read inside the loop, one read of the
record at the end.

    get_psnr            MT:26-39
    evaluate_views      the measurement on views already on the device (resident views, exported uint8 images, x_rgba);
                        evaluate_record is the same up to the one host read
    report              the record -> the reference's msg_dict (MT:355-399), pure host code
    test_for_inception  MT:41-421 with the reference's signature: directory names, PNGs, checkpoint, printed lines
    evaluate_render     the step=1 measurement (a NeRF retrained on the poisoned views) without the disk

Views are given in cv2's channel order, as stored (the order the classifiers were trained on). Not ported: the e-mail
(send_dict), the annotated images of MT:310-319, and method_name=None (a plain accuracy test of a whole dataset)."""
import math
import os
import time
from pathlib import Path

import numpy as np
import torch

from . import _lib
from . import ops
from ._resize import resize
from .run_nerf_helpers import _cuda

CLASS_LIST = {"chair": 0, "drums": 1, "ficus": 2, "hotdog": 3, "lego": 4, "materials": 5, "mic": 6, "ship": 7}     # MT:49


def get_psnr(target, ref):
    """MT:26-39."""
    diff = torch.flatten(ref - target)
    rmse = torch.sqrt(torch.mean(diff ** 2.))
    eps = torch.finfo(torch.float64).eps
    if rmse == 0:
        rmse = eps
    return 20 * math.log10(255.0 / rmse)


def _format_of(v):
    if v.dim() >= 2 and v.dtype == torch.uint8 and v.shape[-1] == 4:
        return _lib.EVAL_U8C4
    if v.dim() >= 2 and v.dtype == torch.uint8 and v.shape[-1] == 3:
        return _lib.EVAL_U8C3
    if v.dim() >= 2 and v.dtype == torch.float32 and v.shape[-1] == 4:
        return _lib.EVAL_F32C4
    raise ValueError('a view must be uint8 [H,W,4], uint8 [H,W,3] or float32 [H,W,4] (got %s %s)' % (v.dtype, tuple(v.shape)))


def _views(seq, dev):
    """(list of per-view device tensors, format, (H, W)) of a sequence of views or a stacked tensor [B,H,W,C]."""
    views = list(seq.unbind(0)) if isinstance(seq, torch.Tensor) else list(seq)
    if not views:
        raise ValueError('no views to evaluate')
    fmt = _format_of(views[0])
    out = []
    for v in views:
        if _format_of(v) != fmt or v.dim() != 3 or v.shape != views[0].shape:
            raise ValueError('every view of a side must be [H,W,C] with one dtype and shape')
        v = v.detach()
        if v.device != dev:
            v = v.to(dev)
        v = v.contiguous()
        if v.data_ptr() % (16 if fmt == _lib.EVAL_F32C4 else 4):        # e.g. a slice of stacked [B,H,W,3] uint8 with 3 H W odd
            v = v.clone()
        out.append(v)
    return out, fmt, tuple(views[0].shape[:2])


def report(record, label, num_classes):
    """The set record of nerfail_eval_fold (float64 [NERFAIL_EVAL_RECORD_DOUBLES], on the host) -> msg_dict of MT:355-399 with
    the reference's keys and string forms, plus "loss" and "acc" (MT:350-351) as floats. A view without a prediction (NaN
    logits) is listed under "<label> to -1"."""
    rec = [float(v) for v in record]
    number = int(rec[0])
    if number < 1:
        raise ValueError('report: the record holds no views')
    wrong_class_labels = {}
    for k in range(num_classes):
        if rec[16 + k] > 0:
            wrong_class_labels[str(k)] = int(rec[16 + k])
    if rec[10] > 0:
        wrong_class_labels['-1'] = int(rec[10])
    key = str(label)
    if key not in wrong_class_labels:                                                             # MT:366-373
        msg_dict = {"attack acc": "100.0 %"}
    else:
        msg_dict = {"attack acc": str((1 - wrong_class_labels[key] / number) * 100) + " %"}
    for wk in wrong_class_labels:                                                                 # MT:375-376
        msg_dict[key + " to " + wk] = str((wrong_class_labels[wk] / number) * 100) + " %"
    msg_dict.update({"e min": rec[2], "e avg": rec[3] / number, "e max": rec[1], "d l2 norm": rec[4] / number,      # MT:390-399
                     "d l0 norm": rec[5] / number, "psnr min": rec[6], "psnr max": rec[7], "psnr avg": rec[8] / number,
                     "loss": rec[9] / number, "acc": wrong_class_labels.get(key, 0) / number})
    return msg_dict


def _flat(t):
    return [v.reshape(-1) for v in t.unbind(0)]


def evaluate_record(model, model_name, attacked, originals, label, batch=8, num_classes=8, resize_to=None):
    """evaluate_views up to its host read: the set record of nerfail_eval_fold as a float64 device tensor. Nothing in here waits
    for the device."""
    if not 1 <= num_classes <= 32 or not 0 <= label < num_classes:
        raise ValueError('num_classes must be 1..32 and label a class index')
    dev = _cuda()
    a_views, a_fmt, hw = _views(attacked, dev)
    o_views, o_fmt, hw_o = _views(originals, dev)
    if len(a_views) != len(o_views) or hw != hw_o:
        raise ValueError('attacked and originals must hold the same number of views of one size')
    size = None if model_name == "my_model" else (resize_to or (224 if model_name == "vit_b_16" else 299))
    record = torch.zeros(_lib.EVAL_RECORD_DOUBLES, dtype=torch.float64, device=dev)
    with torch.no_grad():
        for b0 in range(0, len(a_views), batch):
            a, o = a_views[b0:b0 + batch], o_views[b0:b0 + batch]
            if size is None:
                rows, cla_in = ops.eval_view_metrics(a, a_fmt, o, o_fmt, True)
                cla_in = cla_in.view(len(a), 3, hw[0], hw[1])
            else:
                _, a3 = ops.eval_view_metrics(a, a_fmt, a, a_fmt, True)
                _, o3 = ops.eval_view_metrics(o, o_fmt, o, o_fmt, True)
                cla_in = resize(a3.view(len(a), 3, hw[0], hw[1]), size).contiguous()
                o3 = resize(o3.view(len(a), 3, hw[0], hw[1]), size).contiguous()
                rows, _ = ops.eval_view_metrics(_flat(cla_in), _lib.EVAL_FLAT, _flat(o3), _lib.EVAL_FLAT, False)
            logits = model(cla_in)
            if logits.dim() != 2 or logits.shape[1] != num_classes:
                raise ValueError('the classifier returned %s, expected [B,%d]' % (tuple(logits.shape), num_classes))
            pred, ce = ops.eval_logit_stats(logits, label)
            ops.eval_fold(rows, pred, ce, num_classes, record)
    return record


def evaluate_views(model, model_name, attacked, originals, label, batch=8, num_classes=8, resize_to=None):
    """MT:226-399 for one class of views: returns report()'s dict.

    attacked, originals: sequences (or ViewLists) of per-view tensors, or stacked tensors - uint8 [H,W,4] (a PNG as cv2 reads
    it, a resident view), uint8 [H,W,3] (a rendered view) or float32 [H,W,4] (x_rgba); the two sides need not share a format.
    model_name "my_model": the distances are measured on the images as given and the native MyCNN classifies the planar
    white-background image written by the same kernel pass. Any other model_name: both sides go through the white background,
    are resized to 299 (224 for "vit_b_16"; `resize_to` overrides) with gauss_net's resize rule, and are measured and classified
    after the resize, as the reference does (MD:110-113, MT:256-266). Nothing is read back inside the loop (evaluate_record);
    the record is read once, here."""
    record = evaluate_record(model, model_name, attacked, originals, label, batch, num_classes, resize_to)
    return report(record.cpu().numpy(), label, num_classes)               # the one host read


def evaluate_render(render_kwargs, poses, hwf, K, chunk, originals, model, model_name, label, **kw):
    """The step=1 measurement without the disk: every pose rendered with run_nerf.render, converted as run_nerf.render_path
    writes it (to8b: 255 * clip(rgb, 0, 1) truncated to uint8) and flipped to cv2's channel order on the device, then
    evaluate_views against `originals`. **kw goes to evaluate_views (batch, num_classes, resize_to)."""
    from .run_nerf import render
    H, W, _ = hwf
    H, W = int(H), int(W)
    views = []
    with torch.no_grad():
        for c2w in poses:
            rgb = render(H, W, K, chunk=chunk, c2w=c2w[:3, :4], **render_kwargs)[0]
            views.append((255 * torch.clamp(rgb, 0, 1)).to(torch.uint8).flip(-1).contiguous())
    return evaluate_views(model, model_name, views, originals, label, **kw)


def _imread_unchanged(path):
    """cv2.imread(path, cv2.IMREAD_UNCHANGED) of a PNG: uint8 [H,W,4] BGRA or [H,W,3] BGR."""
    try:
        import cv2
        img = cv2.imread(path, cv2.IMREAD_UNCHANGED)
    except ImportError:
        from PIL import Image
        im = Image.open(path)
        if im.mode == 'RGBA':
            img = np.asarray(im)[..., [2, 1, 0, 3]]
        else:
            img = np.asarray(im.convert('RGB'))[..., ::-1]
    if img is None or img.ndim != 3 or img.dtype != np.uint8:
        raise ValueError('%s is not an 8-bit 3- or 4-channel image' % path)
    return np.ascontiguousarray(img)


def _indexed_files(directory):
    """MD:77-87: the image files of a folder and their indices (r_12.png or 12.png; *_ori_* and three-part names are skipped)."""
    out = {}
    for f in os.listdir(directory):
        parts = f.split("_")
        if len(parts) < 3 and "ori" not in f:
            stem = parts[1] if len(parts) == 2 else parts[0]
            out[int(stem.replace(".png", "").replace(".jpg", "").replace(".jpeg", ""))] = os.path.join(directory, f)
    return out


def _build_model(model_name, num_classes):
    if model_name == "my_model" or model_name not in ("inception", "vgg16", "alexnet", "vit_b_16", "resnet50", "densenet121", "mobilenet",
                                                     "efficientnet", "swin_b"):
        from .MyModel import MyCNN
        return MyCNN(num_classes=num_classes)                                                     # MT:154-155
    from torchvision import models                                                                # MT:135-153
    if model_name == "inception":
        return models.inception.Inception3(num_classes=num_classes, init_weights=False)
    if model_name == "vgg16":
        return models.vgg16(num_classes=num_classes, init_weights=False)
    ctor = {"alexnet": "alexnet", "vit_b_16": "vit_b_16", "resnet50": "resnet50", "densenet121": "densenet121", "mobilenet": "mobilenet_v2",
            "efficientnet": "efficientnet_b0", "swin_b": "swin_b"}[model_name]
    return getattr(models, ctor)(num_classes=num_classes)


def test_for_inception(scene_name="lego", model_name="vgg16", now_class_idx=10, attack_epochs=100,
                       print_a=2, print_e=32, target_class_idx="n", base_mask_image_number=3, m1=0, m2=0,
                       setname="test", method_name="NeRFail", step=0, something_need_log: dict = None,
                       output_dir: str = None):
    """MT:41-421 for an attacked scene: reads the attacked views (MT:104-128) and the originals
    (./data/nerf_synthetic/<scene>/<setname>), loads ./model/weights/<model>_8_best.pth, measures on the device, prints the
    reference's lines and returns msg_dict (with something_need_log merged in) instead of mailing it."""
    if method_name is None:
        raise NotImplementedError('test_for_inception(method_name=None) is the plain accuracy test of a whole dataset, not an attack '
                                  'evaluation; it is not ported')
    since = time.time()
    class_list = CLASS_LIST
    label = class_list[scene_name]
    ori_dir = "./data/nerf_synthetic/" + scene_name + "/" + setname                               # MT:66
    step_name = {0: "attack", 1: "nerf", 2: "defense", 3: "nerf_defense"}[step]                    # MT:72-79
    if method_name == "IGSM":                                                                     # MT:88-91
        method_name = "NeRFail_S"
    elif method_name == "Universal":
        method_name = "NeRFail"
    print_tab = method_name + " " + step_name + " " + model_name + " " + str(base_mask_image_number) + \
        "P " + str(class_list[scene_name]) + " to " + str(target_class_idx) + \
        " and a=" + str(print_a) + ", e=" + str(print_e) + ", m1=" + str(m1) + ", m2=" + str(m2) + ", set=" + setname
    head = './output/' + model_name + '/' + step_name + '/' + scene_name + '/'
    if method_name == "NeRFail":                                                                  # MT:104-128
        test_dir = head + method_name + '_' + str(base_mask_image_number) + 'P_' + str(attack_epochs) + '_to_' + str(target_class_idx) + \
            '_e_' + str(print_e) + '_m_' + str(m1) + '_' + str(m2) + '/{}'.format(setname)
    elif method_name == "NeRFail_S":
        test_dir = head + method_name + '_' + str(base_mask_image_number) + 'P_' + str(attack_epochs) + '_to_' + str(target_class_idx) + \
            '_e_' + str(print_e) + '_a_' + str(print_a) + '/{}'.format(setname)
    elif method_name == "IGSM_2D":
        test_dir = head + method_name + '_' + str(attack_epochs) + '_to_' + str(target_class_idx) + '_e_' + str(print_e) + '_a_' + \
            str(print_a) + '/{}'.format(setname)
    elif method_name == "No_attack" and step == 0:
        test_dir = ori_dir
    elif method_name == "No_attack":
        test_dir = head + 'no_attack/{}'.format(setname)
    elif method_name == "Universal_2D":
        test_dir = head + 'Universal_2D_' + str(attack_epochs) + '_to_' + str(target_class_idx) + '_e_' + str(print_e) + '_m_' + str(m1) + \
            '_' + str(m2) + '/{}'.format(setname)
    else:
        raise ValueError('unknown method_name %r' % (method_name,))
    num_classes = len(class_list.keys())
    dev = _cuda()
    model = _build_model(model_name, num_classes)
    weights_path = Path("./model/weights/" + model_name + "_" + str(num_classes) + "_best.pth")   # MT:165-169
    print(weights_path.exists())
    print(weights_path.absolute())
    model.load_state_dict(torch.load(weights_path.absolute(), map_location='cpu'))
    model.to(dev).eval()
    print("Start test for AE model = " + model_name + " model!")
    print("Initializing Datasets and Dataloaders...")
    files = _indexed_files(test_dir)
    attacked, originals = [], []
    for idx in sorted(files):
        attacked.append(torch.from_numpy(_imread_unchanged(files[idx])).to(dev))
        originals.append(torch.from_numpy(_imread_unchanged(os.path.join(ori_dir, "r_" + str(idx) + ".png"))).to(dev))   # MD:118-124
    msg_dict = evaluate_views(model, model_name, attacked, originals, label, num_classes=num_classes)
    print('{} Loss: {:.4f} Acc: {:.4f}'.format(model_name, msg_dict["loss"], msg_dict["acc"]))   # MT:353
    print("------------------------" + print_tab + "-----------------------------")
    print("no targeted attack: " + msg_dict["attack acc"])
    prefix = str(label) + " to "
    for k, v in msg_dict.items():
        if k.startswith(prefix):
            print("ground truth class label: " + str(label) + ", now class label: " + k[len(prefix):] + "  ---  " + v)
    for k in ("e min", "e avg", "e max", "d l2 norm", "d l0 norm", "psnr min", "psnr max", "psnr avg"):        # MT:380-387
        print(">>>>>>>>  " + k + ": ", msg_dict[k])
    if something_need_log is not None:                                                            # MT:401-402
        msg_dict.update(something_need_log)
    print("------------------------" + print_tab + "-----------------------------")
    time_elapsed = time.time() - since
    print('Testing complete in {:.0f}m {:.0f}s'.format(time_elapsed // 60, time_elapsed % 60))
    return msg_dict


test_for_inception.__test__ = False          # a product function, not a pytest test
