#!/usr/bin/env python3
"""Fixture g28: the IGSM-2D loop (attack_IGSM_2D.py:263-416 = IG) run through the REFERENCE's universal_2D_net on the CPU.

Run in the build container only (it imports the reference through make_golden.py, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_igsm2d.py

IG is a module-level script and cannot be imported; as for g15 / g24 its loop SHAPE is re-issued here around the reference's own
universal_2D_net (model/GaussNet.py:340-385, imported exactly as make_golden.py imports it) with torch's CrossEntropyLoss /
MSELoss: the table of IG:250-253, per batch the gather of IG:290-301, the statistics of IG:306-331 (float32 batch losses read
with .item() and accumulated in Python floats), the backward and the sign step with the +-epsilon clamp of IG:335-379 as the
reference writes them (cat + max / min), the epoch means of IG:392-400, the strict best rule of IG:407-416 and the last epoch
of IG:286-301, 381-390 that runs the best table without gradient. The dataset items are what MD:247-255 builds from the seeded
images of tests/igsm2d_ref.py (cv2 is absent here, so that torch.where is issued on the seeded arrays). Only DATA is written.

torchvision is absent. Its Resize is stood in for ONLY by an identity that refuses any image not already at the requested size
(make_golden_eval.py's _IdentityResize is the precedent): model_name = "vit_b_16" and 224 x 224 views make Resize([224, 224])
that identity, which is the reference's own behaviour (torchvision returns such an image unchanged).

Shapes: 4 views of 224 x 224 - views 0 and 2 BGRA with transparent regions, views 1 and 3 with alpha 255 everywhere - in batches
of 3 + 1, 4 epochs (3 attack epochs + the export epoch), g15 / g24's stand-in classifier evaluated in float64 (PoolCls64). Two
runs, untargeted and targeted, each in float32 and in float64 (the table and everything derived from it in double).

Stored per run `<tag>_...`: the best and the last table as int8 multiples of a, two float64 checksums per view of every iterate
(igsm2d_ref.checksums), all logits, every epoch's statistics as the reference computes them (f32) and recomputed in float64 from
the same logits and images, the taken flags, the best epoch, and the export pass's two uint8 images of view EXPORT_VIEW.

The generator FAILS unless, on the reference alone: (a) in some run best != last; (b) some epoch ties the best accuracy so far,
so that the strict rule is exercised; (c) over every recorded view the gap between the two largest logits is >= 1e-3 max|logit|;
(d) every non-zero gradient element of every batch has magnitude >= 1e-6 of that batch's largest, so that no sign rests on
rounding - the float32 and the float64 run then produce identical iterates, which is asserted. Seeds, tints, the classifier's
scale, a and epsilon were found by trying them on the reference alone until (a)-(d) held."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (stubs the I/O-only packages and imports the reference's modules)
import make_golden_attack_loop as G24  # noqa: E402  (PoolCls64, ce_f64)
import attack_loop_ref as R  # noqa: E402  (tests/: export_u8, cv2.imwrite's conversion)
import igsm2d_ref as IR  # noqa: E402  (tests/: the seeded images, the checksums)

GN, T = MG.GN, MG.T
N, HW, C, EPOCHS, BATCH = IR.G28_N, IR.G28_HW, IR.G28_C, IR.G28_EPOCHS, IR.G28_BATCH
SEED, TINTS, CLS_SCALE, A, EPSILON = 28, (0.40, 0.46, 0.52, 0.58), 1.0, 16.0, 48.0
RUNS = (('untargeted', False, 1), ('targeted', True, 2))                  # tag, targeted, label: every clean view is class 1, class 2 the runner-up
EXPORT_VIEW = 2


class _IdentityResize(torch.nn.Module):
    def __init__(self, size):
        super().__init__()
        self.size = list(size)

    def forward(self, x):
        assert list(x.shape[-2:]) == self.size, 'only the identity resize is the reference\'s own here (%s -> %s)' % (tuple(x.shape), self.size)
        return x


def make_net(scale):
    cls = G24.PoolCls64()
    with torch.no_grad():
        cls.w.mul_(scale)
    net = GN.universal_2D_net('cpu', 0.02, cls, 'vit_b_16')
    net.torch_resize_224, net.torch_resize_299 = _IdentityResize([224, 224]), _IdentityResize([299, 299])
    return cls, net


def items(images):
    """MD:247-255 per view: uint8 [H,W,3] on the white background."""
    out = []
    for img in images:
        ori_img = T(img)
        alpha = ori_img[:, :, 3].unsqueeze(-1).broadcast_to([ori_img.size()[0], ori_img.size()[1], 3])
        rgb = ori_img[:, :, :3]
        out.append(torch.where(alpha > 0, rgb, torch.ones_like(rgb) * 255))
    return out


def run_loop(net, model, views, label, targeted, a, epsilon, dtype):
    """The IG:263-416 loop shape. Returns a dict of arrays and the smallest |gradient| / largest |gradient| over the batches."""
    criterion = torch.nn.CrossEntropyLoss()
    img_rgba_loss = torch.nn.MSELoss()
    lab = torch.tensor(label)
    n = len(views)
    batches = [list(range(lo, min(lo + BATCH, n))) for lo in range(0, n, BATCH)]        # DataLoader(batch_size, no shuffle)
    table_all = torch.zeros((n, HW, HW, 3), dtype=dtype)                                  # IG:250-253
    init_all = table_all.clone().detach()
    best_all = table_all.clone().detach()
    best_acc = 0 if targeted else 10000                                                   # IG:255-261
    best_epoch = -1
    out = dict(sums=[], stats_f32=[], stats_f64=[], taken=[], ori_cla=[], cla=[])
    grad_ratio = np.inf
    for epoch in range(EPOCHS):
        model.train(False)                                                                # IG:266-272
        net.train(False)
        for param in model.parameters():
            param.requires_grad = False
        export = epoch == EPOCHS - 1
        running_loss = attack_loss = attack_img_loss = attack_total_loss = 0.0
        running_corrects = attack_corrects = 0
        ce64, sq64 = np.zeros(2), 0.0
        ep_ori_cla, ep_cla = [], []
        for ib in batches:                                                                # IG:289
            index = torch.tensor(ib)
            ori_img = torch.stack([views[i] for i in ib])
            t = table_all[index, :, :, :]                                                 # IG:290-292
            t_init = init_all[index, :, :, :]
            if not export:
                t = t.clone().detach().requires_grad_(True)                               # IG:295-296
            else:
                t = best_all[index, :, :, :]                                              # IG:300-301
                t.requires_grad = False
            x, r, cla, ori_f, ori_cla = net(t, ori_img)                                   # IG:304 (x: the perturbation, r: x_rgb)
            lab_r = lab.broadcast_to([ori_cla.size()[0], ])
            loss = criterion(ori_cla, lab_r)                                              # IG:308-313
            _, preds = torch.max(ori_cla, 1)
            running_loss += loss.item() * len(ori_f)
            running_corrects += int(torch.sum(preds == lab_r))
            ae_loss = criterion(cla, lab_r)                                               # IG:315-317
            img_pixel_loss = img_rgba_loss(r, ori_f.to(r.dtype))
            _, ae_preds = torch.max(cla, 1)
            total_loss = (1 * ae_loss) + (0 * img_pixel_loss)                             # IG:319-323 with beta = 0 (IG:69)
            attack_loss += ae_loss.item() * len(ori_f)
            attack_img_loss += img_pixel_loss.item() * len(ori_f)
            attack_total_loss += total_loss.item() * len(ori_f)
            attack_corrects += int(torch.sum(ae_preds == lab_r))
            ce64 += [G24.ce_f64(ori_cla.detach().numpy(), label).sum(), G24.ce_f64(cla.detach().numpy(), label).sum()]
            sq64 += float(((r.detach().double() - ori_f.double()) ** 2).mean()) * len(ib)
            ep_ori_cla.append(ori_cla.detach().float().numpy().copy())
            ep_cla.append(cla.detach().float().numpy().copy())
            if not export:
                total_loss.backward(retain_graph=True)                                    # IG:335
                g = t.grad.data
                nz = g[g != 0].abs()
                grad_ratio = min(grad_ratio, float(nz.min() / nz.max()))
                if targeted:                                                              # IG:343-352
                    t2 = t - a * torch.sign(g)
                else:
                    t2 = t + a * torch.sign(g)
                t_max = t_init + epsilon                                                  # IG:370-377
                t_min = t_init - epsilon
                temp = torch.cat([t2.unsqueeze(0), t_min.unsqueeze(0)], 0)
                t2 = torch.max(temp, dim=0)[0]
                temp = torch.cat([t2.unsqueeze(0), t_max.unsqueeze(0)], 0)
                t2 = torch.min(temp, dim=0)[0]
                table_all[index, :, :, :] = t2.clone().detach()                           # IG:379
                out['sums'].append(IR.checksums(table_all.numpy()))
            elif EXPORT_VIEW in ib:                                                       # IG:381-390: what cv2.imwrite stores
                k = ib.index(EXPORT_VIEW)
                out['export_adv_u8'] = R.export_u8(r[k].detach().numpy())
                out['export_mask_u8'] = R.export_u8(x[k].detach().numpy())
        acc = attack_corrects / n                                                         # IG:392-400
        out['stats_f32'].append([running_loss / n, running_corrects / n, attack_loss / n, acc, attack_img_loss / n,
                                 attack_total_loss / n, n, running_corrects, attack_corrects])
        out['stats_f64'].append([ce64[0] / n, ce64[1] / n, sq64 / n])
        out['ori_cla'].append(np.concatenate(ep_ori_cla))
        out['cla'].append(np.concatenate(ep_cla))
        if export:
            out['best'] = best_all.numpy().copy()                                         # what the export epoch rendered
            out['best_epoch'] = best_epoch
        take = acc > best_acc if targeted else acc < best_acc                             # IG:407-416: strict
        out['taken'].append(int(take))
        if take:
            best_acc, best_epoch = acc, epoch
            best_all = table_all.clone().detach()
    out['last'] = table_all.numpy().copy()
    for k in ('sums', 'stats_f32', 'stats_f64', 'taken', 'ori_cla', 'cla'):
        out[k] = np.asarray(out[k], np.float64 if k.startswith('s') else None)
    return out, grad_ratio


def as_int8(table, a):
    q = np.asarray(table, np.float64) / a
    assert np.array_equal(q, np.rint(q)) and np.abs(q).max() <= 127, 'the table is not a small multiple of a'
    return q.astype(np.int8)


def tie_with_best(run, targeted):
    """(b): some attack epoch's accuracy equals the best before it."""
    best, hit = (0 if targeted else 10000), False
    for v in run['stats_f32'][:EPOCHS - 1, 3]:
        hit |= v == best
        if (v > best) if targeted else (v < best):
            best = v
    return hit


def min_gap(run):
    rows = np.concatenate([run[k].reshape(-1, C) for k in ('ori_cla', 'cla')])
    top = np.sort(rows.astype(np.float64), 1)
    return float((top[:, -1] - top[:, -2]).min() / np.abs(rows).max())


def generate(seed=SEED, tints=TINTS, scale=CLS_SCALE, a=A, epsilon=EPSILON, runs=RUNS, quiet=False):
    """Runs everything and checks (a)-(d). Returns (arrays, ok, why)."""
    images = IR.g28_images(seed, tints)
    views = items(images)
    cls, net = make_net(scale)
    arrs = dict(seed=seed, tints=np.asarray(tints, np.float64), cls_w=cls.w.detach().numpy(), a=a, epsilon=epsilon,
                shape=np.array([N, HW, HW, C, EPOCHS, BATCH]), tags=np.array([r[0] for r in runs]),
                targeted=np.array([int(r[1]) for r in runs]), label=np.array([r[2] for r in runs]), export_view=EXPORT_VIEW)
    differ = tie = False
    gaps, ratios = [], []
    for tag, targeted, label in runs:
        run, ratio = run_loop(net, cls, views, label, targeted, a, epsilon, torch.float32)
        run64, ratio64 = run_loop(net, cls, views, label, targeted, a, epsilon, torch.float64)
        same = (np.array_equal(run['sums'], run64['sums']) and np.array_equal(run['best'], run64['best'])
                and np.array_equal(run['last'], run64['last']) and np.array_equal(run['taken'], run64['taken']))
        if not same:
            return arrs, False, '%s: the float32 and the float64 run differ' % tag
        differ |= not np.array_equal(run['best'], run['last'])
        tie |= tie_with_best(run, targeted)
        gaps.append(min_gap(run))
        ratios.append(min(ratio, ratio64))
        if not quiet:
            print('g28 %-10s attack acc per epoch %s taken %s best epoch %d, best != last: %s, tie: %s, min top-two gap %.2e of max|logit|, '
                  'smallest / largest gradient %.2e' % (tag, run['stats_f32'][:, 3].tolist(), run['taken'].tolist(), run['best_epoch'],
                                                        not np.array_equal(run['best'], run['last']), tie_with_best(run, targeted),
                                                        gaps[-1], ratios[-1]))
            print('    f32 stats - f64 stats (test CE, attack CE, image loss), worst over epochs: %s'
                  % np.abs(run['stats_f32'][:, [0, 2, 4]] - run['stats_f64']).max(0))
        for k, v in run.items():
            arrs['%s_%s' % (tag, k)] = as_int8(v, a) if k in ('best', 'last') else v
    if not differ:
        return arrs, False, '(a) best == last in every run'
    if not tie:
        return arrs, False, '(b) no epoch ties the best accuracy: the strict rule is not exercised'
    if min(gaps) < 1e-3:
        return arrs, False, '(c) an argmax rests on a top-two gap of %.2e max|logit|' % min(gaps)
    if min(ratios) < 1e-6:
        return arrs, False, '(d) a gradient element is %.2e of its batch\'s largest: a sign may rest on rounding' % min(ratios)
    return arrs, True, ''


def g28():
    arrs, ok, why = generate()
    assert ok, why
    MG.save('g28_igsm2d', **arrs)


if __name__ == '__main__':
    g28()
