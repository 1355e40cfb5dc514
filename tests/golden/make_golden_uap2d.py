#!/usr/bin/env python3
"""Fixture g29: the UAP-2D baseline (attack_UAP_2D.py:241-358 = UA) run through the REFERENCE's universal_2D_net and the
REFERENCE's deepfool.deepfool(universal_2d=True) on the CPU.

Run in the build container only (it imports the reference through make_golden.py, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_uap2d.py [--dry] [--verbose]

UA is a module-level script and cannot be imported; as for g27 / g28 its loop SHAPE is re-issued here (run_loop: the while loop
that steps `epoch` itself, the one table of UA:219 every view shares, the four running sums of UA:275-289, the skip test of
UA:297-304, the accumulation with the +-epsilon projection of UA:315-319, the jump of UA:335-338, the strict best rule of
UA:349-358 after EVERY pass, the export epoch of UA:262-270 / 322-333) around the reference's own universal_2D_net and
deepfool.deepfool, both imported exactly as make_golden.py imports them. Only DATA is written.

As in make_golden_nerfail.py a recording wrapper around the net keeps every forward of a deepfool call (with its graph); after
the call the generator differentiates those graphs once more and restates deepfool.py:53-66 / :79-101 on them to get, per
iteration, the bumped top-two gap, value_r of every competitor and the chosen class. The restatement is checked against the call:
the same number of iterations, and the table it predicts for the next forward equals the table deepfool passed to it.

Scene: g28's four 224 x 224 views (igsm2d_ref.g28_images) and EXTRA_TINTS more from a seed stream of their own
(uap2d_ref.g29_images), g15 / g24's stand-in classifier evaluated in float64 (PoolCls64) under model_name "vit_b_16" with the
identity resize of make_golden_igsm2d.py, df_max_iter = 3, four epochs, overshoot = 1.0 (this classifier's gradient norms are
tiny, as g27 explains). The rand-select loader of UA:198 is stood in for by each run's own draws per pass. Every run is made in
float32 and in float64 (PoolClsDouble, the table and everything derived from it in double).

Stored in g29_uap2d.npz: the scene's seeds and tints, the classifier, the constants, the draws; per run `<tag>_...`: per pass the
float64 run's table as float32 (tables) and max |float32 run - float64 run| (tables_dist), the pass records (passes: epoch, next
epoch, views, test loss, test acc, attack loss, attack acc, taken, test correct, attack correct; loss_f64: the float64 run's two
losses), per visit view / skipped / iter_k / the chosen classes (visits, uap2d_ref.visits_array), DeepFool iterations so far at
the end of every pass (iters_so_far), the best tensor and its distance, the number of the first export pass and its three
images per exported view - float64 run: the attacked image and the perturbation as float32, the clean image (whole numbers) as
uint8 - with their float32-vs-float64 distances.

Seeds and constants were found by trying them on the reference alone, until the generator's own conditions held. It FAILS unless,
across its runs: one run is untargeted and one targeted; some visit is skipped; some DeepFool call completes and some hits the cap;
some table element sits on +-epsilon; some pass-mask bit is cleared during a DeepFool forward (an element of ori + r outside
[0, 255]); some pass ties the best accuracy so far, so that the strict rule is exercised; the best tensor differs from the last
attacking pass's table in some run; a pass that changes nothing jumps to the export epoch in some run; the float32 and float64
runs take identical discrete decisions everywhere; every argmax a decision rests on (raw, for the skip and the statistics;
bumped, for the break) has a top-two gap >= 1e-3 max|logit|; the two smallest value_r of every iteration differ by >= 1e-3
relative."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (stubs the I/O-only packages and imports the reference's modules)
import make_golden_attack_loop as G24  # noqa: E402  (PoolCls64: g24's stand-in classifier)
import make_golden_igsm2d as G28  # noqa: E402  (_IdentityResize, items: MD:247-255 per view)
import make_golden_nerfail as G27  # noqa: E402  (PoolClsDouble, top_two_gap)
import deepfool as DF  # noqa: E402  (reference)
import uap2d_ref as UR  # noqa: E402  (tests/: the seeded images, the visit layout)

GN, T = MG.GN, MG.T
HW, C, EPOCHS, DF_MAX_ITER = 224, 8, 4, 3
SEED, TINTS, EXTRA_TINTS, CLS_SCALE = 28, (0.40, 0.46, 0.52, 0.58), (), 1.0
OVERSHOOT = 1.0
EXPORT_VIEWS = [2]
# tag, targeted, label, m1, m2, epsilon, draws per attack pass (pass number -> views; a pass not named draws every view)
RUNS = (('untargeted', False, 1, 1, 100, 8.0, {1: [2]}),
        ('targeted', True, 2, 1, 100, 8.0, {}))


def make_net(double):
    cls = G27.PoolClsDouble() if double else G24.PoolCls64()
    with torch.no_grad():
        cls.w.mul_(CLS_SCALE)
    for p_ in cls.parameters():
        p_.requires_grad = False
    net = GN.universal_2D_net('cpu', 0.02, cls, 'vit_b_16')
    net.torch_resize_224, net.torch_resize_299 = G28._IdentityResize([224, 224]), G28._IdentityResize([299, 299])
    return cls, net


class Recorder:
    """Stands where the net stands in deepfool.deepfool: every forward's table, live logits (graph kept) and their values."""

    def __init__(self, net):
        self.net, self.calls = net, []

    def __call__(self, r, ori):
        out = self.net(r, ori)
        v = out[3].to(r.dtype) + r.detach()
        self.calls.append((r, out[2], out[2].detach().clone(), out[4].detach().clone(), int(((v < 0) | (v > 255)).sum())))
        return out


def restate(calls, r0, target, m1, m2, gaps):
    """deepfool.py:53-101 with universal_2d on the recorded forwards: (loop_i, the chosen class per iteration, pass-mask bits
    cleared over the loop's forwards)."""
    classes, cleared = [], 0
    rot = torch.zeros_like(r0)
    loops = calls[1:]                                                    # calls[0] is deepfool.py:31
    for j, (r_var, cla_live, cla_raw, ori_raw, n_cleared) in enumerate(loops):
        cleared += n_cleared
        o = int(torch.max(ori_raw, 1)[1])
        b = cla_raw[0].clone()
        if target is None:
            b[o] = b[o] + m1
        else:
            b[:target] = b[:target] + m1
            b[target + 1:] = b[target + 1:] + m1
        gaps['bumped'].append(G27.top_two_gap(b.numpy()))
        am = int(torch.max(b, 0)[1])
        if (target is None and am != o) or (target is not None and am == target):
            assert j == len(loops) - 1, 'the restatement breaks where deepfool did not'
            return j, classes, cleared
        ks = [k for k in range(C) if k != o] if target is None else [target]
        g_o = torch.autograd.grad(cla_live[:, o].sum(), r_var, retain_graph=True)[0]
        vals, drs = [], []
        for k in ks:
            g = torch.autograd.grad(cla_live[:, k].sum(), r_var, retain_graph=True)[0] - g_o
            f = torch.abs(b[k] - (b[o] + m2))
            vals.append(float(f / (torch.norm(g) + 0.0001)))
            drs.append((f / ((torch.norm(g) ** 2) + 0.0001)) * g)
        best = int(np.argmin(vals))                                      # (first minimum = the strict < scan)
        if len(vals) > 1:
            v = np.sort(vals)
            gaps['value_r'].append(float((v[1] - v[0]) / v[1]))
        classes.append(ks[best])
        rot = (rot + drs[best]).detach()
        nxt = torch.clamp((r0 + OVERSHOOT * rot).detach(), -255, 255)    # all three channels: no alpha restore
        if j + 1 < len(loops):
            assert torch.equal(nxt, loops[j + 1][0].detach()), 'the restatement predicts another table than deepfool made'
    return len(loops), classes, cleared


def run_loop(double, views, label, targeted, m1, m2, epsilon, draws):
    """The UA:241-358 loop shape. Returns a dict of arrays and the gap lists."""
    dt = torch.float64 if double else torch.float32
    cls, net = make_net(double)
    criterion = torch.nn.CrossEntropyLoss()
    lab = torch.tensor(label)
    n_all = len(views)
    table = torch.zeros((HW, HW, 3), dtype=dt)                            # UA:219
    best = table.detach().clone()
    best_acc = 0 if targeted else 10000                                   # UA:234-237
    gaps = dict(raw=[], bumped=[], value_r=[])
    passes, tables, visits_all, iters_so_far = [], [], [], []
    seen = dict(cleared=0, on_eps=0, jumped=False, tie=False)
    last_attack, total_iters = table, 0
    out = {}
    epoch, n_pass = 0, 0
    while epoch < EPOCHS:
        assert n_pass < 16, 'the loop does not end'
        running_loss = attack_loss = 0.0
        running_corrects = attack_corrects = 0
        not_changed = True
        export = epoch == EPOCHS - 1
        order = list(EXPORT_VIEWS) if export else list(draws.get(n_pass, range(n_all)))
        n_views = len(order)                                              # len(now_dataloader.dataset)
        visits, ex = [], []
        pass_epoch = epoch
        for v in order:
            if export:
                table = best                                              # UA:269-270
                table.requires_grad = False
            ori_v = views[v].unsqueeze(0)
            x, r, cla, ori_f, ori_cla = net(table, ori_v)                 # UA:273 (x: the table, r: x_rgb)
            lab_r = lab.broadcast_to([ori_cla.size()[0], ])
            loss = criterion(ori_cla, lab_r)                              # UA:277-289
            running_loss += loss.item() * len(ori_f)
            running_corrects += int(torch.sum(torch.max(ori_cla, 1)[1] == lab_r))
            ae_loss = criterion(cla, lab_r)
            attack_loss += ae_loss.item() * len(ori_f)
            attack_corrects += int(torch.sum(torch.max(cla, 1)[1] == lab_r))
            gaps['raw'] += [G27.top_two_gap(cla[0].detach().numpy()), G27.top_two_gap(ori_cla[0].detach().numpy())]
            if not export:
                if torch.argmax(cla[0]) == torch.argmax(ori_cla[0]):      # UA:297-304
                    rec = Recorder(net)
                    target = label if targeted else None
                    dr, iter_k, _, _, _ = DF.deepfool((table, ori_v), epsilon, rec, max_iter=DF_MAX_ITER, target_label=target,
                                                      overshoot=OVERSHOOT, m1=m1, m2=m2, universal_2d=True)
                    k2, classes, cleared = restate(rec.calls, table.detach().clone(), target, m1, m2, gaps)
                    assert k2 == iter_k and len(classes) == iter_k, (k2, iter_k, classes)
                    seen['cleared'] += cleared
                    total_iters += iter_k
                    visits.append((v, False, iter_k, classes))
                    if iter_k < DF_MAX_ITER:                              # UA:315-319
                        table += dr
                        not_changed = False
                        table = torch.clamp(table, -epsilon, epsilon)     # project_perturbation(epsilon, inf, .)
                else:
                    visits.append((v, True, 0, []))
            else:
                ex.append((r[0].detach().numpy().copy(), x.detach().numpy().copy(), ori_f[0].detach().numpy().copy()))
                not_changed = False                                       # UA:333
        if not export:
            last_attack = table
            seen['on_eps'] = max(seen['on_eps'], int((table.abs() == epsilon).sum()))
        if not_changed:                                                   # UA:335-338
            seen['jumped'] |= epoch < EPOCHS - 2
            epoch = EPOCHS - 1
        else:
            epoch += 1
        acc = attack_corrects / n_views
        seen['tie'] |= acc == best_acc
        take = acc > best_acc if targeted else acc < best_acc             # UA:349-358: strict, after every pass
        if take:
            best_acc = acc
            best = table.clone().detach()
        if export and 'export' not in out:                                # the first export pass: what it rendered
            out.update(export=ex, export_pass=n_pass)
        passes.append([pass_epoch, epoch, n_views, running_loss / n_views, running_corrects / n_views, attack_loss / n_views, acc,
                       int(take), running_corrects, attack_corrects])
        tables.append(table.detach().numpy().copy())
        visits_all.append(visits)
        iters_so_far.append(total_iters)
        if '--verbose' in sys.argv:
            print('   pass %d epoch %d -> %d acc %.3f take %d visits %s on eps %d' % (
                n_pass, pass_epoch, epoch, acc, take, [('s' if s else k, c) for _, s, k, c in visits], seen['on_eps']), flush=True)
        n_pass += 1
    out.update(passes=np.array(passes, np.float64), tables=np.stack(tables), visits=UR.visits_array(visits_all, DF_MAX_ITER, n_all),
               iters_so_far=np.array(iters_so_far), best=best.numpy().copy(), last_attack=last_attack.detach().numpy().copy(),
               best_acc=best_acc)
    return out, gaps, seen


def g29(save=True):
    images = UR.g29_images(SEED, TINTS, EXTRA_TINTS)
    views = G28.items(images)
    cls, _ = make_net(False)
    common = dict(seed=SEED, tints=np.asarray(TINTS, np.float64), extra_tints=np.asarray(EXTRA_TINTS, np.float64),
                  cls_w=cls.w.detach().numpy(), shape=np.array([len(images), HW, HW, C, EPOCHS, DF_MAX_ITER]), overshoot=OVERSHOOT,
                  export_views=np.array(EXPORT_VIEWS), tags=np.array([r[0] for r in RUNS]),
                  targeted=np.array([int(r[1]) for r in RUNS]), label=np.array([r[2] for r in RUNS]), m1=np.array([r[3] for r in RUNS]),
                  m2=np.array([r[4] for r in RUNS]), epsilon=np.array([r[5] for r in RUNS], np.float64),
                  **{'draws_%s_%d' % (r[0], k): np.array(v) for r in RUNS for k, v in r[6].items()})
    seen = dict(untargeted=False, targeted=False, skipped=False, completed=False, capped=False, on_eps=False, cleared=False, tie=False,
                best_ne_last=False, jumped=False)
    all_gaps = dict(raw=[], bumped=[], value_r=[])
    dist = lambda a, b: float(np.abs(a.astype(np.float64) - b).max())  # noqa: E731
    for tag, targeted, label, m1, m2, epsilon, draws in RUNS:
        r32, gaps32, seen32 = run_loop(False, views, label, targeted, m1, m2, epsilon, draws)
        r64, gaps64, seen64 = run_loop(True, views, label, targeted, m1, m2, epsilon, draws)
        assert np.array_equal(r32['visits'], r64['visits']), '%s: the float32 and float64 runs differ in a visit' % tag
        dec = [0, 1, 2, 4, 6, 7, 8, 9]                                    # every discrete column of a pass record
        assert r32['passes'].shape == r64['passes'].shape and np.array_equal(r32['passes'][:, dec], r64['passes'][:, dec]), \
            '%s: the float32 and float64 runs differ in a pass record' % tag
        for g_ in (gaps32, gaps64):
            for k in all_gaps:
                all_gaps[k] += g_[k]
        v = r32['visits']
        attack_rows = v[r32['passes'][:, 0] < EPOCHS - 1]
        seen['targeted' if targeted else 'untargeted'] = True
        seen['skipped'] |= bool((attack_rows[..., 1] == 1).any())
        seen['completed'] |= bool(((attack_rows[..., 1] == 0) & (attack_rows[..., 2] < DF_MAX_ITER)).any())
        seen['capped'] |= bool(((attack_rows[..., 1] == 0) & (attack_rows[..., 2] == DF_MAX_ITER)).any())
        seen['on_eps'] |= seen32['on_eps'] > 0 and seen64['on_eps'] > 0
        seen['cleared'] |= seen32['cleared'] > 0 and seen64['cleared'] > 0
        seen['tie'] |= seen32['tie']
        seen['jumped'] |= seen32['jumped']
        seen['best_ne_last'] |= not np.array_equal(r32['best'], r32['last_attack'])
        arrs = dict(passes=r32['passes'], loss_f64=r64['passes'][:, [3, 5]], visits=v, iters_so_far=r32['iters_so_far'],
                    tables=r64['tables'].astype(np.float32),
                    tables_dist=np.array([dist(a, b) for a, b in zip(r32['tables'], r64['tables'])]),
                    best=r64['best'].astype(np.float32), best_dist=dist(r32['best'], r64['best']), best_acc=r32['best_acc'],
                    export_pass=r32['export_pass'])
        for k, name in enumerate(('adv', 'mask', 'ori')):
            img = np.stack([e[k] for e in r64['export']])
            if name == 'ori':                                             # the clean image: whole numbers in 0..255
                assert np.array_equal(img.astype(np.uint8), img)
            arrs['export_' + name] = img.astype(np.uint8 if name == 'ori' else np.float32)
            arrs['export_%s_dist' % name] = max(dist(a[k], b[k]) for a, b in zip(r32['export'], r64['export']))
        common.update({'%s_%s' % (tag, k): a for k, a in arrs.items()})
        p = r32['passes']
        print('g29 %-10s passes %d epochs %s -> %s acc %s taken %s' % (tag, len(p), p[:, 0].astype(int).tolist(), p[:, 1].astype(int).tolist(),
                                                                       np.round(p[:, 6], 3).tolist(), p[:, 7].astype(int).tolist()))
        print('    visits per pass (view, skipped, iter_k): %s' % [[tuple(int(x) for x in row[:3]) for row in ps if row[0] >= 0] for ps in v])
        print('    elements on +-epsilon %d, mask bits cleared in DeepFool forwards %d, best != last attack table: %s'
              % (seen32['on_eps'], seen32['cleared'], not np.array_equal(r32['best'], r32['last_attack'])))
        print('    smallest gaps of the run: %s' % {k: '%.2e' % min(gaps32[k] + gaps64[k]) for k in gaps32 if gaps32[k]})
        print('    table distance f32 - f64 per pass %s' % np.array2string(arrs['tables_dist'], precision=2))
    mins = {k: (min(v) if v else float('inf')) for k, v in all_gaps.items()}
    print('g29 conditions %s; smallest gaps: raw %.2e bumped %.2e of max|logit|, value_r %.2e relative' %
          (seen, mins['raw'], mins['bumped'], mins['value_r']))
    for k, ok in seen.items():
        assert ok, 'condition not met: %s' % k
    assert mins['raw'] >= 1e-3 and mins['bumped'] >= 1e-3, 'an argmax rests on a gap below 1e-3 max|logit|'
    assert mins['value_r'] >= 1e-3, 'two value_r of one iteration are closer than 1e-3 relative'
    if save:
        MG.save('g29_uap2d', **common)


if __name__ == '__main__':
    g29(save='--dry' not in sys.argv)
