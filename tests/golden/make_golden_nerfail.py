#!/usr/bin/env python3
"""Fixture g27: the NeRFail universal attack (attack_NeRFail.py:269-512 = AN) run through the REFERENCE's gauss_net and the
REFERENCE's deepfool.deepfool on the CPU.

Run in the build container only (it imports the reference through make_golden.py, which never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nerfail.py

AN is a module-level script and cannot be imported; as for g15 and g24 its loop SHAPE is re-issued here (run_loop: the while loop
that steps `epoch` itself, the four running sums of AN:358-376, the skip test of AN:387-394, the accumulation and the m2 rule of
AN:405-418, the m1_list bisection of AN:434-472, the best rule of AN:490-503, the export epoch) around the reference's own
gauss_net and deepfool.deepfool, both imported exactly as make_golden.py imports them. Only DATA is written.

deepfool.deepfool does not say which class it chose in an iteration. A recording wrapper around the net keeps every forward's
table and logits (with their graph, which deepfool retains); after the call the generator differentiates those same graphs
once more and restates deepfool.py:53-66 / :79-86 on them to get, per iteration: the bumped top-two gap, value_r of every
competitor, the chosen class. The restatement is checked against the call: the same number of iterations, and the table it
predicts for the next forward equals the table deepfool passed to it.

Shapes: those of g24 - P = 3, H = W = 32, 8 classes, the g15 / g24 stand-in classifier (evaluated in float64, PoolCls64 of
make_golden_attack_loop.py; weights x 0.8). 12 views per pass (the m2 rule needs more than 10 DeepFool calls), the first two of
them again in the export pass; df_max_iter = 3; four epochs; overshoot = 1.0 - this classifier's gradient norms are tiny
(||g||^2 far below the 1e-4 of deepfool.py:85's denominator), so with the reference's default 0.02 no call completes within three
iterations. Five runs, each made in float32 and in float64:
    untargeted, targeted, m2_raise (m2 too small: the rule of AN:410-418 raises it),
    bisect (m1 = 2 is out of reach of the eleven views pass 0 draws, so pass 0 changes nothing and AN:442-453 halves m1; passes 1
    and 2 draw a thirteenth view alone; after the export epoch AN:456-468 takes m1 back up, on the best tensor, and the m2 raise
    lets the twelfth call of that pass complete - the reference's loop never ends when the m1 that failed keeps failing),
    one_by_one (a loader that draws one clean view per pass: every pass sees accuracy 1, AN:498 never takes, best != last).

Stored: g27_nerfail.npz - the scene (table, uint8 images, the map as weights + uint16 rows), the classifier, the constants, the
draws; g27_nerfail_<run>.npz per run: per pass the float64 run's table (rgb, as float32) and max |float32 run - float64 run|, the
pass's record (epoch, next epoch, m1 of the pass, m1 / m2 at its end, views, the means, taken, m2 raises, correct counts), per
visit skip / iter_k / the chosen classes / the raw logits, per loop forward the raw logits, the competitors' gradient-difference
norms and the scale (both precisions), the best tensor, the table of the last attacking pass, and the first export pass's x and
x_rgba (float64 run, as float32) with their float32-vs-float64 distances.

Seeds and constants were found by trying them on the reference alone (the classifier scale, overshoot, the runs' m1 / m2 and
draws below), until the generator's own conditions held. It FAILS unless: some visit is skipped; some DeepFool call completes and
some hits the cap; m2 is raised in m2_raise; m1 moves down and back up in bisect; the best tensor differs from the last attacking
pass's table in at least one run; the float32 and float64 runs take identical discrete decisions everywhere; every argmax a
decision rests on (raw, for the skip; bumped, for the break) has a top-two gap >= 1e-3 max|logit|; the two smallest value_r of
every iteration differ by >= 1e-3 relative."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (stubs the I/O-only packages and imports the reference's modules)
import make_golden_attack_loop as G24  # noqa: E402  (PoolCls64: g24's stand-in classifier)
import deepfool as DF  # noqa: E402  (reference)

GN, T = MG.GN, MG.T

P, H, W, C = 3, 32, 32, 8
VIEWS, EXPORT_VIEWS, EPOCHS, DF_MAX_ITER = 12, 2, 4, 3
M2_MAX_LIMIT = 10000
# bisect's draws: pass 0 misses the one view within reach of m1 = 2 on the clean table, passes 1 and 2 draw the thirteenth view alone
BISECT_DRAWS = {0: [v for v in range(VIEWS) if v != 1], 1: [VIEWS], 2: [VIEWS]}
# one_by_one's draws: one clean view per pass. Every pass then sees an accuracy of 1, which the rule of AN:498 never takes: the best
# tensor stays the initial table while the table moves (best != last)
ONE_BY_ONE_DRAWS = {0: [1], 1: [2], 2: [3]}
OVERSHOOT = 1.0
SEED = 27
CLS_SCALE = 0.8
# tag, targeted, label, m1, m2, m2_max_limit[, draws]
RUNS = (('untargeted', False, 1, 1, 110, M2_MAX_LIMIT), ('targeted', True, 6, 1, 80, M2_MAX_LIMIT), ('m2_raise', False, 1, 1, 30, M2_MAX_LIMIT),
        ('bisect', False, 1, 2, 100, M2_MAX_LIMIT, BISECT_DRAWS), ('one_by_one', False, 1, 1, 105, M2_MAX_LIMIT, ONE_BY_ONE_DRAWS))


def scene(seed=SEED):
    """g24's recipe with 12 views: zero rgb table with 85 % opaque rows, random images with a brightness of their own."""
    rs = np.random.RandomState(seed)
    s0 = np.zeros((P, H, W, 4), np.float32)
    s0[..., 3] = np.where(rs.uniform(size=(P, H, W)) < 0.85, 255.0, 0.0)
    ori = MG.synth.disc_alpha_image(VIEWS, H, W, seed=seed + 1)
    tint = rs.uniform(0.3, 0.7, size=(VIEWS, 1, 1, 3)).astype(np.float32)
    ori[..., :3] = np.floor(ori[..., :3] * tint)
    dist = np.sort(np.abs(rs.normal(scale=0.02, size=(VIEWS, H, W, 8))).astype(np.float32), -1)
    idx = rs.randint(0, P * H * W, size=(VIEWS, H, W, 8)).astype(np.float32)
    # one more view, from a stream of its own (the twelve above do not move): only run `bisect` draws it
    rx = np.random.RandomState(seed + 100)
    ori_x = MG.synth.disc_alpha_image(1, H, W, seed=seed + 101)
    ori_x[..., :3] = np.floor(ori_x[..., :3] * rx.uniform(0.3, 0.7, size=(1, 1, 1, 3)).astype(np.float32))
    dist = np.concatenate([dist, np.sort(np.abs(rx.normal(scale=0.02, size=(1, H, W, 8))).astype(np.float32), -1)])
    idx = np.concatenate([idx, rx.randint(0, P * H * W, size=(1, H, W, 8)).astype(np.float32)])
    ori = np.concatenate([ori, ori_x])
    with torch.no_grad():
        wi, _ = GN.create_gauss_w('cpu', 0.02)(T(np.stack([dist, idx], 1)))
    return s0, ori, wi


class PoolClsDouble(G24.PoolCls64):
    """The same classifier left in float64: the float64 runs."""

    def forward(self, x):
        p = torch.nn.functional.adaptive_avg_pool2d(x.double(), 4).reshape(x.shape[0], -1)
        return p @ self.w.double().t()


def make_net(double):
    cls = PoolClsDouble() if double else G24.PoolCls64()
    with torch.no_grad():
        cls.w.mul_(CLS_SCALE)
    for p_ in cls.parameters():
        p_.requires_grad = False
    return cls, GN.gauss_net('cpu', 0.02, cls, 'my_model', epsilon=None)


class Recorder:
    """Stands where the net stands in deepfool.deepfool: every forward's table, live logits (graph kept) and their values."""

    def __init__(self, net):
        self.net, self.calls = net, []

    def __call__(self, s, wi, ori):
        out = self.net(s, wi, ori)
        self.calls.append((s, out[2], out[2].detach().clone(), out[4].detach().clone()))
        return out


def top_two_gap(row):
    v = np.sort(np.asarray(row, np.float64))
    return float(v[-1] - v[-2]) / float(np.abs(row).max())


def restate(calls, s0, target, m1, m2, gaps):
    """deepfool.py:53-105 on the recorded forwards: per loop iteration the chosen class (and the two checks on gaps). Returns
    (loop_i, classes, details): details per loop forward = (raw logits, norms of the competitors' gradient differences, scale)."""
    classes, details = [], []
    rot = torch.zeros_like(s0)
    loops = calls[1:]                                                    # calls[0] is deepfool.py:33
    for j, (s_var, cla_live, cla_raw, ori_raw) in enumerate(loops):
        o = int(torch.max(ori_raw, 1)[1])
        b = cla_raw[0].clone()
        if target is None:
            b[o] = b[o] + m1
        else:
            b[:target] = b[:target] + m1
            b[target + 1:] = b[target + 1:] + m1
        gaps['bumped'].append(top_two_gap(b.numpy()))
        am = int(torch.max(b, 0)[1])
        if (target is None and am != o) or (target is not None and am == target):
            assert j == len(loops) - 1, 'the restatement breaks where deepfool did not'
            details.append((cla_raw[0].numpy().astype(np.float64), np.zeros(C - 1), 0.0))
            return j, classes, details
        ks = [k for k in range(C) if k != o] if target is None else [target]
        g_o = torch.autograd.grad(cla_live[:, o].sum(), s_var, retain_graph=True)[0]
        vals, drs, nrms, scs = [], [], [], []
        for k in ks:
            g = torch.autograd.grad(cla_live[:, k].sum(), s_var, retain_graph=True)[0] - g_o
            f = torch.abs(b[k] - (b[o] + m2))
            vals.append(float(f / (torch.norm(g) + 0.0001)))
            nrms.append(float(torch.norm(g)))
            scs.append(f / ((torch.norm(g) ** 2) + 0.0001))
            drs.append(scs[-1] * g)
        best = int(np.argmin(vals))                                      # (first minimum = the strict < scan)
        if len(vals) > 1:
            v = np.sort(vals)
            gaps['value_r'].append(float((v[1] - v[0]) / v[1]))
        classes.append(ks[best])
        details.append((cla_raw[0].numpy().astype(np.float64), np.array(nrms + [0.0] * (C - 1 - len(nrms))),
                        float(scs[best])))
        rot = (rot + drs[best]).detach()
        nxt = torch.clamp((s0 + OVERSHOOT * rot).detach(), -255, 255)
        nxt = torch.cat([nxt[..., :3], s0[..., 3:]], -1)
        if j + 1 < len(loops):
            assert torch.equal(nxt, loops[j + 1][0].detach()), 'the restatement predicts another table than deepfool made'
    return len(loops), classes, details


def pass_views(subsample, n_pass):
    """The views of attack pass n_pass, in order: all twelve, or - the stand-in of the subsampling loader
    gauss_dataset_rand_select (AN:246-249), whose draw differs from pass to pass - the run's own draws for its first passes."""
    return list(subsample.get(n_pass, range(VIEWS))) if subsample else list(range(VIEWS))


def run_loop(double, s0_np, wi, ori_np, label, targeted, m1, m2_arg, m2_max_limit=M2_MAX_LIMIT, subsample=False):
    """The AN:269-505 loop shape. Returns a dict of arrays and the gap lists."""
    dt = torch.float64 if double else torch.float32
    cls, net = make_net(double)
    criterion = torch.nn.CrossEntropyLoss()
    lab = torch.tensor([label])
    table = T(s0_np).to(dt).clone()                                      # change_target_tensor (zero_init_mask is what s0 is)
    best = table.detach().clone()
    wi = wi.to(dt)
    best_acc = 0 if targeted else 10000                                  # AN:294-303
    m1_best = m2_best = 0
    m1_list = [0, m1]
    epoch, n_pass = 0, 0
    gaps = dict(raw=[], bumped=[], value_r=[])
    passes, tables, visits_all, logits_all, it_all = [], [], [], [], []
    last_attack = table
    out = {}
    while epoch < EPOCHS:
        assert n_pass < 16, 'the loop does not end'
        running_loss = attack_loss = 0.0
        running_corrects = attack_corrects = 0
        no_attack = attack_all = 0
        m2 = m2_arg                                                      # AN:332
        not_changed = True
        export = epoch == EPOCHS - 1
        order = list(range(EXPORT_VIEWS)) if export else pass_views(subsample, n_pass)
        n_views = len(order)                                             # len(now_dataloader.dataset)
        visits = np.full((VIEWS + 1, 2 + DF_MAX_ITER), -1, np.int64)          # skipped, iter_k, classes
        logits = np.zeros((VIEWS + 1, 2, C), np.float64)
        its = np.zeros((VIEWS + 1, DF_MAX_ITER, C + (C - 1) + 1), np.float64)   # per loop forward: raw logits, norms, scale
        raises = 0
        ex_x, ex_r = [], []
        pass_epoch, pass_m1 = epoch, m1
        for v in order:
            if export:
                table = best                                             # AN:345
                table.requires_grad = False
            wi_v, ori_v = wi[v:v + 1], T(ori_np[v:v + 1])
            net.open_update_epsilon_3d()
            x, r, cla, ori_f, ori_cla = net(table, wi_v, ori_v)          # AN:354
            lab_r = lab.broadcast_to([ori_cla.size()[0], ])
            loss = criterion(ori_cla, lab_r)
            running_loss += loss.item() * len(ori_f)
            running_corrects += int(torch.sum(torch.max(ori_cla, 1)[1] == lab_r))
            ae_loss = criterion(cla, lab_r)
            attack_loss += ae_loss.item() * len(ori_f)
            attack_corrects += int(torch.sum(torch.max(cla, 1)[1] == lab_r))
            logits[v, 0], logits[v, 1] = cla[0].detach().numpy(), ori_cla[0].detach().numpy()
            gaps['raw'] += [top_two_gap(logits[v, 0]), top_two_gap(logits[v, 1])]
            if not export:
                net.close_update_epsilon_3d()
                if torch.argmax(cla[0]) == torch.argmax(ori_cla[0]):      # AN:387-394
                    rec = Recorder(net)
                    target = label if targeted else None
                    dr, iter_k, _, _, _ = DF.deepfool((table, wi_v, ori_v), None, rec, max_iter=DF_MAX_ITER, target_label=target,
                                                      overshoot=OVERSHOOT, m1=m1, m2=m2)
                    k2, classes, details = restate(rec.calls, table.detach().clone(), target, m1, m2, gaps)
                    assert k2 == iter_k and len(classes) == iter_k, (k2, iter_k, classes)
                    visits[v, 0], visits[v, 1] = 0, iter_k
                    visits[v, 2:2 + iter_k] = classes
                    for j, d_ in enumerate(details[:DF_MAX_ITER]):
                        its[v, j] = np.concatenate([d_[0], d_[1], [d_[2]]])
                    if iter_k < DF_MAX_ITER:                             # AN:405 (accumulated_incomplete_attack = False)
                        table += dr
                        not_changed = False
                        attack_all += 1
                    elif m2 < m2_max_limit:
                        no_attack += 1
                        attack_all += 1
                        if attack_all > 10 and (no_attack / attack_all) > 0.5:
                            m2 = m2 * 10
                            raises += 1
                            no_attack = attack_all = 0
                else:
                    visits[v, 0], visits[v, 1] = 1, 0
            else:
                ex_x.append(x.detach().numpy().copy())
                ex_r.append(r.detach().numpy().copy())
                not_changed = False                                      # AN:432
        if not export:
            last_attack = table
        if not_changed:                                                  # AN:434-472
            if m1_list[0] < m1 - 1 and epoch == 0:
                m1_list[1] = m1
                m1 = int((m1 + m1_list[0]) / 2)
                m2 = m2_arg
                epoch = 0
            elif m1_list[0] < m1 and epoch == 0:
                m1_list[1] = m1
                m1 = m1_list[0]
                m2 = m2_arg
                epoch = 0
            else:
                epoch = EPOCHS - 1
        elif epoch == EPOCHS - 1:
            if m1 < m1_list[1] - 1:
                m1_list[0] = m1
                m1 = int((m1 + m1_list[1]) / 2)
                m2 = m2_arg
                epoch = 0
            elif m1 < m1_list[1]:
                m1_list[0] = m1
                m1 = m1_list[1]
                m2 = m2_arg
                epoch = 0
            else:
                epoch += 1
        else:
            epoch += 1
        acc = attack_corrects / n_views
        net.epsilon_3d_zero()
        if targeted:                                                     # AN:490-503
            take = (acc >= best_acc and m1 == m1_best) or (m1 > m1_best and acc > 0)
        else:
            take = (acc <= best_acc and m1 == m1_best) or (m1 > m1_best and acc < 1)
        if take:
            best_acc, m1_best, m2_best = acc, m1, m2
            best = table.clone().detach()
        if export and 'export_x' not in out:                             # the first export pass: what it rendered
            out.update(export_x=np.concatenate(ex_x), export_x_rgba=np.concatenate(ex_r), export_pass=n_pass)
        # pass record: epoch, next epoch, m1 of the pass, m1 / m2 at its end, views, test loss / acc, attack loss / acc, taken,
        # m2 raises, test correct, attack correct
        passes.append([pass_epoch, epoch, pass_m1, m1, m2, n_views, running_loss / n_views, running_corrects / n_views,
                       attack_loss / n_views, acc, int(take), raises, running_corrects, attack_corrects])
        tables.append(table.detach().numpy().copy())
        visits_all.append(visits)
        if '--verbose' in sys.argv:
            print('   pass %d epoch %d -> %d m1 %s -> %s m2 %s acc %.3f take %d visits %s' % (n_pass, pass_epoch, epoch, pass_m1, m1, m2, acc, take,
                  [('s' if a == 1 else int(b)) for a, b in visits[order, :2]]), flush=True)
        logits_all.append(logits)
        it_all.append(its)
        n_pass += 1
    out.update(passes=np.array(passes, np.float64), tables=np.stack(tables), visits=np.stack(visits_all), logits=np.stack(logits_all), iters=np.stack(it_all),
               best=best.numpy().copy(), last_attack=last_attack.detach().numpy().copy(), m1_best=m1_best, m2_best=m2_best, best_acc=best_acc)
    return out, gaps


def g27(save=True):
    s0, ori, wi = scene()
    cls, _ = make_net(False)
    idx = wi[:, 1].numpy()
    assert np.array_equal(idx.astype(np.uint16).astype(np.float32), idx)
    common = dict(s0=s0, ori=ori.astype(np.uint8), w=wi[:, 0].numpy(), idx_u16=idx.astype(np.uint16), cls_w=cls.w.detach().numpy(),
                  shape=np.array([P, H, W, C, EPOCHS, VIEWS, EXPORT_VIEWS, DF_MAX_ITER]), overshoot=OVERSHOOT, m2_max_limit=M2_MAX_LIMIT,
                  tags=np.array([r[0] for r in RUNS]), targeted=np.array([int(r[1]) for r in RUNS]), label=np.array([r[2] for r in RUNS]),
                  m1=np.array([r[3] for r in RUNS]), m2=np.array([r[4] for r in RUNS]), m2_limit=np.array([r[5] for r in RUNS]), **{'draws_%s_%d' % (r[0], k): np.array(v) for r in RUNS if len(r) > 6 for k, v in r[6].items()})
    assert np.array_equal(ori.astype(np.uint8).astype(np.float32), ori)
    seen = dict(skipped=False, completed=False, capped=False, raised=False, down_up=False, best_ne_last=False)
    all_gaps = dict(raw=[], bumped=[], value_r=[])
    per_run = {}
    for tag, targeted, label, m1, m2, limit, *sub in RUNS:
        r32, gaps32 = run_loop(False, s0, wi, ori, label, targeted, m1, m2, limit, sub[0] if sub else None)
        r64, gaps64 = run_loop(True, s0, wi, ori, label, targeted, m1, m2, limit, sub[0] if sub else None)
        for k in ('visits',):
            assert np.array_equal(r32[k], r64[k]), '%s: the float32 and float64 runs differ in %s' % (tag, k)
        dec = [0, 1, 2, 3, 4, 5, 7, 9, 10, 11, 12, 13]                   # every discrete column of a pass record
        assert r32['passes'].shape == r64['passes'].shape and np.array_equal(r32['passes'][:, dec], r64['passes'][:, dec]), \
            '%s: the float32 and float64 runs differ in a pass record' % tag
        for g_ in (gaps32, gaps64):
            for k in all_gaps:
                all_gaps[k] += g_[k]
        v = r32['visits']
        attack_rows = v[r32['passes'][:, 0] < EPOCHS - 1]
        seen['skipped'] |= bool((attack_rows[..., 0] == 1).any())
        seen['completed'] |= bool(((attack_rows[..., 0] == 0) & (attack_rows[..., 1] < DF_MAX_ITER)).any())
        seen['capped'] |= bool(((attack_rows[..., 0] == 0) & (attack_rows[..., 1] == DF_MAX_ITER)).any())
        if tag == 'm2_raise':
            seen['raised'] = bool(r32['passes'][:, 11].sum() >= 1)
        if tag == 'bisect':
            m1s = np.concatenate([r32['passes'][:1, 2], r32['passes'][:, 3]])     # the m1 it started with, then m1 at every pass's end
            seen['down_up'] = bool((np.diff(m1s) < 0).any() and (np.diff(m1s) > 0).any())
        seen['best_ne_last'] |= not np.array_equal(r32['best'], r32['last_attack'])
        dist = lambda a, b: float(np.abs(a.astype(np.float64) - b).max())  # noqa: E731
        arrs = dict(passes=r32['passes'], loss_f64=r64['passes'][:, [6, 8]], visits=r32['visits'], logits=r32['logits'].astype(np.float32),
                    iters=r32['iters'].astype(np.float32), iters_f64=r64['iters'],
                    tables_rgb=r64['tables'][..., :3].astype(np.float32),
                    tables_dist=np.array([dist(a, b) for a, b in zip(r32['tables'], r64['tables'])]),
                    best_rgb=r64['best'][..., :3].astype(np.float32), best_dist=dist(r32['best'], r64['best']),
                    last_attack_rgb=r64['last_attack'][..., :3].astype(np.float32), last_attack_dist=dist(r32['last_attack'], r64['last_attack']),
                    export_x=r64['export_x'].astype(np.float32), export_x_rgba=r64['export_x_rgba'].astype(np.float32),
                    export_x_dist=dist(r32['export_x'], r64['export_x']), export_x_rgba_dist=dist(r32['export_x_rgba'], r64['export_x_rgba']),
                    export_pass=r32['export_pass'], m1_best=r32['m1_best'], m2_best=r32['m2_best'], best_acc=r32['best_acc'])
        per_run[tag] = arrs
        p = r32['passes']
        print('g27 %-10s passes %d epochs %s m1 %s m2 %s acc %s taken %s raises %s' % (
            tag, len(p), p[:, 0].astype(int).tolist(), p[:, 3].astype(int).tolist(), p[:, 4].astype(int).tolist(),
            np.round(p[:, 9], 3).tolist(), p[:, 10].astype(int).tolist(), p[:, 11].astype(int).tolist()))
        print('    skipped per pass %s, iter_k per pass %s' % ((v[..., 0] == 1).sum(1).tolist(),
                                                             [[int(k) for k in row[:, 1] if k >= 0] for row in v]))
        print('    smallest gaps of the run: %s' % {k: '%.2e' % min(gaps32[k] + gaps64[k]) for k in gaps32 if gaps32[k]})
        print('    table distance f32 - f64 per pass %s, best != last attack table: %s'
              % (np.array2string(arrs['tables_dist'], precision=2), not np.array_equal(r32['best'], r32['last_attack'])))
    mins = {k: (min(v) if v else float('inf')) for k, v in all_gaps.items()}
    print('g27 conditions %s; smallest gaps: raw %.2e bumped %.2e of max|logit|, value_r %.2e relative' %
          (seen, mins['raw'], mins['bumped'], mins['value_r']))
    for k, ok in seen.items():
        assert ok, 'condition not met: %s' % k
    assert mins['raw'] >= 1e-3 and mins['bumped'] >= 1e-3, 'an argmax rests on a gap below 1e-3 max|logit|'
    assert mins['value_r'] >= 1e-3, 'two value_r of one iteration are closer than 1e-3 relative'
    if save:
        MG.save('g27_nerfail', **common)
        for tag, arrs in per_run.items():
            MG.save('g27_nerfail_' + tag, **arrs)


if __name__ == '__main__':
    g27(save='--dry' not in sys.argv)
