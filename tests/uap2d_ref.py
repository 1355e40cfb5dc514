"""Numpy restatement of the UAP-2D baseline: the three kernels behind nerfail_uap2d_step and nerfail_uap2d_accumulate, DeepFool
with universal_2d (deepfool.py:10-111 = DF) on the one shared image-plane table, and the loop of attack_UAP_2D.py:241-358 (= UA),
written from those lines and from include/nerfail_hip.h, section "2-D universal baseline" - not from the kernels.
tests/test_uap2d_ref.py holds it to fixture g29 (the reference's own run, tests/golden/make_golden_uap2d.py);
tests/test_hip_uap2d_kernels.py holds the kernels to it.

Gate and choice are tests/nerfail_ref.py's (one definition, as in the library); the forward is tests/igsm2d_ref.py's."""
import numpy as np

import attack_loop_ref as R
import igsm2d_ref as IR
import nerfail_ref as NR

F32 = np.float32
NORM_TERMS = 24                  # NERFAIL_UAP2D_NORM_TERMS
NORM_PIXELS = 256 * NORM_TERMS // 3   # pixels of one norm workgroup


# ------------------------------------------------------------------------------------------------ the three launches of the step
def mask_bits(pass_mask):
    """bool [P,3] of a uint8 mask [P]: bit c of pixel p."""
    return ((np.asarray(pass_mask, np.uint8).reshape(-1)[:, None] >> np.arange(3)) & 1).astype(bool)


def norms2(grads, pass_mask):
    """float64 [n_rhs - 1]: the sum over set bits of (G_k - G_0)^2, from the float32 gradients [n_rhs,3,P], every operation in
    float64. A cleared bit contributes 0 whatever the gradient holds."""
    G = np.asarray(grads, F32).reshape(len(grads), 3, -1).astype(np.float64)
    bits = mask_bits(pass_mask).T                                           # [3,P]
    with np.errstate(invalid='ignore', over='ignore'):
        d = G[1:] - G[:1]
        return np.where(bits[None], d * d, 0.).sum((1, 2))


def apply(grads, pass_mask, best, scale, overshoot, r0, rot):
    """(rot', r_out) float32 [P,3] of the apply launch, one rounding per operation. best: slice 1..n_rhs-1; scale 0 or a best
    outside that range leaves rot alone."""
    G = np.asarray(grads, F32).reshape(len(grads), 3, -1)
    r0, rot = np.asarray(r0, F32).reshape(-1, 3), np.array(rot, F32, copy=True).reshape(-1, 3)
    scale, overshoot = F32(scale), F32(overshoot)
    with np.errstate(invalid='ignore', over='ignore'):
        if scale != 0 and 1 <= best < len(G):
            d = np.where(mask_bits(pass_mask), (G[best] - G[0]).astype(F32).T, F32(0))
            rot = (rot + (scale * d).astype(F32)).astype(F32)
        v = (r0 + (overshoot * rot).astype(F32)).astype(F32)
        out = np.where(v < -255, F32(-255), np.where(v > 255, F32(255), v)).astype(F32)     # torch.clamp: a NaN stays
    return rot, out


def step(grads, pass_mask, rec, overshoot, r0, rot, norms2_f32=None):
    """nerfail_uap2d_step: (norms2 float32, best, scale, trace, rot', r_out). norms2_f32: the kernel's own norms when the caller
    checks the rest bit for bit, else the float64 sums rounded once."""
    K = len(grads) - 1
    n2 = norms2(grads, pass_mask).astype(F32) if norms2_f32 is None else np.asarray(norms2_f32, F32)
    best, scale, bi = NR.choose(rec['fabs'], n2, rec['n_comp'], rec['targeted'], K=K)
    trace = int(rec['cls'][bi]) if bi >= 0 else -1
    rot, out = apply(grads, pass_mask, best, scale, overshoot, r0, rot)
    return n2, best, scale, trace, rot, out


def accumulate(table, r_final, epsilon):
    """nerfail_uap2d_accumulate: UA:317-319 with DF:109, float32, one rounding per operation; torch.clamp: a NaN stays."""
    t, rf, eps = np.asarray(table, F32), np.asarray(r_final, F32), F32(epsilon)
    with np.errstate(invalid='ignore', over='ignore'):
        v = (t + (rf - t).astype(F32)).astype(F32)
        return np.where(v < -eps, -eps, np.where(v > eps, eps, v)).astype(F32)


# ------------------------------------------------------------------------------------------------ DF with universal_2d, stand-in classifier
def pool_class_grads(w, rows, H, W):
    """d logit_k / d cls_in of igsm2d_ref.pool_logits for the classes `rows`: float32 [len(rows),3,H*W], evaluated in float64 and
    rounded once (what autograd returns through the float64 classifier)."""
    g = (np.asarray(w).astype(np.float64)[rows].reshape(len(rows), 3, 4, 1, 4, 1) / ((H // 4) * (W // 4)))
    return np.broadcast_to(g, (len(rows), 3, 4, H // 4, 4, W // 4)).reshape(len(rows), 3, H * W).astype(F32)


def deepfool_2d(table, image, w, num_classes, max_iter, target, overshoot, m1, m2):
    """DF:10-111 with universal_2d on one view (`image`: its uint8 store row). target: -1 untargeted. Returns (r_final, loop_i,
    classes, cleared): the table after the last step, the iterations, the class chosen in each, and how many pass-mask bits
    were cleared over the call's forwards."""
    H, W = image.shape[:2]
    r0 = np.asarray(table, F32).reshape(-1, 3)
    store = image[None]
    o = int(np.argmax(IR.pool_logits(IR.u2d_fwd(store, [0], np.zeros((H, W, 3), F32), True)[1], w)[0]))
    ks = [k for k in range(num_classes) if k != o] if target < 0 else [target]
    G = pool_class_grads(w, [o] + ks, H, W)
    rot, cur, classes, cleared = np.zeros_like(r0), r0, [], 0
    loop_i = 0
    while loop_i < max_iter:
        _, cls_in, mask = IR.u2d_fwd(store, [0], cur.reshape(H, W, 3), True)
        cleared += int((~mask_bits(mask[0])).sum())
        rec = NR.gate(IR.pool_logits(cls_in, w)[0], o, target, m1, m2)
        if rec['done']:
            break
        _, _, _, trace, rot, cur = step(G, mask[0], rec, overshoot, r0, rot)
        classes.append(trace)
        loop_i += 1
    return cur.reshape(H, W, 3), loop_i, classes, cleared


# ------------------------------------------------------------------------------------------------ UA:241-358
def run_loop(images, w, label, epochs, epsilon, m1, m2, targeted, df_max_iter, overshoot, num_classes=8, attack_views=None,
             export_views=None, deepfool=None):
    """The loop with the stand-in classifier. attack_views / export_views: lists, or callables of the pass number; default all
    views. deepfool: a stand-in for deepfool_2d above with its arguments and return. Returns a dict: tables (per pass, as the
    pass left it), passes (per pass: epoch, next_epoch, views, test_loss, test_acc, attack_loss, attack_acc, taken, test_correct,
    attack_correct), visits (per pass a list of (view, skipped, iter_k, classes)), iters_so_far (DeepFool iterations up to the
    end of every pass), best, last, best_acc, export (per view of the FIRST export pass: pass, view, the attacked image, the
    perturbation and the clean image as float32), cleared."""
    deepfool = deepfool_2d if deepfool is None else deepfool
    images = np.asarray(images)
    N, H, W = images.shape[:3]
    zero = np.zeros((H, W, 3), F32)
    table = zero.copy()                                                     # UA:219
    best = table.copy()
    best_acc = 0 if targeted else 10000                                     # UA:234-237
    ori_cla = IR.pool_logits(IR.u2d_fwd(images, list(range(N)), zero, True)[1], w)

    def views_of(src, n_pass):
        return list(range(N)) if src is None else list(src(n_pass) if callable(src) else src)
    out = dict(tables=[], passes=[], visits=[], export=[], cleared=0, iters_so_far=[])
    total_iters = 0
    epoch, n_pass = 0, 0
    while epoch < epochs:
        assert n_pass < 64, 'the loop does not end'
        export = epoch == epochs - 1
        items = views_of(export_views if export else attack_views, n_pass)
        sums, correct = np.zeros(2), np.zeros(2, np.int64)
        not_changed, visits, pass_epoch = True, [], epoch
        for v in items:
            if export:
                table = best                                                # UA:269
            x_rgb, cls_in, _ = IR.u2d_fwd(images, [v], table, True)
            cla = IR.pool_logits(cls_in, w)
            st = R.logit_stats(cla, ori_cla[[v]], label)                    # UA:275-289
            sums += st[:2]
            correct += [int(st[2]), int(st[3])]
            if export:
                if not out['export'] or out['export'][0][0] == n_pass:
                    out['export'].append((n_pass, v, x_rgb[0], table.copy(), IR.white(images[v])))
                not_changed = False                                         # UA:333
                continue
            if int(np.argmax(cla[0])) != int(np.argmax(ori_cla[v])):        # UA:297-304
                visits.append((v, True, 0, []))
                continue
            r_final, iter_k, classes, cleared = deepfool(table, images[v], w, num_classes, df_max_iter, label if targeted else -1,
                                                         overshoot, m1, m2)
            out['cleared'] += cleared
            total_iters += iter_k
            visits.append((v, False, iter_k, classes))
            if iter_k < df_max_iter:                                        # UA:315-319
                table = accumulate(table, r_final, epsilon)
                not_changed = False
        epoch = epochs - 1 if not_changed else epoch + 1                    # UA:335-338
        n = len(items)
        acc = correct[1] / n
        take = bool(acc > best_acc) if targeted else bool(acc < best_acc)   # UA:349-358: strict
        if take:
            best_acc, best = acc, table.copy()
        out['passes'].append([pass_epoch, epoch, n, sums[0] / n, correct[0] / n, sums[1] / n, acc, int(take), correct[0], correct[1]])
        out['tables'].append(table.copy())
        out['visits'].append(visits)
        out['iters_so_far'].append(total_iters)
        n_pass += 1
    out.update(best=best, last=table, best_acc=best_acc, passes=np.array(out['passes'], np.float64))
    return out


# ------------------------------------------------------------------------------------------------ fixture g29's scene and layout
G29_EXTRA_SEED = 2900            # the seed stream of the views g29 adds to g28's four
G29_VISIT_COLS = 3               # visits [passes, slots, 3 + df_max_iter]: view, skipped, iter_k, classes (-1 beyond)


def g29_images(seed, tints, extra_tints):
    """g28's four views, then len(extra_tints) opaque views from a seed stream of their own (g28's do not move)."""
    base = IR.g28_images(seed, tints)
    if not len(extra_tints):
        return base
    rs = np.random.RandomState(G29_EXTRA_SEED)
    img = rs.randint(0, 256, size=(len(extra_tints),) + base.shape[1:]).astype(np.float64)
    img[..., :3] = np.floor(img[..., :3] * np.asarray(extra_tints, np.float64).reshape(-1, 1, 1, 1))
    img[..., 3] = 255.
    return np.concatenate([base, img.astype(np.uint8)])


def visits_array(visits, df_max_iter, slots):
    """Per pass the visit list as an int64 array [slots, 3 + df_max_iter], -1 where nothing stands."""
    a = np.full((len(visits), slots, G29_VISIT_COLS + df_max_iter), -1, np.int64)
    for p, vs in enumerate(visits):
        for s, (v, skipped, iter_k, classes) in enumerate(vs):
            a[p, s, :3] = (v, int(skipped), iter_k)
            if classes is not None:
                a[p, s, 3:3 + len(classes)] = classes
    return a


def g29_args(g, i):
    """run_loop's arguments (after images and w) for run i of the fixture, as keywords."""
    tag = str(g['tags'][i])
    draws = {int(k.rsplit('_', 1)[1]): [int(v) for v in g[k]] for k in list(getattr(g, 'files', g)) if k.startswith('draws_%s_' % tag)}
    n = int(g['shape'][0])
    return dict(label=int(g['label'][i]), epochs=int(g['shape'][4]), epsilon=float(g['epsilon'][i]), m1=float(g['m1'][i]),
                m2=float(g['m2'][i]), targeted=bool(g['targeted'][i]), df_max_iter=int(g['shape'][5]), overshoot=float(g['overshoot']),
                num_classes=int(g['shape'][3]), attack_views=lambda n_pass: draws.get(n_pass, list(range(n))),
                export_views=[int(v) for v in g['export_views']])


def g29_bound(ref, dist, iters):
    """The standing bound of the attack-loop tests: twice the fixture's own float32-to-float64 distance plus eight float32 ulps
    of max(|reference|, 1) per DeepFool iteration so far (and one for the forward). The +-epsilon clamp cannot grow an error."""
    return 2. * float(dist) + 8. * 2. ** -24 * np.maximum(np.abs(np.asarray(ref, np.float64)), 1.) * (1 + int(iters))


def g29_check(g, tag, passes, visits, tables, best, export, say=print):
    """Holds one run to the fixture: every discrete decision equal, losses within twice the fixture's own spread + 1e-6
    relative, tables, best and the exported float images within g29_bound. passes: [n,10] as run_loop's; visits: per pass the
    (view, skipped, iter_k, classes or None) list; export: (pass, view, adv, mask, ori) per exported view of the first export pass,
    or None to leave the images to the caller."""
    want = g[tag + '_passes']
    passes = np.asarray(passes, np.float64)
    assert passes.shape == want.shape, (tag, passes.shape, want.shape)
    dec = [0, 1, 2, 4, 6, 7, 8, 9]
    assert np.array_equal(passes[:, dec], want[:, dec]), (tag, passes[:, dec], want[:, dec])
    f64 = g[tag + '_loss_f64']
    for col, j in ((3, 0), (5, 1)):
        bound = 2 * np.abs(want[:, col] - f64[:, j]) + 1e-6 * np.abs(want[:, col])
        assert (np.abs(passes[:, col] - want[:, col]) <= bound).all(), (tag, col, passes[:, col], want[:, col], bound)
    df_max_iter, n = int(g['shape'][5]), int(g['shape'][0])
    wv = g[tag + '_visits']
    got = visits_array(visits, df_max_iter, n)
    assert np.array_equal(got[..., :3], wv[..., :3]), (tag, got[..., :3], wv[..., :3])
    if all(c is not None for vs in visits for _, _, _, c in vs):
        assert np.array_equal(got, wv), (tag, got, wv)
    iters = g[tag + '_iters_so_far']
    worst = 0.
    for p, t in enumerate(tables):
        ref = g[tag + '_tables'][p]
        ratio = float((np.abs(np.asarray(t, np.float64) - ref) / g29_bound(ref, g[tag + '_tables_dist'][p], iters[p])).max())
        worst = max(worst, ratio)
        assert ratio <= 1., (tag, 'table of pass', p, ratio)
    ref = g[tag + '_best']
    ratio = float((np.abs(np.asarray(best, np.float64) - ref) / g29_bound(ref, g[tag + '_best_dist'], iters[-1])).max())
    assert ratio <= 1., (tag, 'best', ratio)
    worst = max(worst, ratio)
    if export is None:
        say('g29 %s: worst error / bound over tables and best %.3f' % (tag, worst))
        return
    assert [e[0] for e in export] == [int(g[tag + '_export_pass'])] * len(g['export_views']), (tag, [e[0] for e in export])
    assert [e[1] for e in export] == [int(v) for v in g['export_views']]
    for k, name in ((2, 'adv'), (3, 'mask')):
        for j, e in enumerate(export):
            ref = g[tag + '_export_' + name][j]
            ratio = float((np.abs(np.asarray(e[k], np.float64) - ref) / g29_bound(ref, g[tag + '_export_%s_dist' % name], iters[-1])).max())
            assert ratio <= 1., (tag, 'export', name, ratio)
            worst = max(worst, ratio)
    for j, e in enumerate(export):
        assert np.array_equal(np.asarray(e[4]).astype(np.float32), g[tag + '_export_ori'][j].astype(np.float32)), (tag, 'export ori')
    say('g29 %s: worst error / bound over tables, best and exported images %.3f' % (tag, worst))
