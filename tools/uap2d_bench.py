"""attack.uap_2d and deepfool.deepfool_2d_native against what the reference writes, and nerfail_uap2d_step against the chip, in
one session at the reference's shape: 800x800 BGRA views, the native MyCNN victim with 8 classes. Event-timed, median of
`--reps` (default 10) after `--warmup` (default 3), the arms alternated call by call, max - min of each arm reported as its spread.

  1  one DeepFool iteration of deepfool.deepfool_2d_native (u2d_fwd, cnn_fwd, gate, one host read, ONE cnn_bwd_data_multi over
     8 one-hot rows, nerfail_uap2d_step) against an iteration that asks for its gradients as DF:44-102 does
     (per_class_deepfool below: deepfool_2d's loop through universal_2D_net with two forwards of the classifier, attacked and
     clean image, then per competitor one autograd.grad of its logit and one more of the clean class's, the norm, a comparison
     the host waits for, rot and the clamp in stock torch ops). m1 is set out of reach, so no call breaks: a call with 1 + K
     iterations minus a call with 1, over K = 3. The comparison arm's create_graph is False (the reference asks for True and
     never uses the second-order graph; MyCNN's backward is not itself differentiable).
  2  one attack pass of attack.uap_2d over 4 views, timed directly: HIP events at the call's start and at the seam where pass 0
     ends, so everything a call pays once (its buffers, the clean logits of the four views) is in the figure; against the
     UA:265-319 loop body in stock torch ops with per_class_deepfool, which pays for the clean logits in every forward. On
     constants with which calls complete. Both arms report how many DeepFool iterations their pass ran.
  3  nerfail_uap2d_step alone with 8 gradient rows over 4 x 800 x 800 pixels (435 MB moved: more than the 256 MB last-level
     cache), with the compulsory bytes per pixel - norms 12 R + 1, apply 73 - and the achieved bytes per second.

No ratio is claimed in advance. Prints one JSON object; --out F also writes it to F (profiles/<round>_uap2d_bench.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.igsm2d_bench import alternate, event_ms, opt_arg, summary, views  # noqa: E402

H = W = 800
VIEWS, K, CLASSES, LABEL, STREAM_PLANES = 4, 3, 8, 4, 4
PASS_KW = dict(epsilon=32., m1=0, m2=1, targeted=False, df_max_iter=3, overshoot=50.)


def per_class_deepfool(table, ori, net, num_classes, max_iter, overshoot, m1, m2):
    """The comparison arm for DeepFool on the shared plane, untargeted: deepfool.deepfool_2d's loop asked for its gradients the
    way DF:31-102 asks for them, because that - not the arithmetic - is what an iteration of the reference costs. Before the
    loop one forward and one backward of the largest logit (DF:31-40). Per iteration universal_2D_net's forward, which runs the
    classifier on the attacked AND on the clean image; then for every competitor one autograd.grad of its logit and one more of
    the clean class's (the same tensor each time, DF:76-77), the norm of their difference, and a comparison whose outcome the
    host waits for (DF:84). create_graph stays False: see the module text. Returns (table moved by, iterations)."""
    start = table.detach().clone()
    cur, moved, done = start, torch.zeros_like(start), 0
    probe = cur.clone().requires_grad_(True)
    torch.autograd.grad(net(probe, ori)[2].max(), probe)
    while done < max_iter:
        probe = cur.detach().clone().requires_grad_(True)
        _, _, logits, _, clean = net(probe, ori)
        o = int(clean.argmax(1))
        bump = torch.zeros_like(logits)
        bump[:, o] = m1
        logits = logits + bump
        if int(logits.argmax(1)) != o:
            break
        smallest, step = float('inf'), torch.zeros_like(moved)
        for k in range(num_classes):
            if k == o:
                continue
            g_k = torch.autograd.grad(logits[0, k], probe, retain_graph=True)[0]
            g_o = torch.autograd.grad(logits[0, o], probe, retain_graph=True)[0]
            diff = g_k - g_o
            gap = (logits[0, k] - (logits[0, o] + m2)).abs()
            nrm = diff.norm()
            ratio = gap / (nrm + 0.0001)
            if bool(ratio < smallest):
                smallest, step = ratio, (gap / (nrm ** 2 + 0.0001)) * diff
        moved = (moved + step).detach()
        cur = (start + overshoot * moved).clamp(-255, 255)
        done += 1
    return (cur - start).detach(), done


def literal_pass(net, oris, lab, kw, count):
    """UA:252-319 for one pass over the views, from the zero table."""
    criterion = torch.nn.CrossEntropyLoss()
    table = torch.zeros((H, W, 3), device=oris.device)
    running_loss = attack_loss = 0.0
    running_corrects = attack_corrects = 0
    for v in range(oris.shape[0]):
        ori_img = oris[v:v + 1]
        x, r, cla, ori_f, ori_cla = net(table, ori_img)
        lab_r = lab.broadcast_to([ori_cla.size()[0], ])
        loss = criterion(ori_cla, lab_r)
        _, preds = torch.max(ori_cla, 1)
        running_loss += loss.item() * len(ori_f)
        running_corrects += torch.sum(preds == lab_r)
        ae_loss = criterion(cla, lab_r)
        _, ae_preds = torch.max(cla, 1)
        attack_loss += ae_loss.item() * len(ori_f)
        attack_corrects += torch.sum(ae_preds == lab_r)
        if torch.argmax(cla[0]) == torch.argmax(ori_cla[0]):
            dr, iter_k = per_class_deepfool(table, ori_img, net, CLASSES, kw['df_max_iter'], kw['overshoot'], kw['m1'], kw['m2'])
            count.append(iter_k)
            if iter_k < kw['df_max_iter']:
                table = table + dr
                table = torch.clamp(table, -kw['epsilon'], kw['epsilon'])
    return table


def main():
    from nerfail_amd import _lib, attack
    from nerfail_amd import deepfool as DF
    from nerfail_amd.GaussNet import universal_2D_net
    from nerfail_amd.MyModel import MyCNN
    reps, warmup = opt_arg('--reps', 10), opt_arg('--warmup', 3)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    victim = MyCNN(CLASSES).to(dev).requires_grad_(False).eval()
    images = views(VIEWS, dev)
    oris = torch.where(images[..., 3:4] > 0, images[..., :3], torch.ones_like(images[..., :3]) * 255)        # MD:247-255
    net = universal_2D_net(dev, 0.02, victim, 'my_model')
    res = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'warmup': warmup,
           'shape': '%dx%d BGRA, %d views, native MyCNN (%d classes)' % (H, W, VIEWS, CLASSES)}

    # ---- 1: one DeepFool iteration (m1 out of reach: no call breaks)
    table = torch.zeros((H, W, 3), device=dev)
    far = dict(overshoot=0.02, m1=1e6, m2=30)
    arms, ran = {}, {}
    for n in (1, 1 + K):
        arms['native_%d' % n] = lambda n=n: ran.__setitem__('native_%d' % n, DF.deepfool_2d_native((table, None), None, net, CLASSES, n, images=images,
                                                                                                    view=0, **far)[1])
        arms['literal_%d' % n] = lambda n=n: ran.__setitem__('literal_%d' % n, per_class_deepfool(table, oris[:1], net, CLASSES, n, **far)[1])
    runs = alternate(arms, reps, warmup)
    it = {k: summary(v) for k, v in runs.items()}
    for name in ('native', 'literal'):
        it['%s_iteration' % name] = summary([(b - a) / K for a, b in zip(runs['%s_1' % name], runs['%s_%d' % (name, 1 + K)])])
    it['iterations_run'] = dict(ran)
    res['deepfool_iteration'] = it
    res['literal_over_native_iteration'] = it['literal_iteration']['median_ms'] / it['native_iteration']['median_ms']

    # ---- 2: one attack pass
    lab = torch.tensor(LABEL, device=dev)
    lit_iters, nat = [], {}

    def native_pass():
        """One call with one attack epoch: HIP events at its start and at the seam where pass 0 ends. What the call pays once
        (freezing the model, its buffers, the clean logits of the four views) is inside the figure."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        orig = attack._uap2d_pass_done
        attack._uap2d_pass_done = lambda index, table: e1.record() if index == 0 else None
        e0.record()
        try:
            r = attack.uap_2d(victim, 'my_model', images, LABEL, 2, log=None, **PASS_KW)
        finally:
            attack._uap2d_pass_done = orig
        torch.cuda.synchronize()
        nat['passes'] = [(d['epoch'], d['attacked'], d['completed'], d['deepfool_iters']) for d in r.stats]
        return e0.elapsed_time(e1)

    def literal_ms():
        lit_iters.clear()
        return event_ms(lambda: literal_pass(net, oris, lab, PASS_KW, lit_iters))
    for _ in range(warmup):
        native_pass(), literal_ms()
    runs = {'native_pass': [], 'literal_pass': []}
    for _ in range(reps):
        runs['native_pass'].append(native_pass())
        runs['literal_pass'].append(literal_ms())
    ps = {k: summary(v) for k, v in runs.items()}
    ps['native_passes (epoch, attacked, completed, deepfool_iters)'] = nat['passes']
    ps['literal_deepfool_iters_per_visit'] = list(lit_iters)
    res['attack_pass'] = ps
    res['literal_over_native_pass'] = ps['literal_pass']['median_ms'] / ps['native_pass']['median_ms']

    # ---- 3: the step alone, over more than the last-level cache holds
    del arms, runs
    torch.cuda.empty_cache()
    lib = _lib.load()
    P, R = STREAM_PLANES * H * W, CLASSES
    G = torch.randn((R, 3, P), device=dev) * 1e-3
    mask = torch.randint(0, 8, (P,), dtype=torch.uint8, device=dev)
    r0, rot, out = (torch.rand((P, 3), device=dev) - .5) * 16., torch.zeros((P, 3), device=dev), torch.empty((P, 3), device=dev)
    nb = lib.nerfail_uap2d_step_scratch_bytes(R, P)
    scratch = torch.empty((nb // 8,), dtype=torch.float64, device=dev)
    record = torch.zeros((_lib.DEEPFOOL_RECORD_WORDS,), dtype=torch.int32, device=dev)
    record[2] = R - 1
    record[4:4 + R - 1] = torch.arange(1, R, dtype=torch.int32, device=dev)
    record[12:12 + R - 1] = torch.full((R - 1,), 100., device=dev).view(torch.int32)
    trace = torch.zeros((1,), dtype=torch.int32, device=dev)
    p = lambda t: _lib.c_p(t.data_ptr())                                   # noqa: E731

    def stp():
        _lib.check(lib.nerfail_uap2d_step(p(G), R, P, p(mask), p(record), p(scratch), nb, 0.02, p(r0), p(rot), p(out), p(trace), _lib.stream()))
    runs = alternate({'uap2d_step': stp}, reps, warmup)
    s = summary(runs['uap2d_step'])
    per_pixel = (12 * R + 1) + 73
    nbytes = per_pixel * P
    s.update(bytes_per_pixel=per_pixel, bytes=nbytes, TB_per_s=nbytes / (s['median_ms'] * 1e-3) / 1e12, chosen_class=int(trace[0]))
    s['of_6.3_TB_per_s'] = s['TB_per_s'] / 6.3
    res['uap2d_step'] = s
    res['uap2d_step_shape'] = '%d gradient rows over %d pixels: %.0f MB moved' % (R, P, nbytes / 1e6)
    res['note'] = ('HIP events around each call, device idle before it; the arms alternate call by call; an iteration is (call with 4 '
                   'iterations - call with 1) / 3 of the same rep; a native pass runs from the start of a call with one attack epoch to '
                   'the end of its pass 0, the once-per-call work included; spread = max - min over the reps; the step\'s time is its three launches together (norms, '
                   'choose, apply); 6.3 TB/s is what a streaming kernel reaches on this chip (README)')
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
