"""The NeRFail loop's two new pieces against what the parent commit offers, in one session at cfg5's shape: 800x800, P = 3
(1.92 M table rows), the native MyCNN victim with 8 classes, resident views named by id. Event-timed, median of `--reps`
(default 20) after `--warmup` (default 5), the arms of a pair alternated call by call.

  1  one DeepFool iteration: deepfool.deepfool_native against the mirror deepfool.deepfool on the same view. Both are timed at
     max_iter = 1 and max_iter = 1 + K (K = 4, m1 so large that the loop never breaks); the iteration is the difference / K, so
     that what a call pays once (uploads, the forward of deepfool.py:33, allocations) is not in it. The calls themselves are
     reported too.
  2  one attack pass of attack.nerfail over 8 resident views (epochs = 2: the pass, then an export epoch over ONE view without an
     export callback; accumulate_incomplete, so that the pass always changes the table and the m1 bisection of AN:442-453 cannot
     add passes) against the literal AN:311-418 loop written by hand around deepfool.deepfool - per view the forward, the four
     .item() statistics of AN:358-376, the skip test, deepfool, the same unconditional accumulation, then the one export forward:
     the parent commit's best. Both arms run exactly 8 visits and one export forward.

No ratio is claimed in advance. The bar: if the native iteration is slower than the mirror's by more than the spread this file
records (max - min over the reps of the mirror arm), native=None has to resolve to the mirror. Prints one JSON object; --out F
also writes it to F (profiles/<round>_nerfail_bench.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_sections as BS  # noqa: E402

BS._heavy_imports()

VIEWS, K, CLASSES, LABEL = 8, 4, 8, 4


def opt_arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def scene(dev):
    from nerfail_amd.GaussNet import gauss_net, register_view
    from nerfail_amd.MyModel import MyCNN
    wi, ori, s_init = BS._attack_inputs(dev, VIEWS, seed=40)
    Ns = s_init.numel() // 4
    ori8 = ori.to(torch.uint8)
    for v in range(VIEWS):
        register_view(('nerfail_bench', v), Ns, weight_and_index=wi[v], ori_img=ori8[v])
    del wi
    torch.manual_seed(0)
    victim = MyCNN(CLASSES).to(dev).requires_grad_(False).eval()
    net = gauss_net(dev, 0.02, victim, 'my_model', epsilon=None)
    return net, s_init, [(None, None, ('nerfail_bench', v)) for v in range(VIEWS)]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms, reps, warmup):
    """{name: [ms per rep]}: every rep runs each arm once, in turn."""
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    runs = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            runs[k].append(event_ms(fn))
    return runs


def summary(ms):
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms)), 'spread_ms': float(max(ms) - min(ms))}


def hand_written_pass(net, table, views, m1, m2, df_max_iter):
    """AN:311-418 for one attack pass, as a user writes it around deepfool.deepfool: four host reads per view for the statistics."""
    from nerfail_amd import deepfool as DF
    criterion = torch.nn.CrossEntropyLoss()
    lab = torch.tensor([LABEL], device=table.device)
    running_loss = attack_loss = 0.0
    running_corrects = attack_corrects = 0
    attack_all = 0
    for _, _, vid in views:
        net.open_update_epsilon_3d()
        with torch.no_grad():
            _, _, cla, _, ori_cla = net(table, None, None, view_ids=[vid])
        running_loss += criterion(ori_cla, lab).item()
        running_corrects += torch.sum(torch.max(ori_cla, 1)[1] == lab).item()
        attack_loss += criterion(cla, lab).item()
        attack_corrects += torch.sum(torch.max(cla, 1)[1] == lab).item()
        net.close_update_epsilon_3d()
        if torch.argmax(cla[0]) == torch.argmax(ori_cla[0]):
            wi, ori = net._last_views.wi_batch(), net._last_ori
            dr, iter_k, _, _, _ = DF.deepfool((table, wi, ori), None, net, num_classes=CLASSES, max_iter=df_max_iter, m1=m1, m2=m2)
            table += dr                                                  # accumulated_incomplete_attack = True (AN:405)
            attack_all += 1
    net.epsilon_3d_zero()
    net.open_update_epsilon_3d()
    with torch.no_grad():                                                # the export epoch's one view (AN:354 on the best tensor)
        net(table, None, None, view_ids=[views[0][2]])
    net.epsilon_3d_zero()
    return attack_corrects / len(views)


def main():
    from nerfail_amd import deepfool as DF
    from nerfail_amd.attack import nerfail
    reps, warmup = opt_arg('--reps', 20), opt_arg('--warmup', 5)
    dev = torch.device('cuda:0')
    net, s_init, views = scene(dev)
    res = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'warmup': warmup,
           'shape': '800x800, P=3, %d resident views, native MyCNN (%d classes)' % (VIEWS, CLASSES)}

    # ---- 1: one DeepFool iteration (m1 = 1e6: the loop never breaks)
    vid = [views[0][2]]
    with torch.no_grad():
        net(s_init, None, None, view_ids=vid)
    wi, ori = net._last_views.wi_batch(), net._last_ori
    kw = dict(num_classes=CLASSES, m1=1e6, m2=100.)
    arms = {}
    for it in (1, 1 + K):
        arms['native_%d' % it] = lambda it=it: DF.deepfool_native((s_init, wi, ori), None, net, max_iter=it, view_ids=vid, **kw)
        arms['mirror_%d' % it] = lambda it=it: DF.deepfool((s_init, wi, ori), None, net, max_iter=it, **kw)
    runs = alternate(arms, reps, warmup)
    one = {k: summary(v) for k, v in runs.items()}
    for name in ('native', 'mirror'):
        per = [(b - a) / K for a, b in zip(runs['%s_1' % name], runs['%s_%d' % (name, 1 + K)])]
        one['%s_iteration' % name] = summary(per)
    res['deepfool_iteration'] = one
    n_it, m_it = one['native_iteration'], one['mirror_iteration']
    res['native_iteration_minus_mirror_ms'] = n_it['median_ms'] - m_it['median_ms']
    res['native_slower_than_mirror_beyond_its_spread'] = bool(n_it['median_ms'] - m_it['median_ms'] > m_it['spread_ms'])

    # ---- 2: one attack pass over the 8 views, df_max_iter = 3
    def nerfail_pass():
        res = nerfail(net, s_init, views, LABEL, 2, m1=8, m2=100, df_max_iter=3, num_classes=CLASSES, accumulate_incomplete=True,
                      export_views=views[:1], log=None)
        assert [d['epoch'] for d in res.stats] == [0, 1], 'the arm is one attack pass and one export pass'
    arms = {'nerfail_pass': nerfail_pass,
            'hand_written_pass': lambda: hand_written_pass(net, s_init.clone(), views, 8, 100, 3)}
    runs = alternate(arms, reps, warmup)
    res['attack_pass'] = {k: summary(v) for k, v in runs.items()}
    res['hand_written_over_nerfail'] = res['attack_pass']['hand_written_pass']['median_ms'] / res['attack_pass']['nerfail_pass']['median_ms']
    res['note'] = ('HIP events around each call, device idle before it; the arms of a pair alternate call by call; the iteration is '
                   '(call at max_iter 5 - call at max_iter 1) / 4 of the same rep; spread = max - min over the reps')
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
