#!/usr/bin/env python3
"""The scene-map stage: the fused 8-NN + weight kernel against the chain it replaces, and scene.build_scene_maps against the
file pipeline (nerf_to_coord.render_path -> create_index_and_dist -> dist_to_weight -> GaussNet.load_view_maps).

    python tools/scene_maps_bench.py [--out FILE] [--skip-pipeline]
    python tools/scene_maps_bench.py --foreground [--out FILE]
    python tools/scene_maps_bench.py --sharded [--out FILE]

(a) `kernel`: one 800x800 view of rendered-view geometry (synth.sphere_view_points) against the 1.92 M points of three such
    views, grid built once. Arm `chain`: create_index_and_dist.index_and_dist (the search, then the torch.stack copy) followed
    by create_gauss_w - what the file pipeline runs per view between its files. Arm `fused`: scene.view_map (one search launch
    with the weights as its epilogue, plus the one-wave fold of sum_d2). Event-timed, the two arms ALTERNATED run by run in one
    session, median of 20 after 5 warm-up; `spread` is each arm's interquartile range, min and max are given too.
(b) `pipeline`: 8 views of 800x800 from a D8 W256 NeRF (synthetic weights, 64 + 128 samples), point set = 3 of them. Wall time
    (host clock around a device synchronisation) of build_scene_maps, render included, against the file pipeline for the same
    views in a fresh temporary directory on the local disk, each arm run twice in alternation (both runs reported); the render
    alone (the same 8 views, nothing else) is timed separately, and the bytes each arm leaves on disk are counted.
(c) `--foreground` (run INSTEAD of (a) and (b)): build_scene_maps(foreground_only=True) against the full call over the same 8
    views of 800x800, the same D8 W256 pair and synth.disc_alpha_image as the views' images (radius 300 of 800: n / P = 0.44);
    `point_set=` is prebuilt from views MASK, so all 8 views take the new path. Wall time of each call, the arms ALTERNATED,
    ROUNDS times each; the render alone likewise (nerf_to_coord.render of every pixel against render_pixels of the lists) -
    `render_ratio` is to be read beside `n_over_P`; and the three new kernels alone on one view, event-timed, median of 20
    after 5 warm-up (pixel list; ray_gen_list; the list search with its zeroing and fold, next to view_map on the whole view).
    Writes profiles/r28_fg_scene_maps_bench.json.
(d) `--sharded` (run INSTEAD of (a) and (b)): a one-GPU sanity number, not a scaling claim - build_scene_maps(shard_batch=8) in
    this one-rank process against the call without the keyword, over shape (b)'s 8 views and point set. One rank owns every
    view, so both arms issue the same launches; wall time of each call, the arms ALTERNATED, ROUNDS times each.
    Writes profiles/r29_sharded_scene_maps_bench.json.
Writes one JSON object (default profiles/r23_scene_maps_bench.json) and prints it."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import synth  # noqa: E402

SIDE, C, WARMUP, RUNS, VIEWS, MASK = 800, 0.02, 5, 20, 8, [0, 3, 6]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    q1, med, q3 = (float(v) for v in np.percentile(ms, [25, 50, 75]))
    return {'ms_median': med, 'ms_min': float(min(ms)), 'ms_max': float(max(ms)), 'spread_iqr_ms': q3 - q1, 'ms': [float(v) for v in ms]}


def kernel_arms(dev):
    from nerfail_amd.create_index_and_dist import index_and_dist
    from nerfail_amd.GaussNet import create_gauss_w
    from nerfail_amd.scene import PointSet, view_map
    S = torch.from_numpy(np.stack([synth.sphere_view_points(SIDE, SIDE, th) for th in (-120., 0., 120.)]).reshape(-1, 3)).to(dev)
    Q = torch.from_numpy(synth.sphere_view_points(SIDE, SIDE, 45.)).to(dev)
    ps = PointSet(S)
    gw = create_gauss_w(dev, C)

    def chain():
        return gw(index_and_dist(Q, ps.points, method='grid').unsqueeze(0))[0][0]

    def fused():
        return view_map(Q, ps, C)[0]
    assert torch.equal(chain(), fused())                      # the two arms compute the same map, bit for bit
    for _ in range(WARMUP):
        chain()
        fused()
    a, b = [], []
    for _ in range(RUNS):
        a.append(event_ms(chain))
        b.append(event_ms(fused))
    res = {'shape': '%dx%d view against %d points (3 views of synth.sphere_view_points), c = %g' % (SIDE, SIDE, S.shape[0], C),
           'chain': summary(a), 'fused': summary(b)}
    res['fused_minus_chain_ms'] = res['fused']['ms_median'] - res['chain']['ms_median']
    res['fused_not_slower_than_chain_by_more_than_its_spread'] = bool(res['fused_minus_chain_ms'] <= res['chain']['spread_iqr_ms'])
    P = SIDE * SIDE
    # what the chain moves and the fused call does not (both write the [2,P,8] map once)
    res['bytes_not_moved_per_view'] = {'dist_idx_written_by_the_search': 2 * P * 32, 'stack_copy_read_and_written': 2 * 2 * P * 32,
                                       'read_back_by_gauss_weight': 2 * P * 32}
    return res


def render_kwargs(dev):
    from nerfail_amd import run_nerf as RN
    from nerfail_amd.run_nerf_helpers import NeRF
    nets = []
    for seed in (1, 2):
        sd = synth.nerf_state_dict(seed=seed)
        m = NeRF(8, 256, 63, 27, 5, [4], True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        nets.append(m.to(dev).requires_grad_(False))
    q = RN.FusedNetworkQuery(RN.get_embedder(10, 0)[0], RN.get_embedder(4, 0)[0])
    return dict(network_query_fn=q, perturb=0., N_importance=128, network_fine=nets[1], N_samples=64, network_fn=nets[0], use_viewdirs=True,
                white_bkgd=True, raw_noise_std=0., ndc=False, lindisp=False, near=2., far=6.)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def tree_bytes(root):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(root) for f in fs)


def pipeline_arms(dev):
    from nerfail_amd import GaussNet as G, nerf_to_coord as NC
    from nerfail_amd.create_index_and_dist import create_index_and_dist
    from nerfail_amd.dist_to_weight import dist_to_weight
    from nerfail_amd.scene import build_scene_maps
    kw = render_kwargs(dev)
    focal, K = synth.lego_intrinsics(SIDE, SIDE)
    hwf = [SIDE, SIDE, focal]
    poses = torch.from_numpy(np.stack([synth.pose_spherical(-180. + 45. * i, -30., 4.) for i in range(VIEWS)]).astype(np.float32))
    chunk = 1024 * 32
    Ns = len(MASK) * SIDE * SIDE

    def render_only():
        with torch.no_grad():
            for c2w in poses:
                NC.render(SIDE, SIDE, K, chunk=chunk, c2w=c2w[:3, :4], **kw)

    def files(base):
        d = os.path.join(base, 'logs', 'blender_paper_bench', 'renderonly_test_000000')
        os.makedirs(d)
        for s in ('train', 'val'):
            os.makedirs(os.path.join(base, 'logs', 'blender_paper_bench', 'renderonly_%s_000000' % s))
        with torch.no_grad():
            NC.render_path(poses, hwf, K, chunk, kw, savedir=d)
        create_index_and_dist('bench', '000000', MASK, basedir=base, train_img_num=0, val_img_num=0, test_img_num=VIEWS)
        v = dist_to_weight('bench', basedir=base, test_number=VIEWS, val_number=0, train_number=0, c=C)
        G.load_view_maps(os.path.join(base, 'logs', 'blender_paper_bench', 'index_and_weight', 'test'), list(range(VIEWS)), Ns)
        return v

    def one_call():
        return build_scene_maps(kw, poses, hwf, K, MASK, c=C, chunk=chunk).v

    def clear():
        for c in (G._VIEW_CACHE, G._VIEW_MAPS, G._VIEW_ORI):
            c.clear()
    render_only()                                             # warm-up: weight images packed, kernels loaded
    res = {'shape': '%d views %dx%d, D8 W256 NeRF, 64 + 128 samples, point set = views %s' % (VIEWS, SIDE, SIDE, MASK),
           'render_only_s': [], 'one_call_s': [], 'file_pipeline_s': [], 'file_pipeline_bytes_on_disk': None, 'one_call_bytes_on_disk': 0}
    devnull = open(os.devnull, 'w')
    for _ in range(2):
        res['render_only_s'].append(wall(render_only)[0])
        clear()
        t, v1 = wall(one_call)
        res['one_call_s'].append(t)
        clear()
        base = tempfile.mkdtemp(prefix='scene_maps_bench_')
        out, sys.stdout = sys.stdout, devnull                 # (the mirrors print a line per view, as the reference's scripts do)
        try:
            t, v2 = wall(lambda: files(base))
        finally:
            sys.stdout = out
        res['file_pipeline_s'].append(t)
        res['file_pipeline_bytes_on_disk'] = tree_bytes(base)
        shutil.rmtree(base)
        assert abs(v1 - v2) <= 1e-5 * v2, (v1, v2)
    res['v'] = v1
    res['one_call_minus_render_s'] = [a - b for a, b in zip(res['one_call_s'], res['render_only_s'])]
    res['file_pipeline_minus_render_s'] = [a - b for a, b in zip(res['file_pipeline_s'], res['render_only_s'])]
    res['note'] = ('wall clock around a device synchronisation; the file pipeline writes and reads a temporary directory of the local disk '
                   '(page cache warm: written and read back within seconds); the one call renders the 8 views once, the file '
                   'pipeline too')
    return res


ROUNDS = 3


def foreground_arms(dev):
    from nerfail_amd import GaussNet as G, nerf_to_coord as NC, run_nerf as RN
    from nerfail_amd.scene import PointSet, build_scene_maps, foreground_pixels, view_map, view_map_pixels
    from nerfail_amd import ops
    kw = render_kwargs(dev)
    focal, K = synth.lego_intrinsics(SIDE, SIDE)
    hwf = [SIDE, SIDE, focal]
    poses = torch.from_numpy(np.stack([synth.pose_spherical(-180. + 45. * i, -30., 4.) for i in range(VIEWS)]).astype(np.float32))
    images = synth.disc_alpha_image(VIEWS, SIDE, SIDE, seed=1).astype(np.uint8)
    chunk = 1024 * 32
    P = SIDE * SIDE
    ps = PointSet.from_render(kw, poses[MASK], hwf, K, chunk)              # (also the warm-up: weight images packed, kernels loaded)
    dimg = [torch.from_numpy(images[i]).to(dev) for i in range(VIEWS)]
    lists = [foreground_pixels(im) for im in dimg]
    n = [int(l.shape[0]) for l in lists]

    def clear():
        for c in (G._VIEW_CACHE, G._VIEW_MAPS, G._VIEW_ORI):
            c.clear()

    def full_call():
        return build_scene_maps(kw, poses, hwf, K, None, c=C, chunk=chunk, images=images, point_set=ps)

    def fg_call():
        return build_scene_maps(kw, poses, hwf, K, None, c=C, chunk=chunk, images=images, point_set=ps, foreground_only=True)

    def render_full():
        with torch.no_grad():
            for c2w in poses:
                NC.render(SIDE, SIDE, K, chunk=chunk, c2w=c2w[:3, :4], **kw)

    def render_lists():
        with torch.no_grad():
            for c2w, pix in zip(poses, lists):
                NC.render_pixels(SIDE, SIDE, K, pix, chunk=chunk, c2w=c2w[:3, :4], **kw)
    res = {'shape': '%d views %dx%d, D8 W256 NeRF, 64 + 128 samples, point set prebuilt from views %s (%d points), disc images' % (VIEWS, SIDE, SIDE, MASK, ps.Ns),
           'n_per_view': n, 'n_over_P': sum(n) / float(VIEWS * P), 'rounds': ROUNDS,
           'full_call_s': [], 'foreground_call_s': [], 'render_full_s': [], 'render_lists_s': []}
    fg_call()
    clear()                                                                # warm-up of the new path
    for _ in range(ROUNDS):
        t, a = wall(full_call)
        res['full_call_s'].append(t)
        clear()
        t, b = wall(fg_call)
        res['foreground_call_s'].append(t)
        clear()
        res['render_full_s'].append(wall(render_full)[0])
        res['render_lists_s'].append(wall(render_lists)[0])
        assert b.rendered['test'] == n and a.Ns == b.Ns
    med = lambda v: float(np.median(v))                                    # noqa: E731
    res['call_ratio'] = med(res['foreground_call_s']) / med(res['full_call_s'])
    res['render_ratio'] = med(res['render_lists_s']) / med(res['render_full_s'])
    res['full_arm_spread_s'] = {'call': max(res['full_call_s']) - min(res['full_call_s']), 'render': max(res['render_full_s']) - min(res['render_full_s'])}
    res['v'] = {'full': a.v, 'foreground': b.v}
    # ---- the three new kernels alone, on view 0
    with torch.no_grad():
        pts = NC.render(SIDE, SIDE, K, chunk=chunk, c2w=poses[0][:3, :4], **kw)[3].reshape(SIDE, SIDE, 3)
    pix = lists[0]
    fg = pts.reshape(-1, 3).index_select(0, pix.long())
    c2w = poses[0][:3, :4]
    arms = {'pixel_list': lambda: ops.fg_pixel_list(dimg[0]), 'ray_gen_list': lambda: RN.ray_gen_list(SIDE, SIDE, K, c2w, 2., 6., pix),
            'ray_gen_whole_view': lambda: RN.ray_gen(SIDE, SIDE, K, c2w, 2., 6.),
            'list_search_zero_and_fold': lambda: view_map_pixels(fg, pix, (SIDE, SIDE), ps, C), 'view_map_whole_view': lambda: view_map(pts, ps, C)}
    want = view_map(pts, ps, C)[0].reshape(2, P, 8)
    got = view_map_pixels(fg, pix, (SIDE, SIDE), ps, C)[0].reshape(2, P, 8)
    assert torch.equal(got[:, pix.long()], want[:, pix.long()]) and int((got != 0).any(-1).any(0).sum()) <= n[0]
    times = {k: [] for k in arms}
    for it in range(WARMUP + RUNS):
        for k, fn in arms.items():                                         # alternated
            ms = event_ms(fn)
            if it >= WARMUP:
                times[k].append(ms)
    res['kernels_view0'] = {k: summary(v) for k, v in times.items()}
    res['kernels_view0']['n'] = n[0]
    new_ms = sum(res['kernels_view0'][k]['ms_median'] for k in ('pixel_list', 'ray_gen_list', 'list_search_zero_and_fold'))
    res['new_kernels_ms_per_view'] = new_ms
    # what of the render's time is not proportional to n / P, beside the full arm's spread and the new kernels
    res['render_excess_s'] = med(res['render_lists_s']) - res['n_over_P'] * med(res['render_full_s'])
    res['call_excess_s'] = med(res['foreground_call_s']) - res['n_over_P'] * med(res['full_call_s'])
    res['note'] = ('wall clock around a device synchronisation, arms alternated; *_excess_s = the foreground arm minus n_over_P x the full arm, '
                   'to be read beside full_arm_spread_s and VIEWS x new_kernels_ms_per_view; the call also holds the per-view host reads '
                   '(the list length, the two counts of the inverted-index build) and register_view, which do not shrink with n')
    return res


def sharded_arms(dev):
    from nerfail_amd import GaussNet as G
    from nerfail_amd.scene import build_scene_maps
    kw = render_kwargs(dev)
    focal, K = synth.lego_intrinsics(SIDE, SIDE)
    hwf = [SIDE, SIDE, focal]
    poses = torch.from_numpy(np.stack([synth.pose_spherical(-180. + 45. * i, -30., 4.) for i in range(VIEWS)]).astype(np.float32))
    chunk = 1024 * 32

    def clear():
        for c in (G._VIEW_CACHE, G._VIEW_MAPS, G._VIEW_ORI):
            c.clear()

    def plain_call():
        return build_scene_maps(kw, poses, hwf, K, MASK, c=C, chunk=chunk)

    def keyword_call():
        return build_scene_maps(kw, poses, hwf, K, MASK, c=C, chunk=chunk, shard_batch=VIEWS)
    res = {'shape': '%d views %dx%d, D8 W256 NeRF, 64 + 128 samples, point set = views %s; one rank, no process group' % (VIEWS, SIDE, SIDE, MASK),
           'rounds': ROUNDS, 'plain_call_s': [], 'shard_batch_call_s': []}
    plain_call()
    clear()                                                                # warm-up: weight images packed, kernels loaded
    for _ in range(ROUNDS):
        t, a = wall(plain_call)
        res['plain_call_s'].append(t)
        clear()
        t, b = wall(keyword_call)
        res['shard_batch_call_s'].append(t)
        clear()
        assert a.v == b.v and a.rendered == b.rendered and b.owned == {'test': list(range(VIEWS))} and b.world == 1
    med = lambda v: float(np.median(v))                                    # noqa: E731
    res['plain_arm_spread_s'] = max(res['plain_call_s']) - min(res['plain_call_s'])
    res['median_difference_s'] = med(res['shard_batch_call_s']) - med(res['plain_call_s'])
    res['inside_the_plain_arm_spread'] = bool(abs(res['median_difference_s']) <= res['plain_arm_spread_s'])
    res['note'] = ('wall clock around a device synchronisation, arms alternated; one rank owns every view, so the keyword changes no '
                   'launch - nothing here measures several devices')
    return res


def main():
    dev = torch.device('cuda:0')
    res = {'device': torch.cuda.get_device_name(0), 'warmup': WARMUP, 'runs': RUNS, 'command': 'python tools/scene_maps_bench.py',
           'commit': subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True).stdout.strip()
           or os.environ.get('NERFAIL_COMMIT', 'unknown')}
    if '--foreground' in sys.argv:
        res['command'] += ' --foreground'
        res['foreground'] = foreground_arms(dev)
        default_out = 'r28_fg_scene_maps_bench.json'
    elif '--sharded' in sys.argv:
        res['command'] += ' --sharded'
        res['sharded'] = sharded_arms(dev)
        default_out = 'r29_sharded_scene_maps_bench.json'
    else:
        res['kernel'] = kernel_arms(dev)
        if '--skip-pipeline' not in sys.argv:
            res['pipeline'] = pipeline_arms(dev)
        default_out = 'r23_scene_maps_bench.json'
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', default_out)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
