#!/usr/bin/env python3
"""One rank of the multi-rank PIPELINE test (tests/test_hip_multirank_pipeline.py): scene maps -> attack -> hand-off -> retrain in
one process group. Started as a fresh process by tests/mgpu/launcher.py with RANK / WORLD_SIZE / MASTER_* in the environment; every
rank uses HIP device 0 (the test box has one GPU), so the group is gloo and sharding stages device tensors through pinned host
memory. The scene is tests/test_hip_scene.py's: 40 x 40 views, COUNTS = test 4 / train 2 / val 1, mask_list [0, 2, 3] (4 800 points:
the grid kernel), D4 W64 nets with 8 + 8 samples, synth.disc_alpha_image images; shard_batch = 4.

    python tests/mgpu/pipeline_rank.py OUTDIR          -> OUTDIR/pipe_w{world}_r{rank}.npz and .json
"""
import datetime
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path[:0] = [os.path.dirname(TESTS), TESTS]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import synth  # noqa: E402
import test_hip_scene as TS  # noqa: E402  (the toy scene: COUNTS, ANGLE, C, _render_kwargs, _toy_net)

SIDE, MASK, SHARD_BATCH, LABEL, CLASSES = 40, [0, 2, 3], 4, 3, 8
TAGS = ('test', 'train', 'val')


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


class TinyCls(torch.nn.Module):
    """Global mean, then a Linear; evaluated in float64 and rounded once (logits that do not depend on a summation order)."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.lin = torch.nn.Linear(3, CLASSES)
        with torch.no_grad():
            self.lin.weight.copy_(torch.randn(CLASSES, 3, generator=g) * 0.05)
            self.lin.bias.copy_(torch.randn(CLASSES, generator=g) * 0.1)

    def forward(self, x):
        return (x.double().mean((2, 3)) @ self.lin.weight.double().t() + self.lin.bias.double()).float()


def retrain_args(basedir):
    return types.SimpleNamespace(multires=10, i_embed=0, use_viewdirs=True, multires_views=4, N_importance=8, N_samples=8, netdepth=4,
                                 netwidth=64, netdepth_fine=4, netwidth_fine=64, netchunk=65536, lrate=5e-4, lrate_decay=250, basedir=basedir,
                                 expname='pipe_toy', ft_path=None, no_reload=False, perturb=1., white_bkgd=True, raw_noise_std=0.,
                                 dataset_type='blender', no_ndc=False, lindisp=False, N_rand=64, no_batching=True, precrop_iters=0,
                                 precrop_frac=.5, i_print=2, i_weights=1000, chunk=1024)


def main(out_dir):
    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    if world > 1:                          # a short timeout: a dead peer ends the rest instead of holding them
        dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from nerfail_amd import GaussNet as G, run_nerf as RN
    from nerfail_amd.attack import STAT_FIELDS, nerfail_s, nerfail_s_into
    from nerfail_amd.retrain import PoisonedTrainSet, poisoned_retrain, render_splits, render_view_u8
    from nerfail_amd.scene import build_scene_maps, perturbation_table
    out, meta = {}, {'world': world, 'rank': rank}

    def barrier():
        if world > 1:
            dist.barrier()

    kw = TS._render_kwargs()
    focal, K = synth.lego_intrinsics(SIDE, SIDE)
    hwf = [SIDE, SIDE, focal]
    poses = {s: torch.from_numpy(np.stack([synth.pose_spherical(TS.ANGLE[s] + 40. * i, -30., 4.) for i in range(n)]).astype(np.float32))
             for s, n in TS.COUNTS.items()}
    images = {s: synth.disc_alpha_image(n, SIDE, SIDE, seed=len(s)).astype(np.uint8) for s, n in TS.COUNTS.items()}

    # ---- 1, 2, 3, 7: the maps - sharded (both routes) and with the keywords left alone
    def build(tag, **more):
        seen = []
        m = build_scene_maps(kw, poses, hwf, K, MASK, c=TS.C, chunk=1024, images=images,
                             on_view=lambda s, i, vid, wi: seen.append([s, i, list(wi.shape)]), **more)
        out[tag + '_points'] = bits(m.point_set.points)
        registered = []
        for s, n in TS.COUNTS.items():
            assert m.view_ids[s] == [(m.scene_key, s, i) for i in range(n)]              # all ids of every split, on every rank
            for i in range(n):
                key = G._view_key(m.view_ids[s][i], m.Ns)
                assert (key in G._VIEW_MAPS) == (key in G._VIEW_CACHE) == (key in G._VIEW_ORI)
                if key not in G._VIEW_MAPS:
                    continue
                registered.append([s, i])
                sd = G._VIEW_CACHE[key].state_dict()
                out['%s_%s%d_map' % (tag, s, i)] = bits(G._VIEW_MAPS[key])
                for k in G.ViewIndex.ARRAYS:           # (a view without entries keeps one never-written element per entry array)
                    keep = sd['n_entries'] if k in ('packed', 'w_sorted') else None
                    out['%s_%s%d_idx_%s' % (tag, s, i, k)] = bits(sd[k][:keep])
                out['%s_%s%d_idx_meta' % (tag, s, i)] = np.array([sd['Ns'], sd['P'], sd['n_entries'], sd['n_rows']] + list(sd['fp'][1:]), np.int64)
        meta[tag] = dict(Ns=m.Ns, grid=m.point_set._grid is not None, v=float(m.v).hex(), rendered=m.rendered, owned=m.owned,
                         shard_batch=m.shard_batch, maps_world=m.world, seen=seen, registered=registered,
                         batches_test=[len(b[2]) for b in m.batches('test', SHARD_BATCH)])
        if more.get('save_dir'):           # what this rank's call left on disk for its own views: read back before the peers are waited for
            own_files = {}
            for s, i in registered:
                d = os.path.join(more['save_dir'], 'index_and_weight', s)
                on_disk = torch.load(os.path.join(d, '%d.pth' % i))
                side = G.ViewIndex.load(os.path.join(d, '%d.idx.pth' % i))
                own_files['%s%d' % (s, i)] = bool(not on_disk.is_cuda and torch.equal(on_disk.to(dev), G._VIEW_MAPS[G._view_key(m.view_ids[s][i], m.Ns)])
                                                  and tuple(side.src) == G._file_sig(os.path.join(d, '%d.pth' % i)) and side.Ns == m.Ns)
            barrier()
            meta[tag]['own_files'] = own_files
            meta[tag]['saved'] = {s: sorted(os.listdir(os.path.join(more['save_dir'], 'index_and_weight', s))) for s in TS.COUNTS}
        return m

    m_full = build('full', shard_batch=SHARD_BATCH, save_dir=os.path.join(out_dir, 'w%d_saved' % world))
    build('fg', shard_batch=SHARD_BATCH, foreground_only=True)
    m_plain = build('plain')
    if world == 1:
        build('plainfg', foreground_only=True)

    # ---- 4: nerfail_s over the sharded maps, and over maps every rank built in full
    s0 = perturbation_table(images['test'][MASK])

    def record(tag, res):
        out[tag + '_best'], out[tag + '_last'] = bits(res.best), bits(res.last)
        meta[tag] = dict(stats=[[float(d[k]).hex() for k in STAT_FIELDS] for d in res.stats], best_epoch=res.best_epoch)

    record('attack_sharded', nerfail_s(TS._toy_net(), s0, m_full.batches('test', SHARD_BATCH), LABEL, 2, a=2., epsilon=32., log=None))
    record('attack_plain', nerfail_s(TS._toy_net(), s0, m_plain.batches('test', SHARD_BATCH), LABEL, 2, a=2., epsilon=32., log=None))

    # ---- 5: the export epoch into a sink per rank, gather(); one process filling a sink from the same best table
    sink = PoisonedTrainSet(m_full.view_ids['train'], SIDE, SIDE, 4)
    res = nerfail_s_into(sink, TS._toy_net(), s0, m_full.batches('train', SHARD_BATCH), LABEL, 2, a=2., epsilon=32., log=None)
    record('handoff', res)
    meta['handoff']['own'] = [v[2] for v in sink.view_ids if v in sink.filled]
    try:
        sink.require_complete()
        meta['handoff']['before_gather'] = ''
    except ValueError as e:
        meta['handoff']['before_gather'] = str(e)
    sink.gather()
    meta['handoff']['missing'] = [v[2] for v in sink.missing()]
    out['sink_images'], out['sink_adv'] = bits(sink.images), bits(sink.adv_u8)
    alone = PoisonedTrainSet(m_plain.view_ids['train'], SIDE, SIDE, 4)
    alone.put(m_plain.view_ids['train'], TS._toy_net().export_forward(res.best, None, None, m_plain.view_ids['train'])[1])
    out['alone_images'], out['alone_adv'] = bits(alone.images), bits(alone.adv_u8)

    # ---- 6: poisoned_retrain on the gathered sink
    all_poses = torch.cat([poses['train'], poses['val'], poses['test']]).numpy()
    i_split = [[0, 1], [2], [3, 4, 5, 6]]
    cls = TinyCls().to(dev).eval().requires_grad_(False)
    originals = {t: torch.from_numpy(images[t]).to(dev) for t in TAGS}
    ev = dict(num_classes=CLASSES, resize_to=SIDE, batch=2)

    def make_nerf(args, calls):
        def make(attempt):
            calls.append(attempt)
            torch.manual_seed(100 + attempt + 10 * rank)      # the ranks START apart: train() makes them rank 0's
            made = RN.create_nerf(args)
            with torch.no_grad():        # a freshly initialised NeRF has sigma <= 0 nearly everywhere: the fixtures' nudge
                for net in (made[0]['network_fn'], made[0]['network_fine']):
                    net.alpha_linear.bias += 0.5
            return made
        return make

    def params(r):
        return np.concatenate([bits(p).reshape(-1) for net in (r.render_kwargs_train['network_fn'], r.render_kwargs_train['network_fine'])
                               for p in net.parameters()])

    args = retrain_args(os.path.join(out_dir, 'w%d_retrain' % world))
    lines, calls = [], []
    r = poisoned_retrain(sink, all_poses, i_split, hwf, K, args, make_nerf=make_nerf(args, calls), originals=originals, model=cls,
                         model_name='tiny_linear', label=LABEL, eval_tags=TAGS, N_iters=5, seed=0, log=lines.append, **ev)
    out['retrain_params'] = params(r)
    meta['retrain'] = dict(logged=[[it, float(l).hex(), float(p).hex()] for it, l, p in r.logged], attempts=r.attempts, calls=calls,
                           last=r.last_iteration, lines=len(lines), reports={t: repr(r.reports[t]) for t in sorted(r.reports)})
    for t in TAGS:
        out['retrain_renders_' + t] = bits(r.renders[t])
        mine = torch.stack([render_view_u8(r.render_kwargs_test, torch.from_numpy(all_poses[i]), hwf, K, args.chunk)
                            for i in i_split[{'train': 0, 'val': 1, 'test': 2}[t]]])           # every pose, on this rank alone
        out['retrain_self_' + t] = bits(mine)
    # render_splits by itself: sharded against the call without the keyword, same weights, plus rank 0's folders
    ro = os.path.join(out_dir, 'w%d_ro' % world)
    sharded = render_splits(r.render_kwargs_test, all_poses, i_split, hwf, K, args.chunk, savedir=ro, start=3, sharded=True)
    plain = render_splits(r.render_kwargs_test, all_poses, i_split, hwf, K, args.chunk)
    meta['render_splits'] = {t: bool(torch.equal(sharded[t], plain[t]) and torch.equal(sharded[t], r.renders[t])) for t in TAGS}
    barrier()
    meta['render_splits']['folders'] = sorted(os.listdir(ro))
    meta['render_splits']['files'] = sorted(os.listdir(os.path.join(ro, 'renderonly_test_000003')))

    # the restart rule: a floor nothing reaches - both ranks restart together
    args2 = retrain_args(os.path.join(out_dir, 'w%d_restart' % world))
    lines, calls = [], []
    r2 = poisoned_retrain(sink, all_poses, i_split, hwf, K, args2, make_nerf=make_nerf(args2, calls), eval_tags=(), N_iters=5, seed=0,
                          restart_below=(2, 1e9), max_restarts=1, log=lines.append)
    out['restart_params'] = params(r2)
    meta['restart'] = dict(logged=[[it, float(l).hex(), float(p).hex()] for it, l, p in r2.logged], attempts=r2.attempts, calls=calls,
                           restarting=sum('restarting' in s for s in lines), kept=sum('no restart left' in s for s in lines))

    # a checkpoint found on disk: refused on every rank
    args3 = retrain_args(os.path.join(out_dir, 'w%d_ckpt' % world))
    if rank == 0:
        d = os.path.join(args3.basedir, args3.expname)
        os.makedirs(d)
        rkt = r.render_kwargs_train
        torch.save({'global_step': 2, 'network_fn_state_dict': rkt['network_fn'].state_dict(),
                    'network_fine_state_dict': rkt['network_fine'].state_dict(), 'optimizer_state_dict': r.optimizer.state_dict()},
                   os.path.join(d, '000002.tar'))
    barrier()
    try:
        poisoned_retrain(sink, all_poses, i_split, hwf, K, args3, N_iters=5, eval_tags=(), log=None)        # (the default make_nerf)
        meta['ckpt'] = ''
    except ValueError as e:
        meta['ckpt'] = str(e)

    np.savez(os.path.join(out_dir, 'pipe_w%d_r%d.npz' % (world, rank)), **out)
    with open(os.path.join(out_dir, 'pipe_w%d_r%d.json' % (world, rank)), 'w') as f:
        json.dump(meta, f)
    assert [l for l in open('/proc/self/maps') if 'libnerfail_hip' in l], 'libnerfail_hip.so is not mapped: the product path did not run'
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    print('rank %d/%d ok' % (rank, world), flush=True)


if __name__ == '__main__':
    main(sys.argv[1])
