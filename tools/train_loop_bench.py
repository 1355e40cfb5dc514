"""The product training loops in one session at the shipped shape: 800x800, 100 resident synthetic views, D8 W256 coarse + fine,
64 + 128 samples, N_rand = 1024, perturb = 1, white background. Three arms, alternated `--rounds` times (default 3):

  a  load_blender.train_step in a Python loop as a user writes it, with a legacy np.random.RandomState (RN:746-801 literally:
     host permutation of H*W, image upload, get_rays of the full image, three gathers, float(loss) every step);
  b  nerfail_amd.train.train, no_batching (one view per step, pixels from the device-side index shuffle);
  c  nerfail_amd.train.train, use_batching (ranges of one permutation of all training pixels).

Per arm and round: the median ms per step over `--steps` (default 60, at least 50) steps after warm-up. Arm a waits for the
GPU every step, so its steps are timed on the host; arms b and c never wait, so an event is recorded at every batch() call
and a step is the time between two events (the whole-loop wall time per step is reported next to it).

--baseline-tree DIR: a checkout of the parent commit with its library built; its bench_sections.train_bench (the step
`bench.py --full` reports as the `train` section) runs there in a child process of this session, and this tree's own runs
in-process, for the figure the loops are held against. Prints one JSON object; --out F also writes it to F."""
import json
import os
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench_sections as BS  # noqa: E402

BS._heavy_imports()
import synth  # noqa: E402

N_VIEWS, N_RAND = 100, 1024
CHILD = ('import json, sys, torch; sys.path.insert(0, "."); sys.path.insert(0, "tests"); import bench_sections as BS; BS._heavy_imports(); '
         'r = BS.train_bench(torch.device("cuda:0"), steps=%d, warmup=5); '
         'print("BASELINE " + json.dumps({k: r[k] for k in ("ms_per_step", "ms_per_step_mean_whole_loop", "warmup")}))')


def opt_arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def scene():
    rs = np.random.RandomState(0)
    base = rs.uniform(size=(BS.H, BS.W, 3)).astype(np.float32)
    images = np.empty((N_VIEWS, BS.H, BS.W, 3), np.float32)
    for i in range(N_VIEWS):
        images[i] = np.roll(base, 8 * i, axis=0)
    poses = np.stack([synth.pose_spherical(3.6 * i - 180., -30., 4.) for i in range(N_VIEWS)])
    focal, K = synth.lego_intrinsics(BS.H, BS.W)
    return images, poses, [BS.H, BS.W, focal], K


def arm_state(dev):
    from nerfail_amd.optim import Adam
    nets = [BS.make_net(s, dev)[1] for s in (31, 32)]
    for n_ in nets:
        n_.requires_grad_(True)
    opt = Adam([p for n_ in nets for p in n_.parameters()], lr=5e-4, betas=(0.9, 0.999))
    kw = {'network_query_fn': None, 'perturb': 1., 'N_importance': BS.N_IMPORTANCE, 'network_fine': nets[1], 'N_samples': BS.N_SAMPLES,
          'network_fn': nets[0], 'use_viewdirs': True, 'white_bkgd': True, 'raw_noise_std': 0., 'ndc': False, 'lindisp': False}
    return {'opt': opt, 'kw': kw, 'step': 0}


def run_a(st, data, steps, warmup):
    from nerfail_amd.load_blender import train_step
    images, poses, hwf, K = data
    rng = st.setdefault('rng', np.random.RandomState(0))
    per = []
    for s in range(warmup + steps):
        t = time.perf_counter()
        train_step(images, poses, np.arange(N_VIEWS), hwf, K, st['kw'], st['opt'], st['step'], N_rand=N_RAND, rng=rng)   # float(loss): waits
        st['step'] += 1
        per.append((time.perf_counter() - t) * 1e3)
    per = per[warmup:]
    return {'median_ms': float(np.median(per)), 'wall_ms_per_step': float(np.mean(per))}


class Stamped:
    """A RayBatcher whose batch() records an event first: the time between two events is one step of the loop."""

    def __init__(self, rb):
        self.rb, self.images, self.marks = rb, rb.images, []

    def batch(self, *a, **k):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append(e)
        return self.rb.batch(*a, **k)


def run_loop(st, data, steps, warmup, use_batching):
    from nerfail_amd.train import RayBatcher, train
    images, poses, hwf, K = data
    if 'rb' not in st:
        st['rb'] = RayBatcher(images, poses, np.arange(N_VIEWS), hwf, K, 2., 6., seed=0)
    args = types.SimpleNamespace(N_rand=N_RAND, no_batching=not use_batching, lrate=5e-4, lrate_decay=250, i_print=10 ** 9,
                                 i_weights=10 ** 9, precrop_iters=0, precrop_frac=.5, chunk=1024 * 32, basedir='.', expname='bench')
    sb = Stamped(st['rb'])
    n = warmup + steps + 1                     # (the last step only closes the last interval)
    torch.cuda.synchronize()
    t = time.perf_counter()
    train(images, poses, [np.arange(N_VIEWS)], hwf, K, args, st['kw'], st['opt'], st['step'], N_iters=st['step'] + n + 1, batcher=sb,
          log=lambda s: None)
    t_host = time.perf_counter() - t
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    st['step'] += n
    per = [sb.marks[i].elapsed_time(sb.marks[i + 1]) for i in range(warmup, warmup + steps)]
    return {'median_ms': float(np.median(per)), 'wall_ms_per_step': wall * 1e3 / n, 'host_ms_per_step': t_host * 1e3 / n}


def baseline(tree, steps):
    r = subprocess.run([sys.executable, '-c', CHILD % steps], cwd=tree, capture_output=True, text=True, timeout=300)
    for line in r.stdout.splitlines():
        if line.startswith('BASELINE '):
            return json.loads(line[9:])
    raise RuntimeError('baseline child failed (%d):\n%s\n%s' % (r.returncode, r.stdout[-2000:], r.stderr[-2000:]))


def main():
    steps, rounds = max(50, opt_arg('--steps', 60)), opt_arg('--rounds', 3)
    tree = opt_arg('--baseline-tree', None, str)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    res = {'device': torch.cuda.get_device_name(0), 'shape': '800x800, %d views, D8 W256, 64+128 samples, N_rand %d' % (N_VIEWS, N_RAND),
           'steps_per_round': steps, 'rounds': rounds}
    if tree is not None:
        res['parent_train_bench'] = [baseline(tree, steps)]
    own = BS.train_bench(dev, steps=steps, warmup=5)
    res['this_tree_train_bench'] = {k: own[k] for k in ('ms_per_step', 'ms_per_step_mean_whole_loop')}
    data = scene()
    arms = {'a_train_step_loop': lambda st, w: run_a(st, data, steps, w),
            'b_train_no_batching': lambda st, w: run_loop(st, data, steps, w, False),
            'c_train_use_batching': lambda st, w: run_loop(st, data, steps, w, True)}
    states = {k: arm_state(dev) for k in arms}
    runs = {k: [] for k in arms}
    for r in range(rounds):
        for k, fn in arms.items():
            runs[k].append(fn(states[k], 8 if r == 0 else 3))
            print('round %d %s %s' % (r, k, json.dumps(runs[k][-1])), file=sys.stderr, flush=True)
    if tree is not None:
        res['parent_train_bench'].append(baseline(tree, steps))
    for k in arms:
        res[k] = {'rounds': runs[k], 'median_ms_per_step': float(np.median([x['median_ms'] for x in runs[k]]))}
    a, b, c = (res[k]['median_ms_per_step'] for k in arms)
    res['a_over_b'], res['a_over_c'] = a / b, a / c
    ref = float(np.median([x['ms_per_step'] for x in res['parent_train_bench']])) if tree is not None else res['this_tree_train_bench']['ms_per_step']
    res['benched_step_ms'], res['b_over_benched_step'], res['c_over_benched_step'] = ref, b / ref, c / ref
    res['note'] = ('per arm and round: median ms per step over steps_per_round steps after warm-up, arms alternated inside a round; '
                   'a: host clock around each step (it waits for the GPU every step); b, c: time between events recorded at each '
                   'batch() call; benched_step_ms: median of the parent tree\'s train_bench runs (before and after the arms) when '
                   '--baseline-tree is given, else this tree\'s')
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
