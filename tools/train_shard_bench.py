"""What data-parallel training (nerfail_amd.train.train with a process group) costs and what it can be expected to give,
measured on ONE GPU. Shape: 800x800, 100 resident synthetic views, D8 W256 coarse + fine, 64 + 128 samples, perturb = 1,
white background, no_batching.

  a  train() of this tree against train() of the parent (--baseline-tree DIR: a checkout of the parent commit with its
     library built) at N_rand = 1024, without a process group: the arms alternated `--rounds` times (default 3), each run a
     fresh process. What the feature costs a 1-rank run: nothing, if the two agree within the parent's own spread.
  b  the step time of train() at N_rand = 1024, 512, 256 and 128: the per-rank shapes of 1, 2, 4 and 8 ranks.
  c  the gradient arena's all-reduce through a 1-rank 'nccl' (RCCL) group with NERFAIL_FORCE_COLLECTIVE=1, HIP events around
     it, and train() on that path at N_rand = 1024. One rank: communicator, stream semantics and launch cost are real, the
     exchange over xGMI is not.

From b and c: `projection`, step(N_rand / k) + all-reduce(1 rank) for k ranks. It is a PROJECTION from one GPU, not a
measurement of k GPUs: the all-reduce of a real k-rank group moves 2 (k - 1) / k of the arena over the links and is not in
it. Step times: the median time between HIP events recorded at each batch() call, `--steps` (default 60) steps after warm-up.
This process never touches the GPU; every measurement is a child process. Prints one JSON object; --out F also writes it."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RANDS = (1024, 512, 256, 128)

# Runs in this tree and in the parent's (cwd = the tree): only what both have.
CHILD = r'''
import json, sys, time, types
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import numpy as np, torch
import bench_sections as BS
BS._heavy_imports()
import synth
from nerfail_amd.optim import Adam
from nerfail_amd.train import RayBatcher, train
N_RANDS, STEPS, WARMUP, NCCL = %r, %d, %d, %d
N_VIEWS = 100
dev = torch.device("cuda:0")
torch.manual_seed(0)
rs = np.random.RandomState(0)
base = rs.uniform(size=(BS.H, BS.W, 3)).astype(np.float32)
images = np.stack([np.roll(base, 8 * i, axis=0) for i in range(N_VIEWS)])
poses = np.stack([synth.pose_spherical(3.6 * i - 180., -30., 4.) for i in range(N_VIEWS)])
focal, K = synth.lego_intrinsics(BS.H, BS.W)
hwf = [BS.H, BS.W, focal]
nets = [BS.make_net(s, dev)[1] for s in (31, 32)]
for n_ in nets:
    n_.requires_grad_(True)
opt = Adam([p for n_ in nets for p in n_.parameters()], lr=5e-4, betas=(0.9, 0.999))
kw = {"network_query_fn": None, "perturb": 1., "N_importance": BS.N_IMPORTANCE, "network_fine": nets[1], "N_samples": BS.N_SAMPLES,
      "network_fn": nets[0], "use_viewdirs": True, "white_bkgd": True, "raw_noise_std": 0., "ndc": False, "lindisp": False}
rb = RayBatcher(images, poses, np.arange(N_VIEWS), hwf, K, 2., 6., seed=0)
extra, out = {}, {}
if NCCL:
    import os, datetime
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29535")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=datetime.timedelta(seconds=120))
    os.environ["NERFAIL_FORCE_COLLECTIVE"] = "1"
    extra["timing"] = {}

class Stamped:
    def __init__(self, rb):
        self.rb, self.images, self.marks, self.n_global = rb, rb.images, [], 0
    def batch(self, *a, **k):
        e = torch.cuda.Event(enable_timing=True); e.record(); self.marks.append(e)
        o = self.rb.batch(*a, **k)
        self.n_global = getattr(self.rb, "n_global", 0)
        return o

step = 0
for n_rand in N_RANDS:
    args = types.SimpleNamespace(N_rand=n_rand, no_batching=True, lrate=5e-4, lrate_decay=250, i_print=10 ** 9, i_weights=10 ** 9,
                                 precrop_iters=0, precrop_frac=.5, chunk=1024 * 32, basedir=".", expname="bench")
    sb = Stamped(rb)
    n = WARMUP + STEPS + 1
    torch.cuda.synchronize()
    t = time.perf_counter()
    train(images, poses, [np.arange(N_VIEWS)], hwf, K, args, kw, opt, step, N_iters=step + n + 1, batcher=sb, log=lambda s: None, **extra)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t
    step += n
    per = [sb.marks[i].elapsed_time(sb.marks[i + 1]) for i in range(WARMUP, WARMUP + STEPS)]
    out[str(n_rand)] = {"median_ms": float(np.median(per)), "wall_ms_per_step": wall * 1e3 / n}
if NCCL:
    ev = extra["timing"]["allreduce_events"]
    ms = [e0.elapsed_time(e1) for e0, e1, _ in ev][WARMUP:]
    out["allreduce"] = {"bytes": int(ev[0][2]), "calls": len(ev), "median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)),
                        "max_ms": float(np.max(ms)), "backend": str(dist.get_backend())}
    dist.destroy_process_group()
print("RESULT " + json.dumps(out))
'''


def opt_arg(name, default, cast=int):
    return cast(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def child(tree, n_rands, steps, warmup, nccl=False):
    r = subprocess.run([sys.executable, '-c', CHILD % (tuple(n_rands), steps, warmup, int(nccl))], cwd=tree, capture_output=True, text=True,
                       timeout=420)
    for line in r.stdout.splitlines():
        if line.startswith('RESULT '):
            return json.loads(line[7:])
    raise RuntimeError('child in %s failed (%d):\n%s\n%s' % (tree, r.returncode, r.stdout[-2000:], r.stderr[-3000:]))


def main():
    steps, rounds, warmup = opt_arg('--steps', 60), opt_arg('--rounds', 3), 8
    tree = opt_arg('--baseline-tree', None, str)
    res = {'shape': '800x800, 100 views, D8 W256, 64+128 samples, perturb 1, no_batching', 'steps_per_run': steps, 'rounds': rounds}
    if tree is not None:                                   # (a) this tree against the parent, one rank, no process group
        a = {'parent': [], 'this_tree': []}
        for r in range(rounds):
            for k, t in (('parent', tree), ('this_tree', ROOT)):
                a[k].append(child(t, (1024,), steps, warmup)['1024'])
                print('a round %d %s %s' % (r, k, json.dumps(a[k][-1])), file=sys.stderr, flush=True)
        med = {k: [x['median_ms'] for x in v] for k, v in a.items()}
        res['a_world1_vs_parent'] = {'runs': a, 'median_ms': med, 'parent_spread_ms': max(med['parent']) - min(med['parent']),
                                     'this_minus_parent_ms': sorted(med['this_tree'])[len(med['this_tree']) // 2] - sorted(med['parent'])[len(med['parent']) // 2]}
    b = child(ROOT, N_RANDS, steps, warmup)                 # (b) the per-rank shapes
    res['b_step_ms_by_n_rand'] = b
    print('b %s' % json.dumps(b), file=sys.stderr, flush=True)
    c = child(ROOT, (1024,), steps, warmup, nccl=True)       # (c) the arena all-reduce and the loop on the RCCL path, 1 rank
    res['c_nccl_1rank'] = c
    print('c %s' % json.dumps(c), file=sys.stderr, flush=True)
    ar = c['allreduce']['median_ms']
    one = b['1024']['median_ms']
    res['projection'] = {str(k): {'per_rank_n_rand': 1024 // k, 'step_ms': b[str(1024 // k)]['median_ms'] + (ar if k > 1 else 0.),
                                  'over_one_rank': one / (b[str(1024 // k)]['median_ms'] + (ar if k > 1 else 0.))} for k in (1, 2, 4, 8)}
    res['note'] = ('a: median ms per step of train() at N_rand 1024, fresh process per run, parent and this tree alternated; b: this tree at '
                   'the per-rank batch of 1, 2, 4, 8 ranks; c: 1-rank nccl group with the forced collective - the all-reduce of the whole '
                   'arena between HIP events, and the loop with it; projection: b + c, NOT a multi-GPU measurement (a k-rank all-reduce '
                   'moves 2 (k - 1) / k of the arena over the links, which one rank does not)')
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
