#!/usr/bin/env python3
"""bench.py - the reference's headline workload on MI355X: full-image NeRF render, Blender-lego shape.

One "step" = one pass of the hot path over one synthetic 800x800 view (BASELINE.json configs[1]):
ray generation -> 64 coarse samples -> fused posenc+MLP (D=8, W=256) -> composite -> 128 importance
samples (sorted merge) -> fine MLP -> composite + per-pixel argmax point (nerf_to_coord's render).
Everything is resident in HBM when the timed region starts; weights are seeded random (no dataset /
checkpoint in the container); poses follow load_blender.py's pose_spherical.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A plain run measures only the headline: the render group (the timed steps above). `--full` adds every other section
(CPU baselines, training step, attack loop, 8-NN, split-precision render; with N > 1 the strong-scaling render leg and
the sharded attack leg). `--dump-outputs DIR` writes what the last timed step returned (rank 0) as DIR/<name>.npy.

This file is the PARENT: it never imports numpy / torch and never touches the GPU. Every section group runs in a fresh
child (`bench.py --child <group> --out <file>`, code in bench_sections.py) that appends result objects to <file> one JSON
line at a time, so whatever a child measured before it died is kept. Groups: render | cpu | train | attack | extras.

STDOUT carries exactly ONE line: the contract line, < 1800 bytes (round 5: round 4's 20 KB line was cut in half by the
driver's capture). Everything else the sections measured goes to `bench_detail.json` (path in the line's `detail` key;
NERFAIL_BENCH_DETAIL overrides it) and to stderr.

N > 1, either way one process per GPU:
  * under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` every rank is one parent + one render
    child (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment); rank 0 prints the line;
  * started plainly (`python bench.py --gpus N`, WORLD_SIZE unset) this parent spawns the N render children itself with that
    environment. Asking for N ranks and getting fewer is an error (exit 2), never a line that says n_gpus 1.
Rays / views are independent units: each rank renders its own view, no data-path collective ("scaling": "weak").
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
LINE_LIMIT = 1800                       # bytes; the driver's stdout tail is 2000 characters
GROUP_OF = {'selftest': 'selftest', 'render': 'render', 'cpu': 'cpu', 'train': 'train', 'attack': 'attack', 'knn': 'extras', 'f16x3': 'extras'}
GROUPS = ('selftest', 'render', 'cpu', 'train', 'attack', 'extras')
FULL_SECTIONS = 'render,cpu,train,attack,knn,f16x3'
PLAIN_SECTIONS = 'render'
PG_TIMEOUT_S = 180                      # the children's process-group timeout (bench_sections.child_render reads it)


# ------------------------------------------------------------------------------------------------------------ children
def _read_results(path):
    """Merge the JSON objects a child appended to `path` ('_merge': true = update a nested dict instead of replacing it)."""
    out = {}
    try:
        lines = open(path).read().splitlines()
    except OSError:
        return out
    for ln in lines:
        try:
            obj = json.loads(ln)
        except ValueError:
            continue                                 # a line cut short by the child's death
        merge = obj.pop('_merge', False)
        for k, v in obj.items():
            if merge and isinstance(v, dict) and isinstance(out.get(k), dict):
                out[k].update(v)
            else:
                out[k] = v
    return out


class _Child:
    """One section group in a fresh process. The parent has not imported torch and never touches the GPU, so starting a
    process here is always allowed; the child's stdout goes to our stderr (RCCL / MIOpen banners must not reach the ONE line)."""

    def __init__(self, group, argv, timeout, env=None):
        self.group, self.timeout, self.t0 = group, timeout, time.time()
        fd, self.path = tempfile.mkstemp(prefix='nf_bench_%s_' % group, suffix='.jsonl')
        os.close(fd)
        e = dict(os.environ)
        e.update(env or {})
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--child', group, '--out', self.path] + argv,
                                     stdout=sys.stderr, stderr=sys.stderr, env=e)

    def wait(self, deadline=None):
        """-> (results so far, status dict)."""
        deadline = self.t0 + self.timeout if deadline is None else deadline
        try:
            rc = self.proc.wait(timeout=max(1.0, deadline - time.time()))
            why = None
        except subprocess.TimeoutExpired:
            self.proc.kill()                         # exactly the process we started
            rc = self.proc.wait()
            why = 'timeout after %.0f s' % (time.time() - self.t0)
        res = _read_results(self.path)
        try:
            os.unlink(self.path)
        except OSError:
            pass
        st = {'rc': rc, 'seconds': round(time.time() - self.t0, 1)}
        if rc != 0:
            st['error'] = 'rc %d (%s)' % (rc, why or ('killed by signal %d' % -rc if rc < 0 else 'exit code'))
        return res, st


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def rank_envs(n, port):
    """Environment of the N render children of a self-launched run: what torch.distributed.run would have set."""
    return [{'RANK': str(r), 'LOCAL_RANK': str(r), 'WORLD_SIZE': str(n), 'LOCAL_WORLD_SIZE': str(n),
             'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port)} for r in range(n)]


# ---------------------------------------------------------------------------------------------------- the contract line
def _num(x, nd=4):
    """Round for the line (6 significant digits are plenty; the detail file keeps full precision)."""
    if isinstance(x, bool) or x is None:
        return x
    if isinstance(x, int):
        return x
    try:
        return float('%.*g' % (nd + 2, float(x)))
    except (TypeError, ValueError):
        return None


def _get(d, *path):
    for k in path:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


def contract_line(detail, world, args, detail_path):
    """The ONE stdout line from everything the children reported: contract keys, one roofline object, one cpu_baseline
    object, flat scalars for the other two numbers of BASELINE.json's metric string (rays/s fwd+bwd, attack iterations/s).
    Guaranteed shorter than LINE_LIMIT: optional keys are dropped, least important first, until it fits."""
    rf = detail.get('roofline') or {}
    cb = detail.get('cpu_baseline') or None
    line = {
        'metric': detail.get('metric', 'rays/sec'), 'value': _num(detail.get('value')), 'unit': detail.get('unit', 'rays/s'),
        'n_gpus': detail.get('n_gpus', world), 'steps': args.steps, 'warmup': args.warmup,
        'ms_per_step': _num(detail.get('ms_per_step')), 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
        'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': 'lego-shaped 800x800 full render (nerf_to_coord.render, incl. argmax point), 64+128 samples, '
                               'D=8 W=256, one view per step per GPU (BASELINE.json configs[1])',
                   'rays_per_step_per_gpu': _get(detail, 'config', 'rays_per_step_per_gpu') or 640000,
                   'parallelism': 'view per rank, no collective'},
        'roofline': ({'kernel': rf.get('kernel'), 'bound': rf.get('bound'), 'achieved': _num(rf.get('achieved')),
                      'peak': rf.get('peak'), 'unit': rf.get('unit'), 'frac': _num(rf.get('frac')),
                      'traffic': _num(rf.get('traffic')), 'avg_launch_ms': _num(rf.get('avg_launch_ms')),
                      'mfma_busy': _num(rf.get('mfma_busy')), 'clock_GHz': _num(rf.get('clock_GHz'))} if rf else None),
        'cpu_baseline': ({'value': _num(cb.get('value')), 'unit': cb.get('unit'), 'cores': cb.get('cores'),
                          'kind': cb.get('kind'), 'sample': str(cb.get('sample', ''))[:110]} if isinstance(cb, dict) else None),
        'rccl_ranks': detail.get('rccl_ranks'),
    }
    # optional keys, most important first (dropped from the END when the line is too long)
    tr, at = detail.get('train') or {}, detail.get('attack') or {}
    gp = at.get('gauss_path_fused_step') or at.get('gauss_path_deterministic') or {}    # N = 1: the sign step fused into K11 (round 6)
    opt = [
        ('fwd_bwd_rays_per_sec', _num(tr.get('train_rays_per_sec_fwd_bwd'))),
        ('fwd_bwd_ms_per_step', _num(tr.get('ms_per_step'))),
        ('fwd_bwd_frac', _num(_get(tr, 'roofline', 'frac'))),
        ('attack_iters_per_sec', _num(gp.get('iters_per_sec') if gp else at.get('iters_per_sec'))),
        ('attack_ms_per_iter', _num(gp.get('ms_per_iter') if gp else at.get('ms_per_iter'))),
        # the primary fraction divides the bytes this form HAS to move (1.19 GB per 8-view iteration) by
        # the measured time. SURVEY 8(d)'s nominal 1.60 GB (fp32 x and images, four gradient channels) are bytes these
        # kernels do not move - by them K10 alone would run above the 8 TB/s peak - so that figure is kept as a secondary key.
        ('attack_frac', _num(_get(gp, 'roofline', 'frac_compulsory'))),
        ('attack_frac_survey_bytes', _num(_get(gp, 'roofline', 'frac'))),
        ('composite_GBps', _num(_get(detail, 'composite_scan', 'achieved'))),
        ('composite_frac', _num(_get(detail, 'composite_scan', 'frac'))),
        # the loop as INTEGRATION.md section 1 writes it (default settings, views named by id: original-image logits computed
        # once); the reference-shaped recompute-every-step figure stays in the detail file (end_to_end_victim_cnn)
        ('attack_e2e_iters_per_sec', _num(_get(at, 'end_to_end_victim_cnn_cached_original_logits', 'iters_per_sec')
                                          or _get(at, 'end_to_end_victim_cnn', 'iters_per_sec'))),
        ('cpu_fwd_bwd_rays_per_sec', _num(_get(detail, 'cpu_baseline_fwd_bwd', 'value'))),
        ('cpu_attack_iters_per_sec', _num(_get(detail, 'cpu_baseline_attack', 'value'))),
        ('render_strong_rays_per_sec', _num(_get(detail, 'render_strong', 'rays_per_sec'))),
        ('allreduce_ms', _num(_get(at, 'allreduce_ms'))),
        ('wall_seconds', detail.get('wall_seconds')),
    ]
    errors = sorted(k for k in detail if k.endswith('_error'))
    if errors:
        line['errors'] = [('%s: %s' % (k, detail[k]))[:80] for k in errors[:4]]
    line['detail'] = detail_path
    for k, v in opt:
        if v is not None:
            line[k] = v
    keys = [k for k, v in opt if v is not None]
    while len(json.dumps(line)) >= LINE_LIMIT and keys:
        line.pop(keys.pop())
    for k in ('errors', 'detail'):
        if len(json.dumps(line)) >= LINE_LIMIT:
            line.pop(k, None)
    assert len(json.dumps(line)) < LINE_LIMIT
    return line


def _write_detail(detail, path):
    try:
        with open(path, 'w') as f:
            json.dump(detail, f, indent=1, sort_keys=True)
            f.write('\n')
        return path
    except OSError as e:
        print('bench.py: cannot write %s (%s)' % (path, e), file=sys.stderr)
        return None


# -------------------------------------------------------------------------------------------------------------- parent
def parent_main(args, argv):
    t_start = time.time()
    sections = args.section_set
    env_world = os.environ.get('WORLD_SIZE')
    if env_world is not None and int(env_world) != args.gpus:
        print('bench.py: --gpus %d but the launcher started WORLD_SIZE=%s ranks' % (args.gpus, env_world), file=sys.stderr)
        sys.exit(2)
    world = args.gpus
    rank = int(os.environ.get('RANK', '0'))
    self_launch = env_world is None and world > 1
    detail, status = {}, {}

    def absorb(group, res, st):
        status[group] = st
        for k, v in res.items():
            if isinstance(v, dict) and isinstance(detail.get(k), dict):
                detail[k].update(v)
            else:
                detail[k] = v
        if 'error' in st:
            detail[group + '_error'] = st['error']

    render_timeout = 120 + 4.0 * (args.steps + args.warmup) + (PG_TIMEOUT_S + 220 if world > 1 else 0)   # N > 1: + the two legs
    if 'render' in sections:
        if self_launch:
            kids = [_Child('render', argv, render_timeout, env=e) for e in rank_envs(world, _free_port())]
            deadline = time.time() + render_timeout
            outs = [k.wait(deadline) for k in kids]
            absorb('render', *outs[0])
            bad = ['rank %d: %s' % (r, st['error']) for r, (_, st) in enumerate(outs) if 'error' in st]
            if bad:
                detail['render_error'] = '; '.join(bad)[:300]
            status['render']['ranks'] = [st['rc'] for _, st in outs]
        else:
            absorb('render', *_Child('render', argv, render_timeout).wait())
        if detail.get('value') is not None and detail.get('n_gpus') != world:
            detail['render_error'] = 'asked for %d ranks, the timed region ran on %s' % (world, detail.get('n_gpus'))
            detail['value'] = None
    if world == 1:                                   # the extra single-GPU sections belong to the N = 1 run
        if not args.no_cpu_baseline and 'cpu' in sections:
            # right behind the render child, alone on the box's cores (beside it the numpy port measured 687 rays/s on the
            # 14 cores left over instead of 900 on all 16: the render child's launch thread spins)
            absorb('cpu', *_Child('cpu', argv, timeout=200).wait())
        if not args.no_attack:
            for group, need in (('train', {'train'}), ('attack', {'attack'}), ('extras', {'knn', 'f16x3'}), ('selftest', {'selftest'})):
                if sections & need:
                    absorb(group, *_Child(group, argv, timeout=240).wait())
    detail['sections'] = status
    detail['wall_seconds'] = round(time.time() - t_start, 1)
    if 'render_f16x3' in detail and detail.get('value'):
        detail['render_f16x3']['speedup_vs_f32_kernel_this_run'] = detail['render_f16x3']['rays_per_sec'] / detail['value']
    # the contract line exists once the render child has delivered it; an extra section's failure is reported inside it.
    # Decided BEFORE the line is assembled (the assembly used to fill in "value": null and hide the failure).
    ok = 'render' not in sections or detail.get('value') is not None
    if rank != 0:                                    # under a launcher only rank 0's child emits the line
        ok = status.get('render', {}).get('rc', 0) == 0
    if rank == 0:
        path = os.environ.get('NERFAIL_BENCH_DETAIL') or os.path.join(ROOT, 'bench_detail.json')
        path = _write_detail(detail, path)
        print(json.dumps(detail), file=sys.stderr, flush=True)
        shown = os.path.relpath(path, ROOT) if path and path.startswith(ROOT + os.sep) else path
        print(json.dumps(contract_line(detail, world, args, shown)), flush=True)
    sys.exit(0 if ok else 1)


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--full', action='store_true',
                    help='run every section (default sections %s; N > 1: also the strong-scaling and sharded attack legs); '
                         'a plain run measures the render group only' % FULL_SECTIONS)
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='write the arrays the last timed render step returned (rank 0) to DIR/<name>.npy')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-attack', action='store_true', help='skip the extra train / attack / knn / f16x3 sections')
    ap.add_argument('--dist-backend', default='nccl', help='nccl (= RCCL; default) or gloo (rehearsal on a 1-GPU box)')
    ap.add_argument('--device', type=int, default=None, help='force the HIP device index (rehearsal: all ranks on GPU 0)')
    ap.add_argument('--sections', default=None,
                    help='comma list of render,cpu,train,attack,knn,f16x3 (the contract keys of the JSON line need render); '
                         'default: %s, with --full or --child: %s' % (PLAIN_SECTIONS, FULL_SECTIONS))
    ap.add_argument('--child', default=None, choices=GROUPS, help='internal / profiling: run ONE section group in this process')
    ap.add_argument('--out', default=None, help='with --child: append result objects to this file instead of printing them')
    args = ap.parse_args(argv)
    if args.sections is None:             # a child runs the one group it was asked for, with all of that group's legs
        args.sections = FULL_SECTIONS if args.full or args.child else PLAIN_SECTIONS
    args.section_set = set(x for x in args.sections.split(',') if x)
    unknown = args.section_set - set(GROUP_OF)
    if unknown:
        ap.error('unknown sections: %s' % ', '.join(sorted(unknown)))
    if args.gpus < 1:
        ap.error('--gpus must be >= 1')
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    return args


def main():
    args = parse_args()
    if args.child:
        import bench_sections
        bench_sections.run_child(args)
        return
    parent_main(args, sys.argv[1:])


if __name__ == '__main__':
    main()
else:
    from bench_sections import *         # noqa: F401,F403  imported as a module (tests, tools): the section functions
    from bench_sections import _heavy_imports
    _heavy_imports(gpu=False)
