"""The classifier-input stage of a stock victim, stock ops against the native kernels, in one session at the workload's shape:
8 views of 800 x 800 (x_rgba) -> [8,3,299,299].

  1  forward, and forward plus backward to x_rgba (the gradient of sum(out * g) for a fixed g):
       stock   gauss_net.cold_tail's ops as they stand: transpose, torch.where, full_like, .contiguous(), _resize.resize;
       native  _resize.classifier_input (one launch each way).
     HIP events, arms alternated call by call, median of `--reps` (default 20) after `--warmup` (default 5), max - min per arm.
  2  the kernels alone over 64 views (655 MB of x_rgba: more than the 256 MB last-level cache): nerfail_cls_input_resize_fwd
     (16 bytes read per source pixel, 12 written per output pixel) and _bwd at R = 1 (12 read per output pixel, 4 of alpha read and
     16 written per source pixel - the alpha reads touch every 64-byte line of x_rgba, both figures are given), as TB/s next to
     the 6.3 TB/s a streaming kernel reaches here.
  3  an observation, not an assertion: whether two runs of the stock backward on identical input give identical bits, and the
     same for the native one.

No ratio is claimed in advance. Prints one JSON object; --out F also writes it to F (profiles/<round>_resize_bench.json)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.igsm2d_bench import alternate, opt_arg, summary, views  # noqa: E402

H = W = 800
SIZE = 299
VIEWS, KERNEL_VIEWS = 8, 64


def stock(x_rgba):
    from nerfail_amd._resize import resize
    c = x_rgba.transpose(2, 3).transpose(1, 2)
    c3 = torch.where(c[:, 3:4] > 0, c[:, :3], torch.full_like(c[:, :3], 255.)).contiguous()
    return resize(c3, SIZE)


def main():
    from nerfail_amd import ops
    from nerfail_amd._resize import classifier_input
    reps, warmup = opt_arg('--reps', 20), opt_arg('--warmup', 5)
    dev = torch.device('cuda:0')
    gen = torch.Generator(device=dev).manual_seed(1)
    x = views(VIEWS, dev).to(torch.float32)
    x[..., :3] += (torch.rand((VIEWS, H, W, 3), device=dev, generator=gen) - .5) * 64.
    g = torch.randn((VIEWS, 3, SIZE, SIZE), device=dev, generator=gen)
    res = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'warmup': warmup,
           'shape': '%d views of %dx%d x_rgba -> [%d,3,%d,%d]' % (VIEWS, H, W, VIEWS, SIZE, SIZE)}

    def fwd_bwd(fn):
        def run():
            leaf = x.detach().requires_grad_(True)
            (fn(leaf) * g).sum().backward()
            return leaf.grad
        return run

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(x)
        return run
    native = lambda t: classifier_input(t, SIZE)   # noqa: E731
    f = alternate({'stock': fwd(stock), 'native': fwd(native)}, reps, warmup)
    fb = alternate({'stock': fwd_bwd(stock), 'native': fwd_bwd(native)}, reps, warmup)
    for name, runs in (('forward', f), ('forward_backward', fb)):
        out = {k: dict(summary(v), runs_ms=[round(t, 4) for t in v]) for k, v in runs.items()}
        out['stock_over_native'] = out['stock']['median_ms'] / out['native']['median_ms']
        out['faster_by_more_than_both_spreads'] = bool(out['stock']['median_ms'] - out['native']['median_ms']
                                                       > out['stock']['spread_ms'] + out['native']['spread_ms'])
        res[name] = out
    res['max_abs_difference_of_the_two_forwards'] = float((fwd(stock)() - fwd(native)()).abs().max())

    # 3: run-to-run bits of either backward
    a, b = fwd_bwd(stock)(), fwd_bwd(stock)()
    res['stock_backward_two_runs_identical_bits'] = bool(torch.equal(a, b))
    a, b = fwd_bwd(native)(), fwd_bwd(native)()
    res['native_backward_two_runs_identical_bits'] = bool(torch.equal(a, b))
    del a, b

    # 2: the kernels alone, beyond the last-level cache
    big = x.repeat(KERNEL_VIEWS // VIEWS, 1, 1, 1).contiguous()
    gbig = g.repeat(KERNEL_VIEWS // VIEWS, 1, 1, 1).contiguous()[None]
    k = alternate({'fwd': lambda: ops.cls_input_resize(big, 0, SIZE, SIZE),
                   'bwd': lambda: ops.cls_input_resize_bwd(gbig, big, 0, H, W)}, reps, warmup)
    src_px, out_px = KERNEL_VIEWS * H * W, KERNEL_VIEWS * 3 * SIZE * SIZE
    bytes_ = {'fwd': 16 * src_px + 4 * out_px, 'bwd': 4 * out_px + (4 + 16) * src_px, 'bwd_alpha_as_lines': 4 * out_px + (16 + 16) * src_px}
    res['kernels'] = {}
    for name in ('fwd', 'bwd'):
        s = summary(k[name])
        s['bytes'] = bytes_[name]
        s['TB_per_s'] = bytes_[name] / (s['median_ms'] * 1e-3) / 1e12
        s['fraction_of_6.3_TB_per_s'] = s['TB_per_s'] / 6.3
        res['kernels'][name] = s
    res['kernels']['bwd']['TB_per_s_counting_alpha_as_whole_lines'] = bytes_['bwd_alpha_as_lines'] / (res['kernels']['bwd']['median_ms'] * 1e-3) / 1e12
    res['kernels']['note'] = ('%d views (%.0f MB of x_rgba), op call included (output allocated per call); HIP events, median of %d after %d'
                              % (KERNEL_VIEWS, 16 * src_px / 1e6, reps, warmup))
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
