"""The hand-off from an attack's export epoch to a ready RayBatcher, through the files (the reference's road) and through
retrain.PoisonedTrainSet, and nerfail_export_train_views against nerfail_export_u8 on the chip, in one session at the
reference's shape: 100 train views of 800x800, the BGRA export x_rgba in batches of 4.

  1  the hand-off, both arms starting from the same float export on the device and ending with a RayBatcher over 100 views:
       file  per batch ops.export_u8 and one host copy (what on_export receives), per view a PNG written with PIL (the encoder
             and its compression level are recorded: the arm depends on them), then load_blender_data(train_dir=...),
             training_images(white_bkgd=True) and the uploading RayBatcher constructor;
       sink  per batch PoisonedTrainSet.put (one launch), then RayBatcher.from_resident.
     Wall clock around each arm with the device idle before and after; median and max - min of `--reps` (default 3) after
     `--warmup` (default 1), the arms alternated.
  2  the kernel alone: nerfail_export_train_views (16 bytes read, 4 + 12 written per pixel = 32) next to nerfail_export_u8
     (16 + 4 = 20) over the same 100-view tensor (1.0 GB: more than the 256 MB last-level cache), event-timed, median of
     `--kernel-reps` (default 20), in GB/s, and their ratio.

No ratio is claimed in advance. Prints one JSON object; --out F also writes it to F (profiles/<round>_retrain_bench.json)."""
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.igsm2d_bench import alternate, opt_arg, summary, views  # noqa: E402

H = W = 800
VIEWS, BATCH = 100, 4
PNG_COMPRESS_LEVEL = 6                                                     # PIL's default (cv2.imwrite, which the reference writes with, defaults to 3)


def write_scene(root, poses):
    """A Blender-format scene whose train split has VIEWS frames (their images come from train_dir) and one val / test view."""
    from PIL import Image
    import synth
    for split, n in (('train', VIEWS), ('val', 1), ('test', 1)):
        os.makedirs(os.path.join(root, split))
        frames = [{'file_path': './%s/r_%d' % (split, i), 'rotation': 0.1, 'transform_matrix': poses[i].tolist()} for i in range(n)]
        json.dump({'camera_angle_x': synth.LEGO_CAMERA_ANGLE_X, 'frames': frames}, open(os.path.join(root, 'transforms_%s.json' % split), 'w'))
        if split != 'train':
            Image.fromarray(np.full((H, W, 4), 255, np.uint8), 'RGBA').save(os.path.join(root, split, 'r_0.png'))


def main():
    import PIL
    from PIL import Image
    import synth
    from nerfail_amd import _lib, ops
    from nerfail_amd.load_blender import load_blender_data, training_images
    from nerfail_amd.retrain import PoisonedTrainSet
    from nerfail_amd.train import RayBatcher
    reps, warmup, kreps = opt_arg('--reps', 3), opt_arg('--warmup', 1), opt_arg('--kernel-reps', 20)
    dev = torch.device('cuda:0')
    base = views(BATCH, dev).to(torch.float32)
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.empty((VIEWS, H, W, 4), dtype=torch.float32, device=dev)
    for lo in range(0, VIEWS, BATCH):                                      # the clean views plus a bounded perturbation, unrounded
        x[lo:lo + BATCH] = base
        x[lo:lo + BATCH, ..., :3] += (torch.rand((BATCH, H, W, 3), device=dev, generator=g) - .5) * 64.
    poses = np.stack([synth.pose_spherical(3.6 * i, -30., 4.) for i in range(VIEWS)]).astype(np.float32)
    focal, K = synth.lego_intrinsics(H, W)
    tmp = tempfile.mkdtemp(prefix='retrain_bench_')
    root = os.path.join(tmp, 'scene')
    write_scene(root, poses)
    res = {'device': torch.cuda.get_device_name(0), 'reps': reps, 'warmup': warmup, 'kernel_reps': kreps,
           'shape': '%d views of %dx%d BGRA, exported in batches of %d' % (VIEWS, H, W, BATCH),
           'png_encoder': 'PIL %s (zlib), compress_level %d' % (PIL.__version__, PNG_COMPRESS_LEVEL)}
    kept = {}

    def file_arm():
        adv = os.path.join(tmp, 'adv')
        shutil.rmtree(adv, ignore_errors=True)
        os.makedirs(adv)
        host = torch.empty((BATCH, H, W, 4), dtype=torch.uint8, pin_memory=True)
        for lo in range(0, VIEWS, BATCH):
            host.copy_(ops.export_u8(x[lo:lo + BATCH]))
            for j, img in enumerate(host.numpy()):
                Image.fromarray(np.ascontiguousarray(img[..., [2, 1, 0, 3]]), 'RGBA').save(os.path.join(adv, 'r_%d.png' % (lo + j)),
                                                                                              compress_level=PNG_COMPRESS_LEVEL)
        images, p, _, hwf, i_split = load_blender_data(root, train_dir=adv)
        imgs = training_images(images, white_bkgd=True, train_dir=adv)
        kept['file'] = RayBatcher(imgs, p, i_split[0], hwf, K, 2., 6.)

    def sink_arm():
        sink = PoisonedTrainSet(list(range(VIEWS)), H, W, 4)
        for lo in range(0, VIEWS, BATCH):
            sink.put(list(range(lo, lo + BATCH)), x[lo:lo + BATCH])
        sink.require_complete()
        kept['sink'] = RayBatcher.from_resident(sink.images, poses, list(range(VIEWS)), [H, W, focal], K, 2., 6.)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3
    runs = {'file': [], 'sink': []}
    for r in range(warmup + reps):
        for name, fn in (('file', file_arm), ('sink', sink_arm)):
            ms = wall_ms(fn)
            if r >= warmup:
                runs[name].append(ms)
    res['handoff'] = {k: summary(v) for k, v in runs.items()}
    res['handoff']['same_targets'] = bool(torch.equal(kept['file'].images, kept['sink'].images))
    res['file_over_sink'] = res['handoff']['file']['median_ms'] / res['handoff']['sink']['median_ms']
    kept.clear()
    shutil.rmtree(tmp, ignore_errors=True)
    torch.cuda.empty_cache()

    # ---- 2: the kernels alone, over the same tensor
    lib = _lib.load()
    P = H * W
    adv = torch.empty((VIEWS, H, W, 4), dtype=torch.uint8, device=dev)
    tgt = torch.empty((VIEWS, H, W, 3), dtype=torch.float32, device=dev)
    slots = (_lib.ctypes.c_int32 * VIEWS)(*range(VIEWS))
    p = lambda t: _lib.c_p(t.data_ptr())                                   # noqa: E731

    def train_views():
        _lib.check(lib.nerfail_export_train_views(p(x), 4, VIEWS, P, slots, VIEWS, p(adv), p(tgt), _lib.stream()))

    def export_u8():
        _lib.check(lib.nerfail_export_u8(p(x), x.numel(), p(adv), _lib.stream()))
    k = alternate({'export_train_views': train_views, 'export_u8': export_u8}, kreps, 5)
    out = {}
    for name, per_pixel in (('export_train_views', 32), ('export_u8', 20)):
        s = summary(k[name])
        s.update(bytes_per_pixel=per_pixel, bytes=per_pixel * P * VIEWS, GB_per_s=per_pixel * P * VIEWS / (s['median_ms'] * 1e-3) / 1e9)
        out[name] = s
    res['kernels'] = out
    res['train_views_over_export_u8_bandwidth'] = out['export_train_views']['GB_per_s'] / out['export_u8']['GB_per_s']
    res['note'] = ('hand-off: wall clock, device idle before and after each arm, arms alternated; kernels: HIP events around each call, '
                   'alternated; spread = max - min over the reps; export_train_views runs %d launches of 16 views' % -(-VIEWS // 16))
    line = json.dumps(res)
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
