"""The stage after the attack (README "retrain"; the paper's closing claim): a second NeRF is trained on the attacked training
views, inherits the perturbation, and its renders are classified again (test_for_inception's step=1, "nerf"). The reference
glues this stage together through the disk - the attack writes PNGs, load_blender_data(train_dir=...) decodes them (LB:62-65),
run_nerf composites them on white (RN:587-588), nerf_render_only.py renders every split into folders, transfer_files.py moves
the folders, test_for_inception reads them back. Here it is one call that stays on the device:

    PoisonedTrainSet     the sink an attack's export epoch fills (attack.nerfail / igsm_2d / uap_2d(export_sink=...),
                         attack.nerfail_s_into): one launch per exported batch (nerfail_export_train_views) writes the uint8 image the PNG would hold AND the float32 training target
                         the file path would make of it, bit for bit, into two resident stores
    render_splits        nerf_render_only.py:619-656: every split rendered, uint8 in cv2's channel order, resident
    attack_output_dir    transfer_files.get_test_dir_after_nerf_attack: the folder names test_for_inception reads
    poisoned_retrain     gather -> require_complete -> RayBatcher.from_resident -> train.train (with the README's restart advice) ->
                         render_splits -> model_test.evaluate_views per split

More than one rank (torch.distributed): an export epoch fills each rank's sink with that rank's views, PoisonedTrainSet.gather()
makes every sink complete, train.train is data-parallel, render_splits(sharded=True) splits the poses and exchanges the uint8
views; poisoned_retrain does all of it and returns the same result on every rank. Executed with gloo ranks sharing one device
(tests/test_hip_multirank_pipeline.py): the claim is the one-rank bits, no speed-up was measured on several devices.

Not supported (the reference's blender configs use neither): half_res and white_bkgd=False targets."""
import os

import numpy as np
import torch

from . import model_test as MT
from . import ops
from . import sharding
from .run_nerf_helpers import _cuda

SPLIT_OF_TAG = {'train': 0, 'val': 1, 'test': 2}          # i_split's order (LB:73)


class PoisonedTrainSet:
    """The attacked training views of one scene, resident. `view_ids`: the train views, under the (hashable) names the attack
    exports them by, in the order the NeRF indexes them (i_split[0]); slot s holds view view_ids[s]. `channels`: 4 for the BGRA
    export x_rgba of NeRFail-S / NeRFail, 3 for the BGR export x_rgb of IGSM-2D / UAP-2D.

        images  float32 [n,H,W,3]  exactly what load_blender.training_images(load_blender_data(train_dir=...)[0], white_bkgd=True,
                                   train_dir=...) returns for the train split of the written PNGs: the NeRF's targets, RGB
        adv_u8  uint8 [n,H,W,C]    exactly what cv2.imread(..., IMREAD_UNCHANGED) returns for those PNGs: what
                                   model_test.evaluate_views takes as the attacked side of the step=0 measurement

    An attack fills it through put(); a view exported twice keeps the later export. Slots never written hold zeros and
    require_complete() refuses to go on with them."""

    def __init__(self, view_ids, H, W, channels, white_bkgd=True, half_res=False, device=None):
        if not white_bkgd:
            raise NotImplementedError('PoisonedTrainSet: white_bkgd=False targets (RN:590: alpha dropped) are not supported - the '
                                      'hand-off kernel composites on white, as every blender config of the reference does')
        if half_res:
            raise NotImplementedError('PoisonedTrainSet: half_res targets (LB:95-104: cv2.INTER_AREA after the decode) are not '
                                      'supported - load the written PNGs through load_blender_data(half_res=True) instead')
        if channels not in (3, 4):
            raise ValueError('PoisonedTrainSet: channels must be 4 (BGRA export) or 3 (BGR export)')
        self.view_ids = list(view_ids)
        if not self.view_ids or len(set(self.view_ids)) != len(self.view_ids):
            raise ValueError('PoisonedTrainSet: view_ids must name at least one view, each once')
        self.H, self.W, self.channels = int(H), int(W), int(channels)
        self.dev = _cuda() if device is None else torch.device(device)
        n = len(self.view_ids)
        self.slot_of = {v: s for s, v in enumerate(self.view_ids)}
        self.images = torch.zeros((n, self.H, self.W, 3), dtype=torch.float32, device=self.dev)
        self.adv_u8 = torch.zeros((n, self.H, self.W, self.channels), dtype=torch.uint8, device=self.dev)
        self.filled = set()
        self.remote = set()                                   # of `filled`: the views another rank's put() wrote (gather)

    def put(self, view_ids, x):
        """THE launch: the float export x [B,H,W,C] (a device tensor, C = channels) of the views `view_ids` into their slots."""
        if view_ids is None:
            raise ValueError('PoisonedTrainSet.put: the exported batch carries no view ids - give every export batch its ids '
                             '(weight_and_index, ori_img, view_ids)')
        ids = [int(v) if isinstance(v, (np.integer, torch.Tensor)) else v for v in view_ids]
        unknown = [v for v in ids if v not in self.slot_of]
        if unknown:
            raise ValueError('PoisonedTrainSet.put: view(s) %s are not among the %d train views of this set' % (unknown, len(self.view_ids)))
        if not isinstance(x, torch.Tensor) or tuple(x.shape) != (len(ids), self.H, self.W, self.channels):
            raise ValueError('PoisonedTrainSet.put: x must be a tensor [%d,%d,%d,%d] (got %s)'
                             % (len(ids), self.H, self.W, self.channels, tuple(getattr(x, 'shape', ()))))
        x = x.detach()
        if x.dtype != torch.float32 or not x.is_contiguous() or x.data_ptr() % 16:
            x = x.to(torch.float32).contiguous().clone()
        ops.export_train_views(x, [self.slot_of[v] for v in ids], self.adv_u8, self.images)
        self.filled.update(ids)
        self.remote.difference_update(ids)

    def missing(self):
        return [v for v in self.view_ids if v not in self.filled]

    def require_complete(self):
        """Raises, naming them, when views were never exported: their slots would train the NeRF on black images."""
        miss = self.missing()
        if not miss:
            return
        world = sharding.world_and_rank(None)[0]
        more = ''
        if world > 1:
            more = (' - with %d ranks an export sink holds only the views its own rank exported until gather() has made it the union of '
                    'the ranks\' sinks: call gather() on every rank after the export epoch (poisoned_retrain does)' % world)
        raise ValueError('PoisonedTrainSet: %d of %d train views were never exported: %s%s' % (len(miss), len(self.view_ids), miss, more))

    def gather(self, group=None):
        """After an export epoch on several ranks (torch.distributed; `group`, None = the default group), called on every rank:
        each rank's sink becomes the union of the ranks' sinks. One all-reduce of 2 n int32 says who filled which slot; a slot
        filled on more than one rank is a ValueError naming it, on every rank; every other filled slot travels from its owner
        by broadcast (runs of neighbouring slots of one owner in one call): a copy, so `images` and `adv_u8` hold the bits the
        owner's put() wrote. A slot no rank filled stays missing. One rank: nothing happens. A view received here still belongs
        to its owner, so a second gather() finds the same owners and changes nothing. Returns self."""
        world, rank = sharding.world_and_rank(group)
        if world == 1:
            return self
        owner = gather_slots(self.images, self.adv_u8, [v in self.filled and v not in self.remote for v in self.view_ids], group)
        twice = [self.view_ids[s] for s, o in enumerate(owner) if o == DUPLICATE]
        if twice:
            raise ValueError('PoisonedTrainSet.gather: view(s) %s were exported on more than one rank - every view of an export epoch '
                             'belongs to one rank (attack.nerfail_s_into shards its export batches that way)' % (twice,))
        self.remote = {self.view_ids[s] for s, o in enumerate(owner) if o is not None and o != rank}
        self.filled |= self.remote
        return self


DUPLICATE = -1


def gather_slots(images, adv_u8, filled, group=None):
    """The exchange behind PoisonedTrainSet.gather, over plain tensors: `images` and `adv_u8` ([n, ...], contiguous, on one
    device) and `filled` (n booleans: the slots this rank wrote). Returns the owner of every slot, the same list on every rank:
    a rank, None (nobody filled it) or DUPLICATE (more than one rank did); with a DUPLICATE nothing has been moved, else every
    owned slot of both tensors now holds its owner's bytes on every rank."""
    world, rank = sharding.world_and_rank(group)
    n = len(filled)
    mine = torch.tensor([1 if f else 0 for f in filled] + [rank if f else 0 for f in filled], dtype=torch.int32)
    who = sharding.all_reduce_sum_(mine.to(images.device), group).cpu().tolist()       # [0:n] how many ranks filled it, [n:2n] which
    owner = [None if who[s] == 0 else (who[n + s] if who[s] == 1 else DUPLICATE) for s in range(n)]
    if DUPLICATE in owner:
        return owner
    s = 0
    while s < n:
        e = s + 1
        while e < n and owner[e] == owner[s]:
            e += 1
        if owner[s] is not None:
            sharding.broadcast_(images[s:e], owner[s], group)
            sharding.broadcast_(adv_u8[s:e], owner[s], group)
        s = e
    return owner


# ---------------------------------------------------------------------------------------------- nerf_render_only.py:619-656
def _imwrite_bgr(path, img):
    """cv2.imwrite(path, img) of a uint8 [H,W,3] BGR (or [H,W,4] BGRA) host array; PIL when cv2 is absent."""
    try:
        import cv2
        cv2.imwrite(path, img)
    except ImportError:
        from PIL import Image
        if img.shape[-1] == 4:
            Image.fromarray(np.ascontiguousarray(img[..., [2, 1, 0, 3]]), 'RGBA').save(path)
        else:
            Image.fromarray(np.ascontiguousarray(img[..., ::-1]), 'RGB').save(path)


def _write_views(directory, views):
    os.makedirs(directory, exist_ok=True)
    for i, v in enumerate(views.cpu().numpy()):
        _imwrite_bgr(os.path.join(directory, '{:03d}.png'.format(i)), v)


def render_view_u8(render_kwargs, c2w, hwf, K, chunk):
    """One pose rendered with run_nerf.render and converted as model_test.evaluate_render converts it (to8b: 255 * clip(rgb, 0, 1)
    truncated to uint8, flipped to cv2's channel order): uint8 [H,W,3] on the device."""
    from .run_nerf import render
    H, W = int(hwf[0]), int(hwf[1])
    with torch.no_grad():
        rgb = render(H, W, K, chunk=chunk, c2w=c2w[:3, :4], **render_kwargs)[0]
        return (255 * torch.clamp(rgb, 0, 1)).to(torch.uint8).flip(-1).contiguous()


def render_splits(render_kwargs_test, poses, i_split, hwf, K, chunk, tags=("test", "train", "val"), savedir=None, start=0, sharded=False,
                  group=None):
    """nerf_render_only.py:619-656: for every tag the poses of its split (i_split = [train, val, test]) rendered with
    `render_kwargs_test` (near / far included). Returns {tag: uint8 [N,H,W,3]} on the device, converted as run_nerf.to8b converts
    and in cv2's channel order - what model_test.evaluate_render measures and what cv2.imread returns for the PNGs the reference
    writes. `savedir`: additionally writes savedir/renderonly_<tag>_<start:06d>/<i:03d>.png, the reference's folders.
    sharded=True (opt-in; torch.distributed, `group`, the same weights on every rank): of each tag's N poses this rank renders
    sharding.shard_range(N, rank, world), the uint8 views are exchanged (sharding.all_gather_ranges_), every rank returns the
    full tensors - the unsharded call's bits - and rank 0 alone writes `savedir`. One rank: the unsharded call."""
    world, rank = sharding.world_and_rank(group) if sharded else (1, 0)
    H, W = int(hwf[0]), int(hwf[1])
    out = {}
    for tag in tags:
        if tag not in SPLIT_OF_TAG:
            raise ValueError('render_splits: unknown tag %r (train, val or test)' % (tag,))
        idx = [int(i) for i in i_split[SPLIT_OF_TAG[tag]]]
        if not idx:
            raise ValueError('render_splits: the %s split holds no view' % tag)
        p = poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else np.asarray(poses)
        split_poses = torch.as_tensor(p[idx], dtype=torch.float32)       # on the host: a pose travels to the ray kernel by value
        if world > 1:
            lo, hi = sharding.shard_range(len(idx), rank, world)
            out[tag] = torch.empty((len(idx), H, W, 3), dtype=torch.uint8, device=_cuda())
            for i in range(lo, hi):
                out[tag][i] = render_view_u8(render_kwargs_test, split_poses[i], hwf, K, chunk)
            sharding.all_gather_ranges_(out[tag], sharding.shard_ranges(len(idx), world), group)
        else:
            out[tag] = torch.stack([render_view_u8(render_kwargs_test, c2w, hwf, K, chunk) for c2w in split_poses])
        if savedir is not None and rank == 0:
            _write_views(os.path.join(savedir, 'renderonly_{}_{:06d}'.format(tag, start)), out[tag])
    return out


def attack_output_dir(scene_name="lego", model_name="vgg16", now_class_idx=10, attack_epochs=100, print_a=2, print_e=32,
                      target_class_idx="n", base_mask_image_number=3, m1=0, m2=0, method_name="NeRFail", step=0,
                      something_need_log: dict = None):
    """transfer_files.get_test_dir_after_nerf_attack: where the views of an attack (step 0) or of the NeRF retrained on it (step 1)
    live, with train / test / val below it - the folder model_test.test_for_inception reads with the same arguments (MT:88-128;
    that function builds its path inline, so the rows stand here once more; tests/test_retrain_paths.py holds the two together).
    None for No_attack at step 0, method_name None and unknown methods, as the reference returns."""
    if method_name == "IGSM":
        method_name = "NeRFail_S"
    elif method_name == "Universal":
        method_name = "NeRFail"
    head = './output/' + model_name + '/' + {0: "attack", 1: "nerf", 2: "defense", 3: "nerf_defense"}[step] + '/' + scene_name + '/'
    e, to = '_e_' + str(print_e), '_to_' + str(target_class_idx)
    if method_name == "NeRFail":
        return head + 'NeRFail_' + str(base_mask_image_number) + 'P_' + str(attack_epochs) + to + e + '_m_' + str(m1) + '_' + str(m2)
    if method_name == "NeRFail_S":
        return head + 'NeRFail_S_' + str(base_mask_image_number) + 'P_' + str(attack_epochs) + to + e + '_a_' + str(print_a)
    if method_name == "IGSM_2D":
        return head + 'IGSM_2D_' + str(attack_epochs) + to + e + '_a_' + str(print_a)
    if method_name == "No_attack" and step != 0:
        return head + 'no_attack'
    if method_name == "Universal_2D":
        return head + 'Universal_2D_' + str(attack_epochs) + to + e + '_m_' + str(m1) + '_' + str(m2)
    return None


# ---------------------------------------------------------------------------------------------- the product call
class RetrainResult:
    """What poisoned_retrain returns. `render_kwargs_train` / `render_kwargs_test` / `optimizer`: the kept attempt's NeRF;
    `last_iteration` and `logged` ([(iteration, loss, psnr)]): train.train's; `attempts`: how many NeRFs were started;
    `renders`: {tag: uint8 [N,H,W,3]} (render_splits); `reports`: {tag: msg_dict} (model_test.report), empty without a classifier."""

    def __init__(self, render_kwargs_train, render_kwargs_test, optimizer, last_iteration, logged, attempts, renders, reports):
        self.render_kwargs_train, self.render_kwargs_test, self.optimizer = render_kwargs_train, render_kwargs_test, optimizer
        self.last_iteration, self.logged, self.attempts, self.renders, self.reports = last_iteration, logged, attempts, renders, reports


def _newest_checkpoint(args):
    """The file run_nerf.create_nerf reloads (RN:210-218)."""
    if getattr(args, 'ft_path', None) is not None and args.ft_path != 'None':
        return args.ft_path
    d = os.path.join(args.basedir, args.expname)
    ckpts = [os.path.join(d, f) for f in sorted(os.listdir(d)) if 'tar' in f] if os.path.isdir(d) else []
    return ckpts[-1] if ckpts else None


def poisoned_retrain(train_set, poses, i_split, hwf, K, args, make_nerf=None, originals=None, model=None, model_name=None, label=None,
                     eval_tags=("test", "val"), N_iters=None, seed=0, restart_below=None, max_restarts=2, save_dir=None, log=print,
                     **eval_kw):
    """The retrain stage as one call: a NeRF trained on the attacked views of `train_set` (a complete PoisonedTrainSet; its
    view_ids name the train views in the order of i_split[0], under whatever names the attack knows them by: slot s is trained
    under pose i_split[0][s]), rendered over the splits and measured as test_for_inception(step=1) measures it.

    `make_nerf(attempt)` returns create_nerf's 5-tuple for attempt 0, 1, ...; default: run_nerf.create_nerf(args). The README asks
    for a fresh NeRF ("delete the .tar files"): a start iteration other than 0 is a ValueError that names the checkpoint, unless
    resume=True is given. `args`: the namespace train.train reads (N_rand, no_batching, lrate, lrate_decay, i_print, i_weights,
    basedir, expname, chunk ...). `N_iters`, `seed`: train.train's.

    `restart_below=(iteration, psnr)`: the reference README's operating advice ("PSNR < 15 ... restart 1 or 2 times"). When the
    PSNR logged at that iteration is below the floor (or NaN) the attempt is discarded and attempt + 1 starts, at most
    `max_restarts` times; the last allowed attempt is kept whatever it logs. The iteration must be a multiple of args.i_print
    (it has to be logged), lie before the first checkpoint (args.i_weights: a discarded attempt leaves no file behind) and before
    N_iters. An attempt trains to that iteration, is judged, and goes on from there: the same steps as one uninterrupted run.

    Then render_splits over `eval_tags` - over train, test and val when `save_dir` is given, which also writes
    save_dir/<tag>/<i:03d>.png (attack_output_dir(..., step=1) names the folder test_for_inception reads) - and, with `model`,
    `model_name`, `label` and `originals` ({tag: the split's clean views, uint8, cv2 order}), evaluate_views per tag of
    `eval_tags`. near = 2, far = 6 (RN:573-574) unless given; what remains of **eval_kw goes to evaluate_views (batch,
    num_classes, resize_to).

    More than one rank (torch.distributed, the default group): every rank calls this with its own sink and the same arguments.
    train_set.gather() first makes every sink the union of what the ranks' export epochs put; train.train is data-parallel
    (rank 0's parameters, one gradient all-reduce per step, the ranks' parameters compared at every log point); `logged` is the
    same on every rank, so restart_below restarts all ranks together, and a found checkpoint is refused on every rank;
    render_splits(sharded=True) splits the poses of each tag and exchanges the views; evaluate_views then runs on every rank
    over the full renders (not sharded on purpose: 2.4 ms per 8 views, no rule for merging device records, the same bits
    everywhere). `save_dir` and the log lines are rank 0's. The RetrainResult is identical on every rank.
    Returns a RetrainResult."""
    from . import run_nerf as RN
    from .train import RayBatcher, train
    resume = bool(eval_kw.pop('resume', False))
    near, far = float(eval_kw.pop('near', 2.)), float(eval_kw.pop('far', 6.))
    world, rank = sharding.world_and_rank(None)
    train_set.gather()                                                    # (one rank: nothing happens)
    train_set.require_complete()
    i_train = [int(i) for i in i_split[0]]
    if len(train_set.view_ids) != len(i_train):
        raise ValueError('poisoned_retrain: the set holds %d views, the train split %d - slot s must hold the view of pose i_split[0][s]'
                         % (len(train_set.view_ids), len(i_train)))
    i_print, i_weights = int(getattr(args, 'i_print', 100)), int(getattr(args, 'i_weights', 10000))
    n_iters = int(getattr(args, 'N_iters', 200000)) + 1 if N_iters is None else int(N_iters)
    if restart_below is not None:
        check_at, floor = int(restart_below[0]), float(restart_below[1])
        if check_at < 1 or check_at % i_print != 0 or check_at >= i_weights or check_at >= n_iters:
            raise ValueError('poisoned_retrain: restart_below\'s iteration %d must be a multiple of i_print = %d (it has to be logged), '
                             'lie before the first checkpoint (i_weights = %d) and before N_iters = %d' % (check_at, i_print, i_weights, n_iters))
    if make_nerf is None:
        make_nerf = lambda attempt: RN.create_nerf(args)                  # noqa: E731
    evaluate = model is not None and originals is not None
    if evaluate and (model_name is None or label is None):
        raise ValueError('poisoned_retrain: a classifier needs its model_name and the label')
    say = log if log is not None and rank == 0 else (lambda *_: None)    # rank 0 speaks (train.train silences the others itself)
    attempts = 0
    while True:
        render_kwargs_train, render_kwargs_test, start, grad_vars, optimizer = make_nerf(attempts)
        attempts += 1
        if start != 0 and not resume:
            raise ValueError('poisoned_retrain: the NeRF starts at iteration %d, reloaded from %s - a retrain on attacked views starts '
                             'fresh (delete the .tar files of %s, or pass resume=True to continue that run)'
                             % (start, _newest_checkpoint(args), os.path.join(str(args.basedir), str(args.expname))))
        render_kwargs_train.update(near=near, far=far)
        render_kwargs_test.update(near=near, far=far)
        batcher = RayBatcher.from_resident(train_set.images, poses, i_train, hwf, K, near, far, seed=seed)
        run = dict(near=near, far=far, seed=seed, batcher=batcher, log=say)
        logged = []
        if restart_below is not None:
            if check_at <= start:
                raise ValueError('poisoned_retrain: restart_below\'s iteration %d is not after the start iteration %d' % (check_at, start))
            start, logged = train(None, poses, i_split, hwf, K, args, render_kwargs_train, optimizer, start, N_iters=check_at + 1, **run)
            psnr = logged[-1][2]
            if not psnr >= floor:
                if attempts <= max_restarts:
                    say('[RETRAIN] attempt %d: PSNR %s at iteration %d is below %s - restarting' % (attempts - 1, psnr, check_at, floor))
                    continue
                say('[RETRAIN] attempt %d: PSNR %s at iteration %d is below %s - kept, no restart left' % (attempts - 1, psnr, check_at, floor))
        last, more = train(None, poses, i_split, hwf, K, args, render_kwargs_train, optimizer, start, N_iters=n_iters, **run)
        logged = logged + more
        break
    tags = list(eval_tags)
    if save_dir is not None:
        tags += [t for t in ('train', 'test', 'val') if t not in tags]
    renders = render_splits(render_kwargs_test, poses, i_split, hwf, K, int(getattr(args, 'chunk', 1024 * 32)), tags=tags, sharded=world > 1)
    if save_dir is not None and rank == 0:
        for tag in ('train', 'test', 'val'):
            _write_views(os.path.join(save_dir, tag), renders[tag])
    reports = {}
    if evaluate:
        for tag in eval_tags:
            reports[tag] = MT.evaluate_views(model, model_name, renders[tag], originals[tag], label, **eval_kw)
    return RetrainResult(render_kwargs_train, render_kwargs_test, optimizer, last, logged, attempts, renders, reports)
