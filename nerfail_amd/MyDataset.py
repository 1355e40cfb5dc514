"""Mirror of the attack datasets of MyDataset.py (reference = MD): `gauss_dataset` (MD:187-204) and
`gauss_dataset_rand_select` (MD:207-232, seed 1003) - same constructor arguments, same 5-tuple per item
(index, ori_img uint8 BGRA [H,W,4], img_index_and_dist float32 [2,H,W,8], save name, mask save name) - and of the 2-D
baselines' `universal_2D_dataset` / `universal_2D_dataset_rand_select` (MD:235-294).

What differs is WHERE the tensors come from. The reference reads the PNG and `torch.load`s the 41 MB map from disk for
every item of every iteration (MD:199-204) and the DataLoader stacks eight of them into a fresh batch tensor. A view's map
and image never change, so here an item is loaded ONCE and then lives on the device under its view id (views.
register_view; 288 GB of HBM hold a whole scene); later __getitem__ calls return those resident tensors, and
`collate_views` hands the batch to gauss_net.forward / nerfail_s_step as a list of per-view tensors plus their ids instead of
stacking 328 MB per iteration. With the default collate function the batch is a stacked DEVICE tensor, as in the reference.
Host-side file I/O only; PNG decoding through cv2 when present (as the reference), else PIL."""
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from . import views as _views
from .run_nerf_helpers import _cuda


def _imread_unchanged(path):
    """cv2.imread(path, cv2.IMREAD_UNCHANGED): uint8 [H,W,4] in BGRA order."""
    try:
        import cv2
        return cv2.imread(path, cv2.IMREAD_UNCHANGED)
    except ImportError:
        from PIL import Image
        a = np.asarray(Image.open(path).convert('RGBA'))
        return np.ascontiguousarray(a[..., [2, 1, 0, 3]])


def _file_sig(path):
    try:
        st = os.stat(path)
        return (int(st.st_mtime_ns), int(st.st_size))
    except OSError:
        return (0, 0)


class ViewList(list):
    """A batch as per-view tensors (no stacking) + the ids under which the views are resident."""

    def __init__(self, items, view_ids):
        super().__init__(items)
        self.view_ids = list(view_ids)

    @property
    def shape(self):
        return (len(self),) + tuple(self[0].shape)


class gauss_dataset(Dataset):
    """MD:187-204. `Ns` (rows of the perturbation table, P*H*W) switches residency on: items are then kept on the device by
    view id (see view_id), together with their inverted index."""

    def __init__(self, all_index_and_dist_name_list, all_img_name_list, all_img_save_to_name_list, all_img_mask_save_to_name_list,
                 device, Ns=None):
        self.length = len(all_img_name_list)
        self.all_index_and_dist_name_list = all_index_and_dist_name_list
        self.all_img_name_list = all_img_name_list
        self.all_img_save_to_name_list = all_img_save_to_name_list
        self.all_img_mask_save_to_name_list = all_img_mask_save_to_name_list
        self.device = device
        self.Ns = Ns
        self._vids = {}

    def __len__(self):
        return self.length

    def view_id(self, index):
        """(map path, its mtime_ns and size, the image's mtime_ns and size): a regenerated map or image file is ANOTHER view
        as far as the device-resident copies and cached logits are concerned (load_view_indices records the same
        signature in its sidecars)."""
        vid = self._vids.get(index)
        if vid is None:                    # taken when the dataset first touches the view (two stat calls), then fixed for its life
            m, i = self.all_index_and_dist_name_list[index], self.all_img_name_list[index]
            vid = self._vids[index] = (os.path.abspath(m),) + _file_sig(m) + _file_sig(i)
        return vid

    def __getitem__(self, index):
        dev = _cuda()
        wi, ori = _views.resident(self.view_id(index), self.Ns) if self.Ns is not None else (None, None)
        missing = wi is None or ori is None
        if ori is None:
            ori = torch.tensor(_imread_unchanged(self.all_img_name_list[index])).to(dev)
        if wi is None:
            wi = torch.load(self.all_index_and_dist_name_list[index], map_location=dev)
        if self.Ns is not None and missing:
            _views.register_view(self.view_id(index), self.Ns, weight_and_index=wi, ori_img=ori)
            wi, ori = _views.resident(self.view_id(index), self.Ns)
        return index, ori, wi, self.all_img_save_to_name_list[index], self.all_img_mask_save_to_name_list[index]

    def collate_views(self, batch):
        """collate_fn for the DataLoader: (indices, ori_img ViewList, img_index_and_dist ViewList, save names, mask names) -
        nothing is stacked; the ViewLists carry the view ids gauss_net.forward / nerfail_s_step look the views up by."""
        idx = [b[0] for b in batch]
        ids = [self.view_id(i) for i in idx] if self.Ns is not None else None
        return (torch.tensor(idx), ViewList([b[1] for b in batch], ids or idx), ViewList([b[2] for b in batch], ids or idx),
                [b[3] for b in batch], [b[4] for b in batch])


class gauss_dataset_rand_select(gauss_dataset):
    """MD:207-232: a fixed random subset (seed 1003) of the views."""

    def __init__(self, all_index_and_dist_name_list, all_img_name_list, all_img_save_to_name_list, all_img_mask_save_to_name_list,
                 device, select_rate=0.2, Ns=None):
        random.seed(1003)
        ori_length = len(all_img_name_list)
        n = int(ori_length * select_rate)
        sel = random.sample(range(ori_length), n)
        super().__init__([all_index_and_dist_name_list[i] for i in sel], [all_img_name_list[i] for i in sel],
                         [all_img_save_to_name_list[i] for i in sel], [all_img_mask_save_to_name_list[i] for i in sel], device, Ns)


class universal_2D_dataset(Dataset):
    """MD:235-259: the views of the 2-D baselines (attack_IGSM_2D.py, attack_Universal_2D.py) - same constructor arguments, same
    item tuple (index, ori_img_3channel uint8 [H,W,3] on the white background of MD:247-255, save name, mask save name). The
    item is stock torch on `device`; `store()` stacks the files as read (uint8 [N,H,W,4|3]) for attack.igsm_2d, which makes the
    white background itself (nerfail_u2d_fwd)."""

    def __init__(self, all_img_name_list, all_img_save_to_name_list, all_img_mask_save_to_name_list, device):
        self.length = len(all_img_name_list)
        self.all_img_name_list = all_img_name_list
        self.all_img_save_to_name_list = all_img_save_to_name_list
        self.all_img_mask_save_to_name_list = all_img_mask_save_to_name_list
        self.device = device

    def __len__(self):
        return self.length

    def __getitem__(self, index):
        ori_img = torch.tensor(_imread_unchanged(self.all_img_name_list[index])).to(self.device)
        alpha = ori_img[:, :, 3].unsqueeze(-1).broadcast_to([ori_img.size()[0], ori_img.size()[1], 3])     # MD:250-255
        rgb = ori_img[:, :, :3]
        ori_img_3channel = torch.where(alpha > 0, rgb, torch.ones_like(rgb) * 255)
        return index, ori_img_3channel, self.all_img_save_to_name_list[index], self.all_img_mask_save_to_name_list[index]

    def store(self, device=None):
        """Every file as read, stacked: uint8 [N,H,W,4] (BGRA) or [N,H,W,3], on `device` (default: the dataset's)."""
        imgs = [np.ascontiguousarray(_imread_unchanged(n)) for n in self.all_img_name_list]
        if len({i.shape for i in imgs}) > 1:
            raise ValueError('universal_2D_dataset: the files differ in size or channel count')
        return torch.from_numpy(np.stack(imgs)).to(self.device if device is None else device)


class universal_2D_dataset_rand_select(universal_2D_dataset):
    """MD:262-294: a fixed random subset (seed 1003, random.sample) of the views."""

    def __init__(self, all_img_name_list, all_img_save_to_name_list, all_img_mask_save_to_name_list, device, select_rate=0.2):
        random.seed(1003)
        ori_length = len(all_img_name_list)
        sel = random.sample(range(ori_length), int(ori_length * select_rate))
        super().__init__([all_img_name_list[i] for i in sel], [all_img_save_to_name_list[i] for i in sel],
                         [all_img_mask_save_to_name_list[i] for i in sel], device)


def find_classes(directory):
    """MD:15-25: the class folders of a dataset, sorted, and their indices."""
    classes = sorted(entry.name for entry in os.scandir(directory) if entry.is_dir())
    if not classes:
        raise FileNotFoundError(f"Couldn't find any class folder in {directory}.")
    return classes, {cls_name: i for i, cls_name in enumerate(classes)}


class MySimpleDataset(Dataset):
    """MD:28-185 for the branch model_train.py uses (_3_channels=True, no ori_img_from, load_later=False): the classification
    set `root/<class>/<set_name>/*.png` - same constructor, same class table, file filter (MD:81-87) and index rule
    (start_idx + img_index), and per item the reference's float [3,H,W] white-background tensor and the label.

    What differs is where the views live. The reference keeps one float tensor per view (7.7 MB at 800 x 800) and the
    DataLoader stacks 16 of them per batch; here the set is resident as ONE uint8 store [N,H,W,ch] plus an int32 label vector
    on the device (`store`, `labels`, row k = index `indices[k]`), and a batch is gathered from it by device indices
    (torch.ops.nerfail_mi.cls_batch, which also makes the white background of MD:98-105) - what
    nerfail_amd.model_train.train_classifier does. Files of mixed channel counts or sizes raise; the reference's other branches
    raise NotImplementedError."""

    def __init__(self, root, set_name, class_names_path=None, test_dir_change_dict=None, ori_img_from=None, _3_channels=False,
                 resize_frame=False, resize_frame_size=None, device='cpu', load_later=False, return_img_before_resize=False):
        if ori_img_from is not None:
            raise NotImplementedError('MySimpleDataset: ori_img_from (MD:73-75, 118-142) is not ported')
        if load_later:
            raise NotImplementedError('MySimpleDataset: load_later=True (MD:90-91, 149-171) is not ported')
        if not _3_channels:
            raise NotImplementedError('MySimpleDataset: _3_channels=False (four-channel items, MD:98) is not ported')
        if return_img_before_resize:
            raise NotImplementedError('MySimpleDataset: return_img_before_resize=True (MD:107-108, 173-174) is not ported')
        if resize_frame and resize_frame_size is not None:
            raise NotImplementedError('MySimpleDataset: a resize at load time (MD:110-111) is not ported; train_classifier '
                                      'resizes the batches of the models that need it')
        self.classes, self.class_to_idx = find_classes(root)
        if class_names_path is not None:
            with open(class_names_path, 'w') as f:
                for i_classes in self.classes:
                    f.write(str(self.class_to_idx[i_classes]) + " -- " + i_classes + "\n")
        self.root, self.set_name, self.device = root, set_name, device
        self.test_dir_change_dict = test_dir_change_dict
        self.now_index = 0
        images, self.label_set = {}, {}
        for class_name in self.classes:
            self._read_one_class(class_name, set_name, images)
        self.length = len(images)
        self.indices = sorted(images)
        self._row = {idx: k for k, idx in enumerate(self.indices)}
        shapes = {images[i].shape for i in self.indices}
        if len(shapes) > 1:
            raise ValueError('MySimpleDataset: the files of %s/*/%s differ in size or channel count: %s'
                             % (root, set_name, sorted(shapes)))
        dev = torch.device(device)
        if self.length:
            self.store = torch.from_numpy(np.stack([images[i] for i in self.indices])).to(dev)
        else:
            self.store = torch.zeros((0, 0, 0, 3), dtype=torch.uint8, device=dev)
        self.labels = torch.tensor([self.label_set[i] for i in self.indices], dtype=torch.int32).to(dev)

    def _read_one_class(self, class_name, set_name, images):
        class_path = os.path.join(self.root, class_name, set_name)
        class_idx = self.class_to_idx[class_name]
        if self.test_dir_change_dict is not None and class_idx in self.test_dir_change_dict.keys():
            class_path = self.test_dir_change_dict[class_idx]
        start_idx = self.now_index
        for img_file in os.listdir(class_path):
            parts = img_file.split("_")
            if (len(parts) < 3) and ("ori" not in img_file):                                     # MD:82
                stem = parts[1] if len(parts) == 2 else parts[0]
                img_index = int(stem.replace(".png", "").replace(".jpg", "").replace(".jpeg", ""))
                img_idx = start_idx + img_index
                img = _imread_unchanged(os.path.join(class_path, img_file))
                if img is None or img.ndim != 3 or img.shape[2] not in (3, 4) or img.dtype != np.uint8:
                    raise ValueError('MySimpleDataset: %s is not an 8-bit image of 3 or 4 channels' % os.path.join(class_path, img_file))
                images[img_idx] = np.ascontiguousarray(img)
                self.label_set[img_idx] = class_idx
                self.now_index += 1

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        from . import ops
        k = self._row[idx]
        x, _ = ops.cls_batch(self.store, self.labels, torch.tensor([k], dtype=torch.int64, device=self.store.device))
        return x[0], self.label_set[idx]
