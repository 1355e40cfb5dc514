"""The views of the gauss path on the host: per-view inverted indices, device-resident maps and images, the batch object the
kernels read, and the cache of the unperturbed images' logits. Everything here is the project's own; the mirror of
model/GaussNet.py (nerfail_amd/GaussNet.py) imports these names and keeps the kernels' wrappers and the modules.

The stores are plain module-level dicts / one set. Tests, tools and the benchmark hold on to them and `.clear()` them, so
they are never rebound and nothing derived (a running byte total, say) is kept beside them: a clear from outside is a
complete reset. One helper, _put(), is the only eviction; _touch() is the only refresh.

The rules of the view store, each pinned by tests/test_view_store.py (stubs, no GPU) or tests/test_hip_gauss.py:
 1. A view is keyed by _view_key(id, Ns) when the caller names it (`view_ids=`), else by a content fingerprint of its map
    plus Ns. _BATCH_KEYS remembers the fingerprints of a batch tensor OBJECT (weak reference, address and version), so a
    resident tensor passed again is not fingerprinted again; at 64 entries it is emptied.
 2. A caller-named id is only as good as the caller's naming. Checked on every use: image size and table size of a cached
    index (a mismatch raises instead of reading out of bounds). Checked ONCE per id: the index's stored fingerprint
    against the first device map seen under that id (ViewIndex.verified), and a passed device map against the resident
    one (_VIEW_PASSED_OK; register_view of a new map under the id asks for that check again).
 3. _VIEW_CACHE (ViewIndex per view) is bounded by VIEW_CACHE_BYTES over ViewIndex.nbytes(); every hit makes the entry the
    newest, the least recently USED entries leave first. register_view_index puts an index there without evicting.
 4. _VIEW_MAPS and _VIEW_ORI are bounded by VIEW_MAPS_BYTES each, over tensor bytes. A read NEVER refreshes an entry: they
    are evicted in REGISTRATION order (a re-registered id becomes the newest). Kept that way on purpose - an attack walks
    all views of a scene every epoch, so use order says nothing that registration order does not.
 5. _CSR_CACHE (whole-batch inverted indices, identity-keyed) holds CSR_CACHE_SIZE entries, refreshed on a hit.
 6. A value larger than its budget is still stored (alone); replacing a key does not count the old value.
 7. With `view_ids`, a resident map / image wins over the tensor passed under that id, which is then not touched at all.
 8. _set_resident_image() is the ONE writer of _VIEW_ORI: every write bumps _VIEW_ORI_EPOCH[key], which is part of the logit
    key (rule L3), so logits of an image that was replaced, or uploaded again after an eviction or a clear, are never reused.

The rules of OriLogitCache (one per gauss_net), pinned by tests/test_view_store.py:
 L1. The caller gets a clone and the cache stores a clone: writing into returned logits never changes a later hit.
 L2. A changed classifier-state key drops everything; at SIZE (64) entries everything is dropped before the next is stored.
 L3. ori_logit_key(): the SET of view ids with their image epochs ('ids' key; a subset or another order is another key),
     else the identity of the device tensor the caller passed, else the identity of the float images.
 L4. For a key that is not an 'ids' key the source tensor is held, so that its address cannot be recycled while the key can
     be looked up; at most SIZE such references are kept."""
import os
import weakref

import torch

from . import _lib
from .run_nerf_helpers import _cuda


def _put(store, key, value, budget, size):
    """store[key] = value as the newest entry; first the oldest entries leave until what stays and `value` fit `budget`
    (sizes by `size(v)`, summed over the dict on every call)."""
    store.pop(key, None)
    total = sum(size(v) for v in store.values()) + size(value)
    while store and total > budget:
        total -= size(store.pop(next(iter(store))))
    store[key] = value


def _touch(store, key):
    """store.get(key); a hit becomes the newest entry."""
    hit = store.pop(key, None)
    if hit is not None:
        store[key] = hit
    return hit


def _tensor_bytes(t):
    return t.numel() * t.element_size()


def _dense(t, dev):
    """`t` itself when the kernels can read it as it is (keeps its identity), else a contiguous float32 device copy."""
    return t if (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) else _lib.f32c(t, dev)


def _dev_image(o, dev):
    """An image (batch) on the device as the kernels read it: uint8 stays uint8, anything else becomes contiguous float32."""
    o = torch.as_tensor(o)
    return o.to(dev).contiguous() if o.dtype == torch.uint8 else _lib.f32c(o, dev)


def _tensor_key(t):
    return ('tensor', t.data_ptr(), t._version, tuple(t.shape), str(t.dtype))


class GaussCSR:
    """Inverted index of a batch of views' 8-NN maps (built once per batch tensor, reused by every backward):
    row_ptr [Ns+1] int32, contrib / w_sorted / row_of [B*P*8] (nerfail_gauss_csr_build: the entries sorted by
    destination row, zero-weight entries dropped behind row_ptr[Ns])."""

    def __init__(self, wi, Ns):
        lib = _lib.load()
        B, P = wi.shape[0], wi.shape[2] * wi.shape[3]
        nbytes = lib.nerfail_gauss_csr_workspace_bytes(Ns, B, P)
        if nbytes == 0:
            raise ValueError('batch too large for the 32-bit inverted index (B*P*8 < 2^31)')
        dev = wi.device
        self.Ns, self.B, self.P = Ns, B, P
        self.row_ptr = torch.empty((Ns + 1,), dtype=torch.int32, device=dev)
        self.contrib = torch.empty((B * P * 8,), dtype=torch.int32, device=dev)
        self.w_sorted = torch.empty((B * P * 8,), dtype=torch.float32, device=dev)
        self.row_of = torch.empty((B * P * 8,), dtype=torch.int32, device=dev)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        _lib.check(lib.nerfail_gauss_csr_build(_lib.dev(wi), Ns, B, P, _lib.dev(self.row_ptr), _lib.dev(self.contrib),
                                               _lib.dev(self.w_sorted), _lib.dev(self.row_of), _lib.dev(ws), nbytes,
                                               _lib.stream()))
        self._wi = wi          # keeps the map alive so its address cannot be recycled under the cache key


_CSR_CACHE = {}
CSR_CACHE_SIZE = 8


def csr_for(wi, Ns):
    """Inverted index of a whole BATCH tensor, identity-keyed (address, version): for callers that keep one resident batch
    tensor and reuse it (tests, the multi-RHS kernel checks). The attack loop goes through view_indices() instead."""
    key = (wi.data_ptr(), wi._version, tuple(wi.shape), int(Ns))
    hit = _touch(_CSR_CACHE, key)
    if hit is None:
        hit = GaussCSR(wi, Ns)
        _put(_CSR_CACHE, key, hit, CSR_CACHE_SIZE, lambda _: 1)
    return hit


# ---------------------------------------------------------------------------------------------- per-view inverted indices
class ViewIndex:
    """Inverted index of ONE view's 8-NN map ("per-view CSR"): for every row of the perturbation
    table the (pixel, weight) pairs that gather from it, sorted by row, zero-weight pairs dropped. A view's map never
    changes, so this is built once per view - whatever batch the view later appears in (the reference's DataLoader
    shuffles: batch compositions do not repeat) - and can be stored next to index_and_weight/<split>/<i>.pth.
    Arrays are trimmed to the entries that exist (background pixels contribute none: ~40 % of 8*H*W on a real view)."""

    ARRAYS = ('packed', 'w_sorted', 'chunk_ord', 'pos')

    def __init__(self, wi_view=None, Ns=None, state=None):
        self.verified = False          # set once the index has been checked against (or built from) a map seen in this process
        if state is not None:
            self.Ns, self.P = int(state['Ns']), int(state['P'])
            self.n_entries, self.n_rows = int(state['n_entries']), int(state['n_rows'])
            self.fp = tuple(state['fp']) if state.get('fp') is not None else None
            self.src = state.get('src')                  # (mtime_ns, size) of the map file the index was built from
            dev = _cuda()
            for k in self.ARRAYS:
                setattr(self, k, state[k].to(dev).contiguous())
            return
        lib = _lib.load()
        self.fp = fingerprints(wi_view.unsqueeze(0) if wi_view.dim() == 4 else wi_view)[0]      # content key of the map
        self.src = None
        self.verified = True
        full = GaussCSR(wi_view.unsqueeze(0) if wi_view.dim() == 4 else wi_view, Ns)     # sorted entries (B = 1), temporary
        dev = full.row_ptr.device
        cap = full.contrib.numel()
        # compact form (nerfail_gauss_view_pack): 8 bytes per entry (pixel * 2 + row-start flag, weight), one row ordinal
        # per 512 entries, and pos[Ns] (row -> ordinal in the view's compact row-sum array, -1 = no entry)
        self.pos = torch.empty((Ns,), dtype=torch.int32, device=dev)
        packed = torch.empty((cap,), dtype=torch.int32, device=dev)
        chunk_ord = torch.zeros((int(lib.nerfail_gauss_view_chunks(cap)),), dtype=torch.int32, device=dev)
        counts = torch.empty((1,), dtype=torch.int32, device=dev)
        nb = lib.nerfail_gauss_view_pack_workspace_bytes(Ns)
        ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
        _lib.check(lib.nerfail_gauss_view_pack(_lib.dev(full.row_ptr), _lib.dev(full.row_of), _lib.dev(full.contrib), Ns, cap,
                                               _lib.dev(self.pos), _lib.dev(packed), _lib.dev(chunk_ord), _lib.dev(counts),
                                               _lib.dev(ws), nb, _lib.stream()))
        n = int(full.row_ptr[-1])                      # host reads: once per view, at build time only
        self.n_entries, self.n_rows = n, int(counts[0])
        self.Ns, self.P = Ns, full.P
        # trimmed to the entries that exist (kept >= 1 long so that the pointers stay valid for an all-background view)
        self.packed, self.w_sorted = packed[:max(n, 1)].clone(), full.w_sorted[:max(n, 1)].clone()
        self.chunk_ord = chunk_ord[:max(int(lib.nerfail_gauss_view_chunks(n)), 1)].clone()

    def nbytes(self):
        return sum(_tensor_bytes(getattr(self, k)) for k in self.ARRAYS)

    def fill(self, st):
        """Writes this index into a nerfail_view_index struct (the tensors must stay alive while it is used)."""
        for k in self.ARRAYS:
            setattr(st, k, getattr(self, k).data_ptr())
        st.n_entries, st.n_rows = self.n_entries, self.n_rows

    def state_dict(self):
        d = {k: getattr(self, k).cpu() for k in self.ARRAYS}
        d.update(Ns=self.Ns, P=self.P, n_entries=self.n_entries, n_rows=self.n_rows, fp=self.fp, src=self.src)
        return d

    def save(self, path):
        torch.save(self.state_dict(), path)

    @staticmethod
    def load(path):
        return ViewIndex(state=torch.load(path, map_location='cpu'))


def view_table(indices):
    """Host table of nerfail_view_index structs for nerfail_gauss_bwd_views, and the floats of scratch that call needs."""
    table = (_lib.ViewIndexStruct * len(indices))()
    for b, vi in enumerate(indices):
        if vi.P != indices[0].P or vi.Ns != indices[0].Ns:
            raise ValueError('view indices of different image / table sizes in one batch: P %d vs %d, Ns %d vs %d'
                             % (vi.P, indices[0].P, vi.Ns, indices[0].Ns))
        vi.fill(table[b])
    return table, _lib.load().nerfail_gauss_bwd_views_scratch_floats(table, len(indices), indices[0].P, 1)


_VIEW_CACHE = {}                     # key -> ViewIndex, insertion order = LRU order
VIEW_CACHE_BYTES = 64 << 30          # 400 views of a scene are ~12 GB; HBM is 288 GB
_BATCH_KEYS = {}                     # (address, version, shape) of a resident batch tensor -> its views' keys


def fingerprints(wi):
    """Content keys of the views of a batch tensor [B,2,H,W,8] (one kernel + one 16*B-byte read back)."""
    B = wi.shape[0]
    out = torch.empty((B, 2), dtype=torch.int64, device=wi.device)
    _lib.check(_lib.load().nerfail_fingerprint(_lib.dev(wi), wi[0].numel(), B, _lib.dev(out), _lib.stream()))
    return [('fp',) + tuple(int(v) for v in row) + tuple(wi.shape[1:]) for row in out.cpu().tolist()]


def _view_key(v, Ns):
    return ('id', v if isinstance(v, (str, bytes, tuple)) else int(v), int(Ns))


def view_indices(wi, Ns, view_ids=None):
    """The ViewIndex of every view of the batch `wi` (a tensor [B,2,H,W,8] or a list of per-view tensors [2,H,W,8]), built
    on first sight and cached per VIEW (rules 1-3 of the module docstring).

    A caller-named id must be unique per (scene, split, resolution) - use tuples like (map_dir, i), as load_view_indices /
    load_view_maps do; a bare int reused for another split would name another view's index."""
    Ns = int(Ns)
    views = list(wi) if isinstance(wi, (list, tuple)) else [wi[b] for b in range(wi.shape[0])]
    if view_ids is not None:
        keys = [_view_key(v, Ns) for v in view_ids]
        if len(keys) != len(views):
            raise ValueError('view_ids must name every view of the batch')
    elif isinstance(wi, torch.Tensor):
        # identity shortcut: only for the very same tensor OBJECT (weak reference). An address alone proves nothing - the
        # allocator hands a freed batch tensor's memory to the next one, with other views in it.
        ident = (wi.data_ptr(), wi._version, tuple(wi.shape))
        hit = _BATCH_KEYS.get(ident)
        keys = hit[1] if hit is not None and hit[0]() is wi else None
        if keys is None:
            keys = [k + (Ns,) for k in fingerprints(wi)]
            if len(_BATCH_KEYS) >= 64:
                _BATCH_KEYS.clear()
            _BATCH_KEYS[ident] = (weakref.ref(wi), keys)
    else:
        keys = [fingerprints(v.unsqueeze(0))[0] + (Ns,) for v in views]
    out = []
    for key, wv in zip(keys, views):
        P = int(wv.shape[-3] * wv.shape[-2]) if wv is not None else None
        vi = _touch(_VIEW_CACHE, key)
        if vi is None:
            if wv is None:
                raise KeyError('view %r has neither a cached index nor a map to build one from' % (key,))
            vi = ViewIndex(wv, Ns)
            _put(_VIEW_CACHE, key, vi, VIEW_CACHE_BYTES, ViewIndex.nbytes)
        else:
            if vi.Ns != Ns or (P is not None and vi.P != P):
                raise ValueError('cached index of view %r was built for %d pixels / %d table rows, this call has %s / %d: the id '
                                 'names another view (ids must be unique per scene, split and resolution)' % (key, vi.P, vi.Ns, P, Ns))
            if key[0] == 'id' and not vi.verified and wv is not None and wv.is_cuda:
                fp = fingerprints(wv.unsqueeze(0))[0]        # once per id: one 0.1 ms kernel
                if vi.fp is not None and tuple(vi.fp) != tuple(fp):
                    raise ValueError('the index registered for view %r was built from a different map (fingerprint mismatch): '
                                     'stale sidecar or a reused id' % (key,))
                vi.fp, vi.verified = fp, True
        out.append(vi)
    return out


def _file_sig(path):
    st = os.stat(path)
    return (int(st.st_mtime_ns), int(st.st_size))


def load_view_indices(map_dir, ids, Ns, save_missing=True):
    """Per-view indices stored next to the maps they belong to: for every i in `ids` loads
    `<map_dir>/<i>.idx.pth` (ViewIndex.save) or, if it is not there yet - or was built from another version of the map
    (the sidecar records the map file's mtime and size, and the map's fingerprint) - builds it from `<map_dir>/<i>.pth`
    (the float32 [2,H,W,8] weight / index map dist_to_weight writes, DW:95-97) and stores it. The indices are registered
    in the cache; returns the view ids to hand to gauss_net.forward / nerfail_s_step (`view_ids=`), which then neither
    fingerprint nor rebuild anything, whatever batches the DataLoader composes."""
    out = []
    for i in ids:
        vid = (os.path.abspath(map_dir), int(i))
        side = os.path.join(map_dir, '%d.idx.pth' % int(i))
        mpath = os.path.join(map_dir, '%d.pth' % int(i))
        vi = None
        if os.path.exists(side):
            vi = ViewIndex.load(side)
            if vi.Ns != int(Ns):
                raise ValueError('%s was built for a table of %d rows, not %d' % (side, vi.Ns, int(Ns)))
            if os.path.exists(mpath) and (vi.src is None or tuple(vi.src) != _file_sig(mpath)):
                vi = None                   # the map was regenerated (another c, another NeRF, another resolution): rebuild
        if vi is None:
            wi = _lib.f32c(torch.load(mpath, map_location='cpu'), _cuda())
            vi = ViewIndex(wi, int(Ns))
            vi.src = _file_sig(mpath)
            if save_missing:
                vi.save(side)
        register_view_index(vid, vi, Ns, replace=True)
        out.append(vid)
    return out


def register_view_index(view_id, index, Ns=None, replace=False):
    """Put a ViewIndex loaded from disk (ViewIndex.load) into the cache under the caller's view id. An id that is already
    taken by an index of ANOTHER map (different fingerprint or size) is refused unless replace=True."""
    key = _view_key(view_id, Ns or index.Ns)
    old = _VIEW_CACHE.get(key)
    if old is not None and not replace and old is not index and (
            old.P != index.P or (old.fp is not None and index.fp is not None and tuple(old.fp) != tuple(index.fp))):
        raise ValueError('view id %r already names the index of another map; pass replace=True to overwrite it' % (view_id,))
    _VIEW_CACHE[key] = index


# ---------------------------------------------------------------------------------------------- device-resident views
# The reference's dataset hands the attack loop a freshly loaded map per view and step (MyDataset.py:199-204: torch.load of
# 41 MB + a cv2.imread per view; AS:304-317 passes them straight to the net): 8 x 51 MB over PCIe per iteration would be
# ~20x the 0.35 ms gauss path. A view's map and image never change, so they are kept on the device BY VIEW ID (288 GB of
# HBM hold a whole 400-view scene: 16 GB of maps + 1 GB of uint8 images): a forward that names its views finds them here
# and ignores the tensors it was handed.
_VIEW_MAPS = {}                      # key -> [2,H,W,8] float32 device tensor, insertion order = registration order
_VIEW_ORI = {}                       # key -> [H,W,4] uint8 (or float32) device tensor
_VIEW_ORI_EPOCH = {}                 # key -> how often the resident image of that id was written: part of the logit-cache key
_VIEW_PASSED_OK = set()              # keys whose resident map was compared once with a map the caller passed under that id
VIEW_MAPS_BYTES = 96 << 30


def _set_resident_image(key, img):
    """The one writer of _VIEW_ORI (rule 8): cached original-image logits of this id are stale now."""
    _put(_VIEW_ORI, key, img, VIEW_MAPS_BYTES, _tensor_bytes)
    _VIEW_ORI_EPOCH[key] = _VIEW_ORI_EPOCH.get(key, 0) + 1


def resident(view_id, Ns):
    """(map or None, image or None) kept on the device under `view_id`; a read, so nothing is refreshed (rule 4)."""
    key = _view_key(view_id, Ns)
    return _VIEW_MAPS.get(key), _VIEW_ORI.get(key)


def register_view(view_id, Ns, weight_and_index=None, ori_img=None):
    """Keep a view's [2,H,W,8] map and / or its image (uint8 BGRA as the dataset reads it, or float) on the device under
    `view_id`. Also builds (or verifies) the view's inverted index."""
    key = _view_key(view_id, Ns)
    dev = _cuda()
    if weight_and_index is not None:
        wi = _lib.f32c(torch.as_tensor(weight_and_index), dev)
        if wi.dim() != 4 or wi.shape[0] != 2 or wi.shape[3] != 8:
            raise ValueError('a view map must be [2,H,W,8] (DW:95-97)')
        view_indices([wi], Ns, [view_id])
        _put(_VIEW_MAPS, key, wi, VIEW_MAPS_BYTES, _tensor_bytes)
        _VIEW_PASSED_OK.discard(key)
    if ori_img is not None:
        _set_resident_image(key, _dev_image(ori_img, dev))
    return key


def load_view_maps(map_dir, ids, Ns, images=None):
    """Device-resident maps for the attack loop: `<map_dir>/<i>.pth` of every i in `ids` is loaded ONCE,
    kept on the device under the same ids load_view_indices uses, its inverted index loaded / built alongside. `images`:
    optional {i: uint8 [H,W,4] array} (the cv2.imread result of MyDataset.py:200) kept resident too. Returns the view ids
    for gauss_net.forward / nerfail_s_step (`view_ids=`)."""
    vids = load_view_indices(map_dir, ids, Ns)
    for i, vid in zip(ids, vids):
        if resident(vid, Ns)[0] is None:
            key = _view_key(vid, Ns)
            wi = _lib.f32c(torch.load(os.path.join(map_dir, '%d.pth' % int(i)), map_location='cpu'), _cuda())
            vi = _VIEW_CACHE[key]
            if vi.P != wi.shape[1] * wi.shape[2]:
                raise ValueError('%s/%d.pth does not match its index (pixels %d vs %d)' % (map_dir, int(i), wi.shape[1] * wi.shape[2], vi.P))
            _put(_VIEW_MAPS, key, wi, VIEW_MAPS_BYTES, _tensor_bytes)
        if images is not None and i in images:
            register_view(vid, Ns, ori_img=images[i])
    return vids


class BatchViews:
    """The views of one forward, one entry per view: device map [2,H,W,8], device image ([H,W,4] uint8 or float32), key.
    Built by resolve_views from what the caller passed and what is resident."""

    def __init__(self, wi, ori, ori_u8, view_ids, Ns, batch_wi=None, batch_ori=None):
        self.wi, self.ori, self.ori_u8, self.view_ids, self.Ns = wi, ori, ori_u8, view_ids, Ns
        self.batch_wi, self.batch_ori = batch_wi, batch_ori           # the contiguous batch tensors, when they came that way
        # identity of the image tensor the caller passed, when it lives on the device (logit cache key), and the tensor itself:
        # the address cannot be recycled while the key may be looked up
        self.ori_src = self.ori_keep = None
        self.B = len(wi)
        self.H, self.W = int(wi[0].shape[1]), int(wi[0].shape[2])
        self.P = self.H * self.W

    def table(self):
        t = (_lib.ViewFwdStruct * self.B)()
        for b in range(self.B):
            t[b].weight_and_index, t[b].ori_img = self.wi[b].data_ptr(), self.ori[b].data_ptr()
        return t

    def indices(self):
        return view_indices(self.batch_wi if (self.batch_wi is not None and self.view_ids is None) else self.wi, self.Ns, self.view_ids)

    def index_table(self):
        """(table of the views' inverted indices, the float scratch the backward kernels over it need)."""
        table, floats = view_table(self.indices())
        return table, torch.empty((floats,), dtype=torch.float32, device=self.wi[0].device)

    def ori_float(self):
        """[B,H,W,4] float32 (GN:55), materialised only when somebody needs it."""
        if self.batch_ori is not None and self.batch_ori.dtype == torch.float32:
            return self.batch_ori
        return torch.stack([o.float() for o in self.ori])

    def wi_batch(self):
        return self.batch_wi if self.batch_wi is not None else torch.stack(self.wi)


def _batch_views(wl, ol, view_ids, Ns, text, batch_wi=None, batch_ori=None):
    """The BatchViews of per-view maps and images after the checks both forms of resolve_views share: one image format, and
    every map [2,H,W,8] with an image [H,W,4] - the kernels index ori / x as [B*H*W] pixels and the table as float4[Ns],
    mismatched shapes would read out of bounds. `text`: the caller's error text over %(w)s and %(o)s."""
    if len({o.dtype for o in ol}) > 1:                       # mixed uint8 / float images: one format for the kernel
        ol, batch_ori = [o.float() for o in ol], None
    H, W = wl[0].shape[1], wl[0].shape[2]
    for w, o in zip(wl, ol):
        if tuple(w.shape) != (2, H, W, 8) or tuple(o.shape) != (H, W, 4):
            raise ValueError(text % {'w': tuple(w.shape), 'o': tuple(o.shape)})
    return BatchViews(wl, ol, ol[0].dtype == torch.uint8, view_ids, Ns, batch_wi, batch_ori)


def _resolve_list(wi_in, ori_in, view_ids, Ns, dev):
    """A batch handed over as per-view tensors (MyDataset.collate_views): nothing is stacked, ids travel with the list."""
    if view_ids is None and getattr(wi_in, 'view_ids', None) is not None:
        view_ids = wi_in.view_ids
    wl = [_dense(w, dev) for w in wi_in]
    ol = [_dev_image(o, dev) for o in ori_in]
    if len(wl) != len(ol) or (view_ids is not None and len(view_ids) != len(wl)):
        raise ValueError('maps, images and view ids of a batch must have the same length')
    return _batch_views(wl, ol, view_ids, Ns, 'a view must be a [2,H,W,8] map with a [H,W,4] image, got %(w)s and %(o)s')


def _resolve_tensor(wi_in, ori_in, view_ids, Ns, dev, keep_resident):
    """A batch tensor (or nothing) plus whatever is resident under `view_ids` (rule 7)."""
    B = len(view_ids) if view_ids is not None else wi_in.shape[0]
    keys = [_view_key(v, Ns) for v in view_ids] if view_ids is not None else [None] * B
    res_wi = [_VIEW_MAPS.get(k) if k is not None else None for k in keys]
    res_ori = [_VIEW_ORI.get(k) if k is not None else None for k in keys]
    batch_wi = batch_ori = None
    # ONCE per id the passed map - if it is a device tensor, i.e. free to look at - is compared with the resident one by
    # content fingerprint, so that an id reused for another scene / split or a regenerated map file raises instead of silently
    # differentiating through the wrong view.
    if view_ids is not None and isinstance(wi_in, torch.Tensor) and wi_in.is_cuda and wi_in.dim() == 5 and wi_in.shape[0] == B:
        todo = [b for b, k in enumerate(keys) if res_wi[b] is not None and k not in _VIEW_PASSED_OK]
        if todo and wi_in.dtype == torch.float32 and wi_in.is_contiguous():
            got = fingerprints(wi_in)
            for b in todo:
                if tuple(wi_in.shape[1:]) != tuple(res_wi[b].shape) or got[b] != fingerprints(res_wi[b].unsqueeze(0))[0]:
                    raise ValueError('view id %r is resident with a DIFFERENT map than the one passed under that id (reused id or '
                                     'regenerated map file): register_view(..., weight_and_index=) to replace it' % (view_ids[b],))
                _VIEW_PASSED_OK.add(keys[b])
    if any(w is None for w in res_wi):
        if wi_in is None:
            raise KeyError('a view of the batch is not resident and no weight_and_index_list was passed')
        if not isinstance(wi_in, torch.Tensor) or wi_in.dim() != 5 or wi_in.shape[1] != 2 or wi_in.shape[4] != 8:
            raise ValueError('weight_and_index_list must be [B,2,H,W,8] (DW:95-97)')
        if all(w is None for w in res_wi):
            batch_wi = _dense(wi_in, dev)        # (a tensor already resident keeps its identity -> inverted-index cache hit)
            res_wi = [batch_wi[b] for b in range(B)]
        else:
            res_wi = [w if w is not None else _lib.f32c(wi_in[b], dev) for b, w in enumerate(res_wi)]
        if keep_resident and view_ids is not None:
            for b, k in enumerate(keys):
                if k not in _VIEW_MAPS:
                    _put(_VIEW_MAPS, k, res_wi[b].clone() if batch_wi is not None else res_wi[b], VIEW_MAPS_BYTES, _tensor_bytes)
    if any(o is None for o in res_ori):
        o_in = torch.as_tensor(ori_in)
        if o_in.dim() != 4 or o_in.shape[0] != B or o_in.shape[-1] != 4:
            raise ValueError('ori_img must be [B,H,W,4] with the B of the batch, got %s' % (tuple(o_in.shape),))
        up = _dev_image(o_in, dev)                                                         # GN:55
        if all(o is None for o in res_ori) and up.dtype != torch.uint8:
            batch_ori = up
        res_ori = [o if o is not None else up[b] for b, o in enumerate(res_ori)]
        if keep_resident and view_ids is not None:
            for b, k in enumerate(keys):
                if k not in _VIEW_ORI:
                    _set_resident_image(k, res_ori[b].clone())
    bv = _batch_views(res_wi, res_ori, view_ids, Ns, 'ori_img must be [B,H,W,4] with the B, H, W of weight_and_index_list, got %(o)s vs %(w)s',
                      batch_wi, batch_ori)
    if isinstance(ori_in, torch.Tensor) and ori_in.is_cuda:
        bv.ori_src, bv.ori_keep = _tensor_key(ori_in), ori_in
    return bv


def resolve_views(spatial_rgb, weight_and_index_list, ori_img, view_ids=None, keep_resident=False):
    """What the kernels will read for this batch. With `view_ids`, a view whose map / image is resident (load_view_maps,
    register_view, or an earlier call with keep_resident) is taken from the device and the passed tensor is NOT touched -
    the reference-shaped loop hands over CPU tensors from a DataLoader every iteration."""
    dev = _cuda()
    Ns = int(spatial_rgb.numel() // 4)
    if isinstance(weight_and_index_list, (list, tuple)):
        return _resolve_list(weight_and_index_list, ori_img, view_ids, Ns, dev)
    return _resolve_tensor(weight_and_index_list, ori_img, view_ids, Ns, dev, keep_resident)


# ---------------------------------------------------------------------------------------------- original-image logits
def ori_logit_key(views, ori_float=None):
    """(key, tensor to hold or None) of the unperturbed images' logits of a BatchViews (rule L3). `ori_float`: the float images
    or a callable that yields them, looked at only when neither ids nor a passed device tensor key the batch; without it
    such a batch has no key: (None, None)."""
    if views.view_ids is not None:
        return ('ids', tuple((k, _VIEW_ORI_EPOCH.get(k, 0)) for k in (_view_key(v, views.Ns) for v in views.view_ids))), None
    if views.ori_src is not None:
        return views.ori_src, views.ori_keep
    if ori_float is None:
        return None, None
    o = ori_float() if callable(ori_float) else ori_float
    return _tensor_key(o), o


class OriLogitCache:
    """Logits of unperturbed images under ori_logit_key()'s keys, for one classifier (rules L1-L4 of the module docstring)."""
    SIZE = 64

    def __init__(self):
        self.logits, self.state_key, self.keep = {}, None, []

    def get(self, state_key, key):
        """A clone of the logits under `key`, or None; `state_key` other than the last one seen empties the cache first."""
        if state_key != self.state_key:              # a weight or buffer was written (or replaced): every stored logit is stale
            self.logits.clear()
            self.state_key = state_key
        hit = self.logits.get(key)
        return None if hit is None else hit.clone()  # the caller owns what it gets (the reference's callers write into logits in place, deepfool.py:54-57)

    def put(self, key, logits, keep=None):
        """Store a clone of `logits` (the tensor itself stays the caller's); `keep`: the tensor an address-based key names."""
        if len(self.logits) >= self.SIZE:
            self.logits.clear()
        self.logits[key] = logits.clone()
        if key[0] != 'ids':
            self.keep = self.keep[-(self.SIZE - 1):] + [keep]
