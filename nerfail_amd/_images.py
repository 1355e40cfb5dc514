"""One versioned cache for the device weight images of a module (NeRF: f32, f32_T, x3, x3f, f16, f16_T; MyCNN: packed, x3).

Plain Python: no library, no GPU, not an nn.Module (state_dict(), parameters() and .to() of the owner never see it). The
owner hands in `params`, a callable returning its parameters in one fixed order, and a table name -> (pack, source):
`pack()` returns the image, or `pack(source_image)` for an image made from another one; it may return None. The callables
must be bound methods of the owner (or not refer to it at all): copy.deepcopy re-binds bound methods to the copy and keeps
plain functions and closures by reference, which would pack the copy's images from the original's weights.

The rules, each pinned by tests/test_image_cache.py (stub packers) and tests/test_hip_image_cache.py (launch counts):
 1. An unchanged owner never packs twice: every lookup after the first returns the cached image.
 2. The key is (data_ptr, _version) over `params()`, computed once per lookup. An in-place write (p.add_(),
    load_state_dict, nerfail_amd.optim's step, which increments the versions itself) or a move (.to(device), p.data =
    new storage) changes it and drops EVERY image of the owner.
 3. An image made from another one is re-made exactly when its source was re-packed for a new key.
 4. get_joint() fills several images from one call of a joint packer; afterwards a lookup of any of them is a hit.
 5. Nothing is packed before it is asked for: which images a code path needs is the caller's business.
 6. A deep copy or a second instance never sees this owner's images: the copy's parameters have other pointers.
 7. None is a legal cached value (a shape the kernel does not cover): it is neither sized nor packed again.
 8. adopt(name, image) takes an image the owner itself brought up to date while it wrote the parameters (a fused optimizer
    step that updates weights and image in one launch, MyCNN.sgd_step): the key is re-read AFTER that write, `image` is
    cached under it, and every OTHER image of the owner is dropped as after any write. The next lookup of `name` is a hit;
    any further write drops it again (rule 2). The image's contents are the owner's promise (tests/test_hip_cls_flat.py
    holds MyCNN to it bitwise); rule pinned by tests/test_image_cache_adopt.py.
Known blind spot, kept as it is: a write through `.data` of an existing storage bumps no version and goes unseen."""


class ImageCache:
    def __init__(self, params, table):
        self._params, self._table = params, table
        self._key, self._images = None, {}

    def _now(self):
        return tuple((p.data_ptr(), p._version) for p in self._params())

    def _sync(self):
        key = self._now()
        if key != self._key:
            self._key, self._images = key, {}

    def _get(self, name):
        if name not in self._images:
            pack, source = self._table[name]
            self._images[name] = pack() if source is None else pack(self._get(source))
        return self._images[name]

    def get(self, name):
        """The current image `name`: cached, or packed now (its source first)."""
        self._sync()
        return self._get(name)

    def get_joint(self, names, pack):
        """The images `names` as a tuple; unless all are cached, ONE call of `pack()` makes all of them."""
        self._sync()
        if not all(n in self._images for n in names):
            self._images.update(zip(names, pack()))
        return tuple(self._images[n] for n in names)

    def adopt(self, name, image):
        """Cache `image` as the image `name` of the parameters as they are NOW; every other image is dropped."""
        if name not in self._table:
            raise KeyError(name)
        self._key, self._images = self._now(), {name: image}

    def holds(self, name, buffer):
        """True when `buffer` is the image `name` this cache packed last (whatever happened to the parameters since)."""
        mine = self._images.get(name)
        return mine is not None and buffer is not None and buffer.data_ptr() == mine.data_ptr()

    def is_current(self, name, buffer):
        """holds(), and no parameter was written or moved since that image was packed."""
        return self.holds(name, buffer) and self._key == self._now()
