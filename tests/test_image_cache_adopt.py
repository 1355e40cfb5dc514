"""Rule 8 of nerfail_amd/_images.py: ImageCache.adopt() - an image the owner brought up to date itself, in the launch that wrote
the parameters (MyCNN.sgd_step). Stub packers on CPU tensors, as tests/test_image_cache.py; the launch counts on the real module
are in tests/test_hip_cls_flat.py."""
import pytest
import torch

from nerfail_amd._images import ImageCache


class Owner:
    def __init__(self):
        self.w = torch.zeros(4)
        self.packs = {'a': 0, 'b': 0}
        self.cache = ImageCache(lambda: [self.w], {'a': (self._pack_a, None), 'b': (self._pack_b, 'a')})

    def _pack_a(self):
        self.packs['a'] += 1
        return self.w.clone()

    def _pack_b(self, a):
        self.packs['b'] += 1
        return a * 2


def test_adopt_makes_the_next_lookup_a_hit_and_drops_the_other_images():
    o = Owner()
    a, b = o.cache.get('a'), o.cache.get('b')
    assert o.packs == {'a': 1, 'b': 1}
    o.w.add_(1.0)                                  # the fused step: parameters written ...
    a.add_(1.0)                                    # ... and the image brought up to date by the same launch
    o.cache.adopt('a', a)
    assert o.cache.get('a') is a and o.packs == {'a': 1, 'b': 1}         # a hit: nothing packed
    assert o.cache.is_current('a', a)
    assert torch.equal(o.cache.get('b'), a * 2) and o.cache.get('b') is not b and o.packs == {'a': 1, 'b': 2}    # b was dropped
    assert o.cache.get('a') is a and o.packs['a'] == 1


def test_a_write_after_adopt_drops_the_adopted_image():
    o = Owner()
    a = o.cache.get('a')
    o.w.add_(1.0)
    o.cache.adopt('a', a)
    o.w.add_(1.0)                                  # any further write: rule 2
    assert not o.cache.is_current('a', a) and o.cache.holds('a', a)
    assert o.cache.get('a') is not a and o.packs['a'] == 2


def test_adopt_without_a_write_and_unknown_names():
    o = Owner()
    img = torch.ones(4)
    o.cache.adopt('a', img)                        # nothing was packed before: the adopted image is the first
    assert o.cache.get('a') is img and o.packs['a'] == 0
    with pytest.raises(KeyError):
        o.cache.adopt('c', img)
