"""The rules of nerfail_amd/_images.py (its module docstring, by number) on CPU tensors with stub packers that count their
calls and return fresh tensors: no GPU, no library."""
import collections
import copy

import torch
from torch import nn

from nerfail_amd._images import ImageCache


class Owner(nn.Module):
    """Two parameters, a plain image, one made from it, one that does not exist (None) and a joint pair."""

    def __init__(self):
        super().__init__()
        self.a, self.b = nn.Linear(3, 2), nn.Linear(2, 1)
        self.calls = collections.Counter()
        self.images = ImageCache(self._params, {'f32': (self._pack_f32, None), 'f32_T': (self._pack_T, None),
                                                'x3': (self._pack_x3, 'f32'), 'none': (self._pack_none, 'f32')})

    def _params(self):
        return [self.a.weight, self.a.bias, self.b.weight, self.b.bias]

    def _pack_f32(self):
        self.calls['f32'] += 1
        return torch.cat([p.detach().reshape(-1) for p in self._params()])

    def _pack_T(self):
        self.calls['f32_T'] += 1
        return self.a.weight.detach().t().clone()

    def _pack_x3(self, f32):
        self.calls['x3'] += 1
        return f32 * 3

    def _pack_none(self, f32):
        self.calls['none'] += 1                                 # (the size query of an uncovered shape)
        return None

    def _pack_both(self):
        self.calls['both'] += 1
        return torch.cat([p.detach().reshape(-1) for p in self._params()]), self.a.weight.detach().t().clone()

    def both(self):
        return self.images.get_joint(('f32', 'f32_T'), self._pack_both)


def test_rule_1_an_unchanged_owner_never_packs_twice():
    o = Owner()
    first = o.images.get('f32')
    assert all(o.images.get('f32') is first for _ in range(3))
    x3 = o.images.get('x3')
    assert o.images.get('x3') is x3 and o.images.get('f32') is first
    assert o.calls == {'f32': 1, 'x3': 1}


def test_rule_2_writes_and_moves_invalidate_every_image():
    o = Owner()

    def all_three():
        return o.images.get('f32'), o.images.get('f32_T'), o.images.get('x3')
    before = all_three()
    writes = [lambda: o.b.bias.add_(1.),
              lambda: o.load_state_dict({k: v + 1 for k, v in o.state_dict().items()}),
              lambda: setattr(o.a.weight, 'data', o.a.weight.data.clone())]       # same values, new storage
    for n, write in enumerate(writes, start=2):
        with torch.no_grad():
            write()
        after = all_three()
        assert all(x is not y for x, y in zip(before, after))
        assert o.calls == {'f32': n, 'f32_T': n, 'x3': n}
        assert all(x is y for x, y in zip(after, all_three()))                    # ... and cached again
        before = after
    assert torch.equal(before[0], torch.cat([p.detach().reshape(-1) for p in o._params()]))


def test_rule_3_a_derived_image_follows_its_source():
    o = Owner()
    x3 = o.images.get('x3')                                     # packs its source first
    assert o.calls == {'f32': 1, 'x3': 1} and torch.equal(x3, o.images.get('f32') * 3)
    o.images.get('f32_T')                                       # another image of the same version: nothing re-made
    assert o.images.get('x3') is x3 and o.calls == {'f32': 1, 'x3': 1, 'f32_T': 1}
    with torch.no_grad():
        o.a.bias.add_(1.)
    f32 = o.images.get('f32')                                   # the source alone is re-packed ...
    assert o.calls == {'f32': 2, 'x3': 1, 'f32_T': 1}
    x3 = o.images.get('x3')                                     # ... and the derived image is re-made from THAT buffer, once
    assert o.calls == {'f32': 2, 'x3': 2, 'f32_T': 1} and torch.equal(x3, f32 * 3)
    assert o.images.get('x3') is x3 and o.calls['x3'] == 2


def test_rule_4_one_joint_pack_fills_both_images():
    o = Owner()
    f32, f32_T = o.both()
    assert o.images.get('f32') is f32 and o.images.get('f32_T') is f32_T
    again = o.both()
    assert again[0] is f32 and again[1] is f32_T
    assert o.calls == {'both': 1}
    with torch.no_grad():
        o.a.weight.add_(1.)
    assert o.both()[0] is not f32 and o.calls == {'both': 2}
    with torch.no_grad():
        o.a.weight.add_(1.)
    single = o.images.get('f32')                                # one image cached, the other not: the joint packer makes both
    assert o.both()[0] is not single and o.calls == {'both': 3, 'f32': 1}
    assert o.images.get('f32_T') is o.both()[1] and o.calls == {'both': 3, 'f32': 1}


def test_rule_6_copies_and_other_instances_have_their_own_images():
    o, other = Owner(), Owner()
    f32 = o.images.get('f32')
    assert other.images.get('f32') is not f32 and other.calls == {'f32': 1}
    twin = copy.deepcopy(o)
    with torch.no_grad():
        twin.a.weight.add_(1.)
    t32 = twin.images.get('f32')                                # packed by the copy, from the copy's weights
    assert twin.calls['f32'] == 2 and o.calls == {'f32': 1}
    assert torch.equal(t32[:6], twin.a.weight.detach().reshape(-1)) and not torch.equal(t32, f32)
    assert o.images.get('f32') is f32 and twin.images.get('f32') is t32
    assert not o.images.holds('f32', t32) and not twin.images.holds('f32', f32)
    fresh = copy.deepcopy(o)                                    # an unwritten copy still re-packs: other pointers
    assert fresh.images.get('f32') is not f32 and fresh.calls['f32'] == 2 and o.calls == {'f32': 1}


def test_rule_7_none_is_cached():
    o = Owner()
    assert all(o.images.get('none') is None for _ in range(4))
    assert o.calls == {'f32': 1, 'none': 1}
    with torch.no_grad():
        o.a.bias.add_(1.)
    assert o.images.get('none') is None and o.images.get('none') is None
    assert o.calls == {'f32': 2, 'none': 2}
    assert not o.images.is_current('none', None)                # no buffer, nothing to be current


def test_is_current_three_outcomes():
    o, other = Owner(), Owner()
    f32 = o.images.get('f32')
    assert o.images.is_current('f32', f32)                                           # current
    foreign = other.images.get('f32')
    assert not o.images.is_current('f32', foreign) and not o.images.holds('f32', foreign)          # another buffer
    assert not o.images.is_current('f32_T', f32)                                     # (never packed)
    with torch.no_grad():
        o.b.weight.add_(1.)
    assert not o.images.is_current('f32', f32) and o.images.holds('f32', f32)        # parameters written since
    new = o.images.get('f32')
    assert o.images.is_current('f32', new) and not o.images.holds('f32', f32)        # repacked: the old one is another buffer
    o.a.weight.data = o.a.weight.data.clone()
    assert not o.images.is_current('f32', new) and o.images.holds('f32', new)        # parameters moved since
