"""The rules of nerfail_amd/views.py (its module docstring) that need neither the library nor a GPU: the one eviction helper over
plain dicts, OriLogitCache and ori_logit_key, on CPU tensors and stubs with an nbytes()."""
import torch

from nerfail_amd import views as V


class Stub:
    def __init__(self, n):
        self.n = n

    def nbytes(self):
        return self.n


def put(store, key, n, budget=10):
    V._put(store, key, Stub(n), budget, Stub.nbytes)


def test_put_under_budget_keeps_everything():
    s = {}
    for k, n in (('a', 3), ('b', 3), ('c', 4)):                  # 10 of 10: exactly at the budget is within it
        put(s, k, n)
    assert list(s) == ['a', 'b', 'c']


def test_put_over_budget_evicts_the_oldest_until_it_fits():
    s = {}
    for k, n in (('a', 3), ('b', 3), ('c', 3)):
        put(s, k, n)
    put(s, 'd', 2)                                               # 11 > 10: one entry leaves, not more
    assert list(s) == ['b', 'c', 'd']
    put(s, 'e', 6)                                               # 14 > 10: b and c leave (d + e = 8)
    assert list(s) == ['d', 'e']


def test_put_stores_a_value_larger_than_the_budget_alone():
    s = {}
    put(s, 'a', 3)
    put(s, 'big', 11)
    assert list(s) == ['big'] and s['big'].n == 11
    put(s, 'b', 1)                                               # ... and it leaves like any other entry
    assert list(s) == ['b']


def test_put_replacing_a_key_does_not_count_the_old_value():
    s = {}
    put(s, 'a', 4)
    put(s, 'b', 6)
    put(s, 'b', 5)                                               # 4 + 5 fits; counting the old 6 too would evict a
    assert list(s) == ['a', 'b'] and s['b'].n == 5
    put(s, 'a', 5)                                               # a replaced key becomes the newest entry
    assert list(s) == ['b', 'a']


def test_touch_makes_a_hit_the_newest_and_a_plain_read_changes_nothing():
    s = {}
    for k in 'abc':
        put(s, k, 3)
    assert s.get('a').n == 3 and list(s) == ['a', 'b', 'c']      # _VIEW_MAPS / _VIEW_ORI are read like this: registration order
    put(s, 'd', 3)
    assert list(s) == ['b', 'c', 'd']                            # ... so the first registered left, read or not
    assert V._touch(s, 'b').n == 3 and list(s) == ['c', 'd', 'b']     # _VIEW_CACHE / _CSR_CACHE are read like this
    put(s, 'e', 3)
    assert list(s) == ['d', 'b', 'e']
    assert V._touch(s, 'nope') is None and list(s) == ['d', 'b', 'e']


def test_put_after_an_outside_clear_sees_an_empty_store():
    s = {}
    for k in 'abc':
        put(s, k, 3)
    s.clear()                                                    # what tests, tools and the benchmark do to the module's dicts
    put(s, 'x', 9)
    put(s, 'y', 1)                                               # 10 of 10: nothing of a, b, c is counted any more
    assert list(s) == ['x', 'y']


def test_put_by_count_and_by_tensor_bytes():
    s = {}
    for k in range(10):
        V._put(s, k, object(), V.CSR_CACHE_SIZE, lambda _: 1)    # csr_for's use
    assert list(s) == list(range(10 - V.CSR_CACHE_SIZE, 10))
    t = {}
    for k in range(4):
        V._put(t, k, torch.zeros(4, dtype=torch.uint8 if k % 2 else torch.float32), 24, V._tensor_bytes)    # 16, 4, 16, 4 bytes
    assert list(t) == [1, 2, 3]


def test_the_stores_are_plain_containers_shared_with_GaussNet():
    from nerfail_amd import GaussNet as G
    for name in ('_CSR_CACHE', '_VIEW_CACHE', '_BATCH_KEYS', '_VIEW_MAPS', '_VIEW_ORI', '_VIEW_ORI_EPOCH'):
        assert type(getattr(V, name)) is dict and getattr(G, name) is getattr(V, name), name
    assert type(V._VIEW_PASSED_OK) is set and G._VIEW_PASSED_OK is V._VIEW_PASSED_OK


# ---------------------------------------------------------------------------------------------- OriLogitCache, ori_logit_key
def ids_key(*names):
    return ('ids', tuple((('id', n, 7), 0) for n in names))


def test_logits_returned_and_stored_are_distinct_storages():
    c = V.OriLogitCache()
    mine = torch.arange(6.).reshape(2, 3)
    want = mine.clone()
    c.put(ids_key('a'), mine)
    mine.add_(100.)                                              # the tensor that was put stays the caller's
    first = c.get(None, ids_key('a'))
    assert torch.equal(first, want)
    first.add_(1000.)                                            # ... and so does every tensor that comes back
    again = c.get(None, ids_key('a'))
    assert torch.equal(again, want) and again.data_ptr() != first.data_ptr()
    assert c.get(None, ids_key('b')) is None and c.get(None, ids_key('a', 'b')) is None      # a superset is another key


def test_a_new_classifier_state_key_empties_the_cache():
    c = V.OriLogitCache()
    assert c.get(((1, 0),), ids_key('a')) is None
    c.put(ids_key('a'), torch.ones(1, 3))
    c.put(ids_key('b'), torch.ones(1, 3))
    assert c.get(((1, 0),), ids_key('a')) is not None
    assert c.get(((1, 1),), ids_key('a')) is None and c.get(((1, 1),), ids_key('b')) is None and not c.logits
    c.put(ids_key('a'), torch.ones(1, 3))
    assert c.get(((1, 1),), ids_key('a')) is not None


def test_the_65th_distinct_key_empties_the_cache_first():
    c = V.OriLogitCache()
    for k in range(64):
        c.put(ids_key(k), torch.full((1, 2), float(k)))
    assert len(c.logits) == 64 and all(float(c.get(None, ids_key(k))[0, 0]) == k for k in range(64))
    c.put(ids_key(64), torch.zeros(1, 2))
    assert list(c.logits) == [ids_key(64)]


def test_only_address_keys_hold_their_source_and_never_more_than_64():
    c = V.OriLogitCache()
    c.put(ids_key('a'), torch.ones(1, 2), None)
    assert c.keep == []
    srcs = [torch.zeros(1) for _ in range(70)]
    for n, t in enumerate(srcs):
        c.put(V._tensor_key(t), torch.ones(1, 2), t)
        assert len(c.keep) == min(n + 1, 64)
    assert all(x is y for x, y in zip(c.keep, srcs[-64:]))       # the newest 64, whatever the logit dict dropped meanwhile


def test_logit_key_ids_with_epochs_then_the_passed_tensor_then_the_float_images():
    maps = [torch.zeros(2, 3, 4, 8)] * 2
    imgs = [torch.zeros(3, 4, 4, dtype=torch.uint8)] * 2
    named = V.BatchViews(maps, imgs, True, ['u', 'v'], 7)
    ku, kv = V._view_key('u', 7), V._view_key('v', 7)
    V._VIEW_ORI_EPOCH.pop(ku, None), V._VIEW_ORI_EPOCH.pop(kv, None)
    assert V.ori_logit_key(named) == (('ids', ((ku, 0), (kv, 0))), None)
    V._VIEW_ORI_EPOCH[kv] = 3                                    # the image of v was written three times (rule 8)
    try:
        assert V.ori_logit_key(named) == (('ids', ((ku, 0), (kv, 3))), None)
        named.ori_src = ('tensor', 1)                            # ids win over everything else
        assert V.ori_logit_key(named)[0][0] == 'ids'
    finally:
        del V._VIEW_ORI_EPOCH[kv]
    assert V.ori_logit_key(V.BatchViews(maps[:1], imgs[:1], True, ['u'], 7))[0] != V.ori_logit_key(named)[0]      # a subset: another key
    # no ids: the identity of the (device) tensor the caller passed, as resolve_views records it
    anon = V.BatchViews(maps, imgs, True, None, 7)
    passed = torch.zeros(2, 3, 4, 4, dtype=torch.uint8)
    anon.ori_src, anon.ori_keep = V._tensor_key(passed), passed
    key, keep = V.ori_logit_key(anon, lambda: 1 / 0)             # the float images are not asked for
    assert key == ('tensor', passed.data_ptr(), passed._version, (2, 3, 4, 4), 'torch.uint8') and keep is passed
    passed.add_(1)                                               # written in place: another version, another key
    assert V._tensor_key(passed) != key
    # neither: the float images' identity when they are at hand (tensor or callable), else no key
    bare = V.BatchViews(maps, imgs, True, None, 7)
    assert V.ori_logit_key(bare) == (None, None)
    f = torch.zeros(2, 3, 4, 4)
    for arg in (f, lambda: f):
        key, keep = V.ori_logit_key(bare, arg)
        assert key == V._tensor_key(f) and keep is f and key[0] != 'ids'
