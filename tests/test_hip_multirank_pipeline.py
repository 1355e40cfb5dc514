"""-m gpu: one process group from the trained NeRF to the evaluation of the retrained one - scene.build_scene_maps(shard_batch=),
attack.nerfail_s over the sharded maps, PoisonedTrainSet.gather, retrain.render_splits(sharded=True) and retrain.poisoned_retrain
on 1, 2 and 3 gloo ranks that share the box's one GPU (tests/mgpu/pipeline_rank.py, started through the clean launcher). The
claim is correctness, not scaling: everything is compared with == on bits against the one-rank run of the same script, which in
turn equals the calls without the new keywords.

The scene is tests/test_hip_scene.py's (40 x 40 views: 1 600 pixels are ragged over 3 ranks; test 4 / train 2 / val 1 views; 4 800
points: the grid kernel) with shard_batch = 4, so with 3 ranks the test split is owned 2 / 1 / 1, rank 2 owns no train view and
ranks 1 and 2 no val view: the uneven-shard and the idle-rank branches both run. These are the smallest shapes that still reach
the grid search, a ragged shard and an idle rank."""
import json
import os

import numpy as np
import pytest

from conftest import ROOT
from nerfail_amd import sharding

pytestmark = pytest.mark.gpu
SCRIPT = os.path.join(ROOT, 'tests', 'mgpu', 'pipeline_rank.py')
COUNTS = {'test': 4, 'train': 2, 'val': 1}
SIDE, B = 40, 4
VIEWS = [(s, i) for s in ('test', 'train', 'val') for i in range(COUNTS[s])]
MANY = [(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]                    # (world, rank) of the multi-rank runs


class Run:
    def __init__(self, out, world, rank):
        self.a = dict(np.load(os.path.join(out, 'pipe_w%d_r%d.npz' % (world, rank))))
        with open(os.path.join(out, 'pipe_w%d_r%d.json' % (world, rank))) as f:
            self.m = json.load(f)


@pytest.fixture(scope='module')
def runs(rank_launcher, tmp_path_factory):
    out = str(tmp_path_factory.mktemp('pipeline'))
    for world in (1, 2, 3):
        rep = rank_launcher(SCRIPT, world, [out], timeout=420)
        assert rep['rc'] == [0] * world, '\n'.join(rep['logs'])
    return {(w, r): Run(out, w, r) for w in (1, 2, 3) for r in range(w)}


def _owned(world, rank):
    return {s: sharding.owned_positions(n, B, rank, world) for s, n in COUNTS.items()}


def _same_view(x, tag_x, y, tag_y, s, i):
    keys = ['%s%d_map' % (s, i), '%s%d_idx_meta' % (s, i)] + ['%s%d_idx_%s' % (s, i, k) for k in ('packed', 'w_sorted', 'chunk_ord', 'pos')]
    for k in keys:
        assert np.array_equal(x.a[tag_x + '_' + k], y.a[tag_y + '_' + k]), (tag_x, tag_y, k)
    assert x.a['%s_%s%d_map' % (tag_x, s, i)].shape == (2, SIDE, SIDE, 8)


def test_the_shards_are_the_ones_the_issue_names():
    assert [_owned(3, r)['test'] for r in range(3)] == [[0, 1], [2], [3]]                  # 2 / 1 / 1
    assert [_owned(3, r)['train'] for r in range(3)] == [[0], [1], []]                     # rank 2 owns no train view
    assert [_owned(3, r)['val'] for r in range(3)] == [[0], [], []]                        # ranks 1 and 2 own no val view
    assert sharding.shard_ranges(SIDE * SIDE, 3) == [(0, 534), (534, 1067), (1067, 1600)]   # ragged pixel ranges


def test_point_set_on_every_rank_is_the_one_rank_point_set(runs):
    """1."""
    one = runs[1, 0]
    assert one.m['full']['Ns'] == 3 * SIDE * SIDE and one.m['full']['grid'] is True
    for wr in MANY:
        for tag in ('full', 'fg'):
            assert np.array_equal(runs[wr].a[tag + '_points'], one.a[tag + '_points']), (wr, tag)
            assert runs[wr].m[tag]['Ns'] == one.m['full']['Ns'] and runs[wr].m[tag]['grid'] is True
    assert np.array_equal(one.a['fg_points'], one.a['full_points'])


@pytest.mark.parametrize('tag', ['full', 'fg'])
def test_owned_views_are_the_one_rank_views(runs, tag):
    """2: every owned view's map and inverted index, bit for bit; nothing else is registered; rendered and v on every rank."""
    one = runs[1, 0]
    for w, r in MANY:
        x, own = runs[w, r], _owned(w, r)
        assert x.m[tag]['owned'] == own and x.m[tag]['shard_batch'] == B and x.m[tag]['maps_world'] == w
        mine = [[s, i] for s, i in VIEWS if i in own[s]]
        assert x.m[tag]['registered'] == mine, (w, r)                                          # a view not owned is not registered
        assert [v[:2] for v in x.m[tag]['seen']] == mine                                       # on_view: own views only
        for s, i in mine:
            _same_view(x, tag, one, tag, s, i)
        assert x.m[tag]['rendered'] == one.m[tag]['rendered']                                  # the counts of ALL views
        assert x.m[tag]['v'] == one.m[tag]['v'], (w, r, float.fromhex(x.m[tag]['v']), float.fromhex(one.m[tag]['v']))
        assert x.m[tag]['batches_test'] == [4]
        if tag == 'full':                                                                      # save_dir: every rank wrote its own views' files
            assert x.m[tag]['own_files'] == {'%s%d' % (s, i): True for s, i in mine}
            assert x.m[tag]['saved'] == {s: sorted(['%d.pth' % i for i in range(n)] + ['%d.idx.pth' % i for i in range(n)]) for s, n in COUNTS.items()}
    counts = [n for s in COUNTS for n in one.m[tag]['rendered'][s]]
    if tag == 'fg':
        assert 0 < min(counts) and max(counts) < SIDE * SIDE                                   # really the foreground route
    else:
        assert counts == [SIDE * SIDE] * 7
    assert float.fromhex(one.m[tag]['v']) > 0


def test_default_is_unchanged_under_two_ranks(runs):
    """3: shard_batch=None - every rank still builds all 7 views, the one-rank call's."""
    one = runs[1, 0]
    for wr in MANY:
        x = runs[wr]
        assert x.m['plain']['registered'] == [list(v) for v in VIEWS] and len(x.m['plain']['seen']) == 7
        assert x.m['plain']['shard_batch'] is None and x.m['plain']['maps_world'] == 1
        assert x.m['plain']['owned'] == {s: list(range(n)) for s, n in COUNTS.items()}
        for s, i in VIEWS:
            _same_view(x, 'plain', one, 'plain', s, i)
        assert x.m['plain']['v'] == one.m['plain']['v'] and np.array_equal(x.a['plain_points'], one.a['plain_points'])


def test_attack_on_sharded_maps(runs):
    """4: nerfail_s over maps.batches('test', 4) of sharded maps = the same multi-rank run over maps every rank built in full,
    identical on all ranks: ownership by the attack's rule leaves no view missing and none wrong."""
    for w in (2, 3):
        first = runs[w, 0]
        for r in range(w):
            x = runs[w, r]
            for k in ('_best', '_last'):
                assert np.array_equal(x.a['attack_sharded' + k], first.a['attack_sharded' + k]), (w, r, k)
                assert np.array_equal(x.a['attack_sharded' + k], x.a['attack_plain' + k]), (w, r, k)
            assert x.m['attack_sharded'] == first.m['attack_sharded'] == x.m['attack_plain']
            assert len(x.m['attack_sharded']['stats']) == 2 and x.m['attack_sharded']['best_epoch'] == 0
        best = first.a['attack_sharded_best'].view(np.float32)
        assert (best[..., :3] != 0).any()                                             # the attack moved the table
    one = runs[1, 0]                                                                            # 7: one rank, keyword or not
    assert np.array_equal(one.a['attack_sharded_best'], one.a['attack_plain_best']) and one.m['attack_sharded'] == one.m['attack_plain']


def test_handoff_gather(runs):
    """5: the export epoch through nerfail_s_into(sink, ...) on every rank, then gather(): both stores identical on all ranks and
    equal to a sink one process fills from the same best table."""
    for w in (2, 3):
        for r in range(w):
            x = runs[w, r]
            assert x.m['handoff']['own'] == _owned(w, r)['train']
            assert 'never exported' in x.m['handoff']['before_gather'] and 'gather()' in x.m['handoff']['before_gather']
            assert x.m['handoff']['missing'] == []
            for k in ('images', 'adv'):
                assert np.array_equal(x.a['sink_' + k], runs[w, 0].a['sink_' + k]), (w, r, k)
                assert np.array_equal(x.a['sink_' + k], x.a['alone_' + k]), (w, r, k)
            assert x.a['sink_images'].shape == (2, SIDE, SIDE, 3) and x.a['sink_adv'].shape == (2, SIDE, SIDE, 4)
            assert all(x.a['sink_adv'][v].any() for v in range(2))                               # no slot was left black
    one = runs[1, 0]
    assert one.m['handoff']['before_gather'] == '' and np.array_equal(one.a['sink_images'], one.a['alone_images'])


def test_poisoned_retrain_on_every_rank(runs):
    """6: returns on all ranks with the same logged values, parameters, renders and reports; the sharded renders are what each
    rank gets by rendering every pose itself with the returned weights; restart and checkpoint refusal happen on all ranks."""
    for w in (2, 3):
        first = runs[w, 0]
        for r in range(w):
            x = runs[w, r]
            assert x.m['retrain']['attempts'] == 1 and x.m['retrain']['calls'] == [0] and x.m['retrain']['last'] == 4
            assert [l[0] for l in x.m['retrain']['logged']] == [2, 4]                            # check_ranks_agree ran at both
            assert x.m['retrain']['logged'] == first.m['retrain']['logged']
            assert x.m['retrain']['reports'] == first.m['retrain']['reports'] and sorted(x.m['retrain']['reports']) == ['test', 'train', 'val']
            assert np.array_equal(x.a['retrain_params'], first.a['retrain_params'])
            assert (x.m['retrain']['lines'] > 0) == (r == 0)                                     # rank 0 speaks
            for t, n in COUNTS.items():
                assert x.a['retrain_renders_' + t].shape == (n, SIDE, SIDE, 3) and x.a['retrain_renders_' + t].dtype == np.uint8
                assert np.array_equal(x.a['retrain_renders_' + t], first.a['retrain_renders_' + t]), (w, r, t)
                assert np.array_equal(x.a['retrain_renders_' + t], x.a['retrain_self_' + t]), (w, r, t)      # sharded = unsharded
            assert x.m['render_splits'] == dict(test=True, train=True, val=True, files=['%03d.png' % i for i in range(4)],
                                                folders=['renderonly_test_000003', 'renderonly_train_000003', 'renderonly_val_000003'])
            assert x.m['restart']['attempts'] == 2 and x.m['restart']['calls'] == [0, 1]         # all ranks restart together
            assert x.m['restart']['logged'] == first.m['restart']['logged'] and [l[0] for l in x.m['restart']['logged']] == [2, 4]
            assert np.array_equal(x.a['restart_params'], first.a['restart_params'])
            assert (x.m['restart']['restarting'], x.m['restart']['kept']) == ((1, 1) if r == 0 else (0, 0))
            assert '000002.tar' in x.m['ckpt'] and 'starts at iteration 2' in x.m['ckpt']        # refused on every rank
        assert len(set(first.a['retrain_renders_test'].reshape(-1).tolist())) > 8                # a rendered image, not a constant
        assert not np.array_equal(first.a['restart_params'], first.a['retrain_params'])          # attempt 1's NeRF, another seed


def test_one_rank_with_the_keywords_is_the_plain_call(runs):
    """7: shard_batch=4 and sharded=True in a one-rank process equal the calls without them."""
    one = runs[1, 0]
    for tag, plain in (('full', 'plain'), ('fg', 'plainfg')):
        assert one.m[tag]['owned'] == {s: list(range(n)) for s, n in COUNTS.items()} and one.m[tag]['maps_world'] == 1
        assert one.m[tag]['shard_batch'] == B and one.m[plain]['shard_batch'] is None
        assert one.m[tag]['registered'] == one.m[plain]['registered'] == [list(v) for v in VIEWS]
        for s, i in VIEWS:
            _same_view(one, tag, one, plain, s, i)
        assert one.m[tag]['v'] == one.m[plain]['v'] and one.m[tag]['rendered'] == one.m[plain]['rendered']
        assert np.array_equal(one.a[tag + '_points'], one.a[plain + '_points'])
    assert one.m['render_splits']['test'] and one.m['render_splits']['train'] and one.m['render_splits']['val']
    for t in COUNTS:
        assert np.array_equal(one.a['retrain_renders_' + t], one.a['retrain_self_' + t])
    assert one.m['retrain']['attempts'] == 1 and one.m['restart']['attempts'] == 2 and '000002.tar' in one.m['ckpt']
