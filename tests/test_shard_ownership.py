"""Host logic of the multi-rank scene: the ownership rule (sharding.batch_owner / owned_positions = attack._share, per batch),
SceneMaps.batches on sharded maps, and PoisonedTrainSet.gather through 2 and 3 gloo ranks on CPU tensors. No GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from nerfail_amd import sharding

NS, BATCHES, WORLDS = range(0, 21), range(1, 10), range(1, 10)


def test_owned_positions_partition_every_list():
    for n in NS:
        for bs in BATCHES:
            for world in WORLDS:
                own = [sharding.owned_positions(n, bs, r, world) for r in range(world)]
                assert sorted(p for o in own for p in o) == list(range(n)), (n, bs, world)      # each position once: a partition
                assert all(o == sorted(o) for o in own)


def test_batch_owner_agrees_with_owned_positions():
    for n in NS:
        for bs in BATCHES:
            for world in WORLDS:
                own = [set(sharding.owned_positions(n, bs, r, world)) for r in range(world)]
                for p in range(n):
                    r = sharding.batch_owner(p, n, bs, world)
                    assert p in own[r] and sum(p in o for o in own) == 1, (p, n, bs, world)


def test_every_batch_is_cut_by_shard_range():
    for n in NS:
        for bs in BATCHES:
            for world in WORLDS:
                for r in range(world):
                    own = sharding.owned_positions(n, bs, r, world)
                    for b0 in range(0, n, bs):
                        B = min(bs, n - b0)
                        lo, hi = sharding.shard_range(B, r, world)
                        assert [p for p in own if b0 <= p < b0 + B] == list(range(b0 + lo, b0 + hi)), (n, bs, world, r, b0)
                        if r >= B:                                   # a rank beyond a short batch's size owns nothing of it
                            assert hi == lo and not [p for p in own if b0 <= p < b0 + B]


def test_the_rule_refuses_nonsense():
    for bad in ((0, 0, 4, 2), (4, 4, 4, 2), (-1, 4, 4, 2), (0, 4, 0, 2)):
        with pytest.raises(ValueError):
            sharding.batch_owner(*bad)
    with pytest.raises(ValueError):
        sharding.owned_positions(4, 0, 0, 2)
    with pytest.raises(ValueError):
        sharding.owned_positions(4, 2, 2, 2)


def test_attack_share_is_the_same_rule(monkeypatch):
    """attack._share itself, on plain id lists with None maps and with CPU tensors: the ids it hands rank r of every batch are the
    ids at owned_positions(n, batch_size, r, world)."""
    from nerfail_amd import attack
    for n, bs, world in ((7, 4, 3), (4, 4, 3), (2, 4, 3), (1, 4, 3), (20, 8, 8), (13, 5, 2), (9, 9, 9), (6, 2, 1)):
        ids = [('scene', 'test', i) for i in range(n)]
        wi, ori = torch.arange(n * 2.).reshape(n, 2), torch.arange(n * 3.).reshape(n, 3)
        for r in range(world):
            monkeypatch.setattr(sharding, 'world_and_rank', lambda group=None, _w=world, _r=r: (_w, _r))
            got, got_wi = [], []
            for b0 in range(0, n, bs):
                parts, B, sharded = attack._share((None, None, ids[b0:b0 + bs]))
                assert B == len(ids[b0:b0 + bs]) and sharded == (world > 1)
                got += list(parts[2]) if parts is not None else []
                parts = attack._share((wi[b0:b0 + bs], ori[b0:b0 + bs], ids[b0:b0 + bs]))[0]
                got_wi += parts[0][:, 0].tolist() if parts is not None else []
            own = sharding.owned_positions(n, bs, r, world)
            assert got == [ids[p] for p in own], (n, bs, world, r)
            assert got_wi == [2. * p for p in own]


def test_scene_maps_batches_on_sharded_maps():
    from nerfail_amd.scene import SceneMaps

    class PS:
        Ns = 8
    ids = {'test': list('abcde'), 'train': list('xyz')}
    plain = SceneMaps(PS(), ids, 0., 0.02, (2, 2), 'k')
    assert plain.shard_batch is None and plain.world == 1 and plain.owned == {'test': [0, 1, 2, 3, 4], 'train': [0, 1, 2]}
    assert [b[2] for b in plain.batches(('test', 'train'), 4)] == [list('abcd'), list('exyz')]          # as before: one list, cut
    sh = SceneMaps(PS(), ids, 0., 0.02, (2, 2), 'k', owned={'test': [0, 1, 4], 'train': [0, 1]}, shard_batch=4, world=2)
    assert [b[2] for b in sh.batches(('test', 'train'), 4)] == [list('abcd'), ['e'], list('xyz')]       # each split on its own
    assert [b[2] for b in sh.batches('train', 4)] == [list('xyz')] and sh.batches('train', 4)[0][:2] == (None, None)
    with pytest.raises(ValueError, match='shard_batch = 4'):
        sh.batches('test', 2)


# ---------------------------------------------------------------------------------------------- PoisonedTrainSet.gather, gloo on CPU
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


N_SLOTS, SIDE = 7, 3
FILLED = {2: {0: [0, 1, 5], 1: [2, 4]},                    # slot 3 and slot 6: nobody
          3: {0: [0, 1], 1: [4], 2: [2, 5]}}
DUP = {2: {0: [0, 1, 5], 1: [1, 2]}, 3: {0: [0], 1: [0, 3], 2: [3, 6]}}


def _stores(rank):
    """What rank `rank`'s put() would have written to every slot: float bit patterns that a sum would not preserve (NaN payloads,
    -0., denormals) next to ordinary values."""
    rs = np.random.RandomState(50 + rank)
    bits = rs.randint(0, 2 ** 32, size=(N_SLOTS, SIDE, SIDE, 3), dtype=np.uint64).astype(np.uint32)
    bits[:, 0, 0, 0] = 0x7fc00001 + rank                     # a NaN with a payload
    bits[:, 0, 0, 1] = 0x80000000                            # -0.
    bits[:, 0, 0, 2] = 0x00000001 + rank                     # a denormal
    return bits.view(np.float32), rs.randint(0, 256, size=(N_SLOTS, SIDE, SIDE, 4)).astype(np.uint8)


def _gather_worker(rank, world, port, out_dir):
    sys.path[:0] = [ROOT]
    from nerfail_amd.retrain import PoisonedTrainSet
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    ids = [('v', s) for s in range(N_SLOTS)]
    out = {}
    for tag, plan in (('ok', FILLED[world]), ('dup', DUP[world])):
        sink = PoisonedTrainSet(ids, SIDE, SIDE, 4, device='cpu')
        img, adv = _stores(rank)
        for s in plan.get(rank, []):                         # the stores filled directly, not through put()
            sink.images[s] = torch.from_numpy(img[s])
            sink.adv_u8[s] = torch.from_numpy(adv[s])
            sink.filled.add(ids[s])
        try:
            assert sink.gather() is sink
            once = (sink.images.clone(), sink.adv_u8.clone(), set(sink.filled))
            sink.gather()                                    # a received view still belongs to its owner: nothing changes
            assert torch.equal(sink.images.view(torch.int32), once[0].view(torch.int32)) and torch.equal(sink.adv_u8, once[1])
            assert sink.filled == once[2]
            out[tag + '_error'] = ''
        except ValueError as e:
            out[tag + '_error'] = str(e)
        out[tag + '_images'], out[tag + '_adv'] = sink.images.numpy().view(np.uint32).copy(), sink.adv_u8.numpy().copy()
        out[tag + '_missing'] = np.array([v[1] for v in sink.missing()], np.int64)
        try:
            sink.require_complete()
            out[tag + '_complete'] = ''
        except ValueError as e:
            out[tag + '_complete'] = str(e)
    np.savez(os.path.join(out_dir, 'w%d_r%d.npz' % (world, rank)), **out)
    dist.destroy_process_group()


@pytest.mark.parametrize('world', [2, 3])
def test_gather_unites_the_sinks_bit_for_bit(world, tmp_path):
    mp.spawn(_gather_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    got = [np.load(tmp_path / ('w%d_r%d.npz' % (world, r))) for r in range(world)]
    want_img, want_adv = np.zeros((N_SLOTS, SIDE, SIDE, 3), np.uint32), np.zeros((N_SLOTS, SIDE, SIDE, 4), np.uint8)
    for r, slots in FILLED[world].items():
        img, adv = _stores(r)
        want_img[slots], want_adv[slots] = img.view(np.uint32)[slots], adv[slots]
    nobody = sorted(set(range(N_SLOTS)) - {s for slots in FILLED[world].values() for s in slots})
    assert nobody == [3, 6]
    for g in got:
        assert str(g['ok_error']) == ''
        assert np.array_equal(g['ok_images'], want_img) and np.array_equal(g['ok_adv'], want_adv)      # the union, the owners' BITS
        assert g['ok_missing'].tolist() == nobody                                                       # nobody's slot is still reported
        msg = str(g['ok_complete'])
        assert "2 of 7 train views were never exported: [('v', 3), ('v', 6)]" in msg and 'gather()' in msg
    dup = sorted(s for s in range(N_SLOTS) if sum(s in slots for slots in DUP[world].values()) > 1)
    for r, g in enumerate(got):                                                                        # refused on EVERY rank, by name
        assert 'more than one rank' in str(g['dup_error']) and str([('v', s) for s in dup]) in str(g['dup_error']), str(g['dup_error'])
        assert g['dup_missing'].tolist() == sorted(set(range(N_SLOTS)) - set(DUP[world].get(r, [])))    # nothing was moved


def test_gather_on_one_rank_is_a_no_op():
    from nerfail_amd.retrain import PoisonedTrainSet
    assert not dist.is_initialized()
    sink = PoisonedTrainSet([0, 1], SIDE, SIDE, 3, device='cpu')
    sink.images[1] = 0.5
    sink.filled.add(1)
    assert sink.gather() is sink and sink.missing() == [0] and float(sink.images[1].min()) == 0.5
    with pytest.raises(ValueError, match=r'1 of 2 train views were never exported: \[0\]$'):          # the one-rank text, unchanged
        sink.require_complete()
