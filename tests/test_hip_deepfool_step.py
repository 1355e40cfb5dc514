"""-m gpu: nerfail_deepfool_gate against tests/nerfail_ref.py, and nerfail_deepfool_step against the three things it fuses -
the existing nerfail_deepfool_norms, the mirror's torch arithmetic (nerfail_amd/deepfool.py:84-92) and the existing
nerfail_deepfool_apply - run on the same device tensors: the same chosen class, rot and spatial_out torch.equal.

Sizes: n = 3 * 32 * 32 table rows (two norm blocks of 2048 rows, the second half full), and n = 1440 = 3 * 24 * 20 (one partial
norm block; 5 full apply blocks of 256 rows and one of 160), the latter also under the guard-page allocator."""
import os
import sys

import numpy as np
import pytest
import torch

import nerfail_ref as R
from conftest import ROOT
from hiputil import N, T, dev

pytestmark = pytest.mark.gpu

SIZES = (3 * 32 * 32, 1440)


def gate(cla, o, target, m1, m2):
    """The record as 20 int32 words (device)."""
    from nerfail_amd import _lib
    lib = _lib.load()
    c = T(np.asarray(cla, np.float32).reshape(1, -1))
    rec = torch.full((_lib.DEEPFOOL_RECORD_WORDS,), 77, dtype=torch.int32, device=dev())
    _lib.check(lib.nerfail_deepfool_gate(_lib.dev(c), c.shape[1], o, target, float(m1), float(m2), _lib.dev(rec), _lib.stream()))
    return rec


GATE_CASES = {
    'o_first': ([5.0, 1.0, -2.0, 3.5, 0.25, -7.0, 4.0, 2.0], 0, -1, 1.0, 30.0),
    'o_middle': ([1.0, -2.0, 3.5, 5.0, 0.25, -7.0, 4.0, 2.0], 3, -1, 1.0, 30.0),
    'o_last': ([1.0, -2.0, 3.5, 0.25, -7.0, 4.0, 2.0, 5.0], 7, -1, 0.125, 100.0),
    'o_not_the_maximum': ([1.0, -2.0, 3.5, 0.25, -7.0, 4.0, 2.0, 5.0], 2, -1, 0.5, 100.0),       # done: the bump does not reach
    'targeted_0': ([1.0, -2.0, 3.5, 0.25, -7.0, 4.0, 2.0, 5.0], 7, 0, 1.0, 30.0),
    'targeted_last': ([1.0, -2.0, 3.5, 0.25, -7.0, 4.0, 2.0, 5.0], 5, 7, 1.0, 30.0),               # the target leads by less than m1
    'targeted_done': ([1.0, -2.0, 3.5, 0.25, -7.0, 4.0, 2.0, 9.5], 5, 7, 1.0, 30.0),
    'targeted_is_o': ([1.0, 6.0, 3.5], 1, 1, 1.0, 30.0),
    'two_classes': ([0.5, -0.5], 0, -1, 1.0, 8.0),
    'two_classes_targeted': ([0.5, -0.5], 0, 1, 0.25, 8.0),
    'tie_first_maximum': ([2.0, 1.0, 2.5, 2.5], 0, -1, 0.5, 1.0),                                 # 2.0 + 0.5 == 2.5 == 2.5: class 0, not done
    'tie_targeted': ([2.0, 1.0, 2.5, 0.0], 0, 2, 0.5, 1.0),                                       # bumped 2.5, 1.5, 2.5, 0.5: class 0 first, not done
    'nan_row': ([2.0, float('nan'), 2.5, 1.0], 0, -1, 0.5, 1.0),
    'nan_made_by_the_bump': ([float('-inf'), 1.0, 2.5, 1.0], 0, -1, float('inf'), 1.0),
    'm1_so_large_nothing_changes': ([5.0, 1.0, -2.0, 3.5, 0.25, -7.0, 4.0, 2.0], 4, -1, 1e6, 30.0),
    'rounding_of_the_bump': ([16777216.0, 3.0, 1.0], 1, -1, 16777215.0, 1.0),                      # 3 + 16777215 rounds to 16777218 in float32
}


@pytest.mark.parametrize('name', sorted(GATE_CASES))
def test_gate_matches_the_restatement(name):
    cla, o, target, m1, m2 = GATE_CASES[name]
    want = R.gate(cla, o, target, m1, m2)
    got = N(gate(cla, o, target, m1, m2))
    assert np.array_equal(got, R.record_words(want)), (name, got, R.record_words(want), want)
    # what the cases are there for
    if name.startswith('tie'):
        assert got[0] == 0 and got[1] == 0
    if name.startswith('nan'):
        assert got[0] == 0 and got[1] == -1
    if name in ('o_not_the_maximum', 'targeted_done'):
        assert got[0] == 1
    if name == 'm1_so_large_nothing_changes':
        assert got[0] == 0 and got[1] == 4


def grads(n_rhs, n, seed, flat=False):
    """[n_rhs][n,4] gradients, each slice at a scale of its own (three decades) unless `flat`."""
    rs = np.random.RandomState(seed)
    g = rs.normal(size=(n_rhs, n, 4)).astype(np.float32)
    return T(g if flat else g * (10.0 ** rs.uniform(-3, 0, size=(n_rhs, 1, 1))).astype(np.float32))


def table(n, seed):
    rs = np.random.RandomState(seed)
    s0 = rs.uniform(-250, 250, size=(n, 4)).astype(np.float32)
    s0[:, 3] = np.where(rs.uniform(size=n) < 0.85, 255.0, 0.0)
    rot = rs.normal(size=(n, 4)).astype(np.float32) * 20
    return T(s0), T(rot)


def step(G, rec, s0, rot, overshoot=0.02):
    """nerfail_deepfool_step on copies: (trace word, rot, spatial_out, scratch tail {norms2[8], best, scale})."""
    from nerfail_amd import _lib
    lib = _lib.load()
    n_rhs, n = G.shape[0], G.shape[1]
    nb = lib.nerfail_deepfool_step_scratch_bytes(n_rhs, n)
    scratch = torch.zeros((nb // 4,), dtype=torch.int32, device=dev())
    rot, out = rot.clone(), torch.full_like(s0, -12345.0)
    trace = torch.full((3,), -7, dtype=torch.int32, device=dev())
    _lib.check(lib.nerfail_deepfool_step(_lib.dev(G), n_rhs, n, _lib.dev(rec), _lib.dev(scratch), nb, float(overshoot), _lib.dev(s0),
                                         _lib.dev(rot), _lib.dev(out), _lib.dev(trace[1:2]), _lib.stream()))
    tr = N(trace)
    assert tr[0] == -7 and tr[2] == -7                                   # the slot, and only the slot
    return int(tr[1]), rot, out, scratch[-16:]


def three_calls(G, rec, s0, rot, targeted, overshoot=0.02):
    """What the mirror does for one iteration: nerfail_deepfool_norms, torch (deepfool.py:84-92), nerfail_deepfool_apply."""
    from nerfail_amd import _lib
    lib = _lib.load()
    C, n = G.shape[0], G.shape[1]
    nb = lib.nerfail_deepfool_norms_scratch_bytes(C, n)
    scratch = torch.empty((nb,), dtype=torch.uint8, device=dev())
    norms2 = torch.empty((C - 1,), dtype=torch.float32, device=dev())
    _lib.check(lib.nerfail_deepfool_norms(_lib.dev(G), C, n, _lib.dev(scratch), nb, _lib.dev(norms2), _lib.stream()))
    nrm = torch.sqrt(norms2)
    f_abs = rec[4 + 8:4 + 8 + C - 1].view(torch.float32)
    cls = rec[4:4 + C - 1]
    if not targeted:
        value_r = f_abs / (nrm + 0.0001)
        value_r = torch.where(torch.isnan(value_r), torch.full_like(value_r, float('inf')), value_r)
        best = torch.argmin(value_r)
        scale = f_abs[best] / ((nrm[best] ** 2) + 0.0001)
        chosen = int(cls[best]) if not bool(torch.isinf(value_r[best])) else -1
        scale = torch.where(torch.isinf(value_r[best]), torch.zeros_like(scale), scale)
    else:
        best = torch.zeros((), dtype=torch.int64, device=dev())
        scale = f_abs[0] / ((nrm[0] ** 2) + 0.0001)
        chosen = int(cls[0])
    rot, out = rot.clone(), torch.empty_like(s0)
    best_i, scale_f = (best + 1).to(torch.int32).reshape(1), scale.to(torch.float32).reshape(1)
    _lib.check(lib.nerfail_deepfool_apply(_lib.dev(G), C, n, _lib.dev(best_i), _lib.dev(scale_f), float(overshoot), _lib.dev(s0), _lib.dev(rot),
                                          _lib.dev(out), _lib.stream()))
    return chosen, rot, out, norms2, int(best_i), scale_f


def record_for(n_rhs, targeted, seed, fabs=None):
    """A record as the gate would leave it for n_rhs - 1 competitors, with |f'| of our choosing."""
    K = n_rhs - 1
    rs = np.random.RandomState(seed)
    f = np.zeros(8, np.float32)
    f[:K] = rs.uniform(0.5, 40.0, size=K) if fabs is None else fabs
    cls = np.full(8, -1, np.int32)
    cls[:K] = [6] if targeted else [k for k in range(n_rhs) if k != 2 % n_rhs][:K]
    return T(R.record_words(dict(done=0, argmax=2 % n_rhs, n_comp=K, targeted=int(targeted), cls=cls, fabs=f)))


def same_as_three_calls(n_rhs, n, targeted, seed, fabs=None, G=None):
    G = grads(n_rhs, n, seed) if G is None else G
    s0, rot = table(n, seed + 1)
    rec = record_for(n_rhs, targeted, seed + 2, fabs)
    cls_a, rot_a, out_a, tail = step(G, rec, s0, rot)
    cls_b, rot_b, out_b, norms2, best_b, scale_b = three_calls(G, rec, s0, rot, targeted)
    K = n_rhs - 1
    assert torch.equal(tail[:K], norms2.view(torch.int32))               # the same fixed tree, the same bits (a NaN included)
    assert cls_a == cls_b and int(tail[8]) == best_b
    assert torch.equal(tail[9:10], scale_b.view(torch.int32)), (tail[9:10].view(torch.float32), scale_b)
    assert torch.equal(rot_a.view(torch.int32), rot_b.view(torch.int32)) and torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))
    assert torch.equal(out_a[:, 3], s0[:, 3])
    return cls_a, rot_a, out_a, rot


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('n_rhs', (2, 3, 8))
def test_step_equals_norms_torch_apply(n_rhs, n):
    cls, rot_a, _, rot = same_as_three_calls(n_rhs, n, False, 10 * n_rhs)
    assert cls >= 0 and not torch.equal(rot_a, rot)


@pytest.mark.parametrize('n', SIZES)
def test_step_targeted_takes_competitor_0(n):
    cls, rot_a, _, rot = same_as_three_calls(2, n, True, 5)
    assert cls == 6 and not torch.equal(rot_a, rot)


def test_step_exact_tie_resolves_to_the_first():
    """Competitors 1 and 3 have the same gradient difference and the same |f'|: value_r ties exactly; competitor 0 is larger."""
    n = SIZES[1]
    G = grads(5, n, 3, flat=True)
    G[4] = G[2]
    cls, *_ = same_as_three_calls(5, n, False, 3, fabs=[900.0, 7.0, 800.0, 7.0], G=G)
    rec = N(record_for(5, False, 5))
    assert cls == int(rec[4 + 1])


def test_step_all_nan_candidates_leave_rot_unchanged():
    n = SIZES[1]
    cls, rot_a, out_a, rot = same_as_three_calls(4, n, False, 7, fabs=[float('nan')] * 3)
    assert cls == -1 and torch.equal(rot_a, rot)
    G = grads(3, n, 8)
    G[1, 5, 2] = float('nan')                                            # a NaN norm: that competitor is never chosen
    G[2, 9, 0] = float('inf')                                            # an infinite norm: value_r = 0 / inf ... = 0 is a number: chosen
    cls, rot_a, _, rot = same_as_three_calls(3, n, False, 9, G=G)
    assert cls == int(N(record_for(3, False, 11))[4 + 1])


def test_step_refuses_a_record_of_another_shape():
    """n_comp from device memory never becomes an address: a record whose competitor count is not n_rhs - 1 (out of range, or
    merely another call's) chooses nothing - rot unchanged, trace -1, spatial_out the clamp of the unchanged rot."""
    n = SIZES[1]
    G = grads(3, n, 12)
    s0, rot = table(n, 13)
    for bad in (9, -1, 1 << 30, 7, 1):
        rec = record_for(3, False, 14)
        rec[2] = bad
        cls, rot_a, out_a, tail = step(G, rec, s0, rot)
        assert cls == -1 and torch.equal(rot_a, rot) and float(tail[9:10].view(torch.float32)) == 0.0
        want = torch.clamp(s0 + 0.02 * rot, -255, 255)
        assert torch.equal(out_a[:, :3], want[:, :3]) and torch.equal(out_a[:, 3], s0[:, 3])


def test_two_runs_give_identical_bits():
    for n_rhs, n in ((8, SIZES[0]), (3, SIZES[1])):
        G = grads(n_rhs, n, 20)
        s0, rot = table(n, 21)
        rec = record_for(n_rhs, False, 22)
        a, b = step(G, rec, s0, rot), step(G, rec, s0, rot)
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))
    cla = GATE_CASES['o_middle']
    assert torch.equal(gate(*cla), gate(*cla))


# ---------------------------------------------------------------------------------------------------------- guard pages
def test_under_guard_pages(rank_launcher):
    """Both entry points at n = 1440 with every buffer ending at an unmapped page (the record is exactly 80 bytes, the scratch
    exactly nerfail_deepfool_step_scratch_bytes): a read or write past an end is a fault in the child's log."""
    rep = rank_launcher(os.path.abspath(__file__), 1, [], timeout=300, env={'NERFAIL_GUARD_ALLOC': '1'})
    log = '\n'.join(rep['logs'])
    assert rep['rc'] == [0], log
    assert 'Memory access fault' not in log and '[guard_alloc] active' in log and 'DEEPFOOL STEP GUARD OK' in log, log


def _guard_child():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import guard
    assert guard.install_if_wanted()
    n = SIZES[1]
    for name in ('o_last', 'targeted_last', 'two_classes', 'nan_row'):
        cla, o, target, m1, m2 = GATE_CASES[name]
        assert np.array_equal(N(gate(cla, o, target, m1, m2)), R.record_words(R.gate(cla, o, target, m1, m2)))
    for n_rhs, targeted in ((8, False), (3, False), (2, True)):
        same_as_three_calls(n_rhs, n, targeted, 30 + n_rhs)
    torch.cuda.synchronize()
    print('DEEPFOOL STEP GUARD OK', flush=True)


if __name__ == '__main__':
    _guard_child()
