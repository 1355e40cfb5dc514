"""tests/nerfail_ref.py (numpy restatement of the DeepFool gate, of the step's choice and of the NeRFail pass bookkeeping) held to
fixture g27, the reference's gauss_net and deepfool.deepfool driven through the AN:269-505 loop shape
(tests/golden/make_golden_nerfail.py). Discrete decisions must be equal; values must lie within the fixture's own
float32-vs-float64 distance."""
import numpy as np
import pytest

import nerfail_problem as NP
import nerfail_ref as R


@pytest.fixture(scope='module')
def g():
    return NP.load()


def _m2_at_calls(g, tag):
    """Replays the pass bookkeeping over the fixture's visits. Yields per pass (book state before the pass, list of
    (view, skipped, iter_k, m1, m2 at the call), the record the book arrives at)."""
    targeted, label, m1, m2, limit = NP.run_args(g, tag)
    P, H, W, C, epochs, n_views, n_export, cap = NP.shape(g)
    run = g['runs'][tag]
    book = R.Book(epochs, m1, m2, targeted, cap, limit)
    out = []
    for p, rec in enumerate(run['passes']):
        assert book.running(), (tag, p)
        export = book.begin_pass()
        epoch, m1_pass = book.epoch, book.m1
        calls = []
        visits, logits = run['visits'][p], run['logits'][p]
        seen = NP.pass_views(g, tag, p) if not export else list(range(n_export))
        assert export or all(visits[v, 0] >= 0 for v in seen)
        correct = 0
        for v in seen:
            cla, ori_cla = logits[v, 0], logits[v, 1]
            correct += int(np.argmax(cla) == label)
            if export:
                book.exported()
                continue
            skipped = int(np.argmax(cla) != np.argmax(ori_cla))              # AN:387-394
            assert skipped == visits[v, 0], (tag, p, v)
            if not skipped:
                calls.append((v, int(visits[v, 1]), book.m1, book.m2))
                book.visit(int(visits[v, 1]))
        raises = book.raises
        taken = book.end_pass(correct / len(seen))
        out.append((epoch, m1_pass, export, calls, dict(next_epoch=book.epoch, m1=book.m1, m2=book.m2, taken=int(taken), raises=raises,
                                                        views=len(seen), attack_correct=correct, attack_acc=correct / len(seen))))
    assert not book.running(), tag
    return out, book


@pytest.mark.parametrize('tag', NP.TAGS)
def test_bookkeeping_reproduces_the_reference_loop(g, tag):
    passes, book = _m2_at_calls(g, tag)
    rec = g['runs'][tag]['passes']
    assert len(passes) == len(rec)
    for p, (epoch, m1_pass, export, calls, d) in enumerate(passes):
        r = rec[p]
        assert (epoch, d['next_epoch'], m1_pass, d['m1'], d['m2']) == tuple(int(r[c]) for c in (NP.EPOCH, NP.NEXT_EPOCH, NP.M1_PASS, NP.M1, NP.M2)), (tag, p)
        assert (d['views'], d['taken'], d['raises'], d['attack_correct']) == tuple(int(r[c]) for c in (NP.VIEWS, NP.TAKEN, NP.RAISES, NP.ATTACK_CORRECT)), (tag, p)
        assert d['attack_acc'] == r[NP.ATTACK_ACC]
    assert (book.m1_best, book.m2_best) == (int(g['runs'][tag]['m1_best']), int(g['runs'][tag]['m2_best'])) and book.best_acc == float(g['runs'][tag]['best_acc'])


def test_fixture_covers_what_it_was_made_for(g):
    cap = NP.shape(g)[7]
    v = np.concatenate([g['runs'][t]['visits'][g['runs'][t]['passes'][:, NP.EPOCH] < NP.shape(g)[4] - 1].reshape(-1, 2 + cap) for t in NP.TAGS])
    v = v[v[:, 0] >= 0]
    assert (v[:, 0] == 1).any() and ((v[:, 0] == 0) & (v[:, 1] < cap)).any() and ((v[:, 0] == 0) & (v[:, 1] == cap)).any()
    assert g['runs']['m2_raise']['passes'][:, NP.RAISES].sum() >= 1
    b = g['runs']['bisect']['passes']
    m1s = np.diff(np.concatenate([b[:1, NP.M1_PASS], b[:, NP.M1]]))     # the m1 it started with, then m1 at every pass's end
    assert (m1s < 0).any() and (m1s > 0).any()
    assert any(not np.array_equal(g['runs'][t]['best_rgb'], g['runs'][t]['last_attack_rgb']) for t in NP.TAGS)


@pytest.mark.parametrize('tag', NP.TAGS)
def test_gate_and_choice_reproduce_every_iteration(g, tag):
    """Every loop forward of every DeepFool call of the float32 run: the gate's break decision against iter_k, the choice
    against the recorded class, the scale against the reference's within its float32-vs-float64 distance."""
    targeted, label = NP.run_args(g, tag)[:2]
    C, cap = NP.shape(g)[3], NP.shape(g)[7]
    run = g['runs'][tag]
    passes, _ = _m2_at_calls(g, tag)
    worst, n_iter = 0., 0
    for p, (epoch, m1_pass, export, calls, d) in enumerate(passes):
        for v, iter_k, m1, m2 in calls:
            o = int(np.argmax(run['logits'][p, v, 1]))
            target = label if targeted else -1
            for j in range(min(iter_k + 1, cap)):
                it32, it64 = run['iters'][p, v, j], run['iters_f64'][p, v, j]
                rec = R.gate(it32[:C], o, target, m1, m2)
                assert rec['done'] == int(j == iter_k), (tag, p, v, j)
                assert rec['n_comp'] == (1 if targeted else C - 1) and rec['targeted'] == int(targeted)
                if j == iter_k:
                    continue
                nrm = it32[C:2 * C - 1].astype(np.float64)
                best, scale, bi = R.choose(rec['fabs'], (nrm * nrm).astype(np.float32), rec['n_comp'], targeted)
                assert int(rec['cls'][bi]) == int(run['visits'][p, v, 2 + j]) and best == bi + 1, (tag, p, v, j)
                ref32, ref64 = float(it32[-1]), float(it64[-1])
                bound, err = abs(ref32 - ref64), abs(float(scale) - ref64)
                assert err <= bound, (tag, p, v, j, float(scale), ref32, ref64)
                worst = max(worst, err / bound if bound > 0 else 0.)
                n_iter += 1
    print('g27 %s: %d iterations, worst |scale - reference f64| / bound %.3f' % (tag, n_iter, worst))
    assert n_iter > 0 and worst <= 1.0


def test_gate_edge_cases():
    cla = np.array([1.0, 3.0, 2.0, -1.0], np.float32)
    r = R.gate(cla, 1, -1, 0.5, 10.0)
    assert (r['done'], r['argmax'], r['n_comp']) == (0, 1, 3) and r['cls'][:4].tolist() == [0, 2, 3, -1]
    assert r['fabs'][:3].tolist() == [abs(np.float32(1.0) - np.float32(13.5)), 11.5, 14.5]
    r = R.gate(cla, 2, -1, 0.0, 10.0)                                    # the clean class is no longer the maximum
    assert (r['done'], r['argmax']) == (1, 1)
    r = R.gate(cla, 1, 2, 0.5, 10.0)                                     # targeted: every class but 2 is bumped
    assert (r['done'], r['argmax'], r['n_comp'], r['cls'][0]) == (0, 1, 1, 2) and r['fabs'][0] == abs(np.float32(2.0) - np.float32(13.5))
    r = R.gate(np.array([2.0, 1.0, 2.5], np.float32), 0, -1, 0.5, 1.0)   # exact tie of the bumped logits: the first maximum
    assert (r['done'], r['argmax']) == (0, 0)
    r = R.gate(np.array([2.0, np.nan, 2.5], np.float32), 0, -1, 0.5, 1.0)
    assert (r['done'], r['argmax']) == (0, -1)
    assert R.choose([1.0, 1.0, 3.0], [4.0, 4.0, 1.0], 3, False)[2] == 0   # exact tie of two value_r: the first
    assert R.choose([np.nan, np.nan], [1.0, 1.0], 2, False) == (1, 0.0, -1)
    assert R.choose([1.0, 2.0], [1.0, 1.0], 2, False, K=3) == (1, 0.0, -1)
