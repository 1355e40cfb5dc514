"""-m gpu: the NeRF training kernels at every width, depth and skip position the C ABI accepts - each kernel instantiation
and host-side table behind `--netdepth/--netwidth[_fine]` that the (8, 256, 4) and (4, 64, no skip) tests never reach.

Truth is always the plain torch network in float64 under autograd (hiputil.torch_nerf_mlp); the yardstick is the SAME
network in float32 on the CPU: its per-parameter L2 distance to the float64 gradient is what rounding alone does (ReLU kinks
included). Bound per parameter, the rule tests/test_hip_train.py applies to the shipped shape:
    l2_err(HIP, f64) <= 2 x l2_err(torch f32, f64) + 2e-6      (2e-6: the kernel's own sin/cos, MFMA / atomic summation order)
Inputs: 37 rays x 31 samples = 1 147 samples = 35 full 32-sample tiles + one ragged tile, ~9 workgroups, the last partly
idle. The measured ratios are in DESIGN.md section 2."""
import numpy as np
import pytest
import torch

import synth
from conftest import l2_err
from hiputil import T, N, hip_nerf, dev, hip_mlp_grads, mlp_shape_inputs, torch_mlp_grads
from oracle import nerf as O

pytestmark = pytest.mark.gpu

R_, N_ = 37, 31

# (D, W, skip): forward-train form | backward-data form | weight-gradient kernel that the automatic dispatch selects
MATRIX = [(2, 256, -1),     # LDS <8,0,T> | LDS ring, zero pair iterations | LDS-staged, 7 groups
          (4, 256, 0),      # LDS <8,1,T> | LDS ring | LDS-staged: the encoding re-enters at layer 1
          (6, 256, 3),      # LDS <8,2,T> | LDS ring | LDS-staged: skip into the second layer of a pair
          (5, 256, 2),      # register <8,T> | register <8> | LDS-staged: odd depth through the automatic dispatch
          (10, 256, 4),     # register (D > 8) | register | LDS-staged: descriptor table full
          (2, 128, -1),     # LDS <4,0,T> | register <4> | register-fed NT = 4
          (4, 128, 1),      # LDS <4,2,T>
          (6, 128, 4),      # LDS <4,1,T>
          (3, 128, 0),      # register <4,T>: odd depth at NT = 4
          (4, 64, 1),       # LDS <2,2,T>
          (4, 64, 2),       # LDS <2,1,T>: W = 64 with a skip that fires
          (5, 64, 2)]       # register <2,T>

_CASES = {}


def _case(D, W, skip, seed=None, R=R_, n=N_):
    """Inputs, the float64 truth and the float32 yardstick of one architecture: computed once, shared, never written to."""
    seed = 1000 + 100 * D + W + skip if seed is None else seed
    key = (D, W, skip, seed, R, n)
    if key not in _CASES:
        sd, skips, pts, dirs, d_raw = mlp_shape_inputs(D, W, skip, R, n, seed)
        truth = torch_mlp_grads(sd, pts, dirs, d_raw, torch.float64, D, W, skips)
        f32 = torch_mlp_grads(sd, pts, dirs, d_raw, torch.float32, D, W, skips)
        _CASES[key] = dict(sd=sd, skips=skips, seed=seed + 1, pts=pts, dirs=dirs, d_raw=d_raw, truth=truth,
                           spread={k: l2_err(f32[k], truth[k]) for k in truth})
    return _CASES[key]


def _net(c, D, W, precision='f32'):
    sd, net = hip_nerf(D, W, c['seed'], requires_grad=True, precision=precision, skips=c['skips'])
    for k in sd:
        assert np.array_equal(sd[k], c['sd'][k])
    return net


def _selected(fwd_sel, bwd_sel, fn):
    """fn() with the forward / backward-data form forced (0 automatic, 1 register, 2 LDS ring); the selection is restored."""
    from nerfail_amd import _lib
    lib = _lib.load()
    pf, pb = lib.nerfail_mlp_fwd_select(fwd_sel), lib.nerfail_mlp_bwd_select(bwd_sel)
    try:
        return fn()
    finally:
        lib.nerfail_mlp_fwd_select(pf)
        lib.nerfail_mlp_bwd_select(pb)


def _judge(label, grads, c):
    """Every parameter against the float64 truth; prints one line per parameter, returns (worst err / bound, lines)."""
    worst, lines = 0.0, []
    assert set(grads) == set(c['truth'])
    for k in c['sd']:
        e, spread = l2_err(grads[k], c['truth'][k]), c['spread'][k]
        assert np.isfinite(grads[k]).all(), (label, k)           # (a NaN would drop out of max() below)
        bound = 2 * spread + 2e-6
        worst = max(worst, e / bound)
        lines.append('%-22s %-26s err %.2e  torch fp32-vs-fp64 %.2e  bound %.2e' % (label, k, e, spread, bound))
    print('\n'.join(lines))
    return worst, lines


@pytest.mark.parametrize('D,W,skip', MATRIX)
def test_mlp_gradients_every_architecture(D, W, skip, monkeypatch):
    """Forward-with-activations -> backward-data -> weight gradients through the C ABI (hiputil.hip_mlp_grads) at every row of
    the matrix, through the automatic dispatch; at W = 256 with both weight-gradient kernels, and at its even depths with both
    forward and both backward-data forms forced as well."""
    c = _case(D, W, skip)
    net = _net(c, D, W)
    pts, dirs, d_raw = T(c['pts']), T(c['dirs']), T(c['d_raw'])
    runs = [('auto', 0, 0, None)]
    if W == 256:
        runs = [('auto dw=lds', 0, 0, 'lds'), ('auto dw=reg', 0, 0, 'reg')]
        if D % 2 == 0 and D <= 8:
            runs += [('fwd=reg bwd=reg dw=lds', 1, 1, 'lds'), ('fwd=lds bwd=lds dw=lds', 2, 2, 'lds')]
    worst_all, all_lines = 0.0, []
    for label, fs, bs, dwk in runs:
        if dwk is not None:
            monkeypatch.setenv('NERFAIL_DW_KERNEL', dwk)
        grads = _selected(fs, bs, lambda: hip_mlp_grads(net, pts, dirs, d_raw))
        worst, lines = _judge(label, grads, c)
        print('HIP f32 training kernels (D, W, skip) = (%d, %d, %d) [%s] vs float64 autograd: worst error / bound = %.2f'
              % (D, W, skip, label, worst))
        worst_all, all_lines = max(worst_all, worst), all_lines + lines
    print('SHAPE (%d, %d, %d): worst error / bound over %d runs = %.2f' % (D, W, skip, len(runs), worst_all))
    assert worst_all <= 1.0, '\n'.join(all_lines)


def test_joint_launch_fills_the_group_and_descriptor_tables(monkeypatch):
    """Two D = 10 W = 256 networks in ONE weight-gradient launch: 16 groups each = kDwMaxGroups, 14 descriptors = kMaxDesc
    (mlp_dw.hip). The first network's sample count is a multiple of 32 (the joint launch's contract); each network is held to
    its own float64 truth by the rule of this file."""
    from nerfail_amd import _train
    monkeypatch.delenv('NERFAIL_DW_KERNEL', raising=False)   # the default at W = 256: the LDS-staged kernel, whose tables these are
    D, W, skip = 10, 256, 4
    c1 = _case(D, W, skip)                                   # second network: the matrix's own case, 1 147 samples
    R0, N0 = 18, 32                                          # first network: 32 * 18 = 576 samples, other weights
    c0 = _case(D, W, skip, seed=4242, R=R0, n=N0)
    n0, n1 = _net(c0, D, W), _net(c1, D, W)
    M0, M1 = R0 * N0, R_ * N_
    assert M0 % 32 == 0
    nA = _train.acts_floats(n0, M0)
    acts = torch.empty((nA + _train.acts_floats(n1, M1),), device=dev())
    _train.mlp_fwd_train(n0, T(c0['pts']), T(c0['dirs']), acts=acts[:nA])
    _train.mlp_fwd_train(n1, T(c1['pts']), T(c1['dirs']), acts=acts[nA:])
    d_raw = torch.cat([T(c0['d_raw']).reshape(-1, 4), T(c1['d_raw']).reshape(-1, 4)]).contiguous()
    g0, g1 = _train._new_grads(n0, False), _train._new_grads(n1, False)
    for t in g0 + g1:
        t.fill_(float('nan'))                                # the LDS-staged kernel overwrites: nothing of this may survive
    _train.mlp_backward2(n0, d_raw, acts, g0, M0, n1, g1, M1)
    worst_all, all_lines = 0.0, []
    for label, net, g, c in (('joint net 0', n0, g0, c0), ('joint net 1', n1, g1, c1)):
        byp = {id(p): n for n, p in net.named_parameters()}
        grads = {byp[id(p)]: t.double().cpu().numpy() for p, t in zip(_train.ordered_params(net), g)}
        worst, lines = _judge(label, grads, c)
        worst_all, all_lines = max(worst_all, worst), all_lines + lines
    print('SHAPE (10, 256, 4) joint two-network launch, 32 groups / 14 descriptors: worst error / bound = %.2f' % worst_all)
    assert worst_all <= 1.0, '\n'.join(all_lines)


@pytest.mark.parametrize('dw_kernel', ['lds', 'reg'])
def test_depth_beyond_the_descriptor_table_is_refused(dw_kernel, monkeypatch):
    """D = 11 needs 15 descriptors; the table holds 14. nerfail_mlp_bwd_weights must refuse on the host, before any launch -
    before the register-fed path's zeroing launch too: the gradient buffers keep their pre-fill pattern."""
    from nerfail_amd import _lib, _train
    from nerfail_amd.run_nerf_helpers import NeRF
    monkeypatch.setenv('NERFAIL_DW_KERNEL', dw_kernel)
    lib = _lib.load()
    D, W, skip, M = 11, 256, 4, 96
    net = NeRF(D=D, W=W, input_ch=63, input_ch_views=27, output_ch=5, skips=[skip], use_viewdirs=True).to(dev())
    na, nz = lib.nerfail_mlp_train_acts_floats(D, W, M), lib.nerfail_mlp_train_dz_floats(D, W, M)
    assert na > 0 and nz > 0
    acts, dz = torch.zeros((na,), device=dev()), torch.zeros((nz,), device=dev())
    g = _train._new_grads(net, False)
    for t in g:
        t.fill_(7.0)
    for flags in (0, _lib.DW_ACCUMULATE):
        scratch, nbytes = _train.dw_scratch(net, M, 0, flags, dev())
        with pytest.raises(_lib.NerfailError, match='too deep'):
            _lib.check(lib.nerfail_mlp_bwd_weights(D, W, skip, _lib.dev(acts), _lib.dev(dz), M, _train._grads_struct(net, g), 0, None,
                                                   flags, _lib.dev(scratch), nbytes, _lib.stream()))
        torch.cuda.synchronize()
        for t in g:
            assert bool((t == 7.0).all())


@pytest.mark.parametrize('D,W,skip', [(4, 64, 1), (3, 128, 0), (6, 256, 3)])
def test_split_precision_kernels_other_architectures(D, W, skip, monkeypatch):
    """precision='f16x3' away from (8, 256, 4) and (4, 64, -): make_f16_layout accepts every shape make_layout accepts, so all
    three run. (i) split backward-data / weight gradients against the exact-f32 kernels on the SAME saved activations: 2e-5 L2
    per parameter, the bound of test_split_backward_kernels_match_f32_kernels; (ii) all three split kernels against the
    float64 truth by the combined rule of test_split_gradients_vs_float64_truth."""
    c = _case(D, W, skip)
    net = _net(c, D, W)
    pts, dirs, d_raw = T(c['pts']), T(c['dirs']), T(c['d_raw'])
    for dwk in (('lds', 'reg') if W == 256 else ('reg',)):
        monkeypatch.setenv('NERFAIL_DW_KERNEL', dwk)
        ref = hip_mlp_grads(net, pts, dirs, d_raw, 'f32', 'f32', 'f32')
        for bd, dw in (('split', 'f32'), ('f32', 'split'), ('split', 'split')):
            got = hip_mlp_grads(net, pts, dirs, d_raw, 'f32', bd, dw)
            assert all(np.isfinite(got[k]).all() for k in ref)
            worst = max((l2_err(got[k], ref[k]), k) for k in ref)
            print('SPLIT (%d, %d, %d) dw=%s bd=%s dw=%s vs exact f32 on the same activations: worst %.2e (%s)'
                  % (D, W, skip, dwk, bd, dw, worst[0], worst[1]))
            assert worst[0] < 2e-5, (dwk, bd, dw, worst)
        e = {}
        for tag, modes in (('f32', ('f32', 'f32', 'f32')), ('split', ('split', 'split', 'split'))):
            got = hip_mlp_grads(net, pts, dirs, d_raw, *modes)
            e[tag] = {k: l2_err(got[k], c['truth'][k]) for k in c['truth']}
        net.precision = 'f32'
        wf, ws = max(e['f32'].values()), max(e['split'].values())
        print('SPLIT (%d, %d, %d) dw=%s vs float64 autograd: worst f32 %.2e, worst split %.2e' % (D, W, skip, dwk, wf, ws))
        for k in c['truth']:
            assert e['f32'][k] < 5e-3 and e['split'][k] < 5e-3, (k, e['f32'][k], e['split'][k])
            assert e['split'][k] < 10 * e['f32'][k] + 3e-4, (k, e['f32'][k], e['split'][k])


# ---------------------------------------------------------------------------------------------- the training step
# (coarse arch, fine arch or None = one network for both passes, N_samples, N_importance, branch of RenderRaysTrain.backward)
STEPS = {'same_4_64_1_40+60': ((4, 64, 1), (4, 64, 1), 40, 60, 'separate'),        # 33 * 40 % 32 != 0; fine count 100: IPL 2
         'same_6_256_3_64+192': ((6, 256, 3), (6, 256, 3), 64, 192, 'joint'),      # fine count 256: IPL 4
         'mixed_4_64_2__5_128_2_64+128': ((4, 64, 2), (5, 128, 2), 64, 128, 'separate'),
         'shared_4_128_1_64+128': ((4, 128, 1), None, 64, 128, 'shared')}


@pytest.mark.parametrize('precision', ['f32', 'f16x3'])
@pytest.mark.parametrize('cfg', list(STEPS))
def test_training_step_other_sample_counts_and_architectures(cfg, precision, monkeypatch):
    """render_rays -> img2mse x 2 -> backward() outside 64 + 128 samples and outside equal architectures, against the
    generalised oracle.nerf.train_step_grads with test_odd_ray_counts_gradients' bounds at R = 33: loss to 1e-5 relative,
    every parameter to 5e-3 L2. Which branch of RenderRaysTrain.backward ran is read off its mlp_backward2 calls."""
    from nerfail_amd import run_nerf as RN, _train
    ac, af, Ns, Ni, branch = STEPS[cfg]
    R = 33

    def sk(a):
        return (a[2],) if a[2] >= 0 else ()
    sc, coarse = hip_nerf(ac[0], ac[1], 91, requires_grad=True, precision=precision, skips=sk(ac))
    sf, fine = (None, None) if af is None else hip_nerf(af[0], af[1], 92, requires_grad=True, precision=precision, skips=sk(af))
    rs = np.random.RandomState(R + Ns)
    rays = synth.ray_batch(R, seed=90 + Ns)
    target = rs.uniform(size=(R, 3)).astype(np.float32)
    t_rand, u = rs.uniform(size=(R, Ns)).astype(np.float32), rs.uniform(size=(R, Ni)).astype(np.float32)
    ref = O.train_step_grads(rays, sc, sf, target, Ns, Ni, t_rand=t_rand, u=u, arch_coarse=(ac[0], ac[1], sk(ac)),
                             arch_fine=None if af is None else (af[0], af[1], sk(af)))
    calls, real = [], _train.mlp_backward2

    def spy(net0, d_raw, acts, grads0, M0, net1, grads1, M1, accumulate=False):
        calls.append((M0, M1, bool(accumulate)))
        return real(net0, d_raw, acts, grads0, M0, net1, grads1, M1, accumulate)
    monkeypatch.setattr(_train, 'mlp_backward2', spy)
    r = RN.render_rays(T(rays), coarse, None, Ns, N_importance=Ni, network_fine=fine, white_bkgd=True, perturb=1.,
                       t_rand=T(t_rand), u=T(u))
    loss = RN.img2mse(r['rgb_map'], T(target)) + RN.img2mse(r['rgb0'], T(target))
    loss.backward()
    Mc, Mf = R * Ns, R * (Ns + Ni)
    want = {'joint': [(Mc, Mf, False)], 'shared': [(Mc + Mf, 0, False)], 'separate': [(Mf, 0, True), (Mc, 0, True)]}[branch]
    assert calls == want, calls
    rel = abs(float(loss.detach()) - ref['loss']) / abs(ref['loss'])
    worst = (0.0, None)
    for tag, net in (('grads_coarse', coarse), ('grads_fine', fine)):
        if net is None:
            continue
        for k, p in net.named_parameters():
            assert bool(torch.isfinite(p.grad).all()), (tag, k)
            worst = max(worst, (l2_err(N(p.grad), ref[tag][k]), tag + ' ' + k))
    print('STEP %s %s [%s]: loss rel err %.1e (bound 1e-5), worst parameter L2 err %.2e (%s, bound 5e-3)'
          % (cfg, precision, branch, rel, worst[0], worst[1]))
    assert rel < 1e-5
    assert worst[0] < 5e-3, worst
