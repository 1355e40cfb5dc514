"""tools/mfma_gaps.py on a short hand-written assembly fragment: gap sizes, what is not counted, over-budget gaps with their
mix and landmark, exposed blocks, and the s_nop listing."""
import importlib.util
import os

from conftest import ROOT

FRAGMENT = '''
	.text
	.globl	other_kernel
	.type	other_kernel,@function
other_kernel:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v0, 0
	s_endpgm
.Lfunc_end0:
	.size	other_kernel, .Lfunc_end0-other_kernel
	.globl	stream_kernel
	.type	stream_kernel,@function
stream_kernel:                          ; @stream_kernel
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0                     ; before the first MFMA: no gap
.LBB1_1:                                ; =>This Inner Loop Header: Depth=1
	v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]
	; sched_barrier mask(0x00000000)
	v_mfma_f32_16x16x32_bf16 a[4:7], v[0:3], v[8:11], a[4:7]
	ds_read_b128 v[12:15], v20 offset:1024
	s_waitcnt lgkmcnt(0)
	v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]
	s_nop 7
	v_accvgpr_read_b32 v30, a0
	v_max_i32_e32 v30, 0, v30
	s_nop 0
	v_mfma_f32_16x16x32_bf16 a[4:7], v[0:3], v[8:11], a[4:7]
.LBB1_2:
	s_waitcnt vmcnt(12)
	s_barrier
	s_add_i32 s8, s8, 0x6000
	s_cmp_eq_u32 s8, s9
	s_cselect_b32 s8, s10, s8
	buffer_load_dwordx4 v21, s[44:47], s8 offen offset:1024 lds
	v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]
	v_accvgpr_mov_b32 a8, a0
	v_accvgpr_mov_b32 a9, a1
	v_accvgpr_mov_b32 a10, a2
	v_mfma_f32_16x16x32_bf16 a[4:7], v[0:3], v[8:11], a[4:7]
EXPOSED
	v_mfma_f32_16x16x32_bf16 a[0:3], v[0:3], v[4:7], a[0:3]
	global_store_dwordx4 v[40:41], v[12:15], off
	s_endpgm
.Lfunc_end1:
	.size	stream_kernel, .Lfunc_end1-stream_kernel
'''.replace('EXPOSED\n', '\tv_fma_f32 v50, v51, v52, v50\n' * 20)


def _tool():
    spec = importlib.util.spec_from_file_location('nf_mfma_gaps', os.path.join(ROOT, 'tools', 'mfma_gaps.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fragment_counts():
    G = _tool()
    kernels = G.parse(FRAGMENT)
    assert list(kernels) == ['stream_kernel']                       # a function without MFMAs has no gaps
    gaps = kernels['stream_kernel']
    assert len(gaps) == 6                                           # 7 MFMAs; the store behind the last one is no gap
    assert [G.size(g) for g in gaps] == [0, 1, 2, 5, 3, 20]         # s_nop and s_waitcnt are not counted
    s = G.summarise(gaps)
    assert s['mfmas'] == 7
    assert dict(s['hist']) == {0: 1, 1: 1, 2: 1, 3: 1, 5: 1}
    assert s['exposed'] == [20]
    assert s['waits'] == 2
    assert [(o, p) for o, p, _ in s['nops']] == [('7', 'v_mfma'), ('0', 'v_max_i32_e32')]
    assert s['excess'] == 2
    assert len(s['over']) == 1
    over = s['over'][0]
    assert over.label == '.LBB1_1'                                  # the label before the MFMA that opens the gap
    assert FRAGMENT.splitlines()[over.line - 1].lstrip().startswith('v_mfma')
    mix = {}
    for m, _ in over.ins:
        mix[G.classify(m)] = mix.get(G.classify(m), 0) + 1
    assert mix == {'s_': 5, 'buffer_/global_': 1}                   # s_waitcnt and s_barrier are s_ too; only the size skips the wait


def test_classes_by_prefix():
    G = _tool()
    assert G.classify('v_mfma_f32_32x32x2_f32') == 'v_mfma'
    assert G.classify('v_cvt_pk_bf16_f32') == 'v_'
    assert G.classify('s_cselect_b32') == 's_'
    assert G.classify('ds_read_b128') == 'ds_'
    assert G.classify('buffer_load_dwordx4') == G.classify('global_load_dwordx4') == 'buffer_/global_'
    assert G.classify('flat_load_dword') == 'other'


def test_report_text():
    G = _tool()
    text = G.report('stream_kernel', G.parse(FRAGMENT)['stream_kernel'])
    assert 'static MFMAs 7; stream gaps 5; over budget (> 3) 1, 2 instructions above it; exposed blocks [20]' in text
    assert 's_nop 7   after v_mfma' in text
    assert '(after .LBB1_1): 5 = buffer_/global_1 s_4' in text
    assert 's_barrier:1' in text and 's_waitcnt:1' in text
