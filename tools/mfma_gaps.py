#!/usr/bin/env python3
"""Instructions between consecutive MFMAs in the device assembly of a kernel (static code, in program order).

The bf16x3 render kernel (nerfail_amd/csrc/mlp_x3.hip) runs one wave per SIMD, which issues in order: a 16x16x32 MFMA leaves
about 8 of its 16 cycles for other instructions, so whatever sits between two MFMAs beyond a few instructions delays the
second one directly. This tool reads the assembly hipcc writes with `-S` (the flags of nerfail_amd/build.py; `--emit` runs
that compile) and prints, per kernel:

  * the histogram of gap sizes (instructions between two consecutive MFMAs; `s_nop` and `s_waitcnt` are not counted in the
    size and are listed separately). Gaps longer than EXPOSED instructions are the exposed phases between MFMA streams
    (encoding, heads, part starts) and are listed by size, not in the histogram;
  * every stream gap over BUDGET = 3 instructions: its instruction mix by class and by mnemonic, and the nearest landmark
    (the last label before it and the line of the assembly file);
  * every `s_nop` inside the stream with its operand and the instruction before it (hazard padding).

Mnemonics are classified by prefix only: v_mfma, v_, s_, ds_, buffer_/global_, other.

    python3 tools/mfma_gaps.py file.s [--kernel SUBSTRING] [--quiet]
    python3 tools/mfma_gaps.py --emit nerfail_amd/csrc/mlp_x3.hip [--kernel SUBSTRING] [--quiet]
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

BUDGET = 3          # instructions of any kind per gap, s_nop and s_waitcnt excluded
EXPOSED = 16        # a longer gap is an exposed block, not part of an MFMA stream
UNCOUNTED = ('s_nop', 's_waitcnt')

_LABEL = re.compile(r'^([A-Za-z_.$][\w.$]*):')
_FUNC_TYPE = re.compile(r'^\s*\.type\s+([\w.$]+),@function')
_INS = re.compile(r'^\s+([a-z][a-z0-9_]*)\b\s*([^;]*)')

Gap = collections.namedtuple('Gap', 'line label ins')          # ins: [(mnemonic, operands)]


def classify(mnem):
    if mnem.startswith('v_mfma'):
        return 'v_mfma'
    for p in ('v_', 's_', 'ds_'):
        if mnem.startswith(p):
            return p
    if mnem.startswith('buffer_') or mnem.startswith('global_'):
        return 'buffer_/global_'
    return 'other'


def parse(text):
    """-> {kernel: [Gap]}: for every function, the instructions between consecutive v_mfma, in program order.
    What precedes the first MFMA and follows the last one is no gap."""
    funcs = set(m.group(1) for m in map(_FUNC_TYPE.match, text.splitlines()) if m)
    out, cur, label, pending, seen_mfma, start = collections.OrderedDict(), None, None, [], False, 0
    for no, raw in enumerate(text.splitlines(), 1):
        line = raw.split(';')[0].rstrip()
        m = _LABEL.match(line)
        if m:
            if m.group(1) in funcs:
                cur, seen_mfma, pending = m.group(1), False, []
                out[cur] = []
            elif m.group(1).startswith('.Lfunc_end'):
                cur = None
            label = m.group(1)
            continue
        if cur is None:
            continue
        m = _INS.match(line)
        if not m or line.lstrip().startswith('.'):
            continue
        mnem, ops = m.group(1), m.group(2).strip()
        if classify(mnem) == 'v_mfma':
            if seen_mfma:
                out[cur].append(Gap(start, lab0, pending))
            seen_mfma, pending, start, lab0 = True, [], no, label
            continue
        if seen_mfma:
            pending.append((mnem, ops))
    return collections.OrderedDict((k, v) for k, v in out.items() if v)


def size(gap):
    return sum(1 for m, _ in gap.ins if m not in UNCOUNTED)


def summarise(gaps):
    """-> dict: mfmas, hist {size: count} of stream gaps, exposed [sizes], over [Gap], nops [(operand, previous, line)],
    waits (s_waitcnt inside the stream), excess (instructions above BUDGET summed over the stream gaps)."""
    hist, exposed, over, nops, waits, excess = collections.Counter(), [], [], [], 0, 0
    for g in gaps:
        n = size(g)
        if n > EXPOSED:
            exposed.append(n)
            continue
        hist[n] += 1
        if n > BUDGET:
            over.append(g)
            excess += n - BUDGET
        prev = 'v_mfma'
        for m, o in g.ins:
            if m == 's_nop':
                nops.append((o, prev, g.line))
            if m == 's_waitcnt':
                waits += 1
            prev = m
    return dict(mfmas=len(gaps) + 1, hist=hist, exposed=sorted(exposed), over=over, nops=nops, waits=waits, excess=excess)


def report(name, gaps, quiet=False):
    s = summarise(gaps)
    lines = ['== %s' % name,
             'static MFMAs %d; stream gaps %d; over budget (> %d) %d, %d instructions above it; exposed blocks %s'
             % (s['mfmas'], sum(s['hist'].values()), BUDGET, len(s['over']), s['excess'], s['exposed'] or 'none'),
             'gap size : ' + ' '.join('%5d' % k for k in sorted(s['hist'])),
             'gaps     : ' + ' '.join('%5d' % s['hist'][k] for k in sorted(s['hist'])),
             's_waitcnt in the stream: %d; s_nop in the stream: %d' % (s['waits'], len(s['nops']))]
    byop = collections.Counter((o, p) for o, p, _ in s['nops'])
    for (o, p), n in sorted(byop.items(), key=lambda kv: -kv[1]):
        lines.append('  s_nop %-3s after %-28s x %d' % (o, p, n))
    mix_all = collections.Counter(m for g in s['over'] for m, _ in g.ins)
    if mix_all:
        lines.append('mix of the over-budget gaps: ' + ', '.join('%s %d' % kv for kv in mix_all.most_common()))
    if not quiet:
        for g in s['over']:
            cls = collections.Counter(classify(m) for m, _ in g.ins if m not in UNCOUNTED)
            mix = collections.Counter(m for m, _ in g.ins)
            lines.append('  line %d (after %s): %d = %s | %s' % (g.line, g.label, size(g),
                         ' '.join('%s%d' % (k, v) for k, v in sorted(cls.items())),
                         ' '.join('%s:%d' % kv for kv in sorted(mix.items()))))
    return '\n'.join(lines)


def emit(src):
    """Device assembly of `src` with the flags nerfail_amd/build.py compiles it with."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, here)
    from nerfail_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'dev.s')
        cmd = ([build.HIPCC] + build.CFLAGS + build.FILE_FLAGS.get(os.path.basename(src), [])
               + ['-S', '--cuda-device-only', src, '-o', out])
        subprocess.run(cmd, check=True)
        return open(out).read()


def main(argv):
    quiet = '--quiet' in argv
    kernel = argv[argv.index('--kernel') + 1] if '--kernel' in argv else ''
    if '--emit' in argv:
        text = emit(argv[argv.index('--emit') + 1])
    else:
        files = [a for i, a in enumerate(argv) if not a.startswith('--') and (i == 0 or argv[i - 1] != '--kernel')]
        if len(files) != 1:
            print(__doc__)
            return 2
        text = open(files[0]).read()
    for name, gaps in parse(text).items():
        if kernel in name:
            print(report(name, gaps, quiet))
            print()
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
