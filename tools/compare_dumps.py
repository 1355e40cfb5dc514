"""Compare two `bench.py --dump-outputs` directories array by array.

    python tools/compare_dumps.py A B [--spacing S] [--json]

For every array present in both: max |a-b|, max relative difference (|a-b| / max(|b|, 1e-30) over the finite entries), and
whether the NaN positions are identical. For `pts_max` (the argmax sample point of every ray): how many rays differ, and
by how far, in units of one sample spacing S along the ray (default 4 / 64: the coarse spacing of the near 2 / far 6
Blender rays; fine samples lie closer, so this unit over-counts nothing).
"""
import argparse
import json
import os
import sys

import numpy as np


def compare(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if a.shape != b.shape:
        return {'shape_a': list(a.shape), 'shape_b': list(b.shape), 'same_shape': False}
    na, nb = np.isnan(a), np.isnan(b)
    ok = ~(na | nb)
    d = np.abs(a - b)[ok]
    rel = d / np.maximum(np.abs(b[ok]), 1e-30)
    return {'same_shape': True, 'n': int(a.size), 'max_abs': float(d.max()) if d.size else 0.0,
            'max_rel': float(rel.max()) if rel.size else 0.0, 'nan_positions_equal': bool(np.array_equal(na, nb)),
            'n_nan': int(na.sum())}


def compare_pts_max(a, b, spacing):
    a = np.asarray(a, np.float64).reshape(-1, 3)
    b = np.asarray(b, np.float64).reshape(-1, 3)
    dist = np.linalg.norm(a - b, axis=1)
    diff = dist > 0
    steps = np.rint(dist[diff] / spacing).astype(np.int64)
    hist = {int(k): int(v) for k, v in zip(*np.unique(steps, return_counts=True))}
    return {'rays': int(a.shape[0]), 'rays_differing': int(diff.sum()), 'fraction': float(diff.mean()),
            'max_dist': float(dist.max()) if dist.size else 0.0, 'spacings_histogram': hist}


def compare_dirs(da, db, spacing=4.0 / 64):
    names = sorted(f[:-4] for f in os.listdir(da) if f.endswith('.npy') and os.path.exists(os.path.join(db, f)))
    out = {}
    for n in names:
        a, b = np.load(os.path.join(da, n + '.npy')), np.load(os.path.join(db, n + '.npy'))
        out[n] = compare(a, b)
        if n == 'pts_max' and out[n]['same_shape']:
            out[n]['pts_max'] = compare_pts_max(a, b, spacing)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a')
    ap.add_argument('b')
    ap.add_argument('--spacing', type=float, default=4.0 / 64)
    ap.add_argument('--json', action='store_true', help='print one JSON object instead of the table')
    args = ap.parse_args(argv)
    res = compare_dirs(args.a, args.b, args.spacing)
    if args.json:
        print(json.dumps(res, sort_keys=True))
        return 0
    for n, r in res.items():
        if not r['same_shape']:
            print('%-10s shape differs: %s vs %s' % (n, r['shape_a'], r['shape_b']))
            continue
        print('%-10s max|a-b| %.3e  max rel %.3e  NaN positions %s (%d NaN)' %
              (n, r['max_abs'], r['max_rel'], 'equal' if r['nan_positions_equal'] else 'DIFFER', r['n_nan']))
        if 'pts_max' in r:
            p = r['pts_max']
            print('%-10s %d of %d rays differ (%.4f %%), max distance %.3e, in spacings: %s' %
                  ('', p['rays_differing'], p['rays'], 100 * p['fraction'], p['max_dist'], p['spacings_histogram']))
    return 0


if __name__ == '__main__':
    sys.exit(main())
