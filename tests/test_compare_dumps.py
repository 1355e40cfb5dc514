"""CPU: tools/compare_dumps.py on two small synthetic --dump-outputs directories."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write(d, arrays):
    os.makedirs(d)
    for k, v in arrays.items():
        np.save(os.path.join(d, k + '.npy'), v)


def test_compare_dumps_reports_differences_nans_and_pts_max_moves(tmp_path):
    rs = np.random.RandomState(0)
    rgb = rs.rand(100, 3).astype(np.float32)
    disp = rs.rand(100).astype(np.float32)
    disp[7] = np.nan
    pts = rs.rand(100, 3).astype(np.float32)
    rgb2 = rgb.copy()
    rgb2[3, 1] += 1e-6
    disp2 = disp.copy()
    disp2[9] = np.nan
    pts2 = pts.copy()
    pts2[5] += np.float32(2 * 0.0625 / np.sqrt(3))                 # two sample spacings along the diagonal
    _write(str(tmp_path / 'a'), {'rgb_map': rgb, 'disp_map': disp, 'pts_max': pts})
    _write(str(tmp_path / 'b'), {'rgb_map': rgb2, 'disp_map': disp2, 'pts_max': pts2})
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'compare_dumps.py'), str(tmp_path / 'a'),
                        str(tmp_path / 'b'), '--json'], capture_output=True, text=True, check=True)
    res = json.loads(r.stdout)
    assert abs(res['rgb_map']['max_abs'] - 1e-6) < 1e-7
    assert res['rgb_map']['nan_positions_equal']
    assert not res['disp_map']['nan_positions_equal']
    p = res['pts_max']['pts_max']
    assert p['rays_differing'] == 1 and p['spacings_histogram'] == {'2': 1}
    # the table form runs too
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'compare_dumps.py'), str(tmp_path / 'a'),
                        str(tmp_path / 'a')], capture_output=True, text=True, check=True)
    assert '0 of 100 rays differ' in r.stdout
