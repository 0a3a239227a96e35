"""bench.py's host side: the --dump-outputs writer and the options a plain / --full run is chosen by."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float_npy(tmp_path):
    import bench
    d = str(tmp_path / 'out' / 'run')
    arrays = {'obs': np.arange(12, dtype=np.float32).reshape(4, 3), 'done': np.array([0, 1, 0, 1], np.uint8),
              'success': np.array([0, 2, 0, 1], np.int64), 'wide': np.array([1 / 3, 2 / 3])}
    bench.dump_outputs(d, arrays)
    assert sorted(os.listdir(d)) == sorted(k + '.npy' for k in arrays)
    for k, a in arrays.items():
        b = np.load(os.path.join(d, k + '.npy'))
        assert b.dtype == (np.float64 if a.dtype == np.float64 else np.float32) and b.shape == a.shape
        np.testing.assert_array_equal(b, a)


def test_options():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], stdout=subprocess.PIPE, text=True, check=True)
    for opt in ('--gpus', '--steps', '--warmup', '--full', '--dump-outputs'):
        assert opt in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 2 and '--steps' in r.stderr
