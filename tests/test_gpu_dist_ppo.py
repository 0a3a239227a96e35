"""PPO training across ranks on the HIP backend: two ranks (torch.distributed.run, gloo) share the one
GPU, each a fresh child process with 8 ScratchItchPR2 envs of the 16 global ones, and run two
DistPPOTrainer iterations of 16-step rollouts, 2 epochs x 2 minibatches (N = 256, segments of 16
samples; tests/gpu_dist_ppo_worker.py).  One process runs DistPPOTrainer(group=None) on all 16 envs
from the same explicit reset states.  Weights, Adam's moments and the gathered rollouts must be equal,
bit for bit: the rollouts because env ids, action noise and rollover indices are keyed by the global env
id and the pool rows are shared, the update because every rank combines the same eight segment rows in
the same order."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


@pytest.mark.gpu
def test_two_ranks_train_the_same_weights_as_one_process(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import gpu_dist_ppo_worker as W
    E = 8
    out = str(tmp_path / 'ranks')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', OMP_NUM_THREADS='4')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
           '--master-port', str(_free_port()), os.path.join(ROOT, 'tests', 'gpu_dist_ppo_worker.py'), '--out', out, '--envs', str(E)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
    assert r.returncode == 0, r.stdout[-4000:]
    ranks = [np.load('%s.%d.npz' % (out, k)) for k in range(2)]
    assert all(int(z['world']) == 2 for z in ranks)

    md, table = W.state_table(2 * E)
    one = W.train(table, 0, 1, None, 2 * E)

    steps = W.ITERATIONS * W.N_STEPS
    assert one['obs'].shape == (steps, 2 * E, 30) and one['w'].shape == (13144,)
    assert np.all(np.isfinite(one['w'])) and np.abs(one['m']).max() > 0 and np.all(one['v'] >= 0)
    # live data: rewards vary, envs finished inside the second rollout (at staggered steps) and went on from pool rows
    done = one['done'][W.N_STEPS:]
    assert one['rew'].std() > 0 and not one['done'][:W.N_STEPS].any()
    assert done.sum() == 2 * E and len(set(np.argmax(done, 0).tolist())) == 5
    for name in ('w', 'm', 'v'):
        a, b = ranks[0][name], ranks[1][name]
        assert np.array_equal(_bits(a), _bits(b)), 'ranks differ in %s' % name
        bad = np.argwhere(_bits(a) != _bits(one[name]))
        assert bad.size == 0, '%s: two ranks differ from one process, first words %s' % (name, bad[:5].ravel().tolist())
    for name in W.ROLLOUT_KEYS:
        for k in range(2):
            got = ranks[k][name]
            assert got.shape == one[name].shape and got.dtype == one[name].dtype, name
            bad = np.argwhere(_bits(got) != _bits(one[name]))
            assert bad.size == 0, '%s of rank %d: first mismatches (step, env, ...) %s' % (name, k, bad[:5].tolist())
    for k in range(2):
        assert np.array_equal(_bits(ranks[k]['stats']), _bits(one['stats']))
        # (the episode rows add per-rank sums: equal counts, extrema and steps; the sums to rounding)
        assert np.array_equal(ranks[k]['episodes'][[0, 3, 4, 5]], one['episodes'][[0, 3, 4, 5]])
        assert np.allclose(ranks[k]['episodes'], one['episodes'], rtol=1e-9, atol=1e-9)
