"""CPU: the host side of the PPO update across ranks (avr/ppo.py combine_reference, segments_of,
DistPPOTrainer's argument checks; avr/dist.py gather_stacked / gather_rows over gloo in one process)
and the three new exports in the binding list."""
import numpy as np
import pytest


def crafted_rows():
    """[8, 4] float32 rows whose word 0 is order sensitive under 'add in float64 in ascending order, round
    to float32 once': 1, 2^-53, 2^-53, 2^-24, 0, 0, 0, 0.
      ascending:       1 + 2^-53 is a tie in float64 and rounds to even, 1; again 1; + 2^-24 = 1 + 2^-24 exactly, a
                       tie in float32 that rounds to even: 1.0
      rows 0, 2 swapped: 2^-53 + 2^-53 = 2^-52; + 1 = 1 + 2^-52 exactly; + 2^-24 = 1 + 2^-24 + 2^-52 exactly, above
                       the float32 tie: 1 + 2^-23, the next float32 after 1.0
    Words 1..3 are ordinary numbers."""
    rows = np.random.default_rng(5).normal(0, 1, (8, 4)).astype(np.float32)
    rows[:, 0] = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -24, 0, 0, 0, 0]
    return rows


def test_combine_reference_adds_in_ascending_order_in_double():
    from avr import ppo
    rows = crafted_rows()
    g = ppo.combine_reference(rows)
    assert g.dtype == np.float32 and g.shape == (4,)
    assert g[0] == np.float32(1.0)
    # words of ordinary size: the float64 sum has no rounding of its own to speak of, so the result is the correctly
    # rounded sum (math.fsum is exact)
    import math
    for w in range(1, 4):
        assert g[w] == np.float32(math.fsum(float(x) for x in rows[:, w]))
    # not float32 accumulation: 2^-24 added to 1 in float32 is lost every time, in float64 eight of them make 2^-21
    many = np.zeros((8, 1), np.float32)
    many[:, 0] = 2.0 ** -24
    many[0, 0] = 1.0
    assert ppo.combine_reference(many)[0] == np.float32(1.0 + 7 * 2.0 ** -24)
    acc = np.float32(0)
    for k in range(8):
        acc = np.float32(acc + many[k, 0])
    assert acc == np.float32(1.0)


def test_combine_reference_rejects_a_swapped_pair():
    """The mirror is a check of the order, not only of the set of rows: with rows 0 and 2 exchanged the
    crafted word comes out one float32 ulp higher, so a combine that added in another order would not
    equal the mirror."""
    from avr import ppo
    rows = crafted_rows()
    swapped = rows.copy()
    swapped[[0, 2]] = swapped[[2, 0]]
    a, b = ppo.combine_reference(rows), ppo.combine_reference(swapped)
    assert a[0] == np.float32(1.0) and b[0] == np.nextafter(np.float32(1.0), np.float32(2.0))
    assert a.view(np.uint32)[0] + 1 == b.view(np.uint32)[0]
    assert not np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_combine_reference_entropy_term_and_shape_checks():
    from avr import ppo
    rows = np.random.default_rng(6).normal(0, 1e-2, (8, ppo.PPO_SEG_WORDS)).astype(np.float32)
    g0, g1 = ppo.combine_reference(rows), ppo.combine_reference(rows, ent_coef=0.25, act_dim=7)
    ls = slice(ppo.PW_LOGSTD, ppo.PW_LOGSTD + 7)
    assert np.array_equal(g1[ls], g0[ls] - np.float32(0.25))
    g1[ls] = g0[ls]
    assert np.array_equal(g0.view(np.uint32), g1.view(np.uint32))
    with pytest.raises(AssertionError):
        ppo.combine_reference(rows[:7])
    with pytest.raises(AssertionError):
        ppo.combine_reference(rows.astype(np.float64))


def test_segments_of():
    from avr import ppo
    assert ppo.PPO_SEGMENTS == 8 and ppo.PPO_SEG_WORDS == ppo.PW_WORDS + 8
    assert ppo.segments_of(0, 1) == list(range(8))
    assert ppo.segments_of(1, 2) == [4, 5, 6, 7] and ppo.segments_of(2, 4) == [4, 5] and ppo.segments_of(7, 8) == [7]
    for world in (1, 2, 4, 8):       # the ranks' runs, in rank order, are the segments in order
        assert sum((ppo.segments_of(r, world) for r in range(world)), []) == list(range(8))
    for world in (0, 3, 5, 6, 7, 16):
        with pytest.raises(ValueError, match='does not divide'):
            ppo.segments_of(0, world)
    with pytest.raises(ValueError, match='rank 2 outside'):
        ppo.segments_of(2, 2)


def test_dist_trainer_argument_errors(monkeypatch):
    """A world of 3 ranks and norm_reward=True are refused before the env is touched."""
    from avr import dist as D, ppo
    monkeypatch.setattr(D, 'rank_world', lambda group=None: (0, 3))
    with pytest.raises(ValueError, match='3 ranks does not divide the 8 segments'):
        ppo.DistPPOTrainer(None, None, group=object())
    monkeypatch.setattr(D, 'rank_world', lambda group=None: (1, 2))
    with pytest.raises(NotImplementedError, match='norm_reward'):
        ppo.DistPPOTrainer(None, None, group=object(), norm_reward=True)
    with pytest.raises(NotImplementedError, match='norm_reward'):
        ppo.DistPPOTrainer(None, None, norm_reward=True)


def test_pool_world_argument_errors():
    from avr.env import AVRTorchVecEnv
    with pytest.raises(ValueError, match='pool_world needs reset_pool'):
        AVRTorchVecEnv('ScratchItchPR2-v0', 2, pool_world=(0, 2, None))
    with pytest.raises(ValueError, match='rank 2 outside'):
        AVRTorchVecEnv('ScratchItchPR2-v0', 2, reset_pool=1, pool_world=(2, 2, None))


def _gather_worker(rank, world, port, q):
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'assistive-vr-gym_amd'))
    import torch
    import torch.distributed as dist
    from avr import dist as D
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    x = (1000 * rank + torch.arange(2 * 3 * 5, dtype=torch.float32)).reshape(2, 3, 5)
    g = D.gather_stacked(x, dist.group.WORLD)
    d = D.gather_stacked(torch.full((2, 3), rank + 1, dtype=torch.uint8))
    r = D.gather_rows(torch.full((2, 4), float(rank), dtype=torch.float64))
    if rank == world - 1:
        q.put((g.numpy(), g.is_contiguous(), d.numpy(), r.numpy(), D.rank_world(dist.group.WORLD)))
    dist.barrier()
    dist.destroy_process_group()


def test_gathers_put_the_ranks_in_global_env_order():
    """Two gloo ranks (spawned processes): gather_stacked turns the ranks' [n, E, ...] into [n, 2 E, ...]
    with rank 0's envs first at every step, for float32 and uint8; gather_rows stacks small rows in rank
    order; rank_world reads the group."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    g, contiguous, d, r, rw = q.get(timeout=300)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    x = np.arange(30, dtype=np.float32).reshape(2, 3, 5)
    assert g.shape == (2, 6, 5) and contiguous and np.array_equal(g[:, :3], x) and np.array_equal(g[:, 3:], x + 1000)
    assert d.dtype == np.uint8 and np.array_equal(d, np.repeat([[1, 1, 1, 2, 2, 2]], 2, 0))
    assert r.dtype == np.float64 and np.array_equal(r[:, 0], [0, 0, 1, 1]) and r.shape == (4, 4)
    assert rw == (1, 2)


def test_new_exports_are_bound():
    import os
    import re
    from conftest import ROOT
    from avr import _lib, ppo
    for n in ('avr_ppo_advstat_device', 'avr_ppo_grad_segment_device', 'avr_ppo_combine_device'):
        assert n in _lib.EXPORTS
    txt = open(os.path.join(ROOT, 'include', 'avr.h')).read()
    assert int(re.search(r'#define\s+AVR_PPO_SEGMENTS\s+(\d+)', txt).group(1)) == _lib.PPO_SEGMENTS == ppo.PPO_SEGMENTS
    m = re.search(r'#define\s+AVR_PPO_SEG_WORDS\s+\((\d+)\s*\+\s*AVR_PPO_STAT_WORDS\)', txt)
    assert int(m.group(1)) == ppo.PW_WORDS and _lib.PPO_SEG_WORDS == ppo.PPO_SEG_WORDS == ppo.PW_WORDS + _lib.PPO_STAT_WORDS
    assert int(re.search(r'#define\s+AVR_ABI_VERSION\s+(\d+)', txt).group(1)) == 6


def test_libavr_exports_the_segment_calls(libavr_path):
    import ctypes as C
    lib = C.CDLL(libavr_path)
    for n in ('avr_ppo_advstat_device', 'avr_ppo_grad_segment_device', 'avr_ppo_combine_device'):
        assert hasattr(lib, n)
