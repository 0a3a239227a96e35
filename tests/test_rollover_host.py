"""Host side of the device rollover (include/avr.h avr_rollover_*): the pool-row pick's host mirror
_lib.rollover_index, pinned by known answers from a scalar Philox4x32-10 that is itself checked
against the Random123 vector of tests/test_philox.py, its counters against the other two streams',
and the facade's reset_pool argument check (no GPU calls)."""
import inspect

import numpy as np
import pytest

from avr import _lib
from test_philox import KAT


def philox_scalar(c, k):
    """Philox4x32-10 on Python ints (an implementation independent of _lib's vectorised one)."""
    c, (k0, k1) = list(c), k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return tuple(c)


def rollover_counter(env, episode):
    return (env, episode & 0xFFFFFFFF, 0x40000000, episode >> 32)


# (seed, global env, episode) -> word 0 of the rollover stream; computed with philox_scalar
KNOWN = [
    (1001, 0, 0, 0x6d64041c), (1001, 1, 0, 0xa6c8c84d), (1001, 79, 1, 0x28adfc66), (1001, 4095, 3, 0x8bf18dc2),
    (1001, 1000, (1 << 32) + 5, 0x13384dd8), (1001, 7, 2, 0x9eddfd2d), ((0xdeadbeef << 32) | 0x12345678, 3, 1, 0x480838a6),
]


def test_scalar_philox_matches_random123():
    for ctr, key, want in KAT:
        assert philox_scalar(ctr, key) == want


def test_rollover_index_known_answers():
    for seed, env, ep, x0 in KNOWN:
        assert philox_scalar(rollover_counter(env, ep), (seed & 0xFFFFFFFF, seed >> 32))[0] == x0
        for n_pool in (1, 5, 7, 4096):
            got = _lib.rollover_index(seed, [env], [ep], n_pool)
            assert got.dtype == np.int64 and got.shape == (1,) and int(got[0]) == x0 % n_pool, (seed, env, ep, n_pool)
    # vectorised over envs with one episode per env, and with a scalar episode
    envs = np.array([k[1] for k in KNOWN[:4]])
    eps = np.array([k[2] for k in KNOWN[:4]])
    assert _lib.rollover_index(1001, envs, eps, 5).tolist() == [k[3] % 5 for k in KNOWN[:4]]
    assert _lib.rollover_index(1001, [0, 1], 0, 7).tolist() == [0x6d64041c % 7, 0xa6c8c84d % 7]
    with pytest.raises(ValueError):
        _lib.rollover_index(1001, [0], [0], 0)


def test_rollover_counters_differ_from_the_other_streams():
    """Counter word 2: random_actions uses j >> 2 (0 or 1 for j < 8), policy_noise 0x80000000 | (j >> 2),
    the rollover 0x40000000: with the same (env, t / episode) words no two of the three coincide, so the
    streams' outputs are those of distinct Philox counters."""
    for j in range(8):
        assert len({j >> 2, 0x80000000 | (j >> 2), 0x40000000}) == 3
    # ... and the mirrors really use those counters: reproduce each stream's first word by hand
    seed, env, t = 1001, 12, 9
    key = (seed & 0xFFFFFFFF, seed >> 32)
    a = _lib.random_actions(seed, [env], t)[0]
    for j in range(7):
        x = philox_scalar((env, t, j >> 2, 0), key)[j & 3]
        assert a[j] == np.float32(x >> 8) * np.float32(1.0 / 16777216.0) * np.float32(2.0) - np.float32(1.0)
    assert int(_lib.rollover_index(seed, [env], [t], 1 << 31)[0]) == philox_scalar((env, t, 0x40000000, 0), key)[0] % (1 << 31)
    for j in range(8):
        assert philox_scalar((env, t, 0x40000000, 0), key) != philox_scalar((env, t, j >> 2, 0), key)
        assert philox_scalar((env, t, 0x40000000, 0), key) != philox_scalar((env, t, 0x80000000 | (j >> 2), 0), key)


def test_rollover_index_covers_the_pool():
    envs, eps = np.repeat(np.arange(4096), 4), np.tile(np.arange(4), 4096)
    idx = _lib.rollover_index(1001, envs, eps, 7)
    assert idx.shape == (4 * 4096,) and idx.min() == 0 and idx.max() == 6
    cnt = np.bincount(idx, minlength=7)
    # 16384 draws over 7 rows: mean 2341, sd 45; every row within 6 sd
    assert np.all(cnt > 0) and np.all(np.abs(cnt - 16384 / 7) < 6 * 45)
    # an env's pick changes with its episode, and another seed gives other picks
    assert not np.array_equal(idx[0::4], idx[1::4])
    assert not np.array_equal(idx, _lib.rollover_index(1002, envs, eps, 7))


def test_facade_reset_pool_argument():
    """reset_pool is a keyword of AVRTorchVecEnv; 0 (and other non-positive or fractional values) is
    rejected before a handle is created."""
    from avr.env import AVRTorchVecEnv
    p = inspect.signature(AVRTorchVecEnv.__init__).parameters['reset_pool']
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='reset_pool'):
            AVRTorchVecEnv('FeedingJaco-v0', 4, reset_pool=bad)
