"""CPU: the readable mirrors of the device reward normalisation and episode statistics (avr/ppo.py
reward_norm_reference / episode_stats_reference) against a literal per-step VecNormalize loop and
plain per-env Python accumulators, over two consecutive calls per shape; the new exports in the
binding list.  tests/test_gpu_train_stats.py holds the kernels to the same mirrors on these inputs."""
import math

import numpy as np
import pytest

RED = 256                                    # csrc/avr_trainstats.hip TS_RED_THREADS (checked against _lib below)
SHAPES = [(1, 5), (7, 37), (65, 37), (RED + 6, 5), (1030, 5)]      # (E, n)
GAMMA, EPS = 0.99, 1e-8


def make_calls(E, n, seed=0, n_calls=2, dones=True):
    """n_calls consecutive rollouts' (rew [n, E] float32, done [n, E] uint8, info [n, E, 2] float32).
    rew = 0.3 N(0, 1) - 0.1; info = {a force in [0, 5), a 0 / 1 success}.  done: 10 % of the entries at
    random, then per call c (E >= 7): env 0 done at k = 0, env 2 at k = n-1, env 4 at k = 1 and k = n-1
    (two in one call), env 1 + 4 c none at all, and env 1 done at k = n / 2 of every later call -- so env
    1's first episode spans the calls' boundary.
    E = 1: two dones (k = 0, k = n-1) in call 0, none in call 1.  Read-only arrays."""
    rng = np.random.default_rng([seed, E, n])
    calls = []
    for c in range(n_calls):
        rew = (0.3 * rng.standard_normal((n, E)) - 0.1).astype(np.float32)
        done = (rng.random((n, E)) < 0.1).astype(np.uint8)
        info = np.stack([5.0 * rng.random((n, E)), rng.integers(0, 2, (n, E))], -1).astype(np.float32)
        if not dones:
            done[:] = 0
        elif E == 1:
            done[:] = 0
            if c == 0:
                done[0, 0] = done[n - 1, 0] = 1
        else:
            assert E >= 7 and n >= 5
            done[0, 0] = 1
            done[n - 1, 2] = 1
            done[:, 4] = 0
            done[1, 4] = done[n - 1, 4] = 1
            done[:, 1 + 4 * c] = 0
            if c > 0:
                done[n // 2, 1] = 1
        for a in (rew, done, info):
            a.setflags(write=False)
        calls.append((rew, done, info))
    return calls


def vecnormalize_loop(calls, E, gamma, clip_rew, eps):
    """baselines' VecNormalize reward path, step by step: per call (rew_out float32, (mean, var, count), R)."""
    from avr import policy_eval as PE
    rms, R, res = PE.RunningMeanStd(()), np.zeros(E), []
    for rew, done, _ in calls:
        out = np.zeros(rew.shape, np.float32)
        for k in range(rew.shape[0]):
            r = rew[k].astype(np.float64)
            R = R * gamma + r
            rms.update(R)
            out[k] = np.clip(r / np.sqrt(rms.var + eps), -clip_rew, clip_rew)
            R[done[k] != 0] = 0.0
        res.append((out, (float(rms.mean), float(rms.var), float(rms.count)), R.copy()))
    return res


def episode_loop(calls, E):
    """Plain per-env accumulators: per call (the closed episodes [(e, ret, len, success, mean force)] in
    (k, e) order, the sum of all rewards, copies of the per-env running (ret, len, force))."""
    ep_ret, ep_len, ep_force = [np.float32(0)] * E, [0] * E, [np.float32(0)] * E
    res = []
    for rew, done, info in calls:
        closed, rs = [], []
        for k in range(rew.shape[0]):
            for e in range(E):
                ep_ret[e] = np.float32(ep_ret[e] + rew[k, e])
                ep_force[e] = np.float32(ep_force[e] + info[k, e, 0])
                ep_len[e] += 1
                rs.append(float(rew[k, e]))
                if done[k, e]:
                    closed.append((e, ep_ret[e], ep_len[e], float(info[k, e, 1]), float(ep_force[e]) / ep_len[e]))
                    ep_ret[e], ep_len[e], ep_force[e] = np.float32(0), 0, np.float32(0)
        res.append((closed, math.fsum(rs), (np.array(ep_ret, np.float32), np.array(ep_len, np.int32), np.array(ep_force, np.float32))))
    return res


def close(a, b, rel=1e-12):
    return abs(a - b) <= rel * abs(b)


def clip_counts_ok(call, lo, hi, size):
    """clip_rew = 0.5 must clip on both sides: at least 5 % of the n * E entries of a case's first call sit
    on each bound (from fresh statistics the variance of the discounted return starts small, so the
    first steps clip most: 37 and 20 of 259 at (7, 37), 511 and 173 of 2405 at (65, 37), 1896 and 763 of
    5150 at (1030, 5)); the carried call, whose variance has settled (8 and 3 of 259 at (7, 37)), must
    still reach each bound."""
    return (lo >= 0.05 * size and hi >= 0.05 * size) if call == 0 else (lo >= 1 and hi >= 1)


@pytest.mark.parametrize('E,n', SHAPES)
@pytest.mark.parametrize('clip_rew', [10.0, 0.5])
def test_reward_norm_reference_matches_vecnormalize_loop(E, n, clip_rew):
    """Two consecutive calls: the statistics agree to 1e-12 relative (both are float64; they differ in
    the grouping of the phases, not in the expressions), the outputs to one float32 ulp; with
    clip_rew = 0.5 and E > 1 at least 5 % of the entries sit on each bound."""
    from avr import ppo
    calls = make_calls(E, n)
    want = vecnormalize_loop(calls, E, GAMMA, clip_rew, EPS)
    st = ppo.train_stats_state(E)
    assert (st['mean'], st['var'], st['count']) == (0.0, 1.0, 1e-4)
    for c, ((rew, done, _), (out_w, rms_w, R_w)) in enumerate(zip(calls, want)):
        out = ppo.reward_norm_reference(rew, done, st, GAMMA, clip_rew, EPS, True)
        assert out.dtype == np.float32 and out.shape == (n, E)
        assert np.all(np.abs(out - out_w) <= np.spacing(np.abs(out_w)))
        assert close(st['mean'], rms_w[0]) and close(st['var'], rms_w[1]) and st['count'] == rms_w[2]
        assert np.all(np.abs(st['R'] - R_w) <= 1e-12 * np.abs(R_w))
        if clip_rew == 0.5 and E > 1:
            lo, hi = int((out == np.float32(-0.5)).sum()), int((out == np.float32(0.5)).sum())
            print('E %d n %d: %d of %d at the lower bound, %d at the upper' % (E, n, lo, out.size, hi))
            assert clip_counts_ok(c, lo, hi, out.size)
    if E == 1 and clip_rew == 10.0:
        # the degenerate case: one env's batch variance is 0, the first reward is divided by about sqrt(1e-8)
        assert abs(ppo.reward_norm_reference(calls[0][0], calls[0][1], ppo.train_stats_state(1), GAMMA, 10.0, EPS, True)[0, 0]) == 10.0
    # eval mode: the state is only read, every step uses the frozen variance
    keep = {k: np.copy(v) for k, v in st.items()}
    rew, done, _ = calls[0]
    out = ppo.reward_norm_reference(rew, done, st, GAMMA, clip_rew, EPS, False)
    assert all(np.array_equal(st[k], keep[k]) for k in keep)
    assert np.array_equal(out, np.clip(rew.astype(np.float64) / np.sqrt(st['var'] + EPS), -clip_rew, clip_rew).astype(np.float32))


@pytest.mark.parametrize('E,n', SHAPES)
def test_episode_stats_reference_matches_accumulators(E, n):
    """Two consecutive calls: counts, lengths, the float32 returns, ret_min / ret_max and the per-env
    rows are exact; the float64 sums agree to 1e-12 relative with math.fsum of the same terms."""
    from avr import _lib, ppo
    calls = make_calls(E, n)
    want = episode_loop(calls, E)
    st = ppo.train_stats_state(E)
    finished, last = np.zeros(E, np.int32), {}
    for c, ((rew, done, info), (closed, rew_sum, (ep_ret, ep_len, ep_force))) in enumerate(zip(calls, want)):
        row = dict(zip(_lib.EPISODE_STATS, ppo.episode_stats_reference(rew, done, info, st)))
        rets = [float(x[1]) for x in closed]
        assert closed or (E == 1 and c == 1)         # (every call closes episodes but E = 1's second)
        assert row['episodes'] == len(closed) and row['len_sum'] == sum(x[2] for x in closed) and row['steps'] == n * E
        assert row['success_sum'] == sum(x[3] for x in closed)
        assert close(row['ret_sum'], math.fsum(rets)) and close(row['ret_sumsq'], math.fsum(r * r for r in rets))
        assert close(row['force_mean_sum'], math.fsum(x[4] for x in closed)) and close(row['rew_sum'], rew_sum)
        if closed:
            assert row['ret_min'] == min(rets) and row['ret_max'] == max(rets)
        else:
            assert row['ret_min'] == np.inf and row['ret_max'] == -np.inf
        assert np.array_equal(st['ep_ret'], ep_ret) and np.array_equal(st['ep_len'], ep_len) and np.array_equal(st['ep_force'], ep_force)
        assert st['ep_ret'].dtype == np.float32 and st['ep_len'].dtype == np.int32
        for e, ret, ln, succ, _ in closed:           # (in (k, e) order: the last one of an env stays)
            finished[e] += 1
            last[e] = (ret, ln, succ)
        for e, (ret, ln, succ) in last.items():
            assert st['last_ret'][e] == ret and st['last_len'][e] == ln and st['last_success'][e] == succ
        assert np.array_equal(st['n_finished'], finished)
    if E > 1:
        # the forced cases are there: an episode of env 1 spans the boundary (longer than what call 1 saw of it)
        d1 = calls[1][1][:, 1]
        assert d1.any() and st['n_finished'][1] >= 1 and calls[0][1][:, 1].sum() == 0
        first = int(np.argmax(d1))
        assert any(x[0] == 1 and x[2] == n + first + 1 for x in want[1][0])
        assert calls[0][1][:, 4].sum() == 2 and calls[0][1][:, 1].sum() == 0 and calls[0][1][0, 0] and calls[0][1][n - 1, 2]


def test_no_episode_row():
    from avr import _lib, ppo
    rew, done, info = make_calls(7, 5, dones=False)[0]
    st = ppo.train_stats_state(7)
    row = dict(zip(_lib.EPISODE_STATS, ppo.episode_stats_reference(rew, done, info, st)))
    assert row['episodes'] == 0 and row['ret_min'] == np.inf and row['ret_max'] == -np.inf and row['steps'] == 35
    assert row['ret_sum'] == 0 and row['len_sum'] == 0 and np.all(st['ep_len'] == 5) and np.all(st['n_finished'] == 0)


def test_binding_lists():
    from avr import _lib, ppo
    for name in ('avr_reward_norm_device', 'avr_episode_stats_device', 'avr_train_stats_reset', 'avr_train_stats_buffers'):
        assert name in _lib.EXPORTS
    assert _lib.TS_RED_THREADS == RED and _lib.EPSTAT_WORDS == len(_lib.EPISODE_STATS) == 10
    assert [k for k, _ in _lib.EPISODE_ENV_ROWS] == ['ep_ret', 'ep_len', 'ep_force', 'last_ret', 'last_len', 'last_success', 'n_finished']
    assert ppo.DEFAULTS['norm_reward'] is False and ppo.DEFAULTS['clip_reward'] == 10.0 and ppo.DEFAULTS['episode_stats'] is True
