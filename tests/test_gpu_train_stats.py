"""GPU: reward normalisation and episode statistics on the device (csrc/avr_trainstats.hip, include/avr.h
avr_reward_norm_device / avr_episode_stats_device) against their float64 / float32 mirrors
(avr/ppo.py) on small synthetic rollouts uploaded from the host, two consecutive calls per case so
that the carried state matters; eval mode, in place, determinism, the error paths, and the trainer
end to end (the one test that steps the simulator)."""
import numpy as np
import pytest

from test_gpu_ppo import dev_tensor, make_sim, policy32
from test_train_stats_host import EPS, GAMMA, SHAPES, clip_counts_ok, make_calls

pytestmark = pytest.mark.gpu


def upload(calls):
    import torch
    T = [tuple(torch.from_numpy(a.copy()).cuda() for a in call) for call in calls]
    torch.cuda.synchronize()
    return T


def carried(sim):
    """Host copies of everything the handle carries: R, (mean, var, count), the per-env rows, the row."""
    from avr import _lib
    E = sim.n
    pR, prms, penv, prow = sim.train_stats_buffers()
    sim.sync()
    d = dict(R=dev_tensor(pR, (E,), '<f8').cpu().numpy().copy(), rms=dev_tensor(prms, (3,), '<f8').cpu().numpy().copy(),
             row=dev_tensor(prow, (_lib.EPSTAT_WORDS,), '<f8').cpu().numpy().copy())
    for i, (name, ts) in enumerate(_lib.EPISODE_ENV_ROWS):
        d[name] = dev_tensor(penv + 4 * i * E, (E,), ts).cpu().numpy().copy()
    return d


@pytest.fixture(scope='module')
def handles(scene):
    """get(E): a FeedingJaco handle of E envs in the state avr_train_stats_reset leaves.  Creating a handle
    takes seconds, so the tests of this module share one per E: its first user finds the carried rows
    not yet allocated (the first call allocates and resets them), every later one resets them."""
    _, md = scene
    sims = {}

    def get(E):
        if E in sims:
            sims[E].train_stats_reset()
        else:
            sims[E] = make_sim(md, E)
        return sims[E]
    yield get
    for sim in sims.values():
        sim.close()


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ 1. reward normalisation
@pytest.mark.parametrize('E,n', SHAPES)
@pytest.mark.parametrize('clip_rew', [10.0, 0.5])
def test_reward_norm_matches_mirror(handles, E, n, clip_rew):
    """Two consecutive calls against reward_norm_reference in float64: rew_out within one float32 ulp
    everywhere and equal in at least 99 % of the entries; mean, var and R within 1e-11 * max(1, max|R|)
    -- five orders above double rounding for trees of <= 2048 terms and 74 merges, four below a
    float32 ulp, so a float accumulator fails -- and count exact.  Then, on the carried state: eval
    mode leaves R and the statistics bit for bit and scales with the frozen variance; in place equals
    out of place."""
    import torch
    from avr import ppo
    calls = make_calls(E, n)
    T = upload(calls)
    sim = handles(E)
    st = ppo.train_stats_state(E)
    out = torch.zeros(n, E, device='cuda')
    torch.cuda.synchronize()                     # (the handle's stream is not torch's: fills and copies are done before it runs)
    for c, ((rew, done, _), (t_rew, t_done, _)) in enumerate(zip(calls, T)):
        want = ppo.reward_norm_reference(rew, done, st, GAMMA, clip_rew, EPS, True)
        sim.reward_norm_device(n, GAMMA, clip_rew, EPS, True, t_rew.data_ptr(), t_done.data_ptr(), out.data_ptr())
        S = carried(sim)                         # (synchronises the handle's stream: the output is complete)
        got = out.cpu().numpy()
        tol = 1e-11 * max(1.0, float(np.abs(st['R']).max()))
        err = [abs(S['rms'][0] - st['mean']), abs(S['rms'][1] - st['var']), float(np.abs(S['R'] - st['R']).max())]
        exact = float((got == want).mean())
        print('E %d n %d clip %g call %d: |d mean| %.3g |d var| %.3g max|d R| %.3g (tol %.3g), rew_out exact in %.4f'
              % (E, n, clip_rew, c, err[0], err[1], err[2], tol, exact))
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))
        assert exact >= 0.99
        if E == 1 and clip_rew == 10.0 and c == 0:
            assert abs(float(got[0, 0])) == 10.0      # the degenerate batch variance 0: the first reward clips even at 10
        assert max(err) <= tol and S['rms'][2] == st['count']
        if clip_rew == 0.5 and E > 1:
            assert clip_counts_ok(c, int((got == np.float32(-0.5)).sum()), int((got == np.float32(0.5)).sum()), got.size)
    # eval mode on the carried state
    before = carried(sim)
    t_rew, t_done, _ = T[0]
    sim.reward_norm_device(n, GAMMA, clip_rew, EPS, False, t_rew.data_ptr(), t_done.data_ptr(), out.data_ptr())
    after = carried(sim)
    assert all(bits_equal(before[k], after[k]) for k in before)
    want = ppo.reward_norm_reference(calls[0][0], calls[0][1], st, GAMMA, clip_rew, EPS, False)
    got = out.cpu().numpy()
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))) and float((got == want).mean()) >= 0.99
    # in place equals out of place: eval mode, then update mode from the reset state
    inpl = t_rew.clone()
    torch.cuda.synchronize()
    sim.reward_norm_device(n, GAMMA, clip_rew, EPS, False, inpl.data_ptr(), t_done.data_ptr(), inpl.data_ptr())
    sim.sync()
    assert torch.equal(inpl, out)
    sim.train_stats_reset()
    sim.reward_norm_device(n, GAMMA, clip_rew, EPS, True, t_rew.data_ptr(), t_done.data_ptr(), out.data_ptr())
    Sa = carried(sim)
    sim.train_stats_reset()
    inpl = t_rew.clone()
    torch.cuda.synchronize()
    sim.reward_norm_device(n, GAMMA, clip_rew, EPS, True, inpl.data_ptr(), t_done.data_ptr(), inpl.data_ptr())
    Sb = carried(sim)
    assert torch.equal(inpl, out) and all(bits_equal(Sa[k], Sb[k]) for k in Sa)


# ------------------------------------------------------------------ 2. episode statistics
@pytest.mark.parametrize('E,n', SHAPES)
def test_episode_stats_match_mirror(handles, E, n):
    """Two consecutive calls against episode_stats_reference: the per-env float32 / int32 rows and the
    integer columns exact, ret_min / ret_max exact, the float64 sums within 1e-12 relative; the row
    the caller receives is the handle's own."""
    import torch
    from avr import _lib, ppo
    calls = make_calls(E, n)
    T = upload(calls)
    sim = handles(E)
    st = ppo.train_stats_state(E)
    d_row = torch.zeros(_lib.EPSTAT_WORDS, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    for c, ((rew, done, info), (t_rew, t_done, t_info)) in enumerate(zip(calls, T)):
        want = dict(zip(_lib.EPISODE_STATS, ppo.episode_stats_reference(rew, done, info, st)))
        sim.episode_stats_device(n, t_rew.data_ptr(), t_done.data_ptr(), t_info.data_ptr(), d_row.data_ptr() if c == 0 else None)
        S = carried(sim)
        got = dict(zip(_lib.EPISODE_STATS, S['row']))
        if c == 0:
            assert bits_equal(d_row.cpu().numpy(), S['row'])
        print('E %d n %d call %d: %s' % (E, n, c, {k: (got[k], want[k]) for k in ('episodes', 'ret_sum', 'rew_sum')}))
        for k in ('episodes', 'len_sum', 'success_sum', 'steps', 'ret_min', 'ret_max'):
            assert got[k] == want[k], k
        for k in ('ret_sum', 'ret_sumsq', 'force_mean_sum', 'rew_sum'):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
        for k, _ in _lib.EPISODE_ENV_ROWS:
            assert bits_equal(S[k], st[k]), k


def test_episode_stats_without_episodes(handles):
    """No done at all: episodes 0, ret_min +inf, ret_max -inf, steps and rew_sum still counted."""
    from avr import _lib, ppo
    E, n = 7, 5
    calls = make_calls(E, n, dones=False)
    (t_rew, t_done, t_info), = upload(calls[:1])
    sim = handles(E)
    sim.train_stats_reset()
    zero = dict(zip(_lib.EPISODE_STATS, carried(sim)['row']))
    assert zero['ret_min'] == np.inf and zero['ret_max'] == -np.inf and all(zero[k] == 0 for k in zero if k not in ('ret_min', 'ret_max'))
    sim.episode_stats_device(n, t_rew.data_ptr(), t_done.data_ptr(), t_info.data_ptr())
    S = carried(sim)
    st = ppo.train_stats_state(E)
    want = ppo.episode_stats_reference(*calls[0], st)
    got = dict(zip(_lib.EPISODE_STATS, S['row']))
    assert got['episodes'] == 0 and got['ret_min'] == np.inf and got['ret_max'] == -np.inf and got['steps'] == 35
    assert got['ret_sum'] == 0 and got['len_sum'] == 0 and abs(got['rew_sum'] - want[9]) <= 1e-12 * abs(want[9])
    assert np.all(S['ep_len'] == 5) and np.all(S['n_finished'] == 0) and bits_equal(S['ep_ret'], st['ep_ret'])


# ------------------------------------------------------------------ 3. determinism
def test_deterministic(scene):
    """The same two calls of both entry points on two fresh handles: identical bits in every output and
    every carried row ((65, 37): several blocks of the scans, strided reduction threads idle)."""
    import torch
    _, md = scene
    E, n = 65, 37
    T = upload(make_calls(E, n))
    res = []
    for _ in range(2):
        sim = make_sim(md, E)
        outs = []
        for t_rew, t_done, t_info in T:
            o = torch.zeros(n, E, device='cuda')
            torch.cuda.synchronize()
            sim.reward_norm_device(n, GAMMA, 0.5, EPS, True, t_rew.data_ptr(), t_done.data_ptr(), o.data_ptr())
            sim.episode_stats_device(n, t_rew.data_ptr(), t_done.data_ptr(), t_info.data_ptr())
            S = carried(sim)
            outs += [o.cpu().numpy()] + [S[k] for k in sorted(S)]
        res.append(outs)
        sim.close()
    assert len(res[0]) == len(res[1]) and all(bits_equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------ 4. error paths
def test_errors(handles):
    import torch
    from avr import _abi as ABI, reset_dressing as RD
    E, n = 7, 5
    (t_rew, t_done, t_info), = upload(make_calls(E, n)[:1])
    out = torch.zeros(n, E, device='cuda')
    torch.cuda.synchronize()
    sim = handles(E)
    r, d, i, o = t_rew.data_ptr(), t_done.data_ptr(), t_info.data_ptr(), out.data_ptr()
    with pytest.raises(RuntimeError, match='n 0 < 1'):
        sim.reward_norm_device(0, GAMMA, 10.0, EPS, True, r, d, o)
    with pytest.raises(RuntimeError, match='n 0 < 1'):
        sim.episode_stats_device(0, r, d, i)
    for args in ((None, d, o), (r, None, o), (r, d, None)):
        with pytest.raises(RuntimeError, match='must be given'):
            sim.reward_norm_device(n, GAMMA, 10.0, EPS, True, *args)
    for args in ((None, d, i), (r, None, i), (r, d, None)):
        with pytest.raises(RuntimeError, match='must be given'):
            sim.episode_stats_device(n, *args)
    for g in (-0.01, 1.01, float('nan')):
        with pytest.raises(RuntimeError, match=r'outside \[0, 1\]'):
            sim.reward_norm_device(n, g, 10.0, EPS, True, r, d, o)
    for e in (0.0, -1e-8):
        with pytest.raises(RuntimeError, match='eps .* must be > 0'):
            sim.reward_norm_device(n, GAMMA, 10.0, e, True, r, d, o)
    with pytest.raises(RuntimeError, match='clip_rew'):
        sim.reward_norm_device(n, GAMMA, -1.0, EPS, True, r, d, o)
    sim.reward_norm_device(n, 0.0, 10.0, EPS, True, r, d, o)          # (the ends of the range are fine)
    sim.reward_norm_device(n, 1.0, 10.0, EPS, True, r, d, o)
    assert sim.lib.avr_train_stats_buffers(sim.h, None, None, None, None) == 0
    sim.sync()
    dr = make_sim(ABI.ModelDesc(RD.dressing_scene()), 2)
    for rc in (dr.lib.avr_reward_norm_device(dr.h, 1, 0.99, 10.0, 1e-8, 1, None, None, None),
               dr.lib.avr_episode_stats_device(dr.h, 1, None, None, None, None), dr.lib.avr_train_stats_reset(dr.h),
               dr.lib.avr_train_stats_buffers(dr.h, None, None, None, None)):
        assert rc == -1 and b'not built for DressingJaco' in dr.lib.avr_last_error(dr.h)
    dr.close()


# ------------------------------------------------------------------ 5. the trainer
def test_trainer_end_to_end():
    """ScratchItchPR2, 16 envs from a one-state pool, 128-step rollouts, norm_reward on, two iterate()
    calls.  The TimeLimit is 200, so every env finishes exactly once, in the second rollout: the first
    'episodes' row has no episode, the second 16 of them with len_sum 3200 and the returns of the mirror
    run over the two cloned rollouts; rew_norm is the mirror's under the kernel test's rule, and adv is
    gae_reference of the device's own rew_norm bit for bit.  With both options off a second trainer
    trains on compute_gae(out) and returns no 'episodes'."""
    import copy
    import torch
    from avr import _lib, ppo
    from avr.env import AVRTorchVecEnv
    pol, rms = policy32(30, 48, seed=71)
    hyper = dict(lr=1e-4, epochs=1, n_minibatch=2, update_ob_rms=False)
    env = AVRTorchVecEnv('ScratchItchPR2-v0', 16, reset_pool=1)
    env.reset()
    tr = ppo.PPOTrainer(env, copy.deepcopy(pol), copy.deepcopy(rms), n_steps=128, generator=torch.Generator(device='cuda').manual_seed(3),
                        norm_reward=True, **hyper)
    st = ppo.train_stats_state(16)
    rows = []
    for it in range(2):
        r = tr.iterate()
        torch.cuda.synchronize()
        o = {k: tr.last['out'][k].cpu().numpy().copy() for k in ('rew', 'done', 'info', 'value')}
        row = dict(zip(_lib.EPISODE_STATS, r['episodes'].cpu().numpy()))
        want_row = dict(zip(_lib.EPISODE_STATS, ppo.episode_stats_reference(o['rew'], o['done'], o['info'], st)))
        want_norm = ppo.reward_norm_reference(o['rew'], o['done'], st, tr.hyper['gamma'], tr.hyper['clip_reward'], ppo.RET_EPS, True)
        got_norm = tr.last['rew_norm'].cpu().numpy()
        assert np.all(np.abs(got_norm - want_norm) <= np.spacing(np.abs(want_norm))) and float((got_norm == want_norm).mean()) >= 0.99
        tv = tr.last['out']['term_value'].cpu().numpy()
        adv, ret = ppo.gae_reference(got_norm, o['done'], o['value'], tv, tr.hyper['gamma'], tr.hyper['lam'], tr.hyper['bootstrap'])
        assert np.array_equal(tr.last['adv'].cpu().numpy(), adv) and np.array_equal(tr.last['ret'].cpu().numpy(), ret)
        assert row['steps'] == 128 * 16 and abs(row['rew_sum'] - want_row['rew_sum']) <= 1e-12 * abs(want_row['rew_sum'])
        for k in ('episodes', 'len_sum', 'success_sum', 'ret_min', 'ret_max'):
            assert row[k] == want_row[k], k
        for k in ('ret_sum', 'ret_sumsq', 'force_mean_sum'):
            assert abs(row[k] - want_row[k]) <= 1e-12 * abs(want_row[k]), k
        rows.append((r['episodes'], row))
        assert bool(torch.isfinite(r['stats']).all())
    assert rows[0][1]['episodes'] == 0 and rows[0][1]['ret_min'] == np.inf
    assert rows[1][1]['episodes'] == 16 and rows[1][1]['len_sum'] == 3200
    penv = env.sim.train_stats_buffers()[2]
    last_ret = dev_tensor(penv + 4 * 3 * 16, (16,)).cpu().numpy()
    assert np.array_equal(last_ret, st['last_ret']) and np.all(st['last_len'] == 200) and np.all(st['n_finished'] == 1)
    s0, s1 = ppo.PPOTrainer.episode_summary(rows[0][0]), ppo.PPOTrainer.episode_summary(rows[1][0])
    assert s0['episodes'] == 0 and all(v is None for k, v in s0.items() if k != 'episodes')
    assert set(s1) == {'episodes', 'return_mean', 'return_std', 'return_min', 'return_max', 'length_mean', 'success_rate', 'force_mean'}
    assert s1['episodes'] == 16 and s1['length_mean'] == 200.0 and s1['return_min'] <= s1['return_mean'] <= s1['return_max']
    assert abs(s1['return_mean'] - float(st['last_ret'].astype(np.float64).mean())) <= 1e-12 * abs(s1['return_mean'])
    assert 0.0 <= s1['success_rate'] <= 1.0 and s1['force_mean'] >= 0.0 and s1['return_std'] >= 0.0
    env.close()
    # both options off: today's trainer
    env = AVRTorchVecEnv('ScratchItchPR2-v0', 16, reset_pool=1)
    env.reset()
    tr = ppo.PPOTrainer(env, copy.deepcopy(pol), copy.deepcopy(rms), n_steps=128, generator=torch.Generator(device='cuda').manual_seed(3),
                        norm_reward=False, episode_stats=False, **hyper)
    r = tr.iterate()
    adv = tr.last['adv'].clone()
    a2, _ = env.compute_gae(tr.last['out'], tr.hyper['gamma'], tr.hyper['lam'], tr.hyper['bootstrap'])
    torch.cuda.synchronize()
    assert 'episodes' not in r and tr.last['rew_norm'] is None and torch.equal(a2, adv)
    env.close()
