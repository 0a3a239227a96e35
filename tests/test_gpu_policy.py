"""GPU: the policy on the device (csrc/avr_policy.hip, include/avr.h avr_policy_*): the forward
against a float64 reference, the sampling noise against its host mirror, policy rollouts bit for
bit against the loop of single calls in both replay forms, weight swaps without re-capture, the
error paths and the torch facade."""
import numpy as np
import pytest

from test_policy_host import random_policy, reference_forward

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def feeding(scene):
    """(A, md, 16 FeedingJaco reset states) shared by the tests of this module; never modified."""
    from avr import _lib, reset as RS
    _lib.load()
    A, md = scene
    S, _ = RS.batch_reset_states_fast(A, md, 1001, list(range(16)), impairment='random')
    S = S.astype(np.float32)
    S.setflags(write=False)
    return A, md, S


@pytest.fixture(scope='module')
def policy25():
    from avr import policy_eval as PE
    pol, rms = random_policy(25, 7, 64, seed=0)
    return pol, rms, PE.policy_desc(pol, rms, 25, 7)


def make_sim(md, n, **kw):
    from avr import _lib
    return _lib.Sim(md, n, **kw)


def forward(sim, t, obs, deterministic):
    """policy_act_device on a host observation array -> (action, logp, value) host arrays."""
    import torch
    o = torch.from_numpy(np.ascontiguousarray(obs, np.float32)).cuda()
    a, lp, v = torch.zeros(sim.n, sim.act_dim, device='cuda'), torch.zeros(sim.n, device='cuda'), torch.zeros(sim.n, device='cuda')
    torch.cuda.synchronize()
    sim.policy_act_device(t, o.data_ptr(), deterministic, a.data_ptr(), lp.data_ptr(), v.data_ptr())
    sim.sync()
    return a.cpu().numpy(), lp.cpu().numpy(), v.cpu().numpy()


def test_forward_matches_float64_reference(feeding, policy25):
    """70 envs (tail lanes of the last wavefront live), normalised components beyond the clip.
    Tolerance per quantity: 8 x the error of torch's own CPU fp32 ActorCritic.act against the
    float64 evaluation of the same weights over the batch (another, equally valid, summation order
    and libm).  On an MI355X: mean 1.9e-6 (bound 1.4e-5), value 8.1e-7 (4.9e-6), logp 2.9e-7 (2.3e-6)."""
    import torch
    from avr import policy_eval as PE
    A, md, _ = feeding
    pol, rms, d = policy25
    n = 70
    rng = np.random.default_rng(1)
    obs = (rms.mean + np.sqrt(rms.var) * rng.normal(0, 2, (n, 25))).astype(np.float32)
    obs[::3, 4] += 40.0                       # beyond +clip after normalisation
    obs[1::5, 17] -= 55.0                     # beyond -clip
    x64 = (obs.astype(np.float64) - d['ob_mean']) / np.sqrt(d['ob_var'].astype(np.float64) + d['eps'])
    assert (x64 > 10).any() and (x64 < -10).any()
    ref = reference_forward(d, obs)
    with torch.no_grad():
        v, a, lp, _ = pol.float().cpu().act(PE.normalize(torch.from_numpy(obs), rms), None, None, deterministic=True)
    t32 = (a.numpy(), v.numpy()[:, 0], lp.numpy()[:, 0])
    sim = make_sim(md, n)
    sim.policy_set(d)
    a_g, lp_g, v_g = forward(sim, 0, obs, True)
    sim.close()
    for name, g, t, r in zip(('mean', 'value', 'logp'), (a_g, v_g, lp_g), t32, ref):
        bound = 8 * float(np.abs(t - r).max())
        err = float(np.abs(g - r).max())
        print('forward %s: bound %.3g observed %.3g' % (name, bound, err))
        assert np.all(np.isfinite(g)) and err <= bound, (name, err, bound)


def test_forward_without_ob_rms_and_critic(feeding):
    """No ob_rms: the observation goes in as it is; no critic: the value is 0.  A 40-unit policy
    (zero-padded to the kernel's 64), same tolerance rule as above."""
    import torch
    from avr import policy_eval as PE
    A, md, _ = feeding
    pol, _ = random_policy(25, 7, 40, seed=11)
    d = PE.policy_desc(pol, None, 25, 7)
    n = 70
    obs = np.random.default_rng(12).normal(0, 1.5, (n, 25)).astype(np.float32)
    ref_mean, _, ref_lp = reference_forward(d, obs)
    with torch.no_grad():
        _, a, lp, _ = pol.act(torch.from_numpy(obs), None, None, deterministic=True)
    sim = make_sim(md, n)
    sim.policy_set(dict(d, c_w1=None, c_b1=None, c_w2=None, c_b2=None, c_w3=None, c_b3=None))
    a_g, lp_g, v_g = forward(sim, 0, obs, True)
    sim.close()
    for name, g, t, r in (('mean', a_g, a.numpy(), ref_mean), ('logp', lp_g, lp.numpy()[:, 0], ref_lp)):
        bound, err = 8 * float(np.abs(t - r).max()), float(np.abs(g - r).max())
        print('forward (no ob_rms, no critic) %s: bound %.3g observed %.3g' % (name, bound, err))
        assert err <= bound, (name, err, bound)
    assert np.all(v_g == 0)


@pytest.mark.parametrize('env_offset', [0, 1000])
def test_noise_matches_host_mirror(feeding, policy25, env_offset):
    """(action - mean) / std == policy_noise(seed, env_offset + env, t) within 1e-5: r = sqrt(-2 ln u1)
    <= 5.8 for u1 >= 2^-25; fp32 rounding of the 2 pi u2 argument and of r cos gives ~4e-6.  The
    log-prob is that of the eps drawn: per env within 1e-5 sum|eps| (eps's bound through
    d(eps^2 / 2) = |eps| d eps) + 1e-5 (fp32 rounding of a sum of magnitude < 100)."""
    from avr import _lib
    A, md, _ = feeding
    pol, rms, d = policy25
    n = 70
    obs = (rms.mean + np.sqrt(rms.var) * np.random.default_rng(2).normal(0, 1, (n, 25))).astype(np.float32)
    sim = make_sim(md, n, env_offset=env_offset, seed=1001)
    sim.policy_set(d)
    mean, lp_det, _ = forward(sim, 0, obs, True)
    std = np.exp(d['logstd'].astype(np.float64))
    for t in (0, (1 << 32) + 7):
        act, lp, _ = forward(sim, t, obs, False)
        eps = (act.astype(np.float64) - mean) / std
        ref = _lib.policy_noise(1001, env_offset + np.arange(n), t, 7)
        err = float(np.abs(eps - ref).max())
        print('noise env_offset %d t %d: max |eps - mirror| %.3g' % (env_offset, t, err))
        assert err <= 1e-5
        lp_ref = np.sum(-0.5 * ref ** 2 - d['logstd'].astype(np.float64) - 0.5 * np.log(2 * np.pi), axis=1)
        assert np.all(np.abs(lp - lp_ref) <= 1e-5 * np.abs(ref).sum(1) + 1e-5)
    assert not np.array_equal(forward(sim, 1, obs, False)[0], forward(sim, 2, obs, False)[0])
    sim.close()


def _stacked(n_envs, K, obs_dim):
    import torch
    from avr import _abi as ABI
    z = lambda *s, **kw: torch.zeros(*s, device='cuda', **kw)
    return dict(obs=z(K + 1, n_envs, obs_dim), act=z(K, n_envs, 7), logp=z(K, n_envs), value=z(K + 1, n_envs), rew=z(K, n_envs),
                done=z(K, n_envs, dtype=torch.uint8), info=z(K, n_envs, ABI.INFO_DIM))


def _rollout(sim, t0, K, obs0, det, B):
    sim.rollout_policy_device(t0, K, None if obs0 is None else obs0.data_ptr(), det, B['obs'].data_ptr(), B['act'].data_ptr(), B['logp'].data_ptr(),
                              B['value'].data_ptr(), B['rew'].data_ptr(), B['done'].data_ptr(), B['info'].data_ptr())


def _loop(sim, t0, K, obs0, det, B):
    """the K x {policy_act_device; step_device} loop into the same stacked layout"""
    B['obs'][0].copy_(obs0)
    import torch
    torch.cuda.synchronize()
    for k in range(K):
        sim.policy_act_device(t0 + k, B['obs'][k].data_ptr(), det, B['act'][k].data_ptr(), B['logp'][k].data_ptr(), B['value'][k].data_ptr())
        sim.step_device(B['act'][k].data_ptr(), B['obs'][k + 1].data_ptr(), B['rew'][k].data_ptr(), B['done'][k].data_ptr(), B['info'][k].data_ptr())
    sim.policy_act_device(t0 + K, B['obs'][K].data_ptr(), det, None, None, B['value'][K].data_ptr())
    sim.sync()


def _check_rollout_identity(md, S, desc, groups, K=19, t0=5):
    """rollout_policy_device on one handle == the loop of single calls on a second one, bit for bit,
    in the state and all seven stacked outputs; once deterministic with obs0 passed in, once
    stochastic from the handle's own observation buffer."""
    import torch
    n = len(S)
    sims = [make_sim(md, n) for _ in range(2)]
    assert all(s.env_groups() == groups for s in sims)
    for det in (True, False):
        obs0 = None
        for s in sims:
            s.set_state(S)
            obs0 = s.settle(2)                 # (leaves the settle observation in the handle's buffer)
            s.policy_set(desc)
        obs0 = torch.from_numpy(obs0).cuda()
        Ba, Bb = _stacked(n, K, md.layout.OBS_DIM), _stacked(n, K, md.layout.OBS_DIM)
        torch.cuda.synchronize()
        c0 = sims[0].graph_captures()
        _rollout(sims[0], t0, K, obs0 if det else None, det, Ba)
        sims[0].sync()
        assert sims[0].graph_captures() == c0 + 1          # (the graph path ran, not the direct loop)
        _loop(sims[1], t0, K, obs0, det, Bb)
        torch.cuda.synchronize()
        assert np.array_equal(sims[0].get_state(), sims[1].get_state())
        for k in Ba:
            assert torch.equal(Ba[k], Bb[k]), (k, det)
        assert torch.equal(Ba['obs'][0], obs0)
        assert bool(torch.isfinite(Ba['act']).all()) and float(Ba['act'].abs().max()) > 0
        if not det:
            assert not torch.equal(Ba['act'][0], Ba['act'][1])
        # a second rollout on the same buffers continues from the handle's observation: same graphs
        c1 = sims[0].graph_captures()
        _rollout(sims[0], t0 + K, 3, None, det, Ba)
        sims[0].sync()
        assert sims[0].graph_captures() == c1
        assert torch.equal(Ba['obs'][0], Bb['obs'][K])
    for s in sims:
        s.close()


@pytest.mark.parametrize('mode', ['groups', 'branches'])
def test_rollout_equals_single_call_loop_feeding(feeding, policy25, mode, monkeypatch):
    """FeedingJaco, 80 envs in 3 groups (32 / 32 / 16: a ragged last group), 19 steps (a 16-step
    chunk plus remainder graphs), per-group graphs (the task's default) and branches."""
    monkeypatch.setenv('AVR_ENV_GROUPS', '3')
    monkeypatch.setenv('AVR_ROLLOUT', mode)
    A, md, S = feeding
    _check_rollout_identity(md, np.tile(S, (5, 1)), policy25[2], 3)


def test_rollout_equals_single_call_loop_pr2(monkeypatch):
    """ScratchItchPR2 (obs 30; branches by default), 64 envs in 2 groups."""
    import scratch_util as SU
    from avr import policy_eval as PE
    monkeypatch.setenv('AVR_ENV_GROUPS', '2')
    monkeypatch.delenv('AVR_ROLLOUT', raising=False)
    A, md = SU.scene()
    S, _ = SU.reset_states(A, md, range(8))
    pol, rms = random_policy(30, 7, 48, seed=5)
    _check_rollout_identity(md, np.tile(S.astype(np.float32), (8, 1)), PE.policy_desc(pol, rms, 30, 7), 2)


@pytest.mark.parametrize('env', [{'AVR_ENV_GROUPS': '1'}, {'AVR_ENV_GROUPS': '2', 'AVR_GRAPH': '0'}], ids=['one-group', 'no-graph'])
def test_direct_loop_fallback(feeding, policy25, monkeypatch, env):
    """One env group, or AVR_GRAPH=0: the rollout falls back to the direct loop (no rollout graph is
    captured) and equals the loop of single calls from the same state."""
    import torch
    A, md, S = feeding
    for k in ('AVR_ENV_GROUPS', 'AVR_GRAPH'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, K = 64, 4
    sim = make_sim(md, n)
    sim.policy_set(policy25[2])
    outs = []
    for run in (_rollout, _loop):
        sim.set_state(np.tile(S, (4, 1)))
        obs0 = torch.from_numpy(sim.settle(2)).cuda()
        B = _stacked(n, K, 25)
        torch.cuda.synchronize()
        c = sim.graph_captures()
        run(sim, 7, K, obs0, False, B)
        sim.sync()
        if run is _rollout:
            assert sim.graph_captures() <= c + 1          # (at most the single step's graph)
        outs.append((sim.get_state(), B))
    sim.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    for k in outs[0][1]:
        assert torch.equal(outs[0][1][k], outs[1][1][k]), k


def test_weight_swap_needs_no_recapture(feeding, policy25, monkeypatch):
    import torch
    from avr import policy_eval as PE
    monkeypatch.setenv('AVR_ENV_GROUPS', '3')
    A, md, S = feeding
    n = 80
    sim = make_sim(md, n)
    sim.set_state(np.tile(S, (5, 1)))
    sim.settle(2)
    sim.policy_set(policy25[2])
    B = _stacked(n, 3, 25)
    torch.cuda.synchronize()
    _rollout(sim, 0, 3, None, False, B)
    sim.sync()
    first = B['act'][0].clone()
    c = sim.graph_captures()
    pol2, rms2 = random_policy(25, 7, 32, seed=9)
    sim.policy_set(PE.policy_desc(pol2, rms2, 25, 7))
    assert sim.graph_captures() == c
    _rollout(sim, 3, 3, None, False, B)
    sim.sync()
    assert sim.graph_captures() == c
    a = torch.zeros(n, 7, device='cuda')
    torch.cuda.synchronize()
    sim.policy_act_device(3, B['obs'][0].data_ptr(), False, a.data_ptr(), None, None)
    sim.sync()
    assert torch.equal(B['act'][0], a)
    # ... and they are the new policy's actions: the old weights give others on the same observation
    sim.policy_set(policy25[2])
    sim.policy_act_device(3, B['obs'][0].data_ptr(), False, a.data_ptr(), None, None)
    sim.sync()
    assert not torch.equal(B['act'][0], a) and not torch.equal(first, B['act'][0])
    sim.close()


def test_errors(feeding, policy25):
    import torch
    from avr import _abi as ABI, reset_dressing as RD
    A, md, _ = feeding
    d = policy25[2]
    n = 8
    sim = make_sim(md, n)
    B = _stacked(n, 2, 25)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match='avr_policy_set first'):
        sim.policy_act_device(0, B['obs'][0].data_ptr(), True, B['act'][0].data_ptr())
    with pytest.raises(RuntimeError, match='avr_policy_set first'):
        _rollout(sim, 0, 2, None, True, B)
    wide = dict(d, hidden=65, a_w1=np.zeros((65, 25), np.float32), a_b1=np.zeros(65, np.float32), a_w2=np.zeros((65, 65), np.float32),
                a_b2=np.zeros(65, np.float32), mu_w=np.zeros((7, 65), np.float32))
    with pytest.raises(RuntimeError, match='hidden 65'):
        sim.policy_set(wide)
    with pytest.raises(RuntimeError, match='obs_dim 30'):
        sim.policy_set(dict(d, obs_dim=30))
    with pytest.raises(RuntimeError, match='exactly 2'):
        sim.policy_set(dict(d, n_layers=3))
    with pytest.raises(RuntimeError, match='no policy'):          # (none of the rejected ones was installed)
        _rollout(sim, 0, 2, None, True, B)
    sim.policy_set(d)
    with pytest.raises(RuntimeError, match='< 0'):
        _rollout(sim, -1, 2, None, True, B)
    with pytest.raises(RuntimeError, match='< 0'):
        sim.policy_act_device(-1, B['obs'][0].data_ptr(), True, B['act'][0].data_ptr())
    sim.close()
    Ad = RD.dressing_scene()
    dr = make_sim(ABI.ModelDesc(Ad), 2)
    from avr._lib import avr_policy_desc
    import ctypes as C
    assert dr.lib.avr_policy_set(dr.h, C.byref(avr_policy_desc())) == -1
    assert b'not built for DressingJaco' in dr.lib.avr_last_error(dr.h)
    assert dr.lib.avr_policy_act_device(dr.h, 0, None, 1, None, None, None) == -1
    assert dr.lib.avr_rollout_policy_device(dr.h, 0, 1, None, 1, None, None, None, None, None, None, None) == -1
    dr.close()


def test_torch_facade(feeding, policy25):
    """AVRTorchVecEnv.rollout_policy == the raw call from the same state and observation."""
    import torch
    from avr import policy_eval as PE
    from avr.env import AVRTorchVecEnv
    A, md, _ = feeding
    pol, rms, d = policy25
    n, K = 32, 8
    env = AVRTorchVecEnv('FeedingJaco-v0', n, auto_reset=False)
    obs0 = env.reset()
    S = env.get_state()
    it0 = env.iteration.copy()
    out = env.rollout_policy(pol, rms, K)
    torch.cuda.synchronize()
    assert out['n'] == K and np.array_equal(env.iteration, it0 + K) and out['reset'] is None
    assert torch.equal(out['obs'][0], obs0)
    sim = make_sim(md, n)
    sim.set_state(S)
    sim.policy_set(d)
    B = _stacked(n, K, 25)
    torch.cuda.synchronize()
    _rollout(sim, 0, K, obs0, False, B)
    sim.sync()
    for k in B:
        assert torch.equal(out[k], B[k]), k
    assert np.array_equal(env.get_state(), sim.get_state())
    sim.close()
    # the next rollout starts where this one ended, with the installed policy
    out2 = env.rollout_policy(None, None, 3)
    assert torch.equal(out2['obs'][0], B['obs'][K]) and np.array_equal(env.iteration, it0 + K + 3)
    env.close()


def test_evaluate_fused(policy25):
    """evaluate(fused=True) returns evaluate's keys (plus fused) for a short trial."""
    from avr import policy_eval as PE
    pol, rms, _ = policy25
    n = 32
    r = PE.evaluate('FeedingJaco-v0', pol, rms, n_envs=n, steps=8, deterministic=False, fused=True)
    assert r['fused'] is True and r['policy_graph'] is False
    assert set(r) == {'returns', 'mean_force', 'task_success', 'done', 'loop_s', 'graph_captures', 'policy_graph', 'fused'}
    assert r['returns'].shape == (n,) and r['mean_force'].shape == (n,) and r['task_success'].shape == (n,) and r['done'].shape == (n,)
    assert np.all(np.isfinite(r['returns'])) and r['loop_s'] > 0
