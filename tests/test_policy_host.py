"""Host side of the device policy (no GPU): the sampling noise's host mirror (_lib.policy_noise)
and the descriptor a policy is packed into (policy_eval.policy_desc)."""
import numpy as np
import pytest


def test_policy_noise_statistics():
    """4096 envs x 16 steps x 7 draws of the mirror alone: a unit normal's sample mean has standard
    deviation 1 / sqrt(N) and its sample variance sqrt(2 / N); both are held to 4 of those."""
    from avr import _lib
    z = np.stack([_lib.policy_noise(1001, np.arange(4096), t, 7) for t in range(16)])
    N = z.size
    assert z.shape == (16, 4096, 7) and z.dtype == np.float64
    assert np.all(np.isfinite(z))
    mean, var = float(z.mean()), float(z.var())
    print('policy_noise: N %d mean %.3g (bound %.3g) var - 1 %.3g (bound %.3g)' % (N, mean, 4 / np.sqrt(N), var - 1, 4 * np.sqrt(2 / N)))
    assert abs(mean) <= 4 / np.sqrt(N)
    assert abs(var - 1) <= 4 * np.sqrt(2 / N)
    # per action dimension too (each of the 7 comes from its own word pair / trigonometric branch)
    for j in range(7):
        n = z[..., j].size
        assert abs(z[..., j].mean()) <= 4 / np.sqrt(n) and abs(z[..., j].var() - 1) <= 4 * np.sqrt(2 / n)


def test_policy_noise_is_its_own_stream_and_sharding_stable():
    from avr import _lib
    ids = np.arange(256)
    for t in (0, 3, (1 << 32) + 5):
        z = _lib.policy_noise(1001, ids, t, 7)
        assert not np.allclose(z, _lib.random_actions(1001, ids, t, 7))
        # the Philox words themselves differ for the same key: the action stream's counter word 2 is j >> 2, the noise's has the top bit set
        ca = _lib.philox4x32_10([ids.astype(np.uint64), np.full(256, t & 0xFFFFFFFF, np.uint64), np.zeros(256, np.uint64),
                                 np.full(256, t >> 32, np.uint64)], 1001, 0)
        cn = _lib.philox4x32_10([ids.astype(np.uint64), np.full(256, t & 0xFFFFFFFF, np.uint64), np.full(256, 0x80000000, np.uint64),
                                 np.full(256, t >> 32, np.uint64)], 1001, 0)
        assert not any(np.any(x == y) for x, y in zip(ca, cn))
        # rows depend on the global env id only
        assert np.array_equal(_lib.policy_noise(1001, ids[100:], t, 7), z[100:])
        assert np.array_equal(_lib.policy_noise(1001, ids[::-1].copy(), t, 7), z[::-1])
    assert not np.array_equal(_lib.policy_noise(1001, ids, 0, 7), _lib.policy_noise(1001, ids, 1, 7))
    assert not np.array_equal(_lib.policy_noise(1001, ids, 0, 7), _lib.policy_noise(1002, ids, 0, 7))
    assert not np.array_equal(_lib.policy_noise(1001, ids, 5, 7), _lib.policy_noise(1001, ids, (1 << 32) + 5, 7))


def reference_forward(d, obs):
    """float64 numpy evaluation of a policy_desc dict: (mean, value, deterministic logp)."""
    f = lambda k: np.asarray(d[k], np.float64)
    x = np.asarray(obs, np.float64)
    if d['ob_mean'] is not None:
        x = np.clip((x - f('ob_mean')) / np.sqrt(f('ob_var') + d['eps']), -d['clip_obs'], d['clip_obs'])
    h = np.tanh(np.tanh(x @ f('a_w1').T + f('a_b1')) @ f('a_w2').T + f('a_b2'))
    mean = h @ f('mu_w').T + f('mu_b')
    c = np.tanh(np.tanh(x @ f('c_w1').T + f('c_b1')) @ f('c_w2').T + f('c_b2'))
    value = (c @ f('c_w3').T + f('c_b3'))[:, 0]
    logp = np.full(len(x), float(np.sum(-f('logstd') - 0.5 * np.log(2 * np.pi))))
    return mean, value, logp


def random_policy(obs_dim, act_dim=7, hidden=64, seed=0):
    """A random-init ActorCritic with a non-zero logstd and a non-trivial ob_rms."""
    import torch
    from avr import policy_eval as PE
    g = torch.Generator().manual_seed(seed)
    pol = PE.ActorCritic(obs_dim, act_dim, hidden)
    with torch.no_grad():
        for p in pol.parameters():
            p.copy_(torch.empty_like(p).uniform_(-0.5, 0.5, generator=g))
    rng = np.random.default_rng(seed)
    rms = PE.RunningMeanStd((obs_dim,), rng.normal(0, 0.5, obs_dim), rng.uniform(0.05, 2.0, obs_dim), 1000.0)
    return pol, rms


@pytest.mark.parametrize('obs_dim, hidden', [(25, 64), (30, 40)])
def test_policy_desc_round_trip(obs_dim, hidden):
    import torch
    from avr import policy_eval as PE
    pol, rms = random_policy(obs_dim, 7, hidden, seed=3)
    d = PE.policy_desc(pol, rms, obs_dim, 7)
    assert (d['obs_dim'], d['act_dim'], d['hidden'], d['n_layers']) == (obs_dim, 7, hidden, 2)
    assert d['a_w1'].shape == (hidden, obs_dim) and d['mu_w'].shape == (7, hidden) and d['c_w3'].shape == (1, hidden)
    assert all(d[k].dtype == np.float32 for k in ('ob_mean', 'ob_var', 'a_w1', 'a_b2', 'mu_b', 'logstd', 'c_w2', 'c_b3'))
    obs = np.random.default_rng(4).normal(0, 3, (50, obs_dim))
    mean, value, logp = reference_forward(d, obs)
    pol = pol.double()
    with torch.no_grad():
        x = PE.normalize(torch.from_numpy(obs), rms)
        v, a, lp, _ = pol.act(x, None, None, deterministic=True)
    assert np.allclose(a.numpy(), mean, rtol=0, atol=1e-6)          # (the arrays are the float32 weights: 1e-6 covers ob_rms's float32 copy)
    assert np.allclose(v.numpy()[:, 0], value, rtol=0, atol=1e-6)
    assert np.allclose(lp.numpy()[:, 0], logp, rtol=0, atol=1e-9)
    # without ob_rms: no normalisation
    d0 = PE.policy_desc(pol.float(), None)
    assert d0['ob_mean'] is None and d0['ob_var'] is None
    m0, _, _ = reference_forward(d0, obs)
    with torch.no_grad():
        _, a0, _, _ = pol.double().act(torch.from_numpy(obs), None, None, deterministic=True)
    assert np.allclose(a0.numpy(), m0, rtol=0, atol=1e-9)


def test_policy_desc_rejects_what_the_kernel_does_not_take():
    import torch
    from avr import policy_eval as PE
    with pytest.raises(ValueError, match='hidden'):
        PE.policy_desc(PE.ActorCritic(25, 7, 65), None)
    with pytest.raises(ValueError, match='env needs'):
        PE.policy_desc(PE.ActorCritic(30, 7, 64), None, 25, 7)
    with pytest.raises(ValueError, match='env needs'):
        PE.policy_desc(PE.ActorCritic(25, 6, 64), None, 25, 7)
    with pytest.raises(ValueError, match='ob_rms'):
        PE.policy_desc(PE.ActorCritic(25, 7, 64), PE.RunningMeanStd((30,)))
    deep = PE.ActorCritic(25, 7, 64)
    deep.actor = torch.nn.Sequential(*list(deep.actor), torch.nn.Linear(64, 64), torch.nn.Tanh())
    with pytest.raises(ValueError, match='two hidden layers'):
        PE.policy_desc(deep, None)
