"""CPU: the readable references of the device PPO update (avr/ppo.py): gae_reference against a
literal float64 loop, ppo_loss_reference's gradients against central finite differences, and the
new exports in the binding list."""
import numpy as np
import pytest

from test_policy_host import random_policy


def done_pattern(n, E):
    """done at k = 0, a middle k and k = n-1 (in different envs), one env with none, one with two."""
    d = np.zeros((n, E), np.uint8)
    d[0, 0] = 1
    d[n // 2, 1] = 1
    d[n - 1, 2] = 1
    d[1, 4] = 1
    d[n - 1, 4] = 1
    return d


def gae_loop64(rew, done, value, tv, gamma, lam, bootstrap):
    n, E = rew.shape
    adv, ret = np.zeros((n, E)), np.zeros((n, E))
    for e in range(E):
        gae = 0.0
        for k in range(n - 1, -1, -1):
            if done[k, e]:
                nv = float(tv[e]) if bootstrap else 0.0
            else:
                nv = float(value[k + 1, e])
            delta = float(rew[k, e]) + gamma * nv - float(value[k, e])
            gae = delta + gamma * lam * (0.0 if done[k, e] else gae)
            adv[k, e] = gae
            ret[k, e] = gae + float(value[k, e])
    return adv, ret


@pytest.mark.parametrize('bootstrap', [False, True])
def test_gae_reference_matches_float64_loop(bootstrap):
    """5 x 7.  |adv| <= sum_k |delta| < 5 * (1 + 2 * 3) = 35 here, every operation rounds to fp32 once
    (2^-24 relative) and a value passes through at most 5 steps of 3 operations: 35 * 15 * 2^-24 < 4e-5."""
    from avr import ppo
    n, E = 5, 7
    rng = np.random.default_rng(3)
    rew = rng.normal(0, 0.5, (n, E)).astype(np.float32)
    value = rng.normal(0, 1.0, (n + 1, E)).astype(np.float32)
    tv = rng.normal(0, 1.0, E).astype(np.float32)
    done = done_pattern(n, E)
    adv, ret = ppo.gae_reference(rew, done, value, tv, 0.99, 0.95, bootstrap)
    assert adv.dtype == np.float32 and ret.dtype == np.float32
    a64, r64 = gae_loop64(rew, done, value, tv, 0.99, 0.95, bootstrap)
    assert np.abs(adv - a64).max() < 4e-5 and np.abs(ret - r64).max() < 4e-5
    # the float64 evaluation of the same function is the loop up to float64 rounding
    a, r = ppo.gae_reference(rew, done, value, tv, 0.99, 0.95, bootstrap, dtype=np.float64)
    assert np.abs(a - a64).max() < 1e-13 and np.abs(r - r64).max() < 1e-13
    # bootstrap changes exactly the steps at or before a done
    other, _ = ppo.gae_reference(rew, done, value, tv, 0.99, 0.95, not bootstrap)
    assert np.array_equal(other[:, 3], adv[:, 3]) and not np.array_equal(other[:, 0], adv[:, 0])


def test_gae_reference_hand_computed():
    """3 steps, one env, gamma = 0.5, lam = 0.5, done at k = 1; all values exact in binary:
    k = 2: delta = 1 + 0.5 * 4 - 2 = 1,          gae = 1
    k = 1: done: nv = 8 (bootstrap) or 0:  delta = 2 + 4 - 1 = 5 | 2 + 0 - 1 = 1,  gae = delta
    k = 0: delta = 1 + 0.5 * 1 - 0.5 = 1,        gae = 1 + 0.25 * 5 = 2.25 | 1 + 0.25 * 1 = 1.25"""
    from avr import ppo
    rew = np.array([[1.0], [2.0], [1.0]])
    value = np.array([[0.5], [1.0], [2.0], [4.0]])
    done = np.array([[0], [1], [0]])
    adv, ret = ppo.gae_reference(rew, done, value, np.array([8.0]), 0.5, 0.5, True)
    assert adv[:, 0].tolist() == [2.25, 5.0, 1.0] and ret[:, 0].tolist() == [2.75, 6.0, 3.0]
    adv, ret = ppo.gae_reference(rew, done, value, np.array([8.0]), 0.5, 0.5, False)
    assert adv[:, 0].tolist() == [1.25, 1.0, 1.0] and ret[:, 0].tolist() == [1.75, 2.0, 3.0]


def small_batch(pol, rms, n, seed, clip=0.2):
    """n samples whose ratios fall on both sides of 1 +- clip and whose values fall on both sides of
    the value clip: actions are the policy's means plus noise, logp_old the policy's own log-prob
    shifted by a per-sample offset, value_old the critic's value shifted likewise."""
    import torch
    from avr import policy_eval as PE
    rng = np.random.default_rng(seed)
    od = pol.obs_dim
    mean_o = rms.mean if rms is not None else np.zeros(od)
    sd_o = np.sqrt(rms.var) if rms is not None else np.ones(od)
    obs = (mean_o + sd_o * rng.normal(0, 1.5, (n, od))).astype(np.float32)
    p64 = pol.double()
    with torch.no_grad():
        x = torch.from_numpy(obs).double()
        if rms is not None:
            x = PE.normalize(x, rms)
        mu = p64.mu(p64.actor(x))
        act = mu + p64.logstd.exp() * torch.from_numpy(rng.normal(0, 1, (n, pol.act_dim)))
        lp = (-((act - mu) ** 2) / (2 * torch.exp(2 * p64.logstd)) - p64.logstd - 0.5 * np.log(2 * np.pi)).sum(-1)
        v = p64.critic(x)[:, 0]
    shift = np.resize(np.array([0.0, 0.5, -0.5, 0.05, -0.05, 0.3]), n) * rng.uniform(0.8, 1.2, n)
    vshift = np.resize(np.array([0.5, -0.5, 0.05, -0.05, 0.0, 0.4]), n) * rng.uniform(0.8, 1.2, n)
    pol.float()
    return dict(obs=obs, act=act.numpy().astype(np.float32), logp=(lp.numpy() + shift).astype(np.float32),
                value=(v.numpy() + vshift).astype(np.float32), adv=rng.normal(0.3, 1.0, n).astype(np.float32),
                ret=(v.numpy() + rng.normal(0, 1.0, n)).astype(np.float32))


def test_ppo_loss_reference_gradients_match_finite_differences():
    """float64, 6 samples, hidden 5: every parameter's autograd gradient against central differences
    (h = 1e-6: truncation ~h^2, rounding ~1e-16 / h, both far below the 1e-6 relative bound), on a
    batch that exercises both sides of both clips."""
    import torch
    from avr import ppo
    pol, rms = random_policy(9, 7, 5, seed=4)
    batch = small_batch(pol, rms, 6, seed=5)
    pol = pol.double()
    params = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, norm_adv=True, clip_value=True)
    b64 = {k: torch.from_numpy(v).double() for k, v in batch.items()}
    loss, st = ppo.ppo_loss_reference(pol, rms, b64, None, params)
    # the batch is on both sides of the ratio clip and of the value clip
    with torch.no_grad():
        x = torch.clamp((b64['obs'] - torch.as_tensor(rms.mean)) / torch.sqrt(torch.as_tensor(rms.var) + 1e-8), -10, 10)
        mu = pol.mu(pol.actor(x))
        lp = (-((b64['act'] - mu) ** 2) / (2 * torch.exp(2 * pol.logstd)) - pol.logstd - 0.5 * np.log(2 * np.pi)).sum(-1)
        ratio = torch.exp(lp - b64['logp'])
        dv = pol.critic(x)[:, 0] - b64['value']
    assert (ratio > 1.2).any() and (ratio < 0.8).any() and ((ratio > 0.8) & (ratio < 1.2)).any()
    assert (dv > 0.2).any() and (dv < -0.2).any() and (dv.abs() < 0.2).any()
    assert 0 < float(st['clip_frac']) < 1
    grads = torch.autograd.grad(loss, list(pol.parameters()))
    h = 1e-6
    for p, g in zip(pol.parameters(), grads):
        flat = p.data.view(-1)
        for i in range(flat.numel()):
            old = float(flat[i])
            with torch.no_grad():
                flat[i] = old + h
                lp_, _ = ppo.ppo_loss_reference(pol, rms, b64, None, params)
                flat[i] = old - h
                lm_, _ = ppo.ppo_loss_reference(pol, rms, b64, None, params)
                flat[i] = old
            fd = (float(lp_) - float(lm_)) / (2 * h)
            assert abs(fd - float(g.view(-1)[i])) <= 1e-6 * max(1.0, abs(fd)), (tuple(p.shape), i, fd, float(g.view(-1)[i]))
    # value clipping off: the plain squared error
    l0, s0 = ppo.ppo_loss_reference(pol, rms, b64, None, dict(params, clip_value=False))
    with torch.no_grad():
        plain = 0.5 * ((pol.critic(x)[:, 0] - b64['ret']) ** 2).mean()
    assert float(s0['value_loss']) == float(plain) and float(s0['value_loss']) != float(st['value_loss'])
    # a minibatch is a selection of the batch, advantages normalised over the whole batch
    idx = torch.tensor([4, 1, 2])
    l1, _ = ppo.ppo_loss_reference(pol, rms, b64, idx, params)
    sub = {k: v[idx] for k, v in b64.items()}
    sub['adv'] = ((b64['adv'] - b64['adv'].mean()) / (b64['adv'].std() + 1e-5))[idx]
    l2, _ = ppo.ppo_loss_reference(pol, rms, sub, None, dict(params, norm_adv=False))
    assert abs(float(l1) - float(l2)) < 1e-14


def test_block_layout_helpers_invert_the_packing():
    """unpack_block of a block packed as avr_policy_set packs it returns the descriptor's arrays, and
    block_live_mask marks exactly the words they occupy."""
    from avr import policy_eval as PE, ppo
    pol, rms = random_policy(25, 7, 40, seed=2)
    d = PE.policy_desc(pol, rms, 25, 7)
    H = 40
    w = np.zeros(ppo.PW_WORDS, np.float32)
    for a in range(7):
        w[ppo.PW_LOGSTD + a], w[ppo.PW_BH + a] = d['logstd'][a], d['mu_b'][a]
        for k in range(H):
            w[ppo.PW_WH + k * 8 + a] = d['mu_w'][a, k]
    w[ppo.PW_BH + 7] = d['c_b3'][0]
    for k in range(H):
        w[ppo.PW_WH + k * 8 + 7] = d['c_w3'][0, k]
    for net, p in enumerate('ac'):
        o = ppo.PW_NET + net * ppo.PN_WORDS
        for j in range(H):
            w[o + ppo.PN_B1 + j], w[o + ppo.PN_B2 + j] = d[p + '_b1'][j], d[p + '_b2'][j]
            for k in range(25):
                w[o + ppo.PN_W1 + k * 64 + j] = d[p + '_w1'][j, k]
            for k in range(H):
                w[o + ppo.PN_W2 + k * 64 + j] = d[p + '_w2'][j, k]
    u = ppo.unpack_block(w, 25, 7, H)
    for k, v in u.items():
        assert np.array_equal(v, d[k]), k
    m = ppo.block_live_mask(25, 7, H)
    assert m.sum() == sum(v.size for v in u.values()) and np.all(w[~m] == 0) and np.all(w[m] != 0)
    assert ppo.block_live_mask(25, 7, H, has_critic=False).sum() == m.sum() - sum(u[k].size for k in u if k.startswith('c_'))


def test_new_exports_are_bound():
    from avr import _lib
    for n in ('avr_gae_device', 'avr_ppo_reset', 'avr_ppo_grad_device', 'avr_ppo_adam_device', 'avr_ppo_update_device', 'avr_ppo_buffers',
              'avr_policy_get', 'avr_policy_obs_norm_device', 'avr_ppo_words', 'avr_policy_block'):
        assert n in _lib.EXPORTS
    import ctypes as C
    assert C.sizeof(_lib.avr_ppo_params) == 40 and C.sizeof(_lib.avr_ppo_batch) == 8 + 6 * C.sizeof(C.c_void_p)
