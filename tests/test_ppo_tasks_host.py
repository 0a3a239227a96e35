"""CPU: the batches tests/test_gpu_ppo_tasks.py feeds the three per-task instantiations of the policy
and PPO kernels (observation sizes 24, 25 and 30), and a check that the tolerance rule those tests
apply (test_gpu_ppo.check_8x) rejects the defects they are there to find."""
import numpy as np
import pytest

from test_gpu_ppo import KEYS, PARAMS, check_8x, make_batch, policy32, reference_grads

OBS_DIMS = {'feeding': 25, 'scratch': 30, 'bedbath': 24}


def push_last(obs, obs_dim):
    """Push the last observation component (rows 28-29 of ScratchItchPR2 and row 23 of BedBathingPR2
    are the first-layer rows FeedingJaco's instantiation never touches) beyond +clip_obs on every
    fourth row and beyond -clip_obs on rows 2, 9, 16, ...; the other rows stay where they were drawn."""
    obs[::4, obs_dim - 1] += 40.0
    obs[2::7, obs_dim - 1] -= 55.0
    return obs


def task_batch(pol, rms, N, seed):
    """test_gpu_ppo.make_batch plus push_last (with ob_rms: without it nothing is clipped)."""
    b = make_batch(pol, rms, N, seed)
    if rms is not None:
        push_last(b['obs'], pol.obs_dim)
    return b


def last_component_normalised(obs, rms, obs_dim):
    """float64 normalised value, before the clip, of the last observation component of each row."""
    k = obs_dim - 1
    return (obs[:, k].astype(np.float64) - rms.mean[k]) / np.sqrt(rms.var[k] + 1e-8)


def assert_last_rows_under_test(r64, batch, idx, rms, obs_dim):
    """The float64 reference gradient of the last observation column of both first layers is non-zero
    and, with ob_rms, the minibatch has that component on both sides of the clip."""
    assert np.abs(r64['a_w1'][:, obs_dim - 1]).max() > 0 and np.abs(r64['c_w1'][:, obs_dim - 1]).max() > 0
    if rms is not None:
        x = last_component_normalised(batch['obs'][idx], rms, obs_dim)
        assert (x > 10).any() and (x < -10).any() and (np.abs(x) < 10).any()


@pytest.mark.parametrize('obs_dim', [24, 25, 30])
def test_rule_rejects_a_dropped_swapped_or_shifted_row(obs_dim):
    """A 70-sample batch per observation size; the "device" result is torch's own float32 gradient with
    (a) the last observation column of a_w1 zeroed (a dropped row), (b) the last two observation
    columns of c_w1 swapped (a wrong row stride), (c) logstd shifted by ent_coef (the entropy term
    applied twice or not at all).  The largest altered entry is first shown to lie more than 100 x
    the tensor's bound from float64, so that check_8x, which compares the tensor's maximum error,
    rejects by the rule and not by luck; the unaltered float32 gradient passes.
    Measured (altered error / bound): obs 24 a_w1 4.3e4, c_w1 1.6e5, logstd 1.1e4; obs 25 a_w1 9.4e4,
    c_w1 1.5e5, logstd 1.5e4; obs 30 a_w1 8.3e4, c_w1 5.7e5, logstd 2.4e4."""
    import torch
    pol, rms = policy32(obs_dim, 64, seed=91)
    batch = task_batch(pol, rms, 70, seed=92)
    idx = np.arange(70)
    r64, _ = reference_grads(pol, rms, batch, idx, PARAMS, torch.float64)
    t32, _ = reference_grads(pol, rms, batch, idx, PARAMS, torch.float32)
    assert_last_rows_under_test(r64, batch, idx, rms, obs_dim)
    check_8x('teeth[%d] unaltered' % obs_dim, t32, t32, r64)

    def altered(key, change):
        dev = {k: v.copy() for k, v in t32.items()}
        change(dev[key])
        return dev

    def zero_last(a):
        a[:, obs_dim - 1] = 0.0

    def swap_last_two(a):
        a[:, [obs_dim - 2, obs_dim - 1]] = a[:, [obs_dim - 1, obs_dim - 2]]

    def shift(a):
        a += PARAMS['ent_coef']

    for key, change in (('a_w1', zero_last), ('c_w1', swap_last_two), ('logstd', shift)):
        dev = altered(key, change)
        assert all(np.array_equal(dev[k], t32[k]) for k in KEYS if k != key)
        moved = dev[key] != t32[key]
        bound = 8 * float(np.abs(t32[key] - r64[key]).max())
        err = float(np.abs(dev[key] - r64[key])[moved].max())
        print('teeth[%d] %s: altered error %.3g, bound %.3g, ratio %.3g' % (obs_dim, key, err, bound, err / bound))
        assert moved.any() and err > 100 * bound, (key, err, bound)
        with pytest.raises(AssertionError):
            check_8x('teeth[%d] %s altered' % (obs_dim, key), dev, t32, r64)
