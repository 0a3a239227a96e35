"""GPU: the policy and PPO kernels as ScratchItchPR2 (obs 30) and BedBathingPR2 (obs 24) instantiate
them (csrc/avr_task_tu.h compiles csrc/avr_policy.hip, csrc/avr_ppo.hip and the packing of
csrc/avr_capi.hip once per task with the task's K_OBS_DIM) against float64 references: the forward,
the minibatch gradient, Adam, the read-back, the padding and the ob_rms rows per task; the loss
options, the no-critic gradient, the entropy term and max_grad_norm <= 0 on one task; the
statistics ring past its 256 rows; and one BedBathingPR2 trainer iteration against torch.
The procedures and tolerances are those of tests/test_gpu_policy.py and tests/test_gpu_ppo.py."""
import numpy as np
import pytest

from test_gpu_policy import forward
from test_gpu_ppo import (GRAD_CASES, PARAMS, U32, block, check_8x, dev_tensor, policy32, reference_grads, stats_row, torch_update, upload,
                          value_bias_floor)
from test_policy_host import random_policy, reference_forward
from test_ppo_tasks_host import OBS_DIMS, assert_last_rows_under_test, last_component_normalised, push_last, task_batch

pytestmark = pytest.mark.gpu

N_ENVS = 70                                  # tail lanes of the last wavefront live (8 envs per wavefront: 9 blocks, the last with 6)
PR2 = ('scratch', 'bedbath')
NO_CRITIC = dict(c_w1=None, c_b1=None, c_w2=None, c_b2=None, c_w3=None, c_b3=None)


@pytest.fixture(scope='module')
def handles():
    """handles(task): the module's one 70-env handle of a task, made at first use and closed at the
    end.  No test here needs simulator state: each installs its own policy (policy_set, ppo_reset)."""
    from avr import _abi as ABI, _lib
    _lib.load()
    scenes = dict(feeding=ABI.TASK_FEEDING, scratch=ABI.TASK_SCRATCH, bedbath=ABI.TASK_BEDBATH)
    made = {}

    def get(task):
        if task not in made:
            made[task] = _lib.Sim(ABI.ModelDesc(ABI.load_scene(scenes[task])), N_ENVS)
            assert made[task].obs_dim == OBS_DIMS[task]
        return made[task]
    yield get
    for sim in made.values():
        sim.close()


def install_desc(sim, d):
    sim.policy_set(d)
    sim.ppo_reset()
    return d


def install(sim, pol, rms, critic=True):
    from avr import policy_eval as PE
    d = PE.policy_desc(pol, rms, sim.obs_dim, 7)
    return install_desc(sim, d if critic else dict(d, **NO_CRITIC))


def draw_obs(rms, od, seed, n=N_ENVS):
    """test_forward_matches_float64_reference's observations at obs size od, plus push_last."""
    rng = np.random.default_rng(seed)
    obs = (rms.mean + np.sqrt(rms.var) * rng.normal(0, 2, (n, od))).astype(np.float32)
    obs[::3, 4] += 40.0                       # beyond +clip after normalisation
    obs[1::5, 17] -= 55.0                     # beyond -clip
    return push_last(obs, od)


def check_forward(what, dev, t32, ref):
    """{name: array} of the device, of torch's CPU float32 forward and of float64 under the 8 x rule."""
    for name in dev:
        bound = 8 * float(np.abs(t32[name] - ref[name]).max())
        err = float(np.abs(dev[name] - ref[name]).max())
        print('%s %s: bound %.3g observed %.3g' % (what, name, bound, err))
        assert np.all(np.isfinite(dev[name])) and err <= bound, (name, err, bound)


# ------------------------------------------------------------------ 1. the forward
@pytest.mark.parametrize('task', PR2)
def test_forward_matches_float64_reference(handles, task):
    """70 envs, normalised components beyond +-clip_obs, the last component beyond it on some rows and
    inside on others: mean, value and deterministic log-prob against reference_forward in float64,
    each within 8 x the error of torch's CPU float32 ActorCritic.act against the same float64.
    On an MI355X (observed / bound): scratch mean 1.7e-6 / 1.1e-5, value 1.2e-6 / 6.2e-6, logp 6.9e-8 /
    5.6e-7; bedbath mean 1.6e-6 / 9.7e-6, value 1.2e-6 / 7.9e-6, logp 5.0e-8 / 4.0e-7: at most 0.19 of the bound."""
    import torch
    from avr import policy_eval as PE
    od = OBS_DIMS[task]
    sim = handles(task)
    pol, rms = random_policy(od, 7, 64, seed=100 + od)
    d = PE.policy_desc(pol, rms, od, 7)
    obs = draw_obs(rms, od, seed=101)
    x64 = (obs.astype(np.float64) - d['ob_mean']) / np.sqrt(d['ob_var'].astype(np.float64) + d['eps'])
    assert (x64[:, :od - 1] > 10).any() and (x64[:, :od - 1] < -10).any()
    xl = last_component_normalised(obs, rms, od)
    assert (xl > 10).any() and (xl < -10).any() and (np.abs(xl) < 10).any()
    ref = dict(zip(('mean', 'value', 'logp'), reference_forward(d, obs)))
    with torch.no_grad():
        v, a, lp, _ = pol.float().cpu().act(PE.normalize(torch.from_numpy(obs), rms), None, None, deterministic=True)
    t32 = dict(mean=a.numpy(), value=v.numpy()[:, 0], logp=lp.numpy()[:, 0])
    sim.policy_set(d)
    a_g, lp_g, v_g = forward(sim, 0, obs, True)
    check_forward('forward[%s]' % task, dict(mean=a_g, value=v_g, logp=lp_g), t32, ref)


@pytest.mark.parametrize('task', PR2)
def test_forward_without_ob_rms_and_critic(handles, task):
    """No ob_rms: the observation goes in as it is; no critic: the value is exactly 0.  A 40-unit
    policy (zero-padded to the kernel's 64), same rule.
    On an MI355X (observed / bound): scratch mean 9.2e-7 / 5.2e-6, logp 2.5e-7 / 2.0e-6; bedbath mean
    9.6e-7 / 5.5e-6, logp 2.3e-7 / 1.8e-6: at most 0.18 of the bound."""
    import torch
    from avr import policy_eval as PE
    od = OBS_DIMS[task]
    sim = handles(task)
    pol, _ = random_policy(od, 7, 40, seed=110 + od)
    d = PE.policy_desc(pol, None, od, 7)
    obs = np.random.default_rng(112).normal(0, 1.5, (N_ENVS, od)).astype(np.float32)
    ref_mean, _, ref_lp = reference_forward(d, obs)
    with torch.no_grad():
        _, a, lp, _ = pol.act(torch.from_numpy(obs), None, None, deterministic=True)
    sim.policy_set(dict(d, **NO_CRITIC))
    a_g, lp_g, v_g = forward(sim, 0, obs, True)
    check_forward('forward (no ob_rms, no critic)[%s]' % task, dict(mean=a_g, logp=lp_g), dict(mean=a.numpy(), logp=lp.numpy()[:, 0]),
                  dict(mean=ref_mean, logp=ref_lp))
    assert np.all(v_g == 0)


@pytest.mark.parametrize('ob_rms', [True, False], ids=['ob_rms', 'no_ob_rms'])
@pytest.mark.parametrize('task', ('feeding',) + PR2)
def test_value_only_forward_equals_full_call(handles, task, ob_rms):
    """policy_act_device(t, obs, det, None, None, value) (POL_VALUE_ONLY: the critic alone runs) writes,
    bit for bit, the value of the full call on the same observations, into a buffer that held NaN."""
    import torch
    from avr import policy_eval as PE
    od = OBS_DIMS[task]
    sim = handles(task)
    pol, rms = random_policy(od, 7, 64, seed=120 + od)
    sim.policy_set(PE.policy_desc(pol, rms if ob_rms else None, od, 7))
    obs = draw_obs(rms, od, seed=121) if ob_rms else np.random.default_rng(122).normal(0, 1.5, (N_ENVS, od)).astype(np.float32)
    o = torch.from_numpy(obs).cuda()
    a, lp, v = torch.zeros(N_ENVS, 7, device='cuda'), torch.zeros(N_ENVS, device='cuda'), torch.zeros(N_ENVS, device='cuda')
    v_only = torch.full((N_ENVS,), float('nan'), device='cuda')
    torch.cuda.synchronize()
    sim.policy_act_device(0, o.data_ptr(), True, a.data_ptr(), lp.data_ptr(), v.data_ptr())
    sim.policy_act_device(0, o.data_ptr(), True, None, None, v_only.data_ptr())
    sim.sync()
    assert torch.equal(v, v_only) and bool((v != 0).all())


@pytest.mark.parametrize('task, t', [('scratch', 3), ('bedbath', (1 << 32) + 7)])
def test_noise_matches_host_mirror(handles, task, t):
    """(action - mean) / std == policy_noise(seed, env, t) within 1e-5 and the log-prob is that of the
    eps drawn: tests/test_gpu_policy.py::test_noise_matches_host_mirror's bounds, one t per task.
    On an MI355X: max |eps - mirror| 7.6e-7 (scratch), 7.9e-7 (bedbath)."""
    from avr import _lib, policy_eval as PE
    od = OBS_DIMS[task]
    sim = handles(task)
    pol, rms = random_policy(od, 7, 64, seed=130 + od)
    d = PE.policy_desc(pol, rms, od, 7)
    sim.policy_set(d)
    obs = (rms.mean + np.sqrt(rms.var) * np.random.default_rng(131).normal(0, 1, (N_ENVS, od))).astype(np.float32)
    mean, _, _ = forward(sim, 0, obs, True)
    act, lp, _ = forward(sim, t, obs, False)
    std = np.exp(d['logstd'].astype(np.float64))
    eps = (act.astype(np.float64) - mean) / std
    ref = _lib.policy_noise(1001, np.arange(N_ENVS), t, 7)
    err = float(np.abs(eps - ref).max())
    print('noise[%s] t %d: max |eps - mirror| %.3g' % (task, t, err))
    assert err <= 1e-5
    lp_ref = np.sum(-0.5 * ref ** 2 - d['logstd'].astype(np.float64) - 0.5 * np.log(2 * np.pi), axis=1)
    assert np.all(np.abs(lp - lp_ref) <= 1e-5 * np.abs(ref).sum(1) + 1e-5)


# ------------------------------------------------------------------ 2. the gradient
def run_gradient_case(sim, what, c, params, critic=True):
    """tests/test_gpu_ppo.py::test_gradient_matches_float64_autograd's procedure on `sim`'s task: case c
    (N, M, j, perm, hidden, ob_rms) under `params`; critic False installs the actor alone.  Returns
    (device gradient block, device statistics row, float64 statistics, policy)."""
    import torch
    from avr import ppo
    od = sim.obs_dim
    pol, rms = policy32(od, c.get('hidden', 64), seed=200 + od, ob_rms=c.get('ob_rms', True))
    batch = task_batch(pol, rms, c['N'], seed=201)
    N, M, j = c['N'], c['M'], c['j']
    B = N // M
    perm = np.random.default_rng(202).permutation(N).astype(np.int32) if c.get('perm') else np.arange(N, dtype=np.int32)
    idx = perm[j * B:(j + 1) * B].astype(np.int64)
    r64, s64 = reference_grads(pol, rms, batch, idx, params, torch.float64)
    t32, _ = reference_grads(pol, rms, batch, idx, params, torch.float32)
    if critic:
        assert_last_rows_under_test(r64, batch, idx, rms, od)
    else:
        assert np.abs(r64['a_w1'][:, od - 1]).max() > 0 and all(np.all(r64[k] == 0) for k in r64 if k.startswith('c_'))
    install(sim, pol, rms, critic)
    pb, keep = upload(sim, batch)
    dperm = torch.from_numpy(perm).cuda() if c.get('perm') else None
    torch.cuda.synchronize()
    for jj in sorted({0, j}):                 # (minibatch 0 computes the batch's advantage statistics)
        sim.ppo_grad_device(pb, sim.ppo_params(params), jj, M, None if dperm is None else dperm.data_ptr())
    g = block(sim, 'g')
    st = stats_row(sim, j)
    dev = ppo.unpack_block(g, od, 7, pol.hidden)
    assert np.all(g[~ppo.block_live_mask(od, 7, pol.hidden, has_critic=critic)] == 0)      # header, ob_rms rows, padding (and the absent critic)
    check_8x(what, dev, t32, r64, floor=dict(c_b3=value_bias_floor(pol, rms, batch, idx, params)) if critic else None)
    for i, k in enumerate(('policy_loss', 'value_loss', 'entropy', 'approx_kl', 'clip_frac')):
        if k == 'value_loss' and not critic:
            assert st[i] == 0.0
            continue
        print('stat %s %s: device %.9g reference %.9g' % (what, k, st[i], s64[k]))
        assert abs(st[i] - s64[k]) <= 1e-5 + 1e-5 * abs(s64[k]), (k, st[i], s64[k])
    return g, st, s64, pol


TASK_GRAD_CASES = ('B9', 'M3of100', 'B8221', 'hidden40', 'no_ob_rms')


@pytest.mark.parametrize('case', TASK_GRAD_CASES)
@pytest.mark.parametrize('task', PR2)
def test_gradient_matches_float64_autograd(handles, task, case):
    """Every parameter tensor's gradient of one minibatch against torch float64 autograd of
    ppo_loss_reference under the 8 x rule, the five statistics (1e-5 absolute + 1e-5 relative) and exact
    zeros outside block_live_mask(obs_dim, 7, hidden): a second block with one live row (B9), a dropped
    remainder with indirect indexing (M3of100), two full grid strides and a ragged third (B8221), a
    40-unit policy and no ob_rms.  The last observation component is clipped on some rows of every
    minibatch and not on others, and its first-layer gradients are non-zero in float64.
    Observed on an MI355X, the tensor closest to its bound per case (observed / bound): scratch B9 c_b2
    4.4e-8 / 2.3e-7, M3of100 c_b2 2.7e-8 / 1.1e-7, B8221 a_w1 3.7e-7 / 1.3e-6, hidden40 a_b1 5.8e-8 /
    2.8e-7, no_ob_rms a_b2 1.5e-7 / 6.9e-7; bedbath B9 a_b1 1.4e-7 / 8.6e-7, M3of100 a_w1 4.0e-7 / 2.5e-6,
    B8221 c_b1 1.6e-9 / 1.6e-8, hidden40 mu_w 1.7e-7 / 9.8e-7, no_ob_rms mu_b 2.6e-7 / 1.1e-6: at most
    0.29 of the bound.  c_b3 (observed / its bound, the larger of the rule's and the floor): 9.0e-11 ..
    9.9e-8 / 5.1e-7 .. 8.9e-7, at most 0.11."""
    run_gradient_case(handles(task), 'grad[%s %s]' % (task, case), GRAD_CASES[case], PARAMS)


# ------------------------------------------------------------------ 3. Adam, read-back, padding, the ob_rms rows
def run_adam_case(sim, what, params, epochs=3, M=2, N=N_ENVS):
    """tests/test_gpu_ppo.py::test_adam_matches_torch's procedure on `sim`'s task; max_grad_norm <= 0 in
    `params`: no clipping on either side.  Returns the float64 run's statistics rows."""
    import torch
    od = sim.obs_dim
    clip = params['max_grad_norm'] > 0
    pol, rms = policy32(od, 64, seed=300 + od)
    batch = task_batch(pol, rms, N, seed=301)
    r64, rows = torch_update(pol, rms, batch, params, epochs, M, torch.float64, clip=clip)
    t32, _ = torch_update(pol, rms, batch, params, epochs, M, torch.float32, clip=clip)
    install(sim, pol, rms)
    pb, keep = upload(sim, batch)
    sim.ppo_update_device(pb, sim.ppo_params(params), epochs, M)
    d = sim.policy_get()
    st = np.stack([stats_row(sim, i) for i in range(epochs * M)])
    # c_b3, one number: one ulp of the weight per step (tests/test_gpu_ppo.py::test_adam_matches_torch)
    check_8x(what, d, t32, r64, floor=dict(c_b3=epochs * M * U32 * max(float(np.abs(r64['c_b3']).max()), params['lr'])))
    for i, r in enumerate(rows):
        for col, k in ((5, 'grad_norm'), (3, 'approx_kl'), (4, 'clip_frac')):
            print('stat %s [%d] %s: device %.9g reference %.9g' % (what, i, k, st[i, col], r[k]))
            assert abs(st[i, col] - r[k]) <= 1e-5 + 1e-4 * abs(r[k]), (i, k, st[i, col], r[k])
    return rows


@pytest.mark.parametrize('max_grad_norm', [0.05, 100.0], ids=['clipped', 'unclipped'])
@pytest.mark.parametrize('task', PR2)
def test_adam_matches_torch(handles, task, max_grad_norm):
    """Three epochs x two minibatches of 35 from the same start: the weights read back through
    avr_policy_get against torch float64 Adam + clip_grad_norm_ under the 8 x rule; grad_norm, approx_kl
    and clip_frac of every minibatch (1e-5 absolute + 1e-4 relative).  One case's norm exceeds
    max_grad_norm at every step, the other's never does.
    Observed on an MI355X, the tensor closest to its bound (observed / bound): scratch clipped c_w3
    4.4e-8 / 2.8e-7, unclipped c_b1 1.2e-7 / 4.6e-7; bedbath clipped a_b1 5.9e-8 / 3.3e-7, unclipped a_w1
    1.2e-7 / 7.5e-7: at most 0.26 of the bound.  c_b3 (observed / its bound, the larger of the rule's and
    the floor): scratch 1.4e-8 / 1.3e-7 and 2.1e-8 / 1.7e-7, bedbath 4.0e-9 and 4.3e-9 / 6.8e-8."""
    rows = run_adam_case(handles(task), 'adam[%s %s]' % (task, max_grad_norm), dict(PARAMS, max_grad_norm=max_grad_norm))
    norms = [r['grad_norm'] for r in rows]
    assert all(x > max_grad_norm for x in norms) if max_grad_norm < 1 else all(x < max_grad_norm for x in norms)


@pytest.mark.parametrize('task', PR2)
def test_padding_stays_zero(handles, task):
    """A 40-unit policy, three Adam steps at lr = 1e-2: every padded word of the weight block, of m and of
    v is still exactly 0.0 and every live word moved.  The padded first-layer rows are 30-31 for obs 30
    and 24-31 for obs 24."""
    from avr import ppo
    od = OBS_DIMS[task]
    sim = handles(task)
    pol, rms = policy32(od, 40, seed=310 + od)
    batch = task_batch(pol, rms, N_ENVS, seed=311)
    install(sim, pol, rms)
    w0 = block(sim, 'w')
    pb, keep = upload(sim, batch)
    sim.ppo_update_device(pb, sim.ppo_params(dict(PARAMS, lr=1e-2)), 3, 1)
    live = ppo.block_live_mask(od, 7, 40)
    pad = ~live
    pad[:ppo.PW_LOGSTD] = False
    w, m, v = block(sim, 'w'), block(sim, 'm'), block(sim, 'v')
    # 2 networks x (32 x 64 - od x 40 first-layer words, 64 x 64 - 40 x 40 second-layer, 2 x 24 biases), the heads' 24 x 8, logstd's eighth word
    assert pad.sum() == 2 * ((32 * 64 - od * 40) + (64 * 64 - 40 * 40) + 48) + 24 * 8 + 1
    for net in range(2):
        o = ppo.PW_NET + net * ppo.PN_WORDS + ppo.PN_W1
        rows = pad[o:o + 32 * 64].reshape(32, 64)[:, :40].all(1)
        assert np.array_equal(np.nonzero(rows)[0], np.arange(od, 32))
        for x in (w, m, v):
            assert np.all(x[o:o + 32 * 64].reshape(32, 64)[od:] == 0.0) and np.all(x[o:o + 32 * 64].reshape(32, 64)[od - 1, :40] != 0.0)
    for name, x in (('w', w), ('m', m), ('v', v)):
        assert np.all(x[pad] == 0.0), name
    assert np.array_equal(w[:ppo.PW_LOGSTD], w0[:ppo.PW_LOGSTD])             # header and ob_rms rows untouched
    assert np.all(w[live] != w0[live]) and np.all(v[live] > 0)


@pytest.mark.parametrize('task', PR2)
def test_obs_norm_rows_and_repacking(handles, task):
    """avr_policy_obs_norm_device, given 32-entry device arrays, writes exactly obs_dim rows of PW_MEAN
    (the means) and PW_SD (float32(sqrt(float64(var) + eps)), formed in float64 here) and leaves every
    other word of the block bit-identical; avr_policy_get returns the means and variances that
    avr_policy_set packs to that same block, bit for bit."""
    import torch
    from avr import ppo
    od = OBS_DIMS[task]
    sim = handles(task)
    pol, rms = policy32(od, 64, seed=320 + od)
    install(sim, pol, rms)
    w0 = block(sim, 'w')
    rng = np.random.default_rng(321)
    mean, var = rng.normal(0, 2, 32).astype(np.float32), rng.uniform(0.05, 2.0, 32).astype(np.float32)
    m, v = torch.from_numpy(mean).cuda(), torch.from_numpy(var).cuda()
    torch.cuda.synchronize()
    sim.policy_obs_norm_device(m.data_ptr(), v.data_ptr())
    w = block(sim, 'w')
    assert np.array_equal(w[ppo.PW_MEAN:ppo.PW_MEAN + od], mean[:od])
    assert np.array_equal(w[ppo.PW_SD:ppo.PW_SD + od], np.sqrt(var[:od].astype(np.float64) + np.float64(np.float32(1e-8))).astype(np.float32))
    rest = np.ones(ppo.PW_WORDS, bool)
    rest[ppo.PW_MEAN:ppo.PW_MEAN + od] = rest[ppo.PW_SD:ppo.PW_SD + od] = False
    assert np.array_equal(w.view(np.uint32)[rest], w0.view(np.uint32)[rest])
    assert np.all(w[ppo.PW_MEAN + od:ppo.PW_MEAN + 32] == 0.0) and np.all(w[ppo.PW_SD + od:ppo.PW_SD + 32] == 1.0)
    back = sim.policy_get()
    assert np.array_equal(back['ob_mean'], mean[:od]) and back['ob_var'].shape == (od,)
    # (a variance with the same float32 divisor: both square roots lie within half an ulp, 2^-24 relative, of it, so the
    # radicands var + eps differ by at most twice 2^-23 relative)
    assert np.all(np.abs(back['ob_var'].astype(np.float64) - var[:od]) <= 2 * U32 * (var[:od] + 1e-8))
    sim.policy_set(back)
    assert np.array_equal(block(sim, 'w').view(np.uint32), w.view(np.uint32))


# ------------------------------------------------------------------ 4. options no other test compares with a reference
OPTION_CASES = {
    'norm_adv_off': dict(norm_adv=False), 'clip_value_off': dict(clip_value=False), 'both_off': dict(norm_adv=False, clip_value=False),
    'ent_coef_0': dict(ent_coef=0.0), 'ent_coef_1': dict(ent_coef=1.0),
}


@pytest.mark.parametrize('option', list(OPTION_CASES))
def test_gradient_options_match_float64_autograd(handles, option):
    """ScratchItchPR2, one minibatch of 70: the gradient procedure with advantage normalisation off, the
    value clip off, both off, and the entropy coefficient at 0 and at 1.  The reduce kernel adds the
    constant -ent_coef to logstd's gradient: the 8 x rule bounds logstd's error by about 5e-7, so neither
    a term at ent_coef = 0 nor a missing one at 1 fits.
    Observed on an MI355X, the tensor closest to its bound (observed / bound): norm_adv_off a_b1 1.6e-7 /
    6.1e-7, clip_value_off logstd 1.6e-7 / 5.2e-7, both_off a_b1 1.6e-7 / 6.1e-7, ent_coef_0 logstd 1.6e-7 /
    4.8e-7, ent_coef_1 a_b1 1.5e-7 / 5.9e-7: at most 0.34 of the bound; c_b3 at most 2.6e-8 / its
    bound 8.4e-7."""
    params = dict(PARAMS, **OPTION_CASES[option])
    run_gradient_case(handles('scratch'), 'grad[scratch %s]' % option, GRAD_CASES['B70'], params)


def test_entropy_term_is_the_constant(handles):
    """The same minibatch at ent_coef 0 and 1 (deterministic kernels: the same sums): logstd's gradient
    differs by exactly float32(g - 1), every other word of the gradient block is bit-identical."""
    from avr import ppo
    sim = handles('scratch')
    pol, rms = policy32(sim.obs_dim, 64, seed=400)
    batch = task_batch(pol, rms, N_ENVS, seed=401)
    g = []
    for ent in (0.0, 1.0):
        install(sim, pol, rms)
        pb, keep = upload(sim, batch)
        sim.ppo_grad_device(pb, sim.ppo_params(dict(PARAMS, ent_coef=ent)), 0, 1)
        g.append(block(sim, 'g'))
    ls = slice(ppo.PW_LOGSTD, ppo.PW_LOGSTD + 7)
    assert np.array_equal(g[1][ls], g[0][ls] - np.float32(1.0))
    g[1][ls] = g[0][ls]
    assert np.array_equal(g[0].view(np.uint32), g[1].view(np.uint32))


def test_no_critic_gradient_matches_float64_autograd(handles):
    """ScratchItchPR2 with the actor alone installed and vf_coef = 0: the actor's tensors and logstd
    against float64 autograd of the same loss under the 8 x rule, every critic word of the gradient block
    exactly 0 (block_live_mask(..., has_critic=False)) and the value-loss statistic exactly 0.
    Observed on an MI355X, the tensor closest to its bound (observed / bound): logstd 1.6e-7 / 5.2e-7."""
    from avr import ppo
    g, st, s64, pol = run_gradient_case(handles('scratch'), 'grad[scratch no_critic]', GRAD_CASES['B70'], dict(PARAMS, vf_coef=0.0), critic=False)
    o = ppo.PW_NET + ppo.PN_WORDS
    assert np.all(g[o:] == 0.0) and g[ppo.PW_BH + 7] == 0.0 and np.all(g[ppo.PW_WH:ppo.PW_NET].reshape(64, 8)[:, 7] == 0.0)
    assert np.all(g[ppo.block_live_mask(OBS_DIMS['scratch'], 7, 64, has_critic=False)] != 0.0)


def test_adam_without_clipping_matches_torch(handles):
    """ScratchItchPR2, max_grad_norm = 0: Adam on the gradient as it is, against torch_update without its
    clip_grad_norm_ line (three epochs x two minibatches, N = 70); the statistics row still carries the
    gradient's norm.  max_grad_norm = 0.05 on the same batch clips every step
    (test_adam_matches_torch[scratch-clipped]), so a clip applied here would show.
    Observed on an MI355X, the tensor closest to its bound (observed / bound): c_b1 1.2e-7 / 4.6e-7; c_b3
    2.1e-8 / its bound 1.7e-7."""
    rows = run_adam_case(handles('scratch'), 'adam[scratch max_grad_norm=0]', dict(PARAMS, max_grad_norm=0.0))
    assert all(r['grad_norm'] > 0.05 for r in rows)


# ------------------------------------------------------------------ 5. the statistics ring past its 256 rows
def test_stats_ring_wraps_without_touching_its_neighbours(handles):
    """BedBathingPR2, N = 100 in 100 minibatches of one sample, 3 epochs with a permutation each: 300
    gradient + Adam steps in one avr_ppo_update_device call, whose statistics row is step % 256, against
    the same 300 steps as single calls, whose row is the minibatch index (never beyond 99).  The advantage
    statistics and Adam's step count lie directly behind the ring: a row written there would change every
    later step.  The weight block, m and v are bit-identical, ring row 299 % 256 = 43 equals the loop's last
    row and ring row 44, last written at step 44, the loop's row at that step."""
    import torch
    from avr import _lib
    sim = handles('bedbath')
    od = sim.obs_dim
    N, M, epochs = 100, 100, 3
    assert epochs * M > _lib.PPO_STATS_ROWS
    pol, rms = policy32(od, 64, seed=500)
    batch = task_batch(pol, rms, N, seed=501)
    perm = np.stack([np.random.default_rng(502 + e).permutation(N) for e in range(epochs)]).astype(np.int32)
    pb, keep = upload(sim, batch)
    dperm = torch.from_numpy(perm).cuda()
    torch.cuda.synchronize()
    P = sim.ppo_params(dict(PARAMS, norm_adv=True))
    install(sim, pol, rms)
    sim.ppo_update_device(pb, P, epochs, M, dperm.data_ptr())
    sim.sync()
    upd = [block(sim, k) for k in 'wmv']
    ring = dev_tensor(sim.ppo_buffers()[3], (_lib.PPO_STATS_ROWS, _lib.PPO_STAT_WORDS)).cpu().numpy().copy()
    install(sim, pol, rms)
    row44 = None
    for ep in range(epochs):
        for j in range(M):
            sim.ppo_grad_device(pb, P, j, M, dperm[ep].data_ptr())
            sim.ppo_adam_device(P)
            if ep == 0 and j == 44:
                row44 = stats_row(sim, 44)
    last = stats_row(sim, M - 1)
    loop = [block(sim, k) for k in 'wmv']
    for name, a, b in zip('wmv', upd, loop):
        assert np.all(np.isfinite(a)) and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert np.array_equal(ring[(epochs * M - 1) % _lib.PPO_STATS_ROWS].view(np.uint32), last.view(np.uint32))
    assert np.array_equal(ring[44].view(np.uint32), row44.view(np.uint32))
    assert last[5] > 0 and row44[5] > 0 and not np.array_equal(ring[43], ring[44])      # (grad_norm: rows that were written)


# ------------------------------------------------------------------ 6. one trainer iteration against torch
def test_trainer_iteration_matches_torch_bedbath():
    """BedBathingPR2, 16 envs, reset_pool=1, one PPOTrainer.iterate() of a 6-step rollout and 2 epochs x 1
    minibatch (ob_rms frozen, rewards not normalised): the batch the trainer used -- the rollout's
    stacked observations, actions, log-probs and values and the device's advantages and returns -- goes
    through torch_update in float64 and float32 from the initial weights (one minibatch: the permutation
    changes only the order of the sums), and sync_module()'s weights are held to the 8 x rule.
    ob_rms is the mean (half a deviation off) and variance (+ 0.05) of the 16 reset observations; the last
    observation column of both first layers is asserted to have moved in float64.
    Observed on an MI355X, the tensor closest to its bound (observed / bound): mu_w 9.6e-8 / 2.3e-7, 0.42
    of it; c_b3 4.1e-9 / its bound 3.3e-8 (the rule's; the floor, one ulp of the weight per step, is 2.6e-8)."""
    import copy
    import torch
    from avr import policy_eval as PE, ppo
    from avr.env import AVRTorchVecEnv
    pol, _ = policy32(24, 64, seed=600)
    env = AVRTorchVecEnv('BedBathingPR2-v0', 16, reset_pool=1)
    # ob_rms from the reset observations (float32 values): every variance at least 0.05 and the mean half a deviation
    # off, so that the normalised rollout observations are of order 1 (the first layers do not saturate) and a
    # component that never changes is not normalised to 0, where its first-layer row would get no gradient
    obs0 = env.reset().cpu().numpy().astype(np.float64)
    var0 = (obs0.var(0) + 0.05).astype(np.float32).astype(np.float64)
    rms = PE.RunningMeanStd((24,), (obs0.mean(0) - 0.5 * np.sqrt(var0)).astype(np.float32).astype(np.float64), var0, 16.0)
    hyper = dict(epochs=2, n_minibatch=1, update_ob_rms=False, norm_reward=False)
    tr = ppo.PPOTrainer(env, copy.deepcopy(pol), copy.deepcopy(rms), n_steps=6, generator=torch.Generator(device='cuda').manual_seed(5), **hyper)
    r = tr.iterate()
    torch.cuda.synchronize()
    flat = ppo.flatten_rollout(tr.last['out'], tr.last['adv'], tr.last['ret'])
    batch = {k: np.ascontiguousarray(v.detach().cpu().numpy()) for k, v in flat.items()}
    after, _ = tr.sync_module()
    dev = {k: p.detach().cpu().numpy().astype(np.float64) for k, p in ppo.module_params(after).items()}
    env.close()
    assert batch['obs'].shape == (96, 24) and bool(torch.isfinite(r['stats']).all()) and float(batch['adv'].std()) > 1e-3
    P = dict(ppo.DEFAULTS, **hyper)
    r64, rows = torch_update(pol, rms, batch, P, 2, 1, torch.float64)
    t32, _ = torch_update(pol, rms, batch, P, 2, 1, torch.float32)
    start = {k: p.detach().numpy() for k, p in ppo.module_params(pol).items()}
    assert all(np.abs(r64[k] - start[k]).max() > 1e-5 for k in r64)           # (every tensor moved: lr = 3e-4, two steps)
    assert all(np.abs(r64[k] - start[k])[:, 23].max() > 1e-5 for k in ('a_w1', 'c_w1'))      # (and so did observation row 23)
    check_8x('trainer[bedbath]', dev, t32, r64, floor=dict(c_b3=2 * U32 * max(float(np.abs(r64['c_b3']).max()), P['lr'])))
    st = r['stats'].cpu().numpy()
    for i, row in enumerate(rows):
        for col, k in ((5, 'grad_norm'), (3, 'approx_kl'), (4, 'clip_frac')):
            print('trainer[bedbath] stat[%d] %s: device %.9g reference %.9g' % (i, k, st[i, col], row[k]))
            assert abs(st[i, col] - row[k]) <= 1e-5 + 1e-4 * abs(row[k]), (i, k, st[i, col], row[k])
