"""PPO on the batched backend: the readable references of the device update (csrc/avr_ppo.hip,
include/avr.h avr_gae_device / avr_ppo_*), a small trainer around AVRTorchVecEnv (PPOTrainer) and its
form across the ranks of a torch.distributed group (DistPPOTrainer, combine_reference).

The loss is a2c_ppo_acktr's PPO.update (clipped surrogate, clipped value loss, entropy bonus) on the
harness's ActorCritic (avr/policy_eval.py); the reference ships neither that library nor its
trainer or settings, so the hyper-parameter defaults below are this facade's own choice, not the
reference's.  gae_reference and ppo_loss_reference are the same formulas as the kernels in numpy
and torch at any dtype: the tests use them as the reference, and they can be read next to the
kernels.  reward_norm_reference and episode_stats_reference do the same for the reward half of
VecNormalize and the episode statistics (csrc/avr_trainstats.hip, include/avr.h
avr_reward_norm_device / avr_episode_stats_device).
"""
import numpy as np
import torch

from . import policy_eval as PE

LOG_SQRT_2PI = 0.5 * float(np.log(2 * np.pi))

# This facade's defaults (its own choice; see the module docstring).
DEFAULTS = dict(
    gamma=0.99, lam=0.95, bootstrap=True,           # advantage estimation; bootstrap: a TimeLimit done is a truncation
    clip=0.2, vf_coef=0.5, ent_coef=0.0,            # L = L_pi + vf_coef L_v - ent_coef H
    max_grad_norm=0.5,                              # global L2 clip
    lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5,      # Adam
    norm_adv=True, clip_value=True,
    epochs=4, n_minibatch=8,                        # passes over the batch, minibatches per pass
    update_ob_rms=True,                             # keep VecNormalize's running observation statistics
    norm_reward=False, clip_reward=10.0,            # VecNormalize's reward half: rew / sqrt(var(discounted return) + 1e-8), clipped
    episode_stats=True,                             # reduce the episodes that ended in the rollout (episode_summary)
)
RET_EPS = 1e-8                                      # VecNormalize's epsilon

# the device weight block (csrc/avr_policy.hip PW_* / PN_*), in floats
POL_H = 64
PW_HDR, PW_MEAN, PW_SD, PW_LOGSTD, PW_BH, PW_WH = 0, 8, 40, 72, 80, 88
PW_NET = PW_WH + POL_H * 8
PN_W1, PN_B1 = 0, 32 * POL_H
PN_W2 = PN_B1 + POL_H
PN_B2 = PN_W2 + POL_H * POL_H
PN_WORDS = PN_B2 + POL_H
PW_WORDS = PW_NET + 2 * PN_WORDS


def block_live_mask(obs_dim, act_dim, hidden, has_critic=True):
    """bool [PW_WORDS]: the words of the device weight block that hold a trainable parameter of a
    policy of these dimensions; every other word from PW_LOGSTD on is zero padding (hidden units
    beyond `hidden`, observation rows beyond obs_dim, head column 7 without a critic)."""
    m = np.zeros(PW_WORDS, bool)
    m[PW_LOGSTD:PW_LOGSTD + act_dim] = True
    m[PW_BH:PW_BH + act_dim] = True
    wh = np.zeros((POL_H, 8), bool)
    wh[:hidden, :act_dim] = True
    if has_critic:
        m[PW_BH + 7] = True
        wh[:hidden, 7] = True
    m[PW_WH:PW_NET] = wh.reshape(-1)
    for net in range(2 if has_critic else 1):
        o = PW_NET + net * PN_WORDS
        w1 = np.zeros((32, POL_H), bool)
        w1[:obs_dim, :hidden] = True
        w2 = np.zeros((POL_H, POL_H), bool)
        w2[:hidden, :hidden] = True
        m[o + PN_W1:o + PN_B1] = w1.reshape(-1)
        m[o + PN_W2:o + PN_B2] = w2.reshape(-1)
        m[o + PN_B1:o + PN_B1 + hidden] = True
        m[o + PN_B2:o + PN_B2 + hidden] = True
    return m


def unpack_block(w, obs_dim, act_dim, hidden, has_critic=True):
    """The named arrays (policy_desc's keys, [out][in]) of a host copy of a block-layout array: the
    weight block itself, or a gradient / moment block."""
    w = np.asarray(w)
    d = dict(logstd=w[PW_LOGSTD:PW_LOGSTD + act_dim].copy(), mu_b=w[PW_BH:PW_BH + act_dim].copy())
    wh = w[PW_WH:PW_NET].reshape(POL_H, 8)
    d['mu_w'] = wh[:hidden, :act_dim].T.copy()
    if has_critic:
        d['c_b3'] = w[PW_BH + 7:PW_BH + 8].copy()
        d['c_w3'] = wh[:hidden, 7][None, :].copy()
    for net, p in enumerate('ac' if has_critic else 'a'):
        o = PW_NET + net * PN_WORDS
        d[p + '_w1'] = w[o + PN_W1:o + PN_B1].reshape(32, POL_H)[:obs_dim, :hidden].T.copy()
        d[p + '_b1'] = w[o + PN_B1:o + PN_B1 + hidden].copy()
        d[p + '_w2'] = w[o + PN_W2:o + PN_B2].reshape(POL_H, POL_H)[:hidden, :hidden].T.copy()
        d[p + '_b2'] = w[o + PN_B2:o + PN_B2 + hidden].copy()
    return d


def module_params(actor_critic):
    """{policy_desc key: the module's parameter tensor} of an ActorCritic."""
    a, c = list(actor_critic.actor), list(actor_critic.critic)
    return dict(a_w1=a[0].weight, a_b1=a[0].bias, a_w2=a[2].weight, a_b2=a[2].bias, mu_w=actor_critic.mu.weight, mu_b=actor_critic.mu.bias,
                logstd=actor_critic.logstd, c_w1=c[0].weight, c_b1=c[0].bias, c_w2=c[2].weight, c_b2=c[2].bias, c_w3=c[4].weight, c_b3=c[4].bias)


def gae_reference(rew, done, value, term_value=None, gamma=0.99, lam=0.95, bootstrap=False, dtype=np.float32):
    """Generalised advantage estimation over stacked [n, E] arrays (value [n+1, E]) -> (adv, ret), in
    `dtype` with the device kernel's operations in the kernel's order (float32: bit for bit):
        nv    = done[k] ? (bootstrap ? term_value : 0) : value[k+1]
        delta = (rew[k] + gamma * nv) - value[k]
        gae   = delta + (gamma * lam) * (done[k] ? 0 : gae);  adv[k] = gae;  ret[k] = gae + value[k]
    Every done of this code base is the TimeLimit: bootstrap treats it as a truncation and uses
    V(terminal observation) (term_value [E], each env's most recent), otherwise the return is cut."""
    T = np.dtype(dtype).type
    rew, value = np.asarray(rew, dtype), np.asarray(value, dtype)
    done = np.asarray(done).astype(bool)
    n, E = rew.shape
    assert value.shape == (n + 1, E) and done.shape == (n, E)
    tv = np.asarray(term_value, dtype) if bootstrap else np.zeros(E, dtype)
    g, gl = T(gamma), T(T(gamma) * T(lam))
    adv, ret = np.zeros((n, E), dtype), np.zeros((n, E), dtype)
    gae = np.zeros(E, dtype)
    for k in range(n - 1, -1, -1):
        nv = np.where(done[k], tv, value[k + 1])
        delta = (rew[k] + g * nv) - value[k]
        gae = delta + gl * np.where(done[k], T(0), gae)
        adv[k] = gae
        ret[k] = gae + value[k]
    return adv, ret


def train_stats_state(E):
    """The state avr_train_stats_reset leaves in a handle of E envs, as the dict the two mirrors below
    carry from call to call: the discounted returns R and their running moments (ret_rms), the running
    episodes' accumulators and each env's last finished episode."""
    z = lambda dt: np.zeros(E, dt)
    return dict(R=z(np.float64), mean=0.0, var=1.0, count=1e-4,
                ep_ret=z(np.float32), ep_len=z(np.int32), ep_force=z(np.float32),
                last_ret=z(np.float32), last_len=z(np.int32), last_success=z(np.float32), n_finished=z(np.int32))


def reward_norm_reference(rew, done, state, gamma=0.99, clip_rew=10.0, eps=RET_EPS, update=True):
    """VecNormalize's reward path over stacked [n, E] arrays -> rew_out [n, E] float32, in float64 in the
    device call's phases (csrc/avr_trainstats.hip, include/avr.h avr_reward_norm_device); `state`
    (train_stats_state) is advanced in place unless update is False (eval mode: only the scaling).
      1. per env, k ascending:  R = R * gamma + rew[k];  Rk[k] = R;  R = 0 at done[k]
      2. per step:              bm[k] = mean_e Rk[k], bv[k] = mean_e (Rk[k] - bm[k])^2
      3. k ascending:           RunningMeanStd.update's merge of (bm[k], bv[k], E) into (mean, var, count);
                                var_k[k] = var after it
      4. elementwise:           clip(rew[k] / sqrt(var_k[k] + eps), -clip_rew, clip_rew) as float32
    A step's rewards are scaled with the statistics after that step's update, as baselines does."""
    rew = np.asarray(rew, np.float32).astype(np.float64)
    done = np.asarray(done).astype(bool)
    n, E = rew.shape
    if update:
        R, Rk = state['R'].copy(), np.zeros((n, E))
        for k in range(n):
            R = R * gamma + rew[k]
            Rk[k] = R
            R = np.where(done[k], 0.0, R)
        bm = Rk.mean(1)
        bv = ((Rk - bm[:, None]) ** 2).mean(1)
        mean, var, count, bc = float(state['mean']), float(state['var']), float(state['count']), float(E)
        var_k = np.zeros(n)
        for k in range(n):
            d = float(bm[k]) - mean
            tot = count + bc
            new_mean = mean + d * bc / tot
            var = (var * count + float(bv[k]) * bc + d * d * count * bc / tot) / tot
            mean, count = new_mean, tot
            var_k[k] = var
        state.update(R=R, mean=mean, var=var, count=count)
    else:
        var_k = np.full(n, float(state['var']))
    return np.clip(rew / np.sqrt(var_k + eps)[:, None], -clip_rew, clip_rew).astype(np.float32)


def episode_stats_reference(rew, done, info, state):
    """The aggregate row (float64 [len(_lib.EPISODE_STATS)]) of the episodes that end inside stacked
    rew / done [n, E], info [n, E, 2] = {total_force_on_human, task_success}, in the device call's
    phases (include/avr.h avr_episode_stats_device); `state` (train_stats_state) is advanced in place.
      1. per env, k ascending: ep_ret += rew[k] and ep_force += info[k][0] in float32, ep_len += 1; at
         done[k] the episode closes with (ep_ret, ep_len, info[k][1], ep_force / ep_len), becomes the env's
         last finished one and adds to the env's share of every column in float64; the accumulators restart
      2. per column: the envs' shares summed (ret_min / ret_max: min / max)
    With no episode closed ret_min = +inf and ret_max = -inf."""
    rew, info = np.asarray(rew, np.float32), np.asarray(info, np.float32)
    done = np.asarray(done).astype(bool)
    n, E = rew.shape
    S = state
    names = ('episodes', 'ret_sum', 'ret_sumsq', 'ret_min', 'ret_max', 'len_sum', 'success_sum', 'force_mean_sum', 'steps', 'rew_sum')
    P = {c: np.zeros(E) for c in names}
    P['ret_min'][:], P['ret_max'][:] = np.inf, -np.inf
    for k in range(n):
        S['ep_ret'] = S['ep_ret'] + rew[k]
        S['ep_force'] = S['ep_force'] + info[k, :, 0]
        S['ep_len'] = S['ep_len'] + np.int32(1)
        P['rew_sum'] += rew[k].astype(np.float64)
        d = done[k]
        if d.any():
            ret, ln = S['ep_ret'][d].astype(np.float64), S['ep_len'][d].astype(np.float64)
            P['episodes'][d] += 1.0
            P['ret_sum'][d] += ret
            P['ret_sumsq'][d] += ret * ret
            P['ret_min'][d] = np.minimum(P['ret_min'][d], ret)
            P['ret_max'][d] = np.maximum(P['ret_max'][d], ret)
            P['len_sum'][d] += ln
            P['success_sum'][d] += info[k, d, 1].astype(np.float64)
            P['force_mean_sum'][d] += S['ep_force'][d].astype(np.float64) / ln
            S['last_ret'] = np.where(d, S['ep_ret'], S['last_ret'])
            S['last_len'] = np.where(d, S['ep_len'], S['last_len'])
            S['last_success'] = np.where(d, info[k, :, 1], S['last_success'])
            S['n_finished'] = S['n_finished'] + d.astype(np.int32)
            S['ep_ret'] = np.where(d, np.float32(0), S['ep_ret'])
            S['ep_force'] = np.where(d, np.float32(0), S['ep_force'])
            S['ep_len'] = np.where(d, np.int32(0), S['ep_len'])
    P['steps'][:] = float(n)
    return np.array([P[c].min() if c == 'ret_min' else P[c].max() if c == 'ret_max' else P[c].sum() for c in names])


def ppo_loss_reference(actor_critic, ob_rms, batch, idx, params):
    """The loss of one minibatch and its statistics, in the dtype of the module's parameters.

    batch: dict of flattened tensors obs [N, obs_dim] (raw), act [N, act_dim], logp [N], value [N],
    adv [N], ret [N]; idx: the minibatch's sample indices (LongTensor, or None: all); params: clip,
    vf_coef, ent_coef, norm_adv, clip_value (DEFAULTS' names).  ob_rms None: no normalisation;
    otherwise an object with mean / var (arrays or tensors) applied as policy_eval.normalize does.
    Returns (loss, dict(policy_loss, value_loss, entropy, approx_kl, clip_frac)):
        logp_new = sum_a -(act_a - mean_a)^2 / (2 exp(2 logstd_a)) - logstd_a - log(2 pi) / 2
        ratio = exp(logp_new - logp);  L_pi = -mean(min(ratio A, clamp(ratio, 1 - c, 1 + c) A))
        v_clip = value + clamp(v - value, -c, c);  L_v = 0.5 mean(max((v - ret)^2, (v_clip - ret)^2))
        H = sum_a (0.5 + log(2 pi) / 2 + logstd_a);  L = L_pi + vf_coef L_v - ent_coef H
    with A = (adv - mean(adv)) / (std(adv) + 1e-5) over the whole batch (unbiased std) when norm_adv."""
    p0 = actor_critic.logstd
    dt, dev = p0.dtype, p0.device
    t = lambda x: torch.as_tensor(x).to(device=dev, dtype=dt)
    adv_all = t(batch['adv'])
    if params.get('norm_adv', True):
        adv_all = (adv_all - adv_all.mean()) / (adv_all.std() + 1e-5)
    sel = (lambda x: x) if idx is None else (lambda x: x[idx])
    obs, act, logp_old, adv = sel(t(batch['obs'])), sel(t(batch['act'])), sel(t(batch['logp'])), sel(adv_all)
    if ob_rms is not None:
        obs = torch.clamp((obs - t(ob_rms.mean)) / torch.sqrt(t(ob_rms.var) + PE.EPS), -PE.CLIP_OBS, PE.CLIP_OBS)
    c = float(params['clip'])
    mean = actor_critic.mu(actor_critic.actor(obs))
    logstd = actor_critic.logstd
    logp = (-((act - mean) ** 2) / (2 * torch.exp(2 * logstd)) - logstd - LOG_SQRT_2PI).sum(-1)
    ratio = torch.exp(logp - logp_old)
    policy_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1 - c, 1 + c) * adv).mean()
    entropy = (0.5 + LOG_SQRT_2PI + logstd).sum()
    vf = float(params.get('vf_coef', 0.0))
    if vf != 0.0 or 'ret' in batch and batch['ret'] is not None:
        v = actor_critic.critic(obs)[:, 0]
        ret = sel(t(batch['ret']))
        if params.get('clip_value', True):
            v_old = sel(t(batch['value']))
            v_clip = v_old + torch.clamp(v - v_old, -c, c)
            value_loss = 0.5 * torch.max((v - ret) ** 2, (v_clip - ret) ** 2).mean()
        else:
            value_loss = 0.5 * ((v - ret) ** 2).mean()
    else:
        value_loss = torch.zeros((), dtype=dt, device=dev)
    loss = policy_loss + vf * value_loss - float(params.get('ent_coef', 0.0)) * entropy
    with torch.no_grad():
        stats = dict(policy_loss=policy_loss.detach(), value_loss=value_loss.detach(), entropy=entropy.detach(),
                     approx_kl=(logp_old - logp).mean(), clip_frac=((ratio - 1).abs() > c).to(dt).mean())
    return loss, stats


PPO_SEGMENTS = 8                                    # include/avr.h AVR_PPO_SEGMENTS
PPO_SEG_WORDS = PW_WORDS + 8                        # include/avr.h AVR_PPO_SEG_WORDS: the gradient block, then a statistics row


def combine_reference(rows, ent_coef=0.0, act_dim=0):
    """The host mirror of avr_ppo_combine_device's sum: rows [PPO_SEGMENTS, words] float32 -> [words]
    float32, every word the rows' words added in ascending row order in float64 and rounded to float32
    once; ent_coef is then subtracted, in float32, on the act_dim logstd words (rows of at least the
    weight block's length).  The order is part of the definition: float64 addition is not associative,
    and the one rounding to float32 can land on the other side of a tie."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 2 and rows.shape[0] == PPO_SEGMENTS
    a = np.zeros(rows.shape[1], np.float64)
    for k in range(PPO_SEGMENTS):
        a = a + rows[k].astype(np.float64)
    g = a.astype(np.float32)
    if act_dim:
        g[PW_LOGSTD:PW_LOGSTD + act_dim] = g[PW_LOGSTD:PW_LOGSTD + act_dim] - np.float32(ent_coef)
    return g


def segments_of(rank, world):
    """The segments (of PPO_SEGMENTS) rank `rank` of `world` computes: a contiguous run of PPO_SEGMENTS /
    world, rank 0's first, so that the ranks' rows gathered in rank order are in segment order."""
    rank, world = int(rank), int(world)
    if world < 1 or PPO_SEGMENTS % world:
        raise ValueError('a world of %d ranks does not divide the %d segments of a minibatch (1, 2, 4 or 8 ranks)' % (world, PPO_SEGMENTS))
    if not 0 <= rank < world:
        raise ValueError('rank %d outside 0..%d' % (rank, world - 1))
    per = PPO_SEGMENTS // world
    return list(range(rank * per, (rank + 1) * per))


def flatten_rollout(out, adv, ret):
    """rollout_policy's stacked tensors as ppo_loss_reference's flattened batch (views, no copy)."""
    n, E = out['rew'].shape
    N = n * E
    return dict(obs=out['obs'][:n].reshape(N, -1), act=out['act'].reshape(N, -1), logp=out['logp'].reshape(N), value=out['value'][:n].reshape(N),
                adv=adv.reshape(N), ret=ret.reshape(N))


class PPOTrainer:
    """PPO with every part of the iteration on the device: the rollout (the policy inside the rollout
    graphs), the running observation statistics, advantage estimation and the update all run in
    stream order with no host synchronisation; the weights live in the handle's weight block.

    env: an AVRTorchVecEnv made with reset_pool=m (the device rollover keeps the episode
    boundaries inside the rollouts); actor_critic / ob_rms: the initial policy (ob_rms None: a
    fresh RunningMeanStd); n_steps: steps per rollout.  hyper: any of DEFAULTS' keys --
      gamma 0.99, lam 0.95, bootstrap True (a TimeLimit done bootstraps from V(terminal observation)),
      clip 0.2, vf_coef 0.5, ent_coef 0.0, max_grad_norm 0.5, lr 3e-4, beta1 0.9, beta2 0.999, eps 1e-5,
      norm_adv True, clip_value True, epochs 4, n_minibatch 8, update_ob_rms True,
      norm_reward False, clip_reward 10.0, episode_stats True.
    These defaults are this facade's own choice: the reference ships neither its trainer nor its
    settings.  generator: a torch.Generator on the env's device for the minibatch permutations.

    norm_reward: the reward half of baselines' VecNormalize (the a2c_ppo_acktr pipeline's wrapper): the
    advantages are estimated from rew / sqrt(var + 1e-8) clipped to +-clip_reward, var the running
    variance of the discounted return (gamma), carried across iterations on the device
    (env.normalize_rewards).  The critic then learns returns of normalised rewards: `value` and `ret`
    are in normalised-reward units, not the task's.  save() stores the policy and ob_rms only, as
    before; the return statistics stay in the handle (_lib.Sim.train_stats_buffers).
    episode_stats: every iteration reduces the episodes that ended inside its rollout, from the raw
    rewards (env.episode_stats); episode_summary reads such a row on the host."""

    def __init__(self, env, actor_critic, ob_rms=None, n_steps=128, generator=None, **hyper):
        bad = set(hyper) - set(DEFAULTS)
        if bad:
            raise TypeError('PPOTrainer: unknown hyper-parameters %s' % sorted(bad))
        self.hyper = dict(DEFAULTS, **hyper)
        self.env, self.actor_critic, self.n_steps, self.generator = env, actor_critic, int(n_steps), generator
        if env._cur is None:
            env.reset()
        if self.hyper['bootstrap'] and env._pool is None:
            raise ValueError('PPOTrainer: bootstrap=True needs an env made with reset_pool=m')
        self.ob_rms = ob_rms if ob_rms is not None else PE.RunningMeanStd((env.L.OBS_DIM,))
        env.set_policy(actor_critic, self.ob_rms)
        env.ppo_reset()                             # (a new network: Adam starts from zero moments)
        env.train_stats_reset()                     # (a new run: no return statistics, no episode under way)
        dev = env.dev
        # VecNormalize's running statistics on the device (float64; the block receives float32 copies)
        self._mean = torch.as_tensor(np.asarray(self.ob_rms.mean, np.float64), device=dev)
        self._var = torch.as_tensor(np.asarray(self.ob_rms.var, np.float64), device=dev)
        self._count = torch.tensor(float(self.ob_rms.count), dtype=torch.float64, device=dev)
        self._m32 = torch.zeros(env.L.OBS_DIM, device=dev)
        self._v32 = torch.zeros(env.L.OBS_DIM, device=dev)
        self.iterations = 0

    def _update_ob_rms(self, obs):
        """RunningMeanStd.update with the batch's mean / variance, on the device, then the block's rows."""
        env, torch_ = self.env, torch
        x = obs.reshape(-1, obs.shape[-1]).double()
        bm, bv, bc = x.mean(0), x.var(0, unbiased=False), float(x.shape[0])
        d = bm - self._mean
        tot = self._count + bc
        self._var = (self._var * self._count + bv * bc + d * d * self._count * bc / tot) / tot
        self._mean = self._mean + d * bc / tot
        self._count = tot
        self._m32.copy_(self._mean)
        self._v32.copy_(self._var)
        env.ext.wait_stream(torch_.cuda.current_stream(env.dev))
        env.sim.policy_obs_norm_device(self._m32.data_ptr(), self._v32.data_ptr())
        torch_.cuda.current_stream(env.dev).wait_stream(env.ext)

    def iterate(self):
        """One PPO iteration: rollout, (optional) ob_rms update, episode statistics, (optional) reward
        normalisation, advantage estimation, update.  Returns device tensors: the update's statistics
        rows [epochs * n_minibatch, 6] under 'stats' (columns _lib.PPO_STATS), the rollout's mean raw
        reward under 'mean_reward' and, with episode_stats, the aggregate row of the episodes that ended
        in the rollout under 'episodes' (float64, columns _lib.EPISODE_STATS; episode_summary reads it);
        nothing is synchronised."""
        h, env = self.hyper, self.env
        out = env.rollout_policy(None, None, self.n_steps)
        if h['update_ob_rms']:
            # (the batch keeps the raw observations: the update normalises them with the new statistics)
            self._update_ob_rms(out['obs'][:out['n']])
        res = {}
        if h['episode_stats']:
            res['episodes'] = env.episode_stats(out)                # (the raw rewards, whatever the update trains on)
        rew_norm = None
        if h['norm_reward']:
            rew_norm = env.normalize_rewards(out, h['gamma'], h['clip_reward'], RET_EPS, update=True)
            adv, ret = env.compute_gae(dict(out, rew=rew_norm), h['gamma'], h['lam'], h['bootstrap'])
        else:
            adv, ret = env.compute_gae(out, h['gamma'], h['lam'], h['bootstrap'])
        stats = env.ppo_update(out, adv, ret, h, h['epochs'], h['n_minibatch'], generator=self.generator)
        self.iterations += 1
        self.last = dict(out=out, adv=adv, ret=ret, rew_norm=rew_norm)
        return dict(res, stats=stats, mean_reward=out['rew'].mean())

    @staticmethod
    def episode_summary(row):
        """An 'episodes' row of iterate() (or the sum of several: every column but ret_min / ret_max adds)
        as Python numbers -- the one blocking helper: it copies the row to the host.  Keys: episodes,
        return_mean, return_std (population), return_min, return_max, length_mean, success_rate,
        force_mean (the mean over episodes of the episode's mean total_force_on_human); all but episodes
        are None when no episode ended."""
        from . import _lib
        r = dict(zip(_lib.EPISODE_STATS, (float(x) for x in torch.as_tensor(row).detach().cpu().tolist())))
        m = int(r['episodes'])
        keys = ('return_mean', 'return_std', 'return_min', 'return_max', 'length_mean', 'success_rate', 'force_mean')
        if m == 0:
            return dict(dict.fromkeys(keys), episodes=0)
        mean = r['ret_sum'] / m
        return dict(episodes=m, return_mean=mean, return_std=max(r['ret_sumsq'] / m - mean * mean, 0.0) ** 0.5, return_min=r['ret_min'],
                    return_max=r['ret_max'], length_mean=r['len_sum'] / m, success_rate=r['success_sum'] / m, force_mean=r['force_mean_sum'] / m)

    def sync_module(self):
        """Copy the device weights and observation statistics back into the torch module and ob_rms
        (through avr_policy_get; blocks until the queued work is done)."""
        d = self.env.sim.policy_get()
        with torch.no_grad():
            for k, p in module_params(self.actor_critic).items():
                p.copy_(torch.as_tensor(d[k]).reshape(p.shape))
        self.ob_rms.mean = np.asarray(d['ob_mean'], np.float64)
        self.ob_rms.var = np.asarray(d['ob_var'], np.float64)
        self.ob_rms.count = float(self._count)
        return self.actor_critic, self.ob_rms

    def save(self, path):
        """sync_module, then policy_eval.save_policy: the checkpoint loads with load_policy and runs
        in evaluate(..., fused=True)."""
        self.sync_module()
        PE.save_policy(path, self.actor_critic, self.ob_rms)


class DistPPOTrainer(PPOTrainer):
    """PPOTrainer across the ranks of a torch.distributed group: every rank steps its shard of the global
    env ids (an env made with env_offset = rank * n_envs, reset_pool=m and pool_world=(rank, world,
    group)), and all ranks end every iteration with the same weights, bit for bit the weights one process
    with all world * n_envs envs computes.  PPOTrainer's arguments and hyper-parameters,
    plus group: a torch.distributed process group (torch.distributed.group.WORLD for the default one);
    None runs every segment locally with no collective: the single-process reference.

    iterate(): the rollout and advantage estimation on the shard; the all-gather of obs, act, logp,
    value, adv, ret (and rew, done) in global env order; the running observation statistics from the
    gathered observations; the advantage statistics of the gathered batch; then, per epoch and
    minibatch, this rank's PPO_SEGMENTS / world segment rows (avr_ppo_grad_segment_device), the
    all-gather of the rows, avr_ppo_combine_device and avr_ppo_adam_device on inputs that are identical
    on every rank.  The minibatch permutations come from `generator`, which must be seeded alike on all
    ranks (None: a generator seeded with the env's seed).  'episodes' rows are gathered and added
    (ret_min / ret_max: min / max), 'mean_reward' is the gathered rollout's.

    norm_reward=True is not built: the return statistics reduce over the handle's own envs in a fixed
    tree, which a shard cannot reproduce.  A world that does not divide PPO_SEGMENTS is a ValueError."""

    def __init__(self, env, actor_critic, ob_rms=None, n_steps=128, generator=None, group=None, **hyper):
        if hyper.get('norm_reward', DEFAULTS['norm_reward']):
            raise NotImplementedError('DistPPOTrainer: norm_reward=True (the return statistics are per handle; see DESIGN.md)')
        self.group = group
        self.rank, self.world = (0, 1)
        if group is not None:
            from . import dist as D
            self.rank, self.world = D.rank_world(group)
        self.segments = segments_of(self.rank, self.world)
        super().__init__(env, actor_critic, ob_rms, n_steps, generator, **hyper)
        if self.generator is None:
            self.generator = torch.Generator(device=env.dev).manual_seed(env.seed)
        self._segs = torch.zeros(PPO_SEGMENTS, PPO_SEG_WORDS, device=env.dev)       # the minibatch's rows, in segment order

    def _gather_batch(self, out, adv, ret):
        """The shard's stacked arrays as one packed [n, E, C] tensor, gathered to [n, world * E, C] and
        split into the flattened batch's contiguous tensors (copies only: no arithmetic touches a value)."""
        n = out['n']
        od, ad = out['obs'].shape[-1], out['act'].shape[-1]
        cols = [out['obs'][:n], out['act'], out['logp'][..., None], out['value'][:n, :, None], adv[..., None], ret[..., None], out['rew'][..., None],
                out['done'].to(torch.float32)[..., None]]
        x = torch.cat(cols, -1)
        if self.group is not None:
            from . import dist as D
            x = D.gather_stacked(x, self.group)
        E = x.shape[1]
        o = od + ad
        G = dict(obs=x[..., :od], act=x[..., od:o], logp=x[..., o], value=x[..., o + 1], adv=x[..., o + 2], ret=x[..., o + 3], rew=x[..., o + 4])
        G = {k: v.contiguous() for k, v in G.items()}
        G['done'] = (x[..., o + 5] != 0).to(torch.uint8)
        G['n'], G['E'] = n, E
        return G

    def iterate(self):
        """One iteration (the class docstring's steps).  Returns what PPOTrainer.iterate returns, on every
        rank alike; self.last additionally holds the gathered batch under 'gathered'."""
        from . import _lib, dist as D
        h, env = self.hyper, self.env
        sim, cur = env.sim, torch.cuda.current_stream(env.dev)
        out = env.rollout_policy(None, None, self.n_steps)
        adv, ret = env.compute_gae(out, h['gamma'], h['lam'], h['bootstrap'])
        res = {}
        if h['episode_stats']:
            row = env.episode_stats(out)
            if self.group is not None:
                rows = D.gather_rows(row[None], self.group)
                row = rows.sum(0)
                i0, i1 = _lib.EPISODE_STATS.index('ret_min'), _lib.EPISODE_STATS.index('ret_max')
                row[i0], row[i1] = rows[:, i0].min(), rows[:, i1].max()
            res['episodes'] = row
        G = self._gather_batch(out, adv, ret)
        n, E = G['n'], G['E']
        N = n * E
        if h['update_ob_rms']:
            self._update_ob_rms(G['obs'])
        epochs, M = int(h['epochs']), int(h['n_minibatch'])
        if getattr(env, '_ppo_stats', None) is None:
            env.ppo_reset()
        perm = torch.stack([torch.randperm(N, device=env.dev, generator=self.generator) for _ in range(epochs)]).to(torch.int32).contiguous()
        batch = sim.ppo_batch(n, E, **{k: G[k].data_ptr() for k in ('obs', 'act', 'logp', 'value', 'adv', 'ret')})
        P = sim.ppo_params(h)
        mine = self._segs if self.group is None else self._segs[self.segments[0]:self.segments[-1] + 1]
        env.ext.wait_stream(cur)
        sim.ppo_advstat_device(batch)
        for ep in range(epochs):
            for j in range(M):
                for i, sg in enumerate(self.segments):
                    sim.ppo_grad_segment_device(batch, P, j, M, perm[ep].data_ptr(), sg, mine[i].data_ptr())
                if self.group is not None:
                    cur.wait_stream(env.ext)
                    self._segs.copy_(D.gather_rows(mine, self.group))
                    env.ext.wait_stream(cur)
                sim.ppo_combine_device(P, self._segs.data_ptr())
                sim.ppo_adam_device(P)
        cur.wait_stream(env.ext)
        rows = min(epochs * M, _lib.PPO_STATS_ROWS)
        stats = env._ppo_stats[:rows, :len(_lib.PPO_STATS)].clone()
        self.iterations += 1
        self.last = dict(out=out, adv=adv, ret=ret, rew_norm=None, gathered=G, perm=perm)
        return dict(res, stats=stats, mean_reward=G['rew'].mean())
