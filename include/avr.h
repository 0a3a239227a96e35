/* avr.h -- C-ABI of libavr.so, the MI355X-native replacement for the PyBullet calls on the
 * Assistive Gym step path.
 *
 * The reference reaches its physics through the PyBullet module API, one DIRECT client per env
 * (env.py:23).  One `env.step(a)` of FeedingJaco-v0 issues ~68 PyBullet calls:
 *   p.getJointStates            env.py:320-321, 393; feeding.py:126
 *   p.setJointMotorControlArray env.py:335-337
 *   p.stepSimulation  x5        env.py:342        (2 Bullet sub-steps each, feeding.py:289)
 *   p.getLinkState / multiplyTransforms / resetBasePositionAndOrientation
 *                               feeding.py:345-349 (update_targets), 124, 134
 *   p.getContactPoints          feeding.py:86-89, 111, 116
 *   p.getBasePositionAndOrientation / getBaseVelocity
 *                               feeding.py:59, 65, 100, 106, 125
 * avr_step() replaces that whole sequence for a batch of envs with one call; the task glue
 * (take_step env.py:274-351, get_total_force feeding.py:83-90, get_food_rewards :92-121,
 * _get_obs :123-142, reward :56-77, human_preferences env.py:412-448) is fused into the same
 * device launch.  The Python facade (assistive-vr-gym_amd/avr/env.py) keeps the gym
 * reset/step/observation/reward contract on top of this ABI.
 *
 * Conventions: every function returns 0 on success and a negative code on error; the message is
 * available from avr_last_error(sim).  A handle owns one HIP stream on one device and is not
 * thread-safe.  Host-pointer calls block until outputs are on the host; *_device calls take
 * device pointers and are asynchronous on avr_stream(sim).
 */
#ifndef AVR_H
#define AVR_H
#include <stddef.h>
#include <stdint.h>

#include "avr_model.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AVR_ABI_VERSION 6      /* 3: task-selected layouts (avr_model_desc.task), 5-kernel info, state getters;
                                  4: BedBathingPR2 (avr_model_desc bb_* fields, task 2);
                                  5: avr_graph_captures, per-handle device guard, t >= 0;
                                  6: avr_reset_ik self-contact screening (alt4), avr_robot_self_contact;
                                  still 6: avr_policy_set, avr_policy_act_device, avr_rollout_policy_device are new
                                  exports only -- no existing signature or state layout changed, so recordings
                                  (avr/record.py refuses another ABI number) stay valid; avr_reset_pool_set and
                                  avr_rollover_* likewise */
#define AVR_FLAGS_FAULT_MASK 0x1f  /* avr_get_flags bits 0-4; bit 5 (EPA budget) is informational */

typedef struct avr_config {
    int32_t n_envs;        /* envs owned by this handle (one GPU)                          */
    int32_t device;        /* HIP device ordinal                                           */
    int32_t env_offset;    /* global id of local env 0 (keys per-env RNG; sharding-stable)  */
    int32_t flags;         /* AVR_CFG_* bits, 0 = defaults                                  */
    uint64_t seed;         /* action RNG seed for avr_step_random (env.py:53 uses 1001)     */
} avr_config;

/* avr_config.flags: no flag is defined; avr_create rejects any set bit (bit 0 selected the
 * one-env-per-wavefront part-B kernel, removed in round 2: part B runs four envs per wavefront) */
#define AVR_CFG_RESERVED_MASK 0xffffffff

typedef struct avr_sim avr_sim;

/* Create a handle: copies the compiled scene to the device.  (replaces p.connect + the
 * loadURDF/createMultiBody/createConstraint scene build of world_creation.py:27-93)
 * model->task selects the task (AVR_TASK_FEEDING: FeedingJaco-v0, feeding.py; AVR_TASK_SCRATCH:
 * ScratchItchPR2-v0, scratch_itch.py) and with it the state layout (avr_model.h), the action and
 * observation sizes and the task glue. */
int avr_create(const avr_config *cfg, const avr_model_desc *model, avr_sim **out);
int avr_destroy(avr_sim *sim);

/* Per-env state blocks (n_envs x avr_task_state_words(task) floats, layout in avr_model.h).
 * (replaces resetJointState / resetBasePositionAndOrientation of the reset path) */
int avr_set_state(avr_sim *sim, const float *host_state);
int avr_get_state(avr_sim *sim, float *host_state);
/* Set the state of the envs whose mask byte is non-zero (auto-reset of finished episodes). */
int avr_set_state_masked(avr_sim *sim, const uint8_t *env_mask, const float *host_state);

/* n_frames x p.stepSimulation with the motors as they are, no task glue, then the reset
 * observation (feeding.py:319-320, 325).  obs may be NULL. */
int avr_settle(avr_sim *sim, int32_t n_frames, float *host_obs);

/* Episode reset of the envs whose mask byte is non-zero (mask NULL = all): their state rows
 * are taken from host_state[n_envs*STATE_WORDS] (the host reset path: scene randomisation and
 * IK, feeding.py:144-307), then n_frames x stepSimulation drop the food into the spoon
 * (feeding.py:318-320) and their reset observation goes to host_obs rows (feeding.py:325).
 * Unmasked envs and their host_obs rows are left untouched.  Replaces FeedingEnv.reset(). */
int avr_reset(avr_sim *sim, const uint8_t *env_mask, const float *host_state, int32_t n_frames, float *host_obs);

/* One gym step for every env: act[n_envs*act_dim] -> obs[n_envs*obs_dim], rew[n_envs],
 * done[n_envs] (TimeLimit 200), info[n_envs*2] = {total_force_on_human, task_success}
 * (FeedingJaco: act 7, obs 25, feeding.py:30-81; ScratchItchPR2: act 7, obs 30,
 * scratch_itch.py:30-82). */
int avr_step(avr_sim *sim, const float *act, float *obs, float *rew, uint8_t *done, float *info);
/* avr_step_device: the same with device buffers, asynchronous on avr_stream(sim).  The step's
 * launch sequence is replayed from a captured HIP graph keyed by (d_obs, d_rew, d_done, d_info,
 * mode); d_act is first copied (stream-ordered) into the handle's own action buffer, so a caller
 * may pass a fresh action buffer every step without a re-capture. */
int avr_step_device(avr_sim *sim, const float *d_act, float *d_obs, float *d_rew, uint8_t *d_done, float *d_info);
/* Same, with synthetic actions a[e,t] ~ U(-1,1)^7 drawn on the device from Philox4x32-10
 * keyed by (seed, env_offset + e, t) -- examples/random_actions.py semantics.  t >= 0 (a
 * negative t is rejected). */
int avr_step_random_device(avr_sim *sim, int64_t t, float *d_obs, float *d_rew, uint8_t *d_done, float *d_info);
/* n device-random steps t0 .. t0+n-1, bit-identical to n avr_step_random_device calls.  stacked = 0:
 * every step writes d_obs.. (NULL: the handle's buffers; the last step's outputs remain); stacked = 1:
 * step k writes slot k of d_obs[n][n_envs][obs_dim], d_rew[n][n_envs], d_done[n][n_envs],
 * d_info[n][n_envs][AVR_INFO_DIM] (all four required).  The env groups are joined every 16 steps
 * (not after every step): a group that finishes a step early starts its next one.  Asynchronous;
 * the handle's stream holds the whole rollout. */
int avr_rollout_random_device(avr_sim *sim, int64_t t0, int32_t n, float *d_obs, float *d_rew, uint8_t *d_done, float *d_info, int32_t stacked);
/* Device actions for inspection: d_act[n_envs*7] for step t (same Philox stream). */
int avr_random_actions_device(avr_sim *sim, int64_t t, float *d_act);

/* ---- the policy on the device (FeedingJaco, ScratchItchPR2, BedBathingPR2; DressingJaco: -1) ----
 * An MLP actor-critic with two tanh layers of `hidden` <= 64 units per network (the harness's
 * ActorCritic, avr/policy_eval.py: what enjoy_vr.py:80 loads and :103 calls), with VecNormalize's
 * eval-mode normalisation (enjoy_vr.py:85-88) in front:
 *   x = clip((obs - ob_mean) / sqrt(ob_var + eps), -clip_obs, clip_obs)     (ob_mean, ob_var both NULL: x = obs)
 *   mean = mu_w tanh(a_w2 tanh(a_w1 x + a_b1) + a_b2) + mu_b,  std = exp(logstd)
 *   action = mean (deterministic) or mean + std eps;  logp = sum_a -eps_a^2 / 2 - logstd_a - log(2 pi) / 2
 *   value = c_w3 tanh(c_w2 tanh(c_w1 x + c_b1) + c_b2) + c_b3                (the six c_* all NULL: value = 0)
 * eps[e][a] at step t is a Box-Muller normal from Philox4x32-10 keyed by (seed, env_offset + e, t)
 * on counters the action stream of avr_step_random_device never uses (avr/_lib.py policy_noise is
 * the host mirror).  Host pointers; matrices row-major [out][in] as torch.nn.Linear.weight. */
typedef struct avr_policy_desc {
    int32_t obs_dim, act_dim;     /* must equal the handle's task's (25 / 30 / 24, 7)                  */
    int32_t hidden;               /* 1 .. 64                                                          */
    int32_t n_layers;             /* tanh layers per network: must be 2                               */
    float clip_obs, eps;          /* VecNormalize clipob (10), epsilon (1e-8)                         */
    const float *ob_mean, *ob_var;                        /* [obs_dim]                                */
    const float *a_w1, *a_b1, *a_w2, *a_b2;               /* [hidden][obs_dim], [hidden], [hidden][hidden], [hidden] */
    const float *mu_w, *mu_b, *logstd;                    /* [act_dim][hidden], [act_dim], [act_dim]  */
    const float *c_w1, *c_b1, *c_w2, *c_b2, *c_w3, *c_b3; /* as the actor's, then [1][hidden], [1]    */
} avr_policy_desc;
/* Validate the descriptor and pack it into the handle's device weight block (allocated by the
 * first call, overwritten in stream order by later ones: the block's address never changes, so a
 * new set of weights -- a PPO update between rollouts -- needs no graph re-capture). */
int avr_policy_set(avr_sim *sim, const avr_policy_desc *policy);
/* One forward over all envs at step index t >= 0 (it keys the noise): d_obs[n_envs*obs_dim] ->
 * d_act[n_envs*act_dim], d_logp[n_envs], d_value[n_envs] (d_logp, d_value may be NULL; d_act NULL:
 * the value alone).  Asynchronous on avr_stream(sim).  An error before avr_policy_set. */
int avr_policy_act_device(avr_sim *sim, int64_t t, const float *d_obs, int32_t deterministic, float *d_act, float *d_logp, float *d_value);
/* n steps t0 .. t0+n-1 with the policy in the loop, bit-identical to n x {avr_policy_act_device(t0 + k,
 * obs_k); avr_step_device(act_k)}, with no host work per step: the forward runs between the steps
 * inside the rollout graphs of avr_rollout_random_device (per env group, joined every 16 steps).
 * d_obs0[n_envs*obs_dim] is the observation step t0's policy sees (NULL: the handle's own
 * observation buffer, as avr_reset / avr_settle / an earlier rollout left it); it is first copied
 * in stream order into that buffer.  Outputs are stacked:
 *   d_obs[n+1][n_envs][obs_dim]   slot 0 = obs0, slot k+1 = the observation after step k
 *   d_act[n][n_envs][act_dim], d_logp[n][n_envs], d_rew[n][n_envs], d_done[n][n_envs],
 *   d_info[n][n_envs][AVR_INFO_DIM]                                    one slot per step
 *   d_value[n+1][n_envs]          slot k = V(obs slot k) (the last by one value-only launch)
 * d_logp and d_value may be NULL.  No reset inside a rollout: done comes out and the caller resets
 * (as avr_rollout_random_device) -- unless the rollover mode below is on.  An error before avr_policy_set. */
int avr_rollout_policy_device(avr_sim *sim, int64_t t0, int32_t n, const float *d_obs0, int32_t deterministic, float *d_obs, float *d_act,
                              float *d_logp, float *d_value, float *d_rew, uint8_t *d_done, float *d_info);

/* ---- device-side episode rollover from a reset-state pool (FeedingJaco, ScratchItchPR2, BedBathingPR2;
 *      DressingJaco: -1) ----
 * A pool of settled reset states lives on the device; an env that finishes an episode takes its next
 * initial state from it on the device, inside the rollout's graph replay, with no host work (no
 * reference counterpart: the reference resets one env on the host, feeding.py:144-331).  The rollover
 * of env e:
 *   1. d_term_obs[e] = its d_obs row (the terminal observation);
 *   2. j = x0 % n_pool, x0 = word 0 of Philox4x32-10 on the counter {env_offset + e, (uint32)episode,
 *      0x40000000, (uint32)(episode >> 32)} with key (seed lo, seed hi), episode = d_episode[e] before
 *      the increment (the action stream's counter word 2 is 0 or 1 and the policy noise's has the top bit
 *      set: this stream shares a counter with neither; avr/_lib.py rollover_index is the host mirror);
 *   3. the env's state row = pool state j (T_ITER and T_FLAGS come from the pool row, as in a host reset);
 *   4. its d_obs row = pool observation j;
 *   5. d_episode[e] += 1.
 * done, rew and info of the finishing step stay as the step wrote them.  Integer work and copies only.
 *
 * avr_reset_pool_set: upload n_pool >= 1 reset states host_state[n_pool][avr_task_state_words] (settled
 *   states, as avr_get_state returns them after avr_reset / avr_reset_ik) and their reset observations
 *   host_obs[n_pool][obs_dim] (as the reset wrote them).  The first call allocates the pool's device
 *   block (n_pool rows) and the per-env rows of avr_rollover_buffers (zeroed); later calls overwrite the
 *   contents in stream order, and the kernels read n_pool from device memory, so a new pool needs no
 *   graph re-capture.  A later pool with more rows than the block holds is rejected (the rollout graphs
 *   hold the block's address); n_pool == 0 is an error (avr_rollover_enable(0) switches the mode off). */
int avr_reset_pool_set(avr_sim *sim, int32_t n_pool, const float *host_state, const float *host_obs);
/* avr_rollover_enable: the handle's rollover mode, off by default; an error before avr_reset_pool_set.
 *   While on, every step of avr_rollout_random_device and avr_rollout_policy_device (both replay forms
 *   and the direct loop) is followed by the rollover of the envs whose done byte that step set.  In
 *   stacked rollouts the observation slot of step k then holds, for a rolled env, the reset observation:
 *   in avr_rollout_policy_device slot k + 1 is what the policy acts on at step k + 1, so act[k + 1] and
 *   logp[k + 1] belong to obs[k + 1], done[k] = 1 marks the boundary, and the terminal observation is
 *   in d_term_obs -- of each env's most recent rollover only, when n exceeds an episode.  A non-stacked
 *   rollout leaves the reset observation in the caller's buffer.  With a critic installed,
 *   avr_rollout_policy_device ends with one value-only launch over d_term_obs into d_term_value.
 *   The mode is part of the rollout graphs' key: off and on never replay each other's graphs, and
 *   switching back and forth re-uses both.  avr_step_device and avr_step_random_device never roll over. */
int avr_rollover_enable(avr_sim *sim, int32_t on);
/* avr_rollover_device: the same operation as one call for the per-step API, asynchronous on
 *   avr_stream(sim): the envs with d_done[e] != 0 roll over and their d_obs[n_envs*obs_dim] rows are
 *   rewritten (the mode need not be on; the rollouts' direct loop is this call after every step). */
int avr_rollover_device(avr_sim *sim, const uint8_t *d_done, float *d_obs);
/* avr_rollover_buffers: device pointers owned by the handle (any may be NULL): d_term_obs[n_envs*obs_dim]
 *   the terminal observation of each env's most recent rollover (zero until the first), d_term_value
 *   [n_envs] V of it (avr_rollout_policy_device), d_episode[n_envs] the per-env episode counters. */
int avr_rollover_buffers(avr_sim *sim, float **d_term_obs, float **d_term_value, int32_t **d_episode);
/* avr_rollover_set_episodes: set the counters from host_episode[n_envs] (a facade that mixes host
 *   resets and device rollovers; blocks until done). */
int avr_rollover_set_episodes(avr_sim *sim, const int32_t *host_episode);

/* ---- the PPO update on the device (FeedingJaco, ScratchItchPR2, BedBathingPR2; DressingJaco: -1) ----
 * The consumer of avr_rollout_policy_device's batch: advantage estimation, the clipped-surrogate loss of
 * a2c_ppo_acktr's PPO.update with its backward through both networks, gradient clipping and Adam, writing
 * the handle's weight block in place in stream order on avr_stream(sim) -- the next rollout's graphs read
 * the new weights with no re-capture and no host work (csrc/avr_ppo.hip; no reference counterpart: the
 * reference ships neither its trainer nor a2c_ppo_acktr).  No float atomics: the same call on the same
 * inputs gives the same bits.  avr/ppo.py gae_reference / ppo_loss_reference are the readable mirrors.
 *
 * avr_gae_device: generalised advantage estimation over stacked device arrays d_rew[n][n_envs],
 *   d_done[n][n_envs], d_value[n+1][n_envs] into d_adv[n][n_envs], d_ret[n][n_envs], k = n-1 .. 0 per env in
 *   plain fp32 multiplies and adds in exactly this order:
 *     nv    = done[k] ? (bootstrap ? term_value[e] : 0) : value[k+1][e]
 *     delta = (rew[k] + gamma * nv) - value[k]
 *     gae   = delta + (gamma * lam) * (done[k] ? 0 : gae);   adv[k] = gae;  ret[k] = gae + value[k]
 *   Every done here is the TimeLimit: bootstrap = 1 treats it as a truncation and bootstraps from the
 *   handle's d_term_value row (avr_rollover_buffers; an error before avr_reset_pool_set), bootstrap = 0 cuts
 *   the return there, as a2c_ppo_acktr does by default.  The handle keeps only each env's most recent
 *   terminal value, so bootstrap = 1 with n > max_episode_steps (an env could finish twice) is an error. */
int avr_gae_device(avr_sim *sim, int32_t n, float gamma, float lam, int32_t bootstrap, const float *d_rew, const uint8_t *d_done,
                   const float *d_value, float *d_adv, float *d_ret);
/* A batch of N = n * E samples in device arrays, flattened [n][E] as the rollout stacks them (E need not be
 * the handle's n_envs): obs rows of obs_dim raw observations (the kernel normalises them with the weight
 * block's current ob_rms rows and clip, as the forward does; a rollout's [n+1][E] array is fine, the last
 * slot is not read), act rows of act_dim, logp / value the rollout's (value may be [n+1][E]), adv / ret
 * avr_gae_device's. */
typedef struct avr_ppo_batch {
    int32_t n, E;
    const float *obs, *act, *logp, *value, *adv, *ret;
} avr_ppo_batch;
typedef struct avr_ppo_params {
    float clip;                     /* c of the ratio clip and of the value clip                    */
    float vf_coef, ent_coef;        /* L = L_pi + vf_coef L_v - ent_coef H                           */
    float max_grad_norm;            /* global L2 clip (<= 0: none)                                   */
    float lr, beta1, beta2, eps;    /* Adam (eps > 0)                                                */
    int32_t norm_adv;               /* use (adv - mean) / (std + 1e-5), mean / std over the batch    */
    int32_t clip_value;             /* the clipped value loss (0: 0.5 mean (v - ret)^2)               */
} avr_ppo_params;
#define AVR_PPO_STAT_WORDS 8
#define AVR_PPO_STATS_ROWS 256
/* avr_ppo_reset: allocate (first call) and zero Adam's moments m, v (two blocks of the weight block's
 *   layout), the step count, the gradient block, the partials and the statistics rows.  An error before
 *   avr_policy_set.
 * avr_ppo_grad_device: the gradient of minibatch `minibatch` of n_minibatch: B = N / n_minibatch samples
 *   (the remainder is dropped), sample i of it is d_perm[minibatch * B + i] (d_perm: device int32[N] with
 *   entries in [0, N) -- an entry outside is clamped into the batch, not reported, so that nothing outside
 *   the batch is ever read; NULL: the identity).  Called with minibatch == 0 it first computes the batch's
 *   advantage mean and (unbiased) standard deviation, in double in a fixed tree, and keeps them on the
 *   device for the following minibatches (norm_adv with minibatch != 0 before minibatch 0 of the same adv
 *   array and sample count is an error).  Per sample, with mean / logstd / v the networks' outputs:
 *     logp_new = sum_a -(act_a - mean_a)^2 / (2 exp(2 logstd_a)) - logstd_a - log(2 pi) / 2
 *     ratio = exp(logp_new - logp);  L_pi = -mean(min(ratio A, clamp(ratio, 1 - c, 1 + c) A))
 *     v_clip = value + clamp(v - value, -c, c);  L_v = 0.5 mean(max((v - ret)^2, (v_clip - ret)^2))
 *     H = sum_a (0.5 + log(2 pi) / 2 + logstd_a);  L = L_pi + vf_coef L_v - ent_coef H
 *   d_grad (the weight block's layout; zero in the header and ob_rms rows and in all zero padding) receives
 *   dL / d(every weight, bias and logstd), and statistics row (minibatch % AVR_PPO_STATS_ROWS) of d_stats
 *   {L_pi, L_v, H, approx_kl = mean(logp - logp_new), clip_frac = mean(|ratio - 1| > c), grad_norm, -, -}
 *   (grad_norm by the next avr_ppo_adam_device).  vf_coef != 0 without a critic installed is an error.
 * avr_ppo_adam_device: the global L2 norm of d_grad (in double), d_grad * min(1, max_grad_norm / (norm +
 *   1e-6)), then bias-corrected Adam (torch.optim.Adam's formulas; the step count lives on the device) on
 *   the weight block in place.  Separate from the gradient call so that a caller can read or all-reduce
 *   d_grad in between.
 * avr_ppo_update_device: for every epoch, for every minibatch: the two calls above, with no host
 *   synchronisation and bit-identical to calling them one by one; d_perm is [epochs][N] (NULL: the
 *   identity each epoch); the advantage statistics are computed once, before the first minibatch;
 *   statistics row (epoch * n_minibatch + minibatch) % AVR_PPO_STATS_ROWS.
 * avr_ppo_buffers: device pointers owned by the handle (any may be NULL): d_grad, d_m, d_v (weight block
 *   layout, avr_ppo_words() floats each) and d_stats[AVR_PPO_STATS_ROWS][AVR_PPO_STAT_WORDS].
 * All are asynchronous on avr_stream(sim); all but avr_ppo_reset are errors before it. */
int avr_ppo_reset(avr_sim *sim);
int avr_ppo_grad_device(avr_sim *sim, const avr_ppo_batch *batch, const avr_ppo_params *params, int32_t minibatch, int32_t n_minibatch,
                        const int32_t *d_perm);
int avr_ppo_adam_device(avr_sim *sim, const avr_ppo_params *params);
int avr_ppo_update_device(avr_sim *sim, const avr_ppo_batch *batch, const avr_ppo_params *params, int32_t epochs, int32_t n_minibatch,
                          const int32_t *d_perm);
int avr_ppo_buffers(avr_sim *sim, float **d_grad, float **d_m, float **d_v, float **d_stats);
/* ---- the update across ranks: a minibatch in segments, combined in a fixed order ----
 * A minibatch of B samples is cut into AVR_PPO_SEGMENTS segments of B / AVR_PPO_SEGMENTS consecutive
 * minibatch positions.  The count is a constant: it never depends on how many ranks share the work.  Each
 * rank computes the rows of its own segments, the ranks exchange the rows (an all-gather; the library makes
 * no collective call itself), and every rank combines the same AVR_PPO_SEGMENTS rows in ascending order in
 * double, so the gradient, and after avr_ppo_adam_device the weights, have the same bits on every rank and
 * at every rank count that divides AVR_PPO_SEGMENTS, one process included.
 * avr_ppo_advstat_device: the batch's advantage mean and (unbiased) standard deviation, with the kernels
 *   and into the cache avr_ppo_grad_device's minibatch 0 uses (keyed by the adv pointer and sample count);
 *   only batch->n, E and adv are read.  It also restarts avr_ppo_combine_device's statistics rows at 0.
 * avr_ppo_grad_segment_device: avr_ppo_grad_device's two kernels on segment `segment` of minibatch
 *   `minibatch`: samples d_perm[minibatch * B + segment * B / 8 + i], i < B / 8, each weighted 1 / B (the whole
 *   minibatch's mean), with ent_coef taken as 0.  d_seg[AVR_PPO_SEG_WORDS] (device) receives the segment's
 *   share of dL / dw in the weight block's layout (avr_ppo_words() floats), then AVR_PPO_STAT_WORDS floats in a
 *   statistics row's layout: its share of L_pi, L_v, approx_kl and clip_frac (the H word holds the weights' H,
 *   grad_norm and the rest 0).  The handle's d_grad and statistics rows are not touched.  Errors: those of
 *   avr_ppo_grad_device, B not divisible by AVR_PPO_SEGMENTS, segment outside 0 .. AVR_PPO_SEGMENTS - 1,
 *   d_seg NULL, norm_adv without avr_ppo_advstat_device (or a minibatch 0 of avr_ppo_grad_device) on this batch.
 * avr_ppo_combine_device: d_segs[AVR_PPO_SEGMENTS][AVR_PPO_SEG_WORDS] (device, row k segment k's) into the
 *   handle's d_grad: every word the sum of the rows' words in ascending segment order in double, rounded to
 *   fp32 once, then params->ent_coef subtracted on the logstd words as avr_ppo_grad_device does; the
 *   statistics row likewise (H from the weights), row c % AVR_PPO_STATS_ROWS of d_stats for the c-th call
 *   since the last avr_ppo_advstat_device or avr_ppo_reset.  avr_ppo_adam_device follows it as it follows
 *   avr_ppo_grad_device.  avr/ppo.py combine_reference is the host mirror. */
#define AVR_PPO_SEGMENTS 8
#define AVR_PPO_SEG_WORDS (13144 + AVR_PPO_STAT_WORDS)   /* avr_ppo_words() + AVR_PPO_STAT_WORDS */
int avr_ppo_advstat_device(avr_sim *sim, const avr_ppo_batch *batch);
int avr_ppo_grad_segment_device(avr_sim *sim, const avr_ppo_batch *batch, const avr_ppo_params *params, int32_t minibatch, int32_t n_minibatch,
                                const int32_t *d_perm, int32_t segment, float *d_seg);
int avr_ppo_combine_device(avr_sim *sim, const avr_ppo_params *params, const float *d_segs);
/* Floats in the weight block (and in d_grad, d_m, d_v), and the block's device address (NULL before
 * avr_policy_set); the layout is csrc/avr_policy.hip's PW_* (avr/ppo.py mirrors it: the PW_* / PN_*
 * constants, block_live_mask, unpack_block). */
int32_t avr_ppo_words(void);
void *avr_policy_block(avr_sim *sim);
/* avr_policy_get: the inverse of avr_policy_set's packing: the weight block back into host arrays [out][in]
 *   of the installed policy's dimensions (blocks until done).  Any pointer may be NULL; the critic's arrays
 *   are left untouched without a critic, ob_mean / ob_var without ob_rms.  ob_var is a float for which
 *   avr_policy_set's sqrt(var + eps) gives back the block's divisor bit for bit, so re-installing what this
 *   call returned reproduces the block.  hidden, has_ob_rms, has_critic, clip_obs and eps are filled in. */
typedef struct avr_policy_out {
    int32_t hidden, has_ob_rms, has_critic;
    float clip_obs, eps;
    float *ob_mean, *ob_var;
    float *a_w1, *a_b1, *a_w2, *a_b2;
    float *mu_w, *mu_b, *logstd;
    float *c_w1, *c_b1, *c_w2, *c_b2, *c_w3, *c_b3;
} avr_policy_out;
int avr_policy_get(avr_sim *sim, avr_policy_out *out);
/* avr_policy_obs_norm_device: rewrite the block's ob_rms rows from device arrays d_mean[obs_dim],
 *   d_var[obs_dim] in stream order: mean, and sqrt(var + eps) with the eps of the last avr_policy_set (a
 *   trainer keeps VecNormalize's running statistics without a host round trip).  An error if the installed
 *   policy has no ob_rms. */
int avr_policy_obs_norm_device(avr_sim *sim, const float *d_mean, const float *d_var);

/* ---- reward normalisation and episode statistics on the device (FeedingJaco, ScratchItchPR2, BedBathingPR2;
 * DressingJaco: -1) ----
 * With the device rollover an env finishes and restarts inside a rollout and the host never sees an episode
 * end; these calls read the stacked arrays d_rew[n][n_envs], d_done[n][n_envs], d_info[n][n_envs]
 * [AVR_INFO_DIM] of avr_rollout_policy_device once and carry per-env state across calls in the handle, so an
 * episode may span any number of calls and an env may finish several times in one (csrc/avr_trainstats.hip;
 * avr/ppo.py reward_norm_reference / episode_stats_reference are the readable mirrors).  All are asynchronous
 * on avr_stream(sim) and belong outside any graph (a scratch buffer grows with n).  No atomics, every
 * reduction in double in a fixed order: the same call on the same inputs and carried state gives the same
 * bits.  The carried rows are allocated and reset by the first call of any of them.
 *
 * avr_reward_norm_device: the reward half of baselines' VecNormalize (the pipeline of the checkpoints
 *   enjoy_vr.py loads; the observation half is ob_rms, avr_policy_obs_norm_device).  R[n_envs] is the
 *   discounted return, a double row; (mean, var, count) its running moments, three doubles starting at
 *   (0, 1, 1e-4).  For k = 0 .. n-1 in order, in double:
 *     R[e]  = R[e] * gamma + rew[k][e]
 *     if update: bm = mean_e R, bv = mean_e (R - bm)^2, bc = n_envs
 *                d = bm - mean; tot = count + bc
 *                new_mean = mean + d * bc / tot
 *                var  = (var * count + bv * bc + d * d * count * bc / tot) / tot
 *                mean = new_mean; count = tot
 *     rew_out[k][e] = (float) clamp(rew[k][e] / sqrt(var + eps), -clip_rew, clip_rew)
 *     if done[k][e]: R[e] = 0
 *   A step's rewards are scaled with the statistics after that step's update and R is zeroed after it, as
 *   baselines does.  update = 0 is eval mode: R and the statistics stay untouched, only the scaling runs.
 *   d_rew_out may equal d_rew.  Errors: n < 1, a NULL pointer, gamma outside [0, 1], eps <= 0, clip_rew < 0.
 * avr_episode_stats_device: per env the running episode's return (float32, rewards added in ascending k),
 *   length and summed info[..][0] (total_force_on_human, float32).  At done[k][e] the episode closes with
 *   return ep_ret, length ep_len, success info[k][e][1] and mean force ep_force / ep_len (in double); the
 *   three are kept as the env's last finished episode, its counter of finished episodes goes up, and the
 *   accumulators restart at zero.  d_row (NULL: not wanted; the handle keeps the row either way) receives
 *   this call's aggregate over all episodes closed in it, AVR_EPSTAT_WORDS doubles:
 *     {episodes, ret_sum, ret_sumsq, ret_min, ret_max, len_sum, success_sum, force_mean_sum,
 *      steps = n * n_envs, rew_sum = the sum of all n * n_envs rewards}
 *   each env's share added in ascending k, the envs folded on a fixed tree.  With no episode closed ret_min
 *   = +inf and ret_max = -inf.  Errors: n < 1, d_rew / d_done / d_info NULL.
 * avr_train_stats_reset: allocate (first call) all carried rows, zero them, set the moments to (0, 1, 1e-4)
 *   and the handle's aggregate row to that of a call without episodes.
 * avr_train_stats_buffers: device pointers owned by the handle (any may be NULL; allocates and resets like
 *   the other calls when none has run): d_R[n_envs], d_rms[3] = (mean, var, count), d_env: the per-env
 *   episode rows, [AVR_EPENV_ROWS][n_envs] 4-byte words (float32 or int32 by row, AVR_EPENV_*), d_row
 *   [AVR_EPSTAT_WORDS] the last call's aggregate (what a checkpoint or a merge across ranks reads: the
 *   moments merge by the formula above). */
#define AVR_EPSTAT_WORDS 10
#define AVR_EPENV_ROWS 7
#define AVR_EPENV_RET 0           /* float32: the running episode's return so far           */
#define AVR_EPENV_LEN 1           /* int32:   its length so far                              */
#define AVR_EPENV_FORCE 2         /* float32: its summed total_force_on_human                */
#define AVR_EPENV_LAST_RET 3      /* float32: the last finished episode's return             */
#define AVR_EPENV_LAST_LEN 4      /* int32:   its length                                     */
#define AVR_EPENV_LAST_SUCCESS 5  /* float32: its task_success                               */
#define AVR_EPENV_FINISHED 6      /* int32:   episodes finished since avr_train_stats_reset  */
int avr_reward_norm_device(avr_sim *sim, int32_t n, double gamma, double clip_rew, double eps, int32_t update, const float *d_rew,
                           const uint8_t *d_done, float *d_rew_out);
int avr_episode_stats_device(avr_sim *sim, int32_t n, const float *d_rew, const uint8_t *d_done, const float *d_info, double *d_row);
int avr_train_stats_reset(avr_sim *sim);
int avr_train_stats_buffers(avr_sim *sim, double **d_R, double **d_rms, void **d_env, double **d_row);

/* ---- human height variants inside one handle (FeedingJaco, ScratchItchPR2, BedBathingPR2; DressingJaco: -1) ----
 * The reference's *New-v0 ids draw a new hipbone_to_mouth_height at every reset (feeding.py:170-172) and
 * rebuild the human (human_creation.py); here a handle holds a finite set of height variants and every env
 * picks one per episode through its state row.  The T_GENDER word of the task block is the env's
 * proportions slot: 0 and 1 are the handle's base male and female (every state from before stays valid),
 * 2 + v is variant v.  The word travels with the row, so avr_set_state, recordings, the reset pool and the
 * device rollover carry the choice with no other copy; the layouts and avr_task_state_words do not change.
 *
 * A variant carries its gender and height and the fp32 records that differ from the base scene for that
 * gender, rounded as avr_create rounds a whole scene compiled at {gender: height} (the other gender at the
 * handle's own height), so an env at variant v computes bit for bit what the same env computes in a handle
 * created from that scene:
 *   shape_pose[n_gshapes][7], shape_param[n_gshapes][4], shape_aabb[n_gshapes][6]
 *                                     the shapes with shape_gender == gender, ascending shape index
 *   body_aabb[n_hbodies][6], body_threshold[n_hbodies]
 *                                     the AVR_BODY_HUMAN bodies, ascending body index (this gender's box)
 *   hc_jpos[hc_n][3], hc_inertia[hc_n][3]   the articulated human chain's rows (NULL when hc_n == 0)
 *   bb_targets[AVR_BB_MAX_TARGETS][4] BedBathing's wipe targets of this gender (NULL for the other tasks)
 * n_gshapes and n_hbodies must equal the handle's own counts (a record compiled for another scene is refused).
 *
 * avr_human_variants_set: install n_var <= AVR_MAX_HUMAN_VARIANTS variants (replacing any earlier set;
 *   n_var = 0, v NULL: the base handle again).  Call it after avr_create and before the first state upload:
 *   the tables' device block is allocated by the first call with room for the full capacity, so a later
 *   call moves nothing a captured graph holds, but rows already on the device keep their slots and a
 *   smaller set leaves the kernels clamping them into the loaded range.
 * avr_set_state, avr_set_state_masked, avr_reset, avr_reset_ik and avr_reset_pool_set refuse (-1, message
 *   in avr_last_error, nothing launched or copied) a row whose slot is not 0, 1 or 2 + v with v < n_var.
 * With no variants loaded every kernel reads the base tables at offset 0, as before. */
#define AVR_MAX_HUMAN_VARIANTS 64
typedef struct avr_human_variant {
    int32_t gender;                 /* 0 male, 1 female                                             */
    float height;                   /* hipbone_to_mouth_height, m (reported back; not used in the step) */
    int32_t n_gshapes, n_hbodies;   /* rows in the arrays below                                     */
    const float *shape_pose, *shape_param, *shape_aabb;
    const float *body_aabb, *body_threshold;
    const float *hc_jpos, *hc_inertia;
    const float *bb_targets;
} avr_human_variant;
int avr_human_variants_set(avr_sim *sim, int32_t n_var, const avr_human_variant *v);
/* Variants loaded (0: none); avr_human_variant_info: the gender and height of variant v (either may be NULL). */
int32_t avr_human_variants(avr_sim *sim);
int avr_human_variant_info(avr_sim *sim, int32_t v, int32_t *gender, float *height);

/* One Bullet sub-step of length dt for every env, no task glue (known-answer tests). */
int avr_substep(avr_sim *sim, float dt);

int avr_sync(avr_sim *sim);
void *avr_stream(avr_sim *sim);
void *avr_state_device_ptr(avr_sim *sim);
int32_t avr_n_envs(avr_sim *sim);
/* Env groups whose launch sequences run concurrently on separate streams inside each step call
 * (one per 1024 envs, at most 4; AVR_ENV_GROUPS=1..8 in the environment at avr_create overrides).
 * Results do not depend on it.  No reference counterpart (diagnostic). */
int32_t avr_env_groups(avr_sim *sim);
/* 1 when the handle's sub-steps run the dynamics role in the pair launch (unconstrained velocities
 * and non-contact rows beside the pair enumeration instead of inside kernel a; FeedingJaco's
 * default, AVR_DYN_SPLIT=0|1 in the environment at avr_create overrides), else 0.  Results do not
 * depend on it.  No reference counterpart (diagnostic). */
int32_t avr_dyn_split(const avr_sim *sim);
/* 1 when the pair kernel enumerates the child shape pairs in flat passes over all active body pairs
 * (the task's default, AVR_PAIRS_FLAT=0|1 in the environment at avr_create overrides), else 0.
 * The pair list is the same set in the same order either way.  No reference counterpart (diagnostic). */
int32_t avr_pairs_flat(const avr_sim *sim);
/* 1 when the narrowphase's sphere-hull blocks start the shape pairs that hold a point in the env's
 * contact pool before the others (the task's default, AVR_NP_HOT=0|1 in the environment at avr_create
 * overrides), else 0: list order.  Results are stored by pair index and do not depend on it.  No
 * reference counterpart (diagnostic). */
int32_t avr_np_hot(const avr_sim *sim);
/* 1 when the wave-cooperative narrowphase (EPA, the GJK reruns in double, big hulls) takes a hull's
 * support point wave-wide: a hull of at most 64 vertices one vertex per lane from registers, a larger
 * table hull its cell's candidates one per lane (the task's default, AVR_COOP_WSUP=0|1 in the
 * environment at avr_create overrides), else 0: the serial scans.  The support vertex, and so every
 * result, is the same either way.  No reference counterpart (diagnostic). */
int32_t avr_coop_wsup(const avr_sim *sim);
/* Graph captures made by this handle so far (each distinct step key captures once; a few keys
 * are cached).  No reference counterpart (diagnostic). */
int64_t avr_graph_captures(avr_sim *sim);
int32_t avr_state_words(void);          /* FeedingJaco's: avr_task_state_words(AVR_TASK_FEEDING) */
int32_t avr_abi_version(void);
/* Per-task sizes (-1 for an unknown task) and the handle's task. */
int32_t avr_task_state_words(int32_t task);
int32_t avr_task_obs_dim(int32_t task);
int32_t avr_task_act_dim(int32_t task);
int32_t avr_task(avr_sim *sim);
/* Kernel resource usage: [vgprs, 0, lds_bytes, scratch_bytes] of each kernel of a step, in
 * launch order: pairs (kinematics, broadphase, shape-pair list), narrowphase, a (the
 * wave-cooperative GJK/EPA of the rare pairs that need it, manifolds, dynamics, constraint rows),
 * b (PGS + integration), task (the task glue after the frames): out20 holds 5 x 4 ints. */
int avr_kernel_info(avr_sim *sim, int32_t *out20);

/* ---- state queries (device-side gathers; host buffers; block until done) ----
 * The reference reads these through PyBullet every step; here they come out of the state without
 * copying the whole state block to the host.
 * avr_get_q: joint positions / velocities of every articulated DoF, q[n_envs*n_dof],
 *   qd[n_envs*n_dof] (either may be NULL), n_dof = avr_n_dof(sim): the robot's DoFs in URDF DFS
 *   order, then the articulated human chain's (zeros while that chain is static).
 *   Replaces p.getJointStates(robot | human, ...)[0:2] (env.py:320-321, feeding.py:126,
 *   scratch_itch.py:109). */
int32_t avr_n_dof(avr_sim *sim);
int avr_get_q(avr_sim *sim, float *q, float *qd);
/* avr_get_link_pose: world COM frame (x y z, qx qy qz qw) of articulated link `link` of every
 *   env, out7[n_envs*7]; link < 0 selects the robot base.  Forward kinematics on the current
 *   joint positions, as p.getLinkState(robot, link, computeForwardKinematics=True)[0:2]
 *   (feeding.py:124, scratch_itch.py:105; link indices are the compiled robot's, URDF DFS order
 *   within the simulated subtree). */
int avr_get_link_pose(avr_sim *sim, int32_t link, float *out7);
/* avr_get_contact_summary: per env, out4[n_envs*4] = {contact points, sum of normalForce over all
 *   points, over robot-human points, over tool-human points} of the last sub-step's contact set:
 *   the sums p.getContactPoints(...)[9] feeds to get_total_force (feeding.py:83-90,
 *   scratch_itch.py:84-102). */
int avr_get_contact_summary(avr_sim *sim, float *out4);
/* avr_get_flags: per-env health flags, flags[n_envs] (bit0 NaN / failed mass-matrix
 *   factorisation, bit1 contact pool full, bit2 AABB pair list full, bit3 shape pair list full,
 *   bit4 non-contact row buffer full, bit5 more than AVR_COOP_CAP = 4 penetrating hull pairs in
 *   one sub-step: the EPA ran on a rotating window of 4 of them, the others kept their manifold
 *   points -- informational, the env's state is finite); 0 = healthy.  AVR_FLAGS_FAULT_MASK
 *   selects the fault bits (0-4).  No reference counterpart (PyBullet has no
 *   such report); a vectorised trainer polls it instead of the whole state block. */
int avr_get_flags(avr_sim *sim, int32_t *flags);
const char *avr_last_error(avr_sim *sim);

/* ---- views of the envs: ray-cast depth, shape ids and RGB (FeedingJaco, ScratchItchPR2, BedBathingPR2;
 *      DressingJaco: -1) ----
 * The reference shows its world only through Bullet's GUI (env.py:613-620, record_video_frame :606-608);
 * p.getCameraImage is the PyBullet call these replace.  csrc/avr_render.hip; new exports only.
 *
 * Rendered geometry: the env's collision shapes as its narrowphase addresses them -- the shapes whose
 * shape_gender is -1 or the gender of the env's proportions slot (T_GENDER), with shape_pose and
 * shape_param from that slot's row of the per-variant tables (avr_human_variants_set) -- at the body COM
 * frames the CURRENT state gives: ROBOT links and an articulated human chain by forward kinematics on
 * S_Q, FREE bodies from S_FREE, HUMAN slots from S_HUMAN, STATIC bodies from st_pose, RSTATIC bodies at
 * the robot base.  The frames come from the device code with which a sub-step's pair kernel fills its
 * body-frame table, run on the state as it is now (the table itself is one sub-step old and is not read).
 *   sphere   shape_param[0] = radius
 *   capsule  shape_param[0] = radius, [1] = half height, axis along the shape frame's z
 *   box      shape_param[0..2] = half extents
 *   hull     the convex hull of its hull_verts (the core, without the 1 mm collision margin), as the face
 *            planes n . x <= w installed by avr_render_set_planes
 * A body whose shapes are parked far away (eaten food) is simply out of view.
 *
 * Camera: a pinhole with square pixels.  With f = unit(target - eye), right = unit(f x up), upv = right x f,
 * the ray through the centre of pixel (row r, column c), row 0 at the top, starts at eye along
 *   d = unit(f + x right + y upv),  x = (2 c + 1 - width) k,  y = (height - 2 r - 1) k,  k = tan(fov_y / 2) / height.
 * body = -1: eye, target, up are world coordinates; body >= 0: they are given in that collision body's COM
 * frame of each rendered env (the head slot's body: the participant's view; the tool body: a wrist camera).
 *
 * A hit of a ray is a point where it ENTERS a shape (the surface faces the ray) at a parameter t in
 * [near, far]; a shape that contains the eye, or whose facing surface is nearer than `near`, is not seen.
 * Outputs per rendered env, row-major [height][width]:
 *   depth  float32: t of the nearest hit, metres along the unit ray; +inf for a miss
 *   id     int32: the hit shape's index in the model's shape arrays, -1 for a miss; of two shapes at an
 *          equal t the lower index wins
 *   rgb    uint8 [height][width][3]: round_to_nearest(palette[kind] * (0.3 + 0.7 max(0, -n . d))), n the outward
 *          surface normal at the hit, palette by the hit body's kind: robot and robot-fixed (190, 195, 205),
 *          free bodies / the tool (240, 200, 60), human (230, 170, 140), static (140, 150, 160); a miss is
 *          (204, 230, 255), the reference GUI's background (env.py:618).  No textures, visual meshes or shadows.
 * Nothing is written to the handle's state, workspace or graphs: a render between two steps leaves every
 * later result bit-identical. */
typedef struct avr_camera {
    float eye[3], target[3], up[3];
    float fov_y_deg;                /* vertical field of view, in (0, 180)                          */
    float near, far;                /* 0 < near < far: hits outside [near, far] are not seen        */
    int32_t width, height;          /* 1 .. 4096 each                                               */
    int32_t body;                   /* -1: world frame; else a collision body index                 */
    int32_t reserved[3];            /* 0                                                            */
} avr_camera;
/* Collision bodies of the handle's scene. */
int32_t avr_n_bodies(avr_sim *sim);
/* avr_get_body_poses: the world COM frame (x y z, qx qy qz qw) of every collision body of every env as
 *   defined above, out[n_envs][avr_n_bodies][7] on the host (blocks until done): the counterpart of
 *   p.getBasePositionAndOrientation / p.getLinkState for all bodies at once, and what the renderer
 *   places the shapes at. */
int avr_get_body_poses(avr_sim *sim, float *out);
/* avr_render_set_planes: install the hulls' face planes: planes4[n_planes][4] = (n, w) with unit n in the
 *   shape's frame, shape_range2[n_shapes][2] = (first plane, plane count) per shape, count 0 for shapes
 *   that are no hull and >= 4 for every hull (host arrays; avr/render.py hull_planes builds them from
 *   hull_verts).  The planes belong to the base hulls; height variants move and scale shapes through
 *   shape_pose / shape_param only.  A later call replaces the set (the call waits for the stream). */
int avr_render_set_planes(avr_sim *sim, int32_t n_planes, const float *planes4, const int32_t *shape_range2);
/* avr_render_device: render the n envs env_ids[0 .. n-1] (a host array, validated and copied in; NULL: envs
 *   0 .. n-1; repeats allowed, the order is the output order) through *cam into the device buffers
 *   d_depth[n][height][width], d_id[n][height][width], d_rgb[n][height][width][3]; any of the three may be
 *   NULL, not all.  Queued on avr_stream(sim); the call does not wait for the images.  Two things can
 *   make the host wait all the same: a call that needs more scratch than any before it (more envs or more
 *   shapes) frees and reallocates it, which waits for the device, and the copy of a non-NULL env_ids reads
 *   the caller's pageable array, which the runtime may finish before it returns (the array is free to
 *   change once the call is back).  env_ids NULL and a steady n have neither.
 *   Errors (-1, message in avr_last_error, nothing launched): cam NULL; width or height < 1 or > 4096;
 *   fov_y_deg outside (0, 180); near <= 0 or far <= near; a degenerate view (target == eye, up zero or
 *   parallel to the view direction) or a non-finite field; n < 1 or n > 65535; an env id outside
 *   0 .. n_envs-1; body outside -1 .. avr_n_bodies-1; all three outputs NULL; a scene with hulls before
 *   avr_render_set_planes. */
int avr_render_device(avr_sim *sim, const avr_camera *cam, int32_t n, const int32_t *env_ids, float *d_depth, int32_t *d_id, uint8_t *d_rgb);
/* Diagnostics of the renderer (no reference counterpart; tools/render_bench.py reads them, nothing else
 * needs them).
 * avr_render_tile_stats: what the tile culling of avr_render_device leaves for the same
 *   arguments: host_stats[n][tiles][2] = {shapes in the tile's culled list, hull planes a pixel of the tile
 *   tests}, tiles = ceil(width / 8) * ceil(height / 8), row-major over the tile grid (blocks until done).  It
 *   runs both launches of a render with no image written.
 * avr_render_kernel_info: out8 = [vgprs, 0, lds_bytes, scratch_bytes] of the frame and the trace kernel. */
int avr_render_tile_stats(avr_sim *sim, const avr_camera *cam, int32_t n, const int32_t *env_ids, int32_t *host_stats);
int avr_render_kernel_info(avr_sim *sim, int32_t *out8);

/* ---- device reset (FeedingJaco) ----
 * avr_reset_ik: avr_reset with the reset's inverse kinematics on the device.  Replaces the IK of
 *   FeedingEnv.reset (feeding.py:276-278 -> util.py:34-105 ik_random_restarts) for the masked envs:
 *   host_state rows carry everything the host reset draws (human pose, bowl, impairment, motors;
 *   the arm's joints are overwritten); target7[n_envs*7] is the tool link's COM-frame target
 *   (position, quaternion); init[n_envs*restarts*n_arm] the arm's starting joints of every
 *   restart (drawn by the host from the env's reset stream).  Per env, restarts run in order
 *   with `iters` damped-least-squares updates each until one lands within `tol` (position, m, and
 *   quaternion distance, or a distance within tol of 2: util.py:49) with no robot hull vertex
 *   inside the keep-out box keepout8 = {center xyz, pad, half extents xyz, pad} (NULL: no
 *   screening); else the joints of the restart closest to the target position are kept
 *   (util.py:51-54).  step_sim's self-contact screening (util.py:41-46): alt4[n_envs*restarts*4]
 *   (NULL: none) holds per restart the re-drawn target orientation (the original's Euler angles
 *   +- 45 deg, drawn by the host); a restart whose solution has robot links touching (as
 *   avr_robot_self_contact) switches the target orientation to its alt4 entry, for its own
 *   acceptance check and the later restarts.
 *   The spoon and the food are then placed on the tool frame (world_creation.py:330-343,
 *   feeding.py:291-308) and n_frames settle frames run (feeding.py:319-320), as in avr_reset.
 *   host_ok[n_envs] (may be NULL) receives 1 where a restart was accepted.  Returns -1 for tasks
 *   other than FeedingJaco. */
int avr_reset_ik(avr_sim *sim, const uint8_t *env_mask, const float *host_state, const float *target7, const float *init, const float *alt4,
                 int32_t restarts, int32_t iters, float tol, const float *keepout8, int32_t n_frames, float *host_obs, uint8_t *host_ok);

/* avr_robot_self_contact: len(p.getContactPoints(bodyA=robot, bodyB=robot)) > 0 (util.py:41-46,
 *   63-67) at n joint vectors q[n*avr_n_dof], evaluated at the joint vector itself: the reference
 *   asks after a restart's 5 simulated frames, which are not simulated here -- a known difference,
 *   the same on the host and device IK paths (avr_get_q's layout; everything
 *   else from env 0's state block): out[n] = the robot shape pairs the step's collision pipeline finds
 *   within their contact threshold (compiled robot-robot candidate pairs: the URDF's
 *   URDF_USE_SELF_COLLISION robots, parent-child pairs excluded).  Host screening of the host IK
 *   path (avr/reset.py ik_batch); avr_reset_ik runs the same test on the device. */
int avr_robot_self_contact(avr_sim *sim, int32_t n, const float *q, int32_t *out);

/* avr_narrowphase_query (test hook): the step's narrowphase between shapes pairs[2i] and
 *   pairs[2i+1] (indices into the model's shapes) on body poses poses14[14i..] (A's body:
 *   position, quaternion xyzw; then B's), contact threshold thr -> out8[8i..] = {rc (0 none,
 *   1 contact, 2 unresolved), normal on B xyz, point on B xyz, signed distance}.  The shape-level
 *   counterpart of p.getClosestPoints / the contact a pair adds to its manifold (btGjkEpa2 [ext]);
 *   lets the GJK / EPA be checked against the oracle pair by pair.  Runs the pair as the step
 *   does: a pair whose fp32 lane GJK stalls with an open duality gap is answered by the
 *   cooperative GJK with the double simplex solve, every other pair by the cooperative fp32 path. */
int avr_narrowphase_query(avr_sim *sim, int32_t n, const int32_t *pairs, const float *poses14, float thr, float *out8);
/* avr_narrowphase_query_slots: the same with a proportions slot per query (slots[n]: 0, 1 or 2 + v of a
 *   loaded height variant, avr_human_variants_set): query i's shapes are read from that variant's tables.
 *   FeedingJacoNew-v0's reset asks it for p.getClosestPoints(human, robot, 0.05) (feeding.py:238): the
 *   human shapes of the env's variant against the robot's at the IK pose (avr/reset.py human_robot_distance).
 *   A slot that is not loaded is refused (-1). */
int avr_narrowphase_query_slots(avr_sim *sim, int32_t n, const int32_t *pairs, const float *poses14, const int32_t *slots, float thr, float *out8);

/* avr_bb_closest_query (test hook, BedBathingPR2): min p.getClosestPoints(tool, human, 4.0)[8]
 *   (bed_bathing.py:61) of every env's current state, computed by the step's own code in the
 *   step's two parts: the lane and wave-cooperative narrowphase over the tool x human shape pairs,
 *   which queues the pairs whose fp32 lane GJK stalls with an open duality gap in the env's
 *   workspace, then the queue's rerun with the double simplex solve.  The counterpart of the
 *   oracle's avr_oracle_bb_closest; no step is taken, and state, observation and reward buffers are
 *   not touched.  out4[4e..] = {the final minimum, the number of queued pairs, the minimum before
 *   the rerun (the lane and cooperative pairs only), the number of stalled pairs past the queue's
 *   capacity (the rerun finds them again with the lane GJK and gives them the double solve as
 *   well)}; "no pair within reach" reads as the query
 *   distance 4.0, as in the reward.  cap limits the queue for this call: 0 <= cap <= the step's
 *   capacity (60), negative = the step's.  Returns -1 for the other tasks. */
int avr_bb_closest_query(avr_sim *sim, int32_t cap, float *out4);

/* ---- device base-pose search (ScratchItchPR2, BedBathingPR2) ----
 * avr_base_search: position_robot_toc (env.py:489-585; scratch_itch.py:189-190,
 *   bed_bathing.py:317) for n envs on the device, one lane per (env, attempt).  Host buffers:
 *   base7[n*attempts*7] each attempt's robot base pose (position, quaternion xyzw; the host draws
 *   the random offset and yaw, env.py:509-511), rest[n*attempts*n_arm] its IK rest pose
 *   (util.py:99), tstart3[n*3] the start goal of the tool link's COM (identity orientation),
 *   goals9[n*9] the shoulder, elbow and wrist positions.  Per attempt: damped-least-squares IK
 *   (`iters` updates, util.py:59-74 ik_jlwki with success threshold `tol`) to the start goal --
 *   missed: the attempt is discarded -- then to each human goal; reached goals add their
 *   joint-limit-weighted kinematic isotropy (env.py:536-553).  Per env the best attempt (most
 *   goals, then manipulability, the first on ties; none reaching the start goal: the closest)
 *   goes to best[n], ok[n] (1: start goal reached) and q_arm[n*n_arm] (its start-goal joints).
 *   res4[n*attempts*4] (may be NULL) receives every attempt's {goals reached or -1,
 *   manipulability, start position error, start quaternion distance}.  The state is not touched.
 *   Returns -1 for FeedingJaco (fixed base). */
int avr_base_search(avr_sim *sim, int32_t n, int32_t attempts, const float *base7, const float *rest, const float *tstart3,
                    const float *goals9, int32_t iters, float tol, int32_t *best, uint8_t *ok, float *q_arm, float *res4);

/* Per-kernel timing on the handle's stream: while enabled, every launch of a step/settle is
 * bracketed by HIP events (adds a little launch overhead; off by default).  avr_kernel_times
 * returns the accumulated milliseconds and launch counts per kernel kind
 * [take_step, substep_a, substep_b, task, substep_pairs, narrowphase, -, -] since enabling
 * (synchronises the stream). */
int avr_profile_kernels(avr_sim *sim, int32_t enable);
int avr_kernel_times(avr_sim *sim, double *ms8, int64_t *count8);

/* Diagnostics (phase-timer builds only, -DAVR_PROF): attach a device buffer of
 * [n_envs][16] uint64 cycle counters.  A no-op for the shipped kernel. */
int avr_set_profile_buffer(avr_sim *sim, void *d_prof);

/* Support-mapping table of one convex hull (host-only utility; avr_create builds one for every
 * hull with more than AVR_TAB_MIN_NV vertices).  Cube map of 6*G*G direction cells; cell c lists,
 * in ascending vertex order, every vertex that can be the support point (first strictly largest
 * projection, as Bullet's btConvexHullShape scan) for some direction of the cell:
 * cell[2c] = offset into idx, cell[2c+1] = count.  idx receives at most cap entries.  Returns the
 * total entry count (allocate that many and call again), or -1 on bad arguments.  Replaces the
 * per-query full vertex scan behind btConvexHullShape::localGetSupportingVertexWithoutMargin
 * (reached from p.stepSimulation, env.py:342) with an exact sub-linear lookup. */
int32_t avr_hull_support_table(const float *verts, int32_t nv, int32_t G, int32_t *cell, int32_t *idx, int32_t cap);

#ifdef __cplusplus
}
#endif
#endif
