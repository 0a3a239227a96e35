// avr_rollover.hip -- device-side episode rollover from a reset-state pool (include/avr.h
// avr_reset_pool_set / avr_rollover_*): an env whose step set its done byte takes its next initial
// state from a device-resident pool of settled reset states, inside the same rollout graph replay.
// Included once per task inside the task's namespace (avr_task_tu.h): K_STATE_WORDS / K_OBS_DIM are
// the task's.
//
// The pool block (one allocation, its address baked into the rollout graphs):
//   words 0..3   header {n_pool, capacity (rows), -, -} as int32: the kernels read both from here, so a
//                later avr_reset_pool_set with another n_pool needs no re-capture
//   then         states [capacity][K_STATE_WORDS]   (16-byte aligned rows where K_STATE_WORDS % 4 == 0)
//   then         observations [capacity][K_OBS_DIM]
//
// Rollover of env e (integer work and copies only, no floating-point arithmetic):
//   term_obs[e] = obs[e];  j = x0 % n_pool with x0 = word 0 of philox4x32_10 on the counter
//   {env_offset + e, (u32)episode, 0x40000000, (u32)(episode >> 32)}, key (seed lo, seed hi), episode =
//   episode[e];  state[e] = pool state j (T_ITER, T_FLAGS included);  obs[e] = pool observation j;
//   episode[e] += 1.  philox_action's counter word 2 is 0 or 1 and philox_normal's has the top bit
//   set, so this stream shares a counter with neither.  _lib.rollover_index is the host mirror.
//
// Mapping: one wavefront per env.  Finishing envs are rare: a wave whose env is not done loads the
// done byte and leaves (the stacked variant first copies the env's W = K_OBS_DIM + 4 output words
// to the rollout slot, one lane each).  A rolled env's wave copies the 1.4k - 1.9k state words in
// coalesced 64-lane strides, 16 bytes per lane where the layout allows (FeedingJaco: 1900 words),
// dwords otherwise (the PR2 layout: 1361 words); decided statically per task.  All lanes that need
// episode[e] belong to the one wave that also increments it, after its own (single-instruction)
// load: no other wave reads or writes the counter during the launch.

#define ROLL_HDR 4                                // header words in front of the pool's states
#define ROLL_V4 (K_STATE_WORDS % 4 == 0)          // 16-byte copies: whole float4s per row, rows 16-byte aligned
#define ROLL_EPB 4                                // envs (wavefronts) per 256-thread block

static_assert(K_OBS_DIM <= 32 && AVR_INFO_DIM + 2 <= 32, "avr_rollover: one wavefront holds an env's output words");

// the whole wave of env `env` calls this; returns the pool observation word of lane < K_OBS_DIM
// (what obs[env][lane] now holds), 0 for the other lanes
AVR_DI float rollover_env(const float *__restrict__ pool, unsigned long long seed, int env_offset, float *__restrict__ state, float *obs,
                          float *__restrict__ term_obs, int *episode, int env, int lane) {
    const long long ep = episode[env];            // (every lane, before lane 0's store below)
    const unsigned n_pool = ((const unsigned *)pool)[0], cap = ((const unsigned *)pool)[1];
    if (n_pool == 0u || n_pool > cap) return 0.f; // (never installed so: avr_reset_pool_set rejects both)
    unsigned c[4] = {(unsigned)(env_offset + env), (unsigned)ep, 0x40000000u, (unsigned)((unsigned long long)ep >> 32)};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned j = c[0] % n_pool;
    const float *src = pool + ROLL_HDR + (size_t)j * K_STATE_WORDS;
    float *dst = state + (size_t)env * K_STATE_WORDS;
#if ROLL_V4
    for (int i = lane; i < K_STATE_WORDS / 4; i += 64) ((float4 *)dst)[i] = ((const float4 *)src)[i];
#else
    for (int i = lane; i < K_STATE_WORDS; i += 64) dst[i] = src[i];
#endif
    float v = 0.f;
    if (lane < K_OBS_DIM) {
        const size_t o = (size_t)env * K_OBS_DIM + lane;
        term_obs[o] = obs[o];
        v = pool[ROLL_HDR + (size_t)cap * K_STATE_WORDS + (size_t)j * K_OBS_DIM + lane];
        obs[o] = v;
    }
    if (lane == 0) episode[env] = (int)ep + 1;
    return v;
}

// envs [env0, env1) with done[env] != 0 roll over; their obs rows become the pool's reset observations
// (non-stacked rollouts, avr_rollover_device)
__global__ __launch_bounds__(64 * ROLL_EPB) void avr_rollover_kernel(const float *__restrict__ pool, unsigned long long seed, int env_offset,
                                                                     float *__restrict__ state, const unsigned char *__restrict__ done, float *obs,
                                                                     float *__restrict__ term_obs, int *episode, int env0, int env1) {
    const int lane = threadIdx.x & 63, env = env0 + blockIdx.x * ROLL_EPB + (threadIdx.x >> 6);
    if (env >= env1 || !done[env]) return;
    (void)rollover_env(pool, seed, env_offset, state, obs, term_obs, episode, env, lane);
}

// a stacked rollout with the rollover mode on: avr_rollout_copy_kernel's slot copy of the step just
// taken (envs [env0, env1), the handle's output rows to slot *kslot of the caller's [n][E][...]
// arrays) and the rollover of the envs that step finished, in the one launch a stacked step already
// has.  A rolled env's slot (and the handle's obs row, which the next forward reads) receives the
// reset observation; rew, done and info stay the finishing step's.
__global__ __launch_bounds__(64 * ROLL_EPB) void avr_rollover_copy_kernel(const long long *__restrict__ kslot, const float *__restrict__ pool,
                                                                          unsigned long long seed, int env_offset, float *__restrict__ state, float *obs,
                                                                          const float *__restrict__ rew, const unsigned char *__restrict__ done,
                                                                          const float *__restrict__ info, float *__restrict__ term_obs, int *episode,
                                                                          float *__restrict__ o_obs, float *__restrict__ o_rew,
                                                                          unsigned char *__restrict__ o_done, float *__restrict__ o_info, int env0, int env1,
                                                                          int E) {
    const int lane = threadIdx.x & 63, env = env0 + blockIdx.x * ROLL_EPB + (threadIdx.x >> 6);
    if (env >= env1) return;
    const size_t o = (size_t)*kslot * E + env;
    const unsigned char d = done[env];
    const int w = lane - 32;                      // lanes 32 ..: info words, rew, done
    if (w >= 0 && w < AVR_INFO_DIM) o_info[o * AVR_INFO_DIM + w] = info[(size_t)env * AVR_INFO_DIM + w];
    else if (w == AVR_INFO_DIM) o_rew[o] = rew[env];
    else if (w == AVR_INFO_DIM + 1) o_done[o] = d;
    float v = 0.f;
    if (!d) {
        if (lane < K_OBS_DIM) v = obs[(size_t)env * K_OBS_DIM + lane];
    } else {
        v = rollover_env(pool, seed, env_offset, state, obs, term_obs, episode, env, lane);
    }
    if (lane < K_OBS_DIM) o_obs[o * K_OBS_DIM + lane] = v;
}

hipError_t avr_launch_rollover(const float *pool, unsigned long long seed, int env_offset, float *state, const unsigned char *done, float *obs,
                               float *term_obs, int *episode, int env0, int env1, hipStream_t stream) {
    if (env1 <= env0) return hipSuccess;
    hipLaunchKernelGGL(avr_rollover_kernel, dim3((env1 - env0 + ROLL_EPB - 1) / ROLL_EPB), dim3(64 * ROLL_EPB), 0, stream, pool, seed, env_offset, state,
                       done, obs, term_obs, episode, env0, env1);
    return hipGetLastError();
}

hipError_t avr_launch_rollover_copy(const long long *kslot, const float *pool, unsigned long long seed, int env_offset, float *state, float *obs,
                                    const float *rew, const unsigned char *done, const float *info, float *term_obs, int *episode, float *o_obs,
                                    float *o_rew, unsigned char *o_done, float *o_info, int env0, int env1, int E, hipStream_t stream) {
    if (env1 <= env0) return hipSuccess;
    hipLaunchKernelGGL(avr_rollover_copy_kernel, dim3((env1 - env0 + ROLL_EPB - 1) / ROLL_EPB), dim3(64 * ROLL_EPB), 0, stream, kslot, pool, seed,
                       env_offset, state, obs, rew, done, info, term_obs, episode, o_obs, o_rew, o_done, o_info, env0, env1, E);
    return hipGetLastError();
}
