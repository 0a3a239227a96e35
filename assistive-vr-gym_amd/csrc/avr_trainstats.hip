// avr_trainstats.hip -- what a trainer needs from a rollout besides the update, on the device
// (include/avr.h avr_reward_norm_device / avr_episode_stats_device): VecNormalize's reward path (each
// reward divided by the running standard deviation of the discounted return) and the statistics of
// the episodes that ended inside the rollout.  Both read the stacked [n][E] arrays of
// avr_rollout_policy_device once and carry per-env state across calls in the handle.  Included once
// per task inside the task's namespace (avr_task_tu.h) after avr_ppo.hip; nothing here depends on the
// task.
//
// Reward normalisation, four launches, parallel over the steps wherever the data allow:
//   1. avr_ts_return_scan_kernel   one thread per env walks k = 0 .. n-1 (coalesced over e):
//                                  R = R * gamma + rew[k], stored to Rk[k][e], zeroed at a done.  The
//                                  discounted return depends on no statistics, so the only sequential
//                                  part of the whole call is this scan and step 3's n scalar merges.
//   2. avr_ts_moments_kernel       one block per step: the row's mean, then its mean squared
//                                  deviation from that mean (two passes, as numpy's var).
//   3. avr_ts_merge_kernel         one thread merges the n (mean, variance) pairs into the running
//                                  statistics in order (RunningMeanStd.update's expressions) and
//                                  leaves the variance after each step in var_k[k].
//   4. avr_ts_scale_kernel         elementwise: clamp(rew / sqrt(var_k + eps), -c, c) as float.
// Eval mode (update = 0) is launch 4 alone with the handle's variance at every step.
//
// Episode statistics, two launches: avr_ts_episode_scan_kernel walks each env's steps with its
// carried accumulators in registers and leaves the env's share of the aggregate row, column-major in
// part[c][e]; avr_ts_episode_reduce_kernel folds one column per block over the envs.
//
// Determinism: no atomics.  Every thread adds in a fixed order (ascending k, or e = t, t + 256, ...),
// the blocks fold their 256 partials on one fixed tree, all in double under fp contract(off); the
// launch shapes depend on (n, E) alone.

#define TS_RED_THREADS 256                        // threads of a reduction block (a row's moments, an aggregate column)
#define TS_SCAN_THREADS 64                        // threads of a scan block: E / 64 blocks spread a 4096-env scan over 64 CUs

// the per-env episode rows (include/avr.h AVR_EPENV_*), E 4-byte words each
enum { TE_RET = AVR_EPENV_RET, TE_LEN = AVR_EPENV_LEN, TE_FORCE = AVR_EPENV_FORCE, TE_LAST_RET = AVR_EPENV_LAST_RET,
       TE_LAST_LEN = AVR_EPENV_LAST_LEN, TE_LAST_SUCCESS = AVR_EPENV_LAST_SUCCESS, TE_FINISHED = AVR_EPENV_FINISHED };
// the aggregate row's columns (include/avr.h; avr/_lib.py EPISODE_STATS)
enum { ES_EPISODES = 0, ES_RET_SUM = 1, ES_RET_SUMSQ = 2, ES_RET_MIN = 3, ES_RET_MAX = 4, ES_LEN_SUM = 5, ES_SUCCESS_SUM = 6,
       ES_FORCE_MEAN_SUM = 7, ES_STEPS = 8, ES_REW_SUM = 9 };
static_assert(ES_REW_SUM + 1 == AVR_EPSTAT_WORDS, "the aggregate row's columns");

// a[0] = the 256 entries folded on a fixed tree: op 0 sum, 1 min, 2 max (barriers at both ends)
AVR_DI void ts_tree(double *a, int t, int op) {
#pragma clang fp contract(off)
    for (int s = TS_RED_THREADS / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) a[t] = op == 0 ? a[t] + a[t + s] : (op == 1 ? fmin(a[t], a[t + s]) : fmax(a[t], a[t + s]));
    }
    __syncthreads();
}

// ------------------------------------------------------------------ reward normalisation
__global__ __launch_bounds__(TS_SCAN_THREADS) void avr_ts_return_scan_kernel(const float *__restrict__ rew, const unsigned char *__restrict__ done,
                                                                             double gamma, int n, int E, double *__restrict__ R,
                                                                             double *__restrict__ Rk) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * TS_SCAN_THREADS + threadIdx.x;
    if (e >= E) return;
    double r = R[e];
#pragma unroll 4
    for (int k = 0; k < n; k++) {
        const size_t o = (size_t)k * E + e;
        r = r * gamma + (double)rew[o];
        Rk[o] = r;
        if (done[o]) r = 0.0;                     // (after the step's statistics and scaling have seen it, as baselines does)
    }
    R[e] = r;
}

// mom[2 k] = mean_e Rk[k][e], mom[2 k + 1] = mean_e (Rk[k][e] - mean)^2; block k
__global__ __launch_bounds__(TS_RED_THREADS) void avr_ts_moments_kernel(const double *__restrict__ Rk, int E, double *__restrict__ mom) {
#pragma clang fp contract(off)
    __shared__ double sa[TS_RED_THREADS];
    const int t = threadIdx.x;
    const double *row = Rk + (size_t)blockIdx.x * E;
    double a = 0.0;
    for (int e = t; e < E; e += TS_RED_THREADS) a += row[e];
    sa[t] = a;
    ts_tree(sa, t, 0);
    const double bm = sa[0] / (double)E;
    __syncthreads();                              // (every thread has read sa[0])
    double q = 0.0;
    for (int e = t; e < E; e += TS_RED_THREADS) {
        const double d = row[e] - bm;
        q += d * d;
    }
    sa[t] = q;
    ts_tree(sa, t, 0);
    if (t == 0) {
        mom[2 * blockIdx.x] = bm;
        mom[2 * blockIdx.x + 1] = sa[0] / (double)E;
    }
}

// rms = (mean, var, count) merged with the n batches (mom[2 k], mom[2 k + 1], E) in ascending k by
// thread 0, RunningMeanStd.update's expressions in its order; var_k[k] = the variance after batch k.
// One block: its threads stage 256 steps' moments in LDS and write the 256 variances back.
__global__ __launch_bounds__(TS_RED_THREADS) void avr_ts_merge_kernel(const double *__restrict__ mom, int n, int E, double *__restrict__ rms,
                                                                      double *__restrict__ var_k) {
#pragma clang fp contract(off)
    __shared__ double sm[TS_RED_THREADS], sv[TS_RED_THREADS];
    const int t = threadIdx.x;
    double mean = 0.0, var = 0.0, count = 0.0;
    if (t == 0) { mean = rms[0]; var = rms[1]; count = rms[2]; }
    const double bc = (double)E;
    for (int base = 0; base < n; base += TS_RED_THREADS) {
        const int k = base + t, m = n - base < TS_RED_THREADS ? n - base : TS_RED_THREADS;
        if (k < n) { sm[t] = mom[2 * k]; sv[t] = mom[2 * k + 1]; }
        __syncthreads();
        if (t == 0)
            for (int j = 0; j < m; j++) {
                const double d = sm[j] - mean, tot = count + bc;
                const double new_mean = mean + d * bc / tot;
                var = (var * count + sv[j] * bc + d * d * count * bc / tot) / tot;
                mean = new_mean;
                count = tot;
                sv[j] = var;
            }
        __syncthreads();
        if (k < n) var_k[k] = sv[t];
        __syncthreads();                          // (the next chunk overwrites sm / sv)
    }
    if (t == 0) { rms[0] = mean; rms[1] = var; rms[2] = count; }
}

// out[k][e] = (float) clamp(rew[k][e] / sqrt(var[k * var_stride] + eps), -clip, clip); out may be rew
__global__ __launch_bounds__(256) void avr_ts_scale_kernel(const float *rew, const double *__restrict__ var, int var_stride, double eps, double clip,
                                                           long long N, int E, float *out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const long long k = i / E;
    const double sd = sqrt(var[k * var_stride] + eps);
    double x = (double)rew[i] / sd;
    x = x < -clip ? -clip : (x > clip ? clip : x);
    out[i] = (float)x;
}

// ------------------------------------------------------------------ episode statistics
// one thread per env, k ascending; env: the carried rows [AVR_EPENV_ROWS][E] (floats and int32s by
// row); part[c][e]: the env's share of aggregate column c over this call's steps
__global__ __launch_bounds__(TS_SCAN_THREADS) void avr_ts_episode_scan_kernel(const float *__restrict__ rew, const unsigned char *__restrict__ done,
                                                                              const float *__restrict__ info, int n, int E, float *__restrict__ env,
                                                                              double *__restrict__ part) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * TS_SCAN_THREADS + threadIdx.x;
    if (e >= E) return;
    int *envi = (int *)env;
    float ep_ret = env[(size_t)TE_RET * E + e], ep_force = env[(size_t)TE_FORCE * E + e];
    int ep_len = envi[(size_t)TE_LEN * E + e];
    float last_ret = env[(size_t)TE_LAST_RET * E + e], last_success = env[(size_t)TE_LAST_SUCCESS * E + e];
    int last_len = envi[(size_t)TE_LAST_LEN * E + e], finished = envi[(size_t)TE_FINISHED * E + e];
    double episodes = 0.0, ret_sum = 0.0, ret_sumsq = 0.0, ret_min = INFINITY, ret_max = -INFINITY, len_sum = 0.0, success_sum = 0.0,
           force_mean_sum = 0.0, rew_sum = 0.0;
#pragma unroll 4
    for (int k = 0; k < n; k++) {
        const size_t o = (size_t)k * E + e;
        const float r = rew[o], force = info[o * AVR_INFO_DIM], success = info[o * AVR_INFO_DIM + 1];
        ep_ret += r;
        ep_force += force;
        ep_len += 1;
        rew_sum += (double)r;
        if (done[o]) {
            const double ret = (double)ep_ret;
            episodes += 1.0;
            ret_sum += ret;
            ret_sumsq += ret * ret;
            ret_min = fmin(ret_min, ret);
            ret_max = fmax(ret_max, ret);
            len_sum += (double)ep_len;
            success_sum += (double)success;
            force_mean_sum += (double)ep_force / (double)ep_len;
            last_ret = ep_ret; last_len = ep_len; last_success = success;
            finished += 1;
            ep_ret = 0.f; ep_force = 0.f; ep_len = 0;
        }
    }
    env[(size_t)TE_RET * E + e] = ep_ret;
    env[(size_t)TE_FORCE * E + e] = ep_force;
    envi[(size_t)TE_LEN * E + e] = ep_len;
    env[(size_t)TE_LAST_RET * E + e] = last_ret;
    env[(size_t)TE_LAST_SUCCESS * E + e] = last_success;
    envi[(size_t)TE_LAST_LEN * E + e] = last_len;
    envi[(size_t)TE_FINISHED * E + e] = finished;
    part[(size_t)ES_EPISODES * E + e] = episodes;
    part[(size_t)ES_RET_SUM * E + e] = ret_sum;
    part[(size_t)ES_RET_SUMSQ * E + e] = ret_sumsq;
    part[(size_t)ES_RET_MIN * E + e] = ret_min;
    part[(size_t)ES_RET_MAX * E + e] = ret_max;
    part[(size_t)ES_LEN_SUM * E + e] = len_sum;
    part[(size_t)ES_SUCCESS_SUM * E + e] = success_sum;
    part[(size_t)ES_FORCE_MEAN_SUM * E + e] = force_mean_sum;
    part[(size_t)ES_STEPS * E + e] = (double)n;
    part[(size_t)ES_REW_SUM * E + e] = rew_sum;
}

// block c folds column c over the envs (sum; ret_min / ret_max: min / max) into row[c] and, when given, row2[c]
__global__ __launch_bounds__(TS_RED_THREADS) void avr_ts_episode_reduce_kernel(const double *__restrict__ part, int E, double *__restrict__ row,
                                                                               double *__restrict__ row2) {
#pragma clang fp contract(off)
    __shared__ double sa[TS_RED_THREADS];
    const int t = threadIdx.x, c = blockIdx.x;
    const int op = c == ES_RET_MIN ? 1 : (c == ES_RET_MAX ? 2 : 0);
    const double *col = part + (size_t)c * E;
    double a = op == 0 ? 0.0 : (op == 1 ? INFINITY : -INFINITY);
    for (int e = t; e < E; e += TS_RED_THREADS) a = op == 0 ? a + col[e] : (op == 1 ? fmin(a, col[e]) : fmax(a, col[e]));
    sa[t] = a;
    ts_tree(sa, t, op);
    if (t == 0) {
        row[c] = sa[0];
        if (row2) row2[c] = sa[0];
    }
}

// the state after avr_train_stats_reset that is not zero: (mean, var, count) = (0, 1, 1e-4) and the
// aggregate row of a call that closed no episode
__global__ __launch_bounds__(64) void avr_ts_init_kernel(double *__restrict__ rms, double *__restrict__ row) {
    const int t = threadIdx.x;
    if (t == 0) { rms[0] = 0.0; rms[1] = 1.0; rms[2] = 1e-4; }
    if (t < AVR_EPSTAT_WORDS) row[t] = t == ES_RET_MIN ? INFINITY : (t == ES_RET_MAX ? -INFINITY : 0.0);
}

// ------------------------------------------------------------------ launch helpers
// scratch: n * E + 3 n doubles (Rk, the moments, var_k); update 0: scratch unused, rms[1] scales every step
hipError_t avr_launch_reward_norm(const float *rew, const unsigned char *done, int n, int E, double gamma, double clip, double eps, int update,
                                  double *R, double *rms, double *scratch, float *out, hipStream_t stream) {
    const long long N = (long long)n * E;
    const double *var = rms + 1;
    if (update) {
        double *Rk = scratch, *mom = scratch + (size_t)N, *var_k = mom + 2 * (size_t)n;
        hipLaunchKernelGGL(avr_ts_return_scan_kernel, dim3((E + TS_SCAN_THREADS - 1) / TS_SCAN_THREADS), dim3(TS_SCAN_THREADS), 0, stream, rew, done,
                           gamma, n, E, R, Rk);
        hipLaunchKernelGGL(avr_ts_moments_kernel, dim3(n), dim3(TS_RED_THREADS), 0, stream, Rk, E, mom);
        hipLaunchKernelGGL(avr_ts_merge_kernel, dim3(1), dim3(TS_RED_THREADS), 0, stream, mom, n, E, rms, var_k);
        var = var_k;
    }
    hipLaunchKernelGGL(avr_ts_scale_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, rew, var, update ? 1 : 0, eps, clip, N, E, out);
    return hipGetLastError();
}

hipError_t avr_launch_episode_stats(const float *rew, const unsigned char *done, const float *info, int n, int E, float *env, double *part,
                                    double *row, double *row2, hipStream_t stream) {
    hipLaunchKernelGGL(avr_ts_episode_scan_kernel, dim3((E + TS_SCAN_THREADS - 1) / TS_SCAN_THREADS), dim3(TS_SCAN_THREADS), 0, stream, rew, done,
                       info, n, E, env, part);
    hipLaunchKernelGGL(avr_ts_episode_reduce_kernel, dim3(AVR_EPSTAT_WORDS), dim3(TS_RED_THREADS), 0, stream, part, E, row, row2);
    return hipGetLastError();
}

hipError_t avr_launch_train_stats_init(double *rms, double *row, hipStream_t stream) {
    hipLaunchKernelGGL(avr_ts_init_kernel, dim3(1), dim3(64), 0, stream, rms, row);
    return hipGetLastError();
}
