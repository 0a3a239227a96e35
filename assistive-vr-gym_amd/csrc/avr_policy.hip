// avr_policy.hip -- the policy on the device: an MLP actor-critic forward (avr/policy_eval.py
// ActorCritic + VecNormalize's eval-mode normalisation) that runs between the steps of a rollout
// graph (avr_rollout_policy_device, avr_capi.hip).  Included once per task inside the task's
// namespace (avr_task_tu.h): K_OBS_DIM / K_ACT_DIM are the task's.
//
// Mapping: one wavefront per block serves POL_EPW = 8 envs.  Lane j owns hidden unit j of the
// layer being computed and carries one accumulator per env, so every weight is loaded once per
// wavefront (row k of the transposed matrix: 64 consecutive floats, one coalesced load) and feeds
// 8 FMAs; the previous layer's activations of the 8 envs sit in LDS and are read at the same
// address by all lanes (broadcast, 16 bytes at a time).  The actor and the critic run one after
// the other through the same code.  The 7 action heads and the value head are 64-term dot
// products again: lane 8 e + a computes head a of env e (a = 7: the value), so the whole forward,
// heads included, is sums of fmaf in ascending-k order, which a host mirror can follow; only the
// log-prob's sum over the action dimensions is a cross-lane (xor butterfly) sum.
// Arithmetic: explicit fmaf under fp contract(off), accurate tanhf / expf / logf / sinf / cosf.
//
// Noise: eps[env][a] at step t is a Box-Muller normal from philox4x32_10 keyed by
// (seed, env_offset + env, t) as the action stream is, with the top bit of counter word c[2] set:
// philox_action's c[2] is j >> 2, which never has it, so the two streams never share a counter.
// Block b = a >> 2 yields four words; (x0, x1) make the pair for a & 3 = 0 (cos) and 1 (sin),
// (x2, x3) the pair for a & 3 = 2 (cos) and 3 (sin): u1 = ((x >> 8) + 0.5) / 2^24 in fp32 (never
// 0; the sum rounds to nearest even above 2^23), u2 = (x' >> 8) / 2^24, eps = sqrt(-2 ln u1) *
// cos | sin (2 pi u2).  _lib.policy_noise is the host mirror.

#define POL_H 64                                  // hidden units per layer (capacity; narrower layers are zero-padded)
#define POL_EPW 8                                 // envs per wavefront
#define POL_KO4 ((K_OBS_DIM + 3) & ~3)            // observation words, rounded up to whole float4s
#define POL_XS (POL_KO4 + 4)                      // LDS row stride of the staged observations
#define POL_HS (POL_H + 4)                        // LDS row stride of the activations: the 8 envs' rows start 4 banks apart
#define POL_NS (POL_EPW * POL_HS + 16)            // the critic's activations start 16 banks after the actor's (head reads: no conflict)

// the handle's device weight block (floats); matrices are stored transposed, [in][POL_H]
enum {
    PW_HDR = 0,                                   // {has ob_rms, has critic, clip_obs, -, -, -, -, -}
    PW_MEAN = 8,                                  // [32] ob_rms mean
    PW_SD = PW_MEAN + 32,                         // [32] sqrt(ob_rms var + eps)
    PW_LOGSTD = PW_SD + 32,                       // [8]
    PW_BH = PW_LOGSTD + 8,                        // [8] head biases: mu_b[0..6], the critic's last bias
    PW_WH = PW_BH + 8,                            // [POL_H][8] head weights: columns 0..6 mu_w rows, column 7 the critic's last layer
    PW_NET = PW_WH + POL_H * 8,                   // the actor's, then the critic's, two tanh layers:
    PN_W1 = 0,                                    //   [32][POL_H]
    PN_B1 = PN_W1 + 32 * POL_H,                   //   [POL_H]
    PN_W2 = PN_B1 + POL_H,                        //   [POL_H][POL_H]
    PN_B2 = PN_W2 + POL_H * POL_H,                //   [POL_H]
    PN_WORDS = PN_B2 + POL_H,
    PW_WORDS = PW_NET + 2 * PN_WORDS
};
enum { POL_DETERMINISTIC = 1, POL_VALUE_ONLY = 2 };

static_assert(K_OBS_DIM <= 32 && K_ACT_DIM <= 7, "avr_policy: observation / action capacity");

struct __attribute__((aligned(16))) PolicyLDS {
    float x[POL_EPW][POL_XS];                     // normalised observations
    float h[2 * POL_NS];                          // [actor, critic][env][POL_HS] activations of the layer just computed
};

// eps of action dimension j of (global) env `env` at step t
AVR_DI float philox_normal(unsigned long long seed, int env, long long t, int j) {
#pragma clang fp contract(off)
    unsigned c[4] = {(unsigned)env, (unsigned)t, 0x80000000u | (unsigned)(j >> 2), (unsigned)((unsigned long long)t >> 32)};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned xa = (j & 2) ? c[2] : c[0], xb = (j & 2) ? c[3] : c[1];
    const float u1 = ((float)(xa >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = (float)(xb >> 8) * (1.0f / 16777216.0f);
    const float r = sqrtf(-2.0f * logf(u1));
    const float th = 6.283185307179586f * u2;
    return r * ((j & 1) ? sinf(th) : cosf(th));
}

// one tanh layer for the wavefront's 8 envs: acc[e] = b[lane] + sum_k WT[k][lane] in[e][k], k ascending
template <int K, int STRIDE>
AVR_DI void policy_layer(const float *__restrict__ WT, const float *__restrict__ b, const float *in, int lane, float acc[POL_EPW]) {
#pragma clang fp contract(off)
    const float b0 = b[lane];
#pragma unroll
    for (int e = 0; e < POL_EPW; e++) acc[e] = b0;
#pragma unroll 4
    for (int k = 0; k < K; k += 4) {
        const float w0 = WT[(k + 0) * POL_H + lane], w1 = WT[(k + 1) * POL_H + lane], w2 = WT[(k + 2) * POL_H + lane],
                    w3 = WT[(k + 3) * POL_H + lane];
#pragma unroll
        for (int e = 0; e < POL_EPW; e++) {
            const float4 v = *(const float4 *)(in + e * STRIDE + k);
            acc[e] = fmaf(w0, v.x, acc[e]);
            acc[e] = fmaf(w1, v.y, acc[e]);
            acc[e] = fmaf(w2, v.z, acc[e]);
            acc[e] = fmaf(w3, v.w, acc[e]);
        }
    }
}

// envs [env0, env1): obs -> action (mean, or mean + std eps), log-prob, value.  t < 0: the step
// index is env group -t - 1's device counter (a rollout graph's node, as avr_take_step_kernel).
// act / logp / value are [E]-row buffers (logp, value may be NULL; POL_VALUE_ONLY writes value
// alone); o_act / o_logp / o_value (each may be NULL) are stacked [n][E] arrays of which slot
// *kslot (NULL: slot 0) receives the same results.
__global__ __launch_bounds__(64) void avr_policy_act_kernel(const float *__restrict__ W, const long long *__restrict__ step_t, long long t,
                                                            unsigned long long seed, int env_offset, const float *__restrict__ obs,
                                                            float *__restrict__ act, float *__restrict__ logp, float *__restrict__ value,
                                                            float *__restrict__ o_act, float *__restrict__ o_logp, float *__restrict__ o_value,
                                                            const long long *__restrict__ kslot, int E, int flags, int env0, int env1) {
#pragma clang fp contract(off)
    __shared__ PolicyLDS L;
    const int lane = threadIdx.x;
    const int eb = env0 + blockIdx.x * POL_EPW;
    const bool has_norm = W[PW_HDR] != 0.f, has_critic = W[PW_HDR + 1] != 0.f, value_only = (flags & POL_VALUE_ONLY) != 0;
    const float clip = W[PW_HDR + 2];
    if (t < 0) t = step_t[-t - 1];
    for (int i = lane; i < POL_EPW * POL_KO4; i += 64) {
        const int e = i / POL_KO4, k = i - e * POL_KO4, env = eb + e;
        float x = 0.f;
        if (k < K_OBS_DIM && env < env1) {
            x = obs[(size_t)env * K_OBS_DIM + k];
            if (has_norm) x = clampf((x - W[PW_MEAN + k]) / W[PW_SD + k], -clip, clip);     // policy_eval.normalize
        }
        L.x[e][k] = x;
    }
    __syncthreads();
#pragma unroll 1
    for (int net = value_only ? 1 : 0; net < (has_critic ? 2 : 1); net++) {
        const float *Wn = W + PW_NET + net * PN_WORDS;
        float *hn = L.h + net * POL_NS;
        float acc[POL_EPW];
        policy_layer<POL_KO4, POL_XS>(Wn + PN_W1, Wn + PN_B1, &L.x[0][0], lane, acc);
#pragma unroll
        for (int e = 0; e < POL_EPW; e++) hn[e * POL_HS + lane] = tanhf(acc[e]);
        __syncthreads();
        policy_layer<POL_H, POL_HS>(Wn + PN_W2, Wn + PN_B2, hn, lane, acc);
        __syncthreads();                          // (every lane has read the first layer's activations)
#pragma unroll
        for (int e = 0; e < POL_EPW; e++) hn[e * POL_HS + lane] = tanhf(acc[e]);
    }
    __syncthreads();
    // heads: lane 8 e + a; a < K_ACT_DIM the action means on the actor's activations, a = 7 the value on the critic's
    const int e = lane >> 3, a = lane & 7, env = eb + e;
    const bool is_v = a == 7, is_a = a < K_ACT_DIM && !value_only;
    float out = 0.f;
    if (is_v ? has_critic : is_a) {
        const float *hv = L.h + (is_v ? POL_NS : 0) + e * POL_HS;
        out = W[PW_BH + a];
#pragma unroll 8
        for (int k = 0; k < POL_H; k++) out = fmaf(W[PW_WH + k * 8 + a], hv[k], out);
    }
    float action = out, term = 0.f;
    if (is_a) {
        // ActorCritic.act's log-prob with action - mean = std eps: -eps^2 / 2 - logstd - log(2 pi) / 2 per dimension
        const float ls = W[PW_LOGSTD + a];
        float eps = 0.f;
        if (!(flags & POL_DETERMINISTIC)) {
            eps = philox_normal(seed, env_offset + env, t, a);
            action = fmaf(expf(ls), eps, out);
        }
        term = -0.5f * eps * eps - ls - 0.9189385332046727f;
    }
    term += __shfl_xor(term, 1, 64);
    term += __shfl_xor(term, 2, 64);
    term += __shfl_xor(term, 4, 64);
    if (env >= env1) return;
    const size_t so = (size_t)(kslot ? *kslot : 0) * E + env;
    if (is_a) {
        act[(size_t)env * K_ACT_DIM + a] = action;
        if (o_act) o_act[so * K_ACT_DIM + a] = action;
        if (a == 0) {
            if (logp) logp[env] = term;
            if (o_logp) o_logp[so] = term;
        }
    }
    if (is_v) {
        if (value) value[env] = out;
        if (o_value) o_value[so] = out;
    }
}

hipError_t avr_launch_policy(const float *W, const long long *step_t, long long t, unsigned long long seed, int env_offset, const float *obs, float *act,
                             float *logp, float *value, float *o_act, float *o_logp, float *o_value, const long long *kslot, int E, int flags, int env0,
                             int env1, hipStream_t stream) {
    if (env1 <= env0) return hipSuccess;
    hipLaunchKernelGGL(avr_policy_act_kernel, dim3((env1 - env0 + POL_EPW - 1) / POL_EPW), dim3(64), 0, stream, W, step_t, t, seed, env_offset, obs, act,
                       logp, value, o_act, o_logp, o_value, kslot, E, flags, env0, env1);
    return hipGetLastError();
}
