// avr_ppo.hip -- the PPO update on the device (include/avr.h avr_gae_device / avr_ppo_*): advantage
// estimation over a rollout's stacked arrays, the clipped-surrogate loss of a minibatch with its
// backward through both 64-unit tanh networks, and gradient clipping + Adam writing the handle's
// weight block (avr_policy.hip PW_*) in place.  Included once per task inside the task's namespace
// (avr_task_tu.h) after avr_policy.hip: K_OBS_DIM / K_ACT_DIM are the task's.
//
// Gradient kernel mapping: the forward's.  One wavefront per block takes 8 samples per pass of a
// grid-stride loop; blockIdx.y selects the network (0 the actor with the action heads and logstd,
// 1 the critic with the value head): the loss couples the two only through the sum, so each block
// runs one network's forward and backward and the two halves of the grid never meet.  Lane j owns
// hidden unit j: it computes the unit's activation for the 8 samples (policy_layer, the forward's
// own fmaf chains), its back-propagated delta, and carries column j of both weight-gradient
// matrices in registers for the whole launch (dW2[k][j], k < 64, and dW1[k][j], k < POL_KO4: 92 -
// 96 accumulators), adding the 8 samples of a pass in ascending order.  The other operand of every
// product -- the previous layer's activations, the next layer's deltas -- sits in LDS and is read
// at one address by all lanes (broadcast, 16 bytes at a time).  The one transposed product,
// dh1[k] = sum_j W2[k][j] dz2[j], reads row k of the second layer from an LDS copy with a row
// stride of 65 words: lane k's word j is at bank (k + j) % 32, distinct over a 32-lane group.  The
// heads work as in the forward: lane 8 e + a is head a of sample e.
//
// Determinism: no atomics.  A block adds its samples in a fixed order and writes one partial (one
// network's PPO_PART words); avr_ppo_reduce_kernel adds the partials of a word in ascending block
// order (in double, rounded to fp32 once); the number of blocks is min(ceil(B / 8),
// PPO_MAX_BLOCKS), a function of the minibatch size alone.  The statistics and the gradient norm
// are accumulated in double, in fixed trees.
//
// Across ranks (avr_ppo_grad_segment_device / avr_ppo_combine_device): the same two kernels run on an
// eighth of a minibatch at a time and avr_ppo_combine_kernel adds the eight results in ascending
// order in double, so ranks that share the eight segments among them arrive at the same gradient
// bits as one process that computes all eight.
//
// Padding: hidden units beyond `hidden`, observation rows beyond K_OBS_DIM and head column 7
// without a critic have zero inputs or zero outgoing weights, so every product that forms their
// gradient has an exactly-zero factor and the sums are exactly zero; Adam then moves them by
// lr * 0 / (sqrt(0) + eps) = 0.
// Arithmetic: explicit fmaf under fp contract(off), accurate tanhf / expf / logf.

#define PPO_MAX_BLOCKS 512                        // gradient blocks per network (partials per word)
#define PPO_W2S (POL_H + 1)                       // row stride of the LDS copy of the second layer
#define PPO_STAT_WORDS 8                          // floats per statistics row
#define PPO_STATS_ROWS 256                        // statistics rows the handle keeps (a ring)
#define PPO_ADV_BLOCKS 256                        // blocks (partials) of the advantage statistics, at most
#define PPO_SEGMENTS AVR_PPO_SEGMENTS             // segments of a minibatch (avr_ppo_grad_segment_device): fixed, whatever the rank count
#define PPO_SEG_WORDS (PW_WORDS + PPO_STAT_WORDS) // floats of a segment row: the gradient block, then a statistics row's words

// one network's partial: [8] logstd, [8] head biases, [POL_H][8] head weights, then the network (PN_*)
enum { PP_LOGSTD = 0, PP_BH = 8, PP_WH = 16, PP_NET = 16 + POL_H * 8, PPO_PART = PP_NET + PN_WORDS };
enum { PS_LPI = 0, PS_LV = 1, PS_H = 2, PS_KL = 3, PS_CLIPFRAC = 4, PS_GNORM = 5 };

struct PpoArgs {
    const float *obs, *act, *logp, *value, *adv, *ret;   // the flattened [N] batch (obs rows K_OBS_DIM, act rows K_ACT_DIM)
    const int *perm;                                      // sample s of the minibatch is perm[base + s] (NULL: base + s)
    long long base, N;
    int B;
    float clip, vf_coef, inv_B;
    int norm_adv, clip_value;
};

// ------------------------------------------------------------------ advantage estimation
// one thread per env, k = n-1 .. 0; plain multiplies and adds in the order a float32 host mirror
// follows (avr/ppo.py gae_reference); term_value NULL: a done cuts the return
__global__ __launch_bounds__(256) void avr_gae_kernel(const float *__restrict__ rew, const unsigned char *__restrict__ done,
                                                      const float *__restrict__ value, const float *__restrict__ term_value, float gamma, float gl,
                                                      int n, int E, float *__restrict__ adv, float *__restrict__ ret) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const float tv = term_value ? term_value[e] : 0.f;
    float gae = 0.f, vnext = value[(size_t)n * E + e];
    for (int k = n - 1; k >= 0; k--) {
        const size_t o = (size_t)k * E + e;
        const bool d = done[o] != 0;
        const float v = value[o];
        const float nv = d ? tv : vnext;
        const float delta = (rew[o] + gamma * nv) - v;
        gae = delta + gl * (d ? 0.f : gae);
        adv[o] = gae;
        ret[o] = gae + v;
        vnext = v;
    }
}

// ------------------------------------------------------------------ advantage statistics
AVR_DI void ppo_tree256(double *a, double *b, int t) {
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) { a[t] += a[t + s]; b[t] += b[t + s]; }
    }
    __syncthreads();
}

// partial sums (sum, sum of squares) of adv[N] in double: part[2 b], part[2 b + 1]
__global__ __launch_bounds__(256) void avr_ppo_advstat_kernel(const float *__restrict__ adv, long long N, double *__restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double sa[256], sq[256];
    const int t = threadIdx.x;
    double a = 0.0, q = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + t; i < N; i += (long long)gridDim.x * 256) {
        const double x = (double)adv[i];
        a += x;
        q += x * x;
    }
    sa[t] = a; sq[t] = q;
    ppo_tree256(sa, sq, t);
    if (t == 0) { part[2 * blockIdx.x] = sa[0]; part[2 * blockIdx.x + 1] = sq[0]; }
}

// out[0] = mean, out[1] = standard deviation (unbiased, as torch.Tensor.std) over the nb <= 256 partials
__global__ __launch_bounds__(256) void avr_ppo_advstat_final_kernel(const double *__restrict__ part, int nb, long long N, float *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double sa[256], sq[256];
    const int t = threadIdx.x;
    sa[t] = t < nb ? part[2 * t] : 0.0;
    sq[t] = t < nb ? part[2 * t + 1] : 0.0;
    ppo_tree256(sa, sq, t);
    if (t == 0) {
        const double mean = sa[0] / (double)N;
        double var = N > 1 ? (sq[0] - sa[0] * mean) / (double)(N - 1) : 0.0;
        if (!(var > 0.0)) var = 0.0;
        out[0] = (float)mean;
        out[1] = (float)sqrt(var);
    }
}

// ------------------------------------------------------------------ the minibatch gradient
struct __attribute__((aligned(16))) PpoLDS {
    float x[POL_EPW][POL_XS];                     // normalised observations
    float h1[POL_EPW][POL_HS], h2[POL_EPW][POL_HS];   // the two layers' activations
    float dz[POL_EPW][POL_HS];                    // the second layer's pre-activation deltas
    float d1[POL_EPW][POL_HS];                    // the first layer's
    float dout[POL_EPW][8];                       // the heads' deltas
    float w2[POL_H * PPO_W2S];                    // the second layer's weights, rows 65 words apart
};

AVR_DI long long ppo_index(const PpoArgs &A, int s) {
    long long i = A.base + s;
    if (A.perm) i = A.perm[i];
    return i < 0 ? 0 : (i >= A.N ? A.N - 1 : i);  // (a permutation's entries are in [0, N); nothing outside the batch is read)
}

__global__ __launch_bounds__(64) void avr_ppo_grad_kernel(const float *__restrict__ W, const PpoArgs A, const float *__restrict__ advstat,
                                                          float *__restrict__ part, double *__restrict__ spart) {
#pragma clang fp contract(off)
    __shared__ PpoLDS L;
    const int lane = threadIdx.x, net = blockIdx.y;
    float *P = part + ((size_t)blockIdx.x * 2 + net) * PPO_PART;
    double *SP = spart + ((size_t)blockIdx.x * 2 + net) * PPO_STAT_WORDS;
    const bool has_norm = W[PW_HDR] != 0.f, has_critic = W[PW_HDR + 1] != 0.f;
    if (net == 1 && !has_critic) {                // no critic: its words (head column 7 included) get zero partials
        for (int i = lane; i < PPO_PART; i += 64) P[i] = 0.f;
        if (lane < PPO_STAT_WORDS) SP[lane] = 0.0;
        return;
    }
    const float clipo = W[PW_HDR + 2];
    const float *Wn = W + PW_NET + net * PN_WORDS;
    for (int i = lane; i < POL_H * POL_H; i += 64) L.w2[(i >> 6) * PPO_W2S + (i & 63)] = Wn[PN_W2 + i];
    const int he = lane >> 3, ha = lane & 7;      // head role: sample row he of the pass, head ha
    const bool head_on = net ? ha == 7 : ha < K_ACT_DIM;
    float wh[8];                                  // hidden role: head weights of unit `lane`
    {
        const float4 w0 = *(const float4 *)(W + PW_WH + lane * 8), w1 = *(const float4 *)(W + PW_WH + lane * 8 + 4);
        wh[0] = w0.x; wh[1] = w0.y; wh[2] = w0.z; wh[3] = w0.w; wh[4] = w1.x; wh[5] = w1.y; wh[6] = w1.z; wh[7] = w1.w;
    }
    const float bh = W[PW_BH + ha], ls = net ? 0.f : W[PW_LOGSTD + ha];
    const float inv_var = expf(-2.f * ls);
    const float a_mean = advstat[0], a_sd = advstat[1] + 1e-5f;
    float aW1[POL_KO4], aW2[POL_H], aWH[8], ab1 = 0.f, ab2 = 0.f, abh = 0.f, als = 0.f;
#pragma unroll
    for (int k = 0; k < POL_KO4; k++) aW1[k] = 0.f;
#pragma unroll
    for (int k = 0; k < POL_H; k++) aW2[k] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; i++) aWH[i] = 0.f;
    double st_l = 0.0, st_kl = 0.0, st_cf = 0.0;  // this lane's sums of the loss term, logp_old - logp_new, clipped
    __syncthreads();
#pragma unroll 1
    for (int g = blockIdx.x; g * POL_EPW < A.B; g += gridDim.x) {
        for (int i = lane; i < POL_EPW * POL_KO4; i += 64) {
            const int e = i / POL_KO4, k = i - e * POL_KO4, s = g * POL_EPW + e;
            float x = 0.f;
            if (k < K_OBS_DIM && s < A.B) {
                x = A.obs[(size_t)ppo_index(A, s) * K_OBS_DIM + k];
                if (has_norm) x = clampf((x - W[PW_MEAN + k]) / W[PW_SD + k], -clipo, clipo);     // as avr_policy_act_kernel
            }
            L.x[e][k] = x;
        }
        __syncthreads();
        float acc[POL_EPW], h1[POL_EPW], h2[POL_EPW];
        policy_layer<POL_KO4, POL_XS>(Wn + PN_W1, Wn + PN_B1, &L.x[0][0], lane, acc);
#pragma unroll
        for (int e = 0; e < POL_EPW; e++) { h1[e] = tanhf(acc[e]); L.h1[e][lane] = h1[e]; }
        __syncthreads();
        policy_layer<POL_H, POL_HS>(Wn + PN_W2, Wn + PN_B2, &L.h1[0][0], lane, acc);
#pragma unroll
        for (int e = 0; e < POL_EPW; e++) { h2[e] = tanhf(acc[e]); L.h2[e][lane] = h2[e]; }
        __syncthreads();
        // heads (lane 8 e + a) and the loss's derivative with respect to them
        const int s = g * POL_EPW + he;
        const bool live = s < A.B;
        const size_t idx = (size_t)ppo_index(A, live ? s : 0);
        float out = 0.f, dout = 0.f;
        if (head_on) {
            out = bh;
#pragma unroll 8
            for (int k = 0; k < POL_H; k++) out = fmaf(W[PW_WH + k * 8 + ha], L.h2[he][k], out);
        }
        if (net == 0) {
            float d = 0.f, term = 0.f;
            if (head_on) {
                d = A.act[idx * K_ACT_DIM + ha] - out;
                term = -0.5f * (d * d) * inv_var - ls - 0.9189385332046727f;
            }
            term += __shfl_xor(term, 1, 64);
            term += __shfl_xor(term, 2, 64);
            term += __shfl_xor(term, 4, 64);
            const float lp_old = A.logp[idx];
            const float ratio = expf(term - lp_old);
            float adv = A.adv[idx];
            if (A.norm_adv) adv = (adv - a_mean) / a_sd;
            const float rc = clampf(ratio, 1.f - A.clip, 1.f + A.clip);
            const float s1 = ratio * adv, s2 = rc * adv;
            // d min(s1, s2) / d ratio: adv inside the clip range (both terms are the ratio's) or where the
            // unclipped term is the smaller, 0 where the clipped one is
            const float gr = (rc == ratio || s1 < s2) ? adv : 0.f;
            const float glp = live ? -(gr * ratio) * A.inv_B : 0.f;       // dL / d logp_new
            if (head_on) {
                dout = glp * (d * inv_var);
                als = fmaf(glp, (d * d) * inv_var - 1.f, als);
            }
            if (live && ha == 0) {
                st_l -= (double)fminf(s1, s2);
                st_kl += (double)(lp_old - term);
                st_cf += fabsf(ratio - 1.f) > A.clip ? 1.0 : 0.0;
            }
        } else if (head_on && live) {
            const float r = A.ret[idx], g1 = out - r, l1 = g1 * g1;
            float gv = g1, lv = l1;
            if (A.clip_value) {
                const float vo = A.value[idx], dv = out - vo;
                const float g2 = (vo + clampf(dv, -A.clip, A.clip)) - r, l2 = g2 * g2;
                const float g2m = fabsf(dv) <= A.clip ? g2 : 0.f;         // (the clamp passes no gradient outside its range)
                gv = l1 > l2 ? g1 : (l2 > l1 ? g2m : 0.5f * (g1 + g2m));
                lv = fmaxf(l1, l2);
            }
            dout = (A.vf_coef * gv) * A.inv_B;
            st_l += 0.5 * (double)lv;
        }
        abh += dout;
        L.dout[he][ha] = dout;
        __syncthreads();
        // head weights: word lane + 64 i of the [POL_H][8] block is unit he + 8 i, head ha
#pragma unroll
        for (int i = 0; i < 8; i++)
#pragma unroll
            for (int e = 0; e < POL_EPW; e++) aWH[i] = fmaf(L.h2[e][he + 8 * i], L.dout[e][ha], aWH[i]);
        // second layer's deltas of unit `lane`
        float dz2[POL_EPW];
#pragma unroll
        for (int e = 0; e < POL_EPW; e++) {
            const float4 d0 = *(const float4 *)&L.dout[e][0], d1 = *(const float4 *)&L.dout[e][4];
            float t = wh[0] * d0.x;
            t = fmaf(wh[1], d0.y, t); t = fmaf(wh[2], d0.z, t); t = fmaf(wh[3], d0.w, t);
            t = fmaf(wh[4], d1.x, t); t = fmaf(wh[5], d1.y, t); t = fmaf(wh[6], d1.z, t); t = fmaf(wh[7], d1.w, t);
            dz2[e] = t * (1.f - h2[e] * h2[e]);
            L.dz[e][lane] = dz2[e];
            ab2 += dz2[e];
        }
        __syncthreads();
        // dW2[k][lane] += sum_e h1[e][k] dz2[e] (one sample row at a time: 16 broadcast reads live, not 128)
#pragma unroll 1
        for (int e = 0; e < POL_EPW; e++) {
            const float dze = L.dz[e][lane];
#pragma unroll
            for (int k = 0; k < POL_H; k += 4) {
                const float4 v = *(const float4 *)&L.h1[e][k];
                aW2[k + 0] = fmaf(v.x, dze, aW2[k + 0]);
                aW2[k + 1] = fmaf(v.y, dze, aW2[k + 1]);
                aW2[k + 2] = fmaf(v.z, dze, aW2[k + 2]);
                aW2[k + 3] = fmaf(v.w, dze, aW2[k + 3]);
            }
        }
        // first layer's deltas of unit `lane`: dh1 = sum_j W2[lane][j] dz2[j], j ascending
        float dz1[POL_EPW];
#pragma unroll
        for (int e = 0; e < POL_EPW; e++) dz1[e] = 0.f;
#pragma unroll 4
        for (int j = 0; j < POL_H; j += 4) {
            const float w0 = L.w2[lane * PPO_W2S + j], w1 = L.w2[lane * PPO_W2S + j + 1], w2 = L.w2[lane * PPO_W2S + j + 2],
                        w3 = L.w2[lane * PPO_W2S + j + 3];
#pragma unroll
            for (int e = 0; e < POL_EPW; e++) {
                const float4 v = *(const float4 *)&L.dz[e][j];
                dz1[e] = fmaf(w0, v.x, dz1[e]);
                dz1[e] = fmaf(w1, v.y, dz1[e]);
                dz1[e] = fmaf(w2, v.z, dz1[e]);
                dz1[e] = fmaf(w3, v.w, dz1[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < POL_EPW; e++) {
            dz1[e] = dz1[e] * (1.f - h1[e] * h1[e]);
            ab1 += dz1[e];
            L.d1[e][lane] = dz1[e];               // (read back by this lane alone)
        }
        // dW1[k][lane] += sum_e x[e][k] dz1[e]
#pragma unroll 1
        for (int e = 0; e < POL_EPW; e++) {
            const float d1e = L.d1[e][lane];
#pragma unroll
            for (int k = 0; k < POL_KO4; k += 4) {
                const float4 v = *(const float4 *)&L.x[e][k];
                aW1[k + 0] = fmaf(v.x, d1e, aW1[k + 0]);
                aW1[k + 1] = fmaf(v.y, d1e, aW1[k + 1]);
                aW1[k + 2] = fmaf(v.z, d1e, aW1[k + 2]);
                aW1[k + 3] = fmaf(v.w, d1e, aW1[k + 3]);
            }
        }
        __syncthreads();                          // (every lane is done with this pass's LDS rows)
    }
    // the head lanes' sums over the 8 sample rows (lanes of equal ha), then the block's partial
    abh += __shfl_xor(abh, 8, 64);  abh += __shfl_xor(abh, 16, 64);  abh += __shfl_xor(abh, 32, 64);
    als += __shfl_xor(als, 8, 64);  als += __shfl_xor(als, 16, 64);  als += __shfl_xor(als, 32, 64);
    if (lane < 8) { P[PP_LOGSTD + lane] = als; P[PP_BH + lane] = abh; }
#pragma unroll
    for (int i = 0; i < 8; i++) P[PP_WH + lane + 64 * i] = aWH[i];
    float *Pn = P + PP_NET;
#pragma unroll
    for (int k = 0; k < 32; k++) Pn[PN_W1 + k * POL_H + lane] = k < POL_KO4 ? aW1[k < POL_KO4 ? k : 0] : 0.f;
    Pn[PN_B1 + lane] = ab1;
#pragma unroll
    for (int k = 0; k < POL_H; k++) Pn[PN_W2 + k * POL_H + lane] = aW2[k];
    Pn[PN_B2 + lane] = ab2;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        st_l += __shfl_xor(st_l, m, 64);
        st_kl += __shfl_xor(st_kl, m, 64);
        st_cf += __shfl_xor(st_cf, m, 64);
    }
    if (lane == 0) {
        SP[0] = st_l; SP[1] = st_kl; SP[2] = st_cf;
        for (int i = 3; i < PPO_STAT_WORDS; i++) SP[i] = 0.0;
    }
}

// grad[w] = the sum of word w's partials in ascending block order (the entropy bonus's constant
// derivative added to logstd); the statistics row of this minibatch
__global__ __launch_bounds__(256) void avr_ppo_reduce_kernel(const float *__restrict__ part, const double *__restrict__ spart, int nb,
                                                             const float *__restrict__ W, float ent_coef, float inv_B, float *__restrict__ grad,
                                                             float *__restrict__ stats) {
#pragma clang fp contract(off)
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < PW_WORDS) {
        int net = 0, off = -1;
        if (w < PW_LOGSTD) off = -1;              // header, ob_rms: no gradient
        else if (w < PW_BH) off = PP_LOGSTD + (w - PW_LOGSTD);
        else if (w < PW_WH) { net = (w - PW_BH) == 7; off = PP_BH + (w - PW_BH); }
        else if (w < PW_NET) { net = ((w - PW_WH) & 7) == 7; off = PP_WH + (w - PW_WH); }
        else { net = (w - PW_NET) >= PN_WORDS; off = PP_NET + (w - PW_NET) - net * PN_WORDS; }
        float g = 0.f;
        if (off >= 0) {
            // (in double, rounded once: the sum over up to 512 partials adds no fp32 rounding of its own)
            const float *p = part + (size_t)net * PPO_PART + off;
            double a = 0.0;
#pragma unroll 8
            for (int b = 0; b < nb; b++) a += (double)p[(size_t)b * 2 * PPO_PART];
            g = (float)a;
        }
        if (w >= PW_LOGSTD && w < PW_LOGSTD + K_ACT_DIM) g = g - ent_coef;       // d(-ent_coef H) / d logstd_a
        grad[w] = g;
    }
    if (blockIdx.x == 0 && threadIdx.x < 5) {
        const int t = threadIdx.x;
        float r;
        if (t == PS_H) {
            r = 0.f;
            for (int a = 0; a < K_ACT_DIM; a++) r += 0.5f + 0.9189385332046727f + W[PW_LOGSTD + a];
        } else {
            const int net = t == PS_LV, slot = t == PS_KL ? 1 : t == PS_CLIPFRAC ? 2 : 0;
            double a = 0.0;
            for (int b = 0; b < nb; b++) a += spart[((size_t)b * 2 + net) * PPO_STAT_WORDS + slot];
            r = (float)(a * (double)inv_B);
        }
        stats[t] = r;
    }
}

// ------------------------------------------------------------------ the segments of a minibatch, combined
// A minibatch is cut into PPO_SEGMENTS runs of consecutive minibatch positions; the two kernels above
// run on one run at a time (A.B the run's length, A.inv_B the whole minibatch's, ent_coef 0) and write a
// segment row: the weight block's PW_WORDS gradient words, then the reduce kernel's statistics words.
// This kernel adds the rows of a minibatch: word w of `grad` is the sum of the rows' word w in ascending
// segment order in double, rounded to fp32 once, with the entropy bonus's constant derivative on logstd
// as avr_ppo_reduce_kernel adds it; the statistics likewise, H from the weights.  The count of segments
// is a constant, so the sum does not depend on who computed which row.
__global__ __launch_bounds__(256) void avr_ppo_combine_kernel(const float *__restrict__ segs, const float *__restrict__ W, float ent_coef,
                                                              float *__restrict__ grad, float *__restrict__ stats) {
#pragma clang fp contract(off)
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < PW_WORDS) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < PPO_SEGMENTS; k++) a += (double)segs[(size_t)k * PPO_SEG_WORDS + w];
        float g = (float)a;
        if (w >= PW_LOGSTD && w < PW_LOGSTD + K_ACT_DIM) g = g - ent_coef;       // d(-ent_coef H) / d logstd_a
        grad[w] = g;
    }
    if (blockIdx.x == 0 && threadIdx.x < 5) {
        const int t = threadIdx.x;
        float r;
        if (t == PS_H) {
            r = 0.f;
            for (int a = 0; a < K_ACT_DIM; a++) r += 0.5f + 0.9189385332046727f + W[PW_LOGSTD + a];
        } else {
            double a = 0.0;
            for (int k = 0; k < PPO_SEGMENTS; k++) a += (double)segs[(size_t)k * PPO_SEG_WORDS + PW_WORDS + t];
            r = (float)a;
        }
        stats[t] = r;
    }
}

// ------------------------------------------------------------------ gradient clipping and Adam
struct PpoAdam { float max_grad_norm, lr, beta1, beta2, eps; };

// one block: the gradient's L2 norm in double (a fixed tree), the clip scale, then bias-corrected
// Adam on every trainable word of the weight block in place; m, v use the block's layout
__global__ __launch_bounds__(1024) void avr_ppo_adam_kernel(float *__restrict__ W, const float *__restrict__ grad, float *__restrict__ m,
                                                            float *__restrict__ v, int *__restrict__ step, float *__restrict__ stats, const PpoAdam p) {
#pragma clang fp contract(off)
    __shared__ double red[1024];
    __shared__ float sh[3];
    const int t = threadIdx.x;
    double q = 0.0;
    for (int w = t; w < PW_WORDS; w += 1024) {
        const double g = (double)grad[w];
        q += g * g;
    }
    red[t] = q;
    for (int s = 512; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) red[t] += red[t + s];
    }
    __syncthreads();
    if (t == 0) {
        const float norm = (float)sqrt(red[0]);
        const int n = *step + 1;
        *step = n;
        sh[0] = p.max_grad_norm > 0.f ? fminf(1.f, p.max_grad_norm / (norm + 1e-6f)) : 1.f;
        sh[1] = (float)((double)p.lr / (1.0 - pow((double)p.beta1, (double)n)));
        sh[2] = (float)sqrt(1.0 - pow((double)p.beta2, (double)n));
        if (stats) stats[PS_GNORM] = norm;
    }
    __syncthreads();
    const float scale = sh[0], step_size = sh[1], sbc2 = sh[2];
    for (int w = PW_LOGSTD + t; w < PW_WORDS; w += 1024) {
        const float g = grad[w] * scale;
        const float mm = fmaf(p.beta1, m[w], (1.f - p.beta1) * g);
        const float vv = fmaf(p.beta2, v[w], (1.f - p.beta2) * (g * g));
        m[w] = mm;
        v[w] = vv;
        W[w] = W[w] - step_size * (mm / (sqrtf(vv) / sbc2 + p.eps));
    }
}

// PW_MEAN / PW_SD from device arrays (avr_policy_obs_norm_device): sd as avr_policy_set forms it
__global__ __launch_bounds__(64) void avr_policy_obs_norm_kernel(float *__restrict__ W, const float *__restrict__ mean, const float *__restrict__ var,
                                                                 float eps) {
    const int k = threadIdx.x;
    if (k >= K_OBS_DIM) return;
    const float sd = (float)sqrt((double)var[k] + (double)eps);
    W[PW_MEAN + k] = mean[k];
    if (sd > 0.f) W[PW_SD + k] = sd;              // (a non-positive variance keeps the row's divisor)
}

// ------------------------------------------------------------------ launch helpers
hipError_t avr_launch_gae(const float *rew, const unsigned char *done, const float *value, const float *term_value, float gamma, float lam, int n, int E,
                          float *adv, float *ret, hipStream_t stream) {
    hipLaunchKernelGGL(avr_gae_kernel, dim3((E + 255) / 256), dim3(256), 0, stream, rew, done, value, term_value, gamma, gamma * lam, n, E, adv, ret);
    return hipGetLastError();
}

hipError_t avr_launch_ppo_advstat(const float *adv, long long N, double *part, float *out, hipStream_t stream) {
    const long long want = (N + 255) / 256;
    const int nb = (int)(want < PPO_ADV_BLOCKS ? want : PPO_ADV_BLOCKS);
    hipLaunchKernelGGL(avr_ppo_advstat_kernel, dim3(nb), dim3(256), 0, stream, adv, N, part);
    hipLaunchKernelGGL(avr_ppo_advstat_final_kernel, dim3(1), dim3(256), 0, stream, part, nb, N, out);
    return hipGetLastError();
}

inline int avr_ppo_blocks(int B) { return std::min((B + POL_EPW - 1) / POL_EPW, PPO_MAX_BLOCKS); }

hipError_t avr_launch_ppo_grad(const float *W, const PpoArgs &A, float ent_coef, const float *advstat, float *part, double *spart, float *grad,
                               float *stats, hipStream_t stream) {
    const int nb = avr_ppo_blocks(A.B);
    hipLaunchKernelGGL(avr_ppo_grad_kernel, dim3(nb, 2), dim3(64), 0, stream, W, A, advstat, part, spart);
    hipLaunchKernelGGL(avr_ppo_reduce_kernel, dim3((PW_WORDS + 255) / 256), dim3(256), 0, stream, part, spart, nb, W, ent_coef, A.inv_B, grad, stats);
    return hipGetLastError();
}

hipError_t avr_launch_ppo_combine(const float *segs, const float *W, float ent_coef, float *grad, float *stats, hipStream_t stream) {
    hipLaunchKernelGGL(avr_ppo_combine_kernel, dim3((PW_WORDS + 255) / 256), dim3(256), 0, stream, segs, W, ent_coef, grad, stats);
    return hipGetLastError();
}

hipError_t avr_launch_ppo_adam(float *W, const float *grad, float *m, float *v, int *step, float *stats, const PpoAdam &p, hipStream_t stream) {
    hipLaunchKernelGGL(avr_ppo_adam_kernel, dim3(1), dim3(1024), 0, stream, W, grad, m, v, step, stats, p);
    return hipGetLastError();
}

hipError_t avr_launch_obs_norm(float *W, const float *mean, const float *var, float eps, hipStream_t stream) {
    hipLaunchKernelGGL(avr_policy_obs_norm_kernel, dim3(1), dim3(64), 0, stream, W, mean, var, eps);
    return hipGetLastError();
}
