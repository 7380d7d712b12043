// dxrl_pg.hip -- policy-gradient learner on MI355X (no reference counterpart:
// the reference's only learner is the SimpleLearner hill-climber; SURVEY.md
// §8(a) A11-A13).  Actor-critic MLP, PPO-clip heads, Adam; the GAE(gamma, lambda) reverse
// scan and the advantage moments are dxrl_pg_gae.hip.
//
// k_pg_rollout is the reference rollout (feature-major tape / diag 16; the production kernels
// are its bit-identity twins in dxrl_pg_rollout16.hip and dxrl_pg_rollout8.hip): one workgroup
// owns 64 envs for the whole horizon.  Per env step it runs the actor MLP on its 64-row tile with
// bf16 MFMA (weights streamed from L2, activations in LDS), samples
// a = mu + sigma * eps (Philox), optionally injects dynamics / observation
// noise (robustness_tests.py:140-211, config C5), steps the 64 envs (the
// same env_step as dxrl_env_step), writes the training tape and auto-resets.
// No inter-workgroup communication: envs and weights are independent/read-only.
#include "dxrl_gemm.h"
#include "dxrl_pg.h"
#include "dxrl_pg_mlp.h"
#include "dxrl_pg_rollout.h"

using namespace dxrl;
using namespace dxrl::pg;

namespace dxrl {

// log N(a | mu, sigma) summed over the action dims
__device__ __forceinline__ float gauss_logp(const float* a, const float* mu, const float* logstd) {
    float lp = 0.0f;
#pragma unroll
    for (int k = 0; k < kAct; ++k) {
        const float z = (a[k] - mu[k]) * __expf(-logstd[k]);
        lp += -0.5f * z * z - logstd[k] - 0.5f * kLog2Pi;
    }
    return lp;
}

// 15 (or more) standard normals from one Philox stream position
template <int N>
__device__ __forceinline__ void philox_normals(float* out, uint32_t k0, uint32_t k1, uint64_t ctr, uint32_t stream) {
#pragma unroll
    for (int b = 0; b < (N + 3) / 4; ++b) {
        float n0, n1, n2, n3;
        if (stream == kStreamPolicy) {
            const u32x4 r = philox(u32x4{(uint32_t)ctr, (uint32_t)(ctr >> 32), stream, (uint32_t)b}, k0, k1);
            box_muller(r.x, r.y, n0, n1);
            box_muller(r.z, r.w, n2, n3);
        } else {  // a noise stream
            float nz[4];
            noise_normals4(ctr, stream, (uint32_t)b, k0, k1, nz);
            n0 = nz[0];
            n1 = nz[1];
            n2 = nz[2];
            n3 = nz[3];
        }
        if (4 * b + 0 < N) out[4 * b + 0] = n0;
        if (4 * b + 1 < N) out[4 * b + 1] = n1;
        if (4 * b + 2 < N) out[4 * b + 2] = n2;
        if (4 * b + 3 < N) out[4 * b + 3] = n3;
    }
}


constexpr int kTile = 64;           // envs per workgroup
constexpr int kXs = kIn + 8;        // LDS row strides (bf16) -- conflict-free b128 fragment reads
constexpr int kHs = kH + 8;

// observation element k of ME:254-264 (k is a compile-time constant after unrolling)
__device__ __forceinline__ float obs_elem(const Env& e, int k) {
    if (k < kD) return e.jp[k];
    if (k < 2 * kD) return e.jv[k - kD];
    if (k < 2 * kD + 3) return (float)e.op[k - 2 * kD];
    if (k < 2 * kD + 7) return k == 2 * kD + 3 ? 1.0f : 0.0f;  // identity quaternion
    if (k < 2 * kD + 10) return e.ov[k - 2 * kD - 7];
    return (float)((e.flags >> (k - 2 * kD - 10)) & 1u);
}

// Policy input row: obs (+ observation noise, robustness_tests.py:199-207: obs + f32(N(0, s))),
// streamed 4 elements per Philox block into the bf16 LDS row and the tape.
__device__ __forceinline__ void write_policy_obs(const Env& e, bf16* xrow, float obs_noise, uint32_t k0, uint32_t k1,
                                                 uint64_t ctr, bf16* tape_rm, bf16* tape_fm, int64_t m,
                                                 int64_t ld_fm) {
#pragma unroll
    for (int b = 0; b < (kObs + 3) / 4; ++b) {
        float nz[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (obs_noise > 0.0f) noise_normals4(ctr, kStreamObs, (uint32_t)b, k0, k1, nz);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = 4 * b + q;
            if (k >= kObs) break;
            float v = obs_elem(e, k);
            if (obs_noise > 0.0f) v = v + obs_noise * nz[q];
            xrow[k] = to_bf16(v);
        }
    }
    if (tape_rm) {
#pragma unroll
        for (int q = 0; q < kIn / 8; ++q) {
            bf16x8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 8 * q + j;
                v[j] = k < kObs ? xrow[k] : (k == kObsIn ? (bf16)1.0f : (bf16)0.0f);
            }
            reinterpret_cast<bf16x8*>(tape_rm + m * kIn)[q] = v;
        }
    }
    if (tape_fm) {
#pragma unroll
        for (int k = 0; k < kObs; ++k) tape_fm[(int64_t)k * ld_fm + m] = xrow[k];
    }
}

// 4 waves (one per SIMD, so a wave may use 256 VGPRs + 256 AGPRs): wave w owns hidden
// columns kCpw*w .. kCpw*w + kCpw - 1 of both hidden layers; waves 2, 3 compute the mu head.
constexpr int kRolloutWaves = 4, kCpw = kH / kRolloutWaves, kNT = kCpw / 32;

constexpr int kW1s = kIn + 8, kW3s = kH + 8;  // LDS-resident W1 [256][72], W3 [32][264]

// kDense: the env's reward (dense_reward / sparse_reward), as in every rollout kernel
template <bool kDense = true>
__global__ __launch_bounds__(64 * kRolloutWaves, 1) void k_pg_rollout(PgRolloutArgs p) {
    __shared__ __attribute__((aligned(16))) bf16 W1s[kH * kW1s];
    __shared__ __attribute__((aligned(16))) bf16 W3s[kOut * kW3s];
    __shared__ __attribute__((aligned(16))) bf16 X[kTile * kXs];
    __shared__ __attribute__((aligned(16))) bf16 H1[kTile * kHs];
    __shared__ __attribute__((aligned(16))) bf16 H2[kTile * kHs];
    __shared__ __attribute__((aligned(16))) float MU[kTile * (kOut + 1)];
    __shared__ float LS[kActPad], SIG[kActPad], ISIG[kActPad];  // log_std, exp(log_std), exp(-log_std)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = p.s.n;
    const int64_t i = (int64_t)blockIdx.x * kTile + lane;  // env of this lane (wave 0)
    const bool live = i < n;
    const int64_t T = p.horizon;
    if (threadIdx.x < kAct) {
        const float ls = p.params[kOffLogStd + threadIdx.x];
        LS[threadIdx.x] = ls;
        SIG[threadIdx.x] = __expf(ls);
        ISIG[threadIdx.x] = __expf(-ls);
    }
    // ---- weights, loaded once per launch: W2 slab in registers (wave w: columns 32w..),
    //      W1 and the mu head W3 in LDS
    WTile<kH / 16> w2[kNT];
#pragma unroll
    for (int j = 0; j < kNT; ++j) load_wtile(w2[j], p.wbf + kBfW2a, kHx, kCpw * wave + 32 * j, lane);
    for (int c = threadIdx.x; c < kH * (kIn / 8); c += 64 * kRolloutWaves) {
        const int row = c / (kIn / 8), col = 8 * (c % (kIn / 8));
        *reinterpret_cast<bf16x8*>(W1s + row * kW1s + col) =
            *reinterpret_cast<const bf16x8*>(p.wbf + kBfW1a + (int64_t)row * kIn + col);
    }
    for (int c = threadIdx.x; c < kOut * (kH / 8); c += 64 * kRolloutWaves) {
        const int row = c / (kH / 8), col = 8 * (c % (kH / 8));
        *reinterpret_cast<bf16x8*>(W3s + row * kW3s + col) =
            *reinterpret_cast<const bf16x8*>(p.wbf + kBfW3a + (int64_t)row * kHx + col);
    }
    const int r32 = lane & 31, h2 = lane >> 5;
    const auto w1frag = [&](int j, int k) {
        return *reinterpret_cast<const bf16x8*>(W1s + (kCpw * wave + 32 * j + r32) * kW1s + 16 * k + 8 * h2);
    };
    const auto w2frag = [&](int j, int k) { return w2[j].b[k]; };
    Env e;
    EpisodeBook book;
    uint32_t ek0 = 0, ek1 = 0, pk0 = 0, pk1 = 0;
    uint64_t rctr = 0;
    if (wave == 0) {
        // constant padding of the X tile: bias column, zeros
        for (int k = kObs; k < kIn; ++k) X[lane * kXs + k] = k == kObsIn ? (bf16)1.0f : (bf16)0.0f;
        if (live) {
            load_env(p.s, i, e);
            book.ep_ret = p.ep_ret[i];
            rctr = p.s.reset_ctr[i];
            env_key(p.env_seed, p.gid0 + i, ek0, ek1);
            env_key(p.policy_seed, p.gid0 + i, pk0, pk1);
        } else {
            for (int k = 0; k < kObs; ++k) X[lane * kXs + k] = (bf16)0.0f;
        }
    }
    const bool mlp = !(p.diag & 1);
    for (int64_t t = 0; t < T; ++t) {
        const int64_t m = t * n + i;
        const uint64_t ctr = p.iteration * (uint64_t)T + (uint64_t)t;
        if (wave == 0 && live)
            write_policy_obs(e, X + lane * kXs, p.obs_noise, pk0, pk1, ctr, p.obs_rm, p.obs_fm, m, T * n);
        __syncthreads();
        if (mlp) wave_layer<kIn / 16, kNT, true>(X, kXs, w1frag, kCpw * wave, nullptr, 0, H1, kHs, lane);  // b: col 45
        __syncthreads();
        if (mlp)
            wave_layer<kH / 16, kNT, true>(H1, kHs, w2frag, kCpw * wave, p.params + kOffW2a + kH, kHx, H2, kHs, lane);
        __syncthreads();
        if (mlp && wave >= kRolloutWaves - 2) {  // mu head: 32 rows per wave, 32 output columns
            const int r = lane & 31, h = lane >> 5, row0 = 32 * (wave - (kRolloutWaves - 2));
            f32x16 acc;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
            for (int k = 0; k < kH / 16; ++k) {
                const bf16x8 a = *reinterpret_cast<const bf16x8*>(H2 + (row0 + r) * kHs + 16 * k + 8 * h);
                const bf16x8 b = *reinterpret_cast<const bf16x8*>(W3s + r * kW3s + 16 * k + 8 * h);
                acc = mfma32(a, b, acc);
            }
            const float bias = p.params[kOffW3a + (int64_t)r * kHx + kH];
#pragma unroll
            for (int q = 0; q < 16; ++q) MU[(row0 + acc_row(q, lane)) * (kOut + 1) + r] = acc[q] + bias;
        }
        __syncthreads();
        if (wave == 0 && live) {
            // a = mu + sigma * eps and log pi(a|s) accumulated in gauss_logp's exact order
            float a[kAct];
            float lp = 0.0f;
#pragma unroll
            for (int b = 0; b < (kAct + 3) / 4; ++b) {
                const u32x4 rr = philox(u32x4{(uint32_t)ctr, (uint32_t)(ctr >> 32), kStreamPolicy, (uint32_t)b},
                                        pk0, pk1);
                float nz[4];
                box_muller(rr.x, rr.y, nz[0], nz[1]);
                box_muller(rr.z, rr.w, nz[2], nz[3]);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int k = 4 * b + q;
                    if (k >= kAct) break;
                    const float mu = mlp ? MU[lane * (kOut + 1) + k] : 0.0f;
                    a[k] = mu + SIG[k] * nz[q];
                    const float z = (a[k] - mu) * ISIG[k];
                    lp += -0.5f * z * z - LS[k] - 0.5f * kLog2Pi;
                }
            }
            p.logp[m] = lp;
            float4* arow = reinterpret_cast<float4*>(p.act + m * kActPad);
            arow[0] = float4{a[0], a[1], a[2], a[3]};
            arow[1] = float4{a[4], a[5], a[6], a[7]};
            arow[2] = float4{a[8], a[9], a[10], a[11]};
            arow[3] = float4{a[12], a[13], a[14], 0.0f};
            if (p.dyn_noise > 0.0f) {  // robustness_tests.py:180-187 (the tape keeps the policy's action)
                float dn[kAct];
                philox_normals<kAct>(dn, pk0, pk1, ctr, kStreamDyn);
#pragma unroll
                for (int k = 0; k < kAct; ++k) a[k] = clipf(a[k] + p.dyn_noise * dn[k], -1.0f, 1.0f);
            }
            if (p.applied_act) {
#pragma unroll
                for (int k = 0; k < kActPad; ++k) p.applied_act[m * kActPad + k] = k < kAct ? a[k] : 0.0f;
            }
            bool te = false, tr = false;
            double cp[4], r = 0.0;
            if (!(p.diag & 2)) r = env_step(e, a, kDense, p.w, p.max_episode_steps, te, tr, cp);
            const bool d = !(p.diag & 2) && (te || tr || e.t >= p.max_steps);
            book.settle_step(p, r, d, te, e.t, t, i, true);
            write_step_end(p, m, d, te, e.t);
            if (d) {
                env_reset_philox(e, p.s.curricula[e.cfg], ek0, ek1, rctr);
                ++rctr;
            }
        }
    }
    if (wave == 0 && live) {
        // bootstrap observation (slot T) -- with observation noise as the policy would see it
        bf16 tmp[kObs];
        const uint64_t ctr = p.iteration * (uint64_t)T + (uint64_t)T;
        write_policy_obs(e, tmp, p.obs_noise, pk0, pk1, ctr, p.obs_rm, nullptr, T * n + i, 0);
        store_env(p.s, i, e);
        p.s.reset_ctr[i] = rctr;
        book.store(p, i);
    }
}

// out[slot] = sum(partials) (fixed order)
// Sum of nb partials by a 256-thread block in one fixed order: thread-strided sums, a butterfly
// inside each wave (lane pairs add the same two values, so every lane holds the same bits), then
// the four wave sums in wave order.  k_sum_partials and every k_adam_pack workgroup use it, so the
// two optimiser paths clip with bit-identical norms.
__device__ __forceinline__ double block_sum256(double s, double* red4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}
// (thread t adds partial[t], partial[t + 256], ... in that order; the loads go out in batches of 8
// ahead of their adds -- one L2 latency per batch, not per partial, for the ~2.6 k partials of
// dxrl_pg_fused_pair_gnorm -- and the + 0.0 of a batch's tail leaves the sum's bits unchanged)
// (kStride: the partials are one column of a row-major table, partial[k * kStride])
template <int kStride = 1>
__device__ __forceinline__ double block_sum_partials(const double* __restrict__ partial, int nb, double* red4) {
    constexpr int kB = 8;
    double s = 0.0;
    for (int k0 = threadIdx.x; k0 < nb; k0 += 256 * kB) {
        double v[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) v[u] = k0 + 256 * u < nb ? partial[(int64_t)(k0 + 256 * u) * kStride] : 0.0;
#pragma unroll
        for (int u = 0; u < kB; ++u) s += v[u];
    }
    return block_sum256(s, red4);
}

__global__ __launch_bounds__(256) void k_sum_partials(const double* __restrict__ partial, int nb,
                                                      double* __restrict__ out, int slot) {
    __shared__ double red4[4];
    const double s = block_sum_partials(partial, nb, red4);
    if (threadIdx.x == 0) out[slot] = s;
}


// ------------------------------------------------------------------ PPO heads
struct HeadArgs {
    const float* mu;       // [M][kOut] f32 (actor head)
    const float* V;        // [M] f32 (critic head row 0, feature-major)
    const float* act;      // [M][kActPad]
    const float* logp_old; // [M]
    const float* adv;      // [M]
    const float* ret;      // [M]
    const double* stats;   // normalisation stats
    const float* params;   // log_std
    int64_t M;
    double inv_total;      // 1 / global sample count (mean over all ranks)
    float clip_eps, vf_coef;
    bf16* dmu_rm;          // [M][kOut]
    bf16* dmu_fm;          // [kOut][M]
    bf16* dv_rm;           // [M][kOut] (col 0)
    bf16* dv_fm;           // [kOut][M] (row 0)
    float* dlogstd_partial;// [blocks][kActPad]
    double* loss_partial;  // [blocks][4]: policy loss, value loss, clip fraction, approx kl
};

__global__ __launch_bounds__(256) void k_ppo_heads(HeadArgs h) {
    __shared__ float red[256][kActPad];
    __shared__ double lred[256][4];
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    float dls[kAct];
#pragma unroll
    for (int k = 0; k < kAct; ++k) dls[k] = 0.0f;
    double lp_loss = 0.0, lv = 0.0, clipped = 0.0, kl = 0.0;
    if (m < h.M) {
        float ls[kAct], mu[kAct], a[kAct];
#pragma unroll
        for (int k = 0; k < kAct; ++k) {
            ls[k] = h.params[kOffLogStd + k];
            mu[k] = h.mu[m * kOut + k];
            a[k] = h.act[m * kActPad + k];
        }
        const float lp = gauss_logp(a, mu, ls);
        const float ratio = __expf(lp - h.logp_old[m]);
        const float A = (float)(((double)h.adv[m] - h.stats[2]) / (h.stats[4] + 1e-8));
        const float s1 = ratio * A;
        const float rc = fminf(fmaxf(ratio, 1.0f - h.clip_eps), 1.0f + h.clip_eps);
        const float s2 = rc * A;
        // d(-min(s1, s2))/d logp
        float g = 0.0f;
        if (s1 <= s2) g = -A * ratio;
        else if (ratio == rc) g = -A * ratio;
        const float sc = (float)h.inv_total;
        g *= sc;
#pragma unroll
        for (int k = 0; k < kAct; ++k) {
            const float iv = __expf(-2.0f * ls[k]);
            const float d = a[k] - mu[k];
            const float dmu = g * d * iv;              // dlogp/dmu = (a - mu) / sigma^2
            dls[k] = g * (d * d * iv - 1.0f);          // dlogp/dlogstd = (a-mu)^2/sigma^2 - 1
            h.dmu_rm[m * kOut + k] = to_bf16(dmu);
            if (h.dmu_fm) h.dmu_fm[(int64_t)k * h.M + m] = to_bf16(dmu);
        }
        const float v = h.V[m];
        const float dv = 2.0f * h.vf_coef * (v - h.ret[m]) * sc;
        h.dv_rm[m * kOut] = to_bf16(dv);
        if (h.dv_fm) h.dv_fm[m] = to_bf16(dv);
        lp_loss = -(double)fminf(s1, s2);
        lv = (double)(v - h.ret[m]) * (double)(v - h.ret[m]);
        clipped = fabsf(ratio - 1.0f) > h.clip_eps ? 1.0 : 0.0;
        kl = (double)(h.logp_old[m] - lp);
    }
#pragma unroll
    for (int k = 0; k < kAct; ++k) red[threadIdx.x][k] = dls[k];
    lred[threadIdx.x][0] = lp_loss;
    lred[threadIdx.x][1] = lv;
    lred[threadIdx.x][2] = clipped;
    lred[threadIdx.x][3] = kl;
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
#pragma unroll
            for (int k = 0; k < kAct; ++k) red[threadIdx.x][k] += red[threadIdx.x + w][k];
#pragma unroll
            for (int k = 0; k < 4; ++k) lred[threadIdx.x][k] += lred[threadIdx.x + w][k];
        }
        __syncthreads();
    }
    if (threadIdx.x < kActPad)
        h.dlogstd_partial[(int64_t)blockIdx.x * kActPad + threadIdx.x] = threadIdx.x < kAct ? red[0][threadIdx.x] : 0.0f;
    if (threadIdx.x < 4) h.loss_partial[(int64_t)blockIdx.x * 4 + threadIdx.x] = lred[0][threadIdx.x];
}

// grads[kOffLogStd + k] = sum_b partial[b][k] - ent_coef  (entropy bonus: d(-c H)/d logstd = -c)
__global__ __launch_bounds__(256) void k_logstd_grad(const float* __restrict__ partial, int nb, float ent_coef,
                                                     float* __restrict__ grads) {
    __shared__ float red[256][kActPad + 1];
    float s[kActPad];
#pragma unroll
    for (int k = 0; k < kActPad; ++k) s[k] = 0.0f;
    for (int b = threadIdx.x; b < nb; b += 256) {  // fixed partition + fixed tree: deterministic
#pragma unroll
        for (int k = 0; k < kActPad; ++k) s[k] += partial[(int64_t)b * kActPad + k];
    }
#pragma unroll
    for (int k = 0; k < kActPad; ++k) red[threadIdx.x][k] = s[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w)
#pragma unroll
            for (int k = 0; k < kActPad; ++k) red[threadIdx.x][k] += red[threadIdx.x + w][k];
        __syncthreads();
    }
    const int k = threadIdx.x;
    if (k < kActPad) grads[kOffLogStd + k] = k < kAct ? red[0][k] - ent_coef : 0.0f;
}

// ------------------------------------------------------------------ optimiser
// grad-norm^2 partials, then Adam with global-norm clipping (scale on device)
__global__ __launch_bounds__(256) void k_sumsq(const float* __restrict__ x, int64_t n, double* __restrict__ partial) {
    __shared__ double red4[4];
    double s = 0.0;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        s += (double)x[k] * (double)x[k];
    s = block_sum256(s, red4);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m1,
                       float* __restrict__ m2, int64_t n, float lr, float b1, float b2, float eps, float bc1,
                       float bc2, const double* __restrict__ gnorm2, float max_norm) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float scale = 1.0f;
    if (max_norm > 0.0f) {
        const float nrm = (float)sqrt(gnorm2[0]);
        scale = nrm > max_norm ? max_norm / (nrm + 1e-6f) : 1.0f;
    }
    const float gk = g[k] * scale;
    const float a = b1 * m1[k] + (1.0f - b1) * gk;
    const float b = b2 * m2[k] + (1.0f - b2) * gk * gk;
    m1[k] = a;
    m2[k] = b;
    p[k] -= lr * (a / bc1) / (sqrtf(b / bc2) + eps);
}

// f32 master -> bf16 forward weights + transposed copies for input gradients: work item k of the
// pack, reading master element j as p(j)
template <typename Src>
__device__ __forceinline__ void pack_item(int64_t k, const Src& p, bf16* __restrict__ w) {
    // forward copies (same layout as the master blocks)
    if (k < kW1) {
        w[kBfW1a + k] = to_bf16(p(kOffW1a + k));
        w[kBfW1c + k] = to_bf16(p(kOffW1c + k));
    }
    if (k < kW2) {
        w[kBfW2a + k] = to_bf16(p(kOffW2a + k));
        w[kBfW2c + k] = to_bf16(p(kOffW2c + k));
    }
    if (k < kW3) {
        w[kBfW3a + k] = to_bf16(p(kOffW3a + k));
        w[kBfW3c + k] = to_bf16(p(kOffW3c + k));
    }
    if (k < kW2T) {  // W2T[i][o] = W2[o][i]
        const int64_t i = k / kH, o = k % kH;
        w[kBfW2aT + k] = to_bf16(p(kOffW2a + o * kHx + i));
        w[kBfW2cT + k] = to_bf16(p(kOffW2c + o * kHx + i));
    }
    if (k < kW3T) {  // W3T[i][o] = W3[o][i]
        const int64_t i = k / kOut, o = k % kOut;
        w[kBfW3aT + k] = to_bf16(p(kOffW3a + o * kHx + i));
        w[kBfW3cT + k] = to_bf16(p(kOffW3c + o * kHx + i));
    }
    // fragment-ordered copies (dxrl_pg.h): element k of a [N][K] matrix's fragment stream
    const auto frag_rc = [](int64_t k, int K, int64_t& row, int64_t& col) {
        const int e = (int)(k & 7), lane = (int)((k >> 3) & 63);
        const int64_t fk = k >> 9, ks = K / 16, ft = fk / ks, kk = fk % ks;
        row = 32 * ft + (lane & 31);
        col = 16 * kk + 8 * (lane >> 5) + e;
    };
#pragma unroll
    for (int net = 0; net < 2; ++net) {
        const int64_t o1 = net ? kOffW1c : kOffW1a, o2 = net ? kOffW2c : kOffW2a, o3 = net ? kOffW3c : kOffW3a;
        bf16* f = w + kFr + net * kFrNet;
        int64_t row, col;
        if (k < kFrW1) {
            frag_rc(k, kIn, row, col);
            f[kFrOffW1 + k] = to_bf16(p(o1 + row * kIn + col));
        }
        if (k < kFrW2) {
            frag_rc(k, kH, row, col);
            f[kFrOffW2 + k] = to_bf16(p(o2 + row * kHx + col));
            f[kFrOffW2T + k] = to_bf16(p(o2 + col * kHx + row));  // W2T[row][col] = W2[col][row]
        }
        if (k < kFrW3) {
            frag_rc(k, kH, row, col);
            f[kFrOffW3 + k] = to_bf16(p(o3 + row * kHx + col));
        }
        if (k < kFrW3T) {
            frag_rc(k, kOut, row, col);
            f[kFrOffW3T + k] = to_bf16(p(o3 + col * kHx + row));  // W3T[row][col] = W3[col][row]
        }
    }
}

__global__ void k_pack_weights(const float* __restrict__ p, bf16* __restrict__ w) {
    pack_item((int64_t)blockIdx.x * blockDim.x + threadIdx.x, [p](int64_t j) { return p[j]; }, w);
}

// Position of element (row, col) of a [N][K] matrix in its fragment stream (the inverse of
// pack_item's frag_rc: 64-lane x 8-element fragments, 32 rows x 16 columns each, k-steps inner)
__device__ __forceinline__ int64_t frag_index(int row, int col, int K) {
    const int lane = (row & 31) + 32 * ((col >> 3) & 1);
    return ((int64_t)((row >> 5) * (K / 16) + (col >> 4)) << 9) + lane * 8 + (col & 7);
}

// Every packed bf16 copy of master element j (value v): the scatter form of pack_item's gathers --
// the forward copy, the transposed copy and the fragment streams of W1 / W2 / W3 (log σ and the
// pad slots between the nets are master-only)
__device__ __forceinline__ void pack_scatter(int64_t j, float v, bf16* __restrict__ w) {
    const bf16 b = to_bf16(v);
    const bool c = j >= kOffW1c;
    const int64_t r = j - (c ? kOffW1c : kOffW1a);
    bf16* f = w + kFr + (c ? kFrNet : 0);
    if (r < 0) return;
    if (r < kW1) {  // W1 [kH][kIn]
        const int row = (int)(r / kIn), col = (int)(r % kIn);
        w[(c ? kBfW1c : kBfW1a) + r] = b;
        f[kFrOffW1 + frag_index(row, col, kIn)] = b;
    } else if (r < kW1 + kW2) {  // W2 [kH][kHx], column kH = bias
        const int64_t q = r - kW1;
        const int row = (int)(q / kHx), col = (int)(q % kHx);
        w[(c ? kBfW2c : kBfW2a) + q] = b;
        if (col < kH) {
            w[(c ? kBfW2cT : kBfW2aT) + (int64_t)col * kH + row] = b;
            f[kFrOffW2 + frag_index(row, col, kH)] = b;
            f[kFrOffW2T + frag_index(col, row, kH)] = b;
        }
    } else if (r < kW1 + kW2 + kW3) {  // W3 [kOut][kHx]
        const int64_t q = r - kW1 - kW2;
        const int row = (int)(q / kHx), col = (int)(q % kHx);
        w[(c ? kBfW3c : kBfW3a) + q] = b;
        if (col < kH) {
            w[(c ? kBfW3cT : kBfW3aT) + (int64_t)col * kOut + row] = b;
            f[kFrOffW3 + frag_index(row, col, kH)] = b;
            f[kFrOffW3T + frag_index(col, row, kOut)] = b;
        }
    }
}

// One optimiser launch after k_sumsq: every workgroup sums the grad-norm partials in
// k_sum_partials' order (so the clip scale is bit for bit k_adam's); thread j applies Adam to
// master element j (k_adam's expression, once) and scatters the updated value into every packed
// bf16 copy (pack_scatter).  The updated master goes to a second buffer (the trainer swaps the
// pair).  The gather form (k_pack_weights / pack_item, which recomputed the update of every
// element it packed: up to 20 updates per thread) took 13.3 us per step.
struct AdamPackArgs {
    const float *p, *g, *m1, *m2;
    float *po, *m1o, *m2o;
    int64_t n;
    float lr, b1, b2, eps, bc1, bc2, max_norm;
    const double* partial;
    int nb;
    double* gnorm2;
    bf16* w;
};

// The global-norm clip factor and the Adam update of one master element, stated once for both
// optimiser-step kernels (k_adam's expressions).
__device__ __forceinline__ float clip_scale(double g2, float max_norm) {
    if (!(max_norm > 0.0f)) return 1.0f;
    const float nrm = (float)sqrt(g2);
    return nrm > max_norm ? max_norm / (nrm + 1e-6f) : 1.0f;
}

__device__ __forceinline__ void adam_pack_element(const AdamPackArgs& a, int64_t j, float scale, float lr, float bc1,
                                                  float bc2) {
    const float gk = a.g[j] * scale;
    const float m = a.b1 * a.m1[j] + (1.0f - a.b1) * gk;
    const float v = a.b2 * a.m2[j] + (1.0f - a.b2) * gk * gk;
    const float pn = a.p[j] - lr * (m / bc1) / (sqrtf(v / bc2) + a.eps);
    a.po[j] = pn;
    a.m1o[j] = m;
    a.m2o[j] = v;
    pack_scatter(j, pn, a.w);
}

__global__ __launch_bounds__(256) void k_adam_pack(AdamPackArgs a) {
    __shared__ double red4[4];
    const double g2 = block_sum_partials(a.partial, a.nb, red4);
    if (blockIdx.x == 0 && threadIdx.x == 0) a.gnorm2[0] = g2;
    const float scale = clip_scale(g2, a.max_norm);
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n) return;
    adam_pack_element(a, j, scale, a.lr, a.bc1, a.bc2);
}

// k_adam_pack with the step size decided on the device (dxrl_pg_adam_step_ctl; include/dxrl.h has
// the rules).  Every workgroup finishes the pass's KL sum from the loss partials' column 3 in
// block_sum_partials' fixed order and reads the same state slot, so all workgroups hold the same
// decision bits with no grid-wide exchange; workgroup 0 alone writes the next state, into the
// other slot (the slot a call reads is never the one it writes: the other workgroups of the launch
// may still be reading it).  A stopped pass copies master and moments through and leaves the pack.
struct AdamCtlArgs {
    AdamPackArgs a;            // a.lr unused; a.bc1 / a.bc2: the host's corrections for t = calls
    dxrl_pg_lr_control c;
    double beta1, beta2;
    union {                    // where (kl_sum, rows) come from, one member per kernel:
        const double* loss;    // k_adam_pack_ctl: f64 [loss_rows][4], column 3 = the pass's approx-KL sums
        const double* records; // k_adam_pack_ctl_world: f64 [world][2], the ranks' (kl_sum, rows) in rank order
    };
    union {
        int loss_rows;
        int world;
    };
    double rows;               // k_adam_pack_ctl: samples of the pass (k_adam_pack_ctl_world: unused)
    const int64_t* rd;         // state slot read
    int64_t* wr;               // state slot written
    double* row;               // f64 [DXRL_PG_OPT_COLS] or null
};

// (the rules, once, for both forms below: g2 the squared grad norm, (kl_sum, rows) the pass's KL
// sum and samples, each already the same bits in every thread of the launch)
__device__ __forceinline__ void adam_pack_ctl_apply(const AdamCtlArgs& x, double g2, double kl_sum, double rows) {
    const AdamPackArgs& a = x.a;
    const dxrl_pg_lr_control& c = x.c;
    const double* rdf = reinterpret_cast<const double*>(x.rd);
    const bool first = c.pass_index == 0;
    const int64_t applied = x.rd[DXRL_PG_OPT_APPLIED], skipped = x.rd[DXRL_PG_OPT_SKIPPED];
    const double lr_scale = rdf[DXRL_PG_OPT_SCALE];
    const double kl = kl_sum / rows;
    bool stopped = !first && x.rd[DXRL_PG_OPT_STOPPED] != 0;
    const bool stops = c.target_kl > 0.0 && !stopped && kl > c.stop_factor * c.target_kl;
    stopped = stopped || stops;
    double lr = c.lr_nominal * lr_scale;
    lr = lr < c.lr_min ? c.lr_min : (lr > c.lr_max ? c.lr_max : lr);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.gnorm2[0] = g2;
        double* wrf = reinterpret_cast<double*>(x.wr);
        const int64_t it_applied = (first ? 0 : x.rd[DXRL_PG_OPT_ITER_APPLIED]) + (stopped ? 0 : 1);
        const int64_t it_skipped = (first ? 0 : x.rd[DXRL_PG_OPT_ITER_SKIPPED]) + (stopped ? 1 : 0);
        const int64_t stop_pass = stops ? (int64_t)c.pass_index : (first ? -1 : x.rd[DXRL_PG_OPT_STOP_PASS]);
        double lr_first = first ? 0.0 : rdf[DXRL_PG_OPT_LR_FIRST], lr_last = first ? 0.0 : rdf[DXRL_PG_OPT_LR_LAST];
        if (!stopped) {
            if (it_applied == 1) lr_first = lr;
            lr_last = lr;
        }
        const double kl_prev = rdf[DXRL_PG_OPT_KL_MAX];
        const double kl_max = first || kl > kl_prev ? kl : kl_prev;
        double acc_kl = first ? 0.0 : rdf[DXRL_PG_OPT_KL_SUM], acc_rows = first ? 0.0 : rdf[DXRL_PG_OPT_KL_ROWS];
        if (c.last_epoch) {
            acc_kl += kl_sum;
            acc_rows += rows;
        }
        double next = lr_scale;
        if (c.last_pass) {
            const double kl_epoch = acc_rows > 0.0 ? acc_kl / acc_rows : 0.0;
            if (c.adapt && c.target_kl > 0.0 && acc_rows > 0.0) {
                if (kl_epoch > c.adapt_band * c.target_kl) next = next / c.adapt_factor;
                else if (kl_epoch < c.target_kl / c.adapt_band) next = next * c.adapt_factor;
            }
            // lr_nominal * next kept inside [lr_min, lr_max]: the quotient, one ulp inwards when
            // the product of the rounded quotient still lands outside
            if (c.lr_nominal * next > c.lr_max) {
                next = c.lr_max / c.lr_nominal;
                if (c.lr_nominal * next > c.lr_max) next = nextafter(next, 0.0);
            } else if (c.lr_nominal * next < c.lr_min) {
                next = c.lr_min / c.lr_nominal;
                if (c.lr_nominal * next < c.lr_min) next = nextafter(next, HUGE_VAL);
            }
            if (x.row) {
                x.row[DXRL_PG_OPT_COL_LR] = lr_first;
                x.row[DXRL_PG_OPT_COL_LR_LAST] = lr_last;
                x.row[DXRL_PG_OPT_COL_UPDATES] = (double)it_applied;
                x.row[DXRL_PG_OPT_COL_SKIPPED] = (double)it_skipped;
                x.row[DXRL_PG_OPT_COL_STOP_PASS] = (double)stop_pass;
                x.row[DXRL_PG_OPT_COL_KL_MAX] = kl_max;
                x.row[DXRL_PG_OPT_COL_KL_EPOCH] = kl_epoch;
                x.row[DXRL_PG_OPT_COL_LR_SCALE] = next;
            }
        }
        x.wr[DXRL_PG_OPT_APPLIED] = applied + (stopped ? 0 : 1);
        x.wr[DXRL_PG_OPT_SKIPPED] = skipped + (stopped ? 1 : 0);
        wrf[DXRL_PG_OPT_SCALE] = next;
        x.wr[DXRL_PG_OPT_STOPPED] = stopped ? 1 : 0;
        x.wr[DXRL_PG_OPT_STOP_PASS] = stop_pass;
        x.wr[DXRL_PG_OPT_ITER_APPLIED] = it_applied;
        x.wr[DXRL_PG_OPT_ITER_SKIPPED] = it_skipped;
        wrf[DXRL_PG_OPT_LR_FIRST] = lr_first;
        wrf[DXRL_PG_OPT_LR_LAST] = lr_last;
        wrf[DXRL_PG_OPT_KL_MAX] = kl_max;
        wrf[DXRL_PG_OPT_KL_SUM] = acc_kl;
        wrf[DXRL_PG_OPT_KL_ROWS] = acc_rows;
        for (int k = DXRL_PG_OPT_NAMED; k < DXRL_PG_OPT_SLOT_WORDS; ++k) x.wr[k] = 0;
    }
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= a.n) return;
    if (stopped) {
        a.po[j] = a.p[j];
        a.m1o[j] = a.m1[j];
        a.m2o[j] = a.m2[j];
        return;
    }
    // Adam's t counts applied passes.  While no pass was ever skipped t is the host's call count
    // and the host's corrections are used (the parent's bytes); afterwards 1 - beta^t in f64 here.
    float bc1 = a.bc1, bc2 = a.bc2;
    if (skipped != 0) {
        const double t = (double)(applied + 1);
        bc1 = (float)(1.0 - pow(x.beta1, t));
        bc2 = (float)(1.0 - pow(x.beta2, t));
    }
    adam_pack_element(a, j, clip_scale(g2, a.max_norm), (float)lr, bc1, bc2);
}

__global__ __launch_bounds__(256) void k_adam_pack_ctl(AdamCtlArgs x) {
    __shared__ double red4[4];
    const double g2 = block_sum_partials(x.a.partial, x.a.nb, red4);
    __syncthreads();  // red4 is reused
    const double kl_sum = block_sum_partials<4>(x.loss + 3, x.loss_rows, red4);
    adam_pack_ctl_apply(x, g2, kl_sum, x.rows);
}

// The sharded form (dxrl_pg_adam_step_ctl_world): x.records is the gathered f64 [x.world][2] records
// (kl_sum, rows) of dxrl_pg_kl_rank_pack in rank order.
// Every thread merges the 2 x world doubles sequentially in rank order -- the same bytes on every
// rank, so the same decision on every rank -- and the rest is k_adam_pack_ctl's.
__global__ __launch_bounds__(256) void k_adam_pack_ctl_world(AdamCtlArgs x) {
    __shared__ double red4[4];
    const double g2 = block_sum_partials(x.a.partial, x.a.nb, red4);
    double kl_sum = x.records[0], rows = x.records[1];
    for (int r = 1; r < x.world; ++r) {
        kl_sum += x.records[2 * r];
        rows += x.records[2 * r + 1];
    }
    adam_pack_ctl_apply(x, g2, kl_sum, rows);
}

// dxrl_pg_kl_rank_pack: one workgroup; record = (column 3 of the loss partials summed in
// k_adam_pack_ctl's order, the pass's rows)
__global__ __launch_bounds__(256) void k_kl_rank_pack(const double* __restrict__ loss, int loss_rows, double rows,
                                                      double* __restrict__ record) {
    __shared__ double red4[4];
    const double kl_sum = block_sum_partials<4>(loss + 3, loss_rows, red4);
    if (threadIdx.x == 0) {
        record[0] = kl_sum;
        record[1] = rows;
    }
}

// dxrl_pg_popart_rescale (include/dxrl.h states the arithmetic and the three cases): one workgroup,
// thread j < 257 owns element j of the critic head's row 0 (256 weights, then the bias) and
// scatters the new value into its packed copies with pack_scatter, as the optimiser does.  Every
// thread reads both pairs and takes the same branch; thread 0 writes the block and the row behind
// a barrier, after every thread has read the words it replaces.
constexpr int kPopartThreads = 320;  // >= kH + 1 head elements, whole waves
__device__ __forceinline__ double popart_std(double n, double m2) { return n > 0.0 ? sqrt(m2 / n) : 0.0; }
__global__ __launch_bounds__(kPopartThreads) void k_popart_rescale(float* __restrict__ params, bf16* __restrict__ w,
                                                                    const double* __restrict__ vn,
                                                                    double* __restrict__ pa,
                                                                    double* __restrict__ row) {
    const double mu_h = pa[DXRL_PG_POPART_MU_HEAD], sigma_h = pa[DXRL_PG_POPART_SIGMA_HEAD];
    const double mu_n = vn[DXRL_PG_VNORM_MU], sigma_n = vn[DXRL_PG_VNORM_SIGMA];
    const bool lead = threadIdx.x == 0;
    const bool usable = isfinite(mu_h) && isfinite(mu_n) && isfinite(sigma_h) && isfinite(sigma_n) && sigma_h > 0.0 &&
                        sigma_n > 0.0;
    if (!usable) {  // (only thread 0 reads SKIPPED: no barrier needed)
        if (lead) pa[DXRL_PG_POPART_SKIPPED] += 1.0;
        return;
    }
    const bool same = __double_as_longlong(mu_h) == __double_as_longlong(mu_n) &&
                      __double_as_longlong(sigma_h) == __double_as_longlong(sigma_n);
    const double s = same ? 1.0 : sigma_h / sigma_n;
    const double shift = same ? 0.0 : (mu_h - mu_n) / sigma_n;
    if (!same) {
        const int j = (int)threadIdx.x;
        if (j <= kH) {
            const double x = (double)params[kOffW3c + j];
            const float y = j < kH ? (float)(x * s) : (float)((sigma_h * x + (mu_h - mu_n)) / sigma_n);
            params[kOffW3c + j] = y;
            pack_scatter(kOffW3c + j, y, w);
        }
        __syncthreads();  // every thread holds the old pair before thread 0 replaces it
        if (lead) {
            pa[DXRL_PG_POPART_MU_HEAD] = mu_n;
            pa[DXRL_PG_POPART_SIGMA_HEAD] = sigma_n;
            pa[DXRL_PG_POPART_RESCALES] += 1.0;
            pa[DXRL_PG_POPART_LAST_SCALE] = s;
            pa[DXRL_PG_POPART_LAST_SHIFT] = shift;
        }
    }
    if (lead && row) {
        row[DXRL_PG_VNORM_LOG_MU] = mu_n;
        row[DXRL_PG_VNORM_LOG_SIGMA] = sigma_n;
        row[DXRL_PG_VNORM_LOG_MU_PREV] = mu_h;
        row[DXRL_PG_VNORM_LOG_SIGMA_PREV] = sigma_h;
        row[DXRL_PG_VNORM_LOG_SCALE] = s;
        row[DXRL_PG_VNORM_LOG_SHIFT] = shift;
        row[DXRL_PG_VNORM_LOG_RESCALED] = same ? 0.0 : 1.0;
        row[DXRL_PG_VNORM_LOG_COUNT] = vn[DXRL_PG_VNORM_COUNT];
        row[DXRL_PG_VNORM_LOG_MEAN] = vn[DXRL_PG_VNORM_MEAN];
        row[DXRL_PG_VNORM_LOG_STD] = popart_std(vn[DXRL_PG_VNORM_COUNT], vn[DXRL_PG_VNORM_M2]);
        row[DXRL_PG_VNORM_LOG_BATCH_MEAN] = vn[DXRL_PG_VNORM_BATCH_MEAN];
        row[DXRL_PG_VNORM_LOG_BATCH_STD] = popart_std(vn[DXRL_PG_VNORM_BATCH_COUNT], vn[DXRL_PG_VNORM_BATCH_M2]);
        row[DXRL_PG_VNORM_LOG_CALLS] = vn[DXRL_PG_VNORM_CALLS];
        row[DXRL_PG_VNORM_LOG_FORGET] = vn[DXRL_PG_VNORM_FORGET];
    }
}

static int reduce_to(const double* partial, int nb, double* out, int slot, hipStream_t st) {
    hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, st, partial, nb, out, slot);
    return launch_check("k_sum_partials");
}

}  // namespace dxrl

// =========================================================================== C ABI
extern "C" {

int dxrl_pg_sizes(int64_t* params, int64_t* packed_bf16) {
    DXRL_REQUIRE(params && packed_bf16, "null outputs");
    *params = kParams;
    *packed_bf16 = kBf;
    return DXRL_OK;
}

int dxrl_pg_pack_weights(int32_t device, const float* params, void* packed, void* stream) {
    DXRL_REQUIRE(params && packed, "null params/packed");
    DeviceGuard g(device);
    const int64_t n = kW2 > kW2T ? kW2 : kW2T;  // largest block
    hipLaunchKernelGGL(k_pack_weights, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), params,
                       static_cast<bf16*>(packed));
    return launch_check("k_pack_weights");
}

}  // extern "C"
namespace dxrl {
namespace {
// The rollout kernel dxrl_pg_rollout launches for n envs: 0 the 64-env reference kernel (feature-
// major tape / diag 16), 1 the 16-env kernel, 2 the 32-env kernel (>= 32 envs per CU: one round
// where the 16-env kernel would need two; diag 1024 / 2048 force it / the 16-env kernel).
int rollout_kernel(int64_t n, int32_t diag_flags, bool obs_fm) {
    if (obs_fm || (diag_flags & 16)) return 0;
    static const int cus = [] {
        int dev = 0, c = 0;
        (void)hipGetDevice(&dev);
        return hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0 ? c : 256;
    }();
    const bool e8 = !(diag_flags & 2048) && ((diag_flags & 1024) || n >= (int64_t)kE8Envs * cus);
    return e8 ? 2 : 1;
}
}  // namespace
}  // namespace dxrl
extern "C" {

int dxrl_pg_rollout_kernel(const dxrl_env* env, int32_t diag_flags, int32_t* kernel) {
    DXRL_REQUIRE(env && kernel, "null argument");
    DeviceGuard g(env->device);
    *kernel = rollout_kernel(env->cfg.num_envs, diag_flags, false);
    return DXRL_OK;
}

int dxrl_pg_rollout(dxrl_env* env, const void* packed, const float* params, const dxrl_pg_rollout_args* a,
                    void* stream) {
    DXRL_REQUIRE(env && packed && params && a, "null argument");
    DXRL_REQUIRE(a->horizon > 0 && a->max_steps > 0, "horizon and max_steps must be > 0");
    DXRL_REQUIRE(a->obs_rm && a->act && a->logp && a->rew && a->done && a->ep_return && a->ep_count &&
                     a->ep_sum_return && a->ep_sum_length && a->ep_successes,
                 "null tape / episode buffer");
    DXRL_REQUIRE(a->record_cap == 0 || (a->rec_return && a->rec_length && a->rec_success && a->rec_end_step),
                 "record_cap > 0 needs all four record buffers");
    DXRL_REQUIRE(!a->ep_code || (a->max_steps < 16384 && env->cfg.max_episode_steps < 16383),
                 "ep_code holds episode lengths below 2^14: max_steps / max_episode_steps too large");
    PgRolloutArgs p{env->soa,
                    weights_of(env->cfg),
                    env->cfg.max_episode_steps,
                    a->max_steps,
                    a->horizon,
                    static_cast<const bf16*>(packed),
                    params,
                    env->cfg.seed,
                    a->policy_seed,
                    env->cfg.global_env_offset,
                    a->iteration,
                    (float)a->obs_noise_std,
                    (float)a->dyn_noise_std,
                    static_cast<bf16*>(a->obs_rm),
                    static_cast<bf16*>(a->obs_fm),
                    a->act,
                    a->logp,
                    a->rew,
                    a->done,
                    a->ep_return,
                    a->ep_count,
                    a->ep_sum_return,
                    a->ep_sum_length,
                    a->ep_successes,
                    a->diag_flags,
                    a->success_rule == DXRL_SUCCESS_TERMINATED,
                    a->record_cap,
                    a->rec_return,
                    a->rec_length,
                    a->rec_success,
                    a->rec_end_step,
                    a->ep_code,
                    a->applied_act,
                    a->dyn_noise_tape,
                    a->obs_noise_tape,
                    static_cast<bf16*>(a->h2_tape)};

    DXRL_REQUIRE(!(a->dyn_noise_tape || a->obs_noise_tape) || !(a->obs_fm || (a->diag_flags & 16)),
                 "the noise tapes are written by the 16- and 32-env rollout kernels only");
    DeviceGuard g(env->device);
    const int64_t n = env->cfg.num_envs;
    DXRL_REQUIRE((reinterpret_cast<uintptr_t>(a->h2_tape) & 15) == 0, "pg_rollout: h2_tape must be 16-byte aligned");
    DXRL_REQUIRE(!a->h2_tape || rollout_kernel(n, a->diag_flags, a->obs_fm != nullptr) != 0,
                 "h2_tape is written by the 16- and 32-env rollout kernels only (dxrl_pg_rollout_kernel)");
    // the reward follows the env's config: every kernel has a dense and a sparse instantiation
    const bool dense = env->cfg.reward_type == DXRL_REWARD_DENSE;
    if (a->obs_fm || (a->diag_flags & 16)) {  // feature-major tape / A-B reference: the 64-env kernel
        const dim3 grid((unsigned)((n + kTile - 1) / kTile)), block(64 * kRolloutWaves);
        if (dense) hipLaunchKernelGGL(k_pg_rollout<true>, grid, block, 0, as_stream(stream), p);
        else hipLaunchKernelGGL(k_pg_rollout<false>, grid, block, 0, as_stream(stream), p);
        return launch_check("k_pg_rollout");
    }
    DXRL_REQUIRE(!(a->diag_flags & (32 | 64)), "diag_flags 32 / 64 named the retired k_pg_rollout_ls");
    static unsigned long long* stamps = nullptr;
    static int64_t stamps_n = 0;
    if ((a->diag_flags & 128) && stamps_n < n) {
        if (stamps) (void)hipFree(stamps);
        // 16 per env (32-env kernel) or 8 per wave of a 16-env workgroup: both fit (n + 15) 16
        (void)hipMalloc(&stamps, (size_t)(n + 15) * 16 * sizeof(unsigned long long));
        stamps_n = n;
    }
    p.stamps = stamps;
    // which template instantiation: fused noise (or its parity tapes) / diagnostics compiled in
    const bool noise = a->obs_noise_std > 0.0 || a->dyn_noise_std > 0.0 || a->dyn_noise_tape || a->obs_noise_tape;
    const bool diag = (a->diag_flags & ~(1024 | 2048)) != 0 || a->applied_act || a->dyn_noise_tape || a->obs_noise_tape;
    const auto launch = rollout_kernel(n, a->diag_flags, false) == 2 ? launch_pg_rollout_e8 : launch_pg_rollout_ws;
    return launch(p, n, noise, diag, dense, as_stream(stream));
}

int dxrl_pg_popart_rescale(int32_t device, const dxrl_pg_popart_args* a, void* stream) {
    DXRL_REQUIRE(a, "null args");
    DXRL_REQUIRE(a->params && a->packed && a->vnorm && a->popart, "null argument");
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_popart_rescale, dim3(1), dim3(kPopartThreads), 0, as_stream(stream), a->params,
                       static_cast<bf16*>(a->packed), a->vnorm, a->popart, a->row_out);
    return launch_check("k_popart_rescale");
}

int dxrl_pg_heads(int32_t device, const dxrl_pg_heads_args* a, void* stream) {
    DXRL_REQUIRE(a, "null args");
    DeviceGuard g(device);
    HeadArgs h{a->mu, a->values, a->act, a->logp_old, a->adv, a->ret, a->stats, a->params, a->num_samples,
               a->inv_total_samples, (float)a->clip_eps, (float)a->vf_coef,
               static_cast<bf16*>(a->dmu_rm), static_cast<bf16*>(a->dmu_fm), static_cast<bf16*>(a->dv_rm),
               static_cast<bf16*>(a->dv_fm), a->dlogstd_partial, a->loss_partial};
    const int nb = (int)((a->num_samples + 255) / 256);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_ppo_heads, dim3(nb), dim3(256), 0, st, h);
    if (int rc = launch_check("k_ppo_heads")) return rc;
    hipLaunchKernelGGL(k_logstd_grad, dim3(1), dim3(256), 0, st, a->dlogstd_partial, nb, (float)a->ent_coef,
                       a->grads);
    return launch_check("k_logstd_grad");
}

int dxrl_pg_grad_sumsq(int32_t device, const float* grads, int64_t n, double* partial, double* out, void* stream) {
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_sumsq, dim3(512), dim3(256), 0, st, grads, n, partial);
    if (int rc = launch_check("k_sumsq")) return rc;
    return reduce_to(partial, 512, out, 0, st);
}

int dxrl_pg_optimizer_step(int32_t device, const float* params, const float* grads, const float* m1, const float* m2,
                           float* params_out, float* m1_out, float* m2_out, int64_t n, double lr, double beta1,
                           double beta2, double eps, int64_t step, double max_norm, double* partial, double* gnorm2,
                           void* packed, void* stream) {
    DXRL_REQUIRE(params && grads && m1 && m2 && params_out && m1_out && m2_out && partial && gnorm2 && packed &&
                     step >= 1,
                 "bad optimizer arguments");
    DXRL_REQUIRE(n == kParams, "optimizer: n must be the padded parameter count %lld", (long long)kParams);
    DXRL_REQUIRE(params != params_out && m1 != m1_out && m2 != m2_out, "optimizer: outputs must not alias inputs");
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    constexpr int kNb = 512;
    hipLaunchKernelGGL(k_sumsq, dim3(kNb), dim3(256), 0, st, grads, n, partial);
    if (int rc = launch_check("k_sumsq")) return rc;
    AdamPackArgs a{params, grads, m1, m2, params_out, m1_out, m2_out, n, (float)lr, (float)beta1, (float)beta2,
                   (float)eps, (float)(1.0 - pow(beta1, (double)step)), (float)(1.0 - pow(beta2, (double)step)),
                   (float)max_norm, partial, kNb, gnorm2, static_cast<bf16*>(packed)};
    hipLaunchKernelGGL(k_adam_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
    return launch_check("k_adam_pack");
}

int dxrl_pg_adam_step(int32_t device, const float* params, const float* grads, const float* m1, const float* m2,
                      float* params_out, float* m1_out, float* m2_out, int64_t n, double lr, double beta1, double beta2,
                      double eps, int64_t step, double max_norm, const double* gnorm_partial, int32_t gnorm_blocks,
                      double* gnorm2, void* packed, void* stream) {
    DXRL_REQUIRE(params && grads && m1 && m2 && params_out && m1_out && m2_out && gnorm_partial && gnorm2 && packed &&
                     step >= 1 && gnorm_blocks >= 1,
                 "bad adam_step arguments");
    DXRL_REQUIRE(n == kParams, "adam_step: n must be the padded parameter count %lld", (long long)kParams);
    DXRL_REQUIRE(params != params_out && m1 != m1_out && m2 != m2_out, "adam_step: outputs must not alias inputs");
    DeviceGuard g(device);
    AdamPackArgs a{params, grads, m1, m2, params_out, m1_out, m2_out, n, (float)lr, (float)beta1, (float)beta2,
                   (float)eps, (float)(1.0 - pow(beta1, (double)step)), (float)(1.0 - pow(beta2, (double)step)),
                   (float)max_norm, gnorm_partial, gnorm_blocks, gnorm2, static_cast<bf16*>(packed)};
    hipLaunchKernelGGL(k_adam_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), a);
    return launch_check("k_adam_pack");
}

// The two controlled entry points after their own argument checks: the k_sumsq launch when the
// caller holds no norm partials, the argument block, and the launch of `kernel`.  (kl, kl_rows,
// rows) is (loss_partial, loss_blocks, pass_rows) for k_adam_pack_ctl and (records, world, unused)
// for k_adam_pack_ctl_world.
static int adam_step_ctl_launch(const char* what, void (*kernel)(AdamCtlArgs), int32_t device, const float* params,
                                const float* grads, const float* m1, const float* m2, float* params_out,
                                float* m1_out, float* m2_out, int64_t n, double beta1, double beta2, double eps,
                                double max_norm, double* gnorm_partial, int32_t gnorm_blocks, double* gnorm2,
                                void* packed, const double* kl, int32_t kl_rows, double rows,
                                const dxrl_pg_lr_control& ctl, int64_t* state, double* row_out, void* stream) {
    DXRL_REQUIRE(n == kParams, "%s: n must be the padded parameter count %lld", what, (long long)kParams);
    DXRL_REQUIRE(params != params_out && m1 != m1_out && m2 != m2_out, "%s: outputs must not alias inputs", what);
    DXRL_REQUIRE(ctl.calls >= 1 && ctl.pass_index >= 0, "%s: calls >= 1 and pass_index >= 0", what);
    DXRL_REQUIRE(ctl.lr_nominal > 0.0 && ctl.lr_min > 0.0 && ctl.lr_min <= ctl.lr_max && ctl.target_kl >= 0.0 &&
                     ctl.stop_factor > 0.0 && ctl.adapt_factor > 0.0 && ctl.adapt_band > 0.0,
                 "%s: 0 < lr_nominal, 0 < lr_min <= lr_max, target_kl >= 0, positive factors", what);
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (gnorm_blocks == 0) {  // dxrl_pg_optimizer_step's source of the norm: gnorm_partial is f64 [512] scratch
        gnorm_blocks = 512;
        hipLaunchKernelGGL(k_sumsq, dim3(gnorm_blocks), dim3(256), 0, st, grads, n, gnorm_partial);
        if (int rc = launch_check("k_sumsq")) return rc;
    }
    AdamCtlArgs x{};
    x.a = AdamPackArgs{params, grads, m1, m2, params_out, m1_out, m2_out, n, 0.0f, (float)beta1, (float)beta2,
                       (float)eps, (float)(1.0 - pow(beta1, (double)ctl.calls)),
                       (float)(1.0 - pow(beta2, (double)ctl.calls)), (float)max_norm, gnorm_partial, gnorm_blocks,
                       gnorm2, static_cast<bf16*>(packed)};
    x.c = ctl;
    x.beta1 = beta1, x.beta2 = beta2;
    x.loss = kl, x.loss_rows = kl_rows, x.rows = rows;
    // call c reads slot (c - 1) & 1 and writes slot c & 1
    x.rd = state + ((ctl.calls - 1) & 1) * DXRL_PG_OPT_SLOT_WORDS;
    x.wr = state + (ctl.calls & 1) * DXRL_PG_OPT_SLOT_WORDS;
    x.row = ctl.last_pass ? row_out : nullptr;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x);
    return launch_check(what);
}

int dxrl_pg_adam_step_ctl(int32_t device, const float* params, const float* grads, const float* m1, const float* m2,
                          float* params_out, float* m1_out, float* m2_out, int64_t n, double beta1, double beta2,
                          double eps, double max_norm, double* gnorm_partial, int32_t gnorm_blocks, double* gnorm2,
                          void* packed, const double* loss_partial, int32_t loss_blocks, int64_t pass_rows,
                          dxrl_pg_lr_control ctl, int64_t* state, double* row_out, void* stream) {
    DXRL_REQUIRE(params && grads && m1 && m2 && params_out && m1_out && m2_out && gnorm_partial && gnorm2 && packed &&
                     loss_partial && state && gnorm_blocks >= 0 && loss_blocks >= 1 && pass_rows >= 1,
                 "bad adam_step_ctl arguments");
    return adam_step_ctl_launch("adam_step_ctl", k_adam_pack_ctl, device, params, grads, m1, m2, params_out, m1_out,
                                m2_out, n, beta1, beta2, eps, max_norm, gnorm_partial, gnorm_blocks, gnorm2, packed,
                                loss_partial, loss_blocks, (double)pass_rows, ctl, state, row_out, stream);
}

int dxrl_pg_kl_rank_pack(int32_t device, const double* loss_partial, int32_t loss_blocks, int64_t pass_rows,
                         double* record, void* stream) {
    DXRL_REQUIRE(loss_partial && record && loss_blocks >= 1 && pass_rows >= 1, "bad kl_rank_pack arguments");
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_kl_rank_pack, dim3(1), dim3(256), 0, as_stream(stream), loss_partial, loss_blocks,
                       (double)pass_rows, record);
    return launch_check("k_kl_rank_pack");
}

int dxrl_pg_adam_step_ctl_world(int32_t device, const float* params, const float* grads, const float* m1,
                                const float* m2, float* params_out, float* m1_out, float* m2_out, int64_t n,
                                double beta1, double beta2, double eps, double max_norm, double* gnorm_partial,
                                int32_t gnorm_blocks, double* gnorm2, void* packed, const double* records,
                                int32_t world, dxrl_pg_lr_control ctl, int64_t* state, double* row_out,
                                void* stream) {
    DXRL_REQUIRE(params && grads && m1 && m2 && params_out && m1_out && m2_out && gnorm_partial && gnorm2 && packed &&
                     records && state && gnorm_blocks >= 0 && world >= 1,
                 "bad adam_step_ctl_world arguments");
    return adam_step_ctl_launch("adam_step_ctl_world", k_adam_pack_ctl_world, device, params, grads, m1, m2, params_out,
                                m1_out, m2_out, n, beta1, beta2, eps, max_norm, gnorm_partial, gnorm_blocks, gnorm2,
                                packed, records, world, 0.0, ctl, state, row_out, stream);
}

int dxrl_pg_adam(int32_t device, float* params, const float* grads, float* m1, float* m2, int64_t n, double lr,
                 double beta1, double beta2, double eps, int64_t step, const double* gnorm2, double max_norm,
                 void* stream) {
    DXRL_REQUIRE(params && grads && m1 && m2 && step >= 1, "bad adam arguments");
    DeviceGuard g(device);
    const float bc1 = (float)(1.0 - pow(beta1, (double)step)), bc2 = (float)(1.0 - pow(beta2, (double)step));
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), params, grads, m1,
                       m2, n, (float)lr, (float)beta1, (float)beta2, (float)eps, bc1, bc2, gnorm2,
                       (float)max_norm);
    return launch_check("k_adam");
}

}  // extern "C"
