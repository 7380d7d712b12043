// dxrl_pg_gae.hip -- the advantages phase of the policy-gradient learner: the GAE(gamma, lambda)
// reverse scan in its three forms (done byte, time limit, value normalisation), the moments of the
// advantages and returns, and the combines of the ranks' moments (include/dxrl.h states the
// semantics of every entry point).
//
// delta_t = r_t + gamma V_{t+1} (1 - d_t) - V_t ; A_t = delta_t + gamma lambda (1 - d_t) A_{t+1}
// One thread per env scans t = T-1 .. 0 (coalesced across envs), 64-env workgroups so the scan
// spreads over 64 CUs.  The loads of kGaeChunk steps go out together before that chunk's
// recurrence runs (one HBM latency per chunk, not per step).
//
// Normalisation moments without cancellation: each env accumulates f64 sums of (A - K) and
// (A - K)^2 about its own first value K = A_{T-1}, giving (count, mean, M2) with M2 the sum of
// squared deviations; workgroups, the block partials and the ranks then merge these triples
// with Chan et al.'s pairwise update in a fixed order (deterministic).  A plain
// sum(A^2) - mean sum(A) loses ~(mean/std)^2 ulps (2.8e-6 relative at mean/std = 4.6e4).
// Moments, merge and block_merge: dxrl_moments.h.
//
// Time-limit form (kTimeLimit, dxrl_pg_gae_timelimit): the tape is the rollout's u16 episode-end
// code (write_step_end: 0, or (episode length << 1) | terminated) in place of the done byte.  An
// end whose bit 0 is clear is the run_episode loop bound, a time limit: the chain stops there as at
// a termination, but the step still bootstraps -- with V_t, the critic's value of the state the
// last action was taken in, standing in for the value of the pre-reset state the rollout does not
// keep (an approximation: joints and object move by first-order dynamics, so the two states are
// close).  gae_terms states a sample's delta_t and chain coefficient c_t once per tape (k_gae_lds
// keeps its done-byte staging written out, see there); the scans, the moments and the merges are
// the same for both tapes.  Each workgroup also
// counts its real envs' (time limits, terminations) into ends[2 group], ends[2 group + 1].
//
// Value-normalisation form (kVnorm, dxrl_pg_gae_vnorm; composes with either tape): the critic's
// outputs are decoded with the block's (mu, sigma) as they are loaded, so the terms, the scans and
// the advantage moments run on raw values as they are; the decoded values go to values_raw, every
// return also to ret_norm, encoded, and the returns get a second moments triple, reduced exactly as
// the advantages' (the workgroup's triple lands in partial[workgroups + group]).
#include <type_traits>

#include "dxrl_internal.h"
#include "dxrl_moments.h"

namespace dxrl {

template <bool kTimeLimit>
using GaeTape = std::conditional_t<kTimeLimit, uint16_t, uint8_t>;
struct GaeVnorm {
    const double* state;  // the vnorm block: mu and sigma are read, nothing is written
    float* ret_norm;      // [T N]
    float* values_raw;    // [(T + 1) N]
};
// The scan kernels' optional arguments, one trailing parameter whose type the two forms select:
// `ends` with the time-limit tape, `vn` with value normalisation.  The plain done-byte form's is an
// array of no elements: size 0, so it takes no kernel-argument bytes (an empty struct has size 1,
// which pads to 8 and moves the hidden arguments).
template <bool kTimeLimit, bool kVnorm>
struct GaeExtra {
    char none[0];
};
static_assert(sizeof(GaeExtra<false, false>) == 0, "the done-byte form's trailing argument must take no kernarg bytes");
template <>
struct GaeExtra<true, false> {
    int64_t* ends;
};
template <>
struct GaeExtra<false, true> {
    GaeVnorm vn;
};
template <>
struct GaeExtra<true, true> {
    int64_t* ends;
    GaeVnorm vn;
};
__device__ __forceinline__ float gae_decode(float vn, float mu, float sigma) { return sigma * vn + mu; }
__device__ __forceinline__ float gae_encode(float ret, float mu, float sigma) { return (ret - mu) / sigma; }
// a thread's shifted sums as a triple (count c > 0)
__device__ __forceinline__ Moments gae_shifted(double c, double K, double s, double s2) {
    return Moments{c, K + s / c, fmax(s2 - s * (s / c), 0.0)};
}
// a sample's delta_t and chain coefficient c_t (gl = gamma lambda) from its tape entry: the done
// byte, or the time-limit form's episode-end code
struct GaeTerms {
    float delta, c;
};
__device__ __forceinline__ GaeTerms gae_terms(uint8_t done, float r, float v0, float v1, float gamma, float gl) {
    const float nd = done ? 0.0f : 1.0f;
    return GaeTerms{r + gamma * v1 * nd - v0, done ? 0.0f : gl};  // (gamma lambda) (1 - d_t), exactly
}
__device__ __forceinline__ GaeTerms gae_terms(uint16_t code, float r, float v0, float v1, float gamma, float gl) {
    const bool end = code != 0, term = (code & 1) != 0, timeout = end && !term;
    const float vb = timeout ? v0 : v1;
    const float nb = term ? 0.0f : 1.0f;
    return GaeTerms{r + gamma * vb * nb - v0, end ? 0.0f : gl};
}
template <typename Count>
__device__ __forceinline__ void gae_count_end(uint16_t code, Count& timeouts, Count& terminations) {
    terminations += code & 1;
    timeouts += code != 0 && !(code & 1);
}
__device__ __forceinline__ void gae_store_ends(int64_t group, int64_t timeouts, int64_t terminations, int64_t* ends) {
    ends[2 * group] = timeouts;
    ends[2 * group + 1] = terminations;
}
// Two integer counters summed over a workgroup of kWaves waves; thread 0 holds the sums afterwards
// (integers, so exact in any order).  With more than one wave every thread meets one barrier.
template <int kWaves, typename Count>
__device__ __forceinline__ void block_sum_pair(Count& a, Count& b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    if constexpr (kWaves > 1) {
        __shared__ Count wave_sums[2 * kWaves];
        if ((threadIdx.x & 63) == 0) {
            wave_sums[2 * (threadIdx.x >> 6)] = a;
            wave_sums[2 * (threadIdx.x >> 6) + 1] = b;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            a = b = 0;
            for (int w = 0; w < kWaves; ++w) {
                a += wave_sums[2 * w];
                b += wave_sums[2 * w + 1];
            }
        }
    }
}

constexpr int kGaeChunk = 32, kGaeThreads = 64;
template <bool kTimeLimit, bool kVnorm>
__global__ __launch_bounds__(kGaeThreads) void k_gae(const float* __restrict__ rew,
                                                     const GaeTape<kTimeLimit>* __restrict__ done,
                                                     const float* __restrict__ V, int64_t n, int64_t T, float gamma,
                                                     float lam, float* __restrict__ adv, float* __restrict__ ret,
                                                     Moments* __restrict__ partial, GaeExtra<kTimeLimit, kVnorm> x) {
    __shared__ Moments red[kGaeThreads];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ic = i < n ? i : n - 1;  // clamped: every lane loads, only real envs store
    double s = 0.0, s2 = 0.0, K = 0.0;
    float next_adv = 0.0f;
    float next_v = V[T * n + ic];
    [[maybe_unused]] float mu = 0.0f, sigma = 1.0f;
    [[maybe_unused]] double rs = 0.0, rs2 = 0.0, rK = 0.0;  // the returns' shifted sums
    if constexpr (kVnorm) {
        mu = (float)x.vn.state[DXRL_PG_VNORM_MU];
        sigma = (float)x.vn.state[DXRL_PG_VNORM_SIGMA];
        next_v = gae_decode(next_v, mu, sigma);
        if (i < n) x.vn.values_raw[T * n + i] = next_v;
    }
    [[maybe_unused]] int64_t n_timeout = 0, n_term = 0;
    for (int64_t hi = T; hi > 0; hi -= kGaeChunk) {
        const int64_t lo = hi - kGaeChunk > 0 ? hi - kGaeChunk : 0;
        float rv[kGaeChunk], vv[kGaeChunk];
        GaeTape<kTimeLimit> dv[kGaeChunk];
#pragma unroll
        for (int k = 0; k < kGaeChunk; ++k) {
            const int64_t t = lo + k < hi ? lo + k : hi - 1;
            const int64_t m = t * n + ic;
            rv[k] = rew[m];
            vv[k] = V[m];
            dv[k] = done[m];
        }
#pragma unroll
        for (int k = kGaeChunk - 1; k >= 0; --k) {
            if (lo + k >= hi) continue;
            if constexpr (kVnorm) vv[k] = gae_decode(vv[k], mu, sigma);
            const GaeTerms g = gae_terms(dv[k], rv[k], vv[k], next_v, gamma, gamma * lam);
            const float a = g.delta + g.c * next_adv;
            if constexpr (kTimeLimit)
                if (i < n) gae_count_end(dv[k], n_timeout, n_term);
            const int64_t m = (lo + k) * n + ic;
            if (lo + k == T - 1) K = (double)a;
            if (i < n) {
                adv[m] = a;
                ret[m] = a + vv[k];
                const double d = (double)a - K;
                s += d;
                s2 += d * d;
                if constexpr (kVnorm) {
                    const float r = a + vv[k];
                    x.vn.ret_norm[m] = gae_encode(r, mu, sigma);
                    x.vn.values_raw[m] = vv[k];
                    if (lo + k == T - 1) rK = (double)r;
                    const double rd = (double)r - rK;
                    rs += rd;
                    rs2 += rd * rd;
                }
            }
            next_adv = a;
            next_v = vv[k];
        }
    }
    block_merge<kGaeThreads>(i < n ? gae_shifted((double)T, K, s, s2) : Moments{0.0, 0.0, 0.0}, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
    if constexpr (kTimeLimit) {
        block_sum_pair<kGaeThreads / 64>(n_timeout, n_term);
        if (threadIdx.x == 0) gae_store_ends(blockIdx.x, n_timeout, n_term, x.ends);
    }
    if constexpr (kVnorm) {  // (thread 0 has read red[0]; no other thread writes it)
        block_merge<kGaeThreads>(i < n ? gae_shifted((double)T, rK, rs, rs2) : Moments{0.0, 0.0, 0.0}, red);
        if (threadIdx.x == 0) partial[gridDim.x + blockIdx.x] = red[0];
    }
}

// k_gae_lds: the same per-env recurrence (k_gae's expressions), with everything but the
// recurrence itself taken off the serial chain and the recurrence itself a 16-lane wavefront
// prefix per env (round 6, step 2 below).  A 256-thread workgroup owns 16 envs:
//   1. all 256 threads load the envs' whole horizon (rew, V_t, V_{t+1}, done; batches of
//      independent loads) and write delta_t = r_t + gamma V_{t+1} (1 - d_t) - V_t and the chain
//      coefficient c_t = (gamma lambda)(1 - d_t) (selected from the done byte) into env-major LDS
//      rows, zero-padded to a multiple of 8 steps;
//   2. A_t = delta_t + c_t A_{t+1} down the rows as a segmented scan (16 lanes per env, below);
//   3. all 256 threads write adv / ret back coalesced and accumulate the moments.
// The padded steps run first, on zeros: A stays +0, which the chain starts from anyway.
// Round 5: the chain read its operands as 16 scalar loads (delta, done byte) per 8 steps from
// time-major rows and selected c_t on it: 11.7 of the phase's 23.7 us (DXRL_GAE_DIAG ablation,
// profiles/r05/ab_gae_phases.log).
// k_gae (64 single-wave workgroups, the whole step on the chain, a memory latency per 32-step
// chunk) remains for horizons whose staging exceeds the LDS.
// ablation bits for phase timing (A/B builds only; results are wrong when set): 1 no recurrence,
// 2 no moments / merge, 4 no stores of adv / ret
#ifndef DXRL_GAE_DIAG
#define DXRL_GAE_DIAG 0
#endif
constexpr int kGlEnvs = 16, kGlThreads = 256;
// Workgroups are dispatched to the 8 XCDs round robin (block b on XCD b % 8): env group g of
// block b chosen so each XCD owns one contiguous run of groups, and the 64-byte row pieces of
// neighbouring groups (one 128-byte line) are fetched into one L2, not two.  A permutation of
// the groups for any dispatch order; partial[] stays indexed by group, so every sum is unchanged.
__device__ __forceinline__ int64_t xcd_contiguous(int64_t b, int64_t nb) {
    const int64_t q = nb / 8, rem = nb % 8, x = b % 8, j = b / 8;
    return x * q + (x < rem ? x : rem) + j;
}
// env-major row pitch (floats) of the delta / coefficient rows: the horizon padded to 8 steps,
// + 4 so the 16 lanes' 16-byte reads start on distinct bank quads (T = 200: pitch 204)
__host__ __device__ constexpr int64_t gae_pitch(int64_t T) { return (T + 7) / 8 * 8 + 4; }
// delta, coefficient and advantage rows [16][pitch] (env-major), V_t [T][16]
__host__ __device__ constexpr int64_t gae_lds_bytes(int64_t T) { return kGlEnvs * (12 * gae_pitch(T) + 4 * T); }
template <bool kTimeLimit, bool kVnorm>
__global__ __launch_bounds__(kGlThreads) void k_gae_lds(const float* __restrict__ rew,
                                                        const GaeTape<kTimeLimit>* __restrict__ done,
                                                        const float* __restrict__ V, int64_t n, int T, float gamma,
                                                        float lam, float* __restrict__ adv, float* __restrict__ ret,
                                                        Moments* __restrict__ partial,
                                                        GaeExtra<kTimeLimit, kVnorm> x) {
    extern __shared__ __attribute__((aligned(16))) float gl_lds[];
    const int P = (int)gae_pitch(T), T8 = (T + 7) / 8 * 8;
    float* Le = gl_lds;                            // [16][P] delta_t (env-major, zero past T)
    float* Ce = Le + kGlEnvs * P;                  // [16][P] c_t
    float* Vs = Ce + kGlEnvs * P;                  // [T][16] V_t (for ret)
    float* Ae = Vs + (int64_t)T * kGlEnvs;         // [16][P] A_t (env-major; the padded steps' A past T)
    __shared__ Moments red[kGlThreads];
    const int tid = threadIdx.x;
    const int64_t grp = xcd_contiguous(blockIdx.x, gridDim.x);
    const int64_t e0 = grp * kGlEnvs;
    const int64_t cnt = (int64_t)T * kGlEnvs;
    const float gl = gamma * lam;
    [[maybe_unused]] float mu = 0.0f, sigma = 1.0f;
    if constexpr (kVnorm) {
        mu = (float)x.vn.state[DXRL_PG_VNORM_MU];
        sigma = (float)x.vn.state[DXRL_PG_VNORM_SIGMA];
    }
    // 1. batches of kGlBatch elements per thread, every load issued before any lands
    constexpr int kGlBatch = 16;
    [[maybe_unused]] int n_timeout = 0, n_term = 0;  // this thread's ends of real envs (time-limit form)
    for (int64_t q0 = 0; q0 < cnt; q0 += (int64_t)kGlBatch * kGlThreads) {
        float rv[kGlBatch], v0[kGlBatch], v1[kGlBatch];
        GaeTape<kTimeLimit> dv[kGlBatch];
#pragma unroll
        for (int u = 0; u < kGlBatch; ++u) {
            const int64_t q = q0 + (int64_t)u * kGlThreads + tid;
            const int64_t qc = q < cnt ? q : cnt - 1;
            const int64_t t = qc / kGlEnvs, e = qc % kGlEnvs;
            const int64_t ic = e0 + e < n ? e0 + e : n - 1;
            rv[u] = rew[t * n + ic];
            v0[u] = V[t * n + ic];
            v1[u] = V[(t + 1) * n + ic];
            dv[u] = done[t * n + ic];
        }
#pragma unroll
        for (int u = 0; u < kGlBatch; ++u) {
            const int64_t q = q0 + (int64_t)u * kGlThreads + tid;
            if (q < cnt) {
                const int t = (int)(q / kGlEnvs), e = (int)(q % kGlEnvs);
                if constexpr (kVnorm) {  // decoded once per use: the same bits as V_t and as V_{t+1}
                    v0[u] = gae_decode(v0[u], mu, sigma);
                    v1[u] = gae_decode(v1[u], mu, sigma);
                    if (e0 + e < n) {
                        x.vn.values_raw[(int64_t)t * n + e0 + e] = v0[u];
                        if (t == T - 1) x.vn.values_raw[(int64_t)T * n + e0 + e] = v1[u];
                    }
                }
                if constexpr (kTimeLimit) {
                    const GaeTerms g = gae_terms(dv[u], rv[u], v0[u], v1[u], gamma, gl);
                    Le[e * P + t] = g.delta;
                    Ce[e * P + t] = g.c;
                    if (e0 + e < n) gae_count_end(dv[u], n_timeout, n_term);
                } else {
                    // gae_terms' done-byte rule with c_t selected after delta_t is stored: through
                    // gae_terms the compiler issues the select ahead of that store, another
                    // instruction order in the workload's kernel than the one that was measured
                    const float nd = dv[u] ? 0.0f : 1.0f;
                    Le[e * P + t] = rv[u] + gamma * v1[u] * nd - v0[u];
                    Ce[e * P + t] = dv[u] ? 0.0f : gl;  // (gamma lambda) (1 - d_t), exactly
                }
                Vs[q] = v0[u];
            }
        }
    }
    for (int k = tid; k < kGlEnvs * (T8 - T); k += kGlThreads) {  // padded steps: zeros
        const int e = k / (T8 - T), t = T + k % (T8 - T);
        Le[e * P + t] = 0.0f;
        Ce[e * P + t] = 0.0f;
    }
    // every thread meets one barrier here, which publishes the rows: block_sum_pair's, or this one
    if constexpr (kTimeLimit) {
        block_sum_pair<kGlThreads / 64>(n_timeout, n_term);
        if (tid == 0) gae_store_ends(grp, n_timeout, n_term, x.ends);
    } else {
        __syncthreads();
    }
    // 2. the recurrence A_t = delta_t + c_t A_{t+1} as a wavefront prefix: 16 lanes per env (one
    //    wave holds 4 envs), lane s owns the 8-step chunks [s nc / 16, (s + 1) nc / 16) of its env's
    //    nc = T8 / 8 chunks.  (a) each lane composes its segment into the affine map A_start =
    //    D + C A_in (D = the segment's recurrence from A_in = 0, C = the product of its c_t); (b) a
    //    Hillis-Steele suffix scan over the 16 lanes (offsets 1, 2, 4, 8: map_s <- map_s o map_{s+off})
    //    gives each lane A at the start of its segment, and lane s + 1's value is lane s's A_in;
    //    (c) each lane reruns its segment's recurrence from A_in, storing A_t.  The chain is
    //    2 (nc / 16) chunks + 4 scan steps long instead of nc chunks; inside a segment every A_t is
    //    the sequential expression, the segment boundaries' A_in carry the composition's rounding
    //    (pg_reference.gae restates this exact order).  Against one lane per env running the
    //    whole chain (round 5): advantages phase 16.0-16.7 -> 13.1-14.0 us
    //    (profiles/r06/ab_gae_scan.log).
    if (!(DXRL_GAE_DIAG & 1)) {
        const int e = tid >> 4, sg = tid & 15;
        const int nc = T8 / 8, c_lo = sg * nc / 16, c_hi = (sg + 1) * nc / 16;
        const float4* L4 = reinterpret_cast<const float4*>(Le + e * P);
        const float4* C4 = reinterpret_cast<const float4*>(Ce + e * P);
        float D = 0.0f, C = 1.0f;
        for (int k = c_hi - 1; k >= c_lo; --k) {
            const float4 l0 = L4[2 * k], l1 = L4[2 * k + 1], q0 = C4[2 * k], q1 = C4[2 * k + 1];
            const float lq[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
            const float cq[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
            for (int j = 7; j >= 0; --j) {
                D = lq[j] + cq[j] * D;
                C = cq[j] * C;
            }
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const float Dn = __shfl_down(D, off, 16), Cn = __shfl_down(C, off, 16);
            if (sg + off < 16) {
                D = D + C * Dn;
                C = C * Cn;
            }
        }
        const float Dnext = __shfl_down(D, 1, 16);
        float next_adv = sg == 15 ? 0.0f : Dnext;
        for (int k = c_hi - 1; k >= c_lo; --k) {
            const float4 l0 = L4[2 * k], l1 = L4[2 * k + 1], q0 = C4[2 * k], q1 = C4[2 * k + 1];
            const float lq[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
            const float cq[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
            float aq[8];
#pragma unroll
            for (int j = 7; j >= 0; --j) {
                aq[j] = lq[j] + cq[j] * next_adv;
                next_adv = aq[j];
            }
            float4* A4 = reinterpret_cast<float4*>(Ae + e * P + 8 * k);
            A4[0] = make_float4(aq[0], aq[1], aq[2], aq[3]);
            A4[1] = make_float4(aq[4], aq[5], aq[6], aq[7]);
        }
    }
    __syncthreads();
    // 3. store, and the moments of this thread's elements about its first one (merged with Chan's
    // update below and across workgroups: any shift point gives the same moments up to rounding)
    double s = 0.0, s2 = 0.0, K = 0.0, c = 0.0;
    [[maybe_unused]] double rs = 0.0, rs2 = 0.0, rK = 0.0;  // the returns' shifted sums (count c too)
    for (int64_t q = tid; q < cnt; q += kGlThreads) {
        const int64_t t = q / kGlEnvs, e = q % kGlEnvs;
        if (e0 + e < n) {
            const float a = Ae[e * P + t];
            if (!(DXRL_GAE_DIAG & 4)) {
                adv[t * n + e0 + e] = a;
                ret[t * n + e0 + e] = a + Vs[q];
                if constexpr (kVnorm) x.vn.ret_norm[t * n + e0 + e] = gae_encode(a + Vs[q], mu, sigma);
            }
            if (DXRL_GAE_DIAG & 2) continue;
            if constexpr (kVnorm) {
                const float r = a + Vs[q];
                if (c == 0.0) rK = (double)r;
                const double rd = (double)r - rK;
                rs += rd;
                rs2 += rd * rd;
            }
            if (c == 0.0) K = (double)a;
            const double d = (double)a - K;
            s += d;
            s2 += d * d;
            c += 1.0;
        }
    }
    const Moments mo = c > 0.0 ? gae_shifted(c, K, s, s2) : Moments{0.0, 0.0, 0.0};
    if (DXRL_GAE_DIAG & 2) {
        if (tid == 0) partial[grp] = mo;
        if constexpr (kVnorm)
            if (tid == 0) partial[gridDim.x + grp] = mo;
        return;
    }
    block_merge<kGlThreads>(mo, red);
    if (tid == 0) partial[grp] = red[0];
    if constexpr (kVnorm) {  // (thread 0 has read red[0]; no other thread writes it)
        block_merge<kGlThreads>(c > 0.0 ? gae_shifted(c, rK, rs, rs2) : Moments{0.0, 0.0, 0.0}, red);
        if (tid == 0) partial[gridDim.x + grp] = red[0];
    }
}

// Value normalisation: one batch of returns folded into the block's running triple, and the next
// call's constants from it (one thread; include/dxrl.h states the words).  The running triple is
// discounted first with d = 1 - FORGET (count and M2; the mean stays): d = 1 on a block without
// forgetting, which multiplies exactly.
__device__ __forceinline__ void vnorm_fold(double* __restrict__ vn, Moments batch, double eps) {
    const double d = 1.0 - vn[DXRL_PG_VNORM_FORGET];
    const Moments run =
        merge(Moments{d * vn[DXRL_PG_VNORM_COUNT], vn[DXRL_PG_VNORM_MEAN], d * vn[DXRL_PG_VNORM_M2]}, batch);
    vn[DXRL_PG_VNORM_COUNT] = run.n;
    vn[DXRL_PG_VNORM_MEAN] = run.mean;
    vn[DXRL_PG_VNORM_M2] = run.m2;
    vn[DXRL_PG_VNORM_CALLS] += 1.0;
    if (run.n > 0.0) {
        vn[DXRL_PG_VNORM_MU] = (double)(float)run.mean;
        vn[DXRL_PG_VNORM_SIGMA] = (double)(float)sqrt(run.m2 / run.n + eps);
    }
}
__device__ __forceinline__ void vnorm_store_batch(double* __restrict__ vn, Moments ret, Moments adv) {
    vn[DXRL_PG_VNORM_BATCH_COUNT] = ret.n;
    vn[DXRL_PG_VNORM_BATCH_MEAN] = ret.mean;
    vn[DXRL_PG_VNORM_BATCH_M2] = ret.m2;
    vn[DXRL_PG_VNORM_ADV_COUNT] = adv.n;
    vn[DXRL_PG_VNORM_ADV_MEAN] = adv.mean;
    vn[DXRL_PG_VNORM_ADV_M2] = adv.m2;
}

// Global statistics from the ranks' (count, mean, M2) triples, merged in rank order:
// stats[0] count, [1] sum, [2] mean, [3] sum of squared deviations, [4] unbiased std
// (kStride doubles from one rank's triple to the next)
template <int kStride>
__device__ __forceinline__ Moments merge_ranks(const double* __restrict__ moments, int world) {
    Moments a{0.0, 0.0, 0.0};
    for (int r = 0; r < world; ++r)
        a = merge(a, Moments{moments[kStride * r], moments[kStride * r + 1], moments[kStride * r + 2]});
    return a;
}
template <int kStride>
__device__ __forceinline__ Moments stats_combine(const double* __restrict__ moments, int world, double* stats) {
    const Moments a = merge_ranks<kStride>(moments, world);
    stats[0] = a.n;
    stats[1] = a.n * a.mean;
    stats[2] = a.mean;
    stats[3] = a.m2;
    stats[4] = sqrt(a.m2 / (a.n > 1.0 ? a.n - 1.0 : 1.0));
    return a;
}
__global__ void k_stats_combine(const double* __restrict__ moments, int world, double* stats) {
    stats_combine<3>(moments, world, stats);
}
// dxrl_pg_vnorm_combine: rows (return triple, advantage triple) in rank order; one thread
__global__ void k_vnorm_combine(const double* __restrict__ moments6, int world, double* stats,
                                double* __restrict__ vn) {
    const Moments adv = stats_combine<6>(moments6 + 3, world, stats), batch = merge_ranks<6>(moments6, world);
    vnorm_store_batch(vn, batch, adv);
    vnorm_fold(vn, batch, vn[DXRL_PG_VNORM_EPS]);
}

// nb workgroup triples merged by the 256 threads: thread-strided in index order, then block_merge's
// tree; thread 0 holds the result
__device__ __forceinline__ Moments gae_merge_partials(const Moments* __restrict__ partial, int nb) {
    // one array for every call: block_merge ends with a barrier, after which only thread 0 reads
    // red[0], and the next call's first write to red[0] is thread 0's own
    __shared__ Moments red[256];
    Moments a{0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < nb; k += blockDim.x) a = merge(a, partial[k]);
    block_merge<256>(a, red);
    return threadIdx.x == 0 ? red[0] : Moments{0.0, 0.0, 0.0};
}
// The finishing launch of every form, one 256-thread workgroup.
// The rank's advantage moments, contiguous so ranks exchange them as one 3-element block:
// stats[5] = count, stats[6] = mean, stats[7] = M2 (sum of squared deviations), and from them the
// single-rank statistics stats[0..4] (== dxrl_pg_adv_combine(stats + 5, world = 1), which a
// multi-rank caller runs afterwards over the all-gathered triples, overwriting these).
// kTimeLimit: the workgroups' (time limits, terminations) pairs counts[2 + 2 g], counts[3 + 2 g]
// summed into counts[0], counts[1].
// kVnorm: the workgroups' return triples partial[nb ..] merged in the advantage triples' order, the
// batch words of the block and, with fold, the fold.  The scan kernel before it has read mu / sigma
// already.
template <bool kTimeLimit, bool kVnorm>
__global__ void k_gae_finish(const Moments* __restrict__ partial, int nb, double* __restrict__ stats,
                             int64_t* __restrict__ counts, double* __restrict__ vn, double eps, int fold) {
    const Moments adv = gae_merge_partials(partial, nb);
    if (threadIdx.x == 0) {
        stats[5] = adv.n;
        stats[6] = adv.mean;
        stats[7] = adv.m2;
        stats_combine<3>(stats + 5, 1, stats);  // reads stats[5..7], writes stats[0..4]: disjoint
    }
    if constexpr (kTimeLimit) {
        int64_t to = 0, te = 0;
        for (int k = threadIdx.x; k < nb; k += blockDim.x) {
            to += counts[2 + 2 * k];
            te += counts[3 + 2 * k];
        }
        block_sum_pair<256 / 64>(to, te);
        if (threadIdx.x == 0) {
            counts[0] = to;
            counts[1] = te;
        }
    }
    if constexpr (kVnorm) {  // (thread 0 has read its result; no other thread writes red[0])
        const Moments batch = gae_merge_partials(partial + nb, nb);
        if (threadIdx.x == 0) {
            vnorm_store_batch(vn, batch, Moments{stats[5], stats[6], stats[7]});  // this thread wrote them
            vn[DXRL_PG_VNORM_EPS] = eps;
            if (fold) vnorm_fold(vn, batch, eps);
        }
    }
}

namespace {
bool gae_seq_forced() {  // A/B: k_gae, the chunked-load scan (DXRL_GAE_SEQ=1)
    static const bool seq = [] {
        const char* v = getenv("DXRL_GAE_SEQ");
        return v && atoi(v) != 0;
    }();
    return seq;
}

// The two launches of every form.  k_gae_lds while the horizon's staging fits the LDS it may ask
// for (152 of the CU's 160 KiB), else k_gae; then the finishing kernel.  The plain entry points
// pass a dxrl_pg_gae_vnorm_args too, with the members of the forms they lack left null.
constexpr int64_t kGaeLdsLimit = 152 * 1024;
template <bool kTimeLimit, bool kVnorm>
int gae_launch(const dxrl_pg_gae_vnorm_args& a, hipStream_t st) {
    // launch-error labels by form, as the entry points have always reported them
    constexpr const char* lds_name = kVnorm ? "k_gae_lds<vnorm>" : kTimeLimit ? "k_gae_lds<true>" : "k_gae_lds";
    constexpr const char* seq_name = kVnorm ? "k_gae<vnorm>" : kTimeLimit ? "k_gae<true>" : "k_gae";
    const auto lds_kernel = k_gae_lds<kTimeLimit, kVnorm>;
    const auto seq_kernel = k_gae<kTimeLimit, kVnorm>;
    static const bool attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kGaeLdsLimit) == hipSuccess;
    const GaeTape<kTimeLimit>* tape;
    GaeExtra<kTimeLimit, kVnorm> x{};
    if constexpr (kTimeLimit) {
        tape = a.ep_code;
        x.ends = a.counts + 2;  // the workgroups' pairs
    } else {
        tape = a.done;
    }
    if constexpr (kVnorm) x.vn = GaeVnorm{a.vnorm, a.ret_norm, a.values_raw};
    Moments* partial = reinterpret_cast<Moments*>(a.partial);
    const int64_t lds = gae_lds_bytes(a.horizon);
    int nb;
    if (!gae_seq_forced() && attr && lds <= kGaeLdsLimit) {
        nb = (int)((a.num_envs + kGlEnvs - 1) / kGlEnvs);
        hipLaunchKernelGGL(lds_kernel, dim3(nb), dim3(kGlThreads), (size_t)lds, st, a.rew, tape, a.values,
                           a.num_envs, (int)a.horizon, (float)a.gamma, (float)a.lam, a.adv, a.ret, partial, x);
        if (int rc = launch_check(lds_name)) return rc;
    } else {
        nb = (int)((a.num_envs + kGaeThreads - 1) / kGaeThreads);
        hipLaunchKernelGGL(seq_kernel, dim3(nb), dim3(kGaeThreads), 0, st, a.rew, tape, a.values, a.num_envs,
                           a.horizon, (float)a.gamma, (float)a.lam, a.adv, a.ret, partial, x);
        if (int rc = launch_check(seq_name)) return rc;
    }
    hipLaunchKernelGGL((k_gae_finish<kTimeLimit, kVnorm>), dim3(1), dim3(256), 0, st, partial, nb, a.stats, a.counts,
                       a.vnorm, a.eps, (int)a.fold);
    return launch_check("k_gae_finish");
}
}  // namespace

}  // namespace dxrl

using namespace dxrl;

extern "C" {

int dxrl_pg_gae_partial_doubles(int64_t num_envs, int64_t horizon, int64_t* doubles) {
    DXRL_REQUIRE(doubles && num_envs >= 1 && horizon >= 1, "bad argument");
    // one Moments triple per workgroup; k_gae_lds (16 envs per workgroup) launches the most
    static_assert(kGlEnvs <= kGaeThreads, "k_gae_lds must be the kernel with the most workgroups");
    *doubles = 3 * ((num_envs + kGlEnvs - 1) / kGlEnvs);
    return DXRL_OK;
}

int dxrl_pg_gae(int32_t device, const float* rew, const uint8_t* done, const float* values, int64_t num_envs,
                int64_t horizon, double gamma, double lam, float* adv, float* ret, double* partial, double* stats,
                void* stream) {
    DXRL_REQUIRE(rew && done && values && adv && ret && partial && stats, "null argument");
    DXRL_REQUIRE(num_envs >= 1 && horizon >= 1, "num_envs and horizon must be >= 1");
    DeviceGuard g(device);
    dxrl_pg_gae_vnorm_args a{};
    a.rew = rew, a.done = done, a.values = values, a.num_envs = num_envs, a.horizon = horizon;
    a.gamma = gamma, a.lam = lam, a.adv = adv, a.ret = ret, a.partial = partial, a.stats = stats;
    return gae_launch<false, false>(a, as_stream(stream));
}

int dxrl_pg_gae_timelimit_count_words(int64_t num_envs, int64_t horizon, int64_t* words) {
    DXRL_REQUIRE(words && num_envs >= 1 && horizon >= 1, "bad argument");
    // the two sums, then one (time limits, terminations) pair per workgroup of k_gae_lds
    *words = 2 + 2 * ((num_envs + kGlEnvs - 1) / kGlEnvs);
    return DXRL_OK;
}

int dxrl_pg_gae_timelimit(int32_t device, const float* rew, const uint16_t* ep_code, const float* values,
                          int64_t num_envs, int64_t horizon, double gamma, double lam, float* adv, float* ret,
                          double* partial, double* stats, int64_t* counts, void* stream) {
    DXRL_REQUIRE(rew && ep_code && values && adv && ret && partial && stats && counts, "null argument");
    DXRL_REQUIRE(num_envs >= 1 && horizon >= 1, "num_envs and horizon must be >= 1");
    DeviceGuard g(device);
    dxrl_pg_gae_vnorm_args a{};
    a.rew = rew, a.ep_code = ep_code, a.values = values, a.num_envs = num_envs, a.horizon = horizon;
    a.gamma = gamma, a.lam = lam, a.adv = adv, a.ret = ret, a.partial = partial, a.stats = stats, a.counts = counts;
    return gae_launch<true, false>(a, as_stream(stream));
}

int dxrl_pg_gae_vnorm_partial_doubles(int64_t num_envs, int64_t horizon, int64_t* doubles) {
    DXRL_REQUIRE(doubles && num_envs >= 1 && horizon >= 1, "bad argument");
    // two Moments triples per workgroup (advantages, then returns); k_gae_lds launches the most
    *doubles = 2 * 3 * ((num_envs + kGlEnvs - 1) / kGlEnvs);
    return DXRL_OK;
}

int dxrl_pg_gae_vnorm(int32_t device, const dxrl_pg_gae_vnorm_args* a, void* stream) {
    DXRL_REQUIRE(a, "null args");
    DXRL_REQUIRE(a->rew && a->values && a->adv && a->ret && a->ret_norm && a->values_raw && a->partial && a->stats &&
                     a->vnorm,
                 "null argument");
    DXRL_REQUIRE((a->done != nullptr) != (a->ep_code != nullptr), "exactly one of done and ep_code selects the rule");
    DXRL_REQUIRE(!a->ep_code || a->counts, "the time-limit rule needs counts");
    DXRL_REQUIRE(a->num_envs >= 1 && a->horizon >= 1, "num_envs and horizon must be >= 1");
    DXRL_REQUIRE(a->eps >= 0.0, "eps must be >= 0");
    DeviceGuard g(device);
    return a->ep_code ? gae_launch<true, true>(*a, as_stream(stream)) : gae_launch<false, true>(*a, as_stream(stream));
}

int dxrl_pg_vnorm_combine(int32_t device, const double* moments6, int32_t world, double* stats, double* vnorm,
                          void* stream) {
    DXRL_REQUIRE(moments6 && stats && vnorm && world >= 1, "bad argument");
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_vnorm_combine, dim3(1), dim3(1), 0, as_stream(stream), moments6, world, stats, vnorm);
    return launch_check("k_vnorm_combine");
}

int dxrl_pg_adv_combine(int32_t device, const double* moments, int32_t world, double* stats, void* stream) {
    DXRL_REQUIRE(moments && stats && world >= 1, "bad argument");
    DeviceGuard g(device);
    hipLaunchKernelGGL(k_stats_combine, dim3(1), dim3(1), 0, as_stream(stream), moments, world, stats);
    return launch_check("k_stats_combine");
}

int dxrl_pg_adv_finalize(int32_t device, int32_t phase, const float* adv, int64_t count, double* partial,
                         double* stats, void* stream) {
    DXRL_REQUIRE(stats, "null argument");
    DXRL_REQUIRE(phase == 2, "phase must be 2 (the two-pass phases 0 / 1 were retired for the merged moments)");
    (void)adv, (void)count, (void)partial;
    return dxrl_pg_adv_combine(device, stats + 5, 1, stats, stream);
}

}  // extern "C"
