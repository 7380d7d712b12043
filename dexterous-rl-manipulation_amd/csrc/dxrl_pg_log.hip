// dxrl_pg_log.hip -- the per-iteration training log of the policy-gradient trainer
// (include/dxrl.h, dxrl_pg_log_row): learning-curve row, keep-best and convergence on the
// device, so a training run needs no host sync between its first and last iteration.
//
// Three launches per call, all behind the optimiser step on the caller's stream:
//   k_pg_log_reduce   one pass over rew / ret / values[t < T] (f32) and done (u8): 13 bytes per
//                     sample, 10.6 MB at 4096 envs x 200 steps -- HBM-bound.  Each thread owns
//                     whole groups of 16 consecutive samples (three 4 x 16-byte f32 loads and one
//                     16-byte load of done bytes per group; scalar loads where a pointer is not
//                     16-byte aligned and for the last, partial group -- the same samples in the
//                     same order either way, so alignment does not change a bit of the result).
//                     One group per thread up to 1024 workgroups (262,144 groups), so every load of
//                     the pass is in flight at once.  f64 sums; for the two variances, sums of
//                     (x - K) and (x - K)^2 about the workgroup's first sample K, which become one
//                     (count, mean, M2) triple per workgroup.  The same workgroups also sum the
//                     per-env episode counters.  Wave reduction by lane shuffles in a fixed order,
//                     the four waves through LDS; one 12-double partial per workgroup.  Nothing is
//                     read past sample M - 1.
//   k_pg_log_finish   one wave: sums the partials and merges their triples in index order (Chan),
//                     sums the learner's loss partials, writes the row, and applies the keep-best
//                     and convergence rules to the header.
//   k_pg_val_keep_best  the conditional copy the validation rows use too (dxrl_keep_best.h):
//                     params to best_params iff the row's is_best flag is set (read on the device).
//
// Sharded trainers (dxrl_pg_log_rank_pack, dxrl_pg_log_row_world) split the finish where the ranks
// must meet:
//   k_pg_log_pack         one wave behind k_pg_log_reduce: the rank's partials and loss partials to
//                         one record of DXRL_PG_LOG_RANK_DOUBLES f64 (sums, the two triples, counts),
//                         in k_pg_log_finish's reduction order.  Writes no table and no header.
//   (the caller all-gathers the ranks' records)
//   k_pg_log_finish_world one wave: merges the records in rank order and writes the row, keep-best
//                         and convergence over the records' own sample and loss-row counts, so every
//                         rank writes the same bytes; then the same conditional copy.
// gather_partials and finish_row are the two halves of the finish, each stated once: with one
// record (0 + x and merge(zero, x) are exact) the sharded pair writes dxrl_pg_log_row's bytes.
//
// No floating-point atomics, no tickets, no spin-waits: the launch order (and, between pack and
// row_world, the caller's collective) is the only ordering.
// merge and wave_moments are dxrl_moments.h's, wave_sum, quiet_nan and aligned16 dxrl_reduce.h's.
#include "dxrl_keep_best.h"
#include "dxrl_moments.h"

namespace dxrl {
namespace {

constexpr int kLogThreads = 256;       // reduce workgroup (4 waves)
constexpr int kWave = 64;
constexpr int kLogGroup = 16;          // samples per vector group
constexpr int kLogMaxBlocks = 1024;    // 4 workgroups per CU on 256 CUs
constexpr int kLogPartial = 12;        // doubles per workgroup partial
// partial layout: plain sums, then the two triples' (mean, M2) with the shared count
enum { P_REW, P_VAL, P_DONE, P_N, P_TMEAN, P_TM2, P_RMEAN, P_RM2, P_ECNT, P_ELEN, P_ESUC, P_ERET };
static_assert(P_ERET + 1 == kLogPartial, "partial layout");

inline int64_t log_grid(int64_t M) {
    const int64_t groups = (M + kLogGroup - 1) / kLogGroup;
    const int64_t blocks = (groups + kLogThreads - 1) / kLogThreads;
    return blocks < 1 ? 1 : blocks > kLogMaxBlocks ? kLogMaxBlocks : blocks;
}

// (count, mean, M2) from sums of (x - K) and (x - K)^2: this pass accumulates shifted sums, not
// Welford steps, and converts them once per workgroup
__device__ __forceinline__ Moments shifted_moments(double c, double K, double s, double s2) {
    return c > 0.0 ? Moments{c, K + s / c, fmax(s2 - s * (s / c), 0.0)} : Moments{0.0, 0.0, 0.0};
}

constexpr int kAcc = 12;  // per-thread accumulators of the reduce kernel
enum { A_REW, A_VAL, A_DONE, A_N, A_TS, A_TS2, A_RS, A_RS2, A_ECNT, A_ELEN, A_ESUC, A_ERET };

template <bool VEC>
__global__ __launch_bounds__(kLogThreads) void k_pg_log_reduce(
    const float* __restrict__ rew, const float* __restrict__ ret, const uint8_t* __restrict__ done,
    const float* __restrict__ values, int64_t M, const int32_t* __restrict__ ep_count,
    const double* __restrict__ ep_sum_return, const int32_t* __restrict__ ep_sum_length,
    const int32_t* __restrict__ ep_successes, int64_t num_envs, double* __restrict__ partial) {
    __shared__ double wred[kLogThreads / kWave][kAcc];
    const int64_t groups = (M + kLogGroup - 1) / kLogGroup;
    const int64_t gid = (int64_t)blockIdx.x * kLogThreads + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kLogThreads;
    // the workgroup's first sample exists: blockIdx.x * 256 < groups by the grid's size
    const int64_t k0 = (int64_t)blockIdx.x * kLogThreads * kLogGroup;
    const double Kt = (double)ret[k0], Kr = Kt - (double)values[k0];
    double s_rew = 0.0, s_val = 0.0, count = 0.0, ts = 0.0, ts2 = 0.0, rs = 0.0, rs2 = 0.0;
    int32_t n_done = 0;
    for (int64_t g = gid; g < groups; g += stride) {
        const int64_t base = g * kLogGroup;
        float r[kLogGroup], t[kLogGroup], v[kLogGroup];
        uint8_t d[kLogGroup];
        const int cnt = M - base >= kLogGroup ? kLogGroup : (int)(M - base);
        if (VEC && cnt == kLogGroup) {
#pragma unroll
            for (int q = 0; q < kLogGroup / 4; ++q) {
                const float4 a = *reinterpret_cast<const float4*>(rew + base + 4 * q);
                const float4 b = *reinterpret_cast<const float4*>(ret + base + 4 * q);
                const float4 c = *reinterpret_cast<const float4*>(values + base + 4 * q);
                r[4 * q] = a.x, r[4 * q + 1] = a.y, r[4 * q + 2] = a.z, r[4 * q + 3] = a.w;
                t[4 * q] = b.x, t[4 * q + 1] = b.y, t[4 * q + 2] = b.z, t[4 * q + 3] = b.w;
                v[4 * q] = c.x, v[4 * q + 1] = c.y, v[4 * q + 2] = c.z, v[4 * q + 3] = c.w;
            }
            const uint4 db = *reinterpret_cast<const uint4*>(done + base);
            const uint32_t dw[4] = {db.x, db.y, db.z, db.w};
#pragma unroll
            for (int k = 0; k < kLogGroup; ++k) d[k] = (uint8_t)(dw[k / 4] >> (8 * (k % 4)));
        } else {
#pragma unroll
            for (int k = 0; k < kLogGroup; ++k) {  // clamped: every slot loads an in-range sample
                const int64_t m = base + (k < cnt ? k : cnt - 1);
                r[k] = rew[m], t[k] = ret[m], v[k] = values[m], d[k] = done[m];
            }
        }
#pragma unroll
        for (int k = 0; k < kLogGroup; ++k) {
            if (k < cnt) {
                const double td = (double)t[k], vd = (double)v[k];
                s_rew += (double)r[k];
                s_val += vd;
                n_done += d[k] != 0;
                const double dt = td - Kt, dr = (td - vd) - Kr;
                ts += dt, ts2 += dt * dt;
                rs += dr, rs2 += dr * dr;
                count += 1.0;
            }
        }
    }
    // the episode counters (integers < 2^53: exact as doubles in any order)
    long long e_cnt = 0, e_len = 0, e_suc = 0;
    double e_ret = 0.0;
    for (int64_t i = gid; i < num_envs; i += stride) {
        e_cnt += ep_count[i], e_len += ep_sum_length[i], e_suc += ep_successes[i];
        e_ret += ep_sum_return[i];
    }
    double acc[kAcc] = {s_rew, s_val, (double)n_done, count, ts, ts2, rs, rs2,
                        (double)e_cnt, (double)e_len, (double)e_suc, e_ret};
#pragma unroll
    for (int k = 0; k < kAcc; ++k) acc[k] = wave_sum(acc[k]);
    const int wave = threadIdx.x / kWave;
    if (threadIdx.x % kWave == 0) {
#pragma unroll
        for (int k = 0; k < kAcc; ++k) wred[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[kAcc];
#pragma unroll
        for (int k = 0; k < kAcc; ++k) {
            tot[k] = wred[0][k];
            for (int w = 1; w < kLogThreads / kWave; ++w) tot[k] += wred[w][k];
        }
        const Moments mt = shifted_moments(tot[A_N], Kt, tot[A_TS], tot[A_TS2]);
        const Moments mr = shifted_moments(tot[A_N], Kr, tot[A_RS], tot[A_RS2]);
        double* p = partial + (int64_t)blockIdx.x * kLogPartial;
        p[P_REW] = tot[A_REW], p[P_VAL] = tot[A_VAL], p[P_DONE] = tot[A_DONE], p[P_N] = tot[A_N];
        p[P_TMEAN] = mt.mean, p[P_TM2] = mt.m2, p[P_RMEAN] = mr.mean, p[P_RM2] = mr.m2;
        p[P_ECNT] = tot[A_ECNT], p[P_ELEN] = tot[A_ELEN], p[P_ESUC] = tot[A_ESUC], p[P_ERET] = tot[A_ERET];
    }
}

struct FinishArgs {
    dxrl_pg_log_args a;
    int32_t blocks;
};

// What a row is computed from: the sums and triples of the whole batch, however they were gathered
// (one rank's partials in k_pg_log_finish, all ranks' records in k_pg_log_finish_world).
struct RowSums {
    double samples;                                   // M: the divisor of the per-sample columns
    double rew, val, done, eps, e_len, e_suc, e_ret;  // plain sums
    Moments mt, mr;                                   // targets, residuals
    double loss[4], loss_rows;                        // the learner's loss sums and their divisor
};

// One lane-strided pass over the workgroup partials and the learner's loss partials, each lane in
// index order, then the fixed wave order; lane 0 holds the result.  Both one-wave kernels that
// start from partials (finish, pack) run this, so they reduce in the same order to the same bits.
__device__ __forceinline__ RowSums gather_partials(const dxrl_pg_log_args& a, int32_t blocks, int lane) {
    const double* __restrict__ partial = a.partial;
    const double* __restrict__ loss_partial = a.loss_partial;
    constexpr int kSums = 7;
    constexpr int kSumIdx[kSums] = {P_REW, P_VAL, P_DONE, P_ECNT, P_ELEN, P_ESUC, P_ERET};
    double s[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    Moments mt{0.0, 0.0, 0.0}, mr{0.0, 0.0, 0.0};
#pragma unroll 4
    for (int b = lane; b < blocks; b += kWave) {
        const double* p = partial + (int64_t)b * kLogPartial;
#pragma unroll
        for (int k = 0; k < kSums; ++k) s[k] += p[kSumIdx[k]];
        mt = merge(mt, Moments{p[P_N], p[P_TMEAN], p[P_TM2]});
        mr = merge(mr, Moments{p[P_N], p[P_RMEAN], p[P_RM2]});
    }
    // the learner's loss partials
    double loss[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int64_t b = lane; b < a.loss_blocks; b += kWave) {
#pragma unroll
        for (int k = 0; k < 4; ++k) loss[k] += loss_partial[4 * b + k];
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = wave_sum(s[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) loss[k] = wave_sum(loss[k]);
    mt = wave_moments(mt);
    mr = wave_moments(mr);
    return RowSums{mt.n, s[0], s[1], s[2], s[3], s[4], s[5], s[6], mt, mr,
                   {loss[0], loss[1], loss[2], loss[3]}, (double)a.loss_rows};
}

// The row formulas, keep-best and convergence: one lane fills out[DXRL_PG_LOG_COLS] and updates the
// header.  Stated once for both finish kernels.
__device__ __forceinline__ void finish_row(const dxrl_pg_log_args& a, const RowSums& r, double* out) {
    const double M = r.samples, nan = quiet_nan();
    const double s_rew = r.rew, s_val = r.val, s_done = r.done, eps = r.eps, e_len = r.e_len, e_suc = r.e_suc,
                 e_ret = r.e_ret;
    const Moments mt = r.mt, mr = r.mr;
    for (int k = 0; k < DXRL_PG_LOG_COLS; ++k) out[k] = 0.0;
    out[DXRL_PG_LOG_ITERATION] = (double)a.iteration;
    out[DXRL_PG_LOG_ENV_STEPS] = (double)a.env_steps;
    out[DXRL_PG_LOG_EPISODES] = eps;
    out[DXRL_PG_LOG_MEAN_RETURN] = eps > 0.0 ? e_ret / eps : nan;
    out[DXRL_PG_LOG_MEAN_LENGTH] = eps > 0.0 ? e_len / eps : nan;
    out[DXRL_PG_LOG_SUCCESS_RATE] = eps > 0.0 ? e_suc / eps : nan;
    out[DXRL_PG_LOG_MEAN_STEP_REWARD] = s_rew / M;
    out[DXRL_PG_LOG_DONE_FRACTION] = s_done / M;
    out[DXRL_PG_LOG_VALUE_MEAN] = s_val / M;
    const double tvar = mt.m2 / mt.n, rvar = mr.m2 / mr.n;
    out[DXRL_PG_LOG_TARGET_MEAN] = mt.mean;
    out[DXRL_PG_LOG_TARGET_VAR] = tvar;
    out[DXRL_PG_LOG_RESIDUAL_VAR] = rvar;
    out[DXRL_PG_LOG_EXPLAINED_VARIANCE] = tvar == 0.0 ? nan : 1.0 - rvar / tvar;
    out[DXRL_PG_LOG_ADV_MEAN] = a.stats[2];
    out[DXRL_PG_LOG_ADV_STD] = a.stats[4];
    const double rows = r.loss_rows;
    out[DXRL_PG_LOG_POLICY_LOSS] = r.loss[0] / rows;
    out[DXRL_PG_LOG_VALUE_MSE] = r.loss[1] / rows;
    out[DXRL_PG_LOG_CLIP_FRAC] = r.loss[2] / rows;
    out[DXRL_PG_LOG_APPROX_KL] = r.loss[3] / rows;
    out[DXRL_PG_LOG_GRAD_NORM] = sqrt(a.gnorm2[0]);
    dxrl_pg_log_header* h = a.header;
    // keep-best: strict >, so the first maximum wins and a NaN is never best
    if (a.score_col >= 0) {
        const double score = out[a.score_col];
        if (eps >= (double)a.min_episodes && score > h->best_score) {
            out[DXRL_PG_LOG_IS_BEST] = 1.0;
            h->best_score = score;
            h->best_row = a.row;
        }
    }
    // convergence: the window's mean, oldest row first; a NaN in the window fails the test
    double wm = nan;
    if (a.conv_col >= 0 && a.row >= (int64_t)a.conv_window - 1) {
        double ws = 0.0;
        for (int64_t q = a.row - a.conv_window + 1; q < a.row; ++q) ws += a.log[q * DXRL_PG_LOG_COLS + a.conv_col];
        ws += out[a.conv_col];
        wm = ws / (double)a.conv_window;
        if (h->converged_row < 0 && wm > a.conv_threshold) h->converged_row = a.row;
    }
    out[DXRL_PG_LOG_WINDOW_MEAN] = wm;
    h->rows_written = a.row + 1;
}

__global__ __launch_bounds__(kWave) void k_pg_log_finish(const FinishArgs f) {
    __shared__ double out[DXRL_PG_LOG_COLS];
    const dxrl_pg_log_args& a = f.a;
    const int lane = threadIdx.x;
    RowSums r = gather_partials(a, f.blocks, lane);
    if (lane == 0) {
        r.samples = (double)(a.num_envs * a.horizon);
        finish_row(a, r, out);
    }
    __syncthreads();
    if (lane < DXRL_PG_LOG_COLS) a.log[a.row * DXRL_PG_LOG_COLS + lane] = out[lane];
}

// One wave: the rank's partials to its record (enum dxrl_pg_log_rank_col), in k_pg_log_finish's
// reduction order.  Writes the record and nothing else.
__global__ __launch_bounds__(kWave) void k_pg_log_pack(const FinishArgs f, double* __restrict__ record) {
    __shared__ double out[DXRL_PG_LOG_RANK_DOUBLES];
    const int lane = threadIdx.x;
    const RowSums r = gather_partials(f.a, f.blocks, lane);
    if (lane == 0) {
        for (int k = 0; k < DXRL_PG_LOG_RANK_DOUBLES; ++k) out[k] = 0.0;
        out[DXRL_PG_LOG_RANK_SAMPLES] = r.mt.n;
        out[DXRL_PG_LOG_RANK_REWARD_SUM] = r.rew;
        out[DXRL_PG_LOG_RANK_VALUE_SUM] = r.val;
        out[DXRL_PG_LOG_RANK_DONE_COUNT] = r.done;
        out[DXRL_PG_LOG_RANK_TARGET_MEAN] = r.mt.mean;
        out[DXRL_PG_LOG_RANK_TARGET_M2] = r.mt.m2;
        out[DXRL_PG_LOG_RANK_RESIDUAL_MEAN] = r.mr.mean;
        out[DXRL_PG_LOG_RANK_RESIDUAL_M2] = r.mr.m2;
        out[DXRL_PG_LOG_RANK_EPISODES] = r.eps;
        out[DXRL_PG_LOG_RANK_LENGTH_SUM] = r.e_len;
        out[DXRL_PG_LOG_RANK_SUCCESSES] = r.e_suc;
        out[DXRL_PG_LOG_RANK_RETURN_SUM] = r.e_ret;
        out[DXRL_PG_LOG_RANK_POLICY_LOSS_SUM] = r.loss[0];
        out[DXRL_PG_LOG_RANK_VALUE_SE_SUM] = r.loss[1];
        out[DXRL_PG_LOG_RANK_CLIP_SUM] = r.loss[2];
        out[DXRL_PG_LOG_RANK_KL_SUM] = r.loss[3];
        out[DXRL_PG_LOG_RANK_LOSS_ROWS] = r.loss_rows;
    }
    __syncthreads();
    if (lane < DXRL_PG_LOG_RANK_DOUBLES) record[lane] = out[lane];
}

// One wave: the ranks' records merged in rank order (plain f64 additions, the two triples by
// merge) by lane 0 -- a handful of records, and rank order is the definition -- then the row as
// k_pg_log_finish writes it, over the records' own sample and loss-row counts.  All lanes copy the
// records to rank_log[row] when it is given.
__global__ __launch_bounds__(kWave) void k_pg_log_finish_world(const dxrl_pg_log_args a,
                                                                 const double* __restrict__ records, int32_t world,
                                                                 double* __restrict__ rank_log) {
    __shared__ double out[DXRL_PG_LOG_COLS];
    const int lane = threadIdx.x;
    if (lane == 0) {
        RowSums r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, Moments{0.0, 0.0, 0.0}, Moments{0.0, 0.0, 0.0},
                  {0.0, 0.0, 0.0, 0.0}, 0.0};
        for (int32_t w = 0; w < world; ++w) {
            const double* p = records + (int64_t)w * DXRL_PG_LOG_RANK_DOUBLES;
            const double n = p[DXRL_PG_LOG_RANK_SAMPLES];
            r.rew += p[DXRL_PG_LOG_RANK_REWARD_SUM];
            r.val += p[DXRL_PG_LOG_RANK_VALUE_SUM];
            r.done += p[DXRL_PG_LOG_RANK_DONE_COUNT];
            r.mt = merge(r.mt, Moments{n, p[DXRL_PG_LOG_RANK_TARGET_MEAN], p[DXRL_PG_LOG_RANK_TARGET_M2]});
            r.mr = merge(r.mr, Moments{n, p[DXRL_PG_LOG_RANK_RESIDUAL_MEAN], p[DXRL_PG_LOG_RANK_RESIDUAL_M2]});
            r.eps += p[DXRL_PG_LOG_RANK_EPISODES];
            r.e_len += p[DXRL_PG_LOG_RANK_LENGTH_SUM];
            r.e_suc += p[DXRL_PG_LOG_RANK_SUCCESSES];
            r.e_ret += p[DXRL_PG_LOG_RANK_RETURN_SUM];
            r.loss[0] += p[DXRL_PG_LOG_RANK_POLICY_LOSS_SUM];
            r.loss[1] += p[DXRL_PG_LOG_RANK_VALUE_SE_SUM];
            r.loss[2] += p[DXRL_PG_LOG_RANK_CLIP_SUM];
            r.loss[3] += p[DXRL_PG_LOG_RANK_KL_SUM];
            r.loss_rows += p[DXRL_PG_LOG_RANK_LOSS_ROWS];
        }
        r.samples = r.mt.n;  // the sum of the records' counts (integers: exact)
        finish_row(a, r, out);
    }
    if (rank_log) {
        const int64_t words = (int64_t)world * DXRL_PG_LOG_RANK_DOUBLES;
        double* dst = rank_log + a.row * words;
        for (int64_t k = lane; k < words; k += kWave) dst[k] = records[k];
    }
    __syncthreads();
    if (lane < DXRL_PG_LOG_COLS) a.log[a.row * DXRL_PG_LOG_COLS + lane] = out[lane];
}

// What dxrl_pg_log_row checks before any launch (also the two sharded entries')
int check_log_args(const dxrl_pg_log_args& a) {
    DXRL_REQUIRE(a.num_envs >= 1 && a.horizon >= 1, "num_envs and horizon must be >= 1");
    DXRL_REQUIRE(a.cap >= 1 && a.row >= 0 && a.row < a.cap, "row %lld lies outside the table (%lld rows)",
                 (long long)a.row, (long long)a.cap);
    DXRL_REQUIRE(a.score_col < DXRL_PG_LOG_IS_BEST, "score_col %d out of range (< %d, or < 0 for none)", a.score_col,
                 (int)DXRL_PG_LOG_IS_BEST);
    DXRL_REQUIRE(a.conv_col < DXRL_PG_LOG_IS_BEST, "conv_col %d out of range (< %d, or < 0 for none)", a.conv_col,
                 (int)DXRL_PG_LOG_IS_BEST);
    DXRL_REQUIRE(a.conv_col < 0 || a.conv_window >= 1, "conv_window must be >= 1, got %d", a.conv_window);
    DXRL_REQUIRE(a.loss_blocks >= 0 && a.loss_rows >= 1, "loss_blocks must be >= 0 and loss_rows >= 1");
    DXRL_REQUIRE(a.ep_count && a.ep_sum_return && a.ep_sum_length && a.ep_successes, "null episode counters");
    DXRL_REQUIRE(a.rew && a.ret && a.done && a.values, "null rew / ret / done / values");
    DXRL_REQUIRE(a.stats && a.gnorm2 && (a.loss_partial || a.loss_blocks == 0), "null stats / gnorm2 / loss_partial");
    DXRL_REQUIRE(a.partial && a.log && a.header, "null partial / log / header");
    const int64_t blocks = log_grid(a.num_envs * a.horizon);
    DXRL_REQUIRE(a.partial_doubles >= blocks * kLogPartial, "partial holds %lld doubles, needs %lld",
                 (long long)a.partial_doubles, (long long)(blocks * kLogPartial));
    if (a.score_col >= 0 && (a.params || a.best_params))
        DXRL_REQUIRE(a.params && a.best_params && a.num_params >= 1, "keep-best needs params, best_params and num_params >= 1");
    return DXRL_OK;
}

inline bool wants_copy(const dxrl_pg_log_args& a) { return a.score_col >= 0 && (a.params || a.best_params); }

int launch_reduce(const dxrl_pg_log_args& a, int64_t blocks, hipStream_t st) {
    const int64_t M = a.num_envs * a.horizon;
    if (aligned16(a.rew) && aligned16(a.ret) && aligned16(a.done) && aligned16(a.values)) {
        hipLaunchKernelGGL(k_pg_log_reduce<true>, dim3((unsigned)blocks), dim3(kLogThreads), 0, st, a.rew, a.ret, a.done,
                           a.values, M, a.ep_count, a.ep_sum_return, a.ep_sum_length, a.ep_successes, a.num_envs,
                           a.partial);
    } else {
        hipLaunchKernelGGL(k_pg_log_reduce<false>, dim3((unsigned)blocks), dim3(kLogThreads), 0, st, a.rew, a.ret, a.done,
                           a.values, M, a.ep_count, a.ep_sum_return, a.ep_sum_length, a.ep_successes, a.num_envs,
                           a.partial);
    }
    return launch_check("k_pg_log_reduce");
}

int launch_copy(const dxrl_pg_log_args& a, hipStream_t st) {
    return launch_keep_best(st, a.log + a.row * DXRL_PG_LOG_COLS + DXRL_PG_LOG_IS_BEST, a.params, a.best_params,
                            a.num_params);
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_pg_log_partial_doubles(int64_t num_envs, int64_t horizon, int64_t* out) {
    using namespace dxrl;
    DXRL_REQUIRE(out, "null out");
    DXRL_REQUIRE(num_envs >= 1 && horizon >= 1, "num_envs and horizon must be >= 1");
    *out = log_grid(num_envs * horizon) * kLogPartial;
    return DXRL_OK;
}

extern "C" int dxrl_pg_log_row(int32_t device, const dxrl_pg_log_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_pg_log_args& a = *args;
    if (int rc = check_log_args(a)) return rc;
    const int64_t blocks = log_grid(a.num_envs * a.horizon);
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (int rc = launch_reduce(a, blocks, st)) return rc;
    FinishArgs f{a, (int32_t)blocks};
    hipLaunchKernelGGL(k_pg_log_finish, dim3(1), dim3(kWave), 0, st, f);
    if (int rc = launch_check("k_pg_log_finish")) return rc;
    if (wants_copy(a)) return launch_copy(a, st);
    return DXRL_OK;
}

extern "C" int dxrl_pg_log_rank_pack(int32_t device, const dxrl_pg_log_args* args, double* record, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    DXRL_REQUIRE(record, "null record");
    const dxrl_pg_log_args& a = *args;
    if (int rc = check_log_args(a)) return rc;
    const int64_t blocks = log_grid(a.num_envs * a.horizon);
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (int rc = launch_reduce(a, blocks, st)) return rc;
    FinishArgs f{a, (int32_t)blocks};
    hipLaunchKernelGGL(k_pg_log_pack, dim3(1), dim3(kWave), 0, st, f, record);
    return launch_check("k_pg_log_pack");
}

extern "C" int dxrl_pg_log_row_world(int32_t device, const dxrl_pg_log_args* args, const double* records,
                                     int32_t world, double* rank_log, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    DXRL_REQUIRE(records, "null records");
    DXRL_REQUIRE(world >= 1, "world must be >= 1, got %d", world);
    const dxrl_pg_log_args& a = *args;
    if (int rc = check_log_args(a)) return rc;
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_pg_log_finish_world, dim3(1), dim3(kWave), 0, st, a, records, world, rank_log);
    if (int rc = launch_check("k_pg_log_finish_world")) return rc;
    if (wants_copy(a)) return launch_copy(a, st);
    return DXRL_OK;
}
