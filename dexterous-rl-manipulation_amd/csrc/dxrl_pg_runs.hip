// dxrl_pg_runs.hip -- a set of training runs reduced on the device (include/dxrl.h,
// dxrl_pg_runs_summarize): the per-run summary and compute_ablation_statistics of
// evaluation/component_ablation.py:168-186,285-322 and the aggregate of
// evaluation/curriculum_ablation.py:269-282, on the tables PGTrainer.fit() wrote (training logs
// or validation tables, one slab per call), plus contrasts paired by seed.
//
// At most three launches on the caller's stream, no host synchronisation between:
//   k_runs_rows       a wavefront per (run, spec).  Wave lane t holds rows t, t + 64, ..: the
//                     strided column reads of one row group touch 64 rows of cols * 8 bytes.  The
//                     maximum, the first window above the threshold and the NaN count are exact
//                     reductions (order-free); curve_mean is the lane partials added in the fixed
//                     shuffle tree; the final window (a handful of rows) is lane 0's loop.
//   k_runs_groups     a wavefront per (group, spec) over the run table and the CSR member list:
//                     five Welford accumulators (push) merged with Chan et al.'s update
//                     (wave_moments, both dxrl_moments.h), min / max by the same tree
//                     (dxrl_reduce.h).
//   k_runs_contrasts  a wavefront per (contrast, spec): lane t holds positions t, t + 64, .. of
//                     the weighted groups, the weighted sum over the groups in ascending order, and
//                     the same accumulators over the positions.
// The tables of a study are a few hundred rows: every launch is latency, not bandwidth.
// No floating-point atomics (status is an integer OR): bit-identical from call to call.
#include <climits>

#include "dxrl_moments.h"
#include "dxrl_reduce.h"

namespace dxrl {
namespace {

constexpr int kWave = 64;
constexpr int kRunCols = DXRL_PG_RUNS_RUN_COLS, kMetrics = DXRL_PG_RUNS_METRICS;
constexpr int kGroupCols = DXRL_PG_RUNS_GROUP_COLS, kContrastCols = DXRL_PG_RUNS_CONTRAST_COLS;
enum : int { kStRange = 1, kStRows = 2, kStContrast = 4 };

struct Specs {
    dxrl_pg_runs_spec s[DXRL_PG_RUNS_MAX_SPECS];
};

__device__ __forceinline__ bool is_finite(double x) { return fabs(x) < __longlong_as_double(0x7ff0000000000000LL); }

__global__ __launch_bounds__(kWave) void k_runs_rows(int R, int cap, int cols, int S, const Specs specs,
                                                     const double* __restrict__ tables,
                                                     const int32_t* __restrict__ run_rows,
                                                     double* __restrict__ run_table, int32_t* __restrict__ status) {
    const int t = threadIdx.x;
    const int r = blockIdx.x / S, s = blockIdx.x % S;  // the grid is exactly R * S
    const dxrl_pg_runs_spec sp = specs.s[s];
    int n = run_rows[r];
    if (n < 0 || n > cap) {  // uniform over the wave
        if (t == 0) atomicOr(status, kStRows);
        n = 0;
    }
    const double* __restrict__ row0 = tables + (size_t)r * (size_t)cap * (size_t)cols;
    const double* __restrict__ v = row0 + sp.col;  // v[i * cols]
    const double nan = quiet_nan();

    // one pass: the maximum (first wins), the sum and the count of the non-NaN rows
    double best = 0.0, sum = 0.0;
    int best_row = -1, nans = 0, cnt = 0;
    for (int i = t; i < n; i += kWave) {
        const double x = v[(size_t)i * cols];
        if (x != x) {
            ++nans;
            continue;
        }
        if (best_row < 0 || x > best) best = x, best_row = i;
        sum += x;
        ++cnt;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // (value, row) pairs: the greater value, then the earlier row
        const double bv = __shfl_down(best, o, 64);
        const int br = __shfl_down(best_row, o, 64);
        if (br >= 0 && (best_row < 0 || bv > best || (bv == best && br < best_row))) best = bv, best_row = br;
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    nans = wave_sum(nans);

    // the first window whose mean is strictly above the threshold: lane t tries rows W - 1 + t, ..
    const int W = sp.window;
    int conv = INT_MAX;
    for (long long i = (long long)W - 1 + t; i < n; i += kWave) {
        double ws = 0.0;
        for (long long q = i - W + 1; q <= i; ++q) ws += v[(size_t)q * cols];
        if (ws / (double)W > sp.threshold) {  // false for a NaN
            conv = (int)i;
            break;  // this lane's later rows are later
        }
    }
    conv = wave_min(conv);
    if (t != 0) return;
    const int k = sp.final_window < n ? sp.final_window : n;
    double fsum = 0.0;
    for (int i = n - k; i < n; ++i) fsum += v[(size_t)i * cols];
    double* out = run_table + ((size_t)r * S + s) * kRunCols;
    out[DXRL_PG_RUNS_RUN_ROWS] = (double)n;
    out[DXRL_PG_RUNS_RUN_FINAL_WINDOW_MEAN] = k > 0 ? fsum / (double)k : nan;
    out[DXRL_PG_RUNS_RUN_BEST] = best_row >= 0 ? best : nan;
    out[DXRL_PG_RUNS_RUN_BEST_ROW] = (double)best_row;
    out[DXRL_PG_RUNS_RUN_CONVERGENCE_ROW] = conv == INT_MAX ? -1.0 : (double)conv;
    out[DXRL_PG_RUNS_RUN_X_AT_CONVERGENCE] = conv == INT_MAX ? nan : row0[(size_t)conv * cols + sp.x_col];
    out[DXRL_PG_RUNS_RUN_CURVE_MEAN] = cnt > 0 ? sum / (double)cnt : nan;
    out[DXRL_PG_RUNS_RUN_NAN_ROWS] = (double)nans;
}

// the five metrics of a run row (enum dxrl_pg_runs_metric); a run that did not converge has no
// convergence row
__device__ __forceinline__ void run_metrics(const double* __restrict__ rt, double x[kMetrics]) {
    const double conv = rt[DXRL_PG_RUNS_RUN_CONVERGENCE_ROW];
    x[DXRL_PG_RUNS_FINAL_WINDOW_MEAN] = rt[DXRL_PG_RUNS_RUN_FINAL_WINDOW_MEAN];
    x[DXRL_PG_RUNS_BEST] = rt[DXRL_PG_RUNS_RUN_BEST];
    x[DXRL_PG_RUNS_CONVERGENCE_ROW] = conv >= 0.0 ? conv : quiet_nan();
    x[DXRL_PG_RUNS_X_AT_CONVERGENCE] = rt[DXRL_PG_RUNS_RUN_X_AT_CONVERGENCE];
    x[DXRL_PG_RUNS_CURVE_MEAN] = rt[DXRL_PG_RUNS_RUN_CURVE_MEAN];
}

__device__ __forceinline__ bool bad_offsets(int lo, int hi, int num_members) {
    return lo < 0 || hi < lo || hi > num_members;
}

__global__ __launch_bounds__(kWave) void k_runs_groups(int R, int S, int num_members,
                                                       const int32_t* __restrict__ group_offsets,
                                                       const int32_t* __restrict__ group_runs,
                                                       const double* __restrict__ run_table,
                                                       double* __restrict__ group_table,
                                                       int32_t* __restrict__ status) {
    const int t = threadIdx.x;
    const int g = blockIdx.x / S, s = blockIdx.x % S;  // the grid is exactly G * S
    int lo = group_offsets[g], hi = group_offsets[g + 1];
    bool bad = bad_offsets(lo, hi, num_members);
    if (bad) lo = hi = 0;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    Moments mo[kMetrics];
    double mn[kMetrics], mx[kMetrics];
#pragma unroll
    for (int k = 0; k < kMetrics; ++k) mo[k] = Moments{0.0, 0.0, 0.0}, mn[k] = inf, mx[k] = -inf;
    int converged = 0;
    for (long long m = (long long)lo + t; m < hi; m += kWave) {
        const int r = group_runs[m];
        if (r < 0 || r >= R) {
            bad = true;
            continue;
        }
        const double* rt = run_table + ((size_t)r * S + s) * kRunCols;
        double x[kMetrics];
        run_metrics(rt, x);
        converged += rt[DXRL_PG_RUNS_RUN_CONVERGENCE_ROW] >= 0.0;
#pragma unroll
        for (int k = 0; k < kMetrics; ++k)
            if (is_finite(x[k])) {
                push(mo[k], x[k]);
                mn[k] = x[k] < mn[k] ? x[k] : mn[k];
                mx[k] = x[k] > mx[k] ? x[k] : mx[k];
            }
    }
    if (bad) atomicOr(status, kStRange);
    converged = wave_sum(converged);
#pragma unroll
    for (int k = 0; k < kMetrics; ++k) {
        mo[k] = wave_moments(mo[k]);
        mn[k] = wave_min(mn[k]);
        mx[k] = wave_max(mx[k]);
    }
    if (t != 0) return;
    const double nan = quiet_nan();
#pragma unroll
    for (int k = 0; k < kMetrics; ++k) {
        double* out = group_table + (((size_t)g * S + s) * kMetrics + k) * kGroupCols;
        const bool any = mo[k].n > 0.0;
        out[0] = mo[k].n;
        out[1] = any ? mo[k].mean : nan;
        out[2] = any ? sqrt(mo[k].m2 / mo[k].n) : nan;
        out[3] = any ? mn[k] : nan;
        out[4] = any ? mx[k] : nan;
        out[5] = (double)converged;
    }
}

__global__ __launch_bounds__(kWave) void k_runs_contrasts(int R, int S, int G, int num_members,
                                                          const int32_t* __restrict__ group_offsets,
                                                          const int32_t* __restrict__ group_runs,
                                                          const double* __restrict__ weights,
                                                          const double* __restrict__ run_table,
                                                          double* __restrict__ contrast_table,
                                                          int32_t* __restrict__ status) {
    const int t = threadIdx.x;
    const int q = blockIdx.x / S, s = blockIdx.x % S;  // the grid is exactly Q * S
    const double* __restrict__ w = weights + (size_t)q * G;
    // the member count the weighted groups share (every lane walks the same G offsets)
    int m = -1;
    bool mismatch = false;
    for (int g = 0; g < G; ++g) {
        if (w[g] == 0.0) continue;
        const int lo = group_offsets[g], hi = group_offsets[g + 1];
        if (bad_offsets(lo, hi, num_members)) {
            mismatch = true;
            continue;
        }
        if (m < 0) m = hi - lo;
        mismatch |= hi - lo != m;
    }
    double* out0 = contrast_table + ((size_t)q * S + s) * kMetrics * kContrastCols;
    const double nan = quiet_nan();
    if (mismatch) {
        if (t == 0) atomicOr(status, kStContrast);
        if (t < kMetrics * kContrastCols) out0[t] = nan;
        return;
    }
    Moments mo[kMetrics];
#pragma unroll
    for (int k = 0; k < kMetrics; ++k) mo[k] = Moments{0.0, 0.0, 0.0};
    for (int j = t; j < m; j += kWave) {
        double d[kMetrics] = {0.0, 0.0, 0.0, 0.0, 0.0};
        bool ok[kMetrics] = {true, true, true, true, true};
        for (int g = 0; g < G; ++g) {
            const double wg = w[g];
            if (wg == 0.0) continue;
            const int r = group_runs[(size_t)group_offsets[g] + j];
            if (r < 0 || r >= R) {  // the group pass reports it
#pragma unroll
                for (int k = 0; k < kMetrics; ++k) ok[k] = false;
                continue;
            }
            double x[kMetrics];
            run_metrics(run_table + ((size_t)r * S + s) * kRunCols, x);
#pragma unroll
            for (int k = 0; k < kMetrics; ++k) {
                const double term = wg * x[k];
                ok[k] = ok[k] && is_finite(term);
                d[k] += term;
            }
        }
#pragma unroll
        for (int k = 0; k < kMetrics; ++k)
            if (ok[k]) push(mo[k], d[k]);
    }
#pragma unroll
    for (int k = 0; k < kMetrics; ++k) mo[k] = wave_moments(mo[k]);
    if (t != 0) return;
#pragma unroll
    for (int k = 0; k < kMetrics; ++k) {
        double* out = out0 + k * kContrastCols;
        const double n = mo[k].n;
        const double sd = n >= 2.0 ? sqrt(mo[k].m2 / (n - 1.0)) : nan;
        const double se = sd / sqrt(n);
        out[0] = n;
        out[1] = n > 0.0 ? mo[k].mean : nan;
        out[2] = sd;
        out[3] = se;
        out[4] = n > 0.0 ? mo[k].mean / se : nan;
    }
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_pg_runs_summarize(int32_t device, const dxrl_pg_runs_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_pg_runs_args& a = *args;
    DXRL_REQUIRE(a.num_runs >= 1 && a.cap >= 1 && a.cols >= 1, "num_runs, cap and cols must be >= 1, got %d, %d, %d",
                 a.num_runs, a.cap, a.cols);
    DXRL_REQUIRE(a.num_specs >= 1 && a.num_specs <= DXRL_PG_RUNS_MAX_SPECS, "num_specs must be in [1, %d], got %d",
                 DXRL_PG_RUNS_MAX_SPECS, a.num_specs);
    DXRL_REQUIRE(a.num_groups >= 0 && a.num_contrasts >= 0 && a.num_members >= 0,
                 "num_groups, num_contrasts and num_members must be >= 0");
    DXRL_REQUIRE(a.num_contrasts == 0 || a.num_groups >= 1, "contrasts are weights over groups: num_contrasts %d with no group",
                 a.num_contrasts);
    DXRL_REQUIRE(a.tables && a.run_rows && a.specs && a.run_table && a.status,
                 "null tables / run_rows / specs / run_table / status");
    if (a.num_groups > 0) {
        DXRL_REQUIRE(a.group_offsets && a.group_table && (a.group_runs || a.num_members == 0),
                     "null group_offsets / group_runs / group_table");
    }
    if (a.num_contrasts > 0) {
        DXRL_REQUIRE(a.contrast_weights && a.contrast_table, "null contrast_weights / contrast_table");
    }
    DXRL_REQUIRE((int64_t)a.num_runs * a.num_specs <= INT_MAX && (int64_t)a.num_groups * a.num_specs <= INT_MAX &&
                     (int64_t)a.num_contrasts * a.num_specs <= INT_MAX,
                 "runs, groups or contrasts x specs exceed the grid");
    Specs specs{};
    for (int s = 0; s < a.num_specs; ++s) {
        const dxrl_pg_runs_spec& sp = a.specs[s];
        DXRL_REQUIRE(sp.col >= 0 && sp.col < a.cols && sp.x_col >= 0 && sp.x_col < a.cols,
                     "spec %d: col %d / x_col %d outside the %d columns", s, sp.col, sp.x_col, a.cols);
        DXRL_REQUIRE(sp.window >= 1 && sp.final_window >= 1, "spec %d: window and final_window must be >= 1, got %d, %d",
                     s, sp.window, sp.final_window);
        specs.s[s] = sp;
    }
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (int rc = hip_check(hipMemsetAsync(a.status, 0, sizeof(int32_t), st), "memset status")) return rc;
    const int S = a.num_specs;
    hipLaunchKernelGGL(k_runs_rows, dim3(a.num_runs * S), dim3(kWave), 0, st, a.num_runs, a.cap, a.cols, S, specs,
                       a.tables, a.run_rows, a.run_table, a.status);
    if (int rc = launch_check("k_runs_rows")) return rc;
    if (a.num_groups > 0) {
        hipLaunchKernelGGL(k_runs_groups, dim3(a.num_groups * S), dim3(kWave), 0, st, a.num_runs, S, a.num_members,
                           a.group_offsets, a.group_runs, a.run_table, a.group_table, a.status);
        if (int rc = launch_check("k_runs_groups")) return rc;
    }
    if (a.num_contrasts > 0) {
        hipLaunchKernelGGL(k_runs_contrasts, dim3(a.num_contrasts * S), dim3(kWave), 0, st, a.num_runs, S, a.num_groups,
                           a.num_members, a.group_offsets, a.group_runs, a.contrast_weights, a.run_table,
                           a.contrast_table, a.status);
        if (int rc = launch_check("k_runs_contrasts")) return rc;
    }
    return DXRL_OK;
}
