// dxrl_robustness_summary.hip -- the robustness study on the device (dxrl_robustness_summarize):
// the failure rules of evaluation/metrics.py:39-103 per episode, the aggregates of
// metrics.py:128-206 per group and the degradation columns of
// evaluation/robustness_analysis.py:12-77 per level, on the record buffers dxrl_evaluate /
// dxrl_evaluate_mlp wrote -- from the five history words the episode kernels accumulate
// (hist_moments: S1, S2, first-five, last-five, peak), never from a contact_hist row.
//
// Tie rows (n S2 - S1^2 == 2 n^2 at the variance rule) stay as the exact comparison decides them,
// not unstable: without a history row there is nothing np.var could be asked about, the stance
// dxrl_failure_summarize takes in its moments form.  They are counted in slot 13 and listed.
//
// Two launches on the caller's stream, no host synchronisation between:
//   k_robust_groups       a workgroup per group: the group pass of dxrl_metrics_groups.h, which
//                         dxrl_eval_summarize runs too, with the member's 20-byte moments row
//                         gathered beside its record and the rules (failure_word) inline -- no
//                         per-episode pre-pass, no ep_work; group_stats and group_return are
//                         bit-identical to dxrl_eval_summarize on the same records.  One extra
//                         workgroup classifies every episode once more for ep_code and compacts
//                         the tie rows into tie_list in ascending order (compact_rows,
//                         dxrl_reduce.h).
//   k_robust_degradation  a thread per group, behind the group pass: slots 0-2 of its own and its
//                         baseline's group_stats row (48 B each) -> level_table (32 B).
#include "dxrl_metrics_groups.h"

namespace dxrl {
namespace {

constexpr int kRbThreads = kGroupThreads;

__global__ __launch_bounds__(kRbThreads) void k_robust_groups(
    int E, int G, int num_members, int max_steps, int success_threshold, const int32_t* __restrict__ group_offsets,
    const int32_t* __restrict__ group_episodes, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts,
    const double* __restrict__ ep_return, const int32_t* __restrict__ moments, int64_t* __restrict__ group_stats,
    double* __restrict__ group_return, int8_t* __restrict__ ep_code, int32_t* __restrict__ tie_count,
    int32_t* __restrict__ tie_list, int tie_cap, int32_t* __restrict__ status) {
    __shared__ long long si[kIntStats][kRbThreads];
    __shared__ double sd[3][kRbThreads];
    __shared__ int scan[kRbThreads];
    const HistWords rules{moments, max_steps, success_threshold};
    if ((int)blockIdx.x == G) {
        // every episode classified once for ep_code and the count, tie rows once more for the list
        compact_rows<kRbThreads, true>(
            E,
            [=](int e) {
                const int w = rules.word(e, ep_length, ep_success, ep_contacts);
                if (ep_code) ep_code[e] = (int8_t)((w & 0x7f) - 1);
                return (w & kTieBit) != 0;
            },
            [=](int e) { return (rules.word(e, ep_length, ep_success, ep_contacts) & kTieBit) != 0; }, scan, tie_count,
            tie_list, tie_cap, status);
        return;
    }
    metrics_group_pass(blockIdx.x, E, num_members, group_offsets, group_episodes, ep_length, ep_success, ep_contacts,
                       ep_return, rules, group_stats, group_return, status, si, sd);
}

// robustness_analysis.py:22-75: the reference's four floats of a level, with its f64 operations
// in its order (ok / n, sum / n, base - rate, degradation / base * 100)
__global__ __launch_bounds__(kRbThreads) void k_robust_degradation(int G, const int64_t* __restrict__ group_stats,
                                                                    const int32_t* __restrict__ baseline_group,
                                                                    double* __restrict__ level_table,
                                                                    int32_t* __restrict__ status) {
    const int g = blockIdx.x * kRbThreads + threadIdx.x;
    if (g >= G) return;
    const double nan = quiet_nan();
    const int64_t* s = group_stats + 16 * (size_t)g;
    const long long n = s[0];
    double rate = nan, mean_len = nan, degradation = nan, pct = nan;
    if (n > 0) {
        rate = (double)s[1] / (double)n;
        mean_len = (double)s[2] / (double)n;
    }
    const int b = baseline_group[g];
    if (b < -1 || b >= G) {
        atomicOr(status, 4);
    } else if (b >= 0 && n > 0) {
        const int64_t* sb = group_stats + 16 * (size_t)b;
        const long long nb = sb[0];
        if (nb > 0) {
            const double base = (double)sb[1] / (double)nb;
            degradation = base - rate;
            pct = base > 0.0 ? degradation / base * 100.0 : 0.0;
        }
    }
    double* out = level_table + 4 * (size_t)g;
    out[0] = rate, out[1] = mean_len, out[2] = degradation, out[3] = pct;
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_robustness_summarize(int32_t device, const dxrl_robustness_summary_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_robustness_summary_args& a = *args;
    DXRL_REQUIRE(a.total_episodes >= 0 && a.num_groups >= 0 && a.num_members >= 0,
                 "total_episodes, num_groups and num_members must be >= 0");
    DXRL_REQUIRE(a.max_steps > 0 && a.max_steps <= DXRL_SUMMARY_MAX_STEPS,
                 "max_steps must be in [1, %d] (the exact integer variance rule), got %d", DXRL_SUMMARY_MAX_STEPS,
                 a.max_steps);
    DXRL_REQUIRE(a.ep_length && a.ep_success && a.ep_contacts && a.ep_return && a.hist_moments,
                 "null episode record buffers");
    DXRL_REQUIRE(a.group_offsets && (a.group_episodes || a.num_members == 0), "null group table");
    DXRL_REQUIRE(a.baseline_group || a.num_groups == 0, "null baseline_group");
    DXRL_REQUIRE(a.group_stats && a.group_return && a.level_table && a.tie_count && a.status,
                 "null group_stats / group_return / level_table / tie_count / status");
    DXRL_REQUIRE(a.tie_cap >= 0 && (a.tie_list || a.tie_cap == 0), "null tie_list with tie_cap > 0");
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (int rc = hip_check(hipMemsetAsync(a.status, 0, sizeof(int32_t), st), "memset status")) return rc;
    hipLaunchKernelGGL(k_robust_groups, dim3(a.num_groups + 1), dim3(kRbThreads), 0, st, a.total_episodes,
                       a.num_groups, a.num_members, a.max_steps, a.success_threshold, a.group_offsets,
                       a.group_episodes, a.ep_length, a.ep_success, a.ep_contacts, a.ep_return, a.hist_moments,
                       a.group_stats, a.group_return, a.ep_code, a.tie_count, a.tie_list, a.tie_cap, a.status);
    if (int rc = launch_check("k_robust_groups")) return rc;
    if (a.num_groups == 0) return DXRL_OK;
    hipLaunchKernelGGL(k_robust_degradation, dim3((a.num_groups + kRbThreads - 1) / kRbThreads), dim3(kRbThreads), 0,
                       st, a.num_groups, a.group_stats, a.baseline_group, a.level_table, a.status);
    return launch_check("k_robust_degradation");
}
