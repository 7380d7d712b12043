// dxrl_eval_summary.hip -- episode records reduced on the device (dxrl_eval_summarize):
// the failure rules of evaluation/metrics.py:39-103 per episode and the aggregates of
// metrics.py:128-206 per group, on the record buffers dxrl_evaluate / dxrl_evaluate_mlp wrote.
//
// Two launches on the caller's stream, no host synchronisation between:
//   k_summary_episodes  a wave per episode row: all the contact_hist traffic (dword loads of the
//                       row body, byte loads of an unaligned head / tail), a cross-lane reduction
//                       to (S1, S2, first-five, last-five), then the rules on lane 0
//                       (failure_word, dxrl_metrics_groups.h).
//   k_summary_groups    a workgroup per group: the group pass of dxrl_metrics_groups.h on the code
//                       byte the episode pass left in ep_work.  One extra workgroup compacts the
//                       tie rows into tie_list in ascending order (compact_rows, dxrl_reduce.h).
#include "dxrl_hist_row.h"
#include "dxrl_metrics_groups.h"

namespace dxrl {
namespace {

constexpr int kSumThreads = kGroupThreads, kSumWaves = kSumThreads / 64;

__global__ __launch_bounds__(kSumThreads) void k_summary_episodes(
    int E, int max_steps, int success_threshold, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts,
    const uint8_t* __restrict__ hist, uint8_t* __restrict__ ep_work, int8_t* __restrict__ ep_code,
    int32_t* __restrict__ ep_moments) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * kSumWaves + (threadIdx.x >> 6);
    if (e >= E) return;  // whole waves leave together; no barrier below
    const int len = ep_length[e];
    const int n = len < 0 ? 0 : (len > max_steps ? max_steps : len);  // bytes of the row that are read
    const uint8_t* row = hist + (size_t)e * (size_t)max_steps;
    const HistRow h = hist_row_reduce<false>(row, n, lane);
    if (lane != 0) return;
    const int ok = ep_success[e] != 0;
    const int nc = ok ? 0 : ep_contacts[e];  // num_contacts == final_contacts of the last step's info
    const int w = failure_word(len, ok, nc, h.s1, h.s2, h.f5, h.l5, max_steps, success_threshold);
    ep_work[e] = (uint8_t)w;
    if (ep_code) ep_code[e] = (int8_t)((w & 0x7f) - 1);
    if (ep_moments) {
        int32_t* m = ep_moments + 4 * (size_t)e;
        m[0] = h.s1, m[1] = h.s2, m[2] = h.f5, m[3] = h.l5;
    }
}

__global__ __launch_bounds__(kSumThreads) void k_summary_groups(
    int E, int G, int num_members, const int32_t* __restrict__ group_offsets,
    const int32_t* __restrict__ group_episodes, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts,
    const double* __restrict__ ep_return, const uint8_t* __restrict__ ep_work, int64_t* __restrict__ group_stats,
    double* __restrict__ group_return, int32_t* __restrict__ tie_count, int32_t* __restrict__ tie_list, int tie_cap,
    int32_t* __restrict__ status) {
    __shared__ long long si[kIntStats][kSumThreads];
    __shared__ double sd[3][kSumThreads];
    __shared__ int scan[kSumThreads];
    if ((int)blockIdx.x == G) {
        compact_rows<kSumThreads>(E, [=](int e) { return (ep_work[e] & kTieBit) != 0; }, scan, tie_count, tie_list,
                                  tie_cap, status);
        return;
    }
    metrics_group_pass(blockIdx.x, E, num_members, group_offsets, group_episodes, ep_length, ep_success, ep_contacts,
                       ep_return, CodeByte{ep_work}, group_stats, group_return, status, si, sd);
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_eval_summarize(int32_t device, const dxrl_eval_summary_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_eval_summary_args& a = *args;
    DXRL_REQUIRE(a.total_episodes >= 0 && a.num_groups >= 0 && a.num_members >= 0,
                 "total_episodes, num_groups and num_members must be >= 0");
    DXRL_REQUIRE(a.max_steps > 0 && a.max_steps <= DXRL_SUMMARY_MAX_STEPS,
                 "max_steps must be in [1, %d] (the exact integer variance rule), got %d", DXRL_SUMMARY_MAX_STEPS,
                 a.max_steps);
    DXRL_REQUIRE(a.ep_length && a.ep_success && a.ep_contacts && a.ep_return && a.contact_hist,
                 "null episode record buffers");
    DXRL_REQUIRE(a.group_offsets && (a.group_episodes || a.num_members == 0), "null group table");
    DXRL_REQUIRE(a.ep_work && a.group_stats && a.group_return && a.tie_count && a.status,
                 "null ep_work / group_stats / group_return / tie_count / status");
    DXRL_REQUIRE(a.tie_cap >= 0 && (a.tie_list || a.tie_cap == 0), "null tie_list with tie_cap > 0");
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (int rc = hip_check(hipMemsetAsync(a.status, 0, sizeof(int32_t), st), "memset status")) return rc;
    if (a.total_episodes > 0) {
        const int blocks = (a.total_episodes + kSumWaves - 1) / kSumWaves;
        hipLaunchKernelGGL(k_summary_episodes, dim3(blocks), dim3(kSumThreads), 0, st, a.total_episodes, a.max_steps,
                           a.success_threshold, a.ep_length, a.ep_success, a.ep_contacts, a.contact_hist, a.ep_work,
                           a.ep_code, a.ep_moments);
        if (int rc = launch_check("k_summary_episodes")) return rc;
    }
    hipLaunchKernelGGL(k_summary_groups, dim3(a.num_groups + 1), dim3(kSumThreads), 0, st, a.total_episodes,
                       a.num_groups, a.num_members, a.group_offsets, a.group_episodes, a.ep_length, a.ep_success,
                       a.ep_contacts, a.ep_return, a.ep_work, a.group_stats, a.group_return, a.tie_count, a.tie_list,
                       a.tie_cap, a.status);
    return launch_check("k_summary_groups");
}
