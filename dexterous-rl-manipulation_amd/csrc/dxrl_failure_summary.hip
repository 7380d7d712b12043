// dxrl_failure_summary.hip -- the failure-mode study on the device (dxrl_failure_summarize):
// FailureClassifier.classify of evaluation/failure_taxonomy.py:156-239 per episode (mode and
// confidence), and per (group, mode) the sums behind compute_failure_distribution /
// compute_correlations (evaluation/failure_statistics.py:34-159) and analyze_failure_modes
// (evaluation/failure_analysis.py:61-99), on the record buffers dxrl_evaluate / dxrl_evaluate_mlp
// wrote.  The rules, the tie rows and the table layouts are stated in include/dxrl.h; Verdict /
// classify are dxrl_failure_rules.h's.
//
// Two launches on the caller's stream, no host synchronisation between:
//   k_failure_episodes  history form: a wave per contact_hist row (the shared row reduction of
//                       dxrl_hist_row.h, plus the peak), the taxonomy on lane 0.  Moments form: a
//                       thread per episode reads the five words the episode kernel accumulated.
//   k_failure_groups    a workgroup per (group, mode): strided accumulation over the CSR member
//                       list, then a fixed tree in LDS.  The property moments are taken about the
//                       (group, mode)'s first member -- found by a block-wide minimum first -- by
//                       push and merged with merge (dxrl_moments.h) in that fixed order, so
//                       mode_props is bit-identical from run to run (no floating-point atomics);
//                       min / max are exact.  Mode 0's workgroup also writes group_totals; one
//                       extra workgroup compacts the tie rows into tie_list in ascending order
//                       (compact_rows, dxrl_reduce.h).
#include "dxrl_failure_rules.h"
#include "dxrl_hist_row.h"
#include "dxrl_moments.h"
#include "dxrl_reduce.h"

namespace dxrl {
namespace {

constexpr int kFsThreads = 256, kFsWaves = kFsThreads / 64;
constexpr int kModes = DXRL_FAILURE_MODES;
constexpr int kFsTie = 0x80;   // ep_work: low bits mode + 1, bit 7 a tie row,
constexpr int kFsSkip = 0x40;  //          bit 6 left out of the mode tables (tie row, history form)

template <bool kMoments>
__global__ __launch_bounds__(kFsThreads) void k_failure_episodes(
    int E, int max_steps, int timeout_steps, int success_threshold, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts,
    const uint8_t* __restrict__ hist, const int32_t* __restrict__ moments, uint8_t* __restrict__ ep_work,
    int8_t* __restrict__ ep_mode, double* __restrict__ ep_confidence) {
    int e, len, n;
    HistRow h;
    if (kMoments) {
        e = blockIdx.x * kFsThreads + threadIdx.x;
        if (e >= E) return;
        len = ep_length[e];
        n = len < 0 ? 0 : (len > max_steps ? max_steps : len);
        const int32_t* m = moments + 5 * (size_t)e;
        h = HistRow{m[0], m[1], m[2], m[3], m[4]};
    } else {
        const int lane = threadIdx.x & 63;
        e = blockIdx.x * kFsWaves + (threadIdx.x >> 6);
        if (e >= E) return;  // whole waves leave together; no barrier below
        len = ep_length[e];
        n = len < 0 ? 0 : (len > max_steps ? max_steps : len);  // bytes of the row that are read
        h = hist_row_reduce<true>(hist + (size_t)e * (size_t)max_steps, n, lane);
        if (lane != 0) return;
    }
    const Verdict v = classify(ep_success[e] != 0, len, n, h.s1, h.s2, h.f5, h.l5, h.peak, ep_contacts[e],
                               timeout_steps, success_threshold);
    ep_work[e] = (uint8_t)((v.mode + 1) | (v.tie ? kFsTie | (kMoments ? 0 : kFsSkip) : 0));
    if (ep_mode) ep_mode[e] = (int8_t)v.mode;
    if (ep_confidence) ep_confidence[e] = v.conf;
}

__global__ __launch_bounds__(kFsThreads) void k_failure_groups(
    int E, int G, int num_members, const int32_t* __restrict__ group_offsets,
    const int32_t* __restrict__ group_episodes, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts,
    const double* __restrict__ ep_props, const uint8_t* __restrict__ ep_work, int64_t* __restrict__ mode_stats,
    int64_t* __restrict__ group_totals, double* __restrict__ mode_props, int32_t* __restrict__ tie_count,
    int32_t* __restrict__ tie_list, int tie_cap, int32_t* __restrict__ status) {
    __shared__ long long si[5][kFsThreads];
    __shared__ double sn[kFsThreads];
    __shared__ double sd[3][4][kFsThreads];  // per property: mean, M2, min, max
    __shared__ int scan[kFsThreads];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == G) {
        if (blockIdx.y != 0) return;
        compact_rows<kFsThreads>(E, [=](int e) { return (ep_work[e] & kFsTie) != 0; }, scan, tie_count, tie_list,
                                 tie_cap, status);
        return;
    }
    const int g = blockIdx.x, mode = blockIdx.y;
    const int lo = group_offsets[g], hi = group_offsets[g + 1];
    bool bad = lo < 0 || hi < lo || hi > num_members;
    // pass 1: the first member of this (group, mode), and the group's totals
    int first = 0x7fffffff;
    long long tot[3] = {0, 0, 0};
    if (!bad) {
        for (int m = lo + tid; m < hi; m += kFsThreads) {
            const int e = group_episodes[m];
            if (e < 0 || e >= E) {
                bad = true;
                continue;
            }
            const int w = ep_work[e];
            if ((w & 0x3f) - 1 == mode && !(w & kFsSkip) && m < first) first = m;
            tot[0] += 1;
            tot[1] += ep_success[e] != 0;
            tot[2] += (w & kFsTie) != 0;
        }
    }
    if (bad && mode == 0) atomicOr(status, 1);
    scan[tid] = first;
#pragma unroll
    for (int k = 0; k < 3; ++k) si[k][tid] = tot[k];
    __syncthreads();
    for (int s = kFsThreads / 2; s >= 1; s >>= 1) {
        if (tid < s) {
            scan[tid] = min(scan[tid], scan[tid + s]);
#pragma unroll
            for (int k = 0; k < 3; ++k) si[k][tid] += si[k][tid + s];
        }
        __syncthreads();
    }
    first = scan[0];
    if (mode == 0 && tid < 4) group_totals[4 * (size_t)g + tid] = tid < 3 ? si[tid][0] : 0;
    __syncthreads();  // si is reused below
    double K[3] = {0.0, 0.0, 0.0};
    if (first != 0x7fffffff) {
        const double* p = ep_props + 3 * (size_t)group_episodes[first];  // in range: pass 1 checked it
#pragma unroll
        for (int q = 0; q < 3; ++q) K[q] = p[q];
    }
    // pass 2: this mode's members
    long long acc[5] = {0, 0, 0, 0, 0};
    double cnt = 0.0, mean[3] = {0.0, 0.0, 0.0}, m2[3] = {0.0, 0.0, 0.0};
    double mn[3], mx[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) mn[q] = mx[q] = K[q];  // the first member is one of them
    if (first != 0x7fffffff) {
        for (int m = lo + tid; m < hi; m += kFsThreads) {
            const int e = group_episodes[m];
            if (e < 0 || e >= E) continue;
            const int w = ep_work[e];
            if ((w & 0x3f) - 1 != mode || (w & kFsSkip)) continue;
            const long long len = ep_length[e], nc = ep_contacts[e];
            acc[0] += 1;
            acc[1] += len;
            acc[2] += len * len;
            acc[3] += nc;
            acc[4] += nc * nc;
            const double* p = ep_props + 3 * (size_t)e;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const double v = p[q];
                Moments t{cnt, mean[q], m2[q]};  // the three properties share one count (sn below)
                push(t, v - K[q]);
                mean[q] = t.mean, m2[q] = t.m2;
                mn[q] = fmin(mn[q], v);
                mx[q] = fmax(mx[q], v);
            }
            cnt += 1.0;
        }
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) si[k][tid] = acc[k];
    sn[tid] = cnt;
#pragma unroll
    for (int q = 0; q < 3; ++q) sd[q][0][tid] = mean[q], sd[q][1][tid] = m2[q], sd[q][2][tid] = mn[q], sd[q][3][tid] = mx[q];
    __syncthreads();
    for (int s = kFsThreads / 2; s >= 1; s >>= 1) {  // fixed tree
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < 5; ++k) si[k][tid] += si[k][tid + s];
            const double na = sn[tid], nb = sn[tid + s];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const Moments r = merge(Moments{na, sd[q][0][tid], sd[q][1][tid]},
                                        Moments{nb, sd[q][0][tid + s], sd[q][1][tid + s]});
                sd[q][0][tid] = r.mean, sd[q][1][tid] = r.m2;
                sd[q][2][tid] = fmin(sd[q][2][tid], sd[q][2][tid + s]);
                sd[q][3][tid] = fmax(sd[q][3][tid], sd[q][3][tid + s]);
            }
            sn[tid] = na + nb;
        }
        __syncthreads();
    }
    const size_t gm = (size_t)g * kModes + mode;
    if (tid < 8) mode_stats[8 * gm + tid] = tid < 5 ? si[tid][0] : 0;
    if (tid < 15) {
        const int q = tid / 5, f = tid % 5;
        const double n = sn[0];
        double v = 0.0;
        if (n > 0.0) v = f == 0 ? n : f == 1 ? K[q] + sd[q][0][0] : sd[q][f - 1][0];
        mode_props[15 * gm + tid] = v;
    }
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_failure_summarize(int32_t device, const dxrl_failure_summary_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_failure_summary_args& a = *args;
    DXRL_REQUIRE(a.total_episodes >= 0 && a.num_groups >= 0 && a.num_members >= 0,
                 "total_episodes, num_groups and num_members must be >= 0");
    DXRL_REQUIRE(a.max_steps > 0 && a.max_steps <= DXRL_SUMMARY_MAX_STEPS,
                 "max_steps must be in [1, %d] (the exact integer variance rule), got %d", DXRL_SUMMARY_MAX_STEPS,
                 a.max_steps);
    DXRL_REQUIRE(a.ep_length && a.ep_success && a.ep_contacts && a.ep_props, "null episode record buffers");
    DXRL_REQUIRE((a.contact_hist != nullptr) != (a.hist_moments != nullptr),
                 "exactly one of contact_hist and hist_moments must be given");
    DXRL_REQUIRE(a.group_offsets && (a.group_episodes || a.num_members == 0), "null group table");
    DXRL_REQUIRE(a.ep_work && a.mode_stats && a.group_totals && a.mode_props && a.tie_count && a.status,
                 "null ep_work / mode_stats / group_totals / mode_props / tie_count / status");
    DXRL_REQUIRE(a.tie_cap >= 0 && (a.tie_list || a.tie_cap == 0), "null tie_list with tie_cap > 0");
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (int rc = hip_check(hipMemsetAsync(a.status, 0, sizeof(int32_t), st), "memset status")) return rc;
    if (a.total_episodes > 0) {
        if (a.hist_moments) {
            const int blocks = (a.total_episodes + kFsThreads - 1) / kFsThreads;
            hipLaunchKernelGGL(k_failure_episodes<true>, dim3(blocks), dim3(kFsThreads), 0, st, a.total_episodes,
                               a.max_steps, a.timeout_steps, a.success_threshold, a.ep_length, a.ep_success,
                               a.ep_contacts, a.contact_hist, a.hist_moments, a.ep_work, a.ep_mode, a.ep_confidence);
        } else {
            const int blocks = (a.total_episodes + kFsWaves - 1) / kFsWaves;
            hipLaunchKernelGGL(k_failure_episodes<false>, dim3(blocks), dim3(kFsThreads), 0, st, a.total_episodes,
                               a.max_steps, a.timeout_steps, a.success_threshold, a.ep_length, a.ep_success,
                               a.ep_contacts, a.contact_hist, a.hist_moments, a.ep_work, a.ep_mode, a.ep_confidence);
        }
        if (int rc = launch_check("k_failure_episodes")) return rc;
    }
    hipLaunchKernelGGL(k_failure_groups, dim3(a.num_groups + 1, kModes), dim3(kFsThreads), 0, st, a.total_episodes,
                       a.num_groups, a.num_members, a.group_offsets, a.group_episodes, a.ep_length, a.ep_success,
                       a.ep_contacts, a.ep_props, a.ep_work, a.mode_stats, a.group_totals, a.mode_props, a.tie_count,
                       a.tie_list, a.tie_cap, a.status);
    return launch_check("k_failure_groups");
}
