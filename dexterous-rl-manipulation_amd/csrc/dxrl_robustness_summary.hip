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
//   k_robust_groups       a workgroup per group: the member gather of k_summary_groups (about 32 B
//                         per member) plus the member's 20-byte moments row, the rules inline (no
//                         per-episode pre-pass, no ep_work), then k_summary_groups' accumulation
//                         and fixed LDS tree in its order -- group_stats and group_return are
//                         bit-identical to dxrl_eval_summarize on the same records.  One extra
//                         workgroup classifies every episode once more for ep_code and compacts
//                         the tie rows into tie_list in ascending order.
//   k_robust_degradation  a thread per group, behind the group pass: slots 0-2 of its own and its
//                         baseline's group_stats row (48 B each) -> level_table (32 B).
#include "dxrl_internal.h"

namespace dxrl {
namespace {

constexpr int kRbThreads = 256;
constexpr int kRbBatch = 4;      // group members gathered per trip of the group pass
constexpr int kRbIntStats = 14;  // group_stats slots 0..13 (14, 15 stay zero)
constexpr int kRbTie = 0x80;     // classify(): low bits code + 1, bit 7 the tie flag

// metrics.FailureType order (code k <-> list(FailureType)[k])
enum : int { F_SLIPPAGE = 0, F_UNSTABLE = 1, F_MISALIGNED = 2, F_TIMEOUT = 3, F_DROPPED = 4, F_INSUFFICIENT = 5 };

// The rules of k_summary_episodes on (len, success, contacts, S1, S2, F, L); returns
// (code + 1) | tie flag.
__device__ __forceinline__ int classify(int len, int ok, int nc, int s1, int s2, int f5, int l5, int max_steps,
                                        int success_threshold) {
    if (ok) return 0;
    if (len >= max_steps) return F_TIMEOUT + 1;  // :63-65
    if (nc == 0) return F_DROPPED + 1;           // :67-69
    // :72-83, only when the history has more than 5 entries.  np.var(counts) > 2.0 decided exactly:
    // n S2 - S1^2 > 2 n^2 (n <= 4096, counts u8: below 2^41)
    const long long nn = len;
    const long long num = nn * (long long)s2 - (long long)s1 * (long long)s1;
    const long long lim = 2 * nn * nn;
    const int tie = len > 5 && num == lim ? kRbTie : 0;
    const double trend = ((double)l5 / 5.0) - ((double)f5 / 5.0);  // the reference's f64 expression
    if (len > 5 && num > lim) return F_UNSTABLE + 1;
    if (len > 10 && trend < -1.0) return (F_SLIPPAGE + 1) | tie;
    if (nc > 0 && nc < success_threshold) return (F_MISALIGNED + 1) | tie;  // :86-87
    return (F_INSUFFICIENT + 1) | tie;                                       // :90-95
}

__device__ __forceinline__ int classify_episode(int e, int max_steps, int success_threshold,
                                                const int32_t* __restrict__ ep_length,
                                                const uint8_t* __restrict__ ep_success,
                                                const uint8_t* __restrict__ ep_contacts,
                                                const int32_t* __restrict__ moments) {
    const int32_t* m = moments + 5 * (size_t)e;
    return classify(ep_length[e], ep_success[e] != 0, ep_contacts[e], m[0], m[1], m[2], m[3], max_steps,
                    success_threshold);
}

struct Moments {
    double n, mean, m2;
};
// Chan et al.'s pairwise update (as k_summary_groups merges its return moments)
__device__ __forceinline__ Moments merge(const Moments& a, const Moments& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean;
    return Moments{n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

__global__ __launch_bounds__(kRbThreads) void k_robust_groups(
    int E, int G, int num_members, int max_steps, int success_threshold, const int32_t* __restrict__ group_offsets,
    const int32_t* __restrict__ group_episodes, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts,
    const double* __restrict__ ep_return, const int32_t* __restrict__ moments, int64_t* __restrict__ group_stats,
    double* __restrict__ group_return, int8_t* __restrict__ ep_code, int32_t* __restrict__ tie_count,
    int32_t* __restrict__ tie_list, int tie_cap, int32_t* __restrict__ status) {
    __shared__ long long si[kRbIntStats][kRbThreads];
    __shared__ double sd[3][kRbThreads];
    __shared__ int scan[kRbThreads];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == G) {
        // tie rows in ascending episode order: thread t owns episodes [t c, (t + 1) c)
        const int c = (E + kRbThreads - 1) / kRbThreads;
        const int lo = min(tid * c, E), hi = min(lo + c, E);
        int cnt = 0;
        for (int e = lo; e < hi; ++e) {
            const int w = classify_episode(e, max_steps, success_threshold, ep_length, ep_success, ep_contacts, moments);
            if (ep_code) ep_code[e] = (int8_t)((w & 0x7f) - 1);
            cnt += (w & kRbTie) != 0;
        }
        scan[tid] = cnt;
        __syncthreads();
        for (int s = 1; s < kRbThreads; s <<= 1) {  // inclusive Hillis-Steele scan
            const int v = tid >= s ? scan[tid - s] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        int at = scan[tid] - cnt;
        if (cnt)
            for (int e = lo; e < hi; ++e)
                if (classify_episode(e, max_steps, success_threshold, ep_length, ep_success, ep_contacts, moments) &
                    kRbTie) {
                    if (at < tie_cap) tie_list[at] = e;
                    ++at;
                }
        if (tid == kRbThreads - 1) {
            *tie_count = scan[tid];  // the true count, also when the list overflowed
            if (scan[tid] > tie_cap) atomicOr(status, 2);
        }
        return;
    }
    const int g = blockIdx.x;
    const int lo = group_offsets[g], hi = group_offsets[g + 1];
    long long acc[kRbIntStats];
#pragma unroll
    for (int k = 0; k < kRbIntStats; ++k) acc[k] = 0;
    Moments mo{0.0, 0.0, 0.0};
    bool bad = lo < 0 || hi < lo || hi > num_members;
    // the return moments about K, the group's first member's return (see k_summary_groups)
    double K = 0.0;
    if (!bad && lo < hi) {
        const int e0 = group_episodes[lo];
        if (e0 >= 0 && e0 < E) K = ep_return[e0];
    }
    if (!bad) {
        // kRbBatch members per trip: their gathers go out together, then they are accumulated in
        // member order -- k_summary_groups' member-to-thread assignment and order
        for (long long m0 = lo + tid; m0 < hi; m0 += kRbThreads * kRbBatch) {
            int ee[kRbBatch], len_[kRbBatch], nc_[kRbBatch], ok_[kRbBatch], mm_[kRbBatch][4];
            double x_[kRbBatch];
            bool use[kRbBatch];
#pragma unroll
            for (int b = 0; b < kRbBatch; ++b) {
                const long long m = m0 + b * kRbThreads;
                ee[b] = m < hi ? group_episodes[m] : 0;
                use[b] = m < hi && ee[b] >= 0 && ee[b] < E;
                bad |= m < hi && !use[b];
            }
#pragma unroll
            for (int b = 0; b < kRbBatch; ++b) {
                const int e = use[b] ? ee[b] : 0;  // E > 0 whenever a member is in range
                len_[b] = use[b] ? ep_length[e] : 0;
                nc_[b] = use[b] ? ep_contacts[e] : 0;
                ok_[b] = use[b] ? ep_success[e] != 0 : 0;
                x_[b] = use[b] ? ep_return[e] : 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) mm_[b][q] = use[b] ? moments[5 * (size_t)e + q] : 0;
            }
#pragma unroll
            for (int b = 0; b < kRbBatch; ++b) {
                if (!use[b]) continue;
                const long long len = len_[b], nc = nc_[b];
                const int ok = ok_[b];
                const int w = classify(len_[b], ok, nc_[b], mm_[b][0], mm_[b][1], mm_[b][2], mm_[b][3], max_steps,
                                       success_threshold);
                const int code = (w & 0x7f) - 1;
                acc[0] += 1;
                acc[1] += ok;
                acc[2] += len;
                acc[3] += len * len;
                acc[4] += nc;
                acc[5] += ok ? len : 0;
                acc[6] += ok ? nc : 0;
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[7 + k] += code == k;
                acc[13] += (w & kRbTie) != 0;
                // Welford step = Chan merge with a single value
                const double x = x_[b] - K, n1 = mo.n + 1.0, d = x - mo.mean;
                mo.mean += d / n1;
                mo.m2 += d * (x - mo.mean);
                mo.n = n1;
            }
        }
    }
    if (bad) atomicOr(status, 1);
#pragma unroll
    for (int k = 0; k < kRbIntStats; ++k) si[k][tid] = acc[k];
    sd[0][tid] = mo.n, sd[1][tid] = mo.mean, sd[2][tid] = mo.m2;
    __syncthreads();
    for (int s = kRbThreads / 2; s >= 1; s >>= 1) {  // fixed tree
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < kRbIntStats; ++k) si[k][tid] += si[k][tid + s];
            const Moments r = merge(Moments{sd[0][tid], sd[1][tid], sd[2][tid]},
                                    Moments{sd[0][tid + s], sd[1][tid + s], sd[2][tid + s]});
            sd[0][tid] = r.n, sd[1][tid] = r.mean, sd[2][tid] = r.m2;
        }
        __syncthreads();
    }
    if (tid < 16) group_stats[16 * (size_t)g + tid] = tid < kRbIntStats ? si[tid][0] : 0;
    if (tid < 3) group_return[3 * (size_t)g + tid] = tid == 1 && sd[0][0] > 0.0 ? K + sd[1][0] : sd[tid][0];
}

// robustness_analysis.py:22-75: the reference's four floats of a level, with its f64 operations
// in its order (ok / n, sum / n, base - rate, degradation / base * 100)
__global__ __launch_bounds__(kRbThreads) void k_robust_degradation(int G, const int64_t* __restrict__ group_stats,
                                                                    const int32_t* __restrict__ baseline_group,
                                                                    double* __restrict__ level_table,
                                                                    int32_t* __restrict__ status) {
    const int g = blockIdx.x * kRbThreads + threadIdx.x;
    if (g >= G) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
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
