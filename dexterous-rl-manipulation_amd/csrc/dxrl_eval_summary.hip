// dxrl_eval_summary.hip -- episode records reduced on the device (dxrl_eval_summarize):
// the failure rules of evaluation/metrics.py:39-103 per episode and the aggregates of
// metrics.py:128-206 per group, on the record buffers dxrl_evaluate / dxrl_evaluate_mlp wrote.
//
// Two launches on the caller's stream, no host synchronisation between:
//   k_summary_episodes  a wave per episode row: all the contact_hist traffic (dword loads of the
//                       row body, byte loads of an unaligned head / tail), a cross-lane reduction
//                       to (S1, S2, first-five, last-five), then the rules on lane 0.
//   k_summary_groups    a workgroup per group: strided accumulation over the CSR member list
//                       (about 32 B per member), then a fixed tree in LDS -- the return moments,
//                       taken about the group's first return, merge with Chan et al.'s update in
//                       that fixed order, so group_return is bit-identical from run to run (no
//                       floating-point atomics).  One extra
//                       workgroup compacts the tie rows into tie_list in ascending order.
#include "dxrl_hist_row.h"
#include "dxrl_internal.h"

namespace dxrl {
namespace {

constexpr int kSumThreads = 256, kSumWaves = kSumThreads / 64;
constexpr int kBatch = 4;      // group members gathered per trip of the group pass
constexpr int kIntStats = 14;  // group_stats slots 0..13 (14, 15 stay zero)
constexpr int kTieBit = 0x80;  // ep_work: low bits code + 1, bit 7 the tie flag

// metrics.FailureType order (code k <-> list(FailureType)[k])
enum : int { F_SLIPPAGE = 0, F_UNSTABLE = 1, F_MISALIGNED = 2, F_TIMEOUT = 3, F_DROPPED = 4, F_INSUFFICIENT = 5 };

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
    const int s1 = h.s1, s2 = h.s2, f5 = h.f5, l5 = h.l5;
    if (lane != 0) return;
    int code = -1, tie = 0;
    if (!ep_success[e]) {
        const int nc = ep_contacts[e];  // num_contacts == final_contacts of the last step's info
        if (len >= max_steps) {
            code = F_TIMEOUT;  // :63-65
        } else if (nc == 0) {
            code = F_DROPPED;  // :67-69
        } else {
            // :72-83, only when the history has more than 5 entries.  np.var(counts) > 2.0 decided
            // exactly: n S2 - S1^2 > 2 n^2 (n <= 4096, counts u8: below 2^41)
            const long long nn = len;
            const long long num = nn * (long long)s2 - (long long)s1 * (long long)s1;
            const long long lim = 2 * nn * nn;
            tie = len > 5 && num == lim;  // np.var's own rounding decides: left to the host
            const double trend = ((double)l5 / 5.0) - ((double)f5 / 5.0);  // the reference's f64 expression
            if (len > 5 && num > lim) code = F_UNSTABLE;
            else if (len > 10 && trend < -1.0) code = F_SLIPPAGE;
            else if (nc > 0 && nc < success_threshold) code = F_MISALIGNED;  // :86-87
            else code = F_INSUFFICIENT;                                       // :90-95
        }
    }
    ep_work[e] = (uint8_t)((code + 1) | (tie ? kTieBit : 0));
    if (ep_code) ep_code[e] = (int8_t)code;
    if (ep_moments) {
        int32_t* m = ep_moments + 4 * (size_t)e;
        m[0] = s1, m[1] = s2, m[2] = f5, m[3] = l5;
    }
}

struct Moments {
    double n, mean, m2;
};
// Chan et al.'s pairwise update (as dxrl_pg_gae merges its advantage moments)
__device__ __forceinline__ Moments merge(const Moments& a, const Moments& b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean;
    return Moments{n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
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
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == G) {
        // tie rows in ascending episode order: thread t owns episodes [t c, (t + 1) c)
        const int c = (E + kSumThreads - 1) / kSumThreads;
        const int lo = min(tid * c, E), hi = min(lo + c, E);
        int cnt = 0;
        for (int e = lo; e < hi; ++e) cnt += (ep_work[e] & kTieBit) != 0;
        scan[tid] = cnt;
        __syncthreads();
        for (int s = 1; s < kSumThreads; s <<= 1) {  // inclusive Hillis-Steele scan
            const int v = tid >= s ? scan[tid - s] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        int at = scan[tid] - cnt;
        for (int e = lo; e < hi; ++e)
            if (ep_work[e] & kTieBit) {
                if (at < tie_cap) tie_list[at] = e;
                ++at;
            }
        if (tid == kSumThreads - 1) {
            *tie_count = scan[tid];  // the true count, also when the list overflowed
            if (scan[tid] > tie_cap) atomicOr(status, 2);
        }
        return;
    }
    const int g = blockIdx.x;
    const int lo = group_offsets[g], hi = group_offsets[g + 1];
    long long acc[kIntStats];
#pragma unroll
    for (int k = 0; k < kIntStats; ++k) acc[k] = 0;
    Moments mo{0.0, 0.0, 0.0};
    bool bad = lo < 0 || hi < lo || hi > num_members;
    // The return moments are taken about K, the group's first member's return (as dxrl_pg_gae takes
    // an env's about its first advantage): with returns of the form -1e6 + small, a running mean
    // held as an absolute f64 rounds at 1e-10 and costs M2 ~1e-8 relative; about K it does not.
    double K = 0.0;
    if (!bad && lo < hi) {
        const int e0 = group_episodes[lo];
        if (e0 >= 0 && e0 < E) K = ep_return[e0];
    }
    if (!bad) {
        // kBatch members per trip: their gathers go out together (one memory latency per trip, a big
        // group is a chain of trips on one workgroup), then they are accumulated in member order
        for (long long m0 = lo + tid; m0 < hi; m0 += kSumThreads * kBatch) {
            int ee[kBatch], len_[kBatch], nc_[kBatch], ok_[kBatch], w_[kBatch];
            double x_[kBatch];
            bool use[kBatch];
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const long long m = m0 + b * kSumThreads;
                ee[b] = m < hi ? group_episodes[m] : 0;
                use[b] = m < hi && ee[b] >= 0 && ee[b] < E;
                bad |= m < hi && !use[b];
            }
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const int e = use[b] ? ee[b] : 0;  // E > 0 whenever a member is in range
                len_[b] = use[b] ? ep_length[e] : 0;
                nc_[b] = use[b] ? ep_contacts[e] : 0;
                ok_[b] = use[b] ? ep_success[e] != 0 : 0;
                w_[b] = use[b] ? ep_work[e] : 0;
                x_[b] = use[b] ? ep_return[e] : 0.0;
            }
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                if (!use[b]) continue;
                const long long len = len_[b], nc = nc_[b];
                const int ok = ok_[b], w = w_[b], code = (w & 0x7f) - 1;
                acc[0] += 1;
                acc[1] += ok;
                acc[2] += len;
                acc[3] += len * len;
                acc[4] += nc;
                acc[5] += ok ? len : 0;
                acc[6] += ok ? nc : 0;
#pragma unroll
                for (int k = 0; k < 6; ++k) acc[7 + k] += code == k;
                acc[13] += (w & kTieBit) != 0;
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
    for (int k = 0; k < kIntStats; ++k) si[k][tid] = acc[k];
    sd[0][tid] = mo.n, sd[1][tid] = mo.mean, sd[2][tid] = mo.m2;
    __syncthreads();
    for (int s = kSumThreads / 2; s >= 1; s >>= 1) {  // fixed tree
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < kIntStats; ++k) si[k][tid] += si[k][tid + s];
            const Moments r = merge(Moments{sd[0][tid], sd[1][tid], sd[2][tid]},
                                    Moments{sd[0][tid + s], sd[1][tid + s], sd[2][tid + s]});
            sd[0][tid] = r.n, sd[1][tid] = r.mean, sd[2][tid] = r.m2;
        }
        __syncthreads();
    }
    if (tid < 16) group_stats[16 * (size_t)g + tid] = tid < kIntStats ? si[tid][0] : 0;
    if (tid < 3) group_return[3 * (size_t)g + tid] = tid == 1 && sd[0][0] > 0.0 ? K + sd[1][0] : sd[tid][0];
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
