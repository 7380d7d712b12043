// dxrl_study_summary.hip -- training runs reduced on the device (dxrl_study_summarize):
// compute_convergence_metrics / aggregate_metrics of evaluation/curriculum_ablation.py:137-203,
// 269-282 and the per-run summary / compute_ablation_statistics of
// evaluation/component_ablation.py:168-186,285-322, on the episode records dxrl_rollout_simple /
// dxrl_rollout_curriculum wrote.
//
// Two launches on the caller's stream, no host synchronisation between:
//   k_study_lanes   a wavefront per lane (= per training run); wave lane t holds episodes t, t + 64,
//                   ... so the [N][record_cap] rows load coalesced.  The success flags of 64
//                   episodes are one __ballot mask: the window test is a shift and a popcount over
//                   this chunk's mask and the previous one.  The returns are staged in LDS for the
//                   moving average (E * 8 bytes, at most E * w multiply-adds).  Every reduction is a
//                   fixed shuffle tree: bit-identical from run to run.
//   k_study_groups  a workgroup per group over the lane table and a CSR member list: integer sums,
//                   five Welford accumulators taken about the group's first member (push), merged
//                   with Chan et al.'s update (merge, both dxrl_moments.h) in a fixed LDS tree.
//                   One extra workgroup compacts the tie lanes into tie_list in ascending order
//                   (compact_rows, dxrl_reduce.h).
#include <climits>

#include "dxrl_moments.h"
#include "dxrl_reduce.h"

namespace dxrl {
namespace {

constexpr int kWave = 64;
constexpr int kGrpThreads = 128;
constexpr int kStageMaxCap = 8192;  // 64 KiB of LDS; longer rows are read from memory again
constexpr int kLI = DXRL_STUDY_LANE_INTS, kLR = DXRL_STUDY_LANE_REALS, kMetrics = DXRL_STUDY_METRICS;
constexpr int kGrpInts = 16;        // group_stats slots
constexpr int kGrpRed = kGrpInts + 2;  // + min / max of E (status bit 3)
enum : int { L_EPISODES, L_STEPS, L_SUCCESSES, L_FINAL_WINDOW, L_CONV, L_REWARD_CONV, L_LEVEL, L_FLAGS };
constexpr int kFlagTie = 1, kFlagSkipped = 2;

// butterfly reductions of integers (order-free, every lane ends with the result); in this file
// they stand in front of dxrl_reduce.h's lane-0 forms
__device__ __forceinline__ int wave_min(int v) {
    for (int s = kWave / 2; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s));
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
    for (int s = kWave / 2; s >= 1; s >>= 1) {
        const int lo = __shfl_xor((int)(unsigned)(v & 0xffffffffll), s), hi = __shfl_xor((int)(v >> 32), s);
        v += ((long long)hi << 32) | (long long)(unsigned)lo;
    }
    return v;
}

template <bool kStage>
__global__ __launch_bounds__(kWave) void k_study_lanes(
    int cap, int lane_offset, int w, int c_min, double thr, const double* __restrict__ ep_return,
    const int32_t* __restrict__ ep_length, const uint8_t* __restrict__ ep_success, const int32_t* __restrict__ ep_level,
    const int32_t* __restrict__ lane_episodes, int64_t* __restrict__ lane_ints, double* __restrict__ lane_reals,
    int32_t* __restrict__ status) {
    extern __shared__ double staged[];
    const int t = threadIdx.x;
    const int l = blockIdx.x;  // the grid is exactly the buffer's lanes; the rows were range-checked by the host
    const int E = lane_episodes[l];
    int64_t* li = lane_ints + (size_t)kLI * (size_t)(lane_offset + l);
    double* lr = lane_reals + (size_t)kLR * (size_t)(lane_offset + l);
    if (E <= 0 || E > cap) {  // the whole workgroup leaves together
        if (t < kLI) li[t] = t == L_FLAGS ? kFlagSkipped : (t == L_CONV || t == L_REWARD_CONV || t == L_LEVEL ? -1 : 0);
        if (t < kLR) lr[t] = 0.0;
        if (t == 0) atomicOr(status, 4);
        return;
    }
    const double* r = ep_return + (size_t)l * (size_t)cap;
    const int32_t* len = ep_length + (size_t)l * (size_t)cap;
    const uint8_t* ok = ep_success + (size_t)l * (size_t)cap;

    // pass 1: return moments about r[0], steps, successes, the success windows
    const double K = r[0];
    Moments mo{0.0, 0.0, 0.0};
    long long steps = 0;
    int succ = 0, conv = INT_MAX, fws = 0;
    unsigned long long prev = 0;
    const int chunks = E / kWave + 1;  // the chunk that holds episode index E is visited: its window is the final one
    for (int c = 0; c < chunks; ++c) {
        const int e = kWave * c + t;
        const bool in = e < E;
        int s = 0;
        if (in) {
            const double x = r[e];
            if (kStage) staged[e] = x;
            push(mo, x - K);
            steps += len[e];
            s = ok[e] != 0;
        }
        const unsigned long long cur = __ballot(s);
        succ += __popcll(cur);
        // the 64 episodes before e, episode e - 1 in bit 63
        const unsigned long long hist = t == 0 ? prev : (cur << (kWave - t)) | (prev >> t);
        const int cnt = __popcll(hist >> (kWave - w));
        if (in && e >= w && cnt >= c_min) conv = min(conv, e);
        if (e == E) fws = cnt;  // episodes before 0 are zero bits: also right for E < w
        prev = cur;
    }
    for (int s = kWave / 2; s >= 1; s >>= 1) {  // fixed tree; lane 0 ends with the merge of all 64
        const Moments o{__shfl_down(mo.n, s), __shfl_down(mo.mean, s), __shfl_down(mo.m2, s)};
        mo = merge(mo, o);
    }
    steps = wave_sum(steps);
    conv = wave_min(conv);
    fws = (int)wave_sum(fws);
    if (kStage) __syncthreads();
    const double* rr = kStage ? staged : r;

    // pass 2: the reward moving average, its first crossing and the first window within rounding of it
    int rconv = INT_MAX, rtie = INT_MAX;
    if (E >= w) {
        const double inv = 1.0 / (double)w;
        for (int i = t; i <= E - w; i += kWave) {
            double ma = 0.0, mx = 0.0;
            for (int j = 0; j < w; ++j) {
                const double p = rr[i + j] * inv;
                ma = ma + p;
                mx = fmax(mx, fabs(p));
            }
            const double band = (mx * (double)w) * 0x1p-46;  // 64 eps w max|r / w|
            if (fabs(ma - thr) <= band) rtie = min(rtie, i);
            if (ma >= thr) rconv = min(rconv, i);
        }
    } else {
        for (int i = t; i < E; i += kWave)
            if (rr[i] >= thr) rconv = min(rconv, i);
    }
    rconv = wave_min(rconv);
    rtie = wave_min(rtie);
    if (t != 0) return;
    const int k = E < w ? E : w;
    double fsum = 0.0;
    for (int e = E - k; e < E; ++e) fsum = fsum + rr[e];
    li[L_EPISODES] = E;
    li[L_STEPS] = steps;
    li[L_SUCCESSES] = succ;
    li[L_FINAL_WINDOW] = fws;
    li[L_CONV] = conv == INT_MAX ? -1 : conv;
    li[L_REWARD_CONV] = rconv == INT_MAX ? -1 : rconv + w - 1;
    li[L_LEVEL] = ep_level ? ep_level[(size_t)l * (size_t)cap + (size_t)(E - 1)] : -1;
    li[L_FLAGS] = rtie != INT_MAX && rtie <= rconv ? kFlagTie : 0;
    lr[0] = mo.n;
    lr[1] = K + mo.mean;
    lr[2] = mo.m2;
    lr[3] = fsum / (double)k;
}

// the five per-lane metrics of group_metrics; false in use[2] = an infinite coefficient of variation
__device__ __forceinline__ void lane_metrics(const double* lr, double v[kMetrics], bool& cv_finite) {
    const double var = lr[2] / lr[0], sd = sqrt(var), mean = lr[1];
    cv_finite = mean != 0.0;
    v[0] = var, v[1] = sd, v[2] = cv_finite ? sd / mean : 0.0, v[3] = lr[3], v[4] = mean;
}

__global__ __launch_bounds__(kGrpThreads) void k_study_groups(
    int L, int G, int num_members, const int32_t* __restrict__ group_offsets, const int32_t* __restrict__ group_lanes,
    const int64_t* __restrict__ lane_ints, const double* __restrict__ lane_reals, int64_t* __restrict__ group_stats,
    double* __restrict__ group_metrics, int32_t* __restrict__ tie_count, int32_t* __restrict__ tie_list, int tie_cap,
    int32_t* __restrict__ status) {
    __shared__ long long si[kGrpRed][kGrpThreads];
    __shared__ double sd[kMetrics * 3][kGrpThreads];
    __shared__ int scan[kGrpThreads];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x == G) {
        // tie lanes in ascending row order
        compact_rows<kGrpThreads>(L, [=](int l) { return (lane_ints[(size_t)kLI * l + L_FLAGS] & kFlagTie) != 0; },
                                  scan, tie_count, tie_list, tie_cap, status);
        return;
    }
    const int g = blockIdx.x;
    const int lo = group_offsets[g], hi = group_offsets[g + 1];
    long long acc[kGrpRed];
#pragma unroll
    for (int k = 0; k < kGrpRed; ++k) acc[k] = 0;
    acc[6] = LLONG_MAX, acc[7] = LLONG_MIN;              // min / max of final_window_successes
    acc[kGrpInts] = LLONG_MAX, acc[kGrpInts + 1] = LLONG_MIN;  // min / max of E
    Moments mo[kMetrics];
#pragma unroll
    for (int k = 0; k < kMetrics; ++k) mo[k] = Moments{0.0, 0.0, 0.0};
    bool bad = lo < 0 || hi < lo || hi > num_members;
    // the moments are taken about the group's first member's values (zero where it has none)
    double K[kMetrics] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (!bad && lo < hi) {
        const int l0 = group_lanes[lo];
        if (l0 >= 0 && l0 < L && lane_ints[(size_t)kLI * l0 + L_EPISODES] > 0) {  // not a skipped lane
            bool fin;
            lane_metrics(lane_reals + (size_t)kLR * l0, K, fin);
        }
    }
    if (!bad) {
        for (long long m = (long long)lo + tid; m < hi; m += kGrpThreads) {
            const int l = group_lanes[m];
            if (l < 0 || l >= L) {
                bad = true;
                continue;
            }
            const int64_t* li = lane_ints + (size_t)kLI * l;
            if (li[L_EPISODES] <= 0) continue;  // a skipped lane (or a row no lane pass wrote, zeroed by the caller)
            const long long E = li[L_EPISODES], st = li[L_STEPS], fw = li[L_FINAL_WINDOW], cv = li[L_CONV],
                            rc = li[L_REWARD_CONV];
            acc[0] += 1;
            acc[1] += E;
            acc[2] += st;
            acc[3] += st * st;
            acc[4] += fw;
            acc[5] += fw * fw;
            acc[6] = fw < acc[6] ? fw : acc[6];
            acc[7] = fw > acc[7] ? fw : acc[7];
            if (cv >= 0) acc[8] += 1, acc[9] += cv, acc[10] += cv * cv;
            if (rc >= 0) acc[11] += 1, acc[12] += rc, acc[13] += rc * rc;
            acc[14] += (li[L_FLAGS] & kFlagTie) != 0;
            acc[15] += li[L_SUCCESSES];
            acc[kGrpInts] = E < acc[kGrpInts] ? E : acc[kGrpInts];
            acc[kGrpInts + 1] = E > acc[kGrpInts + 1] ? E : acc[kGrpInts + 1];
            double v[kMetrics];
            bool fin;
            lane_metrics(lane_reals + (size_t)kLR * l, v, fin);
#pragma unroll
            for (int k = 0; k < kMetrics; ++k)
                if (k != 2 || fin) push(mo[k], v[k] - K[k]);
        }
    }
    if (bad) atomicOr(status, 1);
#pragma unroll
    for (int k = 0; k < kGrpRed; ++k) si[k][tid] = acc[k];
#pragma unroll
    for (int k = 0; k < kMetrics; ++k) sd[3 * k][tid] = mo[k].n, sd[3 * k + 1][tid] = mo[k].mean, sd[3 * k + 2][tid] = mo[k].m2;
    __syncthreads();
    for (int s = kGrpThreads / 2; s >= 1; s >>= 1) {  // fixed tree
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < kGrpRed; ++k) {
                const long long a = si[k][tid], b = si[k][tid + s];
                const bool mn = k == 6 || k == kGrpInts, mx = k == 7 || k == kGrpInts + 1;
                si[k][tid] = mn ? (b < a ? b : a) : mx ? (b > a ? b : a) : a + b;
            }
#pragma unroll
            for (int k = 0; k < kMetrics; ++k) {
                const Moments r = merge(Moments{sd[3 * k][tid], sd[3 * k + 1][tid], sd[3 * k + 2][tid]},
                                        Moments{sd[3 * k][tid + s], sd[3 * k + 1][tid + s], sd[3 * k + 2][tid + s]});
                sd[3 * k][tid] = r.n, sd[3 * k + 1][tid] = r.mean, sd[3 * k + 2][tid] = r.m2;
            }
        }
        __syncthreads();
    }
    const bool any = si[0][0] > 0;
    if (tid < kGrpInts) group_stats[(size_t)kGrpInts * g + tid] = (tid == 6 || tid == 7) && !any ? 0 : si[tid][0];
    if (tid < kMetrics * 3) {
        const int k = tid / 3, c = tid % 3;
        group_metrics[(size_t)kMetrics * 3 * g + tid] = c == 1 && sd[3 * k][0] > 0.0 ? K[k] + sd[tid][0] : sd[tid][0];
    }
    if (tid == 0 && any && si[kGrpInts][0] != si[kGrpInts + 1][0]) atomicOr(status, 8);
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_study_summarize(int32_t device, const dxrl_study_summary_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_study_summary_args& a = *args;
    DXRL_REQUIRE(a.window >= 1 && a.window <= 64, "window must be in [1, 64] (the success window is a 64-bit mask), got %d",
                 a.window);
    DXRL_REQUIRE(a.record_cap > 0, "record_cap must be > 0, got %d", a.record_cap);
    DXRL_REQUIRE(a.num_lanes >= 0 && a.total_lanes >= 0 && a.num_groups >= 0 && a.num_members >= 0,
                 "num_lanes, total_lanes, num_groups and num_members must be >= 0");
    DXRL_REQUIRE(a.lane_offset >= 0 && (int64_t)a.lane_offset + a.num_lanes <= (int64_t)a.total_lanes,
                 "rows lane_offset .. lane_offset + num_lanes (%d + %d) lie outside the lane table (%d rows)",
                 a.lane_offset, a.num_lanes, a.total_lanes);
    DXRL_REQUIRE(a.lane_ints && a.lane_reals && a.status, "null lane_ints / lane_reals / status");
    DXRL_REQUIRE(a.num_lanes == 0 || (a.ep_return && a.ep_length && a.ep_success && a.lane_episodes),
                 "null episode record buffers / lane_episodes");
    const bool groups = a.group_stats != nullptr;
    if (groups) {
        DXRL_REQUIRE(a.group_metrics && a.tie_count, "null group_metrics / tie_count");
        DXRL_REQUIRE(a.group_offsets && (a.group_lanes || a.num_members == 0), "null group table");
        DXRL_REQUIRE(a.tie_cap >= 0 && (a.tie_list || a.tie_cap == 0), "null tie_list with tie_cap > 0");
    }
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (int rc = hip_check(hipMemsetAsync(a.status, 0, sizeof(int32_t), st), "memset status")) return rc;
    if (a.num_lanes > 0) {
        if (a.record_cap <= kStageMaxCap) {
            hipLaunchKernelGGL(k_study_lanes<true>, dim3(a.num_lanes), dim3(kWave), sizeof(double) * (size_t)a.record_cap,
                               st, a.record_cap, a.lane_offset, a.window, a.min_count, a.reward_threshold, a.ep_return,
                               a.ep_length, a.ep_success, a.ep_level, a.lane_episodes, a.lane_ints, a.lane_reals,
                               a.status);
        } else {
            hipLaunchKernelGGL(k_study_lanes<false>, dim3(a.num_lanes), dim3(kWave), 0, st, a.record_cap, a.lane_offset,
                               a.window, a.min_count, a.reward_threshold, a.ep_return, a.ep_length, a.ep_success,
                               a.ep_level, a.lane_episodes, a.lane_ints, a.lane_reals, a.status);
        }
        if (int rc = launch_check("k_study_lanes")) return rc;
    }
    if (!groups) return DXRL_OK;
    hipLaunchKernelGGL(k_study_groups, dim3(a.num_groups + 1), dim3(kGrpThreads), 0, st, a.total_lanes, a.num_groups,
                       a.num_members, a.group_offsets, a.group_lanes, a.lane_ints, a.lane_reals, a.group_stats,
                       a.group_metrics, a.tie_count, a.tie_list, a.tie_cap, a.status);
    return launch_check("k_study_groups");
}
