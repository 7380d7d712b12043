// dxrl_metrics_groups.h -- the one statement of the failure rules of evaluation/metrics.py:39-103
// and of the group aggregates of metrics.py:128-206, shared by dxrl_eval_summary.hip (rules per
// episode in a pre-pass, a code byte per member in the group pass) and dxrl_robustness_summary.hip
// (rules inline in the group pass, on the history words).  Both run the same group pass, so their
// group_stats and group_return agree bit for bit on the same records.
#pragma once
#include "dxrl_moments.h"
#include "dxrl_reduce.h"

namespace dxrl {

constexpr int kGroupThreads = 256;  // workgroup of the group pass
constexpr int kBatch = 4;           // group members gathered per trip of the group pass
constexpr int kIntStats = 14;       // group_stats slots 0..13 (14, 15 stay zero)
constexpr int kTieBit = 0x80;       // code word: low bits code + 1, bit 7 the tie flag

// metrics.FailureType order (code k <-> list(FailureType)[k])
enum : int { F_SLIPPAGE = 0, F_UNSTABLE = 1, F_MISALIGNED = 2, F_TIMEOUT = 3, F_DROPPED = 4, F_INSUFFICIENT = 5 };

// The rules on (length, success, final contacts) and the history's S1, S2, first-five and
// last-five sums; returns (code + 1) | tie flag, 0 for a success.  `len` is the recorded length,
// not the number of history bytes that were read.  A tie row (n S2 - S1^2 == 2 n^2) is classified
// as the exact comparison decides (not unstable) and flagged; an unstable row is never a tie.
__device__ __forceinline__ int failure_word(int len, int ok, int nc, int s1, int s2, int f5, int l5, int max_steps,
                                            int success_threshold) {
    if (ok) return 0;
    if (len >= max_steps) return F_TIMEOUT + 1;  // :63-65
    if (nc == 0) return F_DROPPED + 1;           // :67-69
    // :72-83, only when the history has more than 5 entries.  np.var(counts) > 2.0 decided exactly:
    // n S2 - S1^2 > 2 n^2 (n <= 4096, counts u8: below 2^41)
    const long long nn = len;
    const long long num = nn * (long long)s2 - (long long)s1 * (long long)s1;
    const long long lim = 2 * nn * nn;
    const int tie = len > 5 && num == lim ? kTieBit : 0;  // np.var's own rounding would decide
    const double trend = ((double)l5 / 5.0) - ((double)f5 / 5.0);  // the reference's f64 expression
    if (len > 5 && num > lim) return F_UNSTABLE + 1;
    if (len > 10 && trend < -1.0) return (F_SLIPPAGE + 1) | tie;
    if (nc > 0 && nc < success_threshold) return (F_MISALIGNED + 1) | tie;  // :86-87
    return (F_INSUFFICIENT + 1) | tie;                                       // :90-95
}

// How a group member's code word is obtained: Raw load(e) is issued with the member's other
// gathers, word(raw, len, ok, nc) is evaluated when the member is accumulated.
struct CodeByte {  // the byte the episode pre-pass left in ep_work
    const uint8_t* __restrict__ ep_work;
    using Raw = int;
    __device__ __forceinline__ Raw load(int e) const { return ep_work[e]; }
    __device__ __forceinline__ int word(Raw w, int, int, int) const { return w; }
};
struct HistWords {  // the rules on the first four of the episode's five hist_moments words
    const int32_t* __restrict__ moments;
    int max_steps, success_threshold;
    struct Raw {
        int m[4];
    };
    __device__ __forceinline__ Raw load(int e) const {
        Raw r;
#pragma unroll
        for (int q = 0; q < 4; ++q) r.m[q] = moments[5 * (size_t)e + q];
        return r;
    }
    __device__ __forceinline__ int word(const Raw& r, int len, int ok, int nc) const {
        return failure_word(len, ok, nc, r.m[0], r.m[1], r.m[2], r.m[3], max_steps, success_threshold);
    }
    __device__ __forceinline__ int word(int e, const int32_t* __restrict__ ep_length,
                                        const uint8_t* __restrict__ ep_success,
                                        const uint8_t* __restrict__ ep_contacts) const {
        return word(load(e), ep_length[e], ep_success[e] != 0, ep_contacts[e]);
    }
};

// Group g of the CSR table by one workgroup of kGroupThreads: strided accumulation over the member
// list (about 32 B per member plus the code source's), then a fixed tree in si / sd.  The return
// moments are taken about K, the group's first member's return (with returns of the form
// -1e6 + small, a running mean held as an absolute f64 rounds at 1e-10 and costs M2 ~1e-8
// relative; about K it does not), by a Welford step per member, and merge with Chan et al.'s
// update in the tree's fixed order: group_return is bit-identical from run to run (no
// floating-point atomics).  A bad offset or member sets status bit 0 and is skipped.
template <class Code>
__device__ __forceinline__ void metrics_group_pass(
    int g, int E, int num_members, const int32_t* __restrict__ group_offsets,
    const int32_t* __restrict__ group_episodes, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts,
    const double* __restrict__ ep_return, const Code code_of, int64_t* __restrict__ group_stats,
    double* __restrict__ group_return, int32_t* __restrict__ status, long long (*si)[kGroupThreads],
    double (*sd)[kGroupThreads]) {
    const int tid = threadIdx.x;
    const int lo = group_offsets[g], hi = group_offsets[g + 1];
    long long acc[kIntStats];
#pragma unroll
    for (int k = 0; k < kIntStats; ++k) acc[k] = 0;
    Moments mo{0.0, 0.0, 0.0};
    bool bad = lo < 0 || hi < lo || hi > num_members;
    double K = 0.0;
    if (!bad && lo < hi) {
        const int e0 = group_episodes[lo];
        if (e0 >= 0 && e0 < E) K = ep_return[e0];
    }
    if (!bad) {
        // kBatch members per trip: their gathers go out together (one memory latency per trip, a big
        // group is a chain of trips on one workgroup), then they are accumulated in member order
        for (long long m0 = lo + tid; m0 < hi; m0 += kGroupThreads * kBatch) {
            int ee[kBatch], len_[kBatch], nc_[kBatch], ok_[kBatch];
            typename Code::Raw raw_[kBatch];
            double x_[kBatch];
            bool use[kBatch];
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                const long long m = m0 + b * kGroupThreads;
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
                raw_[b] = use[b] ? code_of.load(e) : typename Code::Raw{};
                x_[b] = use[b] ? ep_return[e] : 0.0;
            }
#pragma unroll
            for (int b = 0; b < kBatch; ++b) {
                if (!use[b]) continue;
                const long long len = len_[b], nc = nc_[b];
                const int ok = ok_[b], w = code_of.word(raw_[b], len_[b], ok, nc_[b]), code = (w & 0x7f) - 1;
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
                push(mo, x_[b] - K);
            }
        }
    }
    if (bad) atomicOr(status, 1);
#pragma unroll
    for (int k = 0; k < kIntStats; ++k) si[k][tid] = acc[k];
    sd[0][tid] = mo.n, sd[1][tid] = mo.mean, sd[2][tid] = mo.m2;
    __syncthreads();
    for (int s = kGroupThreads / 2; s >= 1; s >>= 1) {  // fixed tree
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

}  // namespace dxrl
