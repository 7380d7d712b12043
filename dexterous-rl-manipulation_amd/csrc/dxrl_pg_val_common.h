// dxrl_pg_val_common.h -- the record reduction of a validation row, shared by dxrl_pg_val.hip (one
// set of G x K records) and dxrl_pg_val_levels.hip (L such sets, one per noise level): the body
// of the reduce workgroup, the per-set part of the finishing wave, the columns both rows share,
// and the keep-best / patience rules of the header.  Both translation units run the same code on
// a set of records, so a level's statistics are the single-set kernel's bit for bit.  merge and
// wave_moments are dxrl_moments.h's; wave_sum, wave_min, quiet_nan and aligned16 dxrl_reduce.h's;
// the conditional parameter copy (launch_keep_best) dxrl_keep_best.h's.  A record enters the
// moments by merge(m, {1, x, 0}), not by push: the two round differently, and this form is the
// contract here.  dxrl_pg_val_paired.hip takes the chunking constants, val_grid and the scratch
// size from here: its pairs are reduced in the chunks and the order of the records.
#pragma once
#include "dxrl_keep_best.h"
#include "dxrl_moments.h"

#include <climits>

namespace dxrl {
namespace {

constexpr int kValThreads = 256;   // reduce workgroup (4 waves)
constexpr int kWave = 64;
constexpr int kValWaves = kValThreads / kWave;
constexpr int kValPerThread = 4;   // consecutive records per thread and pass
constexpr int kValChunk = kValThreads * kValPerThread;
constexpr int kValMaxBlocks = 64;  // one partial per lane of the finishing wave
constexpr int kValPartial = 8;     // doubles per workgroup partial
enum { V_N, V_MEAN, V_M2, V_LEN, V_SUC, V_SLEN, V_CON, V_PAD };
static_assert(V_PAD + 1 == kValPartial, "partial layout");
static_assert(kValMaxBlocks <= kWave, "the finish reads one partial per lane");

inline int64_t val_grid(int64_t G, int64_t K) {
    const int64_t chunks = (G * K + kValChunk - 1) / kValChunk;
    const int64_t by_objects = (G + kValWaves - 1) / kValWaves;
    const int64_t b = chunks > by_objects ? chunks : by_objects;
    return b < 1 ? 1 : b > kValMaxBlocks ? kValMaxBlocks : b;
}
// scratch of one set of records: the workgroup partials, then G i32 object counts
inline int64_t val_partial_doubles(int64_t G) { return (int64_t)kValMaxBlocks * kValPartial + (G + 1) / 2; }

// One reduce workgroup (block `block` of `blocks`, kValThreads threads) over the E = G K records
// behind the four pointers: its partial into partial[block], the success counts of its objects
// into counts.  `wred` is the workgroup's LDS.
template <bool VEC>
__device__ __forceinline__ void val_reduce_block(const double* __restrict__ ep_return,
                                                 const int32_t* __restrict__ ep_length,
                                                 const uint8_t* __restrict__ ep_success,
                                                 const uint8_t* __restrict__ ep_contacts, int64_t E, int64_t G,
                                                 int64_t K, int64_t block, int64_t blocks,
                                                 double* __restrict__ partial, int32_t* __restrict__ counts,
                                                 double (*wred)[kValPartial]) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const double K0 = ep_return[0];  // E >= 1
    Moments m{0.0, 0.0, 0.0};
    long long s_len = 0, s_suc = 0, s_slen = 0, s_con = 0;
    for (int64_t base = block * kValChunk; base < E; base += blocks * kValChunk) {
        const int64_t i0 = base + (int64_t)threadIdx.x * kValPerThread;
        if (i0 >= E) continue;
        const int cnt = E - i0 >= kValPerThread ? kValPerThread : (int)(E - i0);
        double r[kValPerThread];
        int32_t l[kValPerThread];
        uint8_t s[kValPerThread], c[kValPerThread];
        if (VEC && cnt == kValPerThread) {
            const double2 r0 = *reinterpret_cast<const double2*>(ep_return + i0);
            const double2 r1 = *reinterpret_cast<const double2*>(ep_return + i0 + 2);
            const int4 lv = *reinterpret_cast<const int4*>(ep_length + i0);
            const uint32_t sv = *reinterpret_cast<const uint32_t*>(ep_success + i0);
            const uint32_t cv = *reinterpret_cast<const uint32_t*>(ep_contacts + i0);
            r[0] = r0.x, r[1] = r0.y, r[2] = r1.x, r[3] = r1.y;
            l[0] = lv.x, l[1] = lv.y, l[2] = lv.z, l[3] = lv.w;
#pragma unroll
            for (int k = 0; k < kValPerThread; ++k) s[k] = (uint8_t)(sv >> (8 * k)), c[k] = (uint8_t)(cv >> (8 * k));
        } else {
#pragma unroll
            for (int k = 0; k < kValPerThread; ++k) {  // clamped: every slot loads an in-range record
                const int64_t i = i0 + (k < cnt ? k : cnt - 1);
                r[k] = ep_return[i], l[k] = ep_length[i], s[k] = ep_success[i], c[k] = ep_contacts[i];
            }
        }
#pragma unroll
        for (int k = 0; k < kValPerThread; ++k) {
            if (k < cnt) {
                m = merge(m, Moments{1.0, r[k] - K0, 0.0});
                s_len += l[k];
                s_con += c[k];
                if (s[k] != 0) s_suc += 1, s_slen += l[k];
            }
        }
    }
    // the integer sums are below 2^53: exact as doubles in any order
    m = wave_moments(m);
    double acc[4] = {(double)s_len, (double)s_suc, (double)s_slen, (double)s_con};
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
        wred[wave][V_N] = m.n, wred[wave][V_MEAN] = m.mean, wred[wave][V_M2] = m.m2;
#pragma unroll
        for (int k = 0; k < 4; ++k) wred[wave][V_LEN + k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Moments t{wred[0][V_N], wred[0][V_MEAN], wred[0][V_M2]};
        double tot[4] = {wred[0][V_LEN], wred[0][V_SUC], wred[0][V_SLEN], wred[0][V_CON]};
        for (int w = 1; w < kValWaves; ++w) {
            t = merge(t, Moments{wred[w][V_N], wred[w][V_MEAN], wred[w][V_M2]});
#pragma unroll
            for (int k = 0; k < 4; ++k) tot[k] += wred[w][V_LEN + k];
        }
        double* p = partial + block * kValPartial;
        p[V_N] = t.n, p[V_MEAN] = t.mean, p[V_M2] = t.m2;
        p[V_LEN] = tot[0], p[V_SUC] = tot[1], p[V_SLEN] = tot[2], p[V_CON] = tot[3], p[V_PAD] = 0.0;
    }
    // successes of whole objects, one object per wave at a time
    const int64_t waves = blocks * kValWaves;
    for (int64_t o = block * kValWaves + wave; o < G; o += waves) {
        int n = 0;
        for (int64_t k = lane; k < K; k += kWave) n += ep_success[o * K + k] != 0;
        n = wave_sum(n);
        if (lane == 0) counts[o] = n;
    }
}

// What one finishing wave knows of a set of records (valid in lane 0).
struct ValSetStats {
    Moments m;
    double s_len, s_suc, s_slen, s_con;
    int worst, solved;
};

// One wave (`lane` of 64) over the scratch of one set: merges the `blocks` partials in index
// order, takes the minimum and the solved count over the G object counts, and writes the counts
// to object_row when it is given.
__device__ __forceinline__ ValSetStats val_finish_set(const double* __restrict__ partial, int blocks, int64_t G,
                                                      int64_t K, double solve_threshold,
                                                      int32_t* __restrict__ object_row, int lane) {
    // one workgroup partial per lane (blocks <= 64), then the fixed wave order
    Moments m{0.0, 0.0, 0.0};
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < blocks) {
        const double* p = partial + (int64_t)lane * kValPartial;
        m = Moments{p[V_N], p[V_MEAN], p[V_M2]};
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = p[V_LEN + k];
    }
    m = wave_moments(m);
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
    // the objects: worst success count, solved count, and the optional per-object row
    const int32_t* counts = reinterpret_cast<const int32_t*>(partial + (int64_t)kValMaxBlocks * kValPartial);
    int worst = INT_MAX, solved = 0;
    for (int64_t o = lane; o < G; o += kWave) {
        const int c = counts[o];
        worst = c < worst ? c : worst;
        solved += (double)c / (double)K >= solve_threshold;
        if (object_row) object_row[o] = c;
    }
    worst = wave_min(worst);
    solved = wave_sum(solved);
    return ValSetStats{m, s[0], s[1], s[2], s[3], worst, solved};
}

// The statistic columns of a set in the main row's layout (out[DXRL_PG_VAL_COLS], every other
// column 0); first_return is the set's first ep_return, the shift of its moments.
__device__ __forceinline__ void val_set_columns(double* out, const ValSetStats& t, int64_t G, int64_t K,
                                                double first_return) {
    const double E = (double)(G * K);
    for (int k = 0; k < DXRL_PG_VAL_COLS; ++k) out[k] = 0.0;
    out[DXRL_PG_VAL_EPISODES] = E;
    out[DXRL_PG_VAL_SUCCESSES] = t.s_suc;
    out[DXRL_PG_VAL_SUCCESS_RATE] = t.s_suc / E;
    out[DXRL_PG_VAL_MEAN_RETURN] = first_return + t.m.mean;
    out[DXRL_PG_VAL_RETURN_STD] = sqrt(t.m.m2 / t.m.n);
    out[DXRL_PG_VAL_MEAN_LENGTH] = t.s_len / E;
    out[DXRL_PG_VAL_MEAN_SUCCESS_LENGTH] = t.s_suc > 0.0 ? t.s_slen / t.s_suc : quiet_nan();
    out[DXRL_PG_VAL_MEAN_CONTACTS] = t.s_con / E;
    out[DXRL_PG_VAL_MIN_OBJECT_SUCCESS_RATE] = (double)t.worst / (double)K;
    out[DXRL_PG_VAL_OBJECTS_SOLVED] = (double)t.solved;
}

// Keep-best and patience on the header for row `row` with `score` (has_score false: keep-best
// off); fills is_best / since_best of out.  Strict >: the first maximum wins, a NaN is never best.
__device__ __forceinline__ void val_header_rules(dxrl_pg_val_header* h, double* out, int64_t row, bool has_score,
                                                 double score, int32_t status, double min_delta, int32_t patience) {
    bool best = false;
    if (has_score) {
        if (status == 0 && score > h->best_score + min_delta) {
            best = true;
            h->best_score = score;
            h->best_row = row;
        }
    }
    const int64_t since = best ? 0 : h->since_best + 1;
    out[DXRL_PG_VAL_IS_BEST] = best ? 1.0 : 0.0;
    out[DXRL_PG_VAL_SINCE_BEST] = (double)since;
    h->since_best = since;
    if (patience > 0 && h->stopped_row < 0 && since >= (int64_t)patience) h->stopped_row = row;
    h->rows_written = row + 1;
}

}  // namespace
}  // namespace dxrl
