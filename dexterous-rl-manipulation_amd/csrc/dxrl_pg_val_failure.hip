// dxrl_pg_val_failure.hip -- the failure-mode tables of a validation row (include/dxrl.h,
// dxrl_pg_val_failure_row).  Every episode of the level-major records is classified with the
// taxonomy of dxrl_failure_rules.h on the five history words the episode kernel accumulated (the
// moments form of dxrl_failure_summarize: n = ep_length clamped to [0, max_steps], tie rows as the
// exact comparison decides), and per level the per-mode sums, the per-object counts and -- with
// common random numbers -- the class transitions against the baseline are reduced into one row of
// three tables.  The header, the tables of the other rows and keep-best are left alone.
//
// Two launches behind the other rows of the validation, whatever L is:
//   k_pg_val_failure_reduce  a (val_grid(G, K), L) grid: blockIdx.y is the level.  The chunks and
//                            the four consecutive records of a thread are val_reduce_block's
//                            (dxrl_pg_val_common.h); the 16-byte loads are taken where every slice
//                            is aligned, the scalar loads otherwise, in the same record order.  A
//                            thread keeps the six modes' sums in named registers (selects, no
//                            indexed array), the wave sums are wave_sum's, the four waves are
//                            added in index order.  The 7 x 7 class pairs are counted with integer
//                            adds in LDS; the per-object mode counts one object per wave.
//   k_pg_val_failure_finish  one workgroup, one wave per level: the wave adds its level's
//                            partials in index order (a column per lane), scans the object
//                            counts (wave_sum / wave_max / wave_min), lanes 0 .. 5 form the columns of
//                            a mode each and lane 0 the level's row in LDS, and after a barrier
//                            the workgroup writes the L rows.
// Every sum but the confidence's is an integer below 2^53 and exact as a double in any order; the
// confidence sum has the fixed order above.  No floating-point atomics, no tickets, no
// spin-waits: the launch order is the only ordering, and the same inputs give the same bytes.
#include "dxrl_failure_rules.h"
#include "dxrl_pg_val_common.h"

namespace dxrl {
namespace {

constexpr int kMaxLevels = DXRL_PG_VAL_MAX_LEVELS;
constexpr int kModes = DXRL_FAILURE_MODES;
constexpr int kClasses = kModes + 1;  // 0 success, 1 + m mode m
constexpr int kPairs = kClasses * kClasses;
constexpr int kModeCols = DXRL_PG_VAL_FAILURE_MODE_COLS, kLevelCols = DXRL_PG_VAL_FAILURE_LEVEL_COLS;
constexpr int64_t kMaxRecords = DXRL_PG_VAL_FAILURE_MAX_EPISODES;  // c S2 < 2^62 in the finish
static_assert(kMaxLevels * kWave <= 1024, "one wave per level in one workgroup");
static_assert(DXRL_PG_VAL_FAILURE_MODE_NAMED == kModeCols && DXRL_PG_VAL_FAILURE_LEVEL_NAMED == kLevelCols,
              "column enums");
// a workgroup partial: per mode count, sum len, sum len^2, sum contacts, sum confidence; the ties
enum { F_COUNT, F_S1, F_S2, F_C1, F_CONF, F_PER_MODE };
constexpr int kFvTies = kModes * F_PER_MODE, kFvPartial = 32;
static_assert(kFvTies < kFvPartial, "partial layout");
constexpr int kFvPairInts = 50;  // the 49 class pairs of a workgroup, padded to whole doubles
static_assert(kPairs <= kFvPairInts && kFvPairInts % 2 == 0, "pair layout");
// scratch of one level, in doubles: the partials, the class pairs, then G x 6 i32 object counts
constexpr int64_t kFvPairsAt = (int64_t)kValMaxBlocks * kFvPartial;
constexpr int64_t kFvCountsAt = kFvPairsAt + (int64_t)kValMaxBlocks * kFvPairInts / 2;
inline int64_t failure_partial_doubles(int64_t G) { return kFvCountsAt + 3 * G; }

struct Records {
    const int32_t* len;
    const uint8_t* suc;
    const uint8_t* con;
    const int32_t* mom;  // [.][5]
};
__device__ __forceinline__ Records slice(const Records& r, int64_t first) {
    return Records{r.len + first, r.suc + first, r.con + first, r.mom + 5 * first};
}
__device__ __forceinline__ bool records_aligned16(const Records& r) {
    return aligned16(r.len) && aligned16(r.suc) && aligned16(r.con) && aligned16(r.mom);
}

struct Rules {
    int max_steps, timeout_steps, success_threshold;
};

__device__ __forceinline__ Verdict classify_record(const Rules& q, int len, int suc, int nc, const int32_t* m) {
    const int n = len < 0 ? 0 : (len > q.max_steps ? q.max_steps : len);
    return classify(suc != 0, len, n, m[0], m[1], m[2], m[3], m[4], nc, q.timeout_steps, q.success_threshold);
}

// the kValPerThread records from i0 on (cnt of them in range; the others repeat the last one)
struct Quad {
    int32_t len[kValPerThread];
    uint8_t suc[kValPerThread], con[kValPerThread];
    int32_t mom[kValPerThread * 5];
};
template <bool VEC>
__device__ __forceinline__ Quad load_quad(const Records& r, int64_t i0, int cnt) {
    Quad q;
    if (VEC && cnt == kValPerThread) {
        const int4 lv = *reinterpret_cast<const int4*>(r.len + i0);
        const uint32_t sv = *reinterpret_cast<const uint32_t*>(r.suc + i0);
        const uint32_t cv = *reinterpret_cast<const uint32_t*>(r.con + i0);
        q.len[0] = lv.x, q.len[1] = lv.y, q.len[2] = lv.z, q.len[3] = lv.w;
#pragma unroll
        for (int k = 0; k < kValPerThread; ++k) q.suc[k] = (uint8_t)(sv >> (8 * k)), q.con[k] = (uint8_t)(cv >> (8 * k));
        const int4* mv = reinterpret_cast<const int4*>(r.mom + 5 * i0);  // 80 bytes per quad
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int4 v = mv[k];
            q.mom[4 * k] = v.x, q.mom[4 * k + 1] = v.y, q.mom[4 * k + 2] = v.z, q.mom[4 * k + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kValPerThread; ++k) {  // clamped: every slot loads an in-range record
            const int64_t i = i0 + (k < cnt ? k : cnt - 1);
            q.len[k] = r.len[i], q.suc[k] = r.suc[i], q.con[k] = r.con[i];
#pragma unroll
            for (int j = 0; j < 5; ++j) q.mom[5 * k + j] = r.mom[5 * i + j];
        }
    }
    return q;
}

// One reduce workgroup over the E records of a level (`lv`; `base` the baseline's, read when
// PAIRED): its partial into partial[block], its class pairs into pairs[block], the mode counts of
// its objects into counts.
template <bool VEC, bool PAIRED>
__device__ __forceinline__ void failure_reduce_block(const Records& lv, const Records& base, const Rules& q,
                                                     int64_t E, int64_t G, int64_t K, int64_t block, int64_t blocks,
                                                     double* __restrict__ partial, int32_t* __restrict__ pairs,
                                                     int32_t* __restrict__ counts, double (*wred)[kFvPartial],
                                                     int* hist) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (PAIRED) {
        if (threadIdx.x < kPairs) hist[threadIdx.x] = 0;
        __syncthreads();
    }
    long long cnt_m[kModes], s1_m[kModes], s2_m[kModes], c1_m[kModes];
    double conf_m[kModes];
#pragma unroll
    for (int m = 0; m < kModes; ++m) cnt_m[m] = s1_m[m] = s2_m[m] = c1_m[m] = 0, conf_m[m] = 0.0;
    long long ties = 0;
    for (int64_t at = block * kValChunk; at < E; at += blocks * kValChunk) {
        const int64_t i0 = at + (int64_t)threadIdx.x * kValPerThread;
        if (i0 >= E) continue;
        const int cnt = E - i0 >= kValPerThread ? kValPerThread : (int)(E - i0);
        const Quad r = load_quad<VEC>(lv, i0, cnt);
        Quad b;
        if (PAIRED) b = load_quad<VEC>(base, i0, cnt);
#pragma unroll
        for (int k = 0; k < kValPerThread; ++k) {
            if (k < cnt) {
                const Verdict v = classify_record(q, r.len[k], r.suc[k], r.con[k], r.mom + 5 * k);
                const long long len = r.len[k], nc = r.con[k];
#pragma unroll
                for (int m = 0; m < kModes; ++m) {  // selects on named registers: no indexed array
                    const bool is = v.mode == m;
                    cnt_m[m] += is;
                    s1_m[m] += is ? len : 0;
                    s2_m[m] += is ? len * len : 0;
                    c1_m[m] += is ? nc : 0;
                    conf_m[m] += is ? v.conf : 0.0;
                }
                ties += v.tie != 0;
                if (PAIRED) {
                    const Verdict v0 = classify_record(q, b.len[k], b.suc[k], b.con[k], b.mom + 5 * k);
                    atomicAdd(&hist[(v0.mode + 1) * kClasses + (v.mode + 1)], 1);  // integers: any order
                }
            }
        }
    }
    // the integer sums are below 2^53: exact as doubles in any order
#pragma unroll
    for (int m = 0; m < kModes; ++m) {
        const double c = wave_sum((double)cnt_m[m]), s1 = wave_sum((double)s1_m[m]), s2 = wave_sum((double)s2_m[m]);
        const double c1 = wave_sum((double)c1_m[m]), cf = wave_sum(conf_m[m]);
        if (lane == 0) {
            double* w = wred[wave] + m * F_PER_MODE;
            w[F_COUNT] = c, w[F_S1] = s1, w[F_S2] = s2, w[F_C1] = c1, w[F_CONF] = cf;
        }
    }
    const double t = wave_sum((double)ties);
    if (lane == 0) {
        wred[wave][kFvTies] = t;
        wred[wave][kFvTies + 1] = 0.0;
    }
    __syncthreads();  // also: every class pair of the workgroup is in hist
    if (threadIdx.x < kFvPartial) {  // the waves in index order, a column per thread
        double v = wred[0][threadIdx.x];
        for (int w = 1; w < kValWaves; ++w) v += wred[w][threadIdx.x];
        partial[block * kFvPartial + threadIdx.x] = v;
    }
    if (PAIRED && threadIdx.x < kPairs) pairs[block * kFvPairInts + threadIdx.x] = hist[threadIdx.x];
    // mode counts of whole objects, one object per wave at a time
    const int64_t waves = blocks * kValWaves;
    for (int64_t o = block * kValWaves + wave; o < G; o += waves) {
        int n[kModes];
#pragma unroll
        for (int m = 0; m < kModes; ++m) n[m] = 0;
        for (int64_t k = lane; k < K; k += kWave) {
            const int64_t e = o * K + k;
            int32_t mom[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) mom[j] = lv.mom[5 * e + j];
            const Verdict v = classify_record(q, lv.len[e], lv.suc[e], lv.con[e], mom);
#pragma unroll
            for (int m = 0; m < kModes; ++m) n[m] += v.mode == m;
        }
#pragma unroll
        for (int m = 0; m < kModes; ++m) {
            const int c = wave_sum(n[m]);
            if (lane == 0) counts[o * kModes + m] = c;
        }
    }
}

template <bool PAIRED>
__global__ __launch_bounds__(kValThreads) void k_pg_val_failure_reduce(const Records all, const Rules q, int64_t G,
                                                                       int64_t K, double* __restrict__ partial,
                                                                       int64_t level_stride) {
    __shared__ double wred[kValWaves][kFvPartial];
    __shared__ int hist[kPairs];
    const int64_t GK = G * K;
    const Records lv = slice(all, (int64_t)blockIdx.y * GK);
    double* part = partial + (int64_t)blockIdx.y * level_stride;
    int32_t* pairs = reinterpret_cast<int32_t*>(part + kFvPairsAt);
    int32_t* counts = reinterpret_cast<int32_t*>(part + kFvCountsAt);
    // uniform over the workgroup, so the barriers inside are reached by all of its threads
    if (records_aligned16(lv) && (!PAIRED || records_aligned16(all))) {
        failure_reduce_block<true, PAIRED>(lv, all, q, GK, G, K, (int64_t)blockIdx.x, (int64_t)gridDim.x, part, pairs,
                                           counts, wred, hist);
    } else {
        failure_reduce_block<false, PAIRED>(lv, all, q, GK, G, K, (int64_t)blockIdx.x, (int64_t)gridDim.x, part,
                                            pairs, counts, wred, hist);
    }
}

constexpr int kFinishBatch = 8;  // loads in flight per lane in the finish's sums over the workgroups

struct FailureFinishArgs {
    dxrl_pg_val_failure_args a;
    int64_t level_stride;
    int32_t blocks;
};

__global__ __launch_bounds__(kMaxLevels* kWave) void k_pg_val_failure_finish(const FailureFinishArgs f) {
    __shared__ double mode_rows[kMaxLevels][kModes][kModeCols];
    __shared__ double level_rows[kMaxLevels][kLevelCols];
    __shared__ double sums[kMaxLevels][kFvPartial];
    const dxrl_pg_val_failure_args& a = f.a;
    const int lane = threadIdx.x % kWave, l = threadIdx.x / kWave, L = a.num_levels;  // blockDim.x == L * kWave
    const int64_t G = a.num_objects, K = a.episodes_per_object;
    const double* partial = a.partial + (int64_t)l * f.level_stride;
    // the workgroup partials in index order, a column per lane; the loads go out eight at a time
    // (an absent workgroup adds +0.0 to a sum that is never -0.0)
    if (lane < kFvPartial) {
        double v = 0.0;
        for (int b0 = 0; b0 < f.blocks; b0 += kFinishBatch) {
            double t[kFinishBatch];
#pragma unroll
            for (int j = 0; j < kFinishBatch; ++j)
                t[j] = b0 + j < f.blocks ? partial[(int64_t)(b0 + j) * kFvPartial + lane] : 0.0;
#pragma unroll
            for (int j = 0; j < kFinishBatch; ++j) v += t[j];
        }
        sums[l][lane] = v;
    }
    // the objects: per mode how many hold it, the most one holds, and the first that holds that many
    const int32_t* counts = reinterpret_cast<const int32_t*>(partial + kFvCountsAt);
    int holders[kModes], most[kModes], first[kModes];
#pragma unroll
    for (int m = 0; m < kModes; ++m) holders[m] = 0, most[m] = 0, first[m] = INT_MAX;
    for (int64_t o = lane; o < G; o += kWave) {
#pragma unroll
        for (int m = 0; m < kModes; ++m) {
            const int c = counts[o * kModes + m];
            holders[m] += c > 0;
            if (c > most[m]) most[m] = c, first[m] = (int)o;  // ascending o: the lane's first maximum
        }
    }
#pragma unroll
    for (int m = 0; m < kModes; ++m) {
        holders[m] = wave_sum(holders[m]);
        const int top = __shfl(wave_max(most[m]), 0, kWave);
        first[m] = wave_min(most[m] == top && top > 0 ? first[m] : INT_MAX);
        most[m] = top;
    }
    __syncthreads();  // sums
    if (lane < kModes) {  // lane m forms the quotients of mode m; lane 0 also the level's row
        const double* s = sums[l];
        const double n = (double)(G * K);
        double F = 0.0, conf = 0.0, top = 0.0;
        int dominant = -1, present = 0;
#pragma unroll
        for (int m = 0; m < kModes; ++m) {
            const double c = s[m * F_PER_MODE + F_COUNT];
            F += c;
            conf += s[m * F_PER_MODE + F_CONF];
            present += c > 0.0;
            if (c > top) top = c, dominant = m;  // strict: the first mode with the largest count
        }
        const double* t = s + lane * F_PER_MODE;
        double* r = mode_rows[l][lane];
        const double c = t[F_COUNT];
        const bool any = c > 0.0;
        const long long ci = (long long)c, s1 = (long long)t[F_S1], s2 = (long long)t[F_S2];
        r[DXRL_PG_VAL_FAILURE_COUNT] = c;
        r[DXRL_PG_VAL_FAILURE_FREQUENCY] = F > 0.0 ? c / F : 0.0;
        r[DXRL_PG_VAL_FAILURE_EPISODE_SHARE] = c / n;
        r[DXRL_PG_VAL_FAILURE_MEAN_EPISODE_LENGTH] = any ? t[F_S1] / c : 0.0;
        r[DXRL_PG_VAL_FAILURE_STD_EPISODE_LENGTH] = any ? sqrt((double)(ci * s2 - s1 * s1) / (double)(ci * ci)) : 0.0;
        r[DXRL_PG_VAL_FAILURE_MEAN_FINAL_CONTACTS] = any ? t[F_C1] / c : 0.0;
        r[DXRL_PG_VAL_FAILURE_MEAN_CONFIDENCE] = any ? t[F_CONF] / c : 0.0;
        if (lane == 0) {
#pragma unroll
            for (int m = 0; m < kModes; ++m) {  // the object columns: the wave reductions end in lane 0
                double* q = mode_rows[l][m];
                q[DXRL_PG_VAL_FAILURE_OBJECTS] = (double)holders[m];
                q[DXRL_PG_VAL_FAILURE_MAX_OBJECT_COUNT] = (double)most[m];
                q[DXRL_PG_VAL_FAILURE_WORST_OBJECT] = most[m] > 0 ? (double)first[m] : -1.0;
            }
            double* v = level_rows[l];
            v[DXRL_PG_VAL_FAILURE_LEVEL_EPISODES] = n;
            v[DXRL_PG_VAL_FAILURE_LEVEL_FAILURES] = F;
            v[DXRL_PG_VAL_FAILURE_LEVEL_FAILURE_RATE] = F / n;
            v[DXRL_PG_VAL_FAILURE_LEVEL_DOMINANT_MODE] = (double)dominant;
            v[DXRL_PG_VAL_FAILURE_LEVEL_DOMINANT_FREQUENCY] = F > 0.0 ? top / F : 0.0;
            v[DXRL_PG_VAL_FAILURE_LEVEL_MODES_PRESENT] = (double)present;
            v[DXRL_PG_VAL_FAILURE_LEVEL_TIE_ROWS] = s[kFvTies];
            v[DXRL_PG_VAL_FAILURE_LEVEL_MEAN_CONFIDENCE] = F > 0.0 ? conf / F : 0.0;
        }
    }
    if (a.paired && lane < kPairs) {  // the class pairs: integer sums over the workgroups
        const int32_t* pairs = reinterpret_cast<const int32_t*>(partial + kFvPairsAt);
        int t = 0;
        for (int b0 = 0; b0 < f.blocks; b0 += kFinishBatch) {
            int u[kFinishBatch];
#pragma unroll
            for (int j = 0; j < kFinishBatch; ++j) u[j] = b0 + j < f.blocks ? pairs[(b0 + j) * kFvPairInts + lane] : 0;
#pragma unroll
            for (int j = 0; j < kFinishBatch; ++j) t += u[j];
        }
        a.failure_transitions[(a.row * L + l) * kPairs + lane] = t;
    }
    __syncthreads();
    // the rows of the levels are contiguous in LDS and in the tables
    for (int i = threadIdx.x; i < L * kModes * kModeCols; i += blockDim.x)
        a.failure_modes[a.row * L * kModes * kModeCols + i] = (&mode_rows[0][0][0])[i];
    if ((int)threadIdx.x < L * kLevelCols)
        a.failure_levels[a.row * L * kLevelCols + threadIdx.x] = (&level_rows[0][0])[threadIdx.x];
}

int check_shape(int64_t L, int64_t G, int64_t K) {
    DXRL_REQUIRE(L >= 1 && L <= kMaxLevels, "num_levels %lld outside [1, %d]", (long long)L, kMaxLevels);
    DXRL_REQUIRE(G >= 1 && K >= 1, "num_objects and episodes_per_object must be >= 1");
    DXRL_REQUIRE(G <= INT32_MAX / K && L * G * K <= (int64_t)INT32_MAX,
                 "num_levels x num_objects x episodes_per_object exceeds INT32_MAX");
    DXRL_REQUIRE(G * K <= kMaxRecords,
                 "num_objects x episodes_per_object = %lld exceeds %lld (the exact integer variance of the lengths)",
                 (long long)(G * K), (long long)kMaxRecords);
    return DXRL_OK;
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_pg_val_failure_partial_doubles(int32_t num_levels, int64_t num_objects,
                                                   int64_t episodes_per_object, int64_t* out) {
    using namespace dxrl;
    DXRL_REQUIRE(out, "null out");
    if (int rc = check_shape(num_levels, num_objects, episodes_per_object)) return rc;
    *out = num_levels * failure_partial_doubles(num_objects);
    return DXRL_OK;
}

extern "C" int dxrl_pg_val_failure_row(int32_t device, const dxrl_pg_val_failure_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_pg_val_failure_args& a = *args;
    const int64_t G = a.num_objects, K = a.episodes_per_object, L = a.num_levels;
    if (int rc = check_shape(L, G, K)) return rc;
    DXRL_REQUIRE(a.max_steps >= 1 && a.max_steps <= DXRL_SUMMARY_MAX_STEPS,
                 "max_steps must be in [1, %d] (the exact integer variance rule), got %d", DXRL_SUMMARY_MAX_STEPS,
                 a.max_steps);
    DXRL_REQUIRE(a.timeout_steps >= 1, "timeout_steps must be >= 1, got %d", a.timeout_steps);
    DXRL_REQUIRE(a.cap >= 1 && a.row >= 0 && a.row < a.cap, "row %lld lies outside the table (%lld rows)",
                 (long long)a.row, (long long)a.cap);
    DXRL_REQUIRE(a.ep_length && a.ep_success && a.ep_contacts && a.hist_moments, "null episode records");
    DXRL_REQUIRE(a.partial && a.failure_modes && a.failure_levels, "null partial / failure_modes / failure_levels");
    DXRL_REQUIRE(!a.paired || a.failure_transitions, "paired needs failure_transitions");
    const int64_t stride = failure_partial_doubles(G), blocks = val_grid(G, K);
    DXRL_REQUIRE(a.partial_doubles >= L * stride, "partial holds %lld doubles, needs %lld",
                 (long long)a.partial_doubles, (long long)(L * stride));
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    const Records all{a.ep_length, a.ep_success, a.ep_contacts, a.hist_moments};
    const Rules q{a.max_steps, a.timeout_steps, a.success_threshold};
    const dim3 grid((unsigned)blocks, (unsigned)L), threads(kValThreads);
    if (a.paired)
        hipLaunchKernelGGL(k_pg_val_failure_reduce<true>, grid, threads, 0, st, all, q, G, K, a.partial, stride);
    else
        hipLaunchKernelGGL(k_pg_val_failure_reduce<false>, grid, threads, 0, st, all, q, G, K, a.partial, stride);
    if (int rc = launch_check("k_pg_val_failure_reduce")) return rc;
    FailureFinishArgs f{a, stride, (int32_t)blocks};
    hipLaunchKernelGGL(k_pg_val_failure_finish, dim3(1), dim3((unsigned)(L * kWave)), 0, st, f);
    return launch_check("k_pg_val_failure_finish");
}
