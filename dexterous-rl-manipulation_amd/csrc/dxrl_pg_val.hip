// dxrl_pg_val.hip -- the held-out validation row of a training run (include/dxrl.h,
// dxrl_pg_val_row): the episode records dxrl_evaluate_mlp left on the device, reduced to one f64
// row of a device table, with keep-best and patience applied to a small device header, so a
// training run validates on held-out objects without a host sync.
//
// The input is small (14 bytes per episode record: 9 KB at 640 episodes, 573 KB at 40,960), so the
// call is bound by its dependent launches, not by bytes.  Up to three, all behind the episode
// kernel on the caller's stream:
//   k_pg_val_reduce     workgroups of 256 threads over chunks of 1,024 consecutive records, 4 per
//                       thread (one 16-byte load of lengths, two of returns, one 4-byte load each
//                       of success and contact bytes where the pointers are 16-byte aligned and
//                       the four records exist; scalar loads otherwise -- the same records in the
//                       same order either way).  Integer sums; the returns as (count, mean, M2)
//                       of ep_return - ep_return[0], one record merged at a time.  Lanes by
//                       shuffles in a fixed order, the four waves through LDS, one 8-double
//                       partial per workgroup.  At most 64 workgroups (65,536 records in one
//                       pass; a grid-stride loop beyond), so the finish reads one partial per
//                       lane.  The same waves count the successes of whole objects (object o =
//                       records [o K, (o + 1) K)): one object per wave at a time, into i32 counts
//                       behind the partials in the scratch.
//   k_pg_val_finish     one wave: merges the partials in index order, takes the minimum and the
//                       solved count over the objects, writes the row and the optional
//                       object_successes row, applies keep-best and patience to the header.
//   k_pg_val_keep_best  copies params to best_params iff the row's is_best flag is set (read on
//                       the device).
// A single-workgroup path that folds reduce and finish into one launch for small E was not built:
// it would save one dependent launch (about 5 us) behind an episode kernel of a millisecond.
// No floating-point atomics, no tickets, no spin-waits: the launch order is the only ordering.
#include "dxrl_internal.h"
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
constexpr int kCopyThreads = 256;
enum { V_N, V_MEAN, V_M2, V_LEN, V_SUC, V_SLEN, V_CON, V_PAD };
static_assert(V_PAD + 1 == kValPartial, "partial layout");
static_assert(kValMaxBlocks <= kWave, "the finish reads one partial per lane");

inline int64_t val_grid(int64_t G, int64_t K) {
    const int64_t chunks = (G * K + kValChunk - 1) / kValChunk;
    const int64_t by_objects = (G + kValWaves - 1) / kValWaves;
    const int64_t b = chunks > by_objects ? chunks : by_objects;
    return b < 1 ? 1 : b > kValMaxBlocks ? kValMaxBlocks : b;
}
inline int64_t val_partial_doubles(int64_t G) { return (int64_t)kValMaxBlocks * kValPartial + (G + 1) / 2; }

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// fixed-order wave reductions by lane shuffles (offsets 32, 16, .., 1); lane 0 holds the result
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const int b = __shfl_down(v, o, kWave);
        v = b < v ? b : v;
    }
    return v;
}
__device__ __forceinline__ Moments wave_moments(Moments v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const Moments b{__shfl_down(v.n, o, kWave), __shfl_down(v.mean, o, kWave), __shfl_down(v.m2, o, kWave)};
        v = merge(v, b);
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(kValThreads) void k_pg_val_reduce(
    const double* __restrict__ ep_return, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts, int64_t E, int64_t G, int64_t K,
    double* __restrict__ partial, int32_t* __restrict__ counts) {
    __shared__ double wred[kValWaves][kValPartial];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const double K0 = ep_return[0];  // E >= 1
    Moments m{0.0, 0.0, 0.0};
    long long s_len = 0, s_suc = 0, s_slen = 0, s_con = 0;
    for (int64_t base = (int64_t)blockIdx.x * kValChunk; base < E; base += (int64_t)gridDim.x * kValChunk) {
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
        double* p = partial + (int64_t)blockIdx.x * kValPartial;
        p[V_N] = t.n, p[V_MEAN] = t.mean, p[V_M2] = t.m2;
        p[V_LEN] = tot[0], p[V_SUC] = tot[1], p[V_SLEN] = tot[2], p[V_CON] = tot[3], p[V_PAD] = 0.0;
    }
    // successes of whole objects, one object per wave at a time
    const int64_t waves = (int64_t)gridDim.x * kValWaves;
    for (int64_t o = (int64_t)blockIdx.x * kValWaves + wave; o < G; o += waves) {
        int n = 0;
        for (int64_t k = lane; k < K; k += kWave) n += ep_success[o * K + k] != 0;
        n = wave_sum(n);
        if (lane == 0) counts[o] = n;
    }
}

struct FinishArgs {
    dxrl_pg_val_args a;
    int32_t blocks;
};

__global__ __launch_bounds__(kWave) void k_pg_val_finish(const FinishArgs f) {
    __shared__ double out[DXRL_PG_VAL_COLS];
    const dxrl_pg_val_args& a = f.a;
    const int lane = threadIdx.x;
    const int64_t G = a.num_objects, K = a.episodes_per_object;
    // one workgroup partial per lane (blocks <= 64), then the fixed wave order
    Moments m{0.0, 0.0, 0.0};
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < f.blocks) {
        const double* p = a.partial + (int64_t)lane * kValPartial;
        m = Moments{p[V_N], p[V_MEAN], p[V_M2]};
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = p[V_LEN + k];
    }
    m = wave_moments(m);
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
    // the objects: worst success count, solved count, and the optional per-object row
    const int32_t* counts = reinterpret_cast<const int32_t*>(a.partial + (int64_t)kValMaxBlocks * kValPartial);
    int worst = INT_MAX, solved = 0;
    for (int64_t o = lane; o < G; o += kWave) {
        const int c = counts[o];
        worst = c < worst ? c : worst;
        solved += (double)c / (double)K >= a.solve_threshold;
        if (a.object_successes) a.object_successes[a.row * G + o] = c;
    }
    worst = wave_min(worst);
    solved = wave_sum(solved);

    if (lane == 0) {
        const double E = (double)(G * K), nan = quiet_nan();
        const double s_len = s[0], s_suc = s[1], s_slen = s[2], s_con = s[3];
        const int32_t status = *a.status;
        for (int k = 0; k < DXRL_PG_VAL_COLS; ++k) out[k] = 0.0;
        out[DXRL_PG_VAL_ITERATION] = (double)a.iteration;
        out[DXRL_PG_VAL_ENV_STEPS] = (double)a.env_steps;
        out[DXRL_PG_VAL_TRAIN_ROW] = (double)a.train_row;
        out[DXRL_PG_VAL_EPISODES] = E;
        out[DXRL_PG_VAL_SUCCESSES] = s_suc;
        out[DXRL_PG_VAL_SUCCESS_RATE] = s_suc / E;
        out[DXRL_PG_VAL_MEAN_RETURN] = a.ep_return[0] + m.mean;
        out[DXRL_PG_VAL_RETURN_STD] = sqrt(m.m2 / m.n);
        out[DXRL_PG_VAL_MEAN_LENGTH] = s_len / E;
        out[DXRL_PG_VAL_MEAN_SUCCESS_LENGTH] = s_suc > 0.0 ? s_slen / s_suc : nan;
        out[DXRL_PG_VAL_MEAN_CONTACTS] = s_con / E;
        out[DXRL_PG_VAL_MIN_OBJECT_SUCCESS_RATE] = (double)worst / (double)K;
        out[DXRL_PG_VAL_OBJECTS_SOLVED] = (double)solved;
        out[DXRL_PG_VAL_EVAL_STATUS] = (double)status;
        dxrl_pg_val_header* h = a.header;
        // keep-best: strict >, so the first maximum wins and a NaN is never best
        bool best = false;
        if (a.score_col >= 0) {
            const double score = out[a.score_col];
            if (status == 0 && score > h->best_score + a.min_delta) {
                best = true;
                h->best_score = score;
                h->best_row = a.row;
            }
        }
        const int64_t since = best ? 0 : h->since_best + 1;
        out[DXRL_PG_VAL_IS_BEST] = best ? 1.0 : 0.0;
        out[DXRL_PG_VAL_SINCE_BEST] = (double)since;
        h->since_best = since;
        if (a.patience > 0 && h->stopped_row < 0 && since >= (int64_t)a.patience) h->stopped_row = a.row;
        h->rows_written = a.row + 1;
    }
    __syncthreads();
    if (lane < DXRL_PG_VAL_COLS) a.val[a.row * DXRL_PG_VAL_COLS + lane] = out[lane];
}

// params -> best_params iff the row's is_best flag is set; 16-byte copies where both pointers
// allow, scalar otherwise and for the tail
__global__ __launch_bounds__(kCopyThreads) void k_pg_val_keep_best(const double* __restrict__ flag,
                                                                   const float* __restrict__ params,
                                                                   float* __restrict__ best, int64_t n, int vec) {
    if (*flag == 0.0) return;
    const int64_t i = (int64_t)blockIdx.x * kCopyThreads + threadIdx.x;
    if (vec && 4 * i + 4 <= n) {
        reinterpret_cast<float4*>(best)[i] = reinterpret_cast<const float4*>(params)[i];
    } else {
        for (int64_t k = 4 * i; k < 4 * i + 4 && k < n; ++k) best[k] = params[k];
    }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_pg_val_partial_doubles(int64_t num_objects, int64_t episodes_per_object, int64_t* out) {
    using namespace dxrl;
    DXRL_REQUIRE(out, "null out");
    DXRL_REQUIRE(num_objects >= 1 && episodes_per_object >= 1, "num_objects and episodes_per_object must be >= 1");
    DXRL_REQUIRE(num_objects <= INT32_MAX / episodes_per_object, "num_objects x episodes_per_object exceeds INT32_MAX");
    *out = val_partial_doubles(num_objects);
    return DXRL_OK;
}

extern "C" int dxrl_pg_val_row(int32_t device, const dxrl_pg_val_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_pg_val_args& a = *args;
    const int64_t G = a.num_objects, K = a.episodes_per_object;
    DXRL_REQUIRE(G >= 1 && K >= 1, "num_objects and episodes_per_object must be >= 1");
    DXRL_REQUIRE(G <= INT32_MAX / K, "num_objects x episodes_per_object exceeds INT32_MAX");
    DXRL_REQUIRE(a.cap >= 1 && a.row >= 0 && a.row < a.cap, "row %lld lies outside the table (%lld rows)",
                 (long long)a.row, (long long)a.cap);
    DXRL_REQUIRE(a.score_col < DXRL_PG_VAL_IS_BEST, "score_col %d out of range (< %d, or < 0 for none)", a.score_col,
                 (int)DXRL_PG_VAL_IS_BEST);
    DXRL_REQUIRE(a.patience >= 0, "patience must be >= 0, got %d", a.patience);
    DXRL_REQUIRE(a.ep_return && a.ep_length && a.ep_success && a.ep_contacts && a.status,
                 "null episode records / status");
    DXRL_REQUIRE(a.partial && a.val && a.header, "null partial / val / header");
    DXRL_REQUIRE((a.params != nullptr) == (a.best_params != nullptr), "params and best_params go together");
    DXRL_REQUIRE(!a.params || a.num_params >= 1, "keep-best needs num_params >= 1");
    DXRL_REQUIRE(a.partial_doubles >= val_partial_doubles(G), "partial holds %lld doubles, needs %lld",
                 (long long)a.partial_doubles, (long long)val_partial_doubles(G));
    const int64_t E = G * K, blocks = val_grid(G, K);
    const bool copy = a.score_col >= 0 && a.params;
    int32_t* counts = reinterpret_cast<int32_t*>(a.partial + (int64_t)kValMaxBlocks * kValPartial);
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    if (aligned16(a.ep_return) && aligned16(a.ep_length) && aligned16(a.ep_success) && aligned16(a.ep_contacts)) {
        hipLaunchKernelGGL(k_pg_val_reduce<true>, dim3((unsigned)blocks), dim3(kValThreads), 0, st, a.ep_return,
                           a.ep_length, a.ep_success, a.ep_contacts, E, G, K, a.partial, counts);
    } else {
        hipLaunchKernelGGL(k_pg_val_reduce<false>, dim3((unsigned)blocks), dim3(kValThreads), 0, st, a.ep_return,
                           a.ep_length, a.ep_success, a.ep_contacts, E, G, K, a.partial, counts);
    }
    if (int rc = launch_check("k_pg_val_reduce")) return rc;
    FinishArgs f{a, (int32_t)blocks};
    hipLaunchKernelGGL(k_pg_val_finish, dim3(1), dim3(kWave), 0, st, f);
    if (int rc = launch_check("k_pg_val_finish")) return rc;
    if (copy) {
        const int64_t quads = (a.num_params + 3) / 4;
        hipLaunchKernelGGL(k_pg_val_keep_best, dim3((unsigned)((quads + kCopyThreads - 1) / kCopyThreads)),
                           dim3(kCopyThreads), 0, st, a.val + a.row * DXRL_PG_VAL_COLS + DXRL_PG_VAL_IS_BEST, a.params,
                           a.best_params, a.num_params, (int)(aligned16(a.params) && aligned16(a.best_params)));
        if (int rc = launch_check("k_pg_val_keep_best")) return rc;
    }
    return DXRL_OK;
}
