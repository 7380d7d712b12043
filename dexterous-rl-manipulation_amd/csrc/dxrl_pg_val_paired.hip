// dxrl_pg_val_paired.hip -- the paired rows of a noise-level validation run with common random
// numbers (include/dxrl.h, dxrl_pg_val_paired_row).  With dxrl_eval_args.stream_period = G K every
// level of the level-major records replays the baseline's G K episodes under its own noise scale,
// so record l G K + i and record i are one pair: this reduces, per level, which pairs were lost
// and gained and the moments of the per-pair return difference, and leaves the header and the
// three tables of dxrl_pg_val_levels_row alone.
//
// Two launches behind dxrl_pg_val_levels_row, whatever L is:
//   k_pg_val_paired_reduce  a (val_grid(G, K), L) grid: blockIdx.y is the level.  The chunks, the
//                           four consecutive pairs of a thread and the merge order are
//                           val_reduce_block's (dxrl_pg_val_common.h); the 16-byte loads are taken
//                           where the level's and the baseline's slices are all aligned, the scalar
//                           loads otherwise, in the same pair order.  The lost pairs of whole
//                           objects are counted one object per wave.
//   k_pg_val_paired_finish  one workgroup, one wave per level: the wave merges its level's
//                           partials in index order, lane 0 forms the columns in LDS, and after
//                           one barrier the workgroup writes the L rows.
// merge and wave_moments are dxrl_moments.h's, wave_sum / wave_max / quiet_nan / aligned16
// dxrl_reduce.h's, the grid and the scratch size dxrl_pg_val_common.h's.  No floating-point
// atomics, no tickets, no spin-waits: the launch order is the only ordering.
#include "dxrl_pg_val_common.h"

namespace dxrl {
namespace {

constexpr int kMaxLevels = DXRL_PG_VAL_MAX_LEVELS;
constexpr int kCols = DXRL_PG_VAL_PAIRED_COLS;
static_assert(kMaxLevels * kWave <= 1024, "one wave per level in one workgroup");
static_assert(DXRL_PG_VAL_PAIRED_NAMED == DXRL_PG_VAL_PAIRED_COLS, "column enum");
// a workgroup partial: the moments of d - d_first, then the integer sums (exact as doubles)
enum { P_N, P_MEAN, P_M2, P_LOST, P_GAINED, P_BOTH, P_DLEN, P_PAD };
static_assert(P_PAD + 1 == kValPartial, "partial layout");

// One reduce workgroup over the E pairs (r1[i], r0[i]): its partial into partial[block], the lost
// pairs of its objects into counts.
template <bool VEC>
__device__ __forceinline__ void paired_reduce_block(const double* __restrict__ r0, const double* __restrict__ r1,
                                                    const int32_t* __restrict__ l0, const int32_t* __restrict__ l1,
                                                    const uint8_t* __restrict__ s0, const uint8_t* __restrict__ s1,
                                                    int64_t E, int64_t G, int64_t K, int64_t block, int64_t blocks,
                                                    double* __restrict__ partial, int32_t* __restrict__ counts,
                                                    double (*wred)[kValPartial]) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const double d_first = r1[0] - r0[0];  // E >= 1
    Moments m{0.0, 0.0, 0.0};
    long long n_lost = 0, n_gained = 0, n_both = 0, s_dlen = 0;
    for (int64_t base = block * kValChunk; base < E; base += blocks * kValChunk) {
        const int64_t i0 = base + (int64_t)threadIdx.x * kValPerThread;
        if (i0 >= E) continue;
        const int cnt = E - i0 >= kValPerThread ? kValPerThread : (int)(E - i0);
        double ra[kValPerThread], rb[kValPerThread];
        int32_t la[kValPerThread], lb[kValPerThread];
        uint8_t sa[kValPerThread], sb[kValPerThread];
        if (VEC && cnt == kValPerThread) {
            const double2 a0 = *reinterpret_cast<const double2*>(r0 + i0);
            const double2 a1 = *reinterpret_cast<const double2*>(r0 + i0 + 2);
            const double2 b0 = *reinterpret_cast<const double2*>(r1 + i0);
            const double2 b1 = *reinterpret_cast<const double2*>(r1 + i0 + 2);
            const int4 lva = *reinterpret_cast<const int4*>(l0 + i0);
            const int4 lvb = *reinterpret_cast<const int4*>(l1 + i0);
            const uint32_t sva = *reinterpret_cast<const uint32_t*>(s0 + i0);
            const uint32_t svb = *reinterpret_cast<const uint32_t*>(s1 + i0);
            ra[0] = a0.x, ra[1] = a0.y, ra[2] = a1.x, ra[3] = a1.y;
            rb[0] = b0.x, rb[1] = b0.y, rb[2] = b1.x, rb[3] = b1.y;
            la[0] = lva.x, la[1] = lva.y, la[2] = lva.z, la[3] = lva.w;
            lb[0] = lvb.x, lb[1] = lvb.y, lb[2] = lvb.z, lb[3] = lvb.w;
#pragma unroll
            for (int k = 0; k < kValPerThread; ++k) sa[k] = (uint8_t)(sva >> (8 * k)), sb[k] = (uint8_t)(svb >> (8 * k));
        } else {
#pragma unroll
            for (int k = 0; k < kValPerThread; ++k) {  // clamped: every slot loads an in-range pair
                const int64_t i = i0 + (k < cnt ? k : cnt - 1);
                ra[k] = r0[i], rb[k] = r1[i], la[k] = l0[i], lb[k] = l1[i], sa[k] = s0[i], sb[k] = s1[i];
            }
        }
#pragma unroll
        for (int k = 0; k < kValPerThread; ++k) {
            if (k < cnt) {
                const double d = rb[k] - ra[k];
                m = merge(m, Moments{1.0, d - d_first, 0.0});
                s_dlen += (long long)lb[k] - (long long)la[k];
                const bool base_ok = sa[k] != 0, level_ok = sb[k] != 0;
                n_lost += base_ok && !level_ok;
                n_gained += !base_ok && level_ok;
                n_both += base_ok && level_ok;
            }
        }
    }
    // the integer sums are below 2^53 in magnitude: exact as doubles in any order
    m = wave_moments(m);
    double acc[4] = {(double)n_lost, (double)n_gained, (double)n_both, (double)s_dlen};
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = wave_sum(acc[k]);
    if (lane == 0) {
        wred[wave][P_N] = m.n, wred[wave][P_MEAN] = m.mean, wred[wave][P_M2] = m.m2;
#pragma unroll
        for (int k = 0; k < 4; ++k) wred[wave][P_LOST + k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Moments t{wred[0][P_N], wred[0][P_MEAN], wred[0][P_M2]};
        double tot[4] = {wred[0][P_LOST], wred[0][P_GAINED], wred[0][P_BOTH], wred[0][P_DLEN]};
        for (int w = 1; w < kValWaves; ++w) {
            t = merge(t, Moments{wred[w][P_N], wred[w][P_MEAN], wred[w][P_M2]});
#pragma unroll
            for (int k = 0; k < 4; ++k) tot[k] += wred[w][P_LOST + k];
        }
        double* p = partial + block * kValPartial;
        p[P_N] = t.n, p[P_MEAN] = t.mean, p[P_M2] = t.m2;
        p[P_LOST] = tot[0], p[P_GAINED] = tot[1], p[P_BOTH] = tot[2], p[P_DLEN] = tot[3], p[P_PAD] = 0.0;
    }
    // lost pairs of whole objects, one object per wave at a time
    const int64_t waves = blocks * kValWaves;
    for (int64_t o = block * kValWaves + wave; o < G; o += waves) {
        int n = 0;
        for (int64_t k = lane; k < K; k += kWave) n += s0[o * K + k] != 0 && s1[o * K + k] == 0;
        n = wave_sum(n);
        if (lane == 0) counts[o] = n;
    }
}

__global__ __launch_bounds__(kValThreads) void k_pg_val_paired_reduce(const double* __restrict__ ep_return,
                                                                      const int32_t* __restrict__ ep_length,
                                                                      const uint8_t* __restrict__ ep_success,
                                                                      int64_t G, int64_t K,
                                                                      double* __restrict__ partial,
                                                                      int64_t level_stride) {
    __shared__ double wred[kValWaves][kValPartial];
    const int64_t GK = G * K, first = (int64_t)blockIdx.y * GK;
    const double* r1 = ep_return + first;
    const int32_t* l1 = ep_length + first;
    const uint8_t* s1 = ep_success + first;
    double* part = partial + (int64_t)blockIdx.y * level_stride;
    int32_t* counts = reinterpret_cast<int32_t*>(part + (int64_t)kValMaxBlocks * kValPartial);
    // uniform over the workgroup, so the barrier inside is reached by all of its threads
    if (aligned16(ep_return) && aligned16(ep_length) && aligned16(ep_success) && aligned16(r1) && aligned16(l1) &&
        aligned16(s1)) {
        paired_reduce_block<true>(ep_return, r1, ep_length, l1, ep_success, s1, GK, G, K, (int64_t)blockIdx.x,
                                  (int64_t)gridDim.x, part, counts, wred);
    } else {
        paired_reduce_block<false>(ep_return, r1, ep_length, l1, ep_success, s1, GK, G, K, (int64_t)blockIdx.x,
                                   (int64_t)gridDim.x, part, counts, wred);
    }
}

struct PairedFinishArgs {
    dxrl_pg_val_paired_args a;
    int64_t level_stride;
    int32_t blocks;
};

__global__ __launch_bounds__(kMaxLevels* kWave) void k_pg_val_paired_finish(const PairedFinishArgs f) {
    __shared__ double rows[kMaxLevels][kCols];
    const dxrl_pg_val_paired_args& a = f.a;
    const int lane = threadIdx.x % kWave, l = threadIdx.x / kWave, L = a.num_levels;  // blockDim.x == L * kWave
    const int64_t G = a.num_objects, K = a.episodes_per_object, GK = G * K;
    const double* partial = a.partial + (int64_t)l * f.level_stride;
    // one workgroup partial per lane (blocks <= 64), then the fixed wave order
    Moments m{0.0, 0.0, 0.0};
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (lane < f.blocks) {
        const double* p = partial + (int64_t)lane * kValPartial;
        m = Moments{p[P_N], p[P_MEAN], p[P_M2]};
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = p[P_LOST + k];
    }
    m = wave_moments(m);
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
    // the objects: how many lost a pair, the most one lost, and the optional per-object row
    const int32_t* counts = reinterpret_cast<const int32_t*>(partial + (int64_t)kValMaxBlocks * kValPartial);
    int32_t* object_row = a.object_lost ? a.object_lost + (a.row * L + l) * G : nullptr;
    int with_loss = 0, most = 0;
    for (int64_t o = lane; o < G; o += kWave) {
        const int c = counts[o];
        with_loss += c > 0;
        most = c > most ? c : most;
        if (object_row) object_row[o] = c;
    }
    with_loss = wave_sum(with_loss);
    most = wave_max(most);
    if (lane == 0) {
        double* r = rows[l];
        const double n = (double)GK, lost = s[0], gained = s[1], both = s[2];
        const double d_first = a.ep_return[(int64_t)l * GK] - a.ep_return[0];
        r[DXRL_PG_VAL_PAIRED_PAIRS] = n;
        r[DXRL_PG_VAL_PAIRED_LOST] = lost;
        r[DXRL_PG_VAL_PAIRED_GAINED] = gained;
        r[DXRL_PG_VAL_PAIRED_BOTH_SUCCESS] = both;
        r[DXRL_PG_VAL_PAIRED_BOTH_FAIL] = n - lost - gained - both;
        r[DXRL_PG_VAL_PAIRED_MEAN_RETURN_DIFF] = d_first + m.mean;
        r[DXRL_PG_VAL_PAIRED_RETURN_DIFF_STD] = sqrt(m.m2 / m.n);
        r[DXRL_PG_VAL_PAIRED_RETURN_DIFF_STDERR] = GK > 1 ? sqrt(m.m2 / (m.n * (m.n - 1.0))) : quiet_nan();
        r[DXRL_PG_VAL_PAIRED_MEAN_LENGTH_DIFF] = s[3] / n;
        // the header's f64 operations in its order
        const double dn = lost - gained, dc = lost + gained;
        r[DXRL_PG_VAL_PAIRED_DEGRADATION] = dn / n;
        double q = dn * dn;
        q = q / n;
        double v = dc - q;
        v = v / n;
        v = v > 0.0 ? v : 0.0;
        r[DXRL_PG_VAL_PAIRED_DEGRADATION_STDERR] = sqrt(v) / sqrt(n);
        r[DXRL_PG_VAL_PAIRED_MCNEMAR] = dc > 0.0 ? (dn * dn) / dc : 0.0;
        r[DXRL_PG_VAL_PAIRED_OBJECTS_WITH_LOSS] = (double)with_loss;
        r[DXRL_PG_VAL_PAIRED_MAX_OBJECT_LOST] = (double)most;
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < L * kCols)  // rows' rows are contiguous: flat index l * kCols + column
        a.paired[a.row * L * kCols + i] = (&rows[0][0])[i];
}

int check_shape(int64_t L, int64_t G, int64_t K) {
    DXRL_REQUIRE(L >= 1 && L <= kMaxLevels, "num_levels %lld outside [1, %d]", (long long)L, kMaxLevels);
    DXRL_REQUIRE(G >= 1 && K >= 1, "num_objects and episodes_per_object must be >= 1");
    DXRL_REQUIRE(G <= INT32_MAX / K && L * G * K <= (int64_t)INT32_MAX,
                 "num_levels x num_objects x episodes_per_object exceeds INT32_MAX");
    return DXRL_OK;
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_pg_val_paired_partial_doubles(int32_t num_levels, int64_t num_objects,
                                                  int64_t episodes_per_object, int64_t* out) {
    using namespace dxrl;
    DXRL_REQUIRE(out, "null out");
    if (int rc = check_shape(num_levels, num_objects, episodes_per_object)) return rc;
    *out = num_levels * val_partial_doubles(num_objects);
    return DXRL_OK;
}

extern "C" int dxrl_pg_val_paired_row(int32_t device, const dxrl_pg_val_paired_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_pg_val_paired_args& a = *args;
    const int64_t G = a.num_objects, K = a.episodes_per_object, L = a.num_levels;
    if (int rc = check_shape(L, G, K)) return rc;
    DXRL_REQUIRE(a.cap >= 1 && a.row >= 0 && a.row < a.cap, "row %lld lies outside the table (%lld rows)",
                 (long long)a.row, (long long)a.cap);
    DXRL_REQUIRE(a.ep_return && a.ep_length && a.ep_success, "null episode records");
    DXRL_REQUIRE(a.partial && a.paired, "null partial / paired");
    const int64_t stride = val_partial_doubles(G), blocks = val_grid(G, K);
    DXRL_REQUIRE(a.partial_doubles >= L * stride, "partial holds %lld doubles, needs %lld",
                 (long long)a.partial_doubles, (long long)(L * stride));
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_pg_val_paired_reduce, dim3((unsigned)blocks, (unsigned)L), dim3(kValThreads), 0, st,
                       a.ep_return, a.ep_length, a.ep_success, G, K, a.partial, stride);
    if (int rc = launch_check("k_pg_val_paired_reduce")) return rc;
    PairedFinishArgs f{a, stride, (int32_t)blocks};
    hipLaunchKernelGGL(k_pg_val_paired_finish, dim3(1), dim3((unsigned)(L * kWave)), 0, st, f);
    return launch_check("k_pg_val_paired_finish");
}
