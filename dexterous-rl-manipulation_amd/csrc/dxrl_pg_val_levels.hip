// dxrl_pg_val_levels.hip -- the noise-level validation row of a training run (include/dxrl.h,
// dxrl_pg_val_levels_row): the level-major episode records of L noise levels x G objects x K
// episodes that dxrl_evaluate_mlp left on the device, reduced to one row each of the validation
// table (level 0, the clean curve), a per-level table with the degradation columns of
// robustness_analysis.py, and a table of scores over the levels; keep-best and patience run on a
// column of the first or the last, so a run can keep the model that is best under its worst
// noise level without a host sync.
//
// At most three launches behind the episode kernel, whatever L is:
//   k_pg_val_levels_reduce  dxrl_pg_val.hip's reduce workgroup (dxrl_pg_val_common.h) over a
//                           (val_grid(G, K), L) grid: blockIdx.y is the level, its records start
//                           at l G K, its partials and object counts at l x the single-set
//                           scratch.  The 16-byte loads are taken per level where that level's
//                           four slices are aligned (with G K odd they are not); either path
//                           reads the same records in the same order.
//   k_pg_val_levels_finish  one workgroup, one wave per level: each wave is dxrl_pg_val.hip's
//                           finishing wave on its level; after one barrier thread 0 forms the
//                           degradation and robust columns in level order in LDS and applies the
//                           header rules; after a second the workgroup writes the three rows.
//   k_pg_val_keep_best      the conditional copy of params to best_params (dxrl_keep_best.h).
// L dxrl_pg_val_row calls would be 2 L + 1 dependent launches sharing one header.  No
// floating-point atomics, no tickets, no spin-waits: the launch order is the only ordering.
#include "dxrl_pg_val_common.h"

namespace dxrl {
namespace {

constexpr int kMaxLevels = DXRL_PG_VAL_MAX_LEVELS;
static_assert(kMaxLevels * kWave <= 1024, "one wave per level in one workgroup");
static_assert(DXRL_PG_VAL_LEVEL_NAMED == DXRL_PG_VAL_LEVEL_COLS && DXRL_PG_VAL_ROBUST_NAMED == DXRL_PG_VAL_ROBUST_COLS,
              "column enums");

__global__ __launch_bounds__(kValThreads) void k_pg_val_levels_reduce(
    const double* __restrict__ ep_return, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts, int64_t G, int64_t K,
    double* __restrict__ partial, int64_t level_stride) {
    __shared__ double wred[kValWaves][kValPartial];
    const int64_t GK = G * K, first = (int64_t)blockIdx.y * GK;
    const double* ret = ep_return + first;
    const int32_t* len = ep_length + first;
    const uint8_t* suc = ep_success + first;
    const uint8_t* con = ep_contacts + first;
    double* part = partial + (int64_t)blockIdx.y * level_stride;
    int32_t* counts = reinterpret_cast<int32_t*>(part + (int64_t)kValMaxBlocks * kValPartial);
    // uniform over the workgroup, so the barrier inside is reached by all of its threads
    if (aligned16(ret) && aligned16(len) && aligned16(suc) && aligned16(con)) {
        val_reduce_block<true>(ret, len, suc, con, GK, G, K, (int64_t)blockIdx.x, (int64_t)gridDim.x, part, counts,
                               wred);
    } else {
        val_reduce_block<false>(ret, len, suc, con, GK, G, K, (int64_t)blockIdx.x, (int64_t)gridDim.x, part, counts,
                                wred);
    }
}

struct LevelsFinishArgs {
    dxrl_pg_val_levels_args a;
    int64_t level_stride;
    int32_t blocks;
};

__global__ __launch_bounds__(kMaxLevels* kWave) void k_pg_val_levels_finish(const LevelsFinishArgs f) {
    __shared__ double setc[kMaxLevels][DXRL_PG_VAL_COLS];      // each level's columns, main-row layout
    __shared__ double lev[kMaxLevels][DXRL_PG_VAL_LEVEL_COLS];  // the level rows
    __shared__ double rob[DXRL_PG_VAL_ROBUST_COLS];
    const dxrl_pg_val_levels_args& a = f.a;
    const int lane = threadIdx.x % kWave, l = threadIdx.x / kWave, L = a.num_levels;  // blockDim.x == L * kWave
    const int64_t G = a.num_objects, K = a.episodes_per_object;
    const ValSetStats t =
        val_finish_set(a.partial + (int64_t)l * f.level_stride, f.blocks, G, K, a.solve_threshold,
                       a.object_successes ? a.object_successes + (a.row * L + l) * G : nullptr, lane);
    if (lane == 0) val_set_columns(setc[l], t, G, K, a.ep_return[(int64_t)l * G * K]);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int32_t status = *a.status;
        double* out = setc[0];
        out[DXRL_PG_VAL_ITERATION] = (double)a.iteration;
        out[DXRL_PG_VAL_ENV_STEPS] = (double)a.env_steps;
        out[DXRL_PG_VAL_TRAIN_ROW] = (double)a.train_row;
        out[DXRL_PG_VAL_EVAL_STATUS] = (double)status;
        const double base = out[DXRL_PG_VAL_SUCCESS_RATE];
        int worst_level = 0;
        double worst_rate = base, sum_all = 0.0, sum_noisy = 0.0, max_deg = 0.0, max_pct = 0.0;
        double worst_return = out[DXRL_PG_VAL_MEAN_RETURN];
        for (int k = 0; k < L; ++k) {
            const double* s = setc[k];
            double* r = lev[k];
            const double rate = s[DXRL_PG_VAL_SUCCESS_RATE];
            // robustness_analysis.py's f64 operations in its order
            const double degradation = base - rate;
            const double pct = base > 0.0 ? degradation / base * 100.0 : 0.0;
            r[DXRL_PG_VAL_LEVEL_OBS_NOISE_STD] = a.level_noise[2 * k];
            r[DXRL_PG_VAL_LEVEL_DYN_NOISE_STD] = a.level_noise[2 * k + 1];
            r[DXRL_PG_VAL_LEVEL_EPISODES] = s[DXRL_PG_VAL_EPISODES];
            r[DXRL_PG_VAL_LEVEL_SUCCESSES] = s[DXRL_PG_VAL_SUCCESSES];
            r[DXRL_PG_VAL_LEVEL_SUCCESS_RATE] = rate;
            r[DXRL_PG_VAL_LEVEL_MEAN_RETURN] = s[DXRL_PG_VAL_MEAN_RETURN];
            r[DXRL_PG_VAL_LEVEL_RETURN_STD] = s[DXRL_PG_VAL_RETURN_STD];
            r[DXRL_PG_VAL_LEVEL_MEAN_LENGTH] = s[DXRL_PG_VAL_MEAN_LENGTH];
            r[DXRL_PG_VAL_LEVEL_MEAN_CONTACTS] = s[DXRL_PG_VAL_MEAN_CONTACTS];
            r[DXRL_PG_VAL_LEVEL_MIN_OBJECT_SUCCESS_RATE] = s[DXRL_PG_VAL_MIN_OBJECT_SUCCESS_RATE];
            r[DXRL_PG_VAL_LEVEL_DEGRADATION] = degradation;
            r[DXRL_PG_VAL_LEVEL_DEGRADATION_PERCENTAGE] = pct;
            sum_all += rate;
            if (k > 0) {  // level 0 seeds the extrema: strict comparisons, so the first one wins
                sum_noisy += rate;
                if (rate < worst_rate) worst_rate = rate, worst_level = k;
                if (degradation > max_deg) max_deg = degradation;
                if (pct > max_pct) max_pct = pct;
                if (s[DXRL_PG_VAL_MEAN_RETURN] < worst_return) worst_return = s[DXRL_PG_VAL_MEAN_RETURN];
            }
        }
        rob[DXRL_PG_VAL_ROBUST_LEVELS] = (double)L;
        rob[DXRL_PG_VAL_ROBUST_WORST_LEVEL] = (double)worst_level;
        rob[DXRL_PG_VAL_ROBUST_WORST_SUCCESS_RATE] = worst_rate;
        rob[DXRL_PG_VAL_ROBUST_MEAN_SUCCESS_RATE] = sum_all / (double)L;
        rob[DXRL_PG_VAL_ROBUST_MEAN_NOISY_SUCCESS_RATE] = L > 1 ? sum_noisy / (double)(L - 1) : quiet_nan();
        rob[DXRL_PG_VAL_ROBUST_MAX_DEGRADATION] = max_deg;
        rob[DXRL_PG_VAL_ROBUST_MAX_DEGRADATION_PERCENTAGE] = max_pct;
        rob[DXRL_PG_VAL_ROBUST_WORST_MEAN_RETURN] = worst_return;
        const bool has_score = a.score_col >= 0;
        const double score = !has_score ? 0.0 : a.score_table ? rob[a.score_col] : out[a.score_col];
        val_header_rules(a.header, out, a.row, has_score, score, status, a.min_delta, a.patience);
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < DXRL_PG_VAL_COLS) a.val[a.row * DXRL_PG_VAL_COLS + i] = setc[0][i];
    if (i < L * DXRL_PG_VAL_LEVEL_COLS)  // lev's rows are contiguous: flat index l * LEVEL_COLS + column
        a.levels[a.row * L * DXRL_PG_VAL_LEVEL_COLS + i] = (&lev[0][0])[i];
    if (i < DXRL_PG_VAL_ROBUST_COLS) a.robust[a.row * DXRL_PG_VAL_ROBUST_COLS + i] = rob[i];
}

}  // namespace
}  // namespace dxrl

extern "C" int dxrl_pg_val_levels_partial_doubles(int32_t num_levels, int64_t num_objects,
                                                  int64_t episodes_per_object, int64_t* out) {
    using namespace dxrl;
    DXRL_REQUIRE(out, "null out");
    DXRL_REQUIRE(num_levels >= 1 && num_levels <= kMaxLevels, "num_levels %d outside [1, %d]", num_levels, kMaxLevels);
    DXRL_REQUIRE(num_objects >= 1 && episodes_per_object >= 1, "num_objects and episodes_per_object must be >= 1");
    DXRL_REQUIRE(num_objects <= INT32_MAX / episodes_per_object &&
                     num_levels * num_objects * episodes_per_object <= (int64_t)INT32_MAX,
                 "num_levels x num_objects x episodes_per_object exceeds INT32_MAX");
    *out = num_levels * val_partial_doubles(num_objects);
    return DXRL_OK;
}

extern "C" int dxrl_pg_val_levels_row(int32_t device, const dxrl_pg_val_levels_args* args, void* stream) {
    using namespace dxrl;
    DXRL_REQUIRE(args, "null args");
    const dxrl_pg_val_levels_args& a = *args;
    const int64_t G = a.num_objects, K = a.episodes_per_object, L = a.num_levels;
    DXRL_REQUIRE(L >= 1 && L <= kMaxLevels, "num_levels %d outside [1, %d]", a.num_levels, kMaxLevels);
    DXRL_REQUIRE(G >= 1 && K >= 1, "num_objects and episodes_per_object must be >= 1");
    DXRL_REQUIRE(G <= INT32_MAX / K && L * G * K <= (int64_t)INT32_MAX,
                 "num_levels x num_objects x episodes_per_object exceeds INT32_MAX");
    DXRL_REQUIRE(a.cap >= 1 && a.row >= 0 && a.row < a.cap, "row %lld lies outside the table (%lld rows)",
                 (long long)a.row, (long long)a.cap);
    DXRL_REQUIRE(a.score_table == 0 || a.score_table == 1, "score_table must be 0 (main row) or 1 (robust row), got %d",
                 a.score_table);
    const int score_cols = a.score_table ? (int)DXRL_PG_VAL_ROBUST_COLS : (int)DXRL_PG_VAL_IS_BEST;
    DXRL_REQUIRE(a.score_col < score_cols, "score_col %d out of range of table %d (< %d, or < 0 for none)", a.score_col,
                 a.score_table, score_cols);
    DXRL_REQUIRE(a.patience >= 0, "patience must be >= 0, got %d", a.patience);
    DXRL_REQUIRE(a.ep_return && a.ep_length && a.ep_success && a.ep_contacts && a.status,
                 "null episode records / status");
    DXRL_REQUIRE(a.partial && a.val && a.header, "null partial / val / header");
    DXRL_REQUIRE(a.levels && a.robust && a.level_noise, "null levels / robust / level_noise");
    DXRL_REQUIRE((a.params != nullptr) == (a.best_params != nullptr), "params and best_params go together");
    DXRL_REQUIRE(!a.params || a.num_params >= 1, "keep-best needs num_params >= 1");
    const int64_t stride = val_partial_doubles(G), blocks = val_grid(G, K);
    DXRL_REQUIRE(a.partial_doubles >= L * stride, "partial holds %lld doubles, needs %lld",
                 (long long)a.partial_doubles, (long long)(L * stride));
    const bool copy = a.score_col >= 0 && a.params;
    DeviceGuard g(device);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(k_pg_val_levels_reduce, dim3((unsigned)blocks, (unsigned)L), dim3(kValThreads), 0, st,
                       a.ep_return, a.ep_length, a.ep_success, a.ep_contacts, G, K, a.partial, stride);
    if (int rc = launch_check("k_pg_val_levels_reduce")) return rc;
    LevelsFinishArgs f{a, stride, (int32_t)blocks};
    hipLaunchKernelGGL(k_pg_val_levels_finish, dim3(1), dim3((unsigned)(L * kWave)), 0, st, f);
    if (int rc = launch_check("k_pg_val_levels_finish")) return rc;
    if (copy) {
        if (int rc = launch_keep_best(st, a.val + a.row * DXRL_PG_VAL_COLS + DXRL_PG_VAL_IS_BEST, a.params,
                                      a.best_params, a.num_params))
            return rc;
    }
    return DXRL_OK;
}
