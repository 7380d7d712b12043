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
//                       the device); dxrl_keep_best.h, the training log's copy too.
// A single-workgroup path that folds reduce and finish into one launch for small E was not built:
// it would save one dependent launch (about 5 us) behind an episode kernel of a millisecond.
// No floating-point atomics, no tickets, no spin-waits: the launch order is the only ordering.
// The workgroup and wave bodies live in dxrl_pg_val_common.h, shared with the noise-level form of
// this call (dxrl_pg_val_levels.hip), which runs them once per level.
#include "dxrl_pg_val_common.h"

namespace dxrl {
namespace {

template <bool VEC>
__global__ __launch_bounds__(kValThreads) void k_pg_val_reduce(
    const double* __restrict__ ep_return, const int32_t* __restrict__ ep_length,
    const uint8_t* __restrict__ ep_success, const uint8_t* __restrict__ ep_contacts, int64_t E, int64_t G, int64_t K,
    double* __restrict__ partial, int32_t* __restrict__ counts) {
    __shared__ double wred[kValWaves][kValPartial];
    val_reduce_block<VEC>(ep_return, ep_length, ep_success, ep_contacts, E, G, K, (int64_t)blockIdx.x,
                          (int64_t)gridDim.x, partial, counts, wred);
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
    const ValSetStats t = val_finish_set(a.partial, f.blocks, G, K, a.solve_threshold,
                                         a.object_successes ? a.object_successes + a.row * G : nullptr, lane);
    if (lane == 0) {
        const int32_t status = *a.status;
        val_set_columns(out, t, G, K, a.ep_return[0]);
        out[DXRL_PG_VAL_ITERATION] = (double)a.iteration;
        out[DXRL_PG_VAL_ENV_STEPS] = (double)a.env_steps;
        out[DXRL_PG_VAL_TRAIN_ROW] = (double)a.train_row;
        out[DXRL_PG_VAL_EVAL_STATUS] = (double)status;
        val_header_rules(a.header, out, a.row, a.score_col >= 0, a.score_col >= 0 ? out[a.score_col] : 0.0, status,
                         a.min_delta, a.patience);
    }
    __syncthreads();
    if (lane < DXRL_PG_VAL_COLS) a.val[a.row * DXRL_PG_VAL_COLS + lane] = out[lane];
}

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
        if (int rc = launch_keep_best(st, a.val + a.row * DXRL_PG_VAL_COLS + DXRL_PG_VAL_IS_BEST, a.params,
                                      a.best_params, a.num_params))
            return rc;
    }
    return DXRL_OK;
}
