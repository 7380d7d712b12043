// dxrl_eval.hip -- evaluation episode programs.
//
// Replaces the per-episode Python loops of
//   evaluation/evaluator.py:71-181        Evaluator.evaluate_episode (EV)
//   evaluation/evaluator.py:183-262       Evaluator.evaluate_heldout_set
//   evaluation/robustness_tests.py:240-310 RobustnessTester.evaluate_with_noise (RT)
//   evaluation/robustness_tests.py:312-407 RobustnessTester.run_robustness_sweep
// One lane = one chain of segments (fresh env instances, see include/dxrl.h);
// the env state, the frozen policy and both random streams live in registers
// for the whole chain.  Records go out once per episode; the optional
// per-step contact history is one byte per step.
// k_eval is the one-lane-per-chain kernel (DXRL_EVAL_ONE_LANE, the tests' A/B partner) with its
// own whole-row Stream / policy_terms / dyn_terms; k_eval_ls, the default, drives the lane-split
// episode program of dxrl_eval_row.h (shared with k_eval_mlp) with the three frozen policies.
#include "dxrl_eval_row.h"

#include <stdio.h>
#include <stdlib.h>

using namespace dxrl;

namespace dxrl {

// Draw-by-draw reader over a tape row or a Philox stream.  Philox blocks are
// consumed four u32 at a time: two 53-bit uniforms, or four f32 normals.
struct Stream {
    const double* tape;
    int64_t avail;
    int64_t cur;
    uint32_t k0, k1, tag;
    uint64_t ctr;
    bool ok;

    __device__ __forceinline__ u32x4 block() {
        const u32x4 r = philox(u32x4{(uint32_t)ctr, (uint32_t)(ctr >> 32), tag, 0u}, k0, k1);
        ++ctr;
        return r;
    }
    // n raw draws from the tape (cursor advances; false once the tape is exhausted)
    __device__ __forceinline__ bool take(double* out, int n) {
        if (cur + n > avail) {
            ok = false;
            return false;
        }
        for (int k = 0; k < n; ++k) out[k] = tape[cur + k];
        cur += n;
        return true;
    }
    __device__ __forceinline__ void skip(int n) {
        if (cur + n > avail) ok = false;
        cur += n;
    }
};

// f32 noise terms of one policy step (kD values) in the policy's own arithmetic.
template <bool kTape>
__device__ __forceinline__ bool policy_terms(int policy, double sigma, Stream& s, float* nz) {
    if (kTape) {
        double g[kD];
        if (!s.take(g, kD)) return false;
#pragma unroll
        for (int k = 0; k < kD; ++k) {
            if (policy == DXRL_EVAL_POLICY_SIMPLE)
                nz[k] = (float)(0.0 + sigma * g[k]);          // np.random.normal(0, s) (SL:60)
            else if (policy == DXRL_EVAL_POLICY_HEURISTIC)
                nz[k] = (float)(-0.1 + (0.1 - -0.1) * g[k]);  // np.random.uniform(-0.1, 0.1)
            else
                nz[k] = (float)(-1.0 + (1.0 - -1.0) * g[k]);  // Box.sample: uniform(low, high)
        }
        return true;
    }
    if (policy == DXRL_EVAL_POLICY_SIMPLE) {
        const float fs = (float)sigma;
#pragma unroll
        for (int b = 0; b < (kD + 3) / 4; ++b) {
            const u32x4 r = s.block();
            float n[4];
            box_muller(r.x, r.y, n[0], n[1]);
            box_muller(r.z, r.w, n[2], n[3]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (4 * b + q < kD) nz[4 * b + q] = fs * n[q];
        }
    } else {
        const double lo = policy == DXRL_EVAL_POLICY_HEURISTIC ? -0.1 : -1.0;
#pragma unroll
        for (int b = 0; b < (kD + 1) / 2; ++b) {
            const u32x4 r = s.block();
            nz[2 * b] = (float)(lo + (-lo - lo) * u01_53(r.x, r.y));
            if (2 * b + 1 < kD) nz[2 * b + 1] = (float)(lo + (-lo - lo) * u01_53(r.z, r.w));
        }
    }
    return true;
}

// Dynamics noise of one wrapper step: f32(0 + s g) per joint (RT:180-187).
__device__ __forceinline__ void dyn_terms(bool tape, double sigma, Stream& s, float* nz) {
    if (tape) {
        double g[kD];
        if (!s.take(g, kD)) {
#pragma unroll
            for (int k = 0; k < kD; ++k) nz[k] = 0.0f;
            return;
        }
#pragma unroll
        for (int k = 0; k < kD; ++k) nz[k] = (float)(0.0 + sigma * g[k]);
        return;
    }
    const float fs = (float)sigma;
#pragma unroll
    for (int b = 0; b < (kD + 3) / 4; ++b) {
        const u32x4 r = s.block();
        float n[4];
        box_muller(r.x, r.y, n[0], n[1]);
        box_muller(r.z, r.w, n[2], n[3]);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (4 * b + q < kD) nz[4 * b + q] = fs * n[q];
    }
}

template <bool kTape>
__global__ __launch_bounds__(64) void k_eval(const dxrl_curriculum* __restrict__ curricula, EvalParams p) {
    const dxrl_eval_args& a = p.a;
    const int lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= a.num_lanes) return;
    Stream ps{};
    ps.ok = true;
    if (kTape) {
        ps.tape = a.policy_tape + (int64_t)lane * a.policy_stride;
        ps.avail = a.policy_stride;
    } else {
        env_key(a.policy_seed, lane, ps.k0, ps.k1);
        ps.tag = kStreamPolicy;
    }
    float mean[kD];
#pragma unroll
    for (int k = 0; k < kD; ++k) mean[k] = a.mean_action ? a.mean_action[(int64_t)lane * kD + k] : 0.0f;
    const int s0 = a.lane_segments[lane], s1 = a.lane_segments[lane + 1];
    const bool ntape = a.noise_tape != nullptr;
    bool ok = true;
    for (int si = s0; si < s1 && ok; ++si) {
        const dxrl_eval_segment sg = a.segments[si];
        const bool noisy = sg.obs_noise_std > 0.0 || sg.dyn_noise_std > 0.0;
        if (sg.curriculum_row < 0 || sg.curriculum_row >= p.n_curricula || sg.first_episode < 0 ||
            (ntape && noisy && sg.noise_offset < 0)) {
            ok = false;
            break;
        }
        const dxrl_curriculum cu = curricula[sg.curriculum_row];
        Stream ns{};
        ns.ok = true;
        if (ntape) {
            ns.tape = a.noise_tape + sg.noise_offset;
            ns.avail = sg.noise_count;
        } else {
            env_key(a.noise_seed, si, ns.k0, ns.k1);
            ns.tag = kStreamEvalNoise;
        }
        const bool obs_noise = sg.obs_noise_std > 0.0, dyn_noise = sg.dyn_noise_std > 0.0;
        // DexterousManipulationEnv(curriculum_config=row) (EV:94-98, RT:266-270)
        Env e;
#pragma unroll
        for (int k = 0; k < kD; ++k) e.jp[k] = e.jv[k] = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            e.op[i] = p.obj[i];
            e.ov[i] = 0.0f;
        }
        e.flags = p.has_object ? kHasObject : 0u;
        e.t = 0;
        e.cfg = sg.curriculum_row;
        for (int ep = 0; ep < sg.num_episodes && ok; ++ep) {
            const int64_t rec = (int64_t)sg.first_episode + ep;
            if (rec >= a.total_episodes) {
                ok = false;
                break;
            }
            // env.reset(seed=episode_seed) (EV:127, RT:281) [+ wrapper obs noise, RT:193-197]
            if (ntape && obs_noise) ns.skip(kObs);
            if (a.reset_tape) {
                double d[kReset];
#pragma unroll
                for (int k = 0; k < kReset; ++k) d[k] = a.reset_tape[rec * kReset + k];
                env_reset(e, d, cu);
            } else {
                uint32_t rk0, rk1;
                env_key(a.reset_seed, rec, rk0, rk1);
                env_reset_philox(e, cu, rk0, rk1, 0);
            }
            float* otraj = a.obs_traj ? a.obs_traj + rec * (int64_t)(a.max_steps + 1) * kObs : nullptr;
            float* atraj = a.act_traj ? a.act_traj + rec * (int64_t)a.max_steps * kD : nullptr;
            if (otraj) write_obs(e, otraj);
            double ret = 0.0;
            bool te = false, tr = false;
            uint32_t nc = 0;
            int steps = 0;
            uint8_t* hist = a.contact_hist ? a.contact_hist + rec * a.max_steps : nullptr;
            HistAcc hm{0u, 0u};
            for (int step = 0; step < a.max_steps; ++step) {
                float nz[kD], act[kD];
                if (!policy_terms<kTape>(a.policy, a.exploration_noise, ps, nz)) {
                    ok = false;
                    break;
                }
#pragma unroll
                for (int k = 0; k < kD; ++k)
                    act[k] = a.policy == DXRL_EVAL_POLICY_SIMPLE      ? clipf(mean[k] + nz[k], -1.0f, 1.0f)
                             : a.policy == DXRL_EVAL_POLICY_HEURISTIC ? clipf(-0.5f + nz[k], -1.0f, 1.0f)
                                                                      : nz[k];
                if (atraj) {
#pragma unroll
                    for (int k = 0; k < kD; ++k) atraj[step * kD + k] = act[k];
                }
                if (dyn_noise) {  // RT:180-187: clip(a + f32(N(0, s)), low, high)
                    float dz[kD];
                    dyn_terms(ntape, sg.dyn_noise_std, ns, dz);
#pragma unroll
                    for (int k = 0; k < kD; ++k) act[k] = clipf(act[k] + dz[k], -1.0f, 1.0f);
                }
                double cp[4];
                const double r = env_step(e, act, p.dense != 0, p.w, p.max_episode_steps, te, tr, cp);
                if (ntape && obs_noise) ns.skip(kObs);
                ret += r;  // EV:143 / RT:291 episode_reward += reward
                steps = step + 1;
                nc = (uint32_t)__popc(e.flags & 0x1Fu);
                if (hist) hist[step] = (uint8_t)nc;
                hist_acc_step(hm, nc, step);
                if (otraj) write_obs(e, otraj + (int64_t)(step + 1) * kObs);
                if (te || tr) break;
            }
            if (!ok) break;
            a.ep_return[rec] = ret;
            a.ep_length[rec] = steps;
            a.ep_success[rec] = (uint8_t)te;  // success = terminated (EV:157, RT:303)
            if (a.ep_contacts) a.ep_contacts[rec] = (uint8_t)nc;
            if (a.hist_moments) hist_acc_store(hm, a.hist_moments + 5 * rec);
        }
        if (!ns.ok) ok = false;
    }
    if (!ps.ok) ok = false;
    if (a.policy_used) a.policy_used[lane] = (int32_t)ps.cur;
    if (!ok && a.status) atomicOr(a.status, 1);
}


// ------------------------------------------------------------------ lane-split programs
// k_eval_ls: the same episode programs on EvalRow (dxrl_eval_row.h: each env spread over the 16
// lanes of a DPP row, the rows fed from a work queue).  The kernel adds the three frozen policies'
// draws and the loop: a row runs its transitions back to back until an episode is stepping, then
// one step per iteration.  Every draw is the one k_eval takes (tape cursors advance by the step's
// draw count; Philox blocks are addressed by their position in the lane's stream), so records,
// histories, trajectories and tape consumption are identical
// (test_lane_split_eval_matches_one_lane_kernel).

template <bool kTape>
__global__ __launch_bounds__(kEvalThreads) void k_eval_ls(const dxrl_curriculum* __restrict__ curricula,
                                                         EvalParams p, int32_t* __restrict__ queue) {
    const dxrl_eval_args& a = p.a;
    const bool simple = a.policy == DXRL_EVAL_POLICY_SIMPLE, heur = a.policy == DXRL_EVAL_POLICY_HEURISTIC;
    const auto key = [](int64_t i) { return i; };  // device streams are keyed by lane, segment and record index
    EvalRow r(a, threadIdx.x);
    const int s = r.s, sa = r.sa;
    float mean = 0.0f;
    uint32_t iters = 0;  // step iterations this lane executed (diagnostics)
    int64_t noff;        // the observation-noise draws: only the cursor moves (the un-noised observation is recorded)
    bool have;
    while (true) {
        while (r.phase != kStep && r.phase != kDone) {
            if (r.phase == kNeedLane) {
                r.take_lane(a, queue, kTape, !kTape, key);
                if (r.phase != kDone) mean = a.mean_action ? a.mean_action[(int64_t)r.lane * kD + sa] : 0.0f;
            } else if (r.phase == kNeedSeg) {
                r.begin_segment(curricula, p, key);
            } else if (r.phase == kNeedEp) {
                r.begin_episode(a, key, noff, have);
                if (r.phase == kStep && r.otraj) r.write_obs(r.otraj);
            } else if (r.phase == kEndEp) {
                r.end_episode(a);
            } else {
                r.finish_lane(a);
            }
        }
        if (r.phase == kDone) break;
        ++iters;
        // ---- the policy's action (one frozen-policy step; policy_terms' draws, lane s: dim s)
        float nz;
        if (kTape) {
            if (r.pcur + kD > a.policy_stride) {
                r.pok = false;
                r.phase = kFinish;
                continue;
            }
            const double g = r.ptape[r.pcur + sa];
            r.pcur += kD;
            nz = simple ? (float)(0.0 + a.exploration_noise * g)       // np.random.normal(0, s) (SL:60)
                 : heur ? (float)(-0.1 + (0.1 - -0.1) * g)            // np.random.uniform(-0.1, 0.1)
                        : (float)(-1.0 + (1.0 - -1.0) * g);           // Box.sample: uniform(low, high)
        } else if (simple) {
            nz = (float)a.exploration_noise * row_step_normal(r.pctr, kStreamPolicy, r.pk0, r.pk1, sa);
        } else {
            const double lo = heur ? -0.1 : -1.0;
            const uint64_t c = r.pctr + (uint64_t)(sa >> 1);
            const u32x4 u = philox(u32x4{(uint32_t)c, (uint32_t)(c >> 32), kStreamPolicy, 0u}, r.pk0, r.pk1);
            nz = (float)(lo + (-lo - lo) * ((sa & 1) ? u01_53(u.z, u.w) : u01_53(u.x, u.y)));
            r.pctr += (kD + 1) / 2;
        }
        float act = simple ? clipf(mean + nz, -1.0f, 1.0f) : heur ? clipf(-0.5f + nz, -1.0f, 1.0f) : nz;
        if (r.atraj && s < kD) r.atraj[r.step * kD + s] = act;
        const bool over = r.step_env(p, r.dynamics_noise(act), noff, have);
        if (r.otraj) r.write_obs(r.otraj + (int64_t)(r.step + 1) * kObs);
        ++r.step;
        if (over || r.step >= a.max_steps) r.phase = kEndEp;
    }
    if (p.diag_iters) {  // the wave ran as many iterations as its busiest lane: 4 env-step slots each
        uint32_t m = iters;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
        if ((threadIdx.x & 63) == 0) atomicAdd(p.diag_iters, (unsigned long long)m);
    }
}

}  // namespace dxrl

extern "C" int dxrl_evaluate(dxrl_env* env, const dxrl_eval_args* args, void* stream) {
    DXRL_REQUIRE(env && args, "null env / args");
    const dxrl_eval_args& a = *args;
    if (int rc = eval_check_args(env, a, kEvalChkLanes, kEvalChkLanes)) return rc;
    DXRL_REQUIRE(a.policy >= DXRL_EVAL_POLICY_SIMPLE && a.policy <= DXRL_EVAL_POLICY_RANDOM, "unknown policy %d",
                 a.policy);
    if (int rc = eval_check_args(env, a, kEvalChkSteps, kEvalChkStride)) return rc;
    const bool tape = a.policy_tape != nullptr;
    DXRL_REQUIRE(a.stream_period == 0, "stream_period is built for dxrl_evaluate_mlp only, got %lld",
                 (long long)a.stream_period);
    EvalParams p = eval_params(env, a);
    DeviceGuard g(env->device);
    hipStream_t st = as_stream(stream);
    const char* one_env = getenv("DXRL_EVAL_ONE_LANE");  // A/B: the one-lane-per-chain kernel
    const bool one_lane = one_env && atoi(one_env) != 0;
    if (one_lane) {
        const dim3 grid((unsigned)((a.num_lanes + 63) / 64)), block(64);
        if (tape)
            hipLaunchKernelGGL(k_eval<true>, grid, block, 0, st, env->curricula, p);
        else
            hipLaunchKernelGGL(k_eval<false>, grid, block, 0, st, env->curricula, p);
        return launch_check("k_eval");
    }
    // k_eval_ls: rows of 16 lanes over the launch's work queue
    if (int rc = eval_check_args(env, a, kEvalChkQueue, kEvalChkQueue)) return rc;
    const int dev = env->device;
    DXRL_REQUIRE(dev >= 0 && dev < 64, "device index out of range");
    const void* fn = tape ? reinterpret_cast<const void*>(k_eval_ls<true>) : reinterpret_cast<const void*>(k_eval_ls<false>);
    int per_cu = 0;
    (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kEvalThreads, 0);
    // One workgroup (16 rows) per CU by default: with more rows than that the queue runs dry
    // while the first long episodes are still running and most rows then idle in lockstep with
    // them (measured on 40,960 held-out episodes: wave efficiency 46 % -> 72 % on hard objects,
    // kernel time -26 %; 59 % -> 68 %, -5 % on the variable curriculum).  DXRL_EVAL_BPC: A/B.
    static const int bpc_env = [] {
        const char* v = getenv("DXRL_EVAL_BPC");
        return v ? atoi(v) : 1;
    }();
    if (bpc_env > 0 && (per_cu <= 0 || bpc_env < per_cu)) per_cu = bpc_env;
    int64_t blocks = 0;
    if (int rc = eval_queue_grid(a, dev, per_cu, st, blocks)) return rc;
    static unsigned long long* diag[64] = {nullptr};
    const char* dg = getenv("DXRL_EVAL_DIAG");
    if (dg && atoi(dg) != 0) {  // diagnostics: wave step iterations -> stderr after the launch
        if (!diag[dev]) (void)hipMalloc(&diag[dev], sizeof(unsigned long long));
        (void)hipMemsetAsync(diag[dev], 0, sizeof(unsigned long long), st);
        p.diag_iters = diag[dev];
    }
    if (tape)
        hipLaunchKernelGGL(k_eval_ls<true>, dim3((unsigned)blocks), dim3(kEvalThreads), 0, st, env->curricula, p,
                           a.work_queue);
    else
        hipLaunchKernelGGL(k_eval_ls<false>, dim3((unsigned)blocks), dim3(kEvalThreads), 0, st, env->curricula, p,
                           a.work_queue);
    if (int rc = launch_check("k_eval_ls")) return rc;
    if (p.diag_iters) {
        unsigned long long it = 0;
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(&it, p.diag_iters, sizeof(it), hipMemcpyDeviceToHost);
        fprintf(stderr, "k_eval_ls wave_iterations=%llu rows_per_wave=4 blocks=%lld per_cu=%d\n", it, (long long)blocks,
                per_cu);
    }
    return DXRL_OK;
}
