// dxrl_eval_row.h -- the lane-split episode program of the evaluation kernels, once.
//
// k_eval_ls (dxrl_eval.hip) and k_eval_mlp (dxrl_eval_mlp.hip) give a row of 16 lanes to each env
// (the rollout's layout: lane s owns joint s / action s, lanes 0..2 the object axes, the per-row
// sums and minima exchanged by row broadcasts) and 16 rows to each workgroup, and feed the rows
// from the caller's work-queue counter: a row takes the next program lane whenever its current
// one ends, so no row idles behind a long episode.  EvalRow is a row's place in that program and
// its transitions, one per member: take a lane, begin a segment, begin an episode, step the env,
// end the episode, finish the lane.  Each member moves `phase` one state along and leaves the
// loop around it to the kernel: k_eval_ls runs the transitions back to back and draws the
// reference policies' actions; k_eval_mlp takes one transition per pass of its part A, with the
// observation hand-off to the MFMA tile (kEmit) and the workgroup barriers between them.
//
// The members hold no workgroup barrier and touch no LDS; they exchange values through the
// row's DPP broadcasts only (row_bcast, row_contacts, row_object, row_neg_sum_fingers), so the 16
// lanes of a row must call them in uniform control flow.  An EvalRow lives in registers: it is
// passed by reference to forced-inline code only and no member is indexed at run time.
//
// Below the struct: the argument checks, the EvalParams construction and the queue reset / grid
// sizing that dxrl_evaluate and dxrl_evaluate_mlp have in common.
#pragma once
#include "dxrl_eval.h"

namespace dxrl {

// A row's place in its program.  kStep: an episode is running; kDone: the queue is empty.  kEmit
// (the pending observation) is k_eval_mlp's own.
enum EvalPhase { kNeedLane, kNeedSeg, kNeedEp, kEmit, kEndEp, kFinish, kStep, kDone };

// lane s's N(0, 1) of a step that takes kD normals from a Philox stream: four per block, the
// blocks addressed by their position in the stream (k_eval's order of draws)
__device__ __forceinline__ float row_step_normal(uint64_t& ctr, uint32_t tag, uint32_t k0, uint32_t k1, int sa) {
    const uint64_t c = ctr + (uint64_t)(sa >> 2);
    const u32x4 r = philox(u32x4{(uint32_t)c, (uint32_t)(c >> 32), tag, 0u}, k0, k1);
    float n0, n1;
    const bool hi = (sa & 2) != 0;
    box_muller(hi ? r.z : r.x, hi ? r.w : r.y, n0, n1);
    ctr += (kD + 3) / 4;
    return (sa & 1) ? n1 : n0;
}

struct EvalRow {
    int s, sa, s2, gbit;  // lane of the row, its action / reset-extra slot (0 beyond), the row's bit offset
    bool ntape;
    int phase = kNeedLane;
    int lane = 0, si = 0, s1 = 0, ep = 0, step = 0;
    bool ok = true;
    // policy stream (tape cursor or Philox counter) and noise stream of the current segment
    int64_t pcur = 0, ncur = 0, navail = 0;
    uint64_t pctr = 0, nctr = 0;
    bool pok = true, nok = true;
    uint32_t pk0 = 0, pk1 = 0, nk0 = 0, nk1 = 0;
    const double* ptape = nullptr;
    const double* ntp = nullptr;
    double dyn_sigma = 0.0, obs_sigma = 0.0;
    bool obs_noise = false, dyn_noise = false;
    int first_ep = 0, n_eps = 0, cfg = 0;
    double lo2 = 0.0, hi2 = 0.0, cst2 = 0.0;
    bool has2 = true, fric64 = false;
    // env (lane-split)
    float jp = 0.0f, jv = 0.0f, ovd = 0.0f;
    double opd = 0.0, size = 0.0;
    double fric = 0.0;
    uint32_t flags = 0;
    int32_t et = 0;
    int64_t rec = 0;
    float *otraj = nullptr, *atraj = nullptr;
    uint8_t* hist = nullptr;
    HistAcc hm{0u, 0u};
    double ret = 0.0;
    bool te = false;
    uint32_t nc = 0;
    int steps = 0;

    __device__ __forceinline__ EvalRow(const dxrl_eval_args& a, int tid)
        : s(tid & 15), sa(s < kD ? s : 0), s2(s < DXRL_RESET_EXTRA ? s : 0), gbit(16 * ((tid & 63) >> 4)),
          ntape(a.noise_tape != nullptr) {}

    // kNeedLane: the next lane of the queue and its policy stream (tape row or Philox key; `key`
    // maps a lane / segment / record index to the index its device streams are keyed by), or kDone
    template <class Key>
    __device__ __forceinline__ void take_lane(const dxrl_eval_args& a, int32_t* queue, bool tape, bool device,
                                              const Key& key) {
        int L = 0;
        if (s == 0) L = atomicAdd(queue, 1);
        lane = (int)row_bcast_u32<0>((uint32_t)L);
        if (lane >= a.num_lanes) {
            phase = kDone;
            return;
        }
        ok = pok = true;
        pcur = 0;
        pctr = 0;
        if (tape) ptape = a.policy_tape + (int64_t)lane * a.policy_stride;
        if (device) env_key(a.policy_seed, key(lane), pk0, pk1);
        si = a.lane_segments[lane];
        s1 = a.lane_segments[lane + 1];
        phase = kNeedSeg;
    }
    // kFinish: the lane's end
    __device__ __forceinline__ void finish_lane(const dxrl_eval_args& a) {
        if (!pok) ok = false;
        if (s == 0) {
            if (a.policy_used) a.policy_used[lane] = (int32_t)pcur;
            if (!ok && a.status) atomicOr(a.status, 1);
        }
        phase = kNeedLane;
    }
    // kNeedSeg: the next segment of the lane (si), or the lane's end
    template <class Key>
    __device__ __forceinline__ void begin_segment(const dxrl_curriculum* __restrict__ curricula, const EvalParams& p,
                                                  const Key& key) {
        const dxrl_eval_args& a = p.a;
        if (!ok || si >= s1) {
            phase = kFinish;
            return;
        }
        const dxrl_eval_segment sg = a.segments[si];
        const bool noisy = sg.obs_noise_std > 0.0 || sg.dyn_noise_std > 0.0;
        if (sg.curriculum_row < 0 || sg.curriculum_row >= p.n_curricula || sg.first_episode < 0 ||
            (ntape && noisy && sg.noise_offset < 0)) {
            ok = false;
            phase = kFinish;
            return;
        }
        cfg = sg.curriculum_row;
        const dxrl_curriculum& cu = curricula[cfg];
        const double* rg = s2 == 0 ? cu.size_range
                                   : s2 == 1 ? cu.mass_range
                                             : s2 == 2 ? cu.friction_range
                                                       : s2 == 3 ? cu.spawn_x_range : s2 == 4 ? cu.spawn_y_range : cu.spawn_z_range;
        lo2 = rg[0];
        hi2 = rg[1];
        cst2 = s2 == 0 ? cu.object_size : s2 == 1 ? cu.object_mass : cu.friction_coefficient;
        has2 = s2 == 0 ? cu.has_size_range != 0 : s2 == 1 ? cu.has_mass_range != 0 : s2 == 2 ? cu.has_friction_range != 0 : true;
        fric64 = cu.friction_is_f64_scalar != 0;
        nok = true;
        // both cursors, whichever the mode uses: one store to "the tape's or the stream's" cursor
        // would be a member picked at run time and keep the row's state out of registers
        ncur = 0;
        nctr = 0;
        if (ntape) {
            ntp = a.noise_tape + sg.noise_offset;
            navail = sg.noise_count;
        } else {
            env_key(a.noise_seed, key(si), nk0, nk1);
        }
        obs_noise = sg.obs_noise_std > 0.0;
        dyn_noise = sg.dyn_noise_std > 0.0;
        dyn_sigma = sg.dyn_noise_std;
        obs_sigma = sg.obs_noise_std;
        first_ep = sg.first_episode;
        n_eps = sg.num_episodes;
        // DexterousManipulationEnv(curriculum_config=row) (EV:94-98, RT:266-270)
        jp = jv = 0.0f;
        opd = s < 3 ? p.obj[s] : 0.0;
        ovd = 0.0f;
        flags = p.has_object ? kHasObject : 0u;
        et = 0;
        ep = 0;
        phase = kNeedEp;
    }
    // The wrapper's observation-noise draws (RT:193-207) of the observation at hand: the noise-tape
    // cursor moves past them; noff = their position, have = the tape holds them.
    __device__ __forceinline__ void take_obs_noise(int64_t& noff, bool& have) {
        noff = 0;
        have = true;
        if (ntape && obs_noise) {
            have = ncur + kObs <= navail;
            if (!have) nok = false;
            noff = ncur;
            ncur += kObs;
        }
    }
    // kNeedEp: the next episode of the segment (ep) reset and in kStep, or the segment's end
    // (kNeedSeg), or a record out of range (kFinish).  noff / have: take_obs_noise of the reset
    // observation.
    template <class Key>
    __device__ __forceinline__ void begin_episode(const dxrl_eval_args& a, const Key& key, int64_t& noff, bool& have) {
        if (ep >= n_eps) {  // end of the segment
            if (!nok) ok = false;
            ++si;
            phase = kNeedSeg;
            return;
        }
        rec = (int64_t)first_ep + ep;
        if (rec >= a.total_episodes) {
            ok = false;
            phase = kFinish;
            return;
        }
        // env.reset(seed=episode_seed) (EV:127, RT:281) [+ wrapper obs noise, RT:193-197]
        take_obs_noise(noff, have);
        double u1, v2;
        if (a.reset_tape) {
            u1 = a.reset_tape[rec * kReset + sa];
            v2 = has2 ? a.reset_tape[rec * kReset + kD + s2] : cst2;
        } else {
            uint32_t rk0, rk1;
            env_key(a.reset_seed, key(rec), rk0, rk1);
            u1 = joint_reset_draw(reset_uniform_at(sa, rk0, rk1, 0));
            v2 = has2 ? uniform_draw(lo2, hi2, reset_uniform_at(kD + s2, rk0, rk1, 0)) : cst2;
        }
        jp = s < kD ? (float)u1 : 0.0f;  // ME:143-145 .astype(float32)
        jv = 0.0f;
        size = row_bcast<0>(v2);
        fric = row_bcast<2>(v2);
        const double sx = row_bcast<3>(v2), sy = row_bcast<4>(v2), sz = row_bcast<5>(v2);
        const double spawn = s == 1 ? sy : (s == 2 ? sz : sx);
        const bool has = (flags & kHasObject) != 0;
        if (s < 3) object_axis_reset(opd, ovd, has, spawn);
        et = 0;
        flags = flags_after_reset(fric64);
        double op3[3], dmin;
        float g3[3];
        row_object(opd, op3);
        flags |= row_contacts<false>(jp, op3, size, s, gbit, dmin, g3);  // ME:176 (no dmin)
        otraj = a.obs_traj ? a.obs_traj + rec * (int64_t)(a.max_steps + 1) * kObs : nullptr;
        atraj = a.act_traj ? a.act_traj + rec * (int64_t)a.max_steps * kD : nullptr;
        hist = a.contact_hist ? a.contact_hist + rec * a.max_steps : nullptr;
        hm = HistAcc{0u, 0u};
        ret = 0.0;
        te = false;
        nc = 0;
        steps = 0;
        step = 0;
        phase = kStep;
    }
    // the observation (ME:254-264): lane s's elements of the 45 (row_obs_elem's map)
    __device__ __forceinline__ void write_obs(float* o) const {
        if (s < kD) {
            o[s] = jp;
            o[kD + s] = jv;
        }
        if (s < 3) {
            o[2 * kD + s] = (float)opd;
            o[2 * kD + 7 + s] = ovd;
        } else if (s < 7) {
            o[2 * kD + s] = s == 3 ? 1.0f : 0.0f;
        } else if (s < 7 + kF) {
            o[2 * kD + 10 + (s - 7)] = (float)((flags >> (s - 7)) & 1u);
        }
    }
    // the wrapper's dynamics noise on lane s's action (a noise tape that has run out adds nothing)
    __device__ __forceinline__ float dynamics_noise(float act) {
        if (dyn_noise) {  // RT:180-187: clip(a + f32(N(0, s)), low, high)
            float dz = 0.0f;
            if (ntape) {
                if (ncur + kD > navail) {
                    nok = false;
                } else {
                    dz = (float)(0.0 + dyn_sigma * ntp[ncur + sa]);
                    ncur += kD;
                }
            } else {
                dz = (float)dyn_sigma * row_step_normal(nctr, kStreamEvalNoise, nk0, nk1, sa);
            }
            act = clipf(act + dz, -1.0f, 1.0f);
        }
        return act;
    }
    // kStep: env_step, lane-split (ME:198-252), with the episode's return, length, contacts,
    // history byte and moments.  Returns terminated || truncated and leaves `step`, the step limit
    // and the phase to the caller; noff / have: take_obs_noise of the observation the step returns.
    __device__ __forceinline__ bool step_env(const EvalParams& p, float act, int64_t& noff, bool& have) {
        if (s < kD) joint_step(jp, jv, act);
        const AxisState ax = object_axis_step(opd, ovd, s < 3 ? s : 0, fric, flags);
        if (s < 3) {
            opd = ax.q;
            ovd = ax.v;
        }
        flags &= ~kOpIsF32;
        double op3[3], dmin;
        float g3[3];
        row_object(opd, op3);
        const uint32_t c = row_contacts(jp, op3, size, s, gbit, dmin, g3);
        double r;
        if (p.dense) {
            float sum = 0.0f;
            row_neg_sum_fingers(negative_sum(g3), sum);  // finger f's on lane 3 f
            double comp[4];
            r = dense_reward_of(dmin, c, prev_contacts(flags), sum, p.w, comp);
            flags = flags_with_prev_contacts(flags, c);
        } else {
            r = sparse_reward(c);
        }
        flags = flags_with_contacts(flags, c);
        te = __popc(c) >= 3;                        // ME:332-336
        const bool tr = et >= p.max_episode_steps;  // ME:245 (before the increment)
        et += 1;
        take_obs_noise(noff, have);
        ret += r;  // EV:143 / RT:291 episode_reward += reward
        steps = step + 1;
        nc = (uint32_t)__popc(c);
        if (hist && s == 0) hist[step] = (uint8_t)nc;
        hist_acc_step(hm, nc, step);
        return te || tr;
    }
    // kEndEp: the episode's records
    __device__ __forceinline__ void end_episode(const dxrl_eval_args& a) {
        if (s == 0) {
            a.ep_return[rec] = ret;
            a.ep_length[rec] = steps;
            a.ep_success[rec] = (uint8_t)te;  // success = terminated (EV:157, RT:303)
            if (a.ep_contacts) a.ep_contacts[rec] = (uint8_t)nc;
            if (a.hist_moments) hist_acc_store(hm, a.hist_moments + 5 * rec);
        }
        ++ep;
        phase = kNeedEp;
    }
};

}  // namespace dxrl

// ------------------------------------------------------------------ host side of both entry points
// The argument rules dxrl_evaluate and dxrl_evaluate_mlp share, in the order both make them.  Each
// entry point has rules of its own between these, so it runs them as ranges [first, last].
enum { kEvalChkLanes, kEvalChkSteps, kEvalChkSegments, kEvalChkRecords, kEvalChkMoments, kEvalChkStride, kEvalChkQueue };
static int eval_check_args(const dxrl_env* env, const dxrl_eval_args& a, int first, int last) {
    const auto on = [&](int k) { return first <= k && k <= last; };
    DXRL_REQUIRE(!on(kEvalChkLanes) || (a.num_lanes > 0 && a.num_lanes <= env->cfg.num_envs),
                 "num_lanes must be in [1, num_envs]");
    DXRL_REQUIRE(!on(kEvalChkSteps) || (a.max_steps > 0 && a.total_episodes >= 0),
                 "max_steps must be > 0, total_episodes >= 0");
    DXRL_REQUIRE(!on(kEvalChkSegments) || (a.lane_segments && a.segments), "null segment table");
    DXRL_REQUIRE(!on(kEvalChkRecords) || (a.ep_return && a.ep_length && a.ep_success), "null episode record buffers");
    DXRL_REQUIRE(!on(kEvalChkMoments) || !a.hist_moments || a.max_steps <= dxrl::kHistMomentsMaxSteps,
                 "hist_moments packs its sums for max_steps <= %d, got %d", dxrl::kHistMomentsMaxSteps, a.max_steps);
    DXRL_REQUIRE(!on(kEvalChkStride) || !a.policy_tape || a.policy_stride >= 0, "bad policy tape stride");
    DXRL_REQUIRE(!on(kEvalChkQueue) || a.work_queue, "null work_queue (device i32[1] scratch of this launch)");
    return DXRL_OK;
}

static dxrl::EvalParams eval_params(const dxrl_env* env, const dxrl_eval_args& a) {
    return dxrl::EvalParams{dxrl::weights_of(env->cfg),
                            env->cfg.max_episode_steps,
                            env->cfg.reward_type == DXRL_REWARD_DENSE,
                            env->cfg.has_object_position,
                            env->n_curricula,
                            {env->cfg.object_position[0], env->cfg.object_position[1], env->cfg.object_position[2]},
                            a,
                            nullptr};
}

// The work-queue counter is the caller's scratch (a.work_queue), zeroed on the launch stream: no
// state shared between launches, so evaluations on different streams / handles / threads cannot
// reset each other's queue.  blocks = min(ceil(lanes / 16), per_cu x CUs) workgroups of 16 rows.
static int eval_queue_grid(const dxrl_eval_args& a, int dev, int per_cu, hipStream_t st, int64_t& blocks) {
    if (int rc = dxrl::hip_check(hipMemsetAsync(a.work_queue, 0, sizeof(int32_t), st), "eval queue reset")) return rc;
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    blocks = (a.num_lanes + dxrl::kEvalRows - 1) / dxrl::kEvalRows;
    const int64_t resident = (int64_t)(per_cu > 0 ? per_cu : 2) * (cus > 0 ? cus : 256);
    if (blocks > resident) blocks = resident;
    return DXRL_OK;
}
