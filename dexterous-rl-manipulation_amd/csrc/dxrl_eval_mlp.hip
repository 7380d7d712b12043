// dxrl_eval_mlp.hip -- evaluation episode programs of the frozen MLP actor (DXRL_EVAL_POLICY_MLP).
//
// k_eval_mlp runs the episode programs of k_eval_ls (dxrl_eval.hip: a row of 16 lanes per env, 16
// rows per workgroup, rows fed from the caller's work-queue counter; same segments, episodes,
// reset and noise tapes, records, histories, trajectories, policy_used and status word) with the
// action of every step computed by PGTrainer's actor, obs(45) -> 256 -> 256 -> mu(15), from the
// observation the evaluation loop hands its policy (evaluator.py:136-141; inside
// CombinedNoiseWrapper the noisy one, robustness_tests.py:199-207).  The 16 rows of a workgroup
// are one M = 16 MFMA tile: the forward pass is the 16-env rollout's (dxrl_pg_mlp.h
// wave_layer16 on v_mfma_f32_16x16x32_bf16, same k order, tanh and bias arithmetic), so an
// evaluated actor computes the trained actor's mu bit for bit.
//
// Per workgroup step:  A  rows without a running episode take work (queue fetch, segment and
//                         episode set-up, reset observation) -- divergent per row, no barrier
//                      B1 barrier: X tile and the workgroup's "a row is stepping" word visible
//                         L1  H1 = tanh(X W1^T)        wave w: columns 64 w .. 64 w + 63
//                      B2 barrier
//                         L2  H2 = tanh(H1 W2^T + b2)   (W2 slab in registers)
//                      B3 barrier
//                         head mu = H2 W3^T + b3 (every wave, for its own 4 rows), action, dynamics
//                         noise, env step, records, the next observation row -- per row
// Weights: W1 [256][64] and W3 rows 0..15 stay in LDS for the launch; wave w keeps its 64-column
// slab of W2 (32 KiB, 128 VGPRs per lane) in registers as k_pg_rollout does; the layer-2 and head
// biases come from the f32 master.
#include "dxrl_eval.h"
#include "dxrl_pg.h"
#include "dxrl_pg_mlp.h"
#include "dxrl_pg_rollout.h"

using namespace dxrl;
using namespace dxrl::pg;

namespace dxrl {

struct EvalMlpWeights {
    const bf16* wbf;      // bf16 pack (dxrl_pg_pack_weights)
    const float* params;  // f32 master
    const float* std;     // f32 [15] or null (deterministic)
};

enum { kMlpDet = 0, kMlpTape = 1, kMlpDevice = 2 };  // the policy's draws: none, tape, Philox stream

constexpr int kEmW1p = kIn + 16, kEmW3p = kH + 16, kEmXp = kIn + 16;  // LDS pitches (bf16), as k_pg_rollout_ws
constexpr int kEmObsP = 48, kEmMuP = 17;                              // f32 staging row, mu row
constexpr uint32_t kEvalObsBlock = 1u;  // 4th Philox counter word of the observation-noise blocks (dynamics: 0)

// kPeriod: the launch has a stream period (dxrl_eval_args.stream_period > 0).  Without one the
// kernel is the code it was before the period existed.
template <int kMode, bool kPeriod = false>
__global__ __launch_bounds__(kEvalThreads, 1) void k_eval_mlp(const dxrl_curriculum* __restrict__ curricula,
                                                              EvalParams p, EvalMlpWeights w,
                                                              int32_t* __restrict__ queue) {
    __shared__ __attribute__((aligned(16))) bf16 W1s[kH * kEmW1p];
    __shared__ __attribute__((aligned(16))) bf16 W3s[kEvalRows * kEmW3p];
    __shared__ __attribute__((aligned(16))) bf16 X[kEvalRows * kEmXp];
    __shared__ __attribute__((aligned(16))) bf16 H1[kEvalRows * kH];
    __shared__ __attribute__((aligned(16))) bf16 H2[kEvalRows * kH];
    __shared__ __attribute__((aligned(16))) float OBSF[kEvalRows * kEmObsP];
    __shared__ float MU[kEvalRows * kEmMuP];
    __shared__ int ALIVE[2];
    const dxrl_eval_args& a = p.a;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = tid & 15, row = tid >> 4, gbit = 16 * ((tid & 63) >> 4);
    const int r16 = lane & 15, g16 = lane >> 4;  // 16x16x32 fragment row / k group (row == 4 wave + g16)
    const int sa = s < kD ? s : 0;
    const int s2 = s < DXRL_RESET_EXTRA ? s : 0;
    const bool ntape = a.noise_tape != nullptr;
    // stream period P > 0: the device streams of lane, segment and record i are keyed by i % P
    // (the entry point refuses the tapes then).  Taken once per lane, segment and episode in part A.
    // The three indices are i32 counts, so the entry point launches a period above INT32_MAX,
    // which leaves every index as it is, as no period, and the modulo is a 32-bit one.
    const uint32_t period = kPeriod ? (uint32_t)a.stream_period : 0u;
    const auto keyed = [&](int64_t i) __attribute__((always_inline)) {
        return kPeriod ? (int64_t)((uint32_t)i % period) : i;
    };

    // ---- weights, once per launch
    bf16x8 w2[4][kH / 32];  // this wave's L2 columns 64 wave .. + 63 as four 16-column tiles
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < kH / 32; ++k)
            w2[j][k] = *reinterpret_cast<const bf16x8*>(w.wbf + kBfW2a + (int64_t)(64 * wave + 16 * j + r16) * kHx +
                                                        32 * k + 8 * g16);
    for (int c = tid; c < kH * (kIn / 8); c += kEvalThreads) {
        const int r = c / (kIn / 8), col = 8 * (c % (kIn / 8));
        *reinterpret_cast<bf16x8*>(W1s + r * kEmW1p + col) =
            *reinterpret_cast<const bf16x8*>(w.wbf + kBfW1a + (int64_t)r * kIn + col);
    }
    for (int c = tid; c < kEvalRows * (kH / 8); c += kEvalThreads) {
        const int r = c / (kH / 8), col = 8 * (c % (kH / 8));
        *reinterpret_cast<bf16x8*>(W3s + r * kEmW3p + col) =
            *reinterpret_cast<const bf16x8*>(w.wbf + kBfW3a + (int64_t)r * kHx + col);
    }
    for (int c = tid; c < kEvalRows * kEmXp; c += kEvalThreads) X[c] = (bf16)0.0f;
    for (int c = tid; c < kEvalRows * kEmObsP; c += kEvalThreads) OBSF[c] = 0.0f;
    if (tid < 2) ALIVE[tid] = 0;
    const auto w1frag = [&](int j, int k) __attribute__((always_inline)) {
        return *reinterpret_cast<const bf16x8*>(W1s + (64 * wave + 16 * j + r16) * kEmW1p + 32 * k + 8 * g16);
    };
    const auto w2frag = [&](int j, int k) __attribute__((always_inline)) { return w2[j][k]; };
    float b2_reg[16];  // L2 bias of column 64 wave + 16 j + 4 g16 + q
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            b2_reg[4 * j + q] = w.params[kOffW2a + (int64_t)(64 * wave + 16 * j + 4 * g16 + q) * kHx + kH];
    const float b3_reg = w.params[kOffW3a + (int64_t)r16 * kHx + kH];
    const float stdv = kMode != kMlpDet ? w.std[sa] : 0.0f;

    // A row's place in its program.  kStep: an episode is running and its observation row is in X;
    // kDone: the queue is empty.  The others are resolved in part A of the step loop.
    enum { kNeedLane, kNeedSeg, kNeedEp, kEmit, kEndEp, kFinish, kStep, kDone };
    int phase = kNeedLane, after = kStep;  // after: the phase that follows kEmit
    int ln = 0, si = 0, s1 = 0, ep = 0, step = 0;
    bool ok = true;
    // policy stream (tape cursor or Philox counter) and noise stream of the current segment
    int64_t pcur = 0, ncur = 0, navail = 0;
    uint64_t pctr = 0, nctr = 0, octr = 0;
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
    // the pending observation (kEmit): trajectory slot, noise-tape position, "the tape has it"
    float* emit_dst = nullptr;
    int64_t emit_noff = 0;
    bool emit_have = true;
    __syncthreads();  // weights, the zeroed X tile and ALIVE visible

    // Barrier uniformity and termination.  The loop body below has exactly three workgroup
    // barriers (B1, B2, B3) and they stand in workgroup-uniform control flow: everything that
    // depends on a row's state (part A before B1, the row step after B3) is closed before the next
    // barrier, and the only way out of the loop is the `break` after B1, whose condition is one
    // LDS word read by every thread after B1 -- ALIVE[par], set before B1 by every row that has a
    // step to run -- so all four waves leave in the same iteration, after the same number of
    // barriers, whatever their rows did.  The word of the other parity is cleared by thread 0
    // between B1 and B2: its last readers passed it before B2 of the previous iteration (they
    // reached this B1), its next writers run after B3.  The queue fetch is in part A, outside any
    // barrier; a row that has found the queue empty stays in kDone (part A skips it) and feeds
    // zeros.  Part A itself ends: each pass of its loop moves the row one phase along
    // lane -> segment -> episode -> observation -> kStep (or to the lane's end and the next fetch),
    // and the queue counter only grows, so a row passes through it at most once per lane, segment
    // and episode.  Progress: in every iteration that does not break, each row in kStep advances
    // its episode by one step (or ends it); episodes end after at most max_steps steps and lanes
    // hold finitely many episodes, so after finitely many iterations every row is in kDone, no
    // row sets ALIVE and the workgroup leaves.
    for (int par = 0;; par ^= 1) {
        // ---- A: every row ends in kStep (observation row in X, draws available) or kDone
        while (phase != kDone) {
            if (phase == kStep) {
                if (kMode == kMlpTape && pcur + kD > a.policy_stride) {  // the tape ran out
                    pok = false;
                    phase = kFinish;
                    continue;
                }
                break;
            }
            if (phase == kNeedLane) {
                int L = 0;
                if (s == 0) L = atomicAdd(queue, 1);
                ln = (int)row_bcast_u32<0>((uint32_t)L);
                if (ln >= a.num_lanes) {
                    phase = kDone;
                    *reinterpret_cast<bf16x4*>(X + row * kEmXp + 4 * s) =
                        bf16x4{(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};  // an idle row feeds zeros
                    break;
                }
                ok = pok = true;
                pcur = 0;
                pctr = 0;
                if (kMode == kMlpTape) ptape = a.policy_tape + (int64_t)ln * a.policy_stride;
                if (kMode == kMlpDevice) env_key(a.policy_seed, keyed(ln), pk0, pk1);
                si = a.lane_segments[ln];
                s1 = a.lane_segments[ln + 1];
                phase = kNeedSeg;
            } else if (phase == kFinish) {  // the lane's end
                if (!pok) ok = false;
                if (s == 0) {
                    if (a.policy_used) a.policy_used[ln] = (int32_t)pcur;
                    if (!ok && a.status) atomicOr(a.status, 1);
                }
                phase = kNeedLane;
            } else if (phase == kNeedSeg) {  // the next segment of the lane (si), or the lane's end
                if (!ok || si >= s1) {
                    phase = kFinish;
                    continue;
                }
                const dxrl_eval_segment sg = a.segments[si];
                const bool noisy = sg.obs_noise_std > 0.0 || sg.dyn_noise_std > 0.0;
                if (sg.curriculum_row < 0 || sg.curriculum_row >= p.n_curricula || sg.first_episode < 0 ||
                    (ntape && noisy && sg.noise_offset < 0)) {
                    ok = false;
                    phase = kFinish;
                    continue;
                }
                cfg = sg.curriculum_row;
                const dxrl_curriculum& cu = curricula[cfg];
                const double* rg = s2 == 0 ? cu.size_range
                                           : s2 == 1 ? cu.mass_range
                                                     : s2 == 2 ? cu.friction_range
                                                               : s2 == 3 ? cu.spawn_x_range
                                                                         : s2 == 4 ? cu.spawn_y_range : cu.spawn_z_range;
                lo2 = rg[0];
                hi2 = rg[1];
                cst2 = s2 == 0 ? cu.object_size : s2 == 1 ? cu.object_mass : cu.friction_coefficient;
                has2 = s2 == 0 ? cu.has_size_range != 0
                               : s2 == 1 ? cu.has_mass_range != 0 : s2 == 2 ? cu.has_friction_range != 0 : true;
                fric64 = cu.friction_is_f64_scalar != 0;
                nok = true;
                if (ntape) {
                    ntp = a.noise_tape + sg.noise_offset;
                    navail = sg.noise_count;
                    ncur = 0;
                } else {
                    env_key(a.noise_seed, keyed(si), nk0, nk1);
                    nctr = 0;
                    octr = 0;
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
            } else if (phase == kNeedEp) {
                if (ep >= n_eps) {  // end of the segment
                    if (!nok) ok = false;
                    ++si;
                    phase = kNeedSeg;
                    continue;
                }
                rec = (int64_t)first_ep + ep;
                if (rec >= a.total_episodes) {
                    ok = false;
                    phase = kFinish;
                    continue;
                }
                // env.reset(seed=episode_seed) (EV:127, RT:281) [+ wrapper obs noise, RT:193-197]
                emit_noff = 0;
                emit_have = true;
                if (ntape && obs_noise) {
                    emit_have = ncur + kObs <= navail;
                    if (!emit_have) nok = false;
                    emit_noff = ncur;
                    ncur += kObs;
                }
                double u1, v2;
                if (a.reset_tape) {
                    u1 = a.reset_tape[rec * kReset + sa];
                    v2 = has2 ? a.reset_tape[rec * kReset + kD + s2] : cst2;
                } else {
                    uint32_t rk0, rk1;
                    env_key(a.reset_seed, keyed(rec), rk0, rk1);
                    u1 = -0.1 + (0.1 - -0.1) * reset_uniform_at(sa, rk0, rk1, 0);
                    v2 = has2 ? lo2 + (hi2 - lo2) * reset_uniform_at(kD + s2, rk0, rk1, 0) : cst2;
                }
                jp = s < kD ? (float)u1 : 0.0f;  // ME:143-145 .astype(float32)
                jv = 0.0f;
                size = row_bcast<0>(v2);
                fric = row_bcast<2>(v2);
                const double sx = row_bcast<3>(v2), sy = row_bcast<4>(v2), sz = row_bcast<5>(v2);
                const double spawn = s == 1 ? sy : (s == 2 ? sz : sx);
                const bool has = (flags & kHasObject) != 0;  // ME:156-161 sticky position
                if (s < 3) {
                    opd = (double)(float)(has ? opd : spawn);
                    ovd = 0.0f;
                }
                et = 0;
                flags = kOpIsF32 | kHasObject | (fric64 ? kFricF64 : 0u);
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
                emit_dst = otraj;  // slot 0: the reset observation
                after = kStep;
                phase = kEmit;
            } else if (phase == kEmit) {
                // The observation the policy sees next (ME:254-264 [+ wrapper noise, RT:193-207:
                // obs + f32(0 + s g)]): the row's lanes stage their elements as f32, lanes 0..11 then
                // take elements 4 s .. 4 s + 3, add the noise (tape: 45 normals at the segment cursor
                // emit_noff, emit_have = they exist; device: block s of the segment's observation
                // counter), write the trajectory slot and the bf16 X row (column 45 = 1, 46.. = 0).
                // LDS hand-off between the lanes of one row (one wave): program order, no barrier.
                float* ob = OBSF + row * kEmObsP;
                if (s < kD) {
                    ob[s] = jp;
                    ob[kD + s] = jv;
                }
                if (s < 3) {
                    ob[2 * kD + s] = (float)opd;
                    ob[2 * kD + 7 + s] = ovd;
                } else if (s < 7) {
                    ob[2 * kD + s] = s == 3 ? 1.0f : 0.0f;
                } else if (s < 7 + kF) {
                    ob[2 * kD + 10 + (s - 7)] = (float)((flags >> (s - 7)) & 1u);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (s < 12) {
                    const f32x4 v4 = *reinterpret_cast<const f32x4*>(ob + 4 * s);
                    float v[4] = {v4[0], v4[1], v4[2], v4[3]};
                    if (obs_noise) {
                        if (ntape) {
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                if (emit_have && 4 * s + q < kObs)
                                    v[q] = v[q] + (float)(0.0 + obs_sigma * ntp[emit_noff + 4 * s + q]);
                        } else {
                            const uint64_t c = octr * 12u + (uint64_t)s;
                            const u32x4 r = philox(
                                u32x4{(uint32_t)c, (uint32_t)(c >> 32), kStreamEvalNoise, kEvalObsBlock}, nk0, nk1);
                            float n[4];
                            box_muller(r.x, r.y, n[0], n[1]);
                            box_muller(r.z, r.w, n[2], n[3]);
#pragma unroll
                            for (int q = 0; q < 4; ++q) v[q] = v[q] + (float)obs_sigma * n[q];
                        }
                    }
                    if (emit_dst) {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (4 * s + q < kObs) emit_dst[4 * s + q] = v[q];
                    }
                    bf16x4 x;
#pragma unroll
                    for (int q = 0; q < 4; ++q) x[q] = to_bf16(v[q]);
                    if (s == 11) {  // elements 45 (the bias input), 46, 47
                        x[1] = (bf16)1.0f;
                        x[2] = x[3] = (bf16)0.0f;
                    }
                    *reinterpret_cast<bf16x4*>(X + row * kEmXp + 4 * s) = x;
                }
                if (obs_noise && !ntape) ++octr;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                phase = after;
            } else {  // kEndEp
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
        }
        if (phase == kStep && s == 0) ALIVE[par] = 1;
        lds_barrier();  // B1
        if (ALIVE[par] == 0) break;
        if (tid == 0) ALIVE[par ^ 1] = 0;
        // ---- the actor on the workgroup's 16 rows
        wave_layer16<kIn / 32, 4, false, true>(X, kEmXp, w1frag, 64 * wave, H1, kH, lane);  // bias: column 45
        lds_barrier();  // B2
        wave_layer16<kH / 32, 4, true, true>(H1, kH, w2frag, 64 * wave, H2, kH, lane, b2_reg);
        lds_barrier();  // B3
        {
            // mu head, the 16-env rollout's sequence: 16 rows x head rows 0..15 (15 live).  Every
            // wave runs it and keeps the four rows its own lanes step, so no barrier follows.
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            constexpr int kRing = 4;
            bf16x8 ah[kRing], bw[kRing];
#pragma unroll
            for (int k = 0; k < kRing; ++k) {
                ah[k] = *reinterpret_cast<const bf16x8*>(H2 + r16 * kH + swz16(r16, 32 * k + 8 * g16));
                bw[k] = *reinterpret_cast<const bf16x8*>(W3s + r16 * kEmW3p + 32 * k + 8 * g16);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < kH / 32; ++k) {
                acc = mfma16(ah[k % kRing], bw[k % kRing], acc);
                if (k + kRing < kH / 32) {
                    ah[k % kRing] = *reinterpret_cast<const bf16x8*>(H2 + r16 * kH + swz16(r16, 32 * (k + kRing) + 8 * g16));
                    bw[k % kRing] = *reinterpret_cast<const bf16x8*>(W3s + r16 * kEmW3p + 32 * (k + kRing) + 8 * g16);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (g16 == wave) {  // accumulator rows 4 g16 + q = this wave's env rows
#pragma unroll
                for (int q = 0; q < 4; ++q) MU[(4 * g16 + q) * kEmMuP + r16] = acc[q] + b3_reg;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        if (phase != kStep) continue;  // no barrier inside the row step: the next one is B1
        // ---- the policy's action: clip(mu [+ std * draw], -1, 1) (lane s: dim s)
        const float mu = MU[row * kEmMuP + sa];
        float act;
        if (kMode == kMlpDet) {
            act = clipf(mu, -1.0f, 1.0f);
        } else if (kMode == kMlpTape) {
            const double g = ptape[pcur + sa];  // availability checked in part A
            pcur += kD;
            act = clipf(mu + (float)(0.0 + (double)stdv * g), -1.0f, 1.0f);
        } else {  // the Philox policy stream, addressed as k_eval_ls addresses SIMPLE's
            const uint64_t c = pctr + (uint64_t)(sa >> 2);
            const u32x4 r = philox(u32x4{(uint32_t)c, (uint32_t)(c >> 32), kStreamPolicy, 0u}, pk0, pk1);
            float n0, n1;
            const bool hi = (sa & 2) != 0;
            box_muller(hi ? r.z : r.x, hi ? r.w : r.y, n0, n1);
            act = clipf(mu + stdv * ((sa & 1) ? n1 : n0), -1.0f, 1.0f);
            pctr += (kD + 3) / 4;
        }
        if (atraj && s < kD) atraj[step * kD + s] = act;
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
                const uint64_t c = nctr + (uint64_t)(sa >> 2);
                const u32x4 r = philox(u32x4{(uint32_t)c, (uint32_t)(c >> 32), kStreamEvalNoise, 0u}, nk0, nk1);
                float n0, n1;
                const bool hi = (sa & 2) != 0;
                box_muller(hi ? r.z : r.x, hi ? r.w : r.y, n0, n1);
                dz = (float)dyn_sigma * ((sa & 1) ? n1 : n0);
                nctr += (kD + 3) / 4;
            }
            act = clipf(act + dz, -1.0f, 1.0f);
        }
        // ---- env_step, lane-split (ME:198-252), as in k_eval_ls
        if (s < kD) {
            const float ak = clipf(act, -1.0f, 1.0f);
            jv = kC09 * jv + kC01 * ak;
            jp = clipf(jp + jv * kDt, -1.0f, 1.0f);
        }
        {
            const double damp = 1.0 - (fric * 0.1 * 0.01);
            const float dampf = (float)damp;
            const bool op32 = (flags & kOpIsF32) != 0, fric_f64 = (flags & kFricF64) != 0;
            const int ax = s < 3 ? s : 0;
            const double gz = ax == 2 ? kGz : 0.0, lo = ax == 2 ? 0.0 : -0.2, hi = ax == 2 ? 0.3 : 0.2;
            float v = fric_f64 ? (float)((double)ovd * damp) : ovd * dampf;
            v = (float)((double)v + gz);
            const float inc = v * kDt;
            double q = op32 ? (double)((float)opd + inc) : opd + (double)inc;
            q = clipd(q, lo, hi);
            if ((q <= lo && v < 0.0f) || (q >= hi && v > 0.0f)) v = 0.0f;
            if (s < 3) {
                opd = q;
                ovd = v;
            }
        }
        flags &= ~kOpIsF32;
        double op3[3], dmin;
        float g3[3];
        row_object(opd, op3);
        const uint32_t c = row_contacts(jp, op3, size, s, gbit, dmin, g3);
        double r;
        if (p.dense) {  // RS:50-187
            const double dist = exp(-5.0 * dmin);
            const double con = count_over_f_f64(__popc(c));
            float nacc = 0.0f;
#pragma unroll
            for (int j = 0; j < kJ; ++j)
                if (g3[j] < 0.0f) nacc = nacc + g3[j];
            float sum = 0.0f;
            row_neg_sum_fingers(nacc, sum);  // nacc of finger f on lane 3 f
            const float avg = div_f(sum);
            const float clo = clipf(div_f(avg), 0.0f, 1.0f);
            float st = 0.0f;
            if (flags & kHasPrev) {
                const uint32_t prev = (flags >> kPrevShift) & 0xFFu;
                float ch = 0.0f;
#pragma unroll
                for (int f = 0; f < kF; ++f) ch = ch + (float)(((c ^ prev) >> f) & 1u);
                st = clipf(1.0f - count_over_f_f32((uint32_t)ch), 0.0f, 1.0f);
            }
            flags = (flags & ~(0xFFu << kPrevShift)) | (c << kPrevShift) | kHasPrev;
            r = ((p.w.w_dist * dist + p.w.w_con * con) + p.w.w_clo * (double)clo) + p.w.w_st * (double)st;
        } else {
            r = (__popc(c) >= 3) ? 1.0 : -0.01;  // RS:226-231
        }
        flags = (flags & ~0xFFu) | c;
        te = __popc(c) >= 3;                        // ME:332-336
        const bool tr = et >= p.max_episode_steps;  // ME:245 (before the increment)
        et += 1;
        emit_noff = 0;
        emit_have = true;
        if (ntape && obs_noise) {
            emit_have = ncur + kObs <= navail;
            if (!emit_have) nok = false;
            emit_noff = ncur;
            ncur += kObs;
        }
        ret += r;  // EV:143 / RT:291 episode_reward += reward
        steps = step + 1;
        nc = (uint32_t)__popc(c);
        if (hist && s == 0) hist[step] = (uint8_t)nc;
        hist_acc_step(hm, nc, step);
        // the observation this step returns (trajectory slot step + 1, the policy's next input) is
        // written by the next part A, then the episode goes on or ends there
        emit_dst = otraj ? otraj + (int64_t)(step + 1) * kObs : nullptr;
        ++step;
        after = (te || tr || step >= a.max_steps) ? kEndEp : kStep;
        phase = kEmit;
    }
}

}  // namespace dxrl

extern "C" int dxrl_evaluate_mlp(dxrl_env* env, const dxrl_eval_args* args, const dxrl_eval_mlp* mlp, void* stream) {
    DXRL_REQUIRE(env && args && mlp, "null env / args / mlp");
    const dxrl_eval_args& a = *args;
    DXRL_REQUIRE(a.policy == DXRL_EVAL_POLICY_MLP, "dxrl_evaluate_mlp runs DXRL_EVAL_POLICY_MLP (%d), got policy %d",
                 DXRL_EVAL_POLICY_MLP, a.policy);
    DXRL_REQUIRE(mlp->packed && (reinterpret_cast<uintptr_t>(mlp->packed) & 15) == 0,
                 "packed must be a 16-byte aligned bf16 weight pack (dxrl_pg_pack_weights)");
    DXRL_REQUIRE(mlp->params, "null params (f32 master: layer-2 / head biases)");
    DXRL_REQUIRE(a.num_lanes > 0 && a.num_lanes <= env->cfg.num_envs, "num_lanes must be in [1, num_envs]");
    DXRL_REQUIRE(a.max_steps > 0 && a.total_episodes >= 0, "max_steps must be > 0, total_episodes >= 0");
    DXRL_REQUIRE(a.lane_segments && a.segments, "null segment table");
    DXRL_REQUIRE(a.ep_return && a.ep_length && a.ep_success, "null episode record buffers");
    DXRL_REQUIRE(!a.hist_moments || a.max_steps <= kHistMomentsMaxSteps,
                 "hist_moments packs its sums for max_steps <= %d, got %d", kHistMomentsMaxSteps, a.max_steps);
    const bool stochastic = mlp->action_std != nullptr, tape = a.policy_tape != nullptr;
    DXRL_REQUIRE(stochastic || !tape, "a policy tape was given in deterministic mode (action_std == NULL takes no draws)");
    DXRL_REQUIRE(!tape || a.policy_stride >= 0, "bad policy tape stride");
    DXRL_REQUIRE(a.work_queue, "null work_queue (device i32[1] scratch of this launch)");
    DXRL_REQUIRE(a.stream_period >= 0, "stream_period must be >= 0, got %lld", (long long)a.stream_period);
    DXRL_REQUIRE(a.stream_period == 0 || (!a.policy_tape && !a.noise_tape && !a.reset_tape),
                 "stream_period keys the device Philox streams: it cannot be combined with a parity tape");
    EvalParams p{weights_of(env->cfg),
                 env->cfg.max_episode_steps,
                 env->cfg.reward_type == DXRL_REWARD_DENSE,
                 env->cfg.has_object_position,
                 env->n_curricula,
                 {env->cfg.object_position[0], env->cfg.object_position[1], env->cfg.object_position[2]},
                 a,
                 nullptr};
    const EvalMlpWeights w{static_cast<const bf16*>(mlp->packed), mlp->params, mlp->action_std};
    const int dev = env->device;
    DeviceGuard g(dev);
    hipStream_t st = as_stream(stream);
    if (int rc = hip_check(hipMemsetAsync(a.work_queue, 0, sizeof(int32_t), st), "eval queue reset")) return rc;
    // one workgroup (16 rows) per CU, as k_eval_ls has by default (and as the register budget asks)
    int cus = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    int64_t blocks = (a.num_lanes + kEvalRows - 1) / kEvalRows;
    const int64_t resident = cus > 0 ? cus : 256;
    if (blocks > resident) blocks = resident;
    const dim3 grid((unsigned)blocks), block(kEvalThreads);
    const bool period = a.stream_period > 0 && a.stream_period <= (int64_t)INT32_MAX;  // no tape then (above)
    if (!stochastic && period)
        hipLaunchKernelGGL((k_eval_mlp<kMlpDet, true>), grid, block, 0, st, env->curricula, p, w, a.work_queue);
    else if (!stochastic)
        hipLaunchKernelGGL(k_eval_mlp<kMlpDet>, grid, block, 0, st, env->curricula, p, w, a.work_queue);
    else if (tape)
        hipLaunchKernelGGL(k_eval_mlp<kMlpTape>, grid, block, 0, st, env->curricula, p, w, a.work_queue);
    else if (period)
        hipLaunchKernelGGL((k_eval_mlp<kMlpDevice, true>), grid, block, 0, st, env->curricula, p, w, a.work_queue);
    else
        hipLaunchKernelGGL(k_eval_mlp<kMlpDevice>, grid, block, 0, st, env->curricula, p, w, a.work_queue);
    return launch_check("k_eval_mlp");
}
