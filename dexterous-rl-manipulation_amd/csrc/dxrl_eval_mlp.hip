// dxrl_eval_mlp.hip -- evaluation episode programs of the frozen MLP actor (DXRL_EVAL_POLICY_MLP).
//
// k_eval_mlp runs the episode programs of k_eval_ls on the same EvalRow (dxrl_eval_row.h: a row of 16
// lanes per env, 16 rows per workgroup, rows fed from the caller's work-queue counter; same segments,
// episodes, reset and noise tapes, records, histories, trajectories, policy_used and status word) with the
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
#include "dxrl_eval_row.h"
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
    EvalRow r(a, tid);
    const int s = r.s, sa = r.sa, row = tid >> 4;
    const int r16 = lane & 15, g16 = lane >> 4;  // 16x16x32 fragment row / k group (row == 4 wave + g16)
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

    // A row's place in its program is r.phase (EvalPhase).  kStep: an episode is running and its
    // observation row is in X; kDone: the queue is empty.  The others are resolved in part A of the
    // step loop, one transition of the row's program per pass.
    int after = kStep;  // the phase that follows kEmit
    uint64_t octr = 0;  // observation-noise blocks taken from the segment's Philox stream
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
        while (r.phase != kDone) {
            if (r.phase == kStep) {
                if (kMode == kMlpTape && r.pcur + kD > a.policy_stride) {  // the tape ran out
                    r.pok = false;
                    r.phase = kFinish;
                    continue;
                }
                break;
            }
            if (r.phase == kNeedLane) {
                r.take_lane(a, queue, kMode == kMlpTape, kMode == kMlpDevice, keyed);
                if (r.phase == kDone) {
                    *reinterpret_cast<bf16x4*>(X + row * kEmXp + 4 * s) =
                        bf16x4{(bf16)0.0f, (bf16)0.0f, (bf16)0.0f, (bf16)0.0f};  // an idle row feeds zeros
                    break;
                }
            } else if (r.phase == kFinish) {
                r.finish_lane(a);
            } else if (r.phase == kNeedSeg) {
                r.begin_segment(curricula, p, keyed);
                octr = 0;
            } else if (r.phase == kNeedEp) {
                r.begin_episode(a, keyed, emit_noff, emit_have);
                if (r.phase == kStep) {
                    emit_dst = r.otraj;  // slot 0: the reset observation
                    after = kStep;
                    r.phase = kEmit;
                }
            } else if (r.phase == kEmit) {
                // The observation the policy sees next (ME:254-264 [+ wrapper noise, RT:193-207:
                // obs + f32(0 + s g)]): the row's lanes stage their elements as f32, lanes 0..11 then
                // take elements 4 s .. 4 s + 3, add the noise (tape: 45 normals at the segment cursor
                // emit_noff, emit_have = they exist; device: block s of the segment's observation
                // counter), write the trajectory slot and the bf16 X row (column 45 = 1, 46.. = 0).
                // LDS hand-off between the lanes of one row (one wave): program order, no barrier.
                float* ob = OBSF + row * kEmObsP;
                r.write_obs(ob);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                if (s < 12) {
                    const f32x4 v4 = *reinterpret_cast<const f32x4*>(ob + 4 * s);
                    float v[4] = {v4[0], v4[1], v4[2], v4[3]};
                    if (r.obs_noise) {
                        if (r.ntape) {
#pragma unroll
                            for (int q = 0; q < 4; ++q)
                                if (emit_have && 4 * s + q < kObs)
                                    v[q] = v[q] + (float)(0.0 + r.obs_sigma * r.ntp[emit_noff + 4 * s + q]);
                        } else {
                            const uint64_t c = octr * 12u + (uint64_t)s;
                            const u32x4 u = philox(
                                u32x4{(uint32_t)c, (uint32_t)(c >> 32), kStreamEvalNoise, kEvalObsBlock}, r.nk0, r.nk1);
                            float n[4];
                            box_muller(u.x, u.y, n[0], n[1]);
                            box_muller(u.z, u.w, n[2], n[3]);
#pragma unroll
                            for (int q = 0; q < 4; ++q) v[q] = v[q] + (float)r.obs_sigma * n[q];
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
                if (r.obs_noise && !r.ntape) ++octr;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                r.phase = after;
            } else {  // kEndEp
                r.end_episode(a);
            }
        }
        if (r.phase == kStep && s == 0) ALIVE[par] = 1;
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
        if (r.phase != kStep) continue;  // no barrier inside the row step: the next one is B1
        // ---- the policy's action: clip(mu [+ std * draw], -1, 1) (lane s: dim s)
        const float mu = MU[row * kEmMuP + sa];
        float act;
        if (kMode == kMlpDet) {
            act = clipf(mu, -1.0f, 1.0f);
        } else if (kMode == kMlpTape) {
            const double g = r.ptape[r.pcur + sa];  // availability checked in part A
            r.pcur += kD;
            act = clipf(mu + (float)(0.0 + (double)stdv * g), -1.0f, 1.0f);
        } else {  // the Philox policy stream, addressed as k_eval_ls addresses SIMPLE's
            act = clipf(mu + stdv * row_step_normal(r.pctr, kStreamPolicy, r.pk0, r.pk1, sa), -1.0f, 1.0f);
        }
        if (r.atraj && s < kD) r.atraj[r.step * kD + s] = act;
        // dynamics noise and the env step; the observation this step returns (trajectory slot
        // step + 1, the policy's next input) is written by the next part A, then the episode goes on
        // or ends there
        const bool over = r.step_env(p, r.dynamics_noise(act), emit_noff, emit_have);
        emit_dst = r.otraj ? r.otraj + (int64_t)(r.step + 1) * kObs : nullptr;
        ++r.step;
        after = (over || r.step >= a.max_steps) ? kEndEp : kStep;
        r.phase = kEmit;
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
    if (int rc = eval_check_args(env, a, kEvalChkLanes, kEvalChkMoments)) return rc;
    const bool stochastic = mlp->action_std != nullptr, tape = a.policy_tape != nullptr;
    DXRL_REQUIRE(stochastic || !tape, "a policy tape was given in deterministic mode (action_std == NULL takes no draws)");
    if (int rc = eval_check_args(env, a, kEvalChkStride, kEvalChkQueue)) return rc;
    DXRL_REQUIRE(a.stream_period >= 0, "stream_period must be >= 0, got %lld", (long long)a.stream_period);
    DXRL_REQUIRE(a.stream_period == 0 || (!a.policy_tape && !a.noise_tape && !a.reset_tape),
                 "stream_period keys the device Philox streams: it cannot be combined with a parity tape");
    EvalParams p = eval_params(env, a);
    const EvalMlpWeights w{static_cast<const bf16*>(mlp->packed), mlp->params, mlp->action_std};
    const int dev = env->device;
    DeviceGuard g(dev);
    hipStream_t st = as_stream(stream);
    // one workgroup (16 rows) per CU, as k_eval_ls has by default (and as the register budget asks)
    int64_t blocks = 0;
    if (int rc = eval_queue_grid(a, dev, 1, st, blocks)) return rc;
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
