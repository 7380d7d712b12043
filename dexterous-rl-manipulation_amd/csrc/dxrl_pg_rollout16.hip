// dxrl_pg_rollout16.hip -- the fused policy-gradient rollout below 32 envs per CU: the
// warp-specialised 16-env kernel.  16 lanes per env, kLsEnvs = 16 envs per 256 env lanes.  (Round
// 5 retired the 4-wave lane-split kernel k_pg_rollout_ls, diag 64: k_pg_rollout_ws is its 8-wave
// successor and the one-lane k_pg_rollout (dxrl_pg.hip) and the 32-env k_pg_rollout_e8
// (dxrl_pg_rollout8.hip) remain its bit-identity twins.)
#include "dxrl_pg_mlp.h"
#include "dxrl_pg_rollout.h"

#include <stdio.h>

#include <vector>

using namespace dxrl;
using namespace dxrl::pg;

namespace dxrl {

// k_pg_rollout_ws: the lane-split rollout -- each env spread over the 16 lanes of one DPP row
// (lane s owns joint s, lanes 0..2 the object's axis s, every lane a copy of the env's scalars)
// -- with the work that does not depend on this step's env state taken off the env lanes'
// serial chain.  A workgroup owns 16 envs with 8 waves (two per SIMD):
//   * env waves 0..3: lane (env 4w + row, s) -- observation row, sampling, dynamics, contacts,
//     termination, auto-reset;
//   * aux waves 4..7: wave 4 + w is the lane-for-lane twin of env wave w.  While the env lanes
//     step, the twin computes log pi and the act / log pi tape and settles the PREVIOUS step's
//     dense reward and episode bookkeeping (return, records, sums) from the inputs the env lanes
//     left in LDS;
//   * in the head phase, one drawing aux wave per SIMD computes the step's Philox draws for all
//     16 envs (step_draws) while the env waves run the action-independent object update;
//   * all 8 waves split the actor MLP: one 32-column tile of L1 and of L2 each (two waves per
//     SIMD, so one wave's tanh epilogue overlaps the other's MFMAs); aux wave 7 runs the mu head.
// Every value is computed by the same instruction sequence as in k_pg_rollout (same MFMA
// tiles and K order, same Philox calls, same reward ops), so the tapes are bit-identical.
// Exchanges inside an env's 16 lanes are DPP row broadcasts (an env is one DPP row).
constexpr int kWsWaves = 8, kWsThreads = 64 * kWsWaves;

// One env lane's draws, computed by its aux twin (structure of arrays over the 256 env lanes):
// the action / dynamics noise normals and the reset uniforms (at the env's exact reset counter)
// of the current step, and the observation-noise normals of the lane's obs elements
// (row_obs_elem) for the next observation row.  The step's draws are single-buffered (written in
// the head phase, read before the next head phase); the observation noise is double-buffered by
// row parity (row t + 1's is written in step t's P0 while the env lanes read row t's).  The reward inputs (WsReward) are double-buffered
// by step parity: the env lanes write step t's while the aux lanes settle step t-1's.
struct __attribute__((aligned(16))) WsDraws {
    // on: the observation noise, double-buffered by row parity, element k of env e at [e][k]
    float eps[256], dzn[256], on[2][kLsEnvs * 48];
    double u1[256], u2[256];
};
// one env lane's extra reset draw (config.py:44-113 samplers): lo + span u with a range, the
// constant (lo = cst, span = NaN: u is never NaN) without one -- structure of arrays, so the reset
// path's two reads are conflict-free 8-byte loads
struct WsSamplers {
    double lo[256], span[256];
};
struct WsReward {      // an env's dense-reward inputs and episode end of one step
    double dmin;       // minimum finger distance; its square where the aux twin takes the root (kXm)
    uint32_t c, prev;  // contacts, previous contacts (kNoPrev: none)
    float nacc[kF];    // per finger: sum of its negative joint positions
    int32_t len;       // episode length after the step
    int32_t done, te;
    unsigned long long rctr;  // reset counter after the step (the next step's reset draws use it)
};

// Step t of a workgroup (16 envs, 8 waves):
//   P0  env lanes write the observation row (+ its observation noise, drawn in step t-1's P0);
//       aux lanes meanwhile draw the next row's observation noise (other parity buffer) and this
//       step's dynamics noise
//   P1  all waves: L1, one 32-column tile each            (the env lanes also store the obs row)
//   P2  all waves: L2, one 32-column tile each
//   P3  env wave 3: the mu head; all env waves: the object update (env_object_step).  In their
//       shadow, one drawing aux wave per SIMD (step_draws): wave 4 step t's action noise, waves
//       5, 6, 7 the reset uniforms at each env's exact counter (step t-1's episode end is known)
//   P4  env lanes: a = mu + sigma eps, dynamics, contacts, termination, auto-reset.
//       Aux lanes: the same a, log pi (DPP row sum in action order), the act / log pi tape, then
//       settle step t-1's reward and episode bookkeeping
// kNoise: configs with fused noise (or the noise parity tapes); kDiag: diag_flags / parity tapes
// set.  The production instantiations compile out every runtime check of the other's features
// (branches and SGPRs inside the step loop: -8 % rollout time for <false, false>).
// kDense = false: the sparse reward -- settle needs the contacts only, so the env lanes leave
// dmin, nacc[] and prev unwritten, and they leave the previous-contact bits of the env's flags
// alone, as env_step does (flags_with_prev_contacts is the dense reward's).
template <bool kNoise, bool kDiag, bool kDense = true>
__global__ __launch_bounds__(kWsThreads, 1) void k_pg_rollout_ws(PgRolloutArgs p) {
    constexpr int kRows = 32;
    // the env wave running the mu head: the env lanes idle while it runs (wave 0 instead, beside
    // the action-noise wave rather than a reset-draw wave: +-0.5 %, profiles/r05/ab_ws_head_wave_rejected.log)
    constexpr int kHeadWave = 3;
    // LDS images laid out for conflict-free 16-byte fragment reads (16-lane groups, 64 banks):
    // the read-only W1 / W3 and the observation rows padded to a 40 / 136-dword pitch, the hidden
    // rows unpadded with XOR-swizzled chunks (swz16; the padded 36 / 132-dword pitches of the
    // other rollout kernels make every fragment read 2-way)
    constexpr int kW1sW = kIn + 16, kW3sW = kH + 16, kXsW = kIn + 16, kHsW = kH;
    __shared__ __attribute__((aligned(16))) bf16 W1s[kH * kW1sW];
    __shared__ __attribute__((aligned(16))) bf16 W3s[kOut * kW3sW];
    __shared__ __attribute__((aligned(16))) bf16 X[kRows * kXsW];
    __shared__ __attribute__((aligned(16))) bf16 H1[kLsEnvs * kHsW];
    __shared__ __attribute__((aligned(16))) bf16 H2[kLsEnvs * kHsW];
    __shared__ float MU[kLsEnvs * (kOut + 1)];
    __shared__ float LS[kActPad], SIG[kActPad], ISIG[kActPad];
    __shared__ WsDraws DR;
    __shared__ WsReward RW[2][kLsEnvs];
    __shared__ WsSamplers RSMP;
    __shared__ uint32_t KEYS[kLsEnvs][4];           // per env: reset key ek0, ek1, policy key pk0, pk1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool aux = wave >= 4;
    // waves w and w + 4 share SIMD w; with fused noise the env waves issue first (P0's aux lanes
    // run a Philox round beside the observation row): noise configs -2.2 % rollout, the others
    // +1 % (so they keep equal priorities); aux first or per-phase priorities lose 5-10 %
    // (rollout_time A/B, profiles/r04/ab_rollout_wave_priority.log)
    constexpr int kPrio = kNoise ? 1 : 0;
    // Observation row t + 1 written at the end of step t's P4 instead of in step t + 1's P0 (no P0
    // phase, no barrier for it) -- in the instantiations without fused noise only: there the rollout
    // runs 1 % faster; with fused noise the aux waves' P0 draw stays and the env lanes' longer P4
    // (the row's noise add) made it 7 % slower (profiles/r05/ab_ws_obs_in_p4.log)
    constexpr bool kObsInP4 = !kNoise;
    // Two moves of work off the wave that sets a phase's length, in the instantiations without
    // fused noise (per-wave stamps and interleaved A/Bs: DESIGN section 2, profiles/r07/):
    //   kXm: the env lanes leave the minimum SQUARED finger distance in WsReward and the aux twin,
    //     the shorter wave of the SIMD in P4, takes the f64 root in front of settle's exp -- the
    //     same correctly rounded sqrt on the same operand;
    //   kHeadFirst: the head wave issues its object update after the mu head's MFMA chain, in the
    //     chain's latency shadow, not in front of it.
    // With fused noise the aux waves are P4's longer twins already (the root there: +0.4 %).
    constexpr bool kXm = !kNoise, kHeadFirst = !kNoise;
    if (kPrio != 0 && (__builtin_amdgcn_readfirstlane(wave) >= 4) == (kPrio == 2))
        __builtin_amdgcn_s_setprio(1);
    const int et_tid = tid & 255;  // the env lane this thread is (env wave) or twins (aux wave)
    const int eg = et_tid >> 4, s = et_tid & 15, gbit = 16 * (eg & 3);
    const int rbase = et_tid & ~15;
    const int64_t n = p.s.n;
    const int64_t i = (int64_t)blockIdx.x * kLsEnvs + eg;
    const bool live = i < n;
    const int64_t T = p.horizon;
    if (tid < kAct) {
        const float ls = p.params[kOffLogStd + tid];
        LS[tid] = ls;
        SIG[tid] = __expf(ls);
        ISIG[tid] = __expf(-ls);
    }
    // this wave's L2 columns 32 wave .. + 31 as two 16-column tiles of 16x16x32 fragments
    bf16x8 w2[2][kH / 32];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < kH / 32; ++k)
            w2[j][k] = *reinterpret_cast<const bf16x8*>(p.wbf + kBfW2a + (int64_t)(32 * wave + 16 * j + (lane & 15)) * kHx +
                                                        32 * k + 8 * (lane >> 4));
    for (int c = tid; c < kH * (kIn / 8); c += kWsThreads) {
        const int row = c / (kIn / 8), col = 8 * (c % (kIn / 8));
        *reinterpret_cast<bf16x8*>(W1s + row * kW1sW + col) =
            *reinterpret_cast<const bf16x8*>(p.wbf + kBfW1a + (int64_t)row * kIn + col);
    }
    for (int c = tid; c < kOut * (kH / 8); c += kWsThreads) {
        const int row = c / (kH / 8), col = 8 * (c % (kH / 8));
        *reinterpret_cast<bf16x8*>(W3s + row * kW3sW + col) =
            *reinterpret_cast<const bf16x8*>(p.wbf + kBfW3a + (int64_t)row * kHx + col);
    }
    for (int c = tid; c < kRows * kXsW; c += kWsThreads) {
        const int row = c / kXsW, col = c % kXsW;
        X[c] = (row < kLsEnvs && col == kObsIn) ? (bf16)1.0f : (bf16)0.0f;
    }
    const int r16 = lane & 15, g16 = lane >> 4;  // 16x16x32 fragment row / k group
    const auto w1frag = [&](int j, int k) {
        return *reinterpret_cast<const bf16x8*>(W1s + (32 * wave + 16 * j + r16) * kW1sW + 32 * k + 8 * g16);
    };
    const auto w2frag = [&](int j, int k) { return w2[j][k]; };
    // step-invariant biases in registers: L2 columns 32 wave + 16 j + 4 g16 + q, head row r16
    float b2_reg[8];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            b2_reg[4 * j + q] = p.params[kOffW2a + (int64_t)(32 * wave + 16 * j + 4 * g16 + q) * kHx + kH];
    const float b3_reg = p.params[kOffW3a + (int64_t)r16 * kHx + kH];

    // ---- env-lane state (env waves) / episode bookkeeping (aux waves)
    float jp = 0.0f, jv = 0.0f;
    double opd = 0.0;
    float ovd = 0.0f;
    uint32_t flags = 0;
    int32_t et = 0, cfg = 0;
    double size = 0.0, mass = 0.0, fric = 0.0;
    EpisodeBook book;
    uint64_t rctr = 0;
    uint32_t ek0 = 0, ek1 = 0, pk0 = 0, pk1 = 0;
    if (live) {
        if (!aux) {
            if (s < kD) {
                jp = p.s.jp[(int64_t)s * n + i];
                jv = p.s.jv[(int64_t)s * n + i];
            }
            if (s < 3) {
                opd = p.s.op[(int64_t)s * n + i];
                ovd = p.s.ov[(int64_t)s * n + i];
            }
            flags = p.s.flags[i];
            et = p.s.t[i];
            size = p.s.size[i];
            mass = p.s.mass[i];
            fric = p.s.fric[i];
        } else {
            book.ep_ret = p.ep_ret[i];
        }
        cfg = p.s.cfg[i];
        rctr = p.s.reset_ctr[i];
        env_key(p.env_seed, p.gid0 + i, ek0, ek1);
        env_key(p.policy_seed, p.gid0 + i, pk0, pk1);
    }
    const int s2 = s < DXRL_RESET_EXTRA ? s : 0;
    // this lane's extra reset sampler (config.py:44-113) -- read only when an episode ends, so
    // kept in LDS rather than in registers: RSMP.lo / span[et_tid] = {lo, hi - lo} or {constant, NaN}
    double lo2 = 0.0, hi2 = 0.0, cst2 = 0.0;
    bool has2 = true, fric64 = false;
    if (live && !aux) {
        const dxrl_curriculum& cu = p.s.curricula[cfg];
        const double* rg = s2 == 0 ? cu.size_range
                                   : s2 == 1 ? cu.mass_range
                                             : s2 == 2 ? cu.friction_range
                                                       : s2 == 3 ? cu.spawn_x_range : s2 == 4 ? cu.spawn_y_range : cu.spawn_z_range;
        lo2 = rg[0];
        hi2 = rg[1];
        cst2 = s2 == 0 ? cu.object_size : s2 == 1 ? cu.object_mass : cu.friction_coefficient;
        has2 = s2 == 0 ? cu.has_size_range != 0 : s2 == 1 ? cu.has_mass_range != 0 : s2 == 2 ? cu.has_friction_range != 0 : true;
        RSMP.lo[et_tid] = has2 ? lo2 : cst2;
        RSMP.span[et_tid] = has2 ? hi2 - lo2 : __builtin_nan("");
        fric64 = cu.friction_is_f64_scalar != 0;
    }
    const int sa = s < kAct ? s : 0;
    const bool obs_noise = kNoise && p.obs_noise > 0.0f, dyn_noise = kNoise && p.dyn_noise > 0.0f;
    if (live && !aux && s == 0) {
        KEYS[eg][0] = ek0;
        KEYS[eg][1] = ek1;
        KEYS[eg][2] = pk0;
        KEYS[eg][3] = pk1;
        RW[1][eg].rctr = rctr;  // "after step -1"
    }

    // ---- aux: Philox draws.  Each block is computed once per env row and its values written
    // straight into the LDS slots of the env lanes that use them (a lane-split kernel that draws on
    // shared blocks on every lane): lanes 0..10 reset block s (slots 2s, 2s + 1: joint slots 0..14
    // -> u1 of lane k, extra slots 15..20 -> u2 of lane k - 15); lanes 11..14 action- and
    // dynamics-noise block s - 11 (normals 4(s-11) .. +3); lanes 0..11 observation-noise block s
    // (obs elements 4s .. 4s + 3).  Same blocks and arithmetic as philox_normal_at /
    // reset_uniform_at, so the values are identical.
    const auto normals4 = [&](uint64_t ctr, uint32_t stream, int blk, float nz[4]) {  // noise streams only
        noise_normals4(ctr, stream, (uint32_t)blk, pk0, pk1, nz);
    };
    // Step t's action / dynamics noise and reset uniforms, computed in the head phase by the aux
    // waves, one per SIMD (waves w and w + 4 share SIMD w; Philox's 64-bit products are
    // quarter-rate, so two drawing waves on one SIMD serialise), while the env waves run the
    // action-independent object update (env_object_step) and wave 3 the mu head: one Philox block
    // per lane, keys (KEYS) and reset counters (RW[.].rctr) of all 16 envs from LDS, values
    // written straight into the consumers' slots.
    //   wave 4 (SIMD 0)        action noise: lane -> (env lane >> 2, block lane & 3) (the
    //                          dynamics noise is drawn in P0: obs_draws)
    //   waves 5, 6, 7 (SIMD 1, 2, 3 -- 3 also runs the head on the matrix core): group lane
    //                          g < 176 reset block g % 11 of env g / 11 (u01_53 of both halves:
    //                          joint slots 0..14 -> u1, extra slots 15..20 -> u2)
    constexpr int kResetBlocks = (kReset + 1) / 2;
    const auto step_draws = [&](uint64_t ctr, int64_t t_) {
        // the lane id re-read each step (volatile): the task indices and LDS addresses derived
        // from it are then not hoisted out of the step loop, where they only raise register
        // pressure into spills (each reload a vmcnt(0))
        int lane;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
        if (wave == 4) {
            const int e = lane >> 2, blk = lane & 3;
            if ((int64_t)blockIdx.x * kLsEnvs + e >= n) return;
            const u32x4 r = philox(u32x4{(uint32_t)ctr, (uint32_t)(ctr >> 32), kStreamPolicy, (uint32_t)blk},
                                   KEYS[e][2], KEYS[e][3]);
            float4 nz;
            box_muller(r.x, r.y, nz.x, nz.y);
            box_muller(r.z, r.w, nz.z, nz.w);
            // one 16-byte store per lane (slot 15 of the row is never read: kAct = 15); four
            // 4-byte stores at a 16-byte lane stride were 4-way bank conflicts
            *reinterpret_cast<float4*>(&DR.eps[16 * e + 4 * blk]) = nz;
            return;
        }
        if (wave < 5) return;
        const int g = 64 * (wave - 5) + lane;
        if (g >= kLsEnvs * kResetBlocks) return;
        const int e = g / kResetBlocks, blk = g % kResetBlocks;
        if ((int64_t)blockIdx.x * kLsEnvs + e >= n) return;
        const uint64_t rc = RW[(t_ - 1) & 1][e].rctr;
        const u32x4 r = philox(u32x4{(uint32_t)rc, (uint32_t)(rc >> 32), kStreamReset, (uint32_t)blk},
                               KEYS[e][0], KEYS[e][1]);
        const double ua = u01_53(r.x, r.y), ub = u01_53(r.z, r.w);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = 2 * blk + h;
            const double u = h ? ub : ua;
            if (k < kD) DR.u1[16 * e + k] = u;
            else if (k < kReset) DR.u2[16 * e + k - kD] = u;
        }
    };
    // P0 draws of the aux lanes (counter-only, so drawn where the aux waves would wait for the env
    // lanes' observation row): lanes s < 12 of env row eg the observation noise of row ctr (block
    // s) into DR.on[buf]; lanes 12..15 (dyn = true) the dynamics noise of step dctr (block s - 12,
    // normals 4 (s - 12) .. + 3) -- 64 busy lanes per aux wave, one Philox block each.
    const auto obs_draws = [&](uint64_t ctr, int buf, bool dyn = false, uint64_t dctr = 0) {
        constexpr int kOb = (kObs + 3) / 4;  // 12 observation blocks per row
        const bool is_obs = s < kOb, want = is_obs ? obs_noise : (dyn && dyn_noise);
        if (!(obs_noise || (dyn && dyn_noise))) return;
        // one Philox block per lane, the stream / counter / block selected per lane, so the wave
        // runs ONE Philox + Box-Muller sequence (lanes 12..15 branching into a second stream
        // would serialise the two)
        float nz[4];
        normals4(is_obs ? ctr : dctr, is_obs ? kStreamObs : kStreamDyn, is_obs ? s : s - kOb, nz);
        if (!want) return;
        if (!is_obs) {  // one 16-byte store (slot 15 never read), as the action noise
            *reinterpret_cast<float4*>(&DR.dzn[rbase + 4 * (s - kOb)]) = float4{nz[0], nz[1], nz[2], nz[3]};
            return;
        }
        // elements 4 s .. 4 s + 3 of the env's row (45..47 never read): one 16-byte store
        *reinterpret_cast<float4*>(&DR.on[buf][48 * eg + 4 * s]) = float4{nz[0], nz[1], nz[2], nz[3]};
        if (kDiag && p.obs_noise_tape)  // parity tape: the value write_obs_row adds (row ctr - iteration T)
            write_obs_noise_tape(p, (int64_t)(ctr - p.iteration * (uint64_t)T), i, s, nz);
    };
    // ---- aux: the reward (dense_reward_of / sparse_reward) and the episode bookkeeping of a
    // finished step
    const auto settle = [&](int64_t t_) {
        const WsReward& w = RW[t_ & 1][eg];
        double r;
        if constexpr (kDense) {
            float sum = 0.0f;
#pragma unroll
            for (int f = 0; f < kF; ++f) sum = sum + (-w.nacc[f]);
            double comp[4];
            r = dense_reward_of(kXm ? sqrt(w.dmin) : w.dmin, w.c, w.prev, sum, p.w, comp);  // kXm: the square
        } else {
            r = sparse_reward(w.c);
        }
        book.settle_step(p, r, w.done, w.te, w.len, t_, i, s == 0);
    };
    // lane s's elements row_obs_elem(s, 0..3): joint position, joint velocity, object position /
    // identity quaternion (ME:164) / finger contact, object velocity -- the values selected
    // without divergent branches, then at most four predicated 2-byte stores (the if / else-if
    // chain compiled to a serial walk of exec-masked regions on the env waves' critical path)
    const auto write_obs_row = [&](int buf) {  // buf: the row's noise buffer (row parity)
        bf16* xr = X + eg * kXsW;
        const auto put = [&](float v, int k) {
            if (obs_noise) v = v + p.obs_noise * DR.on[buf][48 * eg + k];
            xr[k] = to_bf16(v);
        };
        const float v2 = s < 3 ? (float)opd : (s < 7 ? (s == 3 ? 1.0f : 0.0f) : (float)((flags >> ((s - 7) & 31)) & 1u));
        if (s < kD) {
            put(jp, s);
            put(jv, kD + s);
        }
        if (s < 7 + kF) put(v2, s < 7 ? 2 * kD + s : 2 * kD + 3 + s);
        if (s < 3) put(ovd, 2 * kD + 7 + s);
    };
    const auto tape_obs_row = [&](int64_t m) {
        *reinterpret_cast<bf16x4*>(p.obs_rm + m * kIn + 4 * s) = *reinterpret_cast<const bf16x4*>(X + eg * kXsW + 4 * s);
    };
    const bool mlp = !kDiag || !(p.diag & 1), env_on = !kDiag || !(p.diag & 2);
    // ---- env lanes, head phase of step t: the object's velocity damping, gravity, position and
    // wall stops (ME:212-235) -- independent of the action, so off the P4 chain (the env waves
    // wait for the head and the draws here anyway)
    const auto env_object_step = [&]() {
        const AxisState ax = object_axis_step(opd, ovd, s < 3 ? s : 0, fric, flags);
        if (s < 3) {
            opd = ax.q;
            ovd = ax.v;
        }
        flags &= ~kOpIsF32;
    };
    // ---- env lanes, P4 of step t: action, dynamics, contacts, termination, auto-reset
    const auto env_lane_step = [&](int64_t t, int64_t m) {
        const float mu = mlp ? MU[eg * (kOut + 1) + sa] : 0.0f;
        float a = mu + SIG[sa] * DR.eps[et_tid];
        if (dyn_noise)  // robustness_tests.py:180-187 (the tape keeps the policy's action)
            a = clipf(a + p.dyn_noise * DR.dzn[et_tid], -1.0f, 1.0f);
        bool te = false, tr = false;
        if (env_on) {
            // ---- env_step, lane-split (ME:198-252)
            if (s < kD) joint_step(jp, jv, a);
            // (the object's update, which does not depend on the action, ran in the head phase:
            // env_object_step)
            double op3[3];
            row_object(opd, op3);
            double dmin;
            float g3[3];
            const uint32_t c = row_contacts<kDense, !kXm>(jp, op3, size, s, gbit, dmin, g3);
            // the reward's inputs for the aux twin (RS:101-187; sparse: the contacts)
            WsReward& rw = RW[t & 1][eg];
            if constexpr (kDense) {
                const float nacc = negative_sum(g3);
                if (finger_lane(s)) rw.nacc[s / kJ] = nacc;  // finger f on lane 3 f
                if (s == 0) {
                    rw.dmin = dmin;
                    rw.c = c;
                    rw.prev = prev_contacts(flags);
                }
            } else {
                if (s == 0) rw.c = c;
            }
            if (kDense) flags = flags_with_prev_contacts(flags, c);
            flags = flags_with_contacts(flags, c);
            te = __popc(c) >= 3;
            tr = et >= p.max_episode_steps;
            et += 1;
        }
        const bool d = env_on && (te || tr || et >= p.max_steps);
        if (s == 0) {
            write_step_end(p, m, d, te, et);
            WsReward& rw = RW[t & 1][eg];
            rw.done = d;
            rw.te = te;
            rw.len = et;
        }
        if (d) {
            // ---- env_reset_philox, lane-split: lane s holds slot s (joint) and slot 15 + s
            const double u1 = DR.u1[et_tid], u2 = DR.u2[et_tid];
            const double slo = RSMP.lo[et_tid], span = RSMP.span[et_tid];
            const double v2 = sampler_value(slo, span, u2);
            if (s < kD) {
                jp = (float)joint_reset_draw(u1);
                jv = 0.0f;
            }
            size = row_bcast<0>(v2);
            mass = row_bcast<1>(v2);
            fric = row_bcast<2>(v2);
            const double sx = row_bcast<3>(v2), sy = row_bcast<4>(v2), sz = row_bcast<5>(v2);
            const double spawn = s == 1 ? sy : (s == 2 ? sz : sx);
            const bool has = (flags & kHasObject) != 0;
            if (s < 3) object_axis_reset(opd, ovd, has, spawn);
            et = 0;
            flags = flags_after_reset(fric64);
            double op3[3];
            row_object(opd, op3);
            double dmin;
            float g3[3];
            flags |= row_contacts<false>(jp, op3, size, s, gbit, dmin, g3);  // ME:176 (no dmin)
            ++rctr;
        }
        if (s == 0) RW[t & 1][eg].rctr = rctr;
    };
    // ---- aux lanes, P4 of step t: the policy sample, log pi(a|s) (gauss_logp's order), tapes
    const auto aux_lane_step = [&](int64_t m) {
        const float mu = mlp ? MU[eg * (kOut + 1) + sa] : 0.0f;
        float a = mu + SIG[sa] * DR.eps[et_tid];
        const float z = (a - mu) * ISIG[sa];
        const float term = -0.5f * z * z - LS[sa] - 0.5f * kLog2Pi;
        float lp = 0.0f;
        row_sum_in_order<kAct>(term, lp);
        p.act[m * kActPad + s] = s < kAct ? a : 0.0f;
        if (s == 0) p.logp[m] = lp;
        if (kDiag && p.applied_act) {
            if (dyn_noise) a = clipf(a + p.dyn_noise * DR.dzn[et_tid], -1.0f, 1.0f);
            p.applied_act[m * kActPad + s] = s < kAct ? a : 0.0f;
        }
        if (kDiag && p.dyn_noise_tape)  // parity tape: the value env_lane_step adds to the action
            p.dyn_noise_tape[m * kActPad + s] = (dyn_noise && s < kAct) ? p.dyn_noise * DR.dzn[et_tid] : 0.0f;
    };

    // diag & 128: s_memtime segment stamps per step (diagnostics only), one record per wave:
    // wave w of workgroup g into stamps[(8 g + w) 8 + k], so the longest wave of a phase can be
    // read off (tools/rollout_stamps.py)
    unsigned long long st_acc[8], st_last = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) st_acc[q] = 0;
#define WS_STAMP(k)                                                                              \
    do {                                                                                         \
        if (kDiag && (p.diag & 128)) {                                                           \
            __builtin_amdgcn_sched_barrier(0);                                                   \
            unsigned long long t_;                                                               \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");          \
            __builtin_amdgcn_sched_barrier(0);                                                   \
            st_acc[k] += t_ - st_last;                                                           \
            st_last = t_;                                                                        \
        }                                                                                        \
    } while (0)
    if (aux && live) obs_draws(p.iteration * (uint64_t)T, 0);
    // kObsInP4: observation row t + 1 is written by the env lanes at the end of step t's P4
    // (right after the state it shows), so step t + 1 opens with layer 1 -- no P0 phase and no
    // barrier for it (row 0 here, before the first one)
    if (kObsInP4) {
        __syncthreads();  // row 0's noise (drawn just above) visible
        if (!aux && live) write_obs_row(0);
    }
    __syncthreads();
    WS_STAMP(7);
    for (int64_t t = 0; t < T; ++t) {
        const int64_t m = t * n + i;
        const uint64_t ctr = p.iteration * (uint64_t)T + (uint64_t)t;
        if (!kObsInP4 && !aux && live) write_obs_row((int)(t & 1));
        // the next observation row's noise (aux lanes, own rows; counter-only, so drawn here where
        // the aux waves wait for the env lanes' row, not in the head phase beside the draws)
        if (aux && live && (!kDiag || !(p.diag & 256))) obs_draws(ctr + 1, (int)((t + 1) & 1), true, ctr);
        WS_STAMP(0);
        if (!kObsInP4) lds_barrier();
        if (!aux && live) tape_obs_row(m);
        if (mlp) wave_layer16<kIn / 32, 2, false, true>(X, kXsW, w1frag, 32 * wave, H1, kHsW, lane);  // b: col 45
        WS_STAMP(1);
        lds_barrier();
        if (mlp) wave_layer16<kH / 32, 2, true, true>(H1, kHsW, w2frag, 32 * wave, H2, kHsW, lane, b2_reg);
        WS_STAMP(2);
        lds_barrier();
        if (!aux && live && env_on && !(kHeadFirst && mlp && wave == kHeadWave)) env_object_step();
        if (mlp && wave == kHeadWave) {  // mu head: 16 env rows x head rows 0..15 (15 live)
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
            // H2 rows and W3 rows (head outputs) from LDS as 16x16x32 fragments: a ring of 4
            // k-steps, refilled 4 ahead (pinned by scheduling barriers, as in wave_layer16)
            constexpr int kRing = 4;
            bf16x8 ah[kRing], bw[kRing];
#pragma unroll
            for (int k = 0; k < kRing; ++k) {
                ah[k] = *reinterpret_cast<const bf16x8*>(H2 + r16 * kHsW + swz16(r16, 32 * k + 8 * g16));
                bw[k] = *reinterpret_cast<const bf16x8*>(W3s + r16 * kW3sW + 32 * k + 8 * g16);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int k = 0; k < kH / 32; ++k) {
                acc = mfma16(ah[k % kRing], bw[k % kRing], acc);
                if (k + kRing < kH / 32) {
                    ah[k % kRing] = *reinterpret_cast<const bf16x8*>(H2 + r16 * kHsW + swz16(r16, 32 * (k + kRing) + 8 * g16));
                    bw[k % kRing] = *reinterpret_cast<const bf16x8*>(W3s + r16 * kW3sW + 32 * (k + kRing) + 8 * g16);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (kHeadFirst && live && env_on) env_object_step();  // behind the chain (see kHeadFirst)
#pragma unroll
            for (int q = 0; q < 4; ++q) MU[(4 * g16 + q) * (kOut + 1) + r16] = acc[q] + b3_reg;
        }
        if (!aux && mlp && p.h2_tape) {
            // the step's H2 rows (16 envs x 32 chunks of 16 bytes, chunk c of row r at c ^ r) to
            // the tape that the actor's train pass reads instead of recomputing layer 2; env lane
            // et_tid copies chunks et_tid and et_tid + 256 (wave 3 after its head)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int q = et_tid + 256 * u, row = q >> 5, c = q & 31;
                const int64_t ie = (int64_t)blockIdx.x * kLsEnvs + row;
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(H2 + row * kHsW + ((c ^ row) << 3));
                if (ie < n)  // non-temporal: read back once, by the actor's train pass (ab_h2_tape_nt.log)
                    __builtin_nontemporal_store(v, reinterpret_cast<bf16x8*>(p.h2_tape + (t * n + ie) * kH2Ld + 8 * c));
            }
        }
        if (!kDiag || !(p.diag & 256)) {
            // this step's draws (RW[(t - 1) & 1].rctr: the counters after step t-1's resets)
            if (aux) step_draws(ctr, t);
        }
        WS_STAMP(3);
        lds_barrier();
        WS_STAMP(4);
        if (live) {
            if (aux) {
                aux_lane_step(m);
                if (t > 0 && env_on && !(kDiag && (p.diag & 512))) settle(t - 1);  // step t-1's reward and bookkeeping
            } else {
                env_lane_step(t, m);
                if (kObsInP4) write_obs_row((int)((t + 1) & 1));  // row t + 1 (row T: the bootstrap)
            }
        }
        WS_STAMP(5);
        lds_barrier();  // this step's reward inputs / the next row's noise visible
        WS_STAMP(6);
    }
#undef WS_STAMP
    if (kDiag && (p.diag & 128) && lane == 0) {  // one record per wave: stamps[(8 group + wave) 8 + k]
#pragma unroll
        for (int q = 0; q < 8; ++q) p.stamps[((int64_t)blockIdx.x * kWsWaves + wave) * 8 + q] = st_acc[q];
    }
    if (live && aux) {
        if (T > 0 && env_on) settle(T - 1);
        if (kDiag && (p.diag & 2))
            for (int64_t t = 0; t < T && s == 0; ++t) p.rew[t * n + i] = 0.0f;
        if (s == 0) book.store(p, i);
    }
    if (live && !aux) {
        // bootstrap observation (slot T; with kObsInP4 already written by the last step's P4),
        // then the state back to the slab
        if (!kObsInP4 || T == 0) write_obs_row((int)(T & 1));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        tape_obs_row(T * n + i);
        if (s < kD) {
            p.s.jp[(int64_t)s * n + i] = jp;
            p.s.jv[(int64_t)s * n + i] = jv;
        }
        if (s < 3) {
            p.s.op[(int64_t)s * n + i] = opd;
            p.s.ov[(int64_t)s * n + i] = ovd;
        }
        if (s == 0) {
            p.s.flags[i] = flags;
            p.s.t[i] = et;
            p.s.size[i] = size;
            p.s.mass[i] = mass;
            p.s.fric[i] = fric;
            p.s.reset_ctr[i] = rctr;
        }
    }
}

int launch_pg_rollout_ws(const PgRolloutArgs& p, int64_t n, bool noise, bool diag, bool dense, hipStream_t st) {
    const dim3 grid((unsigned)((n + kLsEnvs - 1) / kLsEnvs)), block(kWsThreads);
    with_rollout_switches(noise, diag, dense, [&](auto kNoise, auto kDiag, auto kDense) {
        hipLaunchKernelGGL((k_pg_rollout_ws<kNoise(), kDiag(), kDense()>), grid, block, 0, st, p);
    });
    if (int rc = launch_check("k_pg_rollout_ws")) return rc;
    if (p.diag & 128) {  // diagnostics: mean cycles per step segment of every wave, env / aux means
        const int64_t groups = (n + kLsEnvs - 1) / kLsEnvs;
        std::vector<unsigned long long> h((size_t)groups * kWsWaves * 8);
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h.data(), p.stamps, h.size() * 8, hipMemcpyDeviceToHost);
        double mean[kWsWaves][7];  // over the workgroups in which the wave has a live env
        for (int wv = 0; wv < kWsWaves; ++wv)
            for (int k = 0; k < 7; ++k) {
                double sum = 0;
                int64_t cnt = 0;
                for (int64_t g = 0; g < groups; ++g)
                    if (g * kLsEnvs + 4 * (wv & 3) < n) {
                        sum += (double)h[(size_t)(g * kWsWaves + wv) * 8 + k];
                        ++cnt;
                    }
                mean[wv][k] = cnt ? sum / cnt / p.horizon : 0.0;
            }
        for (int w = 0; w < 2; ++w) {
            fprintf(stderr, "rollout_ws %s cycles/step:", w ? "aux" : "env");
            for (int k = 0; k < 7; ++k)
                fprintf(stderr, " s%d=%.0f", k, (mean[4 * w][k] + mean[4 * w + 1][k] + mean[4 * w + 2][k] + mean[4 * w + 3][k]) / 4);
            fprintf(stderr, "\n");
            for (int wv = 4 * w; wv < 4 * w + 4; ++wv) {
                fprintf(stderr, "  wave %d:", wv);
                for (int k = 0; k < 7; ++k) fprintf(stderr, " s%d=%.0f", k, mean[wv][k]);
                fprintf(stderr, "\n");
            }
        }
    }
    return DXRL_OK;
}

}  // namespace dxrl
