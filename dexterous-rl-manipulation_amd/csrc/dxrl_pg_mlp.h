// dxrl_pg_mlp.h -- the actor MLP's per-wave layer functions, shared by every kernel that runs the
// network step by step out of LDS / registers (dxrl_pg.hip: the rollout kernels; dxrl_eval_mlp.hip:
// the evaluation kernel): same MFMA tiles, k order, tanh and bias arithmetic wherever they are
// used, so the hidden units agree bit for bit.
#pragma once
#include "dxrl_mfma.h"
#include "dxrl_pg_rollout.h"

namespace dxrl {

// Register-resident weight fragments: one 32-column N tile of a layer, all of
// K (K/16 MFMA k-steps): b[k] = W[n0 + r][16k + 8h .. 16k + 8h + 7].  Loaded
// once per rollout launch, so the per-step MLP reads no weights from memory.
template <int KS>
struct WTile {
    bf16x8 b[KS];
};

template <int KS>
__device__ __forceinline__ void load_wtile(WTile<KS>& w, const bf16* W, int ldw, int n0, int lane) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int k = 0; k < KS; ++k) w.b[k] = *reinterpret_cast<const bf16x8*>(W + (int64_t)(n0 + r) * ldw + 16 * k + 8 * h);
}

// One wave: 64 rows x 32*NT columns of act(A . W^T + b) into LDS.  A: LDS [64][lda]
// bf16; the weight fragment of N-tile j, k-step k comes from wfrag(j, k) (registers
// or LDS); bias: f32 master column (bias[n * ldb]), the values the training GEMMs use, or
// bias_v[j] = that value already in a register (a persistent kernel hoists the load: a global
// load inside the step loop puts a vmcnt(0) -- which also drains every outstanding tape store --
// on the step's critical path).
template <int KS, int NT, bool kTanh, int RT = 2, typename WF, bool kRing = false>
__device__ __forceinline__ void wave_layer(const bf16* A, int lda, const WF& wfrag, int n0, const float* bias_p,
                                           int ldb, bf16* out, int ldo, int lane, const float* bias_v = nullptr) {
    // RT row tiles of 32 (RT == 1: 16 live rows -- accumulator registers q < 8)
    constexpr int kQ = RT == 1 ? 8 : 16;
    const int r = lane & 31, h = lane >> 5;
    f32x16 acc[RT][NT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.0f;
    if constexpr (RT == 1 && !kRing) {
        // one row tile: issue every activation fragment up front (KS LDS reads in flight),
        // then the MFMA chain consumes them with counted waits
        bf16x8 a[KS];
#pragma unroll
        for (int k = 0; k < KS; ++k) a[k] = *reinterpret_cast<const bf16x8*>(A + r * lda + 16 * k + 8 * h);
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[0][j] = mfma32(a[k], wfrag(j, k), acc[0][j]);
    } else if constexpr (RT == 1) {
        // one row tile: a ring of kD activation fragments, refilled kD k-steps ahead; the
        // scheduling barriers keep the refills where they are (under register pressure the
        // scheduler otherwise sinks every read next to its MFMA, exposing one LDS latency per
        // k-step instead of one per chain)
        constexpr int kD = KS < 4 ? KS : 4;
        bf16x8 a[kD];
#pragma unroll
        for (int k = 0; k < kD; ++k) a[k] = *reinterpret_cast<const bf16x8*>(A + r * lda + 16 * k + 8 * h);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < KS; ++k) {
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[0][j] = mfma32(a[k % kD], wfrag(j, k), acc[0][j]);
            if (k + kD < KS) a[k % kD] = *reinterpret_cast<const bf16x8*>(A + r * lda + 16 * (k + kD) + 8 * h);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            bf16x8 a[RT];
#pragma unroll
            for (int i = 0; i < RT; ++i) a[i] = *reinterpret_cast<const bf16x8*>(A + (32 * i + r) * lda + 16 * k + 8 * h);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const bf16x8 b = wfrag(j, k);
#pragma unroll
                for (int i = 0; i < RT; ++i) acc[i][j] = mfma32(a[i], b, acc[i][j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n0 + 32 * j + r;
        const float bias = bias_v ? bias_v[j] : bias_p ? bias_p[(int64_t)n * ldb] : 0.0f;
        const float bk = tanh_bias(bias);
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int q = 0; q < kQ; ++q) {
                const float v = kTanh ? tanh_pre(acc[i][j][q], bk) : acc[i][j][q] + bias;
                out[(32 * i + acc_row(q, lane)) * ldo + n] = to_bf16(v);
            }
    }
}

// 16-row tiles on v_mfma_f32_16x16x32_bf16 for a 16-env workgroup: one wave computes the 16
// activation rows x 16*NT columns with no dead MFMA rows (wave_layer's RT == 1 tile carries 16
// live rows in a 32-row MFMA: twice the matrix-core cycles per output).  A chain of 16x16x32
// MFMAs over k-steps of 32 rounds exactly like the 32x32x16 chain over the same k order
// (tools/mfma_order.hip: 0 of 131,072 outputs differ), so the hidden units stay bit-identical to
// the learner's forward and to the one-lane k_pg_rollout.  Transposed formulation (weights as the A
// operand, as in the learner): lane l's accumulator holds columns n0 + 16 j + 4 (l >> 4) .. +3 of
// activation row l & 15, so the tanh epilogue runs on packed pairs and leaves as one 8-byte LDS
// store per tile.  Fragments: A row l & 15, k 32 k + 8 (l >> 4) ..+7; wfrag(j, k) =
// W[n0 + 16 j + (l & 15)][32 k + 8 (l >> 4) ..+7].  Activation fragments stream through a ring
// kD k-steps ahead (pinned by scheduling barriers).  bias_v[4 j + q]: the bias of column
// n0 + 16 j + 4 (l >> 4) + q (or null: none).
// kSwzA / kSwzOut: the activation rows A / out are 256-element rows stored with their 16-byte
// chunks XOR-swizzled by the row (chunk c of row r at chunk c ^ r, r < 16; swz16): the fragment
// reads (ds_read_b128, lane groups of 16) are then conflict-free and the 8-byte epilogue stores
// stay 2-way, where the padded 264-element pitch made every fragment read 2-way.
template <int KS, int NT, bool kSwzA = false, bool kSwzOut = false, typename WF>
__device__ __forceinline__ void wave_layer16(const bf16* A, int lda, const WF& wfrag, int n0, bf16* out, int ldo,
                                             int lane, const float* bias_v = nullptr) {
    const int r = lane & 15, g = lane >> 4;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int kD = KS < 4 ? KS : 4;
    const auto afrag = [&](int k) {
        const int col = 32 * k + 8 * g;
        return *reinterpret_cast<const bf16x8*>(A + r * lda + (kSwzA ? swz16(r, col) : col));
    };
    bf16x8 a[kD];
#pragma unroll
    for (int k = 0; k < kD; ++k) a[k] = afrag(k);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < KS; ++k) {
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j] = mfma16(wfrag(j, k), a[k % kD], acc[j]);
        if (k + kD < KS) a[k % kD] = afrag(k + kD);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        bf16x4 v;
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
            const f32x2 b = bias_v ? f32x2{tanh_bias(bias_v[4 * j + q]), tanh_bias(bias_v[4 * j + q + 1])}
                                   : f32x2{0.0f, 0.0f};
            const f32x2 t = tanh_pre2(f32x2{acc[j][q], acc[j][q + 1]}, b);
            v[q] = to_bf16(t.x);
            v[q + 1] = to_bf16(t.y);
        }
        const int col = n0 + 16 * j + 4 * g;
        *reinterpret_cast<bf16x4*>(out + r * ldo + (kSwzOut ? swz16(r, col) : col)) = v;
    }
}

}  // namespace dxrl
