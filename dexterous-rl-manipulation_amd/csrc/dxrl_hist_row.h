// dxrl_hist_row.h -- one wave's reduction of a contact_hist row, shared by the per-episode passes
// of dxrl_eval_summarize and dxrl_failure_summarize.
#ifndef DXRL_HIST_ROW_H_
#define DXRL_HIST_ROW_H_
#include <cstdint>

#include <hip/hip_runtime.h>

namespace dxrl {

struct HistRow {
    int s1, s2, f5, l5, peak;  // sum, sum of squares, first-five sum, last-five sum, maximum
};

// The first n bytes of `row` reduced by the 64 lanes of a wave: dword loads of the row body, byte
// loads of an unaligned head / tail (nothing outside [row, row + n) is read).  Every lane returns
// the row's totals; the maximum is computed only with kPeak (0 otherwise).
template <bool kPeak>
__device__ __forceinline__ HistRow hist_row_reduce(const uint8_t* __restrict__ row, int n, int lane) {
    const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 3);
    const int ndw = (mis + n + 3) >> 2;
    int s1 = 0, s2 = 0, f5 = 0, l5 = 0, pk = 0;
    for (int j = lane; j < ndw; j += 64) {
        const int o = 4 * j - mis;  // row offset of this dword's byte 0
        uint32_t w = 0;
        if (o >= 0 && o + 4 <= n) {
            w = *reinterpret_cast<const uint32_t*>(row + o);
        } else {  // head / tail: only the bytes inside [0, n)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = o + k;
                if (t >= 0 && t < n) w |= (uint32_t)row[t] << (8 * k);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int t = o + k;
            const int c = (int)((w >> (8 * k)) & 0xffu);  // 0 outside [0, n)
            s1 += c;
            s2 += c * c;
            if (t < 5) f5 += c;
            if (t >= n - 5) l5 += c;
            if (kPeak) pk = c > pk ? c : pk;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        s1 += __shfl_xor(s1, m, 64);
        s2 += __shfl_xor(s2, m, 64);
        f5 += __shfl_xor(f5, m, 64);
        l5 += __shfl_xor(l5, m, 64);
        if (kPeak) {
            const int o = __shfl_xor(pk, m, 64);
            pk = o > pk ? o : pk;
        }
    }
    return HistRow{s1, s2, f5, l5, pk};
}

}  // namespace dxrl
#endif  // DXRL_HIST_ROW_H_
