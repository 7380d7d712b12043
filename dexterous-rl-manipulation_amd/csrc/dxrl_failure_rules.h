// dxrl_failure_rules.h -- the one statement of the failure taxonomy on the device:
// FailureClassifier.classify of evaluation/failure_taxonomy.py:156-239 on the integer moments of
// an episode's contact counts (the rules, their order and the tie rows are stated in
// include/dxrl.h).  dxrl_failure_summary.hip (the failure-mode study) and dxrl_pg_val_failure.hip
// (the failure tables of a validation row) classify with this code, so the two agree bit for bit.
#pragma once
#include "dxrl_internal.h"

namespace dxrl {
namespace {

// list(FailureMode) order
enum : int { M_SLIPPAGE = 0, M_UNSTABLE = 1, M_MISALIGNMENT = 2, M_TIMEOUT = 3, M_DROPPED = 4, M_INSUFFICIENT = 5 };

struct Verdict {
    int mode, tie;
    double conf;
};

// failure_taxonomy.py:171-239 on the integer moments of the episode's contact counts
__device__ __forceinline__ Verdict classify(bool success, int len, int n, int s1, int s2, int f5, int l5, int peak,
                                            int nc, int timeout_steps, int success_threshold) {
    if (success) return Verdict{-1, 0, 0.0};  // :171-173
    if (n == 0) peak = nc;                    // :190-193 no history: max_contacts = num_contacts
    if (len >= timeout_steps) return Verdict{M_TIMEOUT, 0, 1.0};       // :196-198
    if (nc == 0 && peak > 0) return Verdict{M_DROPPED, 0, 1.0};        // :201-203
    const long long nn = n;
    const long long num = nn * (long long)s2 - (long long)s1 * (long long)s1;  // n^2 var, below 2^41
    int tie = 0;
    if (n > 5) {  // :206-222
        if (n > 10) {
            const double trend = ((double)l5 / 5.0) - ((double)f5 / 5.0);  // np.mean of five small integers
            if (trend < -1.0 && peak >= 1) return Verdict{M_SLIPPAGE, 0, fmin(1.0, fabs(trend) / 2.0)};
        }
        if (num > 2 * nn * nn) {
            const double var = (double)num / (double)(nn * nn);  // both exact: the correctly rounded variance
            return Verdict{M_UNSTABLE, 0, fmin(1.0, var / 5.0)};
        }
        tie = num == 2 * nn * nn;  // np.var's own rounding decides
    }
    if (nc >= 1 && nc <= 2) {  // :225-230 (variance 0.0 for a history of one entry or none)
        if (n <= 1 || num < nn * nn) return Verdict{M_MISALIGNMENT, tie, 0.8};
        tie |= num == nn * nn;
    }
    if (peak < success_threshold) return Verdict{M_INSUFFICIENT, tie, 1.0};  // :233-235
    return Verdict{M_INSUFFICIENT, tie, 0.5};                                 // :238-239
}

}  // namespace
}  // namespace dxrl
