// Retrieval metrics of a round of nvsm_rank's result, on the device (include/cunvsm_amd.h nvsm_evaluate).
// One wave per query; the row's arithmetic is eval_row.h's, which the alpha sweep of lexical.hip shares: nothing is atomic and
// nothing crosses a wave, a repeated call returns the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/cunvsm_amd.h"
#include "kernels.h"
#include "device_utils.h"
#include "eval_row.h"

namespace cunvsm {

static_assert(kEvalMaxCutoffs == NVSM_EVAL_MAX_CUTOFFS, "EvalArgs holds NVSM_EVAL_MAX_CUTOFFS cutoffs");

__global__ __launch_bounds__(64) void eval_metrics_kernel(EvalArgs a) {
    const int lane = threadIdx.x;
    const int q = blockIdx.x;                       // query of the round
    const int64_t gq = a.q0 + q;                    // ... of the call
    int64_t n64 = a.counts[q];
    const int n = static_cast<int>(n64 < a.k ? (n64 < 0 ? 0 : n64) : a.k);
    const int64_t* __restrict__ ids = a.ids + static_cast<size_t>(q) * a.k;
    eval_row(a, gq, n, lane, [ids](int r) { return static_cast<int>(ids[r]); }, a.metrics + gq * (NVSM_EVAL_FIXED + 3 * a.num_cutoffs));
}

void launch_eval_metrics(const EvalArgs& a, int Q, hipStream_t s) {
    if (Q <= 0) return;
    NVSM_LAUNCH(eval_metrics_kernel, dim3(Q), dim3(64), 0, s, a);
}

}  // namespace cunvsm
