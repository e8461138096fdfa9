// The metric row of one ranked list, computed by ONE WAVE (eval.hip eval_metrics_kernel over a list in global memory; lexical.hip
// fuse_sweep_kernel over a list in LDS). Ranks are taken 64 at a time, lane l of block b holds rank i = 64 b + l + 1, looks its
// document up in the query's judged ids (sorted ascending by the host, one branch-free binary search per lane) and the wave turns the
// 64 grades into prefix counts (ballot + mbcnt) and fp64 sums (a fixed __shfl_xor tree). What is carried from block to block is added
// in rank order, nothing is atomic and nothing crosses a wave: the same list gives the same bits wherever its ids lie.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/cunvsm_amd.h"
#include "kernels.h"

namespace cunvsm {

__device__ __forceinline__ double eval_wave_sum(double v) {      // the tree of pairs.hip's wave_sum_f64: every lane gets the same bits
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// lanes of the block that starts at rank b0 + 1 whose rank is <= c, as a lane mask
__device__ __forceinline__ unsigned long long eval_cut_mask(long long c, int b0) {
    const long long m = c - b0;
    return m <= 0 ? 0ull : (m >= 64 ? ~0ull : ((1ull << m) - 1ull));
}

__device__ __forceinline__ double eval_ratio(double a, double b) { return b > 0.0 ? a / b : 0.0; }

// a: the judgments, constants and cutoffs of the call (ids, counts, k, metrics and q0 are not looked at). gq: the query of the call.
// The list is id_at(0) .. id_at(n - 1), n >= 0; `out` receives the row (lane 0 writes it). Every lane of the wave calls this.
template <typename IdAt>
__device__ __forceinline__ void eval_row(const EvalArgs& a, int64_t gq, int n, int lane, IdAt id_at, double* __restrict__ out) {
    const int64_t jb = a.joff[gq];
    const int len = static_cast<int>(a.joff[gq + 1] - jb);
    const int* __restrict__ jid = a.jids + jb;
    const int* __restrict__ jgr = a.jgrades + jb;
    const double* __restrict__ cst = a.consts + gq * (2 + NVSM_EVAL_MAX_CUTOFFS);      // R, idcg, idcg@c
    const double R = cst[0];
    const long long Rn = static_cast<long long>(R);
    int top = len > 0 ? 1 : 0;                      // the largest power of two <= len: the first stride of the search,
    while (top <= len / 2 && top > 0) top *= 2;     //   which then takes ceil(log2(len + 1)) steps

    int carry = 0, first = 0, at_R = 0;             // c_i up to the last block; rank of the first relevant document; c_min(R, n)
    int cut_cnt[NVSM_EVAL_MAX_CUTOFFS];
    double cut_dcg[NVSM_EVAL_MAX_CUTOFFS];
#pragma unroll
    for (int j = 0; j < NVSM_EVAL_MAX_CUTOFFS; ++j) { cut_cnt[j] = 0; cut_dcg[j] = 0.0; }
    double ap = 0.0, dcg = 0.0;

    for (int b0 = 0; b0 < n; b0 += 64) {
        const int i = b0 + lane + 1;
        const int id = i <= n ? id_at(i - 1) : -1;
        // lo = how many judged ids are < id (every lane walks the same strides: the wave stays convergent)
        int lo = 0;
        for (int w = top; w > 0; w >>= 1) {
            const int t = lo + w;
            const int at = (t < len ? t : len) - 1;
            if (t <= len && jid[at] < id) lo = t;
        }
        const int at = lo < len ? lo : (len > 0 ? len - 1 : 0);
        const bool hit = len > 0 && lo < len && jid[at] == id;
        const int g = hit ? jgr[at] : 0;
        const bool rel = g >= 1;
        const unsigned long long mask = __ballot(rel);
        const int below = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(mask), 0u));
        const int c_i = carry + below + (rel ? 1 : 0);
        const double gain = g > 0 ? static_cast<double>(g) / log2(static_cast<double>(i) + 1.0) : 0.0;
        ap += eval_wave_sum(rel ? static_cast<double>(c_i) / static_cast<double>(i) : 0.0);
        dcg += eval_wave_sum(gain);
        if (first == 0 && mask != 0ull) first = b0 + __ffsll(static_cast<long long>(mask));
        at_R += __popcll(mask & eval_cut_mask(Rn, b0));
#pragma unroll
        for (int j = 0; j < NVSM_EVAL_MAX_CUTOFFS; ++j) {
            if (j < a.num_cutoffs && b0 < a.cutoffs[j]) {      // (uniform: the whole wave takes or skips the sum)
                cut_cnt[j] += __popcll(mask & eval_cut_mask(a.cutoffs[j], b0));
                cut_dcg[j] += eval_wave_sum(i <= a.cutoffs[j] ? gain : 0.0);
            }
        }
        carry += __popcll(mask);
    }
    if (lane != 0) return;
    out[NVSM_EVAL_NUM_RET] = static_cast<double>(n);
    out[NVSM_EVAL_NUM_REL] = R;
    out[NVSM_EVAL_NUM_REL_RET] = static_cast<double>(carry);
    out[NVSM_EVAL_AP] = eval_ratio(ap, R);
    out[NVSM_EVAL_RPREC] = eval_ratio(static_cast<double>(at_R), R);
    out[NVSM_EVAL_RECIP_RANK] = first > 0 ? 1.0 / static_cast<double>(first) : 0.0;
    out[NVSM_EVAL_NDCG] = eval_ratio(dcg, cst[1]);
#pragma unroll
    for (int j = 0; j < NVSM_EVAL_MAX_CUTOFFS; ++j) {
        if (j < a.num_cutoffs) {
            out[NVSM_EVAL_FIXED + 3 * j + 0] = static_cast<double>(cut_cnt[j]) / static_cast<double>(a.cutoffs[j]);
            out[NVSM_EVAL_FIXED + 3 * j + 1] = eval_ratio(static_cast<double>(cut_cnt[j]), R);
            out[NVSM_EVAL_FIXED + 3 * j + 2] = eval_ratio(cut_dcg[j], cst[2 + j]);
        }
    }
}

}  // namespace cunvsm
