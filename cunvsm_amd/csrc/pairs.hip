// The entity-entity similarity objective (RepresentationSimilarity::Objective on ENTITY_REPRS, cpp/objective.cu:485-696) for gfx950:
// forward pass and the first half of the backward pass in one launch — the role loss_rows_kernel has for the text objective.
//
// What the reference computes for a batch of M pairs (a_p, b_p, ω_p), ids interleaved features[2p], features[2p + 1]
// (cpp/data.cu:316-334):
//   rows      E[a_p], E[b_p] gathered and COPIED (objective.cu:519-521): both gradients use the rows as they were here
//   s_p       = E[a_p]·E[b_p]                                  (fold_columns + reduce_axis, :526-543)
//   prob_p    = clip(σ(s_p), 1e-7, 1 − 1e-7)                   (truncated_sigmoid, :546-550; the stable two-branch sigmoid of
//               include/cuNVSM/cuda_utils.h:193-214, in float32)
//   mass_p    = ω_p·log prob_p                                 (:553-567); cost = −(1/M)·Σ mass_p (intermediate_results.cu:81-124)
//   mult_p    = ω_p·d(prob_p)·exp(−log M), d(x) = 0 if x ≥ 1 − 1e-6 or x ≤ 1e-6, else 1 − x
//               (sigmoid_to_log_sigmoid_deriv, :607-626, cuda_utils.h:218-235)
//   gradient  column 2p = mult_p·E[b_p], column 2p + 1 = mult_p·E[a_p]   (flip_adjacent_columns + apply_columnwise, :643-661)
// No negative samples, no projection, window 1, no per-entry weights (intermediate_results.cu:300-307); gradient ASCENT.
//
// The kernel does not multiply the rows out: it writes the two rows SWAPPED as the gradient source rows of entries 2p and 2p + 1,
// their coefficient (mult_p x the mixture scale) and the source rows' means of squares — exactly what the documents table pass
// (update.hip, RowPassArgs) takes per entry —, so that the pair entries ride in the SAME sorted, atomic-free pass as the text
// objective's B·R entries. Σ ω·log prob goes through grid_sum_ordered: the same bits every run.
//
// Shape of the work: bandwidth. 2·M·d_e·4 bytes in, the same out, a dozen flops per element. A pair's two rows are read ONCE, 16 B per
// lane; a row shorter than a wave's 1 KB shares the wave with other pairs (groups of G = 2 .. 64 lanes, one pair per group and turn),
// a longer one (d_e up to 1024) takes up to four turns of the whole wave. 44-54 registers at d_e = 256: eight waves per SIMD, each with two rows
// (2 x 16 B per lane) requested per turn, is 64 KB of loads in flight per CU — twice what the memory system needs to stream.
//
// The WORDS-table form (template switch MUL; PairArgs::mul_rows): RepresentationSimilarity::Objective with param_id_ == WORD_REPRS
// (cpp/objective.cu:485-696), the term-term half of TextEntityTermTerm (:747-794). For a batch of M pairs (a_p, b_p, ω_p) of model
// word ids, interleaved:
//   s_p       = W[a_p]·W[b_p];   prob_p = clip(σ(s_p), 1e-7, 1 − 1e-7) in float32 with the two-branch sigmoid
//   cost      = −(1/M)·Σ ω_p·log prob_p;   mult_p = ω_p·d(prob_p)·exp(−log M), the derivative clamp at 1e-6
//   gradient  entry 2p = mult_p·W[b_p], entry 2p + 1 = mult_p·W[a_p], both from the rows as they were at compute_cost
// Window 1, no per-entry weights (include/cuNVSM/intermediate_results.h:328-334), gradient ascent, scaled λ = λ/M; only the words table
// has a gradient (cpp/params.cu:304-307). Mixed with the text objective: cost = (cost_text + cost_pairs)/2, scaled λ = (λ/B + λ/M)/2, the
// pair gradient scaled by w_tt/(w_te + w_tt) (MergeGradientsFn, cpp/intermediate_results.cu:3-60), ONE update of the words table from
// both gradient lists (CompositeGradients, cpp/storage.cu:65-99).
// The words table pass weighs an entry's mean of squares LINEARLY by its coefficient (update.hip: sq = c·s, because the reference
// scatters v with the same repr_weights as the gradient, updates_adam.cu:242-252), where the documents pass has c²·s. A pair entry can
// therefore not ride as "raw row + coefficient": its v share would come out as c_p·msq instead of c_p²·msq. So this form writes the
// MULTIPLIED rows X[2p] = c_p·W[b_p], X[2p + 1] = c_p·W[a_p] (c_p = mult_p x the mixture scale, one v_mul per element), the entries
// weigh 1, and sq[·] is the mean of squares of the stored rows. c_p is known in the group's last lane only, behind the reduction of the
// dot product: that lane hands it to its group (one ds_bpermute), and the squares are summed behind the multiplication.
// A bandwidth kernel like the documents-table form: 2·M·d_w·4 bytes in, the same out. Registers from the compiler's output (hipcc -O3,
// gfx950; profiles/NOTES_term_pairs.md lists every instantiation): d_w = 300 is <V = 4, NITER = 2, G = 64>, 63 VGPRs (56 with a lazily
// decayed table), d_w = 128 <4, 1, 32> 52 (44): eight waves per SIMD; four column turns (d_w 516 .. 1024) 90 (76): five (six).
#include "../../include/cunvsm_amd.h"
#include "kernels.h"
#include "device_utils.h"

#include <algorithm>
#include <string>

namespace cunvsm {

namespace {

constexpr int kPairTurns = 8;      // turns (pairs per lane group) per wave: a block's share of the loss word is one value per 4 x 8 x 64 / G pairs

// sum over the G lanes of a lane group on the DPP network; valid in the group's LAST lane (for G <= 16 and G = 64 in every lane)
template <int G>
__device__ __forceinline__ float group_sum(float v) {
    if constexpr (G == 64) return wave_sum(v);
    if constexpr (G >= 2) v += dpp_mov<0xB1, 0xf>(v);        // quad_perm [1,0,3,2]
    if constexpr (G >= 4) v += dpp_mov<0x4E, 0xf>(v);        // quad_perm [2,3,0,1]
    if constexpr (G >= 8) v += dpp_mov<0x141, 0xf>(v);       // row_half_mirror
    if constexpr (G >= 16) v += dpp_mov<0x140, 0xf>(v);      // row_mirror
    if constexpr (G >= 32) v += dpp_mov<0x142, 0xa>(v);      // row_bcast:15 -> rows 1, 3 hold the sum of their 32 lanes
    return v;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// V floats per lane and turn; NITER column turns of the group (NITER > 1 only with G = 64); LAZY: E decays lazily (LazyView);
// MUL: the words-table form (see the head of this file) — every statement it adds or leaves out sits behind `if constexpr (MUL)`
template <int V, int NITER, int G, bool LAZY, bool MUL>
__global__ __launch_bounds__(256) void pair_loss_kernel(PairArgs a) {
#pragma clang fp contract(on)
    __shared__ float hist[kLazyHistory];
    __shared__ double s_loss[4];
    __shared__ int s_flag;
    if (LAZY) {
        for (int i = threadIdx.x; i < kLazyHistory; i += 256) hist[i] = a.lazyE.decay[i];
        __syncthreads();
    }
    constexpr int kGroups = 64 / G;      // pairs per wave and turn
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int gl = lane % G, grp = lane / G;
    const bool leader = gl == G - 1;
    const int de = a.de;
    const int64_t M = a.M;
    const int64_t wave0 = (static_cast<int64_t>(blockIdx.x) * 4 + wid) * (kPairTurns * kGroups);
    int col[NITER]; bool cv[NITER];
#pragma unroll
    for (int it = 0; it < NITER; ++it) {
        const int c = (it * G + gl) * V;
        cv[it] = c < de;
        col[it] = cv[it] ? c : 0;      // (clamped: a harmless re-read, masked in the arithmetic)
    }
    const uint32_t rows = static_cast<uint32_t>(a.E_rows);
    double lane_loss = 0.0;

    auto load_ids = [&](int64_t p, uint32_t& ia, uint32_t& ib, float& w) __attribute__((always_inline)) {
        const int64_t q = p < M ? p : M - 1;
        ia = static_cast<uint32_t>(a.ids[2 * q]); ib = static_cast<uint32_t>(a.ids[2 * q + 1]);
        ia = ia < rows ? ia : 0u; ib = ib < rows ? ib : 0u;      // (the narrowing already sent bad ids to row 0 and flagged them)
        w = a.w ? a.w[q] : 1.f;
    };

    uint32_t ian, ibn; float wn;
    load_ids(wave0 + grp, ian, ibn, wn);
    for (int t = 0; t < kPairTurns; ++t) {
        const int64_t p = wave0 + static_cast<int64_t>(t) * kGroups + grp;
        if (wave0 + static_cast<int64_t>(t) * kGroups >= M) break;      // (wave-uniform)
        const bool pv = p < M;
        const uint32_t ia = ian, ib = ibn;
        const float w = wn;
        float ea[NITER][V], eb[NITER][V];
        const float* ra = a.E + static_cast<size_t>(ia) * de;
        const float* rb = a.E + static_cast<size_t>(ib) * de;
#pragma unroll
        for (int it = 0; it < NITER; ++it) { ldv<V>(ra + col[it], ea[it]); ldv<V>(rb + col[it], eb[it]); }
        int sa = 0, sb = 0;
        if (LAZY) { sa = a.lazyE.stamp[ia]; sb = a.lazyE.stamp[ib]; }
        if (t + 1 < kPairTurns) load_ids(p + kGroups, ian, ibn, wn);
        if (LAZY) {
            // the factors of the updates the row sat out, one by one, in update order: the dense passes' roundings
            for (int u = sa; u < a.lazyE.now; ++u) {
                const float d = hist[u % kLazyHistory];
#pragma unroll
                for (int it = 0; it < NITER; ++it)
#pragma unroll
                    for (int i = 0; i < V; ++i) ea[it][i] *= d;
            }
            for (int u = sb; u < a.lazyE.now; ++u) {
                const float d = hist[u % kLazyHistory];
#pragma unroll
                for (int it = 0; it < NITER; ++it)
#pragma unroll
                    for (int i = 0; i < V; ++i) eb[it][i] *= d;
            }
        }
        float dot = 0.f, qa = 0.f, qb = 0.f;
#pragma unroll
        for (int it = 0; it < NITER; ++it) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float x = cv[it] ? ea[it][i] : 0.f, y = cv[it] ? eb[it][i] : 0.f;
                dot += x * y; qa += x * x; qb += y * y;
            }
        }
        dot = group_sum<G>(dot);
        if constexpr (MUL) {
            // probability, log and coefficient once per pair, in the group's last lane, which hands the coefficient to its group
            float c = 0.f;
            if (leader && pv) {
                const float sx = dot;
                float pr = (sx >= 0.f) ? 1.f / (1.f + expf(-sx)) : expf(sx) / (1.f + expf(sx));
                pr = fminf(fmaxf(pr, a.sig_eps), a.sig_hi);
                lane_loss += static_cast<double>(logf(pr) * w);
                const float d = (static_cast<double>(pr) >= a.d_hi || pr <= a.d_eps) ? 0.f : 1.f - pr;
                c = (w * (d * a.inv_batch)) * a.scale;
                a.probs[p] = pr;
                a.mults[p] = c;
            }
            c = __shfl(c, lane | (G - 1), 64);
            // the multiplied rows (one multiplication per element) and the sums of their squares
            float ga = 0.f, gb = 0.f;
#pragma unroll
            for (int it = 0; it < NITER; ++it) {
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    ea[it][i] = c * ea[it][i]; eb[it][i] = c * eb[it][i];
                    const float x = cv[it] ? ea[it][i] : 0.f, y = cv[it] ? eb[it][i] : 0.f;
                    ga += x * x; gb += y * y;
                }
            }
            ga = group_sum<G>(ga); gb = group_sum<G>(gb);
            // swapped: entry 2p's gradient row is c·W[b_p], entry 2p + 1's is c·W[a_p]
            if (pv) {
                float* xa = a.X + static_cast<size_t>(2 * p) * de;
#pragma unroll
                for (int it = 0; it < NITER; ++it) {
                    if (cv[it]) { stv<V>(xa + col[it], eb[it]); stv<V>(xa + de + col[it], ea[it]); }
                }
            }
            if (leader && pv) {
                a.sq[2 * p] = gb * a.inv_de;
                a.sq[2 * p + 1] = ga * a.inv_de;
            }
        } else {
            qa = group_sum<G>(qa); qb = group_sum<G>(qb);
            // the rows, swapped: entry 2p's gradient source is E[b_p], entry 2p + 1's is E[a_p]
            if (pv) {
                float* xa = a.X + static_cast<size_t>(2 * p) * de;
#pragma unroll
                for (int it = 0; it < NITER; ++it) {
                    if (cv[it]) { stv<V>(xa + col[it], eb[it]); stv<V>(xa + de + col[it], ea[it]); }
                }
            }
            // probability, log and multiplier once per pair, in the group's last lane
            if (leader && pv) {
                const float sx = dot;
                float pr = (sx >= 0.f) ? 1.f / (1.f + expf(-sx)) : expf(sx) / (1.f + expf(sx));
                pr = fminf(fmaxf(pr, a.sig_eps), a.sig_hi);
                lane_loss += static_cast<double>(logf(pr) * w);
                const float d = (static_cast<double>(pr) >= a.d_hi || pr <= a.d_eps) ? 0.f : 1.f - pr;
                const float m = (w * (d * a.inv_batch)) * a.scale;
                a.probs[p] = pr;
                a.mults[p] = m;
                a.coef[static_cast<size_t>(2 * p) * a.coef_stride] = m;
                a.coef[static_cast<size_t>(2 * p + 1) * a.coef_stride] = m;
                a.sq[2 * p] = qb * a.inv_de;
                a.sq[2 * p + 1] = qa * a.inv_de;
            }
        }
    }
    const double wl = wave_sum_f64(lane_loss);
    if (lane == 0) s_loss[wid] = wl;
    __syncthreads();
    double* dst = a.loss_acc;
    grid_sum_ordered<256>(a.sums.part, a.sums.part2, a.sums.arrive, a.sums.fan, 1, static_cast<int>(blockIdx.x), static_cast<int>(gridDim.x),
                          [&](int) -> double { return (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]); },
                          [&](int i, double v) { dst[i] = v; }, &s_flag);
}

template <int V, int NITER, int G>
void launch_pair_t(const PairArgs& a, int grid, hipStream_t s) {
    if (a.mul_rows) {
        if (a.lazyE.stamp) NVSM_LAUNCH((pair_loss_kernel<V, NITER, G, true, true>), dim3(grid), dim3(256), 0, s, a);
        else NVSM_LAUNCH((pair_loss_kernel<V, NITER, G, false, true>), dim3(grid), dim3(256), 0, s, a);
        return;
    }
    if (a.lazyE.stamp) NVSM_LAUNCH((pair_loss_kernel<V, NITER, G, true, false>), dim3(grid), dim3(256), 0, s, a);
    else NVSM_LAUNCH((pair_loss_kernel<V, NITER, G, false, false>), dim3(grid), dim3(256), 0, s, a);
}

template <int V>
void launch_pair_v(const PairArgs& a, int G, int niter, int grid, hipStream_t s) {
    if (niter > 2) return launch_pair_t<V, 4, 64>(a, grid, s);
    if (niter == 2) return launch_pair_t<V, 2, 64>(a, grid, s);
    switch (G) {
        case 2: return launch_pair_t<V, 1, 2>(a, grid, s);
        case 4: return launch_pair_t<V, 1, 4>(a, grid, s);
        case 8: return launch_pair_t<V, 1, 8>(a, grid, s);
        case 16: return launch_pair_t<V, 1, 16>(a, grid, s);
        case 32: return launch_pair_t<V, 1, 32>(a, grid, s);
        default: return launch_pair_t<V, 1, 64>(a, grid, s);
    }
}

// lanes per pair and column turns for rows of `de` floats
void pair_plan(int de, int* V, int* G, int* niter) {
    *V = (de % 4 == 0) ? 4 : 1;
    const int cols = (de + *V - 1) / *V;
    int g = 2;
    while (g < cols && g < 64) g <<= 1;
    *G = g;
    *niter = (cols + 63) / 64;
}

__global__ void pair_entry_ids_kernel(int* __restrict__ vals, int64_t n_text, int64_t first_src, int R, int64_t n_pair) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n_text + n_pair; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        vals[i] = static_cast<int>(i < n_text ? i : (first_src + (i - n_text)) * R);
}

__global__ void pair_scale_weights_kernel(const float* __restrict__ w, float scale, float* __restrict__ out, int64_t n) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        out[i] = (w ? w[i] : 1.f) * scale;
}

__global__ void pair_entry_weights_kernel(const float* __restrict__ w, float* __restrict__ out, int64_t n_text, int64_t first_src, int R, int64_t n_pair) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n_text + n_pair; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        if (i < n_text) out[i] = w[i];
        else out[(first_src + (i - n_text)) * R] = 1.f;
    }
}

__global__ void pair_materialize_kernel(const float* __restrict__ coef, int coef_stride, const float* __restrict__ X, int64_t n, int de,
                                        float* __restrict__ out) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n * de; i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        out[i] = coef[(i / de) * coef_stride] * X[i];
}

}  // namespace

int pair_loss_blocks(int64_t M, int de) {
    int V, G, niter;
    pair_plan(de, &V, &G, &niter);
    const int64_t per_block = 4 * static_cast<int64_t>(kPairTurns) * (64 / G);
    return static_cast<int>((std::max<int64_t>(M, 1) + per_block - 1) / per_block);
}

void launch_pair_loss(const PairArgs& a_in, hipStream_t s) {
    if (a_in.M <= 0) return;
    const std::string dim_name = a_in.mul_rows ? "word_repr_size" : "entity_repr_size";
    if (a_in.de > 1024 || a_in.de < 1) throw Error(NVSM_ERR_UNSUPPORTED, "pair objective: " + dim_name + " must be in [1, 1024]");
    int V, G, niter;
    pair_plan(a_in.de, &V, &G, &niter);
    if (niter > 4) throw Error(NVSM_ERR_UNSUPPORTED, "pair objective: " + dim_name + " beyond 256 must be a multiple of 4");
    PairArgs a = a_in;
    const int grid = pair_loss_blocks(a.M, a.de);
    if (grid > a.sums.contrib_cap) throw Error(NVSM_ERR_INVALID_ARGUMENT, "pair objective: more pairs than the workspace was sized for");
    a.sums.fan = grid_sum_fan(grid);
    if (V == 4) launch_pair_v<4>(a, G, niter, grid, s); else launch_pair_v<1>(a, G, niter, grid, s);
}

void launch_pair_entry_ids(int* vals, int64_t n_text, int64_t first_src, int R, int64_t n_pair, hipStream_t s) {
    if (n_text + n_pair <= 0) return;
    hipLaunchKernelGGL(pair_entry_ids_kernel, dim3(stream_grid(n_text + n_pair, 256)), dim3(256), 0, s, vals, n_text, first_src, R, n_pair);
}

void launch_pair_scale_weights(const float* w, float scale, float* out, int64_t n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pair_scale_weights_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, s, w, scale, out, n);
}

void launch_pair_entry_weights(const float* w, float* out, int64_t n_text, int64_t first_src, int R, int64_t n_pair, hipStream_t s) {
    if (n_text + n_pair <= 0) return;
    hipLaunchKernelGGL(pair_entry_weights_kernel, dim3(stream_grid(n_text + n_pair, 256)), dim3(256), 0, s, w, out, n_text, first_src, R, n_pair);
}

void launch_pair_materialize(const float* coef, int coef_stride, const float* X, int64_t n, int de, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(pair_materialize_kernel, dim3(stream_grid(n * de, 256)), dim3(256), 0, s, coef, coef_stride, X, n, de, out);
}

}  // namespace cunvsm
