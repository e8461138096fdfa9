// gfx950 kernels of query inference and top-k document ranking (kernels.h "ranking").
//
// Reference semantics (cuNVSM): Model::infer (cpp/model.cu:105-133) gathers the mean of a window's word rows and projects it
// with f(T·x + b), batch normalisation switched off (nullptr statistics, cpp/model.cu:125-128, cpp/params.cu:396-428);
// py/nvsm/base.py:297-323 does the same on the host for queries of any length with np.average (self-information weights) and
// :362-430 ranks every document, or a candidate set, by the cosine DISTANCE to that projection; py/query.py negates the
// distance, so larger is better there as it is here, where the kernels produce the cosine SIMILARITY (or the plain dot
// product) directly. A document row or a projected query of norm 0 has inverse norm 0: score 0, never NaN.
//
//   query side   rank_query_mean_kernel  ragged weighted gather-mean  Σ w·W[id] / Σ w (reads a lazily decayed table through its view)
//                launch_gemm             T·x on the exact-fp32 MFMA kernels (kernels.h)
//                rank_bias_act_kernel    + c·b, then tanh / hard-tanh / identity
//                rank_query_norm_kernel  1 / |p| per query (1 for the dot product)
//   scan         rank_scan_mfma_kernel   d_e % 64 == 0: scores of up to 128 queries against 128 documents per workgroup on
//                                        v_mfma_f32_32x32x2_f32; the row norms come out of the same registers
//                rank_scan_plain_kernel  every other d_e
//                rank_scan_cand_kernel   candidate lists: one wave per (query, candidate)
//   neighbours   nvsm_neighbors scans word rows, the projected vocabulary or document rows with the same kernels (the MFMA scan with
//                a zero-filled tail chunk where the dimension is not a multiple of 32: d_w = 300); rank_gather_rows_kernel makes
//                the query panel from row ids, rank_exclude_self_kernel drops a query's own row, rank_pair_sim_kernel scores pairs
//   selection    radix select on the order-preserving bits of the scores of one slab of documents (three histogram passes:
//                11 + 11 + 10 bits), an ORDERED compaction of the survivors (per-part counts, then positions by prefix sums: no
//                atomics decide where anything lands), and a bitonic sort of (score, ~id) keys: ties come out by ascending id.
//                The only atomics are integer additions into histogram counters, whose sums do not depend on their order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include "../../include/cunvsm_amd.h"
#include "kernels.h"
#include "device_utils.h"

namespace cunvsm {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// float -> unsigned whose order is the floats' order (larger score, larger key); -0 has been folded into +0 by the scan
__device__ __forceinline__ unsigned rank_key(float s) {
    const unsigned b = __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float rank_unkey(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
// (score key, document id) -> one 64-bit key: descending order = score descending, then id ascending
__device__ __forceinline__ unsigned long long rank_key64(unsigned u, unsigned doc) {
    return (static_cast<unsigned long long>(u) << 32) | static_cast<unsigned long long>(0xffffffffu - doc);
}

// the factors of the updates a lazily decayed row sat out, one by one in update order (kernels.h LazyView): the value
// nvsm_get_param would return for the element
__device__ __forceinline__ float rank_lazy(float x, int stamp, int now, const float* hist) {
    for (int u = stamp; u < now; ++u) x *= hist[u % kLazyHistory];
    return x;
}

// ---- query side -----------------------------------------------------------------------------------------------------------
// out[q][t] = Σ_j w_j · W[id_j][t] / Σ_j w_j over the words [offsets[q], offsets[q + 1]) of query q (np.average, base.py:305-307;
// weights null: the plain mean = average_repr_kernel with the query's length as the window). An empty query gives zeros (its
// count is 0). Ids outside [0, num_words) read row 0 and raise NVSM_BAD_WORD_ID (the handle's index contract).
__global__ __launch_bounds__(256) void rank_query_mean_kernel(const float* __restrict__ W, int dw, int64_t num_words,
                                                              const int64_t* __restrict__ ids, const float* __restrict__ wts,
                                                              const int64_t* __restrict__ offsets, float* __restrict__ out,
                                                              LazyView lazy, int* err_flag) {
    __shared__ float hist[kLazyHistory];
    if (lazy.stamp) {
        for (int i = threadIdx.x; i < kLazyHistory; i += blockDim.x) hist[i] = lazy.decay[i];
        __syncthreads();
    }
    const int q = blockIdx.x;
    const int64_t j0 = offsets[q], j1 = offsets[q + 1];
    for (int t = threadIdx.x; t < dw; t += blockDim.x) {
        float acc = 0.f, wsum = 0.f;
        for (int64_t j = j0; j < j1; ++j) {
            int64_t id = ids[j];
            if (id < 0 || id >= num_words) { id = 0; if (err_flag) *err_flag = NVSM_BAD_WORD_ID; }
            float x = W[static_cast<size_t>(id) * dw + t];
            if (lazy.stamp) x = rank_lazy(x, lazy.stamp[id], lazy.now, hist);
            const float w = wts ? wts[j] : 1.f;
            acc += w * x;
            wsum += w;
        }
        out[static_cast<size_t>(q) * dw + t] = (j1 > j0) ? acc / wsum : 0.f;
    }
}

// y = f(pre + c·b)   — no batch normalisation, whatever the handle trains with (cpp/model.cu:125-128)
__global__ __launch_bounds__(256) void rank_bias_act_kernel(float* __restrict__ y, const float* __restrict__ bias, float c, int act,
                                                            float clip_min, float clip_max, int64_t n, int de) {
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * blockDim.x) {
        y[i] = rank_bias_act(y[i], bias[i % de], c, act, clip_min, clip_max);
    }
}

// inv[q] = 1 / |P[q]| (0 for a zero row); one wave per query
__global__ __launch_bounds__(64) void rank_query_norm_kernel(const float* __restrict__ P, int de, float* __restrict__ inv, int cosine) {
    const int q = blockIdx.x;
    float s = 0.f;
    for (int t = threadIdx.x; t < de; t += 64) { const float x = P[static_cast<size_t>(q) * de + t]; s += x * x; }
    s = wave_sum(s);
    if (threadIdx.x == 0) inv[q] = cosine ? (s > 0.f ? 1.f / sqrtf(s) : 0.f) : 1.f;
}

// ---- scan, d_e % 64 == 0 ----------------------------------------------------------------------------------------------------
// A workgroup of four waves scores 128 documents against NT x 32 queries; a wave owns 32 documents. v_mfma_f32_32x32x2_f32 with
// the queries as rows and the documents as columns: lane (x = lane & 31, h = lane >> 5) feeds P[q0 + x][k] and E[d0 + x][k] for
// the SAME k, so any order of the k inside a block of eight is as good as any other: a lane loads four consecutive floats
// (k = 8 kb + 4 h + j) of its row with one 16-byte load and spends them on four MFMAs. The accumulators of a lane all belong to
// document column x, so the lane's own squares, added to those of lane x + 32, are that document's squared norm.
// The reduction over d_e runs in chunks of 32: the query panel of a chunk lies in LDS (36 floats per row: conflict-free
// 16-byte reads), in one of two buffers — while a chunk is multiplied, the next chunk's panel and document elements are on
// their way from L2 / HBM into registers, and one barrier per chunk hands the buffers over. Every chunk goes into fresh
// accumulators that are added to the totals afterwards: chains of 16 additions instead of d_e / 2, which keeps the rounding
// error of a score at that of a blocked float32 sum.
constexpr int kScanDocs = 128, kScanKc = 32, kScanLd = kScanKc + 4;

// TAIL (nvsm_neighbors only: d_w = 300 is nine chunks and a tail of 12): the reduction dimension is any multiple of 4 from 32
// up, whole chunks plus one zero-filled tail chunk. A float4 of a row lies wholly in front of or wholly behind `de`; those
// behind it — panel rows and document elements alike — are not loaded and count as 0, so the tail's MFMAs add zeros and the
// norms still come out of the same registers. Without TAIL (de % 32 == 0) no such test is compiled.
template <int NT, bool TAIL>
__global__ __launch_bounds__(256, 2) void rank_scan_mfma_kernel(const float* __restrict__ E, int de, int64_t d_begin, int S,
                                                             const float* __restrict__ P, int Q, const float* __restrict__ qinv,
                                                             float* __restrict__ scores, int64_t ld_scores, int cosine, LazyView lazy) {
    __shared__ float Ps[2][NT * 32 * kScanLd];
    __shared__ float hist[kLazyHistory];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, x = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.y * (NT * 32);
    const int i0 = blockIdx.x * kScanDocs + wave * 32;                 // first document of the wave, inside the slab
    const int mine = min(i0 + x, S - 1);                               // (past the slab: its last row again, never stored)
    const int64_t doc = d_begin + mine;
    const float* row = E + static_cast<size_t>(doc) * de + 4 * h;
    int stamp = 0;
    if (lazy.stamp) {
        for (int i = threadIdx.x; i < kLazyHistory; i += blockDim.x) hist[i] = lazy.decay[i];
        stamp = lazy.stamp[doc];
    }
    // the panel of a chunk is NT x 32 rows of eight float4: NT float4 per thread
    auto load_panel = [&](int kc, float (&pn)[NT][4]) {
#pragma unroll
        for (int it = 0; it < NT; ++it) {
            const int f = threadIdx.x + it * 256, r = f >> 3, c4 = (f & 7) * 4;
#pragma unroll
            for (int j = 0; j < 4; ++j) pn[it][j] = 0.f;
            if (q0 + r < Q && (!TAIL || kc + c4 < de)) ldv<4>(P + static_cast<size_t>(q0 + r) * de + kc + c4, pn[it]);
        }
    };
    auto store_panel = [&](int buf, const float (&pn)[NT][4]) {
#pragma unroll
        for (int it = 0; it < NT; ++it) {
            const int f = threadIdx.x + it * 256, r = f >> 3, c4 = (f & 7) * 4;
            stv<4>(&Ps[buf][r * kScanLd + c4], pn[it]);
        }
    };
    auto load_rows = [&](int kc, float (&e)[kScanKc / 8][4]) {
#pragma unroll
        for (int kb = 0; kb < kScanKc / 8; ++kb) {
            if constexpr (TAIL) {
#pragma unroll
                for (int j = 0; j < 4; ++j) e[kb][j] = 0.f;
                if (kc + 8 * kb + 4 * h < de) ldv<4>(row + kc + 8 * kb, e[kb]);
            } else {
                ldv<4>(row + kc + 8 * kb, e[kb]);
            }
        }
    };
    f32x16 tot[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[t][r] = 0.f;
    float sq[4] = {0.f, 0.f, 0.f, 0.f};

    float pn[NT][4], e[kScanKc / 8][4], en[kScanKc / 8][4];
    load_panel(0, pn);
    load_rows(0, e);
    store_panel(0, pn);
    __syncthreads();
    const int chunks = TAIL ? (de + kScanKc - 1) / kScanKc : de / kScanKc;
    for (int c = 0; c < chunks; ++c) {
        const bool more = c + 1 < chunks;
        if (more) { load_panel((c + 1) * kScanKc, pn); load_rows((c + 1) * kScanKc, en); }
        if (lazy.stamp) {
#pragma unroll
            for (int kb = 0; kb < kScanKc / 8; ++kb)
#pragma unroll
                for (int j = 0; j < 4; ++j) e[kb][j] = rank_lazy(e[kb][j], stamp, lazy.now, hist);
        }
        const float* panel = Ps[c & 1];
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
        for (int kb = 0; kb < kScanKc / 8; ++kb) {
#pragma unroll
            for (int j = 0; j < 4; ++j) sq[j] += e[kb][j] * e[kb][j];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float p[4];
                ldv<4>(panel + (t * 32 + x) * kScanLd + 8 * kb + 4 * h, p);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[j], e[kb][j], acc[t], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[t][r] += acc[t][r];
        if (more) {
            store_panel((c + 1) & 1, pn);      // (last read in the chunk before this one: every wave is past it)
#pragma unroll
            for (int kb = 0; kb < kScanKc / 8; ++kb)
#pragma unroll
                for (int j = 0; j < 4; ++j) e[kb][j] = en[kb][j];
        }
        __syncthreads();
    }
    float nsq = (sq[0] + sq[1]) + (sq[2] + sq[3]);
    nsq += __shfl_xor(nsq, 32);
    const float dinv = cosine ? (nsq > 0.f ? 1.f / sqrtf(nsq) : 0.f) : 1.f;
    if (i0 + x >= S) return;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + t * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (q < Q) {
                const float s = cosine ? tot[t][r] * dinv * qinv[q] : tot[t][r];
                scores[static_cast<size_t>(q) * ld_scores + i0 + x] = s + 0.f;      // (+ 0: -0 becomes +0, one key per value)
            }
        }
}

// ---- scan, any d_e ----------------------------------------------------------------------------------------------------------
// a thread owns one document and kPlainQ queries (their rows in LDS); four partial sums per score, eight elements apart
constexpr int kPlainQ = 8;
__global__ __launch_bounds__(256) void rank_scan_plain_kernel(const float* __restrict__ E, int de, int64_t d_begin, int S,
                                                              const float* __restrict__ P, int Q, const float* __restrict__ qinv,
                                                              float* __restrict__ scores, int64_t ld_scores, int cosine, LazyView lazy) {
    extern __shared__ float Pq[];                                       // [kPlainQ][de]
    __shared__ float hist[kLazyHistory];
    const int q0 = blockIdx.y * kPlainQ;
    for (int f = threadIdx.x; f < kPlainQ * de; f += 256) {
        const int r = f / de, t = f - r * de;
        Pq[f] = (q0 + r < Q) ? P[static_cast<size_t>(q0 + r) * de + t] : 0.f;
    }
    if (lazy.stamp) for (int i = threadIdx.x; i < kLazyHistory; i += blockDim.x) hist[i] = lazy.decay[i];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const int64_t doc = d_begin + i;
    const float* row = E + static_cast<size_t>(doc) * de;
    const int stamp = lazy.stamp ? lazy.stamp[doc] : 0;
    float acc[kPlainQ][4], sq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < kPlainQ; ++r)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[r][u] = 0.f;
    for (int t0 = 0; t0 < de; t0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u;
            if (t < de) {
                float xv = row[t];
                if (lazy.stamp) xv = rank_lazy(xv, stamp, lazy.now, hist);
                sq[u] += xv * xv;
#pragma unroll
                for (int r = 0; r < kPlainQ; ++r) acc[r][u] += xv * Pq[r * de + t];
            }
        }
    }
    const float nsq = (sq[0] + sq[1]) + (sq[2] + sq[3]);
    const float dinv = cosine ? (nsq > 0.f ? 1.f / sqrtf(nsq) : 0.f) : 1.f;
#pragma unroll
    for (int r = 0; r < kPlainQ; ++r) {
        if (q0 + r < Q) {
            const float d = (acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3]);
            const float s = cosine ? d * dinv * qinv[q0 + r] : d;
            scores[static_cast<size_t>(q0 + r) * ld_scores + i] = s + 0.f;
        }
    }
}

// ---- scan of candidate lists --------------------------------------------------------------------------------------------------
// keys[q][j] = (score of candidate j of query q, ~id) for j < n_q, 0 (below every real key) behind; one wave per slot.
// cand: the queries' DISTINCT candidates, ascending, concatenated; cand_off [Q + 1]
__global__ __launch_bounds__(64) void rank_scan_cand_kernel(const float* __restrict__ E, int de, const float* __restrict__ P,
                                                            const float* __restrict__ qinv, const int* __restrict__ cand,
                                                            const int64_t* __restrict__ cand_off, unsigned long long* __restrict__ keys,
                                                            int64_t npad, int cosine, LazyView lazy) {
    __shared__ float hist[kLazyHistory];
    if (lazy.stamp) {
        for (int i = threadIdx.x; i < kLazyHistory; i += blockDim.x) hist[i] = lazy.decay[i];
        __syncthreads();
    }
    const int q = blockIdx.y;
    const int64_t j = blockIdx.x;
    const int64_t n = cand_off[q + 1] - cand_off[q];
    unsigned long long* out = keys + static_cast<size_t>(q) * npad + j;
    if (j >= n) { if (threadIdx.x == 0) *out = 0ull; return; }
    const int doc = cand[cand_off[q] + j];
    const float* row = E + static_cast<size_t>(doc) * de;
    const float* p = P + static_cast<size_t>(q) * de;
    const int stamp = lazy.stamp ? lazy.stamp[doc] : 0;
    float d = 0.f, sq = 0.f;
    for (int t = threadIdx.x; t < de; t += 64) {
        float xv = row[t];
        if (lazy.stamp) xv = rank_lazy(xv, stamp, lazy.now, hist);
        d += xv * p[t];
        sq += xv * xv;
    }
    d = wave_sum(d);
    sq = wave_sum(sq);
    if (threadIdx.x == 0) {
        const float dinv = cosine ? (sq > 0.f ? 1.f / sqrtf(sq) : 0.f) : 1.f;
        const float s = (cosine ? d * dinv * qinv[q] : d) + 0.f;
        *out = rank_key64(rank_key(s), static_cast<unsigned>(doc));
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------------
constexpr int kSelBins = 2048;
constexpr int kSelBlockMin = 4096, kSelBlockMax = 32768;      // scores of a histogram workgroup (its 8 K counters want many)
constexpr int kSelPart = 1024;             // scores of a wave in the count and emit kernels: 16 per lane
constexpr int kSelCopies = 4;              // LDS copies of a workgroup's histogram (see rank_sel_hist_kernel)
struct SelState { unsigned prefix; unsigned mask; int need; int pad; };      // per query: bits of the k-th key fixed so far, ranks still wanted

// the keys of scores i .. i + 3 of a row (rows start 16-byte aligned: ld_scores % 4 == 0); past the slab: key 0 and in = false
__device__ __forceinline__ void rank_keys4(const float* __restrict__ sc, int i, int S, unsigned (&u)[4], bool (&in)[4]) {
    if (i + 3 < S) {
        const float4 v = *reinterpret_cast<const float4*>(sc + i);
        u[0] = rank_key(v.x); u[1] = rank_key(v.y); u[2] = rank_key(v.z); u[3] = rank_key(v.w);
        in[0] = in[1] = in[2] = in[3] = true;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) { in[c] = i + c < S; u[c] = in[c] ? rank_key(sc[i + c]) : 0u; }
    }
}

__global__ __launch_bounds__(256) void rank_sel_init_kernel(SelState* st, int* hist, int Q, int k) {
    const int q = blockIdx.x;
    if (threadIdx.x == 0) st[q] = SelState{0u, 0u, k, 0};
    for (int b = threadIdx.x; b < kSelBins; b += 256) hist[static_cast<size_t>(q) * kSelBins + b] = 0;
}

// histogram of bits [shift, shift + bits) of the keys that agree with the prefix found so far. Scores crowd into a handful of
// the first pass's bins (sign, exponent, two mantissa bits), and LDS atomics of a wave on one address take turns: a lane adds a
// run of equal bins at once, and neighbouring lanes add into different copies of the histogram.
__global__ __launch_bounds__(256) void rank_sel_hist_kernel(const float* __restrict__ scores, int64_t ld_scores, int S,
                                                            const SelState* __restrict__ st, int* __restrict__ hist, int shift, int bits,
                                                            int per_block) {
    __shared__ int h[kSelCopies][kSelBins];
    const int q = blockIdx.y;
    for (int b = threadIdx.x; b < kSelCopies * kSelBins; b += 256) (&h[0][0])[b] = 0;
    __syncthreads();
    const SelState s = st[q];
    const float* sc = scores + static_cast<size_t>(q) * ld_scores;
    const int base = blockIdx.x * per_block;
    const unsigned binmask = (1u << bits) - 1u;
    int* mine = h[threadIdx.x & (kSelCopies - 1)];
    int run_bin = -1, run = 0;
    for (int i = base + threadIdx.x * 4; i < min(base + per_block, S); i += 1024) {
        unsigned u[4]; bool in[4];
        rank_keys4(sc, i, S, u, in);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!in[c] || (u[c] & s.mask) != s.prefix) continue;
            const int bin = static_cast<int>((u[c] >> shift) & binmask);
            if (bin == run_bin) { ++run; continue; }
            if (run) atomicAdd(&mine[run_bin], run);
            run_bin = bin; run = 1;
        }
    }
    if (run) atomicAdd(&mine[run_bin], run);
    __syncthreads();
    for (int b = threadIdx.x; b < kSelBins; b += 256) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < kSelCopies; ++j) c += h[j][b];
        if (c) atomicAdd(&hist[static_cast<size_t>(q) * kSelBins + b], c);
    }
}

// the bin that holds the `need`-th largest key among those counted; the histogram is cleared for the next pass
__global__ __launch_bounds__(256) void rank_sel_pick_kernel(SelState* st, int* __restrict__ hist, int shift, int bits) {
    __shared__ int part[256];
    __shared__ int above[256];
    const int q = blockIdx.x;
    int* h = hist + static_cast<size_t>(q) * kSelBins;
    // thread t owns the eight bins 2047 - 8 t .. 2040 - 8 t (descending keys)
    int mine[8], sum = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { mine[j] = h[kSelBins - 1 - (8 * threadIdx.x + j)]; sum += mine[j]; }
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) { above[t] = run; run += part[t]; }
    }
    __syncthreads();
    SelState s = st[q];
    int run = above[threadIdx.x];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (run < s.need && s.need <= run + mine[j]) {                 // exactly one (thread, j) in the block
            const unsigned bin = static_cast<unsigned>(kSelBins - 1 - (8 * threadIdx.x + j));
            s.prefix |= bin << shift;
            s.mask |= ((1u << bits) - 1u) << shift;
            s.need -= run;
            st[q] = s;
        }
        run += mine[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) h[kSelBins - 1 - (8 * threadIdx.x + j)] = 0;
}

__device__ __forceinline__ int wave_sum_int(int v) {      // (integer sums: any order gives the same total)
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// per part (the kSelPart scores of one wave): how many keys lie above the k-th key, how many equal it
__global__ __launch_bounds__(256) void rank_sel_count_kernel(const float* __restrict__ scores, int64_t ld_scores, int S,
                                                             const SelState* __restrict__ st, int2* __restrict__ counts, int parts) {
    const int q = blockIdx.y, lane = threadIdx.x & 63;
    const int part = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (part >= parts) return;
    const unsigned v = st[q].prefix;
    const float* sc = scores + static_cast<size_t>(q) * ld_scores;
    const int base = part * kSelPart;
    int g = 0, e = 0;
    for (int i = base + lane * 4; i < min(base + kSelPart, S); i += 256) {
        unsigned u[4]; bool in[4];
        rank_keys4(sc, i, S, u, in);
#pragma unroll
        for (int c = 0; c < 4; ++c) { g += in[c] && u[c] > v; e += in[c] && u[c] == v; }
    }
    g = wave_sum_int(g); e = wave_sum_int(e);
    if (lane == 0) counts[static_cast<size_t>(q) * parts + part] = make_int2(g, e);
}

// the survivors of query q in document order: the g keys above the k-th key to out[0 .. g), of the keys equal to it the
// `need` lowest documents to out[g .. k). A wave finds its positions from the counts of the parts in front of its own and
// the lanes in front of each lane (ballots): no barrier, and no atomic decides where anything lands.
__global__ __launch_bounds__(256) void rank_sel_emit_kernel(const float* __restrict__ scores, int64_t ld_scores, int S, int64_t d_begin,
                                                            const SelState* __restrict__ st, const int2* __restrict__ counts, int parts,
                                                            int k, unsigned long long* __restrict__ keys, int64_t ld_keys, int64_t key_off) {
    const int q = blockIdx.y, lane = threadIdx.x & 63;
    const int part = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (part >= parts) return;
    const int2* cq = counts + static_cast<size_t>(q) * parts;
    const int2 own = cq[part];
    const SelState s = st[q];
    const int g_total = k - s.need;
    if (own.x == 0 && own.y == 0) return;
    int at_g = 0, at_e = 0;
    for (int p = lane; p < part; p += 64) { const int2 c = cq[p]; at_g += c.x; at_e += c.y; }
    at_g = wave_sum_int(at_g); at_e = wave_sum_int(at_e);
    if (own.x == 0 && at_e >= s.need) return;                          // (the equal keys wanted all lie in front)
    const float* sc = scores + static_cast<size_t>(q) * ld_scores;
    unsigned long long* out = keys + static_cast<size_t>(q) * ld_keys + key_off;
    const unsigned long long lower = (1ull << lane) - 1ull;
    const int base = part * kSelPart;
    // a lane owns four consecutive documents of each step of 256: in front of its document c lie the documents of the lanes below
    // (all four ballots) and its own documents below c
    for (int i0 = base; i0 < min(base + kSelPart, S); i0 += 256) {
        const int i = i0 + lane * 4;
        unsigned u[4]; bool in[4];
        rank_keys4(sc, i, S, u, in);
        int before_g = 0, before_e = 0, all_g = 0, all_e = 0;
        bool is_g[4], is_e[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            is_g[c] = in[c] && u[c] > s.prefix; is_e[c] = in[c] && u[c] == s.prefix;
            const unsigned long long mg = __ballot(is_g[c]), me = __ballot(is_e[c]);
            before_g += __popcll(mg & lower); before_e += __popcll(me & lower);
            all_g += __popcll(mg); all_e += __popcll(me);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (is_g[c]) out[at_g + before_g] = rank_key64(u[c], static_cast<unsigned>(d_begin + i + c));
            if (is_e[c] && at_e + before_e < s.need) out[g_total + at_e + before_e] = rank_key64(u[c], static_cast<unsigned>(d_begin + i + c));
            before_g += is_g[c]; before_e += is_e[c];
        }
        at_g += all_g; at_e += all_e;
    }
}

// k >= the slab: every document of it is a survivor
__global__ __launch_bounds__(256) void rank_sel_all_kernel(const float* __restrict__ scores, int64_t ld_scores, int S, int64_t d_begin,
                                                           unsigned long long* __restrict__ keys, int64_t ld_keys, int64_t key_off) {
    const int q = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    keys[static_cast<size_t>(q) * ld_keys + key_off + i] =
        rank_key64(rank_key(scores[static_cast<size_t>(q) * ld_scores + i]), static_cast<unsigned>(d_begin + i));
}

__global__ __launch_bounds__(256) void rank_fill_keys_kernel(unsigned long long* keys, int64_t ld_keys, int64_t from, int64_t to) {
    const int q = blockIdx.y;
    for (int64_t i = from + blockIdx.x * 256 + threadIdx.x; i < to; i += static_cast<int64_t>(gridDim.x) * 256)
        keys[static_cast<size_t>(q) * ld_keys + i] = 0ull;
}

// ---- sort (bitonic, descending) -------------------------------------------------------------------------------------------------
// element i of a query's npad keys (a power of two) meets element i ^ j at level k; the run that holds i is descending when
// (i & k) == 0, which at the last level k = npad is every run. A workgroup holds `chunk` consecutive keys in LDS and runs every
// step with j < chunk of the levels k_lo .. k_hi there; the steps with j >= chunk are rank_sort_global_kernel's, one launch each.
constexpr int kSortChunk = 8192;
__global__ __launch_bounds__(256) void rank_sort_lds_kernel(unsigned long long* __restrict__ keys, int64_t npad, int chunk,
                                                            int64_t k_lo, int64_t k_hi) {
    extern __shared__ unsigned long long sk[];
    const int q = blockIdx.y;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * chunk;
    unsigned long long* g = keys + static_cast<size_t>(q) * npad + base;
    for (int i = threadIdx.x; i < chunk; i += 256) sk[i] = g[i];
    __syncthreads();
    for (int64_t k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = static_cast<int>(min<int64_t>(k >> 1, chunk >> 1)); j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < chunk / 2; p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));      // the lower element of pair p
                const int l = i | j;
                const bool desc = ((base + i) & k) == 0;
                const unsigned long long a = sk[i], b = sk[l];
                if (desc ? a < b : a > b) { sk[i] = b; sk[l] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < chunk; i += 256) g[i] = sk[i];
}
__global__ __launch_bounds__(256) void rank_sort_global_kernel(unsigned long long* __restrict__ keys, int64_t npad, int64_t k, int64_t j) {
    const int q = blockIdx.y;
    unsigned long long* g = keys + static_cast<size_t>(q) * npad;
    for (int64_t p = blockIdx.x * 256ll + threadIdx.x; p < npad / 2; p += static_cast<int64_t>(gridDim.x) * 256) {
        const int64_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int64_t l = i | j;
        const bool desc = (i & k) == 0;
        const unsigned long long a = g[i], b = g[l];
        if (desc ? a < b : a > b) { g[i] = b; g[l] = a; }
    }
}

// the first min(k, n_q) sorted keys of every query as (id, score); (-1, -inf) behind them
__global__ __launch_bounds__(256) void rank_write_kernel(const unsigned long long* __restrict__ keys, int64_t npad, int k,
                                                         const int64_t* __restrict__ cand_off, int64_t n_all,
                                                         int64_t* __restrict__ ids, float* __restrict__ scores, int64_t* __restrict__ counts) {
    const int q = blockIdx.y;
    const int64_t n = cand_off ? cand_off[q + 1] - cand_off[q] : n_all;
    const int64_t cnt = n < k ? n : k;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[q] = cnt;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < k; i += gridDim.x * 256) {
        const size_t o = static_cast<size_t>(q) * k + i;
        if (i < cnt) {
            const unsigned long long key = keys[static_cast<size_t>(q) * npad + i];
            ids[o] = static_cast<int64_t>(0xffffffffu - static_cast<unsigned>(key & 0xffffffffull));
            scores[o] = rank_unkey(static_cast<unsigned>(key >> 32));
        } else {
            ids[o] = -1;
            scores[o] = -__builtin_inff();
        }
    }
}

// ---- nearest neighbours (nvsm_neighbors / nvsm_similarity) --------------------------------------------------------
// out[q] = row ids[q] of a table at its logical values (ids null: rows first, first + 1, ...); the [Q][dim] panel the scans read
__global__ __launch_bounds__(256) void rank_gather_rows_kernel(const float* __restrict__ table, int dim, const int64_t* __restrict__ ids,
                                                               int64_t first, float* __restrict__ out, LazyView lazy) {
    __shared__ float hist[kLazyHistory];
    if (lazy.stamp) {
        for (int i = threadIdx.x; i < kLazyHistory; i += blockDim.x) hist[i] = lazy.decay[i];
        __syncthreads();
    }
    const int q = blockIdx.x;
    const int64_t id = ids ? ids[q] : first + q;
    const int stamp = lazy.stamp ? lazy.stamp[id] : 0;
    for (int t = threadIdx.x; t < dim; t += blockDim.x) {
        float x = table[static_cast<size_t>(id) * dim + t];
        if (lazy.stamp) x = rank_lazy(x, stamp, lazy.now, hist);
        out[static_cast<size_t>(q) * dim + t] = x;
    }
}

// exclude_self: the score of a query's own row becomes -inf behind the scan, below every score of another row, so the
// selection and the sort leave it last and rank_write_kernel writes one slot fewer. self[q] < 0: nothing to leave out.
__global__ __launch_bounds__(256) void rank_exclude_self_kernel(float* __restrict__ scores, int64_t ld_scores, int64_t d_begin, int S,
                                                                const int64_t* __restrict__ self, int Q) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const int64_t i = self[q] - d_begin;
    if (self[q] >= 0 && i >= 0 && i < S) scores[static_cast<size_t>(q) * ld_scores + i] = -__builtin_inff();
}

// out[i] = similarity of rows a[i] and b[i] of one table (term_similarity, base.py:344-353, batched); one wave per pair
__global__ __launch_bounds__(64) void rank_pair_sim_kernel(const float* __restrict__ table, int dim, const int64_t* __restrict__ a,
                                                           const int64_t* __restrict__ b, float* __restrict__ out, int cosine, LazyView lazy) {
    __shared__ float hist[kLazyHistory];
    if (lazy.stamp) {
        for (int i = threadIdx.x; i < kLazyHistory; i += blockDim.x) hist[i] = lazy.decay[i];
        __syncthreads();
    }
    const int64_t ia = a[blockIdx.x], ib = b[blockIdx.x];
    const float* ra = table + static_cast<size_t>(ia) * dim;
    const float* rb = table + static_cast<size_t>(ib) * dim;
    const int sa = lazy.stamp ? lazy.stamp[ia] : 0, sb = lazy.stamp ? lazy.stamp[ib] : 0;
    float d = 0.f, na = 0.f, nb = 0.f;
    for (int t = threadIdx.x; t < dim; t += 64) {
        float x = ra[t], y = rb[t];
        if (lazy.stamp) { x = rank_lazy(x, sa, lazy.now, hist); y = rank_lazy(y, sb, lazy.now, hist); }
        d += x * y; na += x * x; nb += y * y;
    }
    d = wave_sum(d); na = wave_sum(na); nb = wave_sum(nb);
    if (threadIdx.x == 0) {
        const float ainv = na > 0.f ? 1.f / sqrtf(na) : 0.f, binv = nb > 0.f ? 1.f / sqrtf(nb) : 0.f;
        out[blockIdx.x] = (cosine ? d * ainv * binv : d) + 0.f;
    }
}

inline int cdiv(int64_t a, int64_t b) { return static_cast<int>((a + b - 1) / b); }

}  // namespace

void launch_rank_query_mean(const float* W, int dw, int64_t num_words, const int64_t* ids, const float* wts, const int64_t* offsets,
                            int64_t Q, float* out, const LazyView& lazy, int* err_flag, hipStream_t s) {
    if (Q <= 0) return;
    NVSM_LAUNCH(rank_query_mean_kernel, dim3(static_cast<unsigned>(Q)), dim3(256), 0, s, W, dw, num_words, ids, wts, offsets, out, lazy, err_flag);
}

void launch_rank_bias_act(float* y, const float* bias, float c, int act, int64_t Q, int de, hipStream_t s) {
    if (Q <= 0) return;
    const int64_t n = Q * de;
    const float lo = std::nextafter(-1.0f, -1.0f - 1e-5f), hi = std::nextafter(1.0f, 1.0f + 1e-5f);      // as the loss kernel's hard_tanh (cuda_utils.h:91-96)
    NVSM_LAUNCH(rank_bias_act_kernel, dim3(std::min<int64_t>(cdiv(n, 256), 4096)), dim3(256), 0, s, y, bias, c, act, lo, hi, n, de);
}

void launch_rank_query_norm(const float* P, int64_t Q, int de, float* inv, int cosine, hipStream_t s) {
    if (Q <= 0) return;
    NVSM_LAUNCH(rank_query_norm_kernel, dim3(static_cast<unsigned>(Q)), dim3(64), 0, s, P, de, inv, cosine);
}

bool rank_scan_uses_mfma(int de) { return de % 64 == 0; }

void launch_rank_scan(const float* E, int de, int64_t d_begin, int S, const float* P, int Q, const float* qinv, float* scores,
                      int64_t ld_scores, int cosine, const LazyView& lazy, hipStream_t s) {
    if (Q <= 0 || S <= 0) return;
    if (rank_scan_uses_mfma(de)) {
        // query tiles of a workgroup: all of a small batch; 128 queries a group beyond (the table is then read once per group:
        // from 48 queries on the pass is bound by the matrix pipe, not by HBM)
        const int nt = Q <= 32 ? 1 : (Q <= 64 ? 2 : 4);
        const dim3 grid(cdiv(S, kScanDocs), cdiv(Q, nt * 32));
        auto kernel = nt == 1 ? rank_scan_mfma_kernel<1, false> : (nt == 2 ? rank_scan_mfma_kernel<2, false> : rank_scan_mfma_kernel<4, false>);
        NVSM_LAUNCH(kernel, grid, dim3(256), 0, s, E, de, d_begin, S, P, Q, qinv, scores, ld_scores, cosine, lazy);
    } else {
        const dim3 grid(cdiv(S, 256), cdiv(Q, kPlainQ));
        NVSM_LAUNCH(rank_scan_plain_kernel, grid, dim3(256), static_cast<size_t>(kPlainQ) * de * sizeof(float), s, E, de, d_begin, S, P, Q,
                    qinv, scores, ld_scores, cosine, lazy);
    }
}

// nvsm_neighbors' scan: the MFMA kernel for every dimension that is a multiple of 4 from 32 up (with the tail chunk where it is
// not a multiple of 32), the plain kernel for the rest. nvsm_rank keeps rank_scan_uses_mfma (de % 64 == 0).
namespace { bool g_nbr_force_plain = false; }
void set_nbr_scan_force_plain(bool on) { g_nbr_force_plain = on; }
bool nbr_scan_uses_mfma(int dim) { return dim % 4 == 0 && dim >= kScanKc && !g_nbr_force_plain; }

void launch_nbr_scan(const float* E, int dim, int64_t d_begin, int S, const float* P, int Q, const float* qinv, float* scores,
                     int64_t ld_scores, int cosine, const LazyView& lazy, hipStream_t s) {
    if (Q <= 0 || S <= 0) return;
    if (!nbr_scan_uses_mfma(dim)) {
        const dim3 grid(cdiv(S, 256), cdiv(Q, kPlainQ));
        NVSM_LAUNCH(rank_scan_plain_kernel, grid, dim3(256), static_cast<size_t>(kPlainQ) * dim * sizeof(float), s, E, dim, d_begin, S, P, Q,
                    qinv, scores, ld_scores, cosine, lazy);
        return;
    }
    const int nt = Q <= 32 ? 1 : (Q <= 64 ? 2 : 4);
    const dim3 grid(cdiv(S, kScanDocs), cdiv(Q, nt * 32));
    const bool tail = dim % kScanKc != 0;
    auto kernel = rank_scan_mfma_kernel<1, false>;
    if (tail) kernel = nt == 1 ? rank_scan_mfma_kernel<1, true> : (nt == 2 ? rank_scan_mfma_kernel<2, true> : rank_scan_mfma_kernel<4, true>);
    else kernel = nt == 1 ? rank_scan_mfma_kernel<1, false> : (nt == 2 ? rank_scan_mfma_kernel<2, false> : rank_scan_mfma_kernel<4, false>);
    NVSM_LAUNCH(kernel, grid, dim3(256), 0, s, E, dim, d_begin, S, P, Q, qinv, scores, ld_scores, cosine, lazy);
}

void launch_rank_gather_rows(const float* table, int dim, const int64_t* ids, int64_t first, int64_t Q, float* out, const LazyView& lazy, hipStream_t s) {
    if (Q <= 0) return;
    NVSM_LAUNCH(rank_gather_rows_kernel, dim3(static_cast<unsigned>(Q)), dim3(256), 0, s, table, dim, ids, first, out, lazy);
}

void launch_rank_exclude_self(float* scores, int64_t ld_scores, int64_t d_begin, int S, const int64_t* self, int Q, hipStream_t s) {
    if (Q <= 0 || S <= 0) return;
    NVSM_LAUNCH(rank_exclude_self_kernel, dim3(cdiv(Q, 256)), dim3(256), 0, s, scores, ld_scores, d_begin, S, self, Q);
}

void launch_rank_pair_sim(const float* table, int dim, const int64_t* a, const int64_t* b, int64_t n, float* out, int cosine,
                          const LazyView& lazy, hipStream_t s) {
    if (n <= 0) return;
    NVSM_LAUNCH(rank_pair_sim_kernel, dim3(static_cast<unsigned>(n)), dim3(64), 0, s, table, dim, a, b, out, cosine, lazy);
}

void launch_rank_scan_candidates(const float* E, int de, const float* P, const float* qinv, const int* cand, const int64_t* cand_off,
                                 int Q, int64_t npad, unsigned long long* keys, int cosine, const LazyView& lazy, hipStream_t s) {
    if (Q <= 0 || npad <= 0) return;
    NVSM_LAUNCH(rank_scan_cand_kernel, dim3(static_cast<unsigned>(npad), Q), dim3(64), 0, s, E, de, P, qinv, cand, cand_off, keys, npad, cosine, lazy);
}

size_t rank_select_ws_bytes(int Q, int S) {
    return static_cast<size_t>(Q) * (sizeof(SelState) + kSelBins * sizeof(int) + static_cast<size_t>(cdiv(S, kSelPart)) * sizeof(int2)) + 256;
}

bool launch_rank_select(const float* scores, int64_t ld_scores, int S, int64_t d_begin, int Q, int k, void* ws,
                        unsigned long long* keys, int64_t ld_keys, int64_t key_off, hipStream_t s) {
    if (Q <= 0 || S <= 0) return false;
    if (k >= S) {
        NVSM_LAUNCH(rank_sel_all_kernel, dim3(cdiv(S, 256), Q), dim3(256), 0, s, scores, ld_scores, S, d_begin, keys, ld_keys, key_off);
        return false;
    }
    const int parts = cdiv(S, kSelPart);
    SelState* st = static_cast<SelState*>(ws);
    int* hist = reinterpret_cast<int*>(st + Q);
    int2* counts = reinterpret_cast<int2*>(hist + static_cast<size_t>(Q) * kSelBins);
    NVSM_LAUNCH(rank_sel_init_kernel, dim3(Q), dim3(256), 0, s, st, hist, Q, k);
    const int shift[3] = {21, 10, 0}, bits[3] = {11, 11, 10};
    // scores per histogram workgroup: about two thousand workgroups in all, so that clearing and adding up a workgroup's counters
    // is small beside its scores
    int per_block = static_cast<int>(std::min<int64_t>(kSelBlockMax, std::max<int64_t>(kSelBlockMin, static_cast<int64_t>(S) * Q / 2048)));
    per_block = (per_block + 1023) / 1024 * 1024;
    for (int p = 0; p < 3; ++p) {
        NVSM_LAUNCH(rank_sel_hist_kernel, dim3(cdiv(S, per_block), Q), dim3(256), 0, s, scores, ld_scores, S, st, hist, shift[p], bits[p], per_block);
        NVSM_LAUNCH(rank_sel_pick_kernel, dim3(Q), dim3(256), 0, s, st, hist, shift[p], bits[p]);
    }
    NVSM_LAUNCH(rank_sel_count_kernel, dim3(cdiv(parts, 4), Q), dim3(256), 0, s, scores, ld_scores, S, st, counts, parts);
    NVSM_LAUNCH(rank_sel_emit_kernel, dim3(cdiv(parts, 4), Q), dim3(256), 0, s, scores, ld_scores, S, d_begin, st, counts, parts, k, keys, ld_keys, key_off);
    return true;
}

void launch_rank_fill_keys(unsigned long long* keys, int64_t ld_keys, int64_t from, int64_t to, int Q, hipStream_t s) {
    if (Q <= 0 || to <= from) return;
    NVSM_LAUNCH(rank_fill_keys_kernel, dim3(std::min<int64_t>(cdiv(to - from, 256), 1024), Q), dim3(256), 0, s, keys, ld_keys, from, to);
}

bool launch_rank_sort(unsigned long long* keys, int64_t npad, int Q, hipStream_t s) {
    if (Q <= 0 || npad <= 1) return false;
    const int chunk = static_cast<int>(std::min<int64_t>(npad, kSortChunk));
    const size_t lds = static_cast<size_t>(chunk) * sizeof(unsigned long long);
    const dim3 grid(static_cast<unsigned>(npad / chunk), Q);
    NVSM_LAUNCH(rank_sort_lds_kernel, grid, dim3(256), lds, s, keys, npad, chunk, static_cast<int64_t>(2), static_cast<int64_t>(chunk));
    for (int64_t k = 2ll * chunk; k <= npad; k <<= 1) {
        for (int64_t j = k >> 1; j >= chunk; j >>= 1)
            NVSM_LAUNCH(rank_sort_global_kernel, dim3(std::min<int64_t>(cdiv(npad / 2, 256), 2048), Q), dim3(256), 0, s, keys, npad, k, j);
        NVSM_LAUNCH(rank_sort_lds_kernel, grid, dim3(256), lds, s, keys, npad, chunk, k, k);
    }
    return npad > chunk;
}

void launch_rank_write(const unsigned long long* keys, int64_t npad, int Q, int k, const int64_t* cand_off, int64_t n_all,
                       int64_t* ids, float* scores, int64_t* counts, hipStream_t s) {
    if (Q <= 0) return;
    NVSM_LAUNCH(rank_write_kernel, dim3(std::min(cdiv(k, 256), 64), Q), dim3(256), 0, s, keys, npad, k, cand_off, n_all, ids, scores, counts);
}

}  // namespace cunvsm
