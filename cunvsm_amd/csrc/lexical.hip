// gfx950 kernels of query-likelihood ranking over the HBM-resident corpus and of run fusion (include/cunvsm_amd.h
// nvsm_lexical_rank / nvsm_rank_ensemble; kernels.h "lexical").
//
//   lex_cf_kernel         cf(t): one histogram pass over the token arena. Integer atomics: their sum does not depend on their order.
//   lex_set_slots_kernel  term -> slot table of num_words ints: set for a round's distinct remaining query terms, cleared behind it
//   lex_score_kernel      scores[q][d - d0] of one slab of documents, the slab layout of launch_rank_scan. One workgroup per
//                         document at a time, grid-strided: the document's tokens are read coalesced, every token's slot is looked
//                         up (the table is L2-resident), hits are counted into an LDS tf[slot] array with LDS integer adds; behind
//                         a barrier a fixed lane visits the terms of one query IN QUERY ORDER, adds their logs in fp64 in that order
//                         and stores the sum narrowed to fp32, -inf when no term of the query occurs in the document. Then the
//                         counters are zeroed. A document longer than the workgroup is looped over.
//                         lex_score_kernel<true> multiplies every term by its weight (nvsm_lexical_rank_weighted); <false> is the
//                         kernel nvsm_lexical_rank always had
//   lex_rm_accumulate_kernel, lex_rm_narrow_kernel   the relevance model of pseudo-relevance feedback
//   lex_df_kernel         df(t): documents in slabs over a bit table [num_words][slab / 32]; a token ORs its document's bit and the lane
//                         that found it clear counts the document; <false> takes the bits away again behind a slab
//   tfidf_score_kernel    lex_score_kernel's frame with the BM25 term idf·tf·(k1 + 1) / (tf + K) (nvsm_tfidf_rank): no log on the device
//   rerank_gather_kernel  a first-stage round's retrieved ids out of its sorted keys, ascending per query, into the candidate arrays
//                         of rank_scan_cand_kernel (nvsm_rerank)
//   lex_write_kernel      launch_rank_write for slabs that hold -inf entries: what is retrieved ends at the first -inf
//   fuse_lists_kernel     one workgroup per query: normalises two ranked lists over their returned entries, matches the documents
//                         both hold by a bitonic sort of (id, list, position) keys, computes the fused fp64 scores and sorts
//                         (fused score, id)
//   fuse_sweep_kernel     fuse_lists_kernel's match once per workgroup, then per alpha of a strip the fused order and the metric row
//                         of its first `depth` entries, all in LDS (nvsm_ensemble_sweep)
// No float atomics anywhere: a repeated call returns the same bits. All arena offsets are 64-bit.
//
// Arithmetic of a term: fp64 throughout (allowed by the contract, and the accurate log the contract asks for). With tf = 0 — nearly
// every (document, term) pair — the term is base[j] − log(den), base[j] = log(c0[j]) evaluated once per term by the host and
// log(den) once per document: no log per pair.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include "../../include/cunvsm_amd.h"
#include "kernels.h"
#include "device_utils.h"
#include "eval_row.h"

namespace cunvsm {

namespace {

__global__ __launch_bounds__(256) void lex_cf_kernel(const int* __restrict__ tokens, int64_t n, unsigned long long* __restrict__ cf) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) atomicAdd(&cf[tokens[i]], 1ull);
}

__global__ __launch_bounds__(256) void lex_fill_int_kernel(int* __restrict__ p, int64_t n, int v) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) p[i] = v;
}

// slot_of[terms[i]] = i (set) or -1 (clear); the terms are distinct
__global__ __launch_bounds__(256) void lex_set_slots_kernel(int* __restrict__ slot_of, const int* __restrict__ terms, int n, int set) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) slot_of[terms[i]] = set ? i : -1;
}

// w·a rounded on its own: the weighted sum is that of plain fp64 operations, whatever the compiler would contract
__device__ __forceinline__ double lex_weighted(double w, double a) {
#pragma clang fp contract(off)
    return w * a;
}

// WEIGHTED false: nvsm_lexical_rank's kernel as it always was; true: every term times its weight (nvsm_lexical_rank_weighted)
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void lex_score_kernel(LexScoreArgs a) {
    __shared__ int tf[kLexSlots];
    for (int i = threadIdx.x; i < kLexSlots; i += 256) tf[i] = 0;
    __syncthreads();
    for (int64_t d = a.d0 + blockIdx.x; d < a.d0 + a.S; d += gridDim.x) {
        const int64_t lo = a.doc_offsets[d], hi = a.doc_offsets[d + 1];
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
            const int slot = a.slot_of[a.tokens[i]];
            if (slot >= 0) atomicAdd(&tf[slot], 1);
        }
        __syncthreads();
        const double len = static_cast<double>(hi - lo);
        // JM: log((1 − λ)·tf/len + λ·p);  Dirichlet: log((tf + μ·p) / (len + μ)).  c0 = λ·p or μ·p, base = log(c0)
        const double log_den = a.method == NVSM_LEX_DIRICHLET ? log(len + a.param) : 0.0;
        const double jm_scale = hi > lo ? (1.0 - a.param) / len : 0.0;
        for (int q = threadIdx.x; q < a.Q; q += 256) {
            double sum = 0.0;
            bool any = false;
            for (int j = a.qoff[q]; j < a.qoff[q + 1]; ++j) {
                const int t = tf[a.tslot[j]];
                double term;
                if (t > 0) {
                    any = true;
                    term = a.method == NVSM_LEX_DIRICHLET ? log((static_cast<double>(t) + a.c0[j]) / (len + a.param))
                                                          : log(jm_scale * static_cast<double>(t) + a.c0[j]);
                } else {
                    term = a.base[j] - log_den;
                }
                sum += WEIGHTED ? lex_weighted(a.weight[j], term) : term;
            }
            a.scores[static_cast<size_t>(q) * a.ld + (d - a.d0)] = any ? static_cast<float>(sum) : -__builtin_inff();
        }
        __syncthreads();
        for (int i = threadIdx.x; i < a.num_slots; i += 256) tf[i] = 0;
        __syncthreads();
    }
}

// ---- document frequencies, TF-IDF and the hand-over to the re-ranking stage ---------------------------------------
// One wave per document of the slab, grid-strided, a document longer than the wave looped over; no barrier anywhere. Document j of
// the slab owns bit j % 32 of word j / 32 in every term's row of `bits` ([V][W] words). MARK: every token ORs its document's bit
// into its term's row, and the one lane that found the bit clear — whichever occurrence of the term in the document that is, across
// the loop's chunks too — adds 1 to df[term]. Clear pass: every token ANDs the bit away again, so the table is zero for the next slab
// without a memset of the whole table per slab. Integer atomics only: df does not depend on their order.
template <bool MARK>
__global__ __launch_bounds__(256) void lex_df_kernel(const int* __restrict__ tokens, const int64_t* __restrict__ doc_offsets, int64_t d0, int S,
                                                     int64_t W, unsigned* __restrict__ bits, unsigned long long* __restrict__ df) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = blockIdx.x * 4ll + (threadIdx.x >> 6); j < S; j += static_cast<int64_t>(gridDim.x) * 4) {
        const int64_t lo = doc_offsets[d0 + j], hi = doc_offsets[d0 + j + 1];
        const unsigned bit = 1u << (j & 31);
        for (int64_t i = lo + lane; i < hi; i += 64) {
            const int t = tokens[i];
            unsigned* word = bits + static_cast<size_t>(t) * W + (j >> 5);
            if (MARK) {
                if (!(atomicOr(word, bit) & bit)) atomicAdd(&df[t], 1ull);
            } else {
                atomicAnd(word, ~bit);
            }
        }
    }
}

// a = (idf·(tf·(k1 + 1))) / (tf + K), K = k1·((1 − b) + b·(len / avgdl)) once per document; every operation rounded on its own
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void tfidf_score_kernel(TfidfScoreArgs a) {
#pragma clang fp contract(off)
    __shared__ int tf[kLexSlots];
    for (int i = threadIdx.x; i < kLexSlots; i += 256) tf[i] = 0;
    __syncthreads();
    const double k1p = a.k1 + 1.0;
    for (int64_t d = a.d0 + blockIdx.x; d < a.d0 + a.S; d += gridDim.x) {
        const int64_t lo = a.doc_offsets[d], hi = a.doc_offsets[d + 1];
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
            const int slot = a.slot_of[a.tokens[i]];
            if (slot >= 0) atomicAdd(&tf[slot], 1);
        }
        __syncthreads();
        const double K = a.k1 * ((1.0 - a.b) + a.b * (static_cast<double>(hi - lo) / a.avgdl));
        for (int q = threadIdx.x; q < a.Q; q += 256) {
            double sum = 0.0;
            bool any = false;
            for (int j = a.qoff[q]; j < a.qoff[q + 1]; ++j) {
                const int t = tf[a.tslot[j]];
                if (t == 0) continue;      // (a term the document does not hold is worth exactly 0)
                any = true;
                const double tfd = static_cast<double>(t);
                const double term = (a.idf[j] * (tfd * k1p)) / (tfd + K);
                sum += WEIGHTED ? a.weight[j] * term : term;
            }
            a.scores[static_cast<size_t>(q) * a.ld + (d - a.d0)] = any ? static_cast<float>(sum) : -__builtin_inff();
        }
        __syncthreads();
        for (int i = threadIdx.x; i < a.num_slots; i += 256) tf[i] = 0;
        __syncthreads();
    }
}

// One workgroup per query of a first-stage round: the ids of the first n = off[q + 1] − off[q] sorted keys (what the round retrieved,
// a prefix: launch_lex_write), ordered ascending by a bitonic sort in LDS (they are distinct), to cand[off[q] ..): the arrays
// rank_scan_cand_kernel reads. nsort: a power of two >= every n, at most kRerankMaxDepth.
__global__ __launch_bounds__(256) void rerank_gather_kernel(const unsigned long long* __restrict__ keys, int64_t npad,
                                                            const int64_t* __restrict__ off, int* __restrict__ cand, int nsort) {
    extern __shared__ unsigned rerank_ids[];
    const int q = blockIdx.x;
    const unsigned long long* g = keys + static_cast<size_t>(q) * npad;
    int64_t n = off[q + 1] - off[q];
    n = n < 0 ? 0 : (n > nsort ? nsort : n);
    n = n > npad ? npad : n;
    for (int i = threadIdx.x; i < nsort; i += 256)
        rerank_ids[i] = i < n ? 0xffffffffu - static_cast<unsigned>(g[i] & 0xffffffffull) : 0xffffffffu;      // (padding sorts last)
    __syncthreads();
    for (int k = 2; k <= nsort; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < nsort / 2; p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int l = i | j;
                const unsigned x = rerank_ids[i], y = rerank_ids[l];
                if ((x <= y) != ((i & k) == 0)) { rerank_ids[i] = y; rerank_ids[l] = x; }
            }
            __syncthreads();
        }
    }
    int* out = cand + off[q];
    for (int i = threadIdx.x; i < n; i += 256) out[i] = static_cast<int>(rerank_ids[i]);
}

// ---- relevance model ---------------------------------------------------------------------------------------------
// One workgroup per query. The feedback documents are walked in rank order, one at a time: every token counts itself into the query's
// cnt[term] (integer atomics), behind a barrier every token takes the count back with an exchange, and the one lane that receives it
// adds ω·c/len to acc[term] with a plain load and store. Whichever lane that is, the adds of a term happen in rank order: a repeated
// call returns the same bits. (The barriers order the workgroup's global accesses: all its waves share one CU's vector cache.)
__global__ __launch_bounds__(256) void lex_rm_accumulate_kernel(LexRmArgs a) {
    __shared__ double omega[kFeedbackMaxDocs];
    const int q = blockIdx.x;
    int n = a.fb_counts[q];
    n = n < 0 ? 0 : (n > a.fb_docs ? a.fb_docs : n);
    const int* ids = a.fb_ids + static_cast<size_t>(q) * a.fb_docs;
    const float* sc = a.fb_scores + static_cast<size_t>(q) * a.fb_docs;
    double* acc = a.acc + static_cast<size_t>(q) * a.V;
    int* cnt = a.cnt + static_cast<size_t>(q) * a.V;
    for (int i = threadIdx.x; i < n; i += 256) omega[i] = i == 0 ? 1.0 : exp(static_cast<double>(sc[i]) - static_cast<double>(sc[0]));
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += omega[i];
        a.sum_w[q] = sum;
    }
    for (int i = 0; i < n; ++i) {
        const int64_t d = ids[i];
        const int64_t lo = a.doc_offsets[d], hi = a.doc_offsets[d + 1];
        const double len = static_cast<double>(hi - lo);
        const double w = omega[i];
        for (int64_t p = lo + threadIdx.x; p < hi; p += 256) atomicAdd(&cnt[a.tokens[p]], 1);
        __syncthreads();
        for (int64_t p = lo + threadIdx.x; p < hi; p += 256) {
            const int t = a.tokens[p];
            const int c = atomicExch(&cnt[t], 0);
            if (c > 0) acc[t] += w * (static_cast<double>(c) / len);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void lex_rm_narrow_kernel(double* __restrict__ acc, const double* __restrict__ sum_w, int64_t V, int64_t t0,
                                                            int S, float* __restrict__ scores, int64_t ld) {
    const int q = blockIdx.y;
    const double total = sum_w[q];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < S; i += gridDim.x * 256) {
        double* cell = acc + static_cast<size_t>(q) * V + t0 + i;
        const double v = *cell;
        float f = -__builtin_inff();
        if (v > 0.0) {
            const float pi = static_cast<float>(v / total);
            if (pi > 0.f) f = pi;
            *cell = 0.0;
        }
        scores[static_cast<size_t>(q) * ld + i] = f;
    }
}

// the sorted keys of a query as (id, score) up to the first -inf score; (-1, -inf) behind it. A key 0 is a padding key.
__global__ __launch_bounds__(256) void lex_write_kernel(const unsigned long long* __restrict__ keys, int64_t npad, int k, int64_t n_all,
                                                        int64_t* __restrict__ ids, float* __restrict__ scores, int64_t* __restrict__ counts) {
    const int q = blockIdx.y;
    const unsigned long long* g = keys + static_cast<size_t>(q) * npad;
    const int most = static_cast<int>(n_all < k ? n_all : k);
    constexpr unsigned kNegInf = 0x007fffffu;      // rank_key(-inf): below the key of every finite score
    if (blockIdx.x == 0 && threadIdx.x == 0 && (most == 0 || static_cast<unsigned>(g[0] >> 32) <= kNegInf)) counts[q] = 0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < k; i += gridDim.x * 256) {
        const size_t o = static_cast<size_t>(q) * k + i;
        const unsigned long long key = i < most ? g[i] : 0ull;
        const unsigned u = static_cast<unsigned>(key >> 32);
        if (u > kNegInf) {
            ids[o] = static_cast<int64_t>(0xffffffffu - static_cast<unsigned>(key & 0xffffffffull));
            scores[o] = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
            // the last retrieved entry names the count (the keys are sorted: what is retrieved is a prefix)
            if (i + 1 == most || static_cast<unsigned>(g[i + 1] >> 32) <= kNegInf) counts[q] = i + 1;
        } else {
            ids[o] = -1;
            scores[o] = -__builtin_inff();
        }
    }
}

// ---- fusion --------------------------------------------------------------------------------------------------------------------
// double -> uint64 whose order is the doubles' order; never 0 for a number
__device__ __forceinline__ unsigned long long fuse_key(double v) {
    v = v + 0.0;      // -0 folded into +0
    const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double fuse_unkey(unsigned long long u) {
    return __longlong_as_double(static_cast<long long>((u >> 63) ? (u & 0x7fffffffffffffffull) : ~u));
}

struct FuseStats { double mean, std, lo, hi; };

// mean, population standard deviation, min and max of x[0 .. n) in index order (one lane)
// (no contraction into fused multiply-adds in the fusion arithmetic: the contract's fixed order is that of plain fp64 operations)
__device__ FuseStats fuse_stats(const float* __restrict__ x, int n) {
#pragma clang fp contract(off)
    FuseStats s{0.0, 0.0, 0.0, 0.0};
    if (n <= 0) return s;
    double sum = 0.0, lo = x[0], hi = x[0];
    for (int i = 0; i < n; ++i) { const double v = x[i]; sum += v; lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    const double mean = sum / n;
    double sq = 0.0;
    for (int i = 0; i < n; ++i) { const double e = static_cast<double>(x[i]) - mean; sq += e * e; }
    s.mean = mean; s.std = sqrt(sq / n); s.lo = lo; s.hi = hi;
    return s;
}
__device__ __forceinline__ double fuse_normalise(double v, const FuseStats& s, int normalizer) {
#pragma clang fp contract(off)
    if (normalizer == NVSM_NORM_STANDARDIZE) return s.std > 0.0 ? (v - s.mean) / s.std : 0.0;
    if (normalizer == NVSM_NORM_MINMAX) return s.hi > s.lo ? (v - s.lo) / (s.hi - s.lo) : 0.0;
    return v;
}

// bitonic sort of n (a power of two) LDS keys, ascending or descending; with `second`, (key, second) pairs compared lexicographically
template <bool DESC, bool PAIRS>
__device__ void fuse_sort(unsigned long long* key, unsigned* second, int n) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < n / 2; p += 256) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int l = i | j;
                const bool fwd = (i & k) == 0;      // this run sorts in the wanted direction
                const unsigned long long x = key[i], y = key[l];
                bool x_first;      // x belongs before y in the wanted direction
                if (PAIRS) {
                    const unsigned sx = second[i], sy = second[l];
                    x_first = DESC ? (x > y || (x == y && sx >= sy)) : (x < y || (x == y && sx <= sy));
                    if (x_first != fwd) { key[i] = y; key[l] = x; second[i] = sy; second[l] = sx; }
                } else {
                    x_first = DESC ? x >= y : x <= y;
                    if (x_first != fwd) { key[i] = y; key[l] = x; }
                }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(256) void fuse_lists_kernel(FuseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ unsigned long long fuse_lds[];
    const int n2 = a.npad;                               // a power of two >= 2 k
    unsigned long long* sk = fuse_lds;                   // [n2] (id, list, position), ascending
    unsigned long long* fk = fuse_lds + n2;              // [n2] fused score keys, descending
    unsigned* fid = reinterpret_cast<unsigned*>(fuse_lds + 2 * n2);      // [n2] ~id next to them
    __shared__ FuseStats stats[2];
    __shared__ int fused_count;
    const int q = blockIdx.x, k = a.k;
    const int64_t* idA = a.ids_a + static_cast<size_t>(q) * k;
    const int64_t* idB = a.ids_b + static_cast<size_t>(q) * k;
    const float* scA = a.scores_a + static_cast<size_t>(q) * k;
    const float* scB = a.scores_b + static_cast<size_t>(q) * k;
    int nA = static_cast<int>(a.counts_a[q]), nB = static_cast<int>(a.counts_b[q]);
    nA = nA < 0 ? 0 : (nA > k ? k : nA);
    nB = nB < 0 ? 0 : (nB > k ? k : nB);
    if (threadIdx.x == 0) { stats[0] = fuse_stats(scA, nA); fused_count = 0; }
    if (threadIdx.x == 64) stats[1] = fuse_stats(scB, nB);
    for (int i = threadIdx.x; i < n2; i += 256) {
        unsigned long long key = ~0ull;
        if (i < nA) key = (static_cast<unsigned long long>(idA[i]) << 32) | static_cast<unsigned long long>(i);
        else if (i >= k && i - k < nB) key = (static_cast<unsigned long long>(idB[i - k]) << 32) | 0x80000000ull | static_cast<unsigned long long>(i - k);
        sk[i] = key;
    }
    __syncthreads();
    fuse_sort<false, false>(sk, nullptr, n2);
    const double wA = static_cast<double>(a.query_alpha ? a.query_alpha[q] : a.alpha), wB = 1.0 - wA;
    for (int i = threadIdx.x; i < n2; i += 256) {
        const unsigned long long key = sk[i];
        unsigned long long out = 0ull;
        unsigned id = 0u;
        if (key != ~0ull) {
            id = static_cast<unsigned>(key >> 32);
            const bool dup = i > 0 && static_cast<unsigned>(sk[i - 1] >> 32) == id && sk[i - 1] != ~0ull;      // list B's entry of a document list A holds
            if (!dup) {
                const bool in_b = (key & 0x80000000ull) != 0;
                const int pos = static_cast<int>(key & 0x7fffffffull);
                double f;
                if (in_b) {
                    f = wB * fuse_normalise(scB[pos], stats[1], a.normalizer);
                } else {
                    f = wA * fuse_normalise(scA[pos], stats[0], a.normalizer);
                    if (i + 1 < n2 && sk[i + 1] != ~0ull && static_cast<unsigned>(sk[i + 1] >> 32) == id) {
                        const int pb = static_cast<int>(sk[i + 1] & 0x7fffffffull);
                        f = (f + wB * fuse_normalise(scB[pb], stats[1], a.normalizer)) / 2.0;
                    }
                }
                out = fuse_key(f);
            }
        }
        fk[i] = out;
        fid[i] = 0xffffffffu - id;
    }
    __syncthreads();
    fuse_sort<true, true>(fk, fid, n2);
    int64_t* oid = a.out_ids + static_cast<size_t>(q) * 2 * k;
    float* osc = a.out_scores + static_cast<size_t>(q) * 2 * k;
    for (int i = threadIdx.x; i < 2 * k; i += 256) {
        const unsigned long long key = fk[i];
        if (key != 0ull) {
            oid[i] = static_cast<int64_t>(0xffffffffu - fid[i]);
            osc[i] = static_cast<float>(fuse_unkey(key));
            if (i + 1 == 2 * k || fk[i + 1] == 0ull) fused_count = i + 1;
        } else {
            oid[i] = -1;
            osc[i] = -__builtin_inff();
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) a.out_counts[q] = fused_count;
}

// ---- the alpha sweep ----------------------------------------------------------------------------------------------
// fuse_lists_kernel's match and normalisation once, then per alpha of the workgroup's strip its fused keys, its pair sort, and
// eval_metrics_kernel's row of the sorted ids where they lie in LDS. What depends on alpha is the key, one sort and the row.
//   LDS per entry slot: 8 B  the (id, list, position) key, overwritten by the entry's normalised score once its neighbours are read
//                       8 B  fused key        4 B  ~id next to it        4 B  id        1 B  kind
//   kind: 0 padding, or list B's entry of a document list A holds; 1 in list A only; 2 in list B only; 3 list A's entry of a document
//   whose list B entry is the next slot. One double per ENTRY is enough: both lists together hold at most npad entries.
__global__ __launch_bounds__(256) void fuse_sweep_kernel(FuseSweepArgs s) {
#pragma clang fp contract(off)
    extern __shared__ unsigned long long fuse_lds[];
    const FuseArgs& a = s.f;
    const int n2 = a.npad;                               // a power of two >= 2 k
    unsigned long long* sk = fuse_lds;                   // [n2] (id, list, position) ascending; then the bits of the normalised scores
    unsigned long long* fk = fuse_lds + n2;              // [n2] fused score keys, descending
    unsigned* fid = reinterpret_cast<unsigned*>(fuse_lds + 2 * n2);      // [n2] ~id next to them
    unsigned* did = fid + n2;                            // [n2] id of the slot's document
    unsigned char* kind = reinterpret_cast<unsigned char*>(did + n2);    // [n2]
    __shared__ FuseStats stats[2];
    __shared__ int num_docs;
    const int q = blockIdx.x, k = a.k;
    const int64_t* idA = a.ids_a + static_cast<size_t>(q) * k;
    const int64_t* idB = a.ids_b + static_cast<size_t>(q) * k;
    const float* scA = a.scores_a + static_cast<size_t>(q) * k;
    const float* scB = a.scores_b + static_cast<size_t>(q) * k;
    int nA = static_cast<int>(a.counts_a[q]), nB = static_cast<int>(a.counts_b[q]);
    nA = nA < 0 ? 0 : (nA > k ? k : nA);
    nB = nB < 0 ? 0 : (nB > k ? k : nB);
    if (threadIdx.x == 0) { stats[0] = fuse_stats(scA, nA); num_docs = 0; }
    if (threadIdx.x == 64) stats[1] = fuse_stats(scB, nB);
    for (int i = threadIdx.x; i < n2; i += 256) {
        unsigned long long key = ~0ull;
        if (i < nA) key = (static_cast<unsigned long long>(idA[i]) << 32) | static_cast<unsigned long long>(i);
        else if (i >= k && i - k < nB) key = (static_cast<unsigned long long>(idB[i - k]) << 32) | 0x80000000ull | static_cast<unsigned long long>(i - k);
        sk[i] = key;
    }
    __syncthreads();
    fuse_sort<false, false>(sk, nullptr, n2);
    for (int i = threadIdx.x; i < n2; i += 256) {
        const unsigned long long key = sk[i];
        unsigned id = 0u;
        unsigned char kd = 0;
        if (key != ~0ull) {
            id = static_cast<unsigned>(key >> 32);
            const bool dup = i > 0 && static_cast<unsigned>(sk[i - 1] >> 32) == id && sk[i - 1] != ~0ull;
            if (!dup) {
                if ((key & 0x80000000ull) != 0) kd = 2;
                else kd = (i + 1 < n2 && sk[i + 1] != ~0ull && static_cast<unsigned>(sk[i + 1] >> 32) == id) ? 3 : 1;
                atomicAdd(&num_docs, 1);      // (an integer count: its order does not matter)
            }
        }
        did[i] = id;
        kind[i] = kd;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n2; i += 256) {      // every entry's normalised score in place of its key
        const unsigned long long key = sk[i];
        double v = 0.0;
        if (key != ~0ull) {
            const int pos = static_cast<int>(key & 0x7fffffffull);
            v = (key & 0x80000000ull) != 0 ? fuse_normalise(scB[pos], stats[1], a.normalizer) : fuse_normalise(scA[pos], stats[0], a.normalizer);
        }
        sk[i] = static_cast<unsigned long long>(__double_as_longlong(v));
    }
    __syncthreads();
    const int64_t gq = s.e.q0 + q;
    const int width = NVSM_EVAL_FIXED + 3 * s.e.num_cutoffs;
    const int n = s.depth > 0 && s.depth < num_docs ? s.depth : num_docs;
    const int a_end = (blockIdx.y + 1) * kFuseSweepStrip < s.num_alphas ? (blockIdx.y + 1) * kFuseSweepStrip : s.num_alphas;
    for (int ai = blockIdx.y * kFuseSweepStrip; ai < a_end; ++ai) {
        const double wA = static_cast<double>(s.alphas[ai]), wB = 1.0 - wA;
        for (int i = threadIdx.x; i < n2; i += 256) {
            const int kd = kind[i];
            unsigned long long out = 0ull;
            if (kd != 0) {
                const double v = __longlong_as_double(static_cast<long long>(sk[i]));
                double f;
                if (kd == 2) {
                    f = wB * v;
                } else {
                    f = wA * v;
                    if (kd == 3) f = (f + wB * __longlong_as_double(static_cast<long long>(sk[i + 1]))) / 2.0;
                }
                out = fuse_key(f);
            }
            fk[i] = out;
            fid[i] = 0xffffffffu - did[i];
        }
        __syncthreads();
        fuse_sort<true, true>(fk, fid, n2);
        if (threadIdx.x < 64)      // one wave, as eval_metrics_kernel: the row of the first n sorted ids
            eval_row(s.e, gq, n, static_cast<int>(threadIdx.x), [fid](int r) { return static_cast<int>(0xffffffffu - fid[r]); },
                     s.table + (static_cast<int64_t>(ai) * s.total_queries + gq) * width);
        __syncthreads();      // (the next alpha overwrites the keys the wave reads)
    }
}

int grid_for(int64_t n) { return stream_grid(n, 256); }

}  // namespace

void launch_lex_cf(const int* tokens, int64_t n, unsigned long long* cf, hipStream_t s) {
    if (n > 0) NVSM_LAUNCH(lex_cf_kernel, dim3(grid_for(n)), dim3(256), 0, s, tokens, n, cf);
}

void launch_lex_fill_int(int* p, int64_t n, int v, hipStream_t s) {
    if (n > 0) NVSM_LAUNCH(lex_fill_int_kernel, dim3(grid_for(n)), dim3(256), 0, s, p, n, v);
}

void launch_lex_set_slots(int* slot_of, const int* terms, int n, bool set, hipStream_t s) {
    if (n > 0) NVSM_LAUNCH(lex_set_slots_kernel, dim3((n + 255) / 256), dim3(256), 0, s, slot_of, terms, n, set ? 1 : 0);
}

void launch_lex_score(const LexScoreArgs& a, hipStream_t s) {
    if (a.S <= 0 || a.Q <= 0) return;
    // (grid-strided: enough workgroups to fill the device several times over, not one per document of a large slab)
    const int grid = static_cast<int>(a.S < 8192 ? a.S : 8192);
    if (a.weight) NVSM_LAUNCH(lex_score_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else NVSM_LAUNCH(lex_score_kernel<false>, dim3(grid), dim3(256), 0, s, a);
}

int64_t lex_df_row_words(int64_t slab) { return (slab + 31) / 32; }

void launch_lex_df(const int* tokens, const int64_t* doc_offsets, int64_t num_documents, int64_t slab, unsigned* bits,
                   unsigned long long* df, hipStream_t s) {
    if (slab < 1 || slab >= (int64_t(1) << 31)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "lex_df: the slab must hold 1 .. 2^31 - 1 documents");
    const int64_t W = lex_df_row_words(slab);
    for (int64_t d0 = 0; d0 < num_documents; d0 += slab) {
        const int S = static_cast<int>(std::min(slab, num_documents - d0));
        const int grid = static_cast<int>(std::min<int64_t>((S + 3) / 4, 8192));
        NVSM_LAUNCH(lex_df_kernel<true>, dim3(grid), dim3(256), 0, s, tokens, doc_offsets, d0, S, W, bits, df);
        if (d0 + slab < num_documents)      // (behind the last slab the table is left as it is: its owner frees it)
            NVSM_LAUNCH(lex_df_kernel<false>, dim3(grid), dim3(256), 0, s, tokens, doc_offsets, d0, S, W, bits, df);
    }
}

void launch_tfidf_score(const TfidfScoreArgs& a, hipStream_t s) {
    if (a.S <= 0 || a.Q <= 0) return;
    const int grid = static_cast<int>(a.S < 8192 ? a.S : 8192);      // (grid-strided, as launch_lex_score)
    if (a.weight) NVSM_LAUNCH(tfidf_score_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else NVSM_LAUNCH(tfidf_score_kernel<false>, dim3(grid), dim3(256), 0, s, a);
}

void launch_rerank_gather(const unsigned long long* keys, int64_t npad, const int64_t* off, int* cand, int Q, int nsort, hipStream_t s) {
    if (Q <= 0) return;
    if (nsort < 1 || nsort > kRerankMaxDepth || (nsort & (nsort - 1)) != 0)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "rerank_gather: nsort must be a power of two of at most NVSM_RERANK_MAX_DEPTH");
    NVSM_LAUNCH(rerank_gather_kernel, dim3(Q), dim3(256), static_cast<size_t>(nsort) * sizeof(unsigned), s, keys, npad, off, cand, nsort);
}

void launch_lex_rm_accumulate(const LexRmArgs& a, int Q, hipStream_t s) {
    if (Q > 0) NVSM_LAUNCH(lex_rm_accumulate_kernel, dim3(Q), dim3(256), 0, s, a);
}

void launch_lex_rm_narrow(double* acc, const double* sum_w, int64_t V, int64_t t0, int S, int Q, float* scores, int64_t ld, hipStream_t s) {
    if (Q <= 0 || S <= 0) return;
    const int gx = (S + 255) / 256 < 256 ? (S + 255) / 256 : 256;
    NVSM_LAUNCH(lex_rm_narrow_kernel, dim3(gx, Q), dim3(256), 0, s, acc, sum_w, V, t0, S, scores, ld);
}

void launch_lex_write(const unsigned long long* keys, int64_t npad, int Q, int k, int64_t n_all, int64_t* ids, float* scores,
                      int64_t* counts, hipStream_t s) {
    if (Q <= 0) return;
    const int gx = (k + 255) / 256 < 64 ? (k + 255) / 256 : 64;
    NVSM_LAUNCH(lex_write_kernel, dim3(gx, Q), dim3(256), 0, s, keys, npad, k, n_all, ids, scores, counts);
}

void launch_fuse_lists(const FuseArgs& a, int Q, hipStream_t s) {
    if (Q <= 0) return;
    const size_t lds = static_cast<size_t>(a.npad) * (2 * sizeof(unsigned long long) + sizeof(unsigned));
    NVSM_LAUNCH(fuse_lists_kernel, dim3(Q), dim3(256), lds, s, a);
}

static size_t fuse_sweep_lds_bytes(int npad) { return (static_cast<size_t>(npad) * (2 * sizeof(unsigned long long) + 2 * sizeof(unsigned) + 1) + 7) / 8 * 8; }

void launch_fuse_sweep(const FuseSweepArgs& a, int Q, hipStream_t s) {
    if (Q <= 0 || a.num_alphas <= 0) return;
    const int strips = (a.num_alphas + kFuseSweepStrip - 1) / kFuseSweepStrip;
    NVSM_LAUNCH(fuse_sweep_kernel, dim3(Q, strips), dim3(256), fuse_sweep_lds_bytes(a.f.npad), s, a);
}

}  // namespace cunvsm
