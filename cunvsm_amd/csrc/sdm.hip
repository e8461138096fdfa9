// gfx950 kernels of sequential-dependence ranking over the HBM-resident corpus (include/cunvsm_amd.h nvsm_sdm_rank /
// nvsm_sdm_pair_counts; kernels.h "sequential dependence").
//
//   sdm_count_document    lex_score_kernel's frame — one workgroup walks one document — with the order of the tokens read: the
//                         document goes through LDS in tiles of kSdmTile positions, every tile with a halo of window − 1 positions
//                         behind it, clipped at the document's end (the halo never holds a token of the next document). What is
//                         staged is slot_of[token], so a look-ahead compares small integers in LDS and never touches the arena
//                         again. A position whose slot is >= 0 counts itself into tf[slot] and walks that slot's pair entries (a CSR
//                         of the round: other slot, pair id, role): role "first" tests the next position for the ordered count,
//                         every role scans the look-ahead for the other term and counts the POSITION once on the first hit (an
//                         existence test). LDS integer adds only.
//   sdm_collect_kernel    the counting over ALL documents, grid-strided; a workgroup's od / uw totals go into the round's global
//                         64-bit counters at its end (and before its 32-bit LDS counters could wrap). Integer atomics: their order
//                         cannot change a sum.
//   sdm_score_kernel      the counting per document of a slab, then behind a barrier a fixed lane evaluates one query: its three
//                         groups in the order T, O, U, every group's members in query order in fp64, every product and quotient
//                         rounded on its own (contraction off), the sum narrowed to fp32 once; -inf when no remaining term of the
//                         query occurs in the document. The scores go into the slab layout of launch_rank_scan.
//   sdm_postings_collect_kernel / sdm_postings_score_kernel   the same two phases from the positional postings of the round's terms
//                         (DESIGN.md §26): a pair's counts in a document come from merging the two ascending runs of in-document
//                         offsets, the slab is filled in index.hip's ownership scheme, the score is sdm_score_kernel's expression
//                         through the same sdm_feature. The same bits as the scan.
// No float atomics, no inline assembly. All arena offsets are 64-bit.
#include <algorithm>
#include <cstdint>
#include "../../include/cunvsm_amd.h"
#include "kernels.h"
#include "device_utils.h"
#include "index_search.h"

namespace cunvsm {

namespace {

struct SdmCounters {
    int tf[kSdmSlots];
    int od[kSdmPairs];
    int uw[kSdmPairs];
    int stage[kSdmTile + kSdmMaxWindow - 1];
};

__device__ __forceinline__ void sdm_zero(SdmCounters& c, int num_slots, int num_pairs) {
    for (int i = threadIdx.x; i < num_slots; i += kSdmTile) c.tf[i] = 0;
    for (int i = threadIdx.x; i < num_pairs; i += kSdmTile) { c.od[i] = 0; c.uw[i] = 0; }
}

// the counts of document [lo, hi) added into c; the workgroup's barriers are inside. window in [2, kSdmMaxWindow].
__device__ __forceinline__ void sdm_count_document(const SdmCountArgs& a, SdmCounters& c, int64_t lo, int64_t hi) {
    for (int64_t tile = lo; tile < hi; tile += kSdmTile) {
        const int64_t left = hi - tile;
        // the tile and its halo, clipped at the document's end: n <= kSdmTile + window − 1 <= the staged array
        const int n = static_cast<int>(left < kSdmTile + a.window - 1 ? left : kSdmTile + a.window - 1);
        for (int i = threadIdx.x; i < n; i += kSdmTile) c.stage[i] = a.slot_of[a.tokens[tile + i]];
        __syncthreads();
        const int i = threadIdx.x;
        if (i < n) {      // (i < kSdmTile: a position of the tile itself, inside the document)
            const int slot = c.stage[i];
            if (slot >= 0) {
                atomicAdd(&c.tf[slot], 1);
                const int end = i + a.window < n ? i + a.window : n;      // the look-ahead is i + 1 .. end − 1
                for (int e = a.ent_off[slot]; e < a.ent_off[slot + 1]; ++e) {
                    const int other = a.ent_other[e], pr = a.ent_pair[e];
                    const int pair = pr >> 1;
                    if ((pr & 1) && i + 1 < n && c.stage[i + 1] == other) atomicAdd(&c.od[pair], 1);
                    for (int j = i + 1; j < end; ++j)
                        if (c.stage[j] == other) { atomicAdd(&c.uw[pair], 1); break; }
                }
            }
        }
        __syncthreads();      // (the next tile overwrites what the look-aheads read)
    }
}

__global__ __launch_bounds__(kSdmTile) void sdm_collect_kernel(SdmCountArgs a, int64_t num_documents, unsigned long long* __restrict__ cf_o,
                                                               unsigned long long* __restrict__ cf_u) {
    __shared__ SdmCounters c;
    sdm_zero(c, a.num_slots, a.num_pairs);
    __syncthreads();
    int64_t walked = 0;      // tokens counted into the LDS totals since they were last emptied: what bounds every 32-bit counter
    for (int64_t d = blockIdx.x;; d += gridDim.x) {      // (d is the same in every lane: the barriers inside are reached by all)
        const bool done = d >= num_documents;
        const int64_t lo = done ? 0 : a.doc_offsets[d], hi = done ? 0 : a.doc_offsets[d + 1];
        if (done || walked + (hi - lo) > (int64_t(1) << 30)) {
            for (int p = threadIdx.x; p < a.num_pairs; p += kSdmTile) {
                const int o = c.od[p], u = c.uw[p];
                if (o) atomicAdd(&cf_o[p], static_cast<unsigned long long>(o));
                if (u) atomicAdd(&cf_u[p], static_cast<unsigned long long>(u));
                c.od[p] = 0; c.uw[p] = 0;
            }
            walked = 0;
            __syncthreads();
            if (done) break;
        }
        sdm_count_document(a, c, lo, hi);
        walked += hi - lo;
    }
}

// one member of a group: a·b and a/b rounded on their own
__device__ __forceinline__ double sdm_feature(const SdmScoreArgs& a, int count, double c0, double base, double len, double log_den, double jm_scale) {
    if (count > 0)
        return a.method == NVSM_LEX_DIRICHLET ? log((static_cast<double>(count) + c0) / (len + a.param)) : log(jm_scale * static_cast<double>(count) + c0);
    return base - log_den;
}

__global__ __launch_bounds__(kSdmTile) void sdm_score_kernel(SdmScoreArgs a) {
#pragma clang fp contract(off)
    __shared__ SdmCounters c;
    const SdmCountArgs& k = a.count;
    sdm_zero(c, k.num_slots, k.num_pairs);
    __syncthreads();
    for (int64_t d = a.d0 + blockIdx.x; d < a.d0 + a.S; d += gridDim.x) {
        const int64_t lo = k.doc_offsets[d], hi = k.doc_offsets[d + 1];
        sdm_count_document(k, c, lo, hi);      // (ends with a barrier; an empty document leaves the zeros the loop's end wrote)
        __syncthreads();
        const double len = static_cast<double>(hi - lo);
        const double log_den = a.method == NVSM_LEX_DIRICHLET ? log(len + a.param) : 0.0;
        const double jm_scale = hi > lo ? (1.0 - a.param) / len : 0.0;
        for (int q = threadIdx.x; q < a.Q; q += kSdmTile) {
            bool any = false;
            double score = 0.0;
            for (int g = 0; g < 3; ++g) {      // T, O, U
                const int* off = a.goff + static_cast<size_t>(g) * (a.Q + 1);
                const int j0 = off[q], j1 = off[q + 1];
                double sum = 0.0;
                for (int j = j0; j < j1; ++j) {
                    const int idx = a.index[j];
                    const int count = g == 0 ? c.tf[idx] : (g == 1 ? c.od[idx] : c.uw[idx]);
                    if (g == 0 && count > 0) any = true;
                    sum += sdm_feature(a, count, a.c0[j], a.base[j], len, log_den, jm_scale);
                }
                const double coef = a.coef[static_cast<size_t>(q) * 3 + g];      // w_G / Σ w of the present groups, 0 for an absent one
                if (j1 > j0 && coef > 0.0) score += coef * (sum / static_cast<double>(j1 - j0));
            }
            a.scores[static_cast<size_t>(q) * a.ld + (d - a.d0)] = any ? static_cast<float>(score) : -__builtin_inff();
        }
        __syncthreads();
        sdm_zero(c, k.num_slots, k.num_pairs);
        __syncthreads();
    }
}

// ---- the same two phases from positional postings -----------------------------------------------------------------
// A [nA], B [nB]: two ascending runs of in-document offsets of ONE document, so no boundary needs a test. For every i of A the first j
// of B behind it is its only candidate partner: *next counts j == i + 1, *follow counts j < i + window — a position once, as the
// scan's existence test. A run against itself (the pair (a, a)): the partner of A[x] is A[x + 1].
__device__ __forceinline__ void sdm_run_counts(const int* __restrict__ A, int nA, const int* __restrict__ B, int nB, int window, int* next,
                                               int* follow) {
    int jb = 0, o = 0, u = 0;
    for (int x = 0; x < nA; ++x) {
        const int i = A[x];
        while (jb < nB && B[jb] <= i) ++jb;
        if (jb == nB) break;
        const int j = B[jb];
        o += j == i + 1 ? 1 : 0;
        u += j < i + window ? 1 : 0;
    }
    *next += o; *follow += u;
}

// od and, where wanted, uw of the pair (a, b) in one document, from the posting pa of a and pb of b there (pa == pb for a == b):
// sdm_count_document's counts — the first term's positions count both forms, the second term's the unordered one alone
__device__ __forceinline__ void sdm_pair_in_document(const SdmPostingsArgs& k, int64_t pa, int64_t pb, bool want_uw, int* od, int* uw) {
    const int* A = k.pos + k.post_first[pa];
    const int* B = k.pos + k.post_first[pb];
    const int nA = k.post_tf[pa], nB = k.post_tf[pb];
    sdm_run_counts(A, nA, B, nB, k.window, od, uw);
    if (want_uw && pa != pb) {
        int unused = 0;
        sdm_run_counts(B, nB, A, nA, k.window, &unused, uw);
    }
}

// blockIdx.y: a pair of the round; the lanes walk the shorter of its two lists and search the document in the other one
__global__ __launch_bounds__(256) void sdm_postings_collect_kernel(SdmPostingsArgs k, unsigned long long* __restrict__ cf_o,
                                                                   unsigned long long* __restrict__ cf_u) {
    for (int p = blockIdx.y; p < k.num_pairs; p += gridDim.y) {
        const int ta = k.terms[k.pair_a[p]], tb = k.terms[k.pair_b[p]];
        const int64_t a0 = k.post_off[ta], a1 = k.post_off[ta + 1], b0 = k.post_off[tb], b1 = k.post_off[tb + 1];
        const bool walk_a = a1 - a0 <= b1 - b0;
        const int64_t w1 = walk_a ? a1 : b1, s0 = walk_a ? b0 : a0, s1 = walk_a ? b1 : a1;
        unsigned long long o = 0, u = 0;
        for (int64_t x = (walk_a ? a0 : b0) + blockIdx.x * 256ll + threadIdx.x; x < w1; x += static_cast<int64_t>(gridDim.x) * 256) {
            int64_t y = x;
            if (ta != tb) {
                const int d = k.post_doc[x];
                y = index_lower_bound(k.post_doc, s0, s1, d);
                if (y >= s1 || k.post_doc[y] != d) continue;
            }
            int od = 0, uw = 0;
            sdm_pair_in_document(k, walk_a ? x : y, walk_a ? y : x, true, &od, &uw);
            o += static_cast<unsigned long long>(od);
            u += static_cast<unsigned long long>(uw);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { o += __shfl_down(o, off, 64); u += __shfl_down(u, off, 64); }
        if ((threadIdx.x & 63) == 0) {      // integer atomics: their order cannot change a sum
            if (o) atomicAdd(&cf_o[p], o);
            if (u) atomicAdd(&cf_u[p], u);
        }
    }
}

// the posting of slot s that holds document d, inside the slab's bounds; -1: the term does not hold it
__device__ __forceinline__ int64_t sdm_posting_of(const SdmPostingsScoreArgs& a, int s, int d) {
    const int64_t hi = a.hi[s];
    const int64_t p = index_lower_bound(a.post.post_doc, a.lo[s], hi, d);
    return (p < hi && a.post.post_doc[p] == d) ? p : -1;
}

// index.hip's ownership scheme: blockIdx.y takes a member of group 0 — the first of its slot in its query — and a lane one posting of
// its term inside the slab. The posting owns (q, d) if no earlier member's term holds d; the owner gathers every member's count from
// the postings and evaluates sdm_score_kernel's expression, operation for operation, and stores the score once.
__global__ __launch_bounds__(256) void sdm_postings_score_kernel(SdmPostingsScoreArgs a) {
#pragma clang fp contract(off)
    const SdmScoreArgs& sc = a.score;
    const SdmPostingsArgs& k = a.post;
    for (int j = blockIdx.y; j < a.num_entries; j += gridDim.y) {
        if (!a.first[j]) continue;
        const int slot = sc.index[j], q = a.entry_query[j];
        const int j0 = sc.goff[q];
        const int64_t end = a.hi[slot];
        for (int64_t p = a.lo[slot] + blockIdx.x * 256ll + threadIdx.x; p < end; p += static_cast<int64_t>(gridDim.x) * 256) {
            const int d = k.post_doc[p];
            bool earlier = false;
            for (int jj = j0; jj < j && !earlier; ++jj) earlier = sdm_posting_of(a, sc.index[jj], d) >= 0;
            if (earlier) continue;
            const int64_t lo = sc.count.doc_offsets[d], hi = sc.count.doc_offsets[d + 1];
            const double len = static_cast<double>(hi - lo);
            const double log_den = sc.method == NVSM_LEX_DIRICHLET ? log(len + sc.param) : 0.0;
            const double jm_scale = hi > lo ? (1.0 - sc.param) / len : 0.0;
            double score = 0.0;
            for (int g = 0; g < 3; ++g) {      // T, O, U
                const int* off = sc.goff + static_cast<size_t>(g) * (sc.Q + 1);
                const int m0 = off[q], m1 = off[q + 1];
                double sum = 0.0;
                for (int m = m0; m < m1; ++m) {
                    const int idx = sc.index[m];
                    int count = 0;
                    if (g == 0) {
                        const int64_t pm = idx == slot ? p : (m < j ? -1 : sdm_posting_of(a, idx, d));      // (before j: held by no one)
                        count = pm >= 0 ? k.post_tf[pm] : 0;
                    } else {
                        const int sa = k.pair_a[idx], sb = k.pair_b[idx];
                        const int64_t pa = sdm_posting_of(a, sa, d);
                        const int64_t pb = pa < 0 ? -1 : (sb == sa ? pa : sdm_posting_of(a, sb, d));
                        if (pb >= 0) {
                            int od = 0, uw = 0;
                            sdm_pair_in_document(k, pa, pb, g == 2, &od, &uw);
                            count = g == 1 ? od : uw;
                        }
                    }
                    sum += sdm_feature(sc, count, sc.c0[m], sc.base[m], len, log_den, jm_scale);
                }
                const double coef = sc.coef[static_cast<size_t>(q) * 3 + g];
                if (m1 > m0 && coef > 0.0) score += coef * (sum / static_cast<double>(m1 - m0));
            }
            sc.scores[static_cast<size_t>(q) * sc.ld + (d - sc.d0)] = static_cast<float>(score);
        }
    }
}

void sdm_check(const SdmCountArgs& a) {
    if (a.window < 2 || a.window > kSdmMaxWindow) throw Error(NVSM_ERR_INVALID_ARGUMENT, "sdm: the window must be in [2, NVSM_SDM_MAX_WINDOW]");
    if (a.num_slots < 0 || a.num_slots > kSdmSlots || a.num_pairs < 0 || a.num_pairs > kSdmPairs)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "sdm: more slots or pairs than the LDS counters hold");
}

}  // namespace

void launch_sdm_collect(const SdmCountArgs& a, int64_t num_documents, unsigned long long* cf_o, unsigned long long* cf_u, hipStream_t s) {
    sdm_check(a);
    if (num_documents <= 0 || a.num_pairs <= 0) return;
    const int grid = static_cast<int>(num_documents < 4096 ? num_documents : 4096);
    NVSM_LAUNCH(sdm_collect_kernel, dim3(grid), dim3(kSdmTile), 0, s, a, num_documents, cf_o, cf_u);
}

void launch_sdm_score(const SdmScoreArgs& a, hipStream_t s) {
    sdm_check(a.count);
    if (a.S <= 0 || a.Q <= 0) return;
    const int grid = static_cast<int>(a.S < 8192 ? a.S : 8192);      // (grid-strided, as launch_lex_score)
    NVSM_LAUNCH(sdm_score_kernel, dim3(grid), dim3(kSdmTile), 0, s, a);
}

// x: the workgroups one list is spread over, sized by the longest list the round can meet (launch_postings_fill's rule)
static unsigned sdm_postings_grid_x(int64_t longest) {
    return static_cast<unsigned>(std::min<int64_t>((std::max<int64_t>(longest, 1) + 255) / 256, 256));
}

void launch_sdm_postings_collect(const SdmPostingsArgs& a, int64_t max_df, unsigned long long* cf_o, unsigned long long* cf_u, hipStream_t s) {
    if (a.window < 2 || a.window > kSdmMaxWindow) throw Error(NVSM_ERR_INVALID_ARGUMENT, "sdm: the window must be in [2, NVSM_SDM_MAX_WINDOW]");
    if (a.num_pairs <= 0) return;
    NVSM_LAUNCH(sdm_postings_collect_kernel, dim3(sdm_postings_grid_x(max_df), static_cast<unsigned>(std::min(a.num_pairs, 65535))), dim3(256), 0, s,
                a, cf_o, cf_u);
}

void launch_sdm_postings_score(const SdmPostingsScoreArgs& a, int64_t max_df, hipStream_t s) {
    const SdmScoreArgs& sc = a.score;
    if (a.post.window < 2 || a.post.window > kSdmMaxWindow) throw Error(NVSM_ERR_INVALID_ARGUMENT, "sdm: the window must be in [2, NVSM_SDM_MAX_WINDOW]");
    if (sc.S <= 0 || sc.Q <= 0) return;
    launch_index_fill(sc.scores, static_cast<int64_t>(sc.Q) * sc.ld, s);
    if (a.post.num_slots <= 0 || a.num_entries <= 0) return;
    launch_index_bounds(a.post.post_off, a.post.post_doc, a.post.terms, a.post.num_slots, sc.d0, sc.S, a.lo, a.hi, s);
    NVSM_LAUNCH(sdm_postings_score_kernel, dim3(sdm_postings_grid_x(std::min<int64_t>(max_df, sc.S)), static_cast<unsigned>(std::min(a.num_entries, 65535))),
                dim3(256), 0, s, a);
}

}  // namespace cunvsm
