// gfx950 kernels of the device-resident inverted index of the uploaded corpus (include/cunvsm_amd.h nvsm_corpus_index; kernels.h
// "inverted index"): its build, and the postings form of a lexical round's slab fill.
//
// The index is a CSR of postings: post_off [V + 1] int64, post_doc [P] / post_tf [P] int32, P = Σ_t df(t); within a term the
// documents ascend and each appears once. Build, behind sort_pairs(keys = tokens, values = positions), which is stable — every
// term's positions ascend, hence its documents:
//   index_docs_kernel       position -> document, by binary search in doc_offsets, in place
//   index_tile_sums_kernel  heads — entries whose (term, document) differs from their predecessor's — counted per tile of 2048
//   index_scan_sums_kernel  one workgroup: the tile counts' exclusive prefixes, the total behind them
//   index_write_kernel      every head's posting number = its tile's prefix + the heads before it in the tile (recounted): post_doc,
//                           the head's position, and at a term's first head post_off / tok_off of every term up to it from the term
//                           before (the terms in between hold nothing); the last entry closes both arrays and the head positions
//   index_tf_kernel         post_tf = the distance to the next head: the run length
// Three launches make the scan; no workgroup waits on another one, no atomics at all. Every posting and every bound has one writer:
// a second build gives the same bytes.
//
// The postings fill of a slab [d0, d0 + S): index_bounds_kernel finds, per distinct term of the round, its postings inside the slab
// (the lists ascend: two binary searches); lex_postings_kernel / tfidf_postings_kernel take one query entry per blockIdx.y — the
// first entry of each of the query's distinct terms, in query order — and one posting of its term per lane. The posting (t_i, d)
// OWNS (q, d) if none of the query's earlier entries' terms holds d (binary search in their lists); the owner fetches the tf of
// the later entries the same way, adds the terms in query order and stores scores[q][d − d0] once. No two lanes write one address
// and nothing is accumulated in memory. A wave's lanes hold consecutive postings of one list, so their searches in another list
// walk the same upper levels and part only near the leaves.
// The positional layer (nvsm_corpus_index_positions) is the same build with the sorted positions kept:
// index_positions_kernel writes every entry's document and its offset inside it, and the heads index_write_kernel finds are post_first.
// The term expressions are lex_score_kernel's and tfidf_score_kernel's (lexical.hip), operation for operation: the same bits.
#include <algorithm>
#include <cstdint>
#include "../../include/cunvsm_amd.h"
#include "kernels.h"
#include "device_utils.h"
#include "index_search.h"

namespace cunvsm {

namespace {

constexpr int kIndexItems = 8;                                // consecutive entries per lane
constexpr int kIndexTile = 256 * kIndexItems;                 // entries per workgroup

// pos[i]: arena position -> its document: the last d with doc_offsets[d] <= position (empty documents hold nothing)
__global__ __launch_bounds__(256) void index_docs_kernel(int* __restrict__ pos, int64_t n, const int64_t* __restrict__ doc_offsets, int64_t num_documents) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
        const int64_t p = pos[i];
        // first offset > p, among doc_offsets[1 .. num_documents]: the document's end
        int64_t lo = 1, hi = num_documents;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (doc_offsets[mid] <= p) lo = mid + 1; else hi = mid;
        }
        pos[i] = static_cast<int>(lo - 1);
    }
}

// the positional layer: pos[i] an arena position -> doc[i] its document (index_docs_kernel's search), pos[i] the offset inside it
__global__ __launch_bounds__(256) void index_positions_kernel(int* __restrict__ pos, int* __restrict__ doc, int64_t n,
                                                              const int64_t* __restrict__ doc_offsets, int64_t num_documents) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
        const int64_t p = pos[i];
        int64_t lo = 1, hi = num_documents;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (doc_offsets[mid] <= p) lo = mid + 1; else hi = mid;
        }
        doc[i] = static_cast<int>(lo - 1);
        pos[i] = static_cast<int>(p - doc_offsets[lo - 1]);
    }
}

__device__ __forceinline__ bool index_head(const int* __restrict__ term, const int* __restrict__ doc, int64_t i) {
    return i == 0 || term[i] != term[i - 1] || doc[i] != doc[i - 1];
}

// exclusive prefix of v over the workgroup's 256 lanes; *total: the workgroup's sum
__device__ __forceinline__ int index_block_scan(int v, int* total) {
    __shared__ int wave_tot[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(incl, off, 64);
        if (lane >= off) incl += up;
    }
    __syncthreads();      // (the array may still be read from the call before)
    if (lane == 63) wave_tot[w] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) { before += ww < w ? wave_tot[ww] : 0; all += wave_tot[ww]; }
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(256) void index_tile_sums_kernel(const int* __restrict__ term, const int* __restrict__ doc, int64_t n,
                                                              int* __restrict__ tile_sums) {
    const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kIndexTile + threadIdx.x * kIndexItems;
    int mine = 0;
#pragma unroll
    for (int u = 0; u < kIndexItems; ++u) mine += (i0 + u < n && index_head(term, doc, i0 + u)) ? 1 : 0;
    int total;
    (void)index_block_scan(mine, &total);
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// sums[0 .. tiles) -> their exclusive prefixes, sums[tiles] = the total (below 2^31: there are fewer entries than that)
__global__ __launch_bounds__(256) void index_scan_sums_kernel(int* __restrict__ sums, int64_t tiles) {
    int carry = 0;
    for (int64_t t0 = 0; t0 < tiles; t0 += 256) {
        const int64_t t = t0 + threadIdx.x;
        const int v = t < tiles ? sums[t] : 0;
        int total;
        const int ex = index_block_scan(v, &total);
        if (t < tiles) sums[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) sums[tiles] = carry;
}

__global__ __launch_bounds__(256) void index_write_kernel(const int* __restrict__ term, const int* __restrict__ doc, int64_t n, int64_t V,
                                                          const int* __restrict__ tile_sums, int64_t tiles, int* __restrict__ head_pos,
                                                          int* __restrict__ post_doc, int64_t* __restrict__ post_off, int64_t* __restrict__ tok_off) {
    const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kIndexTile + threadIdx.x * kIndexItems;
    bool head[kIndexItems];
    int mine = 0;
#pragma unroll
    for (int u = 0; u < kIndexItems; ++u) { head[u] = i0 + u < n && index_head(term, doc, i0 + u); mine += head[u] ? 1 : 0; }
    int total;
    int64_t p = static_cast<int64_t>(tile_sums[blockIdx.x]) + index_block_scan(mine, &total);
#pragma unroll
    for (int u = 0; u < kIndexItems; ++u) {
        const int64_t i = i0 + u;
        if (head[u]) {
            head_pos[p] = static_cast<int>(i);
            post_doc[p] = doc[i];
            const int t = term[i];
            const int before = i == 0 ? -1 : term[i - 1];
            for (int64_t x = static_cast<int64_t>(before) + 1; x <= t; ++x) { post_off[x] = p; tok_off[x] = i; }      // (none when the term goes on)
            ++p;
        }
        if (i == n - 1) {      // the last entry closes the arrays
            const int64_t P = tile_sums[tiles];
            for (int64_t x = static_cast<int64_t>(term[i]) + 1; x <= V; ++x) { post_off[x] = P; tok_off[x] = n; }
            head_pos[P] = static_cast<int>(n);      // (n < 2^31)
        }
    }
}

__global__ __launch_bounds__(256) void index_tf_kernel(const int* __restrict__ head_pos, int64_t P, int* __restrict__ post_tf) {
    for (int64_t p = blockIdx.x * 256ll + threadIdx.x; p < P; p += static_cast<int64_t>(gridDim.x) * 256) post_tf[p] = head_pos[p + 1] - head_pos[p];
}

// ---- a slab's fill from postings --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void index_fill_kernel(float* __restrict__ p, int64_t n) {
    for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) p[i] = -__builtin_inff();
}

// lo[s], hi[s]: the postings of terms[s] whose documents lie in [d0, d0 + S)
__global__ __launch_bounds__(256) void index_bounds_kernel(const int64_t* __restrict__ post_off, const int* __restrict__ post_doc,
                                                           const int* __restrict__ terms, int n, int64_t d0, int S, int64_t* __restrict__ lo,
                                                           int64_t* __restrict__ hi) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int64_t b = post_off[terms[s]], e = post_off[terms[s] + 1];
    const int64_t l = index_lower_bound(post_doc, b, e, d0);
    lo[s] = l;
    hi[s] = index_lower_bound(post_doc, l, e, d0 + S);
}

// tf of document d in the postings [lo, hi) of one term; 0: the term does not hold it
__device__ __forceinline__ int index_tf_of(const int* __restrict__ post_doc, const int* __restrict__ post_tf, int64_t lo, int64_t hi, int d) {
    const int64_t p = index_lower_bound(post_doc, lo, hi, d);
    return (p < hi && post_doc[p] == d) ? post_tf[p] : 0;
}

// true: an earlier entry of the query holds d, so this posting does not own (q, d). (The entries before j are of other terms: j is
// its term's first.)
__device__ __forceinline__ bool index_owned_earlier(const PostingsArgs& a, int j0, int j, int d) {
    for (int jj = j0; jj < j; ++jj) {
        const int s = a.tslot[jj];
        if (index_tf_of(a.post_doc, a.post_tf, a.lo[s], a.hi[s], d) > 0) return true;
    }
    return false;
}

// w·a rounded on its own (lexical.hip lex_weighted)
__device__ __forceinline__ double index_weighted(double w, double a) {
#pragma clang fp contract(off)
    return w * a;
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void lex_postings_kernel(PostingsArgs a) {
    for (int j = blockIdx.y; j < a.num_entries; j += gridDim.y) {
        if (!a.first[j]) continue;
        const int slot = a.tslot[j], q = a.entry_query[j];
        const int j0 = a.qoff[q], j1 = a.qoff[q + 1];
        const int64_t end = a.hi[slot];
        for (int64_t p = a.lo[slot] + blockIdx.x * 256ll + threadIdx.x; p < end; p += static_cast<int64_t>(gridDim.x) * 256) {
            const int d = a.post_doc[p];
            if (index_owned_earlier(a, j0, j, d)) continue;
            const int own = a.post_tf[p];
            const int64_t lo = a.doc_offsets[d], hi = a.doc_offsets[d + 1];
            const double len = static_cast<double>(hi - lo);
            const double log_den = a.method == NVSM_LEX_DIRICHLET ? log(len + a.param) : 0.0;
            const double jm_scale = hi > lo ? (1.0 - a.param) / len : 0.0;
            double sum = 0.0;
            for (int jj = j0; jj < j1; ++jj) {
                const int s = a.tslot[jj];
                const int t = jj < j ? 0 : (s == slot ? own : index_tf_of(a.post_doc, a.post_tf, a.lo[s], a.hi[s], d));
                double term;
                if (t > 0) {
                    term = a.method == NVSM_LEX_DIRICHLET ? log((static_cast<double>(t) + a.c0[jj]) / (len + a.param))
                                                          : log(jm_scale * static_cast<double>(t) + a.c0[jj]);
                } else {
                    term = a.base[jj] - log_den;
                }
                sum += WEIGHTED ? index_weighted(a.weight[jj], term) : term;
            }
            a.scores[static_cast<size_t>(q) * a.ld + (d - a.d0)] = static_cast<float>(sum);
        }
    }
}

template <bool WEIGHTED>
__global__ __launch_bounds__(256) void tfidf_postings_kernel(PostingsArgs a) {
#pragma clang fp contract(off)
    const double k1p = a.k1 + 1.0;
    for (int j = blockIdx.y; j < a.num_entries; j += gridDim.y) {
        if (!a.first[j]) continue;
        const int slot = a.tslot[j], q = a.entry_query[j];
        const int j0 = a.qoff[q], j1 = a.qoff[q + 1];
        const int64_t end = a.hi[slot];
        for (int64_t p = a.lo[slot] + blockIdx.x * 256ll + threadIdx.x; p < end; p += static_cast<int64_t>(gridDim.x) * 256) {
            const int d = a.post_doc[p];
            if (index_owned_earlier(a, j0, j, d)) continue;
            const int own = a.post_tf[p];
            const int64_t lo = a.doc_offsets[d], hi = a.doc_offsets[d + 1];
            const double K = a.k1 * ((1.0 - a.b) + a.b * (static_cast<double>(hi - lo) / a.avgdl));
            double sum = 0.0;
            for (int jj = j; jj < j1; ++jj) {      // (the entries before j are worth exactly 0 here)
                const int s = a.tslot[jj];
                const int t = s == slot ? own : index_tf_of(a.post_doc, a.post_tf, a.lo[s], a.hi[s], d);
                if (t == 0) continue;
                const double tfd = static_cast<double>(t);
                const double term = (a.c0[jj] * (tfd * k1p)) / (tfd + K);
                sum += WEIGHTED ? a.weight[jj] * term : term;
            }
            a.scores[static_cast<size_t>(q) * a.ld + (d - a.d0)] = static_cast<float>(sum);
        }
    }
}

int index_grid(int64_t n) { return stream_grid(n, 256); }

}  // namespace

int64_t index_tiles(int64_t n) { return (n + kIndexTile - 1) / kIndexTile; }

void launch_index_docs(int* pos, int64_t n, const int64_t* doc_offsets, int64_t num_documents, hipStream_t s) {
    if (n > 0) NVSM_LAUNCH(index_docs_kernel, dim3(index_grid(n)), dim3(256), 0, s, pos, n, doc_offsets, num_documents);
}

void launch_index_positions(int* pos, int* doc, int64_t n, const int64_t* doc_offsets, int64_t num_documents, hipStream_t s) {
    if (n > 0) NVSM_LAUNCH(index_positions_kernel, dim3(index_grid(n)), dim3(256), 0, s, pos, doc, n, doc_offsets, num_documents);
}

void launch_index_fill(float* p, int64_t n, hipStream_t s) {
    if (n > 0) NVSM_LAUNCH(index_fill_kernel, dim3(index_grid(n)), dim3(256), 0, s, p, n);
}

void launch_index_bounds(const int64_t* post_off, const int* post_doc, const int* terms, int n, int64_t d0, int S, int64_t* lo, int64_t* hi,
                         hipStream_t s) {
    if (n > 0) NVSM_LAUNCH(index_bounds_kernel, dim3((n + 255) / 256), dim3(256), 0, s, post_off, post_doc, terms, n, d0, S, lo, hi);
}

void launch_index_scan(const int* term, const int* doc, int64_t n, int* tile_sums, hipStream_t s) {
    if (n <= 0) return;
    const int64_t tiles = index_tiles(n);
    NVSM_LAUNCH(index_tile_sums_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, s, term, doc, n, tile_sums);
    NVSM_LAUNCH(index_scan_sums_kernel, dim3(1), dim3(256), 0, s, tile_sums, tiles);
}

void launch_index_write(const int* term, const int* doc, int64_t n, int64_t V, const int* tile_sums, int* head_pos, int* post_doc,
                        int64_t* post_off, int64_t* tok_off, hipStream_t s) {
    if (n <= 0) return;
    const int64_t tiles = index_tiles(n);
    NVSM_LAUNCH(index_write_kernel, dim3(static_cast<unsigned>(tiles)), dim3(256), 0, s, term, doc, n, V, tile_sums, tiles, head_pos, post_doc,
                post_off, tok_off);
}

void launch_index_tf(const int* head_pos, int64_t P, int* post_tf, hipStream_t s) {
    if (P > 0) NVSM_LAUNCH(index_tf_kernel, dim3(index_grid(P)), dim3(256), 0, s, head_pos, P, post_tf);
}

void launch_postings_fill(const PostingsArgs& a, int64_t max_df, bool tfidf, hipStream_t s) {
    if (a.S <= 0 || a.Q <= 0) return;
    NVSM_LAUNCH(index_fill_kernel, dim3(index_grid(static_cast<int64_t>(a.Q) * a.ld)), dim3(256), 0, s, a.scores, static_cast<int64_t>(a.Q) * a.ld);
    if (a.num_slots <= 0 || a.num_entries <= 0) return;
    NVSM_LAUNCH(index_bounds_kernel, dim3((a.num_slots + 255) / 256), dim3(256), 0, s, a.post_off, a.post_doc, a.terms, a.num_slots, a.d0, a.S,
                a.lo, a.hi);
    // x: the workgroups one list is spread over, sized by the longest list the round can meet inside a slab; y: the round's entries
    const int64_t longest = std::max<int64_t>(1, std::min<int64_t>(max_df, a.S));
    const unsigned gx = static_cast<unsigned>(std::min<int64_t>((longest + 255) / 256, 256));
    const unsigned gy = static_cast<unsigned>(std::min(a.num_entries, 65535));
    if (tfidf) {
        if (a.weight) NVSM_LAUNCH(tfidf_postings_kernel<true>, dim3(gx, gy), dim3(256), 0, s, a);
        else NVSM_LAUNCH(tfidf_postings_kernel<false>, dim3(gx, gy), dim3(256), 0, s, a);
    } else {
        if (a.weight) NVSM_LAUNCH(lex_postings_kernel<true>, dim3(gx, gy), dim3(256), 0, s, a);
        else NVSM_LAUNCH(lex_postings_kernel<false>, dim3(gx, gy), dim3(256), 0, s, a);
    }
}

}  // namespace cunvsm
