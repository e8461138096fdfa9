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
// No float atomics, no inline assembly. All arena offsets are 64-bit.
#include <cstdint>
#include "../../include/cunvsm_amd.h"
#include "kernels.h"
#include "device_utils.h"

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

}  // namespace cunvsm
