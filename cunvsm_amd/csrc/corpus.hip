// Window references -> device batch (nvsm_step_windows and its siblings, include/cunvsm_amd.h "HBM-resident corpus").
//
// A window is 8 bytes: (document, first token inside the document). The corpus — token arena, document offsets, one instance
// weight per document, one feature weight per word — was put into HBM once by nvsm_corpus_upload; this kernel writes the four
// arrays of the nvsm_batch the references denote, in the ABI's own types (int64 ids, float weights), into a staging set of
// compute_cost. Everything behind it (narrowing, prologue, samplers, CSR builds) reads an ordinary device batch.
//
// Shape of the work: index arithmetic and a gather of contiguous tokens; bandwidth. Per window 8 B of reference and 8 B of offset
// in, 4·w B of tokens in, 12·w + 12 B out. A block takes a tile of 256 windows in two phases:
//   1  one lane per window: reference, doc_offsets[doc], doc_offsets[doc + 1] read ONCE, the verdict (good / bad) taken once, the
//      window's first arena index parked in LDS (-1: bad), label and instance weight stored;
//   2  one lane per FOUR consecutive output elements of the tile's [256·w] slice (its first element is a multiple of four, the
//      staging arrays come from hipMalloc): two 16-byte stores of ids, one 16-byte store of weights, for every w. A lane's
//      elements may belong to two windows (w not a multiple of 4): the window index is carried, not divided out again.
// A bad reference (document >= num_documents, or pos + w beyond the document's end) takes the same instructions as a good one
// with the arena index forced to 0 and the result to word 0 / label 0 (no early exit); it stores NVSM_BAD_WINDOW_REF into the
// engine's error word. The arena holds at least one token (the upload pads an empty corpus), so index 0 is always readable.
// All offsets are 64-bit.
#include "kernels.h"
#include "device_utils.h"

namespace cunvsm {

namespace {

constexpr int kTileWindows = 256;      // = the block size: phase 1 is one lane per window

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(kTileWindows) void window_expand_kernel(WindowExpandArgs a) {
    __shared__ int64_t first[kTileWindows];
    const int64_t tiles = (a.B + kTileWindows - 1) / kTileWindows;
    const int w = a.w;
    const int64_t n = a.B * w;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t win0 = tile * kTileWindows;
        {
            const int64_t i = win0 + threadIdx.x;
            if (i < a.B) {
                const uint2 ref = reinterpret_cast<const uint2*>(a.refs)[i];
                const bool doc_ok = static_cast<int64_t>(ref.x) < a.num_documents;
                const int64_t d = doc_ok ? static_cast<int64_t>(ref.x) : 0;      // (num_documents == 0: offsets[0], offsets[1] still exist — see the upload)
                const int64_t lo = a.doc_offsets[d], hi = a.doc_offsets[d + 1];
                const bool ok = doc_ok && static_cast<int64_t>(ref.y) + w <= hi - lo;
                if (!ok) *a.err_flag = NVSM_BAD_WINDOW_REF;
                first[threadIdx.x] = ok ? lo + static_cast<int64_t>(ref.y) : int64_t(-1);
                const int64_t label = ok ? d : 0;
                a.labels[i] = label;
                if (a.doc_weights) a.instw[i] = a.doc_weights[label];
            }
        }
        __syncthreads();
        const int64_t e0 = win0 * w;                                   // first output element of the tile
        const int64_t tile_full = static_cast<int64_t>(kTileWindows) * w;
        const int tile_n = static_cast<int>(n - e0 < tile_full ? n - e0 : tile_full);      // at most 256·w: 32-bit inside the tile
        for (int le = 4 * static_cast<int>(threadIdx.x); le < tile_n; le += 4 * kTileWindows) {
            int lw = le / w;                                          // window inside the tile, position inside the window
            int j = le - lw * w;
            long long id[4];
            float fw[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool live = le + q < tile_n;
                const int64_t f = live ? first[lw] : int64_t(-1);
                const bool ok = f >= 0;
                const int t = a.tokens[ok ? f + j : 0];
                id[q] = ok ? static_cast<long long>(t) : 0ll;
                fw[q] = a.term_weights ? a.term_weights[ok ? t : 0] : 0.f;
                if (++j == w) { j = 0; ++lw; }
            }
            const int64_t e = e0 + le;
            if (le + 4 <= tile_n) {
                i64x2* dst = reinterpret_cast<i64x2*>(a.words + e);
                dst[0] = i64x2{id[0], id[1]};
                dst[1] = i64x2{id[2], id[3]};
                if (a.term_weights) *reinterpret_cast<f32x4*>(a.wwts + e) = f32x4{fw[0], fw[1], fw[2], fw[3]};
            } else {                                                  // the batch's last one to three elements
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (le + q < tile_n) {
                        a.words[e + q] = id[q];
                        if (a.term_weights) a.wwts[e + q] = fw[q];
                    }
                }
            }
        }
        __syncthreads();      // (the next tile's phase 1 rewrites `first`)
    }
}

// nvsm_corpus_upload: every token must name a word of the model. One pass; the verdict is one int.
__global__ void corpus_check_tokens_kernel(const int* __restrict__ tokens, int64_t n, int64_t num_words, int* __restrict__ bad) {
    bool any = false;
    for (int64_t i = blockIdx.x * static_cast<int64_t>(blockDim.x) + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * blockDim.x)
        any |= static_cast<uint64_t>(static_cast<int64_t>(tokens[i])) >= static_cast<uint64_t>(num_words);
    if (any) *bad = 1;
}

}  // namespace

void launch_window_expand(const WindowExpandArgs& a, hipStream_t s) {
    if (a.B <= 0) return;
    // (a copy-stream kernel next to the step: a capped grid — 128 workgroups keep 0.5 M elements of the largest batch at four
    //  tiles each — so that it does not take the step's wave slots)
    const int64_t tiles = (a.B + kTileWindows - 1) / kTileWindows;
    const int grid = static_cast<int>(tiles < 128 ? tiles : 128);
    NVSM_LAUNCH(window_expand_kernel, dim3(grid), dim3(kTileWindows), 0, s, a);
}

void launch_corpus_check_tokens(const int* tokens, int64_t n, int64_t num_words, int* bad, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(corpus_check_tokens_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, s, tokens, n, num_words, bad);
}

}  // namespace cunvsm
