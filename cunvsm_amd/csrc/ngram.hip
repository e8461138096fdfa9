// gfx950 kernel of the n-gram search in document space (kernels.h "n-grams of terms").
//
// Reference semantics: TermBruteforcer (py/nvsm/base.py:106-162) stacks, for k = 1 .. max_ngram_cardinality, the projections
// Model::infer(mean of the k word rows) of every k-combination of the vocabulary in itertools.combinations order, and searches the
// stack by cosine distance. The projection is linear in front of the bias and the activation, so with G[i] = T·W[s_i] (made once per
// call by Model::project_words with c = 0 and the identity) a phrase row is
//   1-gram  a        f(G[a] + c·b)                      row a
//   2-gram  (a, b)   f(0.5·(G[a] + G[b]) + c·b)         row m + a·(2m − a − 1)/2 + (b − a − 1),  a < b < m
// with rank.hip's own bias-and-activation expression (device_utils.h rank_bias_act). ngram_rows_kernel writes the rows
// [p0, p0 + S) of that stack into a slab out[S][de] which nvsm_neighbors' scan then scores like any other table.
//
// Shape of the work: a wave owns kNgramWaveRows consecutive rows. Its first row is decoded ONCE, wave-uniformly — 1-gram below m,
// else the closed form a ≈ ((2m − 1) − sqrt((2m − 1)² − 8t)) / 2 of t = row − m with an integer fix-up against the runs' first rows —
// and from there every lane steps (a, b) by additions only. A row is de / V vectors of V floats (V = 4, 16 bytes per lane, where
// de % 4 == 0; V = 1 otherwise); min(64, de / V) lanes cover a row, and where that is fewer than 64 the wave covers 64 / that many
// rows per pass, so that a pass reads and writes whole rows and consecutive lanes touch consecutive addresses: consecutive rows of a
// run share G[a] and stream consecutive G[b], and the slab is written front to back. No atomics, no LDS, 64-bit row offsets.
#include <algorithm>
#include <cmath>
#include "kernels.h"
#include "device_utils.h"

namespace cunvsm {

namespace {

constexpr int kNgramWaveRows = 16, kNgramWaves = 4;      // rows of a wave; waves of a workgroup

// where row p of the stack stands: a 1-gram (b < 0: word a) or the 2-gram (a, b)
struct NgramPos { int a, b; };

// the first row of the run of a: a·(2m − a − 1)/2 (relative to the first 2-gram)
__device__ __forceinline__ int64_t ngram_run_start(int64_t a, int64_t m) { return a * (2 * m - a - 1) / 2; }

__device__ __forceinline__ NgramPos ngram_decode(int64_t p, int64_t m) {
    NgramPos r;
    if (p < m) { r.a = static_cast<int>(p); r.b = -1; return r; }
    const int64_t t = p - m;
    const double w = static_cast<double>(2 * m - 1);        // (2m − 1)² < 2^35: exact in a double
    int64_t a = static_cast<int64_t>((w - sqrt(w * w - 8.0 * static_cast<double>(t))) * 0.5);
    a = a < 0 ? 0 : (a > m - 2 ? m - 2 : a);
    while (a > 0 && ngram_run_start(a, m) > t) --a;
    while (a < m - 2 && ngram_run_start(a + 1, m) <= t) ++a;
    r.a = static_cast<int>(a);
    r.b = static_cast<int>(a + 1 + (t - ngram_run_start(a, m)));
    return r;
}

// n rows further (n >= 0); p: the row r stands for. May run past the last row (b >= m with a = m − 2 never happens for a row of
// the stack; a caller that steps beyond it does not use the result)
__device__ __forceinline__ NgramPos ngram_step(NgramPos r, int64_t p, int n, int m) {
    if (r.b < 0) {                                          // 1-grams: the next word, or across the boundary into the run of 0
        if (p + n < m) { r.a += n; return r; }
        r.b = 1 + static_cast<int>(p + n - m);
        r.a = 0;
    } else {
        r.b += n;
    }
    while (r.b >= m && r.a < m - 1) { const int over = r.b - m; ++r.a; r.b = r.a + 1 + over; }
    return r;
}

template <int V>
__global__ __launch_bounds__(64 * kNgramWaves) void ngram_rows_kernel(const float* __restrict__ G, int m, int de, const float* __restrict__ bias,
                                                                      float c, int act, float clip_min, float clip_max, int64_t p0, int S,
                                                                      float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (uniform: the decode is scalar work)
    const int dev = de / V;                                 // vectors of a row
    const int row_lanes = dev < 64 ? dev : 64;              // lanes that cover a row
    const int rpp = 64 / row_lanes;                         // rows of a pass
    const int sub = lane / row_lanes, col0 = lane - sub * row_lanes;
    const int r0 = (blockIdx.x * kNgramWaves + wave) * kNgramWaveRows;      // the wave's first row of the slab
    if (r0 >= S || sub >= rpp) return;
    const int r1 = r0 + kNgramWaveRows < S ? r0 + kNgramWaveRows : S;
    const int64_t first = p0 + r0;
    NgramPos at = ngram_step(ngram_decode(first, m), first, sub, m);
    for (int r = r0 + sub; r < r1; r += rpp) {
        const float* ga = G + static_cast<int64_t>(at.a) * de;
        const float* gb = at.b < 0 ? ga : G + static_cast<int64_t>(at.b) * de;
        float* o = out + static_cast<int64_t>(r) * de;
        for (int col = col0; col < dev; col += row_lanes) {
            float x[V], y[V], bv[V], z[V];
            ldv<V>(ga + col * V, x);
            ldv<V>(bias + col * V, bv);
            if (at.b < 0) {
#pragma unroll
                for (int i = 0; i < V; ++i) z[i] = rank_bias_act(x[i], bv[i], c, act, clip_min, clip_max);
            } else {
                ldv<V>(gb + col * V, y);
#pragma unroll
                for (int i = 0; i < V; ++i) z[i] = rank_bias_act(0.5f * (x[i] + y[i]), bv[i], c, act, clip_min, clip_max);
            }
            stv<V>(o + col * V, z);
        }
        at = ngram_step(at, p0 + r, rpp, m);
    }
}

}  // namespace

int64_t ngram_row_count(int64_t m, int max_cardinality) {
    if (m < 1 || max_cardinality < 1 || max_cardinality > 2) return -1;
    if (max_cardinality == 1) return m < (int64_t(1) << 31) ? m : -1;
    if (m > 65535) return -1;                               // m + m(m − 1)/2 >= 2^31 from 65 536 on
    return m + m * (m - 1) / 2;
}

void launch_ngram_rows(const float* G, int m, int de, const float* bias, float c, int act, int64_t p0, int S, float* out, hipStream_t s) {
    if (S <= 0) return;
    const int64_t rows = std::max(ngram_row_count(m, 1), ngram_row_count(m, 2));      // (beyond 65 535 words the stack is its 1-grams)
    if (rows < 0 || de < 1 || p0 < 0 || p0 + S > rows) throw Error(NVSM_ERR_INVALID_ARGUMENT, "launch_ngram_rows: rows outside the stack");
    const float lo = std::nextafter(-1.0f, -1.0f - 1e-5f), hi = std::nextafter(1.0f, 1.0f + 1e-5f);      // as launch_rank_bias_act
    const dim3 grid(static_cast<unsigned>((S + kNgramWaves * kNgramWaveRows - 1) / (kNgramWaves * kNgramWaveRows)));
    if (de % 4 == 0) NVSM_LAUNCH(ngram_rows_kernel<4>, grid, dim3(64 * kNgramWaves), 0, s, G, m, de, bias, c, act, lo, hi, p0, S, out);
    else NVSM_LAUNCH(ngram_rows_kernel<1>, grid, dim3(64 * kNgramWaves), 0, s, G, m, de, bias, c, act, lo, hi, p0, S, out);
}

}  // namespace cunvsm
