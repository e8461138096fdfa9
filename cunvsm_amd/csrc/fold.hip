// gfx950 kernels of the fold-in step (nvsm_step_fold): the documents update restricted to the rows
// [first, rows) of E. W, T, b and the rows below `first` are frozen, so nothing upstream of the loss has a gradient; what is
// left of a step behind the forward pass and the fused loss is
//     g_r = Σ coef[e] · proj[e / R],  q_r = Σ coef[e]² · pp[e / R]   over the entries e of the batch whose id is r >= first,
// and the optimiser's row formula (kernels.h RowKind) on those rows. The kernels read the documents CSR compute_cost builds
// anyway (row_begin / row_end / sorted_key / sorted_entry) and nothing else of it: the chunk lists of update.hip's passes
// cover the frozen rows too and their chunk length depends on the optimiser.
//
// Few new documents against a large batch is the normal case: one row then receives thousands of positives. So a row of
// more than kFoldChunk entries is cut into chunks of kFoldChunk entries, one wave each (fold_chunk_kernel), rows of more
// than kFoldGroup chunks get their chunk sums added in groups of kFoldGroup, one wave each (fold_group_kernel), and
// fold_rows_kernel — one wave per row — adds what is left and applies the formula. No atomics on data. The association of
// a row's sum depends on the row's entry count alone:
//     chunk c      = fma chain over entries [c·C, min((c + 1)·C, cnt)) of the row in ascending entry order, from 0
//     cnt <= C     : g = chunk 0
//     nch <= G     : g = 0 + chunk 0 + chunk 1 + …            (nch = ceil(cnt / C), left to right)
//     nch >  G     : group j = 0 + chunk jG + … + chunk min(nch, (j + 1)G) − 1;  g = 0 + group 0 + group 1 + …
// and q likewise — not on the grid, on max_batch_size, or on what the other rows of the batch hold.
//
// Where a chunk's sum is kept: the sorted entries are cut into SLOTS of kFoldChunk positions, a wave per slot, whose lanes
// look for chunk starts among their positions (position p opens a chunk iff its row is long and p − row_begin is a multiple
// of C). Two chunks of long rows that start in one slot belong to different rows, the first of them is its row's LAST chunk
// (index >= 1) and the second its row's FIRST (a third would need the second to be both): partial row 2·slot + (first chunk
// of its row) is free of collisions, and whoever needs chunk c of row r finds it from row_begin[r] alone. The same holds
// for the groups in windows of kFoldGroup · kFoldChunk positions.
#include "kernels.h"
#include "device_utils.h"

namespace cunvsm {

static_assert(kFoldChunk == 64, "a slot of the sorted entries is one wave's lanes");
constexpr int kFoldInFlight = 4;      // source rows / partials in flight per lane

template <int V>
__device__ __forceinline__ void fold_zero(float (&g)[V]) {
#pragma unroll
    for (int i = 0; i < V; ++i) g[i] = 0.f;
}

// g = Σ coef·X[src][col .. col + V), q = Σ coef²·sq[src] over the sorted entries [begin, end), ascending, one fma per entry
template <int V>
__device__ __forceinline__ void fold_gather(const FoldArgs& f, int begin, int end, int col, float (&g)[V], float& q) {
#pragma clang fp contract(off)
    const int last = end - 1;
    for (int e = begin; e < end; e += kFoldInFlight) {
        float cf[kFoldInFlight], sq[kFoldInFlight], x[kFoldInFlight][V];
#pragma unroll
        for (int u = 0; u < kFoldInFlight; ++u) {
            const uint32_t en = static_cast<uint32_t>(f.sorted_entry[min(e + u, last)]);
            const uint32_t src = static_cast<uint32_t>((static_cast<uint64_t>(en) * f.div_magic) >> 37);
            const float c = (e + u < end) ? f.coefs[en] : 0.f;      // slots past the end re-read the last entry with weight 0
            cf[u] = c;
            sq[u] = f.sq_src ? (c * c) * f.sq_src[src] : 0.f;
            ldv<V>(f.X + static_cast<size_t>(src) * f.dim + col, x[u]);
        }
#pragma unroll
        for (int u = 0; u < kFoldInFlight; ++u) {
            q += sq[u];
#pragma unroll
            for (int i = 0; i < V; ++i) g[i] = __builtin_fmaf(cf[u], x[u][i], g[i]);
        }
    }
}

// where the sum of the chunk that starts at sorted position p lives (first: it is chunk 0 of its row), and a group's likewise
__device__ __forceinline__ size_t fold_chunk_slot(int p, bool first) { return 2 * static_cast<size_t>(p / kFoldChunk) + (first ? 1 : 0); }
__device__ __forceinline__ size_t fold_group_slot(int p, bool first) { return 2 * static_cast<size_t>(p / (kFoldChunk * kFoldGroup)) + (first ? 1 : 0); }

// g, q += chunks [c0, c1) of the row that begins at rb, in chunk order
template <int V>
__device__ __forceinline__ void fold_sum_chunks(const FoldArgs& f, int rb, int c0, int c1, int col, float (&g)[V], float& q) {
    for (int c = c0; c < c1; c += kFoldInFlight) {
        float x[kFoldInFlight][V], pq[kFoldInFlight];
#pragma unroll
        for (int u = 0; u < kFoldInFlight; ++u) {
            const int cc = min(c + u, c1 - 1);
            const size_t slot = fold_chunk_slot(rb + cc * kFoldChunk, cc == 0);
            ldv<V>(f.partial + slot * f.dim + col, x[u]);
            pq[u] = f.partial_q[slot];
        }
#pragma unroll
        for (int u = 0; u < kFoldInFlight; ++u) {
            if (c + u < c1) {
                q += pq[u];
#pragma unroll
                for (int i = 0; i < V; ++i) g[i] += x[u][i];
            }
        }
    }
}

template <int V>
__device__ __forceinline__ void fold_sum_groups(const FoldArgs& f, int rb, int ngroups, int col, float (&g)[V], float& q) {
    for (int j = 0; j < ngroups; j += kFoldInFlight) {
        float x[kFoldInFlight][V], pq[kFoldInFlight];
#pragma unroll
        for (int u = 0; u < kFoldInFlight; ++u) {
            const int jj = min(j + u, ngroups - 1);
            const size_t slot = fold_group_slot(rb + jj * (kFoldChunk * kFoldGroup), jj == 0);
            ldv<V>(f.partial2 + slot * f.dim + col, x[u]);
            pq[u] = f.partial2_q[slot];
        }
#pragma unroll
        for (int u = 0; u < kFoldInFlight; ++u) {
            if (j + u < ngroups) {
                q += pq[u];
#pragma unroll
                for (int i = 0; i < V; ++i) g[i] += x[u][i];
            }
        }
    }
}

// stage 1 (GROUPS false): the chunk sums of the long rows; stage 2 (GROUPS true): the group sums of the rows of more than
// kFoldGroup chunks. A wave per slot of the sorted entries; slots whose entries all belong to frozen or short rows cost
// their keys and nothing else.
template <int V, bool GROUPS>
__global__ __launch_bounds__(256) void fold_partial_kernel(FoldArgs f, int nvec) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
    const int64_t nslots = (f.n + kFoldChunk - 1) / kFoldChunk;
    constexpr int kStride = GROUPS ? kFoldChunk * kFoldGroup : kFoldChunk;
    for (int64_t s = wave; s < nslots; s += nwaves) {
        const int64_t p = s * kFoldChunk + lane;
        int rb = 0, re = 0;
        bool start = false;
        if (p < f.n) {
            const int k = f.sorted_key[p];
            if (k >= f.first) {
                rb = f.row_begin[k]; re = f.row_end[k];
                const int cnt = re - rb, rel = static_cast<int>(p) - rb;
                const bool wanted = GROUPS ? (cnt > kFoldChunk * kFoldGroup) : (cnt > kFoldChunk);
                start = wanted && (rel % kStride == 0);
            }
        }
        uint64_t starts = __ballot(start);
        while (starts) {
            const int l = __ffsll(static_cast<long long>(starts)) - 1;
            starts &= starts - 1;
            const int pb = static_cast<int>(s * kFoldChunk) + l;
            const int rbl = __shfl(rb, l, 64), rel = __shfl(re, l, 64);
            for (int cv = lane; cv < nvec; cv += 64) {
                const int col = cv * V;
                float g[V];
                fold_zero<V>(g);
                float q = 0.f;
                size_t slot;
                if (GROUPS) {
                    const int nch = (rel - rbl + kFoldChunk - 1) / kFoldChunk;
                    const int c0 = (pb - rbl) / kFoldChunk;
                    fold_sum_chunks<V>(f, rbl, c0, min(nch, c0 + kFoldGroup), col, g, q);
                    slot = fold_group_slot(pb, pb == rbl);
                } else {
                    fold_gather<V>(f, pb, min(pb + kFoldChunk, rel), col, g, q);
                    slot = fold_chunk_slot(pb, pb == rbl);
                }
                stv<V>((GROUPS ? f.partial2 : f.partial) + slot * f.dim + col, g);
                if (cv == 0) (GROUPS ? f.partial2_q : f.partial_q)[slot] = q;
            }
        }
    }
}

// The row formula of update.hip's apply_row_formula_sc for columns [col, col + V) of row `row`, every product rounded on its own.
// sc_new: the row's scalar state coming out (kinds that have one).
template <int V>
__device__ __forceinline__ void fold_apply(const FoldArgs& f, size_t off, int cnt, const float (&g)[V], float q, float sc_old, float& sc_new) {
#pragma clang fp contract(off)
    const int kind = f.kind;
    const bool p_always = (f.decay != 1.f) || kind == ROW_ADAM_FULL || kind == ROW_ADAM_DENSE;
    const bool touch_p = p_always || cnt != 0;      // sparse kinds leave rows without entries alone when λ = 0
    float p[V], m[V], v[V];
    fold_zero<V>(p); fold_zero<V>(m); fold_zero<V>(v);
    const bool uses_m = kind == ROW_ADAM_SPARSE_ENT || kind == ROW_ADAM_DENSE || kind == ROW_ADAM_FULL;
    if (uses_m) ldv<V>(f.m + off, m);
    if (kind == ROW_ADAM_FULL) ldv<V>(f.v + off, v);
    if (touch_p) ldv<V>(f.P + off, p);
    if (kind == ROW_SGD) {
        if (!touch_p) return;
#pragma unroll
        for (int i = 0; i < V; ++i) p[i] = p[i] * f.decay + f.lr * g[i];
        stv<V>(f.P + off, p);
    } else if (kind == ROW_ADAGRAD_ENT) {
        const float acc = sc_old + q;
        sc_new = acc;
        if (!touch_p) return;
        const float sc = 1.f / sqrtf(acc + f.eps);
#pragma unroll
        for (int i = 0; i < V; ++i) p[i] = p[i] * f.decay + f.lr * (g[i] * sc);
        stv<V>(f.P + off, p);
    } else if (kind == ROW_ADAM_FULL) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float mn = m[i] * f.s_m + f.one_m_b1 * g[i];
            mn += (-f.c_reg) * p[i];
            float ag = g[i] + (-f.lambda) * p[i];
            ag = ag * ag;
            const float vn = v[i] * f.s_v + ag * f.one_m_b2;
            m[i] = mn;
            v[i] = vn;
            p[i] = p[i] + ((mn / (sqrtf(vn) + f.eps)) * f.bc) * f.lr;
        }
        stv<V>(f.m + off, m);
        stv<V>(f.v + off, v);
        stv<V>(f.P + off, p);
    } else {      // ROW_ADAM_SPARSE_ENT / ROW_ADAM_DENSE: one v per row
#pragma unroll
        for (int i = 0; i < V; ++i) m[i] = m[i] * f.s_m + f.one_m_b1 * g[i];
        stv<V>(f.m + off, m);
        const float vn = sc_old * f.s_v + f.one_m_b2 * q;
        sc_new = vn;
        const float denom = sqrtf(vn) + f.eps;
        if (kind == ROW_ADAM_SPARSE_ENT) {
            if (!touch_p) return;
            const float fc = static_cast<float>(cnt);
#pragma unroll
            for (int i = 0; i < V; ++i) p[i] = p[i] * f.decay + (f.lr * fc) * ((f.bc * m[i]) / denom);
            stv<V>(f.P + off, p);
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) p[i] = p[i] * f.decay + ((m[i] / denom) * f.bc) * f.lr;
            stv<V>(f.P + off, p);
        }
    }
}

// stage 3: a wave per new row — its sum out of entries, chunk sums or group sums, then the formula. The wave owns the row, so the
// scalar state is read (by every lane, before anything of the row is written) and written (by lane 0, last) in place.
template <int V>
__global__ __launch_bounds__(256) void fold_rows_kernel(FoldArgs f, int nvec) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = (static_cast<int64_t>(gridDim.x) * blockDim.x) >> 6;
    const bool scalar = f.kind == ROW_ADAGRAD_ENT || f.kind == ROW_ADAM_SPARSE_ENT || f.kind == ROW_ADAM_DENSE;
    for (int64_t row = f.first + wave; row < f.rows; row += nwaves) {
        const int rb = f.row_begin[row], re = f.row_end[row];
        const int cnt = re - rb;
        if (cnt == 0 && !f.dense) continue;
        const float sc_old = scalar ? f.sc[row] : 0.f;
        float sc_new = sc_old;
        for (int cv = lane; cv < nvec; cv += 64) {
            const int col = cv * V;
            float g[V];
            fold_zero<V>(g);
            float q = 0.f;
            if (cnt > kFoldChunk) {
                const int nch = (cnt + kFoldChunk - 1) / kFoldChunk;
                if (nch > kFoldGroup) fold_sum_groups<V>(f, rb, (nch + kFoldGroup - 1) / kFoldGroup, col, g, q);
                else fold_sum_chunks<V>(f, rb, 0, nch, col, g, q);
            } else if (cnt > 0) {
                fold_gather<V>(f, rb, re, col, g, q);
            }
            fold_apply<V>(f, static_cast<size_t>(row) * f.dim + col, cnt, g, q, sc_old, sc_new);
        }
        if (scalar && lane == 0) f.sc[row] = sc_new;
    }
}

void fold_partial_rows(int64_t max_entries, size_t* chunk_rows, size_t* group_rows) {
    *chunk_rows = 2 * static_cast<size_t>(max_entries / kFoldChunk + 1);
    *group_rows = 2 * static_cast<size_t>(max_entries / (kFoldChunk * kFoldGroup) + 1);
}

template <int V>
static void fold_dispatch(const FoldArgs& f, hipStream_t s) {
    const int nvec = f.dim / V;
    const int64_t slots = (f.n + kFoldChunk - 1) / kFoldChunk;
    const int slot_grid = stream_grid(slots * 64, 256);
    // (both stages always: whether a new row is long is known on the device only, and a slot without one is one key load per lane)
    if (f.n > kFoldChunk) hipLaunchKernelGGL((fold_partial_kernel<V, false>), dim3(slot_grid), dim3(256), 0, s, f, nvec);
    if (f.n > kFoldChunk * kFoldGroup) hipLaunchKernelGGL((fold_partial_kernel<V, true>), dim3(slot_grid), dim3(256), 0, s, f, nvec);
    hipLaunchKernelGGL((fold_rows_kernel<V>), dim3(stream_grid((f.rows - f.first) * 64, 256)), dim3(256), 0, s, f, nvec);
}

void launch_fold_update(const FoldArgs& f, hipStream_t s) {
    if (f.first >= f.rows) return;
    if (f.first < 0 || f.dim < 1 || f.n < 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "launch_fold_update: bad range");
    if (f.dim % 4 == 0) fold_dispatch<4>(f, s);
    else fold_dispatch<1>(f, s);
}

}  // namespace cunvsm
