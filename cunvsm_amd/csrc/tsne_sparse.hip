// Sparse-affinity t-SNE of table rows (include/cunvsm_amd.h nvsm_tsne_sparse): sklearn.manifold.TSNE with
// method='barnes_hut' at angle = 0 — each row keeps its k nearest neighbours, P is a CSR matrix of O(n·k) entries, the attraction
// runs over its stored entries and the repulsion is the exact all-pairs sum, read from Y alone. Nothing here holds n × n values.
// Arithmetic and order follow tsne.hip: what runs once per call is fp64 in a fixed order, the per-iteration pair arithmetic is
// fp32 (rcp and one Newton step), and every sum across lanes, tiles, ranges and rows is a fixed tree or an ascending fp64 sum.
// No float atomics: a repeated call returns the same bits.
#include <cmath>

#include "device_utils.h"
#include "kernels.h"

namespace cunvsm {

namespace {

constexpr double kTsneEps = 2.220446049250313e-16;      // sklearn's MACHINE_EPSILON
constexpr double kTsneTiny = 1.1754943508222875e-38;    // np.finfo(np.float32).tiny (_barnes_hut_tsne.pyx FLOAT32_TINY)
constexpr int kDistTile = 16, kDistK = 32;               // tsne_nn_dist_kernel: 16 × 16 cells a workgroup, 32 columns of X a stage
constexpr int kRepRows = 64;                             // tsne_sp_repulsion_kernel: rows a workgroup (4 waves × 4 groups × 4 rows)
constexpr int kRepTileMax = 4096;                        // ... and the widest LDS tile of Y (32 KiB)
constexpr int kReduceThreads = 1024;

inline unsigned cdiv_u(int64_t a, int64_t b) { return static_cast<unsigned>((a + b - 1) / b); }

// tsne.hip's block_sum_f64: the threads' values in LDS, then a binary tree; every thread calls it and gets the total
template <int T>
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = T / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

// Σ over the wave in fp64 by a butterfly: both partners of a step add the same two values, so every lane ends with the same bits
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// 1 / s for s >= 1 as tsne_forces_kernel takes it: the hardware reciprocal and one Newton step
__device__ __forceinline__ float tsne_q(float s) {
    const float q = __builtin_amdgcn_rcpf(s);
    return fmaf(q, fmaf(-s, q, 1.f), q);
}

// ---- neighbour rounds: the score slab of qn query rows against the rows [j0, j0 + S) --------------------------------------------
// scores[i − q0][j − j0] = −fp32(Σ_t (x_it − x_jt)²), the sum in fp64 in ascending t (tsne_dist_kernel's arithmetic: (i, j) and
// (j, i) give the same float); −inf at j == i. The negation is 0 − d, so a distance of 0 gives +0 and never −0: rank.hip's keys
// order the two zeros apart, and equal distances must tie into ascending ids.
__global__ __launch_bounds__(256) void tsne_nn_dist_kernel(const float* __restrict__ X, int n, int d, int q0, int qn, int j0, int S,
                                                           float* __restrict__ scores, int64_t ld) {
    __shared__ float xi[kDistTile][kDistK + 1], xj[kDistTile][kDistK + 1];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kDistTile + tx;
    const int ib = blockIdx.y * kDistTile, jb = blockIdx.x * kDistTile;      // offsets inside the round and the slab
    double acc = 0.0;
    for (int k0 = 0; k0 < d; k0 += kDistK) {
        for (int e = tid; e < kDistTile * kDistK; e += 256) {
            const int r = e / kDistK, c = e % kDistK;
            const bool col = k0 + c < d;
            xi[r][c] = (col && ib + r < qn) ? X[static_cast<size_t>(q0 + ib + r) * d + k0 + c] : 0.f;
            xj[r][c] = (col && jb + r < S) ? X[static_cast<size_t>(j0 + jb + r) * d + k0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kDistK; ++c) {
            const double df = static_cast<double>(xi[ty][c]) - static_cast<double>(xj[tx][c]);
            acc = fma(df, df, acc);
        }
        __syncthreads();
    }
    const int i = ib + ty, j = jb + tx;
    if (i < qn && j < S) scores[static_cast<size_t>(i) * ld + j] = (q0 + i == j0 + j) ? -__builtin_inff() : 0.f - static_cast<float>(acc);
}

// the round's sorted keys (rank.hip: score key << 32 | ~id, descending) -> nbr_id / nbr_d2 [q0 + q][0 .. k), nearest first
__global__ __launch_bounds__(256) void tsne_nn_write_kernel(const unsigned long long* __restrict__ keys, int64_t npad, int qn, int k, int q0,
                                                            int* __restrict__ nbr_id, float* __restrict__ nbr_d2) {
    const int64_t t = blockIdx.x * 256ll + threadIdx.x;
    if (t >= static_cast<int64_t>(qn) * k) return;
    const int q = static_cast<int>(t / k), r = static_cast<int>(t % k);
    const unsigned long long key = keys[static_cast<size_t>(q) * npad + r];
    const unsigned u = static_cast<unsigned>(key >> 32);
    const float score = __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);      // rank.hip rank_unkey
    const size_t o = static_cast<size_t>(q0 + q) * k + r;
    nbr_id[o] = static_cast<int>(0xffffffffu - static_cast<unsigned>(key));
    nbr_d2[o] = 0.f - score;
}

// ---- conditionals: sklearn's _binary_search_perplexity over a row's k distances, one wave a row, fp64 ----------------------------
// tsne_perplexity_kernel over a row of k entries with no diagonal to skip: a thread's entries ascending, then the LDS tree.
__global__ __launch_bounds__(64) void tsne_nn_perplexity_kernel(const float* __restrict__ d2, int k, double log_perplexity,
                                                                float* __restrict__ cond, double* __restrict__ rowsum) {
    __shared__ double sh[64];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* row = d2 + static_cast<size_t>(i) * k;
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
    double beta_used = 1.0, sum_used = 1.0;
    for (int step = 0; step < 100; ++step) {
        double sp = 0.0, sdp = 0.0;
        for (int j = tid; j < k; j += 64) {
            const double dd = static_cast<double>(row[j]);
            const double p = exp(-dd * beta);
            sp += p;
            sdp += dd * p;
        }
        sp = block_sum_f64<64>(sp, sh);
        sdp = block_sum_f64<64>(sdp, sh);
        if (sp == 0.0) sp = 1e-8;
        beta_used = beta;
        sum_used = sp;
        const double diff = log(sp) + beta * (sdp / sp) - log_perplexity;
        if (fabs(diff) <= 1e-5) break;      // (the same value in every thread: the branch is uniform)
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
    double rs = 0.0;
    for (int j = tid; j < k; j += 64) {
        const float c = static_cast<float>(exp(-static_cast<double>(row[j]) * beta_used) / sum_used);
        cond[static_cast<size_t>(i) * k + j] = c;
        rs += static_cast<double>(c);
    }
    rs = block_sum_f64<64>(rs, sh);
    if (tid == 0) rowsum[i] = rs;
}

// ---- symmetrisation: the 2·n·k directed entries, e < n·k the edge i → j as (row i, column j), e >= n·k the same edge as (j, i) ----
__device__ __forceinline__ int tsne_sym_row(const int* __restrict__ nbr_id, int64_t nk, int k, int64_t e) {
    return e < nk ? static_cast<int>(e / k) : nbr_id[e - nk];
}
__device__ __forceinline__ int tsne_sym_col(const int* __restrict__ nbr_id, int64_t nk, int k, int64_t e) {
    return e < nk ? nbr_id[e] : static_cast<int>((e - nk) / k);
}
// out[t] = the row (ROW) or column of entry perm[t] (perm null: entry t)
template <bool ROW>
__global__ __launch_bounds__(256) void tsne_sym_key_kernel(const int* __restrict__ nbr_id, int64_t nk, int k, const int* __restrict__ perm,
                                                           int* __restrict__ out) {
    for (int64_t t = blockIdx.x * 256ll + threadIdx.x; t < 2 * nk; t += static_cast<int64_t>(gridDim.x) * 256) {
        const int64_t e = perm ? perm[t] : t;
        out[t] = ROW ? tsne_sym_row(nbr_id, nk, k, e) : tsne_sym_col(nbr_id, nk, k, e);
    }
}
// data[p] = fp32((Σ of the conditionals of the run's entries) / max(total, eps)): a run holds one entry, or both directions of an
// edge. Two floats add exactly in fp64 and in either order, so (i, j) and (j, i) receive the same bits.
__global__ __launch_bounds__(256) void tsne_sym_values_kernel(const int* __restrict__ head_pos, const int* __restrict__ perm,
                                                              const float* __restrict__ cond, int64_t nnz, int64_t nk,
                                                              const double* __restrict__ total, float* __restrict__ data) {
    const double denom = fmax(2.0 * total[0], kTsneEps);
    for (int64_t p = blockIdx.x * 256ll + threadIdx.x; p < nnz; p += static_cast<int64_t>(gridDim.x) * 256) {
        double c = 0.0;
        for (int t = head_pos[p]; t < head_pos[p + 1]; ++t) {
            const int64_t e = perm[t];
            c += static_cast<double>(cond[e < nk ? e : e - nk]);
        }
        data[p] = static_cast<float>(c / denom);
    }
}

// ---- one iteration: attraction over the stored entries, a wave a row --------------------------------------------------------------
// attr[i] = Σ_{j in row i} P_ij q_ij (y_i − y_j): lanes stride the row's entries ascending, then the wave's DPP tree — the order
// depends on the row's length alone. A row may be as long as n − 1 (a hub lies in every list).
__global__ __launch_bounds__(256) void tsne_sp_attraction_kernel(const int64_t* __restrict__ indptr, const int* __restrict__ indices,
                                                                 const float* __restrict__ data, const float* __restrict__ Y, int n,
                                                                 float* __restrict__ attr) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;      // (wave-uniform)
    const float2 yi = reinterpret_cast<const float2*>(Y)[i];
    float ax = 0.f, ay = 0.f;
    const int64_t end = indptr[i + 1];
    for (int64_t p = indptr[i] + lane; p < end; p += 64) {
        const float2 yj = reinterpret_cast<const float2*>(Y)[indices[p]];
        const float dx = yi.x - yj.x, dy = yi.y - yj.y;
        const float pq = data[p] * tsne_q(1.f + dx * dx + dy * dy);
        ax += pq * dx;
        ay += pq * dy;
    }
    ax = wave_sum(ax);
    ay = wave_sum(ay);
    if (lane == 0) { attr[2 * i] = ax; attr[2 * i + 1] = ay; }
}

// ---- one iteration: repulsion, the hot path — tsne_forces_kernel without the P read ----------------------------------------------
// part[i][range] = (Σ q² dx, Σ q² dy, Σ q) over the range's j != i. A workgroup: 64 rows × one range of wr columns, walked in LDS
// tiles of tw columns of Y (a multiple of 256, at most 4096). A wave takes 4 rows at a time, 4 columns a lane. Sums: a lane's
// columns of the tile ascending in fp32, the wave's DPP tree, then the tiles in order in fp64 — lane 3·r + c of a wave keeps
// component c of the wave's row r, so the 48 running sums cost two registers.
__global__ __launch_bounds__(256) void tsne_sp_repulsion_kernel(const float* __restrict__ Y, int n, int wr, int tw, int ranges,
                                                                float* __restrict__ part) {
    extern __shared__ float ytile[];      // [tw][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int range = blockIdx.y, r_begin = range * wr, r_end = min(n, r_begin + wr);
    const int base = blockIdx.x * kRepRows + wave * 16;
    double run = 0.0;
    for (int c0 = r_begin; c0 < r_end; c0 += tw) {
        __syncthreads();      // (the tile before is read to its end)
        for (int e = tid; e < tw; e += 256) {
            const int j = c0 + e;
            reinterpret_cast<float2*>(ytile)[e] = j < r_end ? reinterpret_cast<const float2*>(Y)[j] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const int cend = min(tw, r_end - c0);
        for (int g = 0; g < 4; ++g) {
            const int r0 = base + g * 4;
            if (r0 >= n) break;               // (wave-uniform)
            int ri[4];
            float yix[4], yiy[4], acc[4][3];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                ri[u] = min(r0 + u, n - 1);   // (a row beyond n repeats the last one and is not written)
                yix[u] = Y[2 * ri[u]];
                yiy[u] = Y[2 * ri[u] + 1];
                acc[u][0] = acc[u][1] = acc[u][2] = 0.f;
            }
            for (int c = lane * 4; c < cend; c += 256) {
                float yj[8];
                {
                    float a[4], b[4];
                    ldv<4>(ytile + 2 * c, a);
                    ldv<4>(ytile + 2 * c + 4, b);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { yj[e] = a[e]; yj[4 + e] = b[e]; }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int j = c0 + c + e;
                        const bool valid = c + e < cend && j != ri[u];
                        const float dx = yix[u] - yj[2 * e], dy = yiy[u] - yj[2 * e + 1];
                        float q = tsne_q(1.f + dx * dx + dy * dy);
                        q = valid ? q : 0.f;
                        const float qq = q * q;
                        acc[u][0] += qq * dx;
                        acc[u][1] += qq * dy;
                        acc[u][2] += q;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const float v = wave_sum(acc[u][k]);
                    if (lane == (g * 4 + u) * 3 + k) run += static_cast<double>(v);
                }
            }
        }
    }
    const int row = base + lane / 3;
    if (lane < 48 && row < n) part[(static_cast<size_t>(row) * ranges + range) * 3 + lane % 3] = static_cast<float>(run);
}

// Z = Σ_i Σ_range part[i][range][2] in fp64: thread t adds rows t, t + 1024, ... (ranges in order), then the tree. One workgroup.
__global__ __launch_bounds__(kReduceThreads) void tsne_sp_z_kernel(const float* __restrict__ part, int n, int ranges, double* __restrict__ z) {
    __shared__ double sh[kReduceThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kReduceThreads)
        for (int k = 0; k < ranges; ++k) s += static_cast<double>(part[(static_cast<size_t>(i) * ranges + k) * 3 + 2]);
    s = block_sum_f64<kReduceThreads>(s, sh);
    if (threadIdx.x == 0) z[0] = s;
}

// ---- one iteration, last launch: tsne_update_kernel's arithmetic on the attraction and the repulsion partials ---------------------
__global__ __launch_bounds__(256) void tsne_sp_update_kernel(const float* __restrict__ attr, const float* __restrict__ part, int n, int ranges,
                                                             const double* __restrict__ z, float exaggeration, float momentum,
                                                             float learning_rate, float* __restrict__ Y, float* __restrict__ upd,
                                                             float* __restrict__ gains, float* __restrict__ gs, float* __restrict__ graw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double r[2] = {0.0, 0.0};
    for (int k = 0; k < ranges; ++k) {
        const float* p = part + (static_cast<size_t>(i) * ranges + k) * 3;
        r[0] += static_cast<double>(p[0]); r[1] += static_cast<double>(p[1]);
    }
    const double Z = z[0];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float g = static_cast<float>(4.0 * (static_cast<double>(exaggeration) * static_cast<double>(attr[2 * i + c]) - r[c] / Z));
        if (graw) graw[2 * i + c] = g;
        float u = upd[2 * i + c], ga = gains[2 * i + c];
        ga = (u * g < 0.f) ? ga + 0.2f : ga * 0.8f;
        ga = fmaxf(ga, 0.01f);
        g *= ga;
        u = momentum * u - learning_rate * g;
        gains[2 * i + c] = ga;
        upd[2 * i + c] = u;
        gs[2 * i + c] = g;
        Y[2 * i + c] += u;
    }
}

// ---- convergence check, fp64 throughout and with a Z of its own, as tsne_kl_rows_kernel has one ----------------------------------------
// The iteration's Z is a sum of fp32 terms: at the 1e-4 start every 1 + |y_i − y_j|² rounds the same way in fp32, a relative
// 1e-8 .. 6e-8 of Z that shows in the error times e (DESIGN.md §25 has the figures). zpart[workgroup] = Σ q over the workgroup's
// 64 rows × one column range, j != i: the repulsion's walk over LDS tiles of Y with fp64 pairs; a lane adds its pairs in a fixed
// order, then the LDS tree. The caller adds the partials up in order.
__global__ __launch_bounds__(256) void tsne_sp_z64_kernel(const float* __restrict__ Y, int n, int wr, int tw, double* __restrict__ zpart) {
    extern __shared__ float ytile[];      // [tw][2]
    __shared__ double sh[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r_begin = blockIdx.y * wr, r_end = min(n, r_begin + wr);
    const int base = blockIdx.x * kRepRows + wave * 16;
    double acc = 0.0;
    for (int c0 = r_begin; c0 < r_end; c0 += tw) {
        __syncthreads();
        for (int e = tid; e < tw; e += 256) {
            const int j = c0 + e;
            reinterpret_cast<float2*>(ytile)[e] = j < r_end ? reinterpret_cast<const float2*>(Y)[j] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        const int cend = min(tw, r_end - c0);
        for (int r = 0; r < 16; ++r) {
            const int i = base + r;
            if (i >= n) break;               // (wave-uniform)
            const double yx = static_cast<double>(Y[2 * i]), yy = static_cast<double>(Y[2 * i + 1]);
            for (int c = lane; c < cend; c += 64) {
                const double dx = yx - static_cast<double>(ytile[2 * c]), dy = yy - static_cast<double>(ytile[2 * c + 1]);
                const double q = 1.0 / (1.0 + dx * dx + dy * dy);
                acc += (c0 + c != i) ? q : 0.0;
            }
        }
    }
    acc = block_sum_f64<256>(acc, sh);
    if (tid == 0) zpart[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = acc;
}

// klrow[i] = Σ_{j in row i} e·P_ij · log(max(e·P_ij, tiny) / max(q_ij / z[0], tiny)), a wave a row: lanes stride the entries ascending
__global__ __launch_bounds__(256) void tsne_sp_kl_rows_kernel(const int64_t* __restrict__ indptr, const int* __restrict__ indices,
                                                              const float* __restrict__ data, const float* __restrict__ Y, int n,
                                                              const double* __restrict__ z, float exaggeration, double* __restrict__ klrow) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;      // (wave-uniform)
    const double yx = static_cast<double>(Y[2 * i]), yy = static_cast<double>(Y[2 * i + 1]), e = static_cast<double>(exaggeration);
    const double Z = z[0];
    double s = 0.0;
    const int64_t end = indptr[i + 1];
    for (int64_t p = indptr[i] + lane; p < end; p += 64) {
        const int j = indices[p];
        const double dx = yx - static_cast<double>(Y[2 * j]), dy = yy - static_cast<double>(Y[2 * j + 1]);
        const double q = 1.0 / (1.0 + dx * dx + dy * dy);
        const double pe = e * static_cast<double>(data[p]);
        s += pe * log(fmax(pe, kTsneTiny) / fmax(q / Z, kTsneTiny));
    }
    s = wave_sum_f64(s);
    if (lane == 0) klrow[i] = s;
}

}  // namespace

void tsne_sparse_layout(int n, int forced_ranges, int* wr, int* tw, int* ranges) {
    // about 1024 workgroups where n allows it; one range once the n / 64 row blocks fill the device on their own
    const int64_t row_blocks = (n + kRepRows - 1) / kRepRows;
    int64_t w;
    if (forced_ranges > 0) {
        w = std::max<int64_t>(1, (n + forced_ranges - 1) / forced_ranges);
    } else {
        const int64_t want = std::max<int64_t>(1, (1024 + row_blocks - 1) / row_blocks);
        w = (n + want - 1) / want;
        w = std::max<int64_t>(256, (w + 255) / 256 * 256);
    }
    *wr = static_cast<int>(w);
    *tw = static_cast<int>(std::min<int64_t>(kRepTileMax, (w + 255) / 256 * 256));
    *ranges = static_cast<int>((n + w - 1) / w);
}

void launch_tsne_nn_scores(const float* X, int n, int d, int q0, int qn, int j0, int S, float* scores, int64_t ld, hipStream_t s) {
    if (qn <= 0 || S <= 0) return;
    NVSM_LAUNCH(tsne_nn_dist_kernel, dim3(cdiv_u(S, kDistTile), cdiv_u(qn, kDistTile)), dim3(kDistTile, kDistTile), 0, s, X, n, d, q0, qn, j0, S,
                scores, ld);
}

void launch_tsne_nn_write(const unsigned long long* keys, int64_t npad, int qn, int k, int q0, int* nbr_id, float* nbr_d2, hipStream_t s) {
    NVSM_LAUNCH(tsne_nn_write_kernel, dim3(cdiv_u(static_cast<int64_t>(qn) * k, 256)), dim3(256), 0, s, keys, npad, qn, k, q0, nbr_id, nbr_d2);
}

void launch_tsne_nn_conditionals(const float* nbr_d2, int n, int k, float perplexity, float* cond, double* rowsum, hipStream_t s) {
    NVSM_LAUNCH(tsne_nn_perplexity_kernel, dim3(static_cast<unsigned>(n)), dim3(64), 0, s, nbr_d2, k, std::log(static_cast<double>(perplexity)),
                cond, rowsum);
}

void launch_tsne_sym_keys(const int* nbr_id, int n, int k, const int* perm, bool row, int* out, hipStream_t s) {
    const int64_t nk = static_cast<int64_t>(n) * k;
    if (row) NVSM_LAUNCH(tsne_sym_key_kernel<true>, dim3(stream_grid(2 * nk, 256)), dim3(256), 0, s, nbr_id, nk, k, perm, out);
    else NVSM_LAUNCH(tsne_sym_key_kernel<false>, dim3(stream_grid(2 * nk, 256)), dim3(256), 0, s, nbr_id, nk, k, perm, out);
}

void launch_tsne_sym_values(const int* head_pos, const int* perm, const float* cond, int64_t nnz, int n, int k, const double* total, float* data,
                            hipStream_t s) {
    if (nnz <= 0) return;
    NVSM_LAUNCH(tsne_sym_values_kernel, dim3(stream_grid(nnz, 256)), dim3(256), 0, s, head_pos, perm, cond, nnz, static_cast<int64_t>(n) * k, total,
                data);
}

void launch_tsne_sparse_forces(const int64_t* indptr, const int* indices, const float* data, const float* Y, int n, int forced_ranges, float* attr,
                               float* part, double* z, hipStream_t s) {
    int wr, tw, ranges;
    tsne_sparse_layout(n, forced_ranges, &wr, &tw, &ranges);
    NVSM_LAUNCH(tsne_sp_attraction_kernel, dim3(cdiv_u(n, 4)), dim3(256), 0, s, indptr, indices, data, Y, n, attr);
    NVSM_LAUNCH(tsne_sp_repulsion_kernel, dim3(cdiv_u(n, kRepRows), static_cast<unsigned>(ranges)), dim3(256),
                static_cast<size_t>(tw) * 2 * sizeof(float), s, Y, n, wr, tw, ranges, part);
    NVSM_LAUNCH(tsne_sp_z_kernel, dim3(1), dim3(kReduceThreads), 0, s, part, n, ranges, z);
}

void launch_tsne_sparse_update(const float* attr, const float* part, int n, int forced_ranges, const double* z, float exaggeration, float momentum,
                               float learning_rate, float* Y, float* upd, float* gains, float* gs, float* graw, hipStream_t s) {
    int wr, tw, ranges;
    tsne_sparse_layout(n, forced_ranges, &wr, &tw, &ranges);
    NVSM_LAUNCH(tsne_sp_update_kernel, dim3(cdiv_u(n, 256)), dim3(256), 0, s, attr, part, n, ranges, z, exaggeration, momentum, learning_rate, Y,
                upd, gains, gs, graw);
}

void launch_tsne_sparse_kl_rows(const int64_t* indptr, const int* indices, const float* data, const float* Y, int n, double* z64,
                                float exaggeration, double* klrow, hipStream_t s) {
    // klrow holds the partial sums of Z first (fewer than n: the layout of n alone), then, once they are added up, the rows of the error
    int wr, tw, ranges;
    tsne_sparse_layout(n, 0, &wr, &tw, &ranges);
    const unsigned row_blocks = cdiv_u(n, kRepRows);
    NVSM_LAUNCH(tsne_sp_z64_kernel, dim3(row_blocks, static_cast<unsigned>(ranges)), dim3(256), static_cast<size_t>(tw) * 2 * sizeof(float), s, Y, n,
                wr, tw, klrow);
    launch_kmeans_sum(klrow, static_cast<int64_t>(row_blocks) * ranges, z64, s);
    NVSM_LAUNCH(tsne_sp_kl_rows_kernel, dim3(cdiv_u(n, 4)), dim3(256), 0, s, indptr, indices, data, Y, n, z64, exaggeration, klrow);
}

}  // namespace cunvsm
