// k-means (Lloyd) of table rows (include/cunvsm_amd.h nvsm_kmeans; sklearn.cluster.KMeans(algorithm='lloyd')).
//
// Assignment — kmeans_assign_kernel — is the expansion |x − c|² = |x|² − 2 x·c + |c|² on rows and centres centred by the column
// mean of X, the products on the exact f32-input matrix instruction v_mfma_f32_16x16x4_f32 (an fmaf chain per cell: fp32
// accurate, bit-identical for identical rows or identical centres). A workgroup of four waves owns 128 rows, a wave 32 of them;
// it walks the centres in tiles of 128 and the columns in stages of 32 through LDS, and every lane carries a running (minimum,
// index) for the 8 rows of its accumulator cells across the centre tiles. Nothing n × k is written.
//
// Everything else is fp64 in a fixed order and free of float atomics: column mean / variance by row slabs, the centre update as
// a segmented sum over the rows sorted by label (sort_pairs is stable: positions ascend inside a label) cut into chunks of
// kSegChunk members whose partials are added in ascending chunk order — the association of a centre's sum depends on its member
// count alone —, direct (x − c)² for inertia, relocation and the k-means++ start, and a two-level sequential prefix for the draw.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "device_utils.h"
#include "kernels.h"

namespace cunvsm {

namespace {

constexpr int kAsgRows = 128;              // rows a workgroup (4 waves × 2 × 16)
constexpr int kAsgCent = 128;              // centres a tile (8 × 16 per wave)
constexpr int kAsgKc = 32;                 // columns a stage
constexpr int kAsgLd = kAsgKc + 4;         // LDS row stride in floats: rows stay 16-byte aligned
constexpr int kAsgCt = kAsgCent / 16;      // 16-centre groups a tile
constexpr int kSegChunk = 128;             // members a chunk of the segmented sum
constexpr int kStatSlabsMax = 512;         // row slabs of the column statistics
constexpr int kPrefChunk = 1024;           // positions a chunk of the k-means++ prefix
constexpr int kReduceThreads = 1024;

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline unsigned cdiv_u(int64_t a, int64_t b) { return static_cast<unsigned>((a + b - 1) / b); }

// Σ over the workgroup in a fixed order (LDS, then a binary tree); T threads, a power of two; every thread calls it
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

// Σ over the wave's lanes in a fixed order (a butterfly); every lane gets the total
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- column statistics ------------------------------------------------------------------------------------------------------------
// part [slabs][d] = Σ over the slab's rows, ascending, of x (mean null) or (x − mean)²; one thread a column
__global__ __launch_bounds__(256) void kmeans_colpart_kernel(const float* __restrict__ X, int n, int d, int rows_per_slab,
                                                             const double* __restrict__ mean, double* __restrict__ part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    const int r0 = blockIdx.y * rows_per_slab;
    const int r1 = min(n, r0 + rows_per_slab);
    const double m = mean ? mean[c] : 0.0;
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) {
        const double v = static_cast<double>(X[static_cast<size_t>(r) * d + c]) - m;
        acc += mean ? v * v : v;
    }
    part[static_cast<size_t>(blockIdx.y) * d + c] = acc;
}
// out [d] = (Σ slabs in order) / n; out32 (may be null) its fp32 rounding
__global__ __launch_bounds__(256) void kmeans_colfinish_kernel(const double* __restrict__ part, int slabs, int d, int n,
                                                               double* __restrict__ out, float* __restrict__ out32) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= d) return;
    double acc = 0.0;
    for (int s = 0; s < slabs; ++s) acc += part[static_cast<size_t>(s) * d + c];
    acc /= static_cast<double>(n);
    out[c] = acc;
    if (out32) out32[c] = static_cast<float>(acc);
}
// *out = mean over the columns of var [d], in ascending order
__global__ void kmeans_varmean_kernel(const double* __restrict__ var, int d, double* __restrict__ out) {
    double acc = 0.0;
    for (int c = 0; c < d; ++c) acc += var[c];
    *out = acc / static_cast<double>(d);
}

// ---- norms of the centred rows / the centred centres; a wave a row ------------------------------------------------------------------
// cc (may be null) [rows][d] = fp32(x − mean); norm [rows] = fp32(Σ fp64 of the squares of those fp32 values)
__global__ __launch_bounds__(256) void kmeans_center_rows_kernel(const float* __restrict__ X, int64_t rows, int d, const float* __restrict__ mean,
                                                                 float* __restrict__ cc, float* __restrict__ norm) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= rows) return;
    const float* x = X + static_cast<size_t>(r) * d;
    double acc = 0.0;
    for (int t = lane; t < d; t += 64) {
        const float v = x[t] - mean[t];
        if (cc) cc[static_cast<size_t>(r) * d + t] = v;
        acc += static_cast<double>(v) * static_cast<double>(v);
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) norm[r] = static_cast<float>(acc);
}

// ---- the fused assignment ----------------------------------------------------------------------------------------------------------
// label [n] = argmin_j (cn[j] − 2 xc_i·cc_j), the lowest j on a tie; dist [n] = max(xn[i] + that minimum, 0).
// Lane l of a wave holds A[row l & 15][k slot l >> 4] and B[k slot l >> 4][centre l & 15]; a 16-column group is spread over the
// slots so that slot q owns columns 4q .. 4q + 3 (one 16-byte LDS read) and the four MFMAs of the group take one of them each —
// any assignment of columns to slots gives the same dot product as long as rows and centres use the same one. The accumulator
// cell (register r) is row 4 (l >> 4) + r, centre l & 15.
// VEC (d a multiple of 4): a stage is staged with 16-byte loads — a float4 of a row lies wholly inside d or wholly beyond it.
template <bool VEC>
__global__ __launch_bounds__(256, VEC ? 2 : 1) void kmeans_assign_kernel(const float* __restrict__ X, int n, int d, const float* __restrict__ mean,
                                                            const float* __restrict__ Cc, const float* __restrict__ cn,
                                                            const float* __restrict__ xn, int k, int* __restrict__ label,
                                                            float* __restrict__ dist) {
    __shared__ __attribute__((aligned(16))) float xs[kAsgRows * kAsgLd];
    __shared__ __attribute__((aligned(16))) float cs[kAsgCent * kAsgLd];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lq = lane >> 4;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kAsgRows;
    float best[2][4];
    int bidx[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) { best[m][r] = INFINITY; bidx[m][r] = 0; }

    for (int c0 = 0; c0 < k; c0 += kAsgCent) {
        f32x4 acc[2][kAsgCt];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < kAsgCt; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int groups = min(kAsgCt, (k - c0 + 15) / 16);      // 16-centre groups of this tile that hold a centre: the others are skipped
        for (int k0 = 0; k0 < d; k0 += kAsgKc) {
            __syncthreads();
            if (VEC) {
#pragma unroll
                for (int e = 0; e < kAsgRows * kAsgKc / 1024; ++e) {
                    const int idx = e * 256 + tid, r = idx / (kAsgKc / 4), c = (idx % (kAsgKc / 4)) * 4;
                    const int64_t gr = row0 + r;
                    const int gc = k0 + c;
                    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (gr < n && gc < d)
                        v = *reinterpret_cast<const f32x4*>(X + static_cast<size_t>(gr) * d + gc) - *reinterpret_cast<const f32x4*>(mean + gc);
                    *reinterpret_cast<f32x4*>(&xs[r * kAsgLd + c]) = v;
                }
#pragma unroll
                for (int e = 0; e < kAsgCent * kAsgKc / 1024; ++e) {
                    const int idx = e * 256 + tid, r = idx / (kAsgKc / 4), c = (idx % (kAsgKc / 4)) * 4;
                    const int gj = c0 + r, gc = k0 + c;
                    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (gj < k && gc < d) v = *reinterpret_cast<const f32x4*>(Cc + static_cast<size_t>(gj) * d + gc);
                    *reinterpret_cast<f32x4*>(&cs[r * kAsgLd + c]) = v;
                }
            } else {
#pragma unroll
                for (int e = 0; e < kAsgRows * kAsgKc / 256; ++e) {
                    const int idx = e * 256 + tid, r = idx / kAsgKc, c = idx % kAsgKc;
                    const int64_t gr = row0 + r;
                    const int gc = k0 + c;
                    xs[r * kAsgLd + c] = (gr < n && gc < d) ? X[static_cast<size_t>(gr) * d + gc] - mean[gc] : 0.f;
                }
#pragma unroll
                for (int e = 0; e < kAsgCent * kAsgKc / 256; ++e) {
                    const int idx = e * 256 + tid, r = idx / kAsgKc, c = idx % kAsgKc;
                    const int gj = c0 + r, gc = k0 + c;
                    cs[r * kAsgLd + c] = (gj < k && gc < d) ? Cc[static_cast<size_t>(gj) * d + gc] : 0.f;
                }
            }
            __syncthreads();
            // a tile with all its groups runs the unguarded loop; the last tile of the call may skip the groups that hold no centre
            auto products = [&](auto all_groups) {
#pragma unroll
                for (int kk = 0; kk < kAsgKc / 16; ++kk) {
                    f32x4 a[2], b[kAsgCt];
#pragma unroll
                    for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const f32x4*>(&xs[(wave * 32 + m * 16 + li) * kAsgLd + kk * 16 + lq * 4]);
#pragma unroll
                    for (int t = 0; t < kAsgCt; ++t)
                        if (decltype(all_groups)::value || t < groups) b[t] = *reinterpret_cast<const f32x4*>(&cs[(t * 16 + li) * kAsgLd + kk * 16 + lq * 4]);
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int m = 0; m < 2; ++m)
#pragma unroll
                            for (int t = 0; t < kAsgCt; ++t)
                                if (decltype(all_groups)::value || t < groups)
                                    acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[m][s], b[t][s], acc[m][t], 0, 0, 0);
                }
            };
            if (groups == kAsgCt) products(std::true_type{}); else products(std::false_type{});
        }
        // centres ascend within a lane (tile, then t): a strict < keeps the lowest index of equal values
#pragma unroll
        for (int t = 0; t < kAsgCt; ++t) {
            const int j = c0 + t * 16 + li;
            if (j < k) {
                const float cj = cn[j];
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = cj - 2.f * acc[m][t][r];
                        if (v < best[m][r]) { best[m][r] = v; bidx[m][r] = j; }
                    }
            }
        }
    }
    // across the 16 lanes of a row: (value, index) in lexicographic order
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = best[m][r];
            int j = bidx[m][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const float ov = __shfl_xor(v, o, 64);
                const int oj = __shfl_xor(j, o, 64);
                if (ov < v || (ov == v && oj < j)) { v = ov; j = oj; }
            }
            const int64_t row = row0 + wave * 32 + m * 16 + lq * 4 + r;
            if (li == 0 && row < n) {
                label[row] = j;
                dist[row] = fmaxf(xn[row] + v, 0.f);
            }
        }
}

// ---- direct fp64 squared distances, a wave a row -----------------------------------------------------------------------------------
// out64 [n] = Σ_t (x_it − c_t)² for c = C[label[i]] (label given) or the row X[fixed] (label null); min_into: out64 = min(out64, ·);
// out32 (may be null) = its fp32 rounding
__global__ __launch_bounds__(256) void kmeans_rowdist_kernel(const float* __restrict__ X, int n, int d, const float* __restrict__ C,
                                                             const int* __restrict__ label, int64_t fixed, int min_into,
                                                             double* __restrict__ out64, float* __restrict__ out32) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const float* x = X + static_cast<size_t>(r) * d;
    const float* c = label ? C + static_cast<size_t>(label[r]) * d : X + static_cast<size_t>(fixed) * d;
    double acc = 0.0;
    for (int t = lane; t < d; t += 64) {
        const double v = static_cast<double>(x[t]) - static_cast<double>(c[t]);
        acc += v * v;
    }
    acc = wave_sum_f64(acc);
    if (lane == 0) {
        if (min_into) acc = fmin(acc, out64[r]);
        out64[r] = acc;
        if (out32) out32[r] = static_cast<float>(acc);
    }
}
// *out = Σ v [n]: thread partials in ascending strided order, then a tree
__global__ __launch_bounds__(kReduceThreads) void kmeans_sum_kernel(const double* __restrict__ v, int64_t n, double* __restrict__ out) {
    __shared__ double sh[kReduceThreads];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kReduceThreads) acc += v[i];
    acc = block_sum_f64<kReduceThreads>(acc, sh);
    if (threadIdx.x == 0) *out = acc;
}

// ---- centre update -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void kmeans_iota_kernel(int* __restrict__ v, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = i;
}
// start [k + 1]: start[j] = the first sorted position whose label is >= j (start[k] = n)
__global__ __launch_bounds__(256) void kmeans_bounds_kernel(const int* __restrict__ key, int n, int k, int* __restrict__ start) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j > k) return;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (key[mid] < j) lo = mid + 1; else hi = mid;
    }
    start[j] = lo;
}
// choff [k + 1] = exclusive prefix of ceil(count_j / kSegChunk); counts [k] (int64); *n_empty. One workgroup of 1024 threads, each
// owning a run of consecutive clusters.
__global__ __launch_bounds__(1024) void kmeans_chunks_kernel(const int* __restrict__ start, int k, int* __restrict__ choff,
                                                             int64_t* __restrict__ counts, int* __restrict__ n_empty) {
    __shared__ int tot[1024], emp[1024];
    const int per = (k + 1023) / 1024, j0 = threadIdx.x * per, j1 = min(k, j0 + per);
    int mine = 0, e = 0;
    for (int j = j0; j < j1; ++j) {
        const int c = start[j + 1] - start[j];
        counts[j] = c;
        mine += (c + kSegChunk - 1) / kSegChunk;
        e += c == 0;
    }
    tot[threadIdx.x] = mine; emp[threadIdx.x] = e;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0, es = 0;
        for (int t = 0; t < 1024; ++t) { const int v = tot[t]; tot[t] = run; run += v; es += emp[t]; }
        choff[k] = run;
        *n_empty = es;
    }
    __syncthreads();
    int run = tot[threadIdx.x];
    for (int j = j0; j < j1; ++j) {
        choff[j] = run;
        run += (start[j + 1] - start[j] + kSegChunk - 1) / kSegChunk;
    }
}
// part [chunk][d] = Σ in ascending sorted position of the chunk's member rows (fp64); workgroup b is chunk b of the call
__global__ __launch_bounds__(256) void kmeans_segsum_kernel(const float* __restrict__ X, int d, const int* __restrict__ pos,
                                                            const int* __restrict__ start, const int* __restrict__ choff, int k,
                                                            double* __restrict__ part) {
    __shared__ int rows[kSegChunk];
    const int b = blockIdx.x;
    if (b >= choff[k]) return;
    int lo = 0, hi = k;      // the last j with choff[j] <= b: an empty cluster shares its offset with its successor, so this one has members
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (choff[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int j = lo;
    const int m0 = start[j] + (b - choff[j]) * kSegChunk, m1 = min(start[j + 1], m0 + kSegChunk);
    if (threadIdx.x < m1 - m0) rows[threadIdx.x] = pos[m0 + threadIdx.x];
    __syncthreads();
    for (int t = threadIdx.x; t < d; t += 256) {
        double acc = 0.0;
        for (int m = 0; m < m1 - m0; ++m) acc += static_cast<double>(X[static_cast<size_t>(rows[m]) * d + t]);
        part[static_cast<size_t>(b) * d + t] = acc;
    }
}
// Cnew [j] = fp32((Σ chunks of j in order) / count_j), or Cold [j] for a cluster without members; shift [j] = Σ_t (new − old)² (fp64)
__global__ __launch_bounds__(256) void kmeans_finish_kernel(const double* __restrict__ part, const int* __restrict__ start,
                                                            const int* __restrict__ choff, int d, const float* __restrict__ Cold,
                                                            float* __restrict__ Cnew, double* __restrict__ shift) {
    __shared__ double sh[256];
    const int j = blockIdx.x;
    const int b0 = choff[j], b1 = choff[j + 1], cnt = start[j + 1] - start[j];
    double sq = 0.0;
    for (int t = threadIdx.x; t < d; t += 256) {
        const float old = Cold[static_cast<size_t>(j) * d + t];
        float now = old;
        if (cnt > 0) {
            double acc = 0.0;
            for (int b = b0; b < b1; ++b) acc += part[static_cast<size_t>(b) * d + t];
            now = static_cast<float>(acc / static_cast<double>(cnt));
        }
        Cnew[static_cast<size_t>(j) * d + t] = now;
        const double df = static_cast<double>(now) - static_cast<double>(old);
        sq += df * df;
    }
    sq = block_sum_f64<256>(sq, sh);
    if (threadIdx.x == 0) shift[j] = sq;
}
// *changed += the number of rows whose label moved (an integer atomic per workgroup)
__global__ __launch_bounds__(256) void kmeans_changed_kernel(const int* __restrict__ a, const int* __restrict__ b, int n, int* __restrict__ changed) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int diff = i < n && a[i] != b[i];
    const int any = __syncthreads_or(diff);
    if (threadIdx.x == 0 && any) atomicAdd(changed, 1);
}

// ---- the k-means++ draw ------------------------------------------------------------------------------------------------------------
// prefix[p] = (chunk totals before p's chunk, added left to right) + (the chunk's values up to p, added left to right from 0);
// a chunk's total is its own last prefix, so the search below meets exactly the sums kmeans_kpp_chunk_kernel wrote.
__global__ __launch_bounds__(256) void kmeans_kpp_chunk_kernel(const double* __restrict__ dmin, int n, double* __restrict__ part) {
    __shared__ double sh[kPrefChunk];
    const int p0 = blockIdx.x * kPrefChunk, cnt = min(kPrefChunk, n - p0);
    for (int t = threadIdx.x; t < cnt; t += 256) sh[t] = dmin[p0 + t];
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int t = 0; t < cnt; ++t) acc += sh[t];
        part[blockIdx.x] = acc;
    }
}
// out[0] = total; out[1] = the lowest position whose inclusive prefix exceeds u · total (−1: there is none, total is 0)
__global__ __launch_bounds__(256) void kmeans_kpp_pick_kernel(const double* __restrict__ dmin, int n, const double* __restrict__ part,
                                                              int chunks, double u, double* __restrict__ out) {
    __shared__ double sh[kPrefChunk];
    __shared__ double s_total, s_base;
    __shared__ int s_chunk;
    double run = 0.0;
    for (int c0 = 0; c0 < chunks; c0 += kPrefChunk) {
        const int cnt = min(kPrefChunk, chunks - c0);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) sh[t] = part[c0 + t];
        __syncthreads();
        if (threadIdx.x == 0) for (int t = 0; t < cnt; ++t) run += sh[t];
    }
    if (threadIdx.x == 0) { s_total = run; s_chunk = -1; s_base = 0.0; }
    __syncthreads();
    const double target = u * s_total;
    run = 0.0;
    for (int c0 = 0; c0 < chunks; c0 += kPrefChunk) {
        const int cnt = min(kPrefChunk, chunks - c0);
        __syncthreads();
        if (s_chunk >= 0) break;
        for (int t = threadIdx.x; t < cnt; t += 256) sh[t] = part[c0 + t];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int t = 0; t < cnt; ++t) {
                const double next = run + sh[t];
                if (next > target) { s_chunk = c0 + t; s_base = run; break; }
                run = next;
            }
    }
    __syncthreads();
    const int chunk = s_chunk;
    if (chunk < 0) {
        if (threadIdx.x == 0) { out[0] = s_total; out[1] = -1.0; }
        return;
    }
    const int p0 = chunk * kPrefChunk, cnt = min(kPrefChunk, n - p0);
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += 256) sh[t] = dmin[p0 + t];
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0, found = -1.0;
        for (int t = 0; t < cnt; ++t) {
            acc += sh[t];
            if (s_base + acc > target) { found = static_cast<double>(p0 + t); break; }
        }
        out[0] = s_total;
        out[1] = found;
    }
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
bool kmeans_assign_uses_mfma(int d) { return d >= 1; }      // every dimension: a stage's columns beyond d are zeros in LDS

int kmeans_stat_slabs(int n) { return static_cast<int>(std::min<int64_t>(kStatSlabsMax, (static_cast<int64_t>(n) + 255) / 256)); }
int64_t kmeans_max_chunks(int64_t n, int k) { return (n + kSegChunk - 1) / kSegChunk + k; }
int64_t kmeans_prefix_chunks(int64_t n) { return (n + kPrefChunk - 1) / kPrefChunk; }

void launch_kmeans_colstats(const float* X, int n, int d, double* part, double* mean64, float* mean32, double* var, double* var_mean, hipStream_t s) {
    const int slabs = kmeans_stat_slabs(n), per = (n + slabs - 1) / slabs;
    const dim3 grid(cdiv_u(d, 256), slabs);
    hipLaunchKernelGGL(kmeans_colpart_kernel, grid, dim3(256), 0, s, X, n, d, per, static_cast<const double*>(nullptr), part);
    hipLaunchKernelGGL(kmeans_colfinish_kernel, dim3(cdiv_u(d, 256)), dim3(256), 0, s, part, slabs, d, n, mean64, mean32);
    hipLaunchKernelGGL(kmeans_colpart_kernel, grid, dim3(256), 0, s, X, n, d, per, static_cast<const double*>(mean64), part);
    hipLaunchKernelGGL(kmeans_colfinish_kernel, dim3(cdiv_u(d, 256)), dim3(256), 0, s, part, slabs, d, n, var, static_cast<float*>(nullptr));
    hipLaunchKernelGGL(kmeans_varmean_kernel, dim3(1), dim3(1), 0, s, var, d, var_mean);
}

void launch_kmeans_center_rows(const float* X, int64_t rows, int d, const float* mean, float* cc, float* norm, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(kmeans_center_rows_kernel, dim3(cdiv_u(rows, 4)), dim3(256), 0, s, X, rows, d, mean, cc, norm);
}

void launch_kmeans_assign(const float* X, int n, int d, const float* mean, const float* Cc, const float* cn, const float* xn, int k,
                          int* label, float* dist, hipStream_t s) {
    if (d % 4 == 0)
        hipLaunchKernelGGL(kmeans_assign_kernel<true>, dim3(cdiv_u(n, kAsgRows)), dim3(256), 0, s, X, n, d, mean, Cc, cn, xn, k, label, dist);
    else
        hipLaunchKernelGGL(kmeans_assign_kernel<false>, dim3(cdiv_u(n, kAsgRows)), dim3(256), 0, s, X, n, d, mean, Cc, cn, xn, k, label, dist);
}

void launch_kmeans_rowdist(const float* X, int n, int d, const float* C, const int* label, int64_t fixed, bool min_into, double* out64,
                           float* out32, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_rowdist_kernel, dim3(cdiv_u(n, 4)), dim3(256), 0, s, X, n, d, C, label, fixed, min_into ? 1 : 0, out64, out32);
}

void launch_kmeans_sum(const double* v, int64_t n, double* out, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_sum_kernel, dim3(1), dim3(kReduceThreads), 0, s, v, n, out);
}

void launch_kmeans_iota(int* v, int n, hipStream_t s) { hipLaunchKernelGGL(kmeans_iota_kernel, dim3(cdiv_u(n, 256)), dim3(256), 0, s, v, n); }

void launch_kmeans_segments(const int* sorted_label, int n, int k, int* start, int* choff, int64_t* counts, int* n_empty, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_bounds_kernel, dim3(cdiv_u(k + 1, 256)), dim3(256), 0, s, sorted_label, n, k, start);
    hipLaunchKernelGGL(kmeans_chunks_kernel, dim3(1), dim3(1024), 0, s, start, k, choff, counts, n_empty);
}

void launch_kmeans_update(const float* X, int n, int d, const int* pos, const int* start, const int* choff, int k, double* part,
                          const float* Cold, float* Cnew, double* shift, double* shift_total, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_segsum_kernel, dim3(static_cast<unsigned>(kmeans_max_chunks(n, k))), dim3(256), 0, s, X, d, pos, start, choff, k, part);
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(k), dim3(256), 0, s, part, start, choff, d, Cold, Cnew, shift);
    hipLaunchKernelGGL(kmeans_sum_kernel, dim3(1), dim3(kReduceThreads), 0, s, shift, static_cast<int64_t>(k), shift_total);
}

void launch_kmeans_changed(const int* a, const int* b, int n, int* changed, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_changed_kernel, dim3(cdiv_u(n, 256)), dim3(256), 0, s, a, b, n, changed);
}

void launch_kmeans_kpp_pick(const double* dmin, int n, double* part, double u, double* out, hipStream_t s) {
    const int chunks = static_cast<int>(kmeans_prefix_chunks(n));
    hipLaunchKernelGGL(kmeans_kpp_chunk_kernel, dim3(chunks), dim3(256), 0, s, dmin, n, part);
    hipLaunchKernelGGL(kmeans_kpp_pick_kernel, dim3(1), dim3(256), 0, s, dmin, n, part, chunks, u, out);
}

}  // namespace cunvsm
