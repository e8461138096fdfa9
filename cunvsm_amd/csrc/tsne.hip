// Exact t-SNE of table rows (include/cunvsm_amd.h nvsm_tsne; py/visualize.py's sklearn.manifold.TSNE).
// Everything that runs once per call — squared distances, the perplexity search, the joint probabilities, the PCA start, the
// KL of a convergence check — is fp64 in a fixed order. The per-iteration pair (tsne_forces_kernel, tsne_update_kernel) is fp32
// per pair, fp64 where slabs and rows are added up. No atomics anywhere: every sum is lane partials in ascending index, then a
// tree, then slabs / rows in order, so a repeated call returns the same bits.
// The n × n buffer (distances, then conditionals, then P) has rows of ld = n rounded up to 4 floats: 16-byte loads of a row
// start aligned. Cells beyond column n are never read as data (every reader masks j < n).
#include <cmath>

#include "device_utils.h"
#include "kernels.h"

namespace cunvsm {

namespace {

constexpr double kTsneEps = 2.220446049250313e-16;      // sklearn's MACHINE_EPSILON (np.finfo(np.double).eps)
constexpr int kDistTile = 16, kDistK = 32;               // tsne_dist_kernel: 16 × 16 cells a workgroup, 32 columns of X a stage
constexpr int kJointTile = 32;                           // tsne_joint_kernel: pairs of 32 × 32 tiles
constexpr int kForceRows = 64;                           // tsne_forces_kernel: rows a workgroup (4 waves × 4 groups × 4 rows)
constexpr int kForceSlabMax = 4096;                      // ... and the widest column slab (32 KiB of Y in LDS)
constexpr int kReduceThreads = 1024;                     // the one-workgroup sums

inline unsigned cdiv_u(int64_t a, int64_t b) { return static_cast<unsigned>((a + b - 1) / b); }

// Σ over the workgroup in a fixed order: the threads' values in LDS, then a binary tree. T threads, a power of two; every
// thread must call it, and every thread gets the total.
template <int T>
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    __syncthreads();      // (sh[0] of an earlier call may still be being read)
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = T / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

// ---- rows -----------------------------------------------------------------------------------------------------------------------
// x /= |x| in place, one workgroup a row; a zero row stays zero (inverse norm 0)
__global__ __launch_bounds__(256) void tsne_normalize_kernel(float* __restrict__ X, int d) {
    __shared__ double sh[256];
    float* x = X + static_cast<size_t>(blockIdx.x) * d;
    double s = 0.0;
    for (int t = threadIdx.x; t < d; t += 256) s += static_cast<double>(x[t]) * static_cast<double>(x[t]);
    s = block_sum_f64<256>(s, sh);
    const double inv = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
    for (int t = threadIdx.x; t < d; t += 256) x[t] = static_cast<float>(static_cast<double>(x[t]) * inv);
}

// ---- squared distances: D[i][j] = fp32(Σ_t (x_it − x_jt)²), the sum in fp64 in ascending t ------------------------------------------
// (i, j) and (j, i) add the same squares in the same order: the matrix is symmetric bit for bit, its diagonal exactly 0
__global__ __launch_bounds__(256) void tsne_dist_kernel(const float* __restrict__ X, int n, int d, float* __restrict__ D, int64_t ld) {
    __shared__ float xi[kDistTile][kDistK + 1], xj[kDistTile][kDistK + 1];
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kDistTile + tx;
    const int i0 = blockIdx.y * kDistTile, j0 = blockIdx.x * kDistTile;
    double acc = 0.0;
    for (int k0 = 0; k0 < d; k0 += kDistK) {
        for (int e = tid; e < kDistTile * kDistK; e += 256) {
            const int r = e / kDistK, c = e % kDistK;
            const bool col = k0 + c < d;      // (a column beyond d is 0 on both sides: its square adds an exact 0)
            xi[r][c] = (col && i0 + r < n) ? X[static_cast<size_t>(i0 + r) * d + k0 + c] : 0.f;
            xj[r][c] = (col && j0 + r < n) ? X[static_cast<size_t>(j0 + r) * d + k0 + c] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < kDistK; ++c) {
            const double df = static_cast<double>(xi[ty][c]) - static_cast<double>(xj[tx][c]);
            acc = fma(df, df, acc);
        }
        __syncthreads();
    }
    const int i = i0 + ty, j = j0 + tx;
    if (i < n && j < n) D[static_cast<size_t>(i) * ld + j] = static_cast<float>(acc);
}

// ---- perplexity search: sklearn's _binary_search_perplexity, one workgroup a row, fp64 ----------------------------------------------
// The row's distances are replaced by its conditional probabilities (fp32, 0 on the diagonal); rowsum[i] = their sum in fp64.
__global__ __launch_bounds__(256) void tsne_perplexity_kernel(float* __restrict__ D, int n, int64_t ld, double log_perplexity,
                                                              double* __restrict__ rowsum) {
    __shared__ double sh[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    float* row = D + static_cast<size_t>(i) * ld;
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
    double beta_used = 1.0, sum_used = 1.0;      // of the last evaluation: what the stored probabilities are made from
    for (int step = 0; step < 100; ++step) {
        double sp = 0.0, sdp = 0.0;
        for (int j = tid; j < n; j += 256) {
            if (j == i) continue;
            const double dd = static_cast<double>(row[j]);
            const double p = exp(-dd * beta);
            sp += p;
            sdp += dd * p;
        }
        sp = block_sum_f64<256>(sp, sh);
        sdp = block_sum_f64<256>(sdp, sh);
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
    for (int j = tid; j < n; j += 256) {
        const float c = j == i ? 0.f : static_cast<float>(exp(-static_cast<double>(row[j]) * beta_used) / sum_used);
        row[j] = c;
        rs += static_cast<double>(c);
    }
    rs = block_sum_f64<256>(rs, sh);
    if (tid == 0) rowsum[i] = rs;
}

// out[0] = Σ v[0 .. n) in a fixed order: thread t adds v[t], v[t + 1024], ..., then the tree. One workgroup.
__global__ __launch_bounds__(kReduceThreads) void tsne_sum_kernel(const double* __restrict__ v, int n, double* __restrict__ out) {
    __shared__ double sh[kReduceThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kReduceThreads) s += v[i];
    s = block_sum_f64<kReduceThreads>(s, sh);
    if (threadIdx.x == 0) out[0] = s;
}

// ---- joint probabilities in place: P = max((C + Cᵀ) / max(2·ΣC, eps), eps), diagonal 0 ---------------------------------------------
// A workgroup owns the tile pair (bi, bj), (bj, bi) with bi <= bj: both tiles are read whole before either is written.
__global__ __launch_bounds__(256) void tsne_joint_kernel(float* __restrict__ C, int n, int64_t ld, const double* __restrict__ total) {
    __shared__ float A[kJointTile][kJointTile + 1], B[kJointTile][kJointTile + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bi > bj) return;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const double denom = fmax(2.0 * total[0], kTsneEps);
    for (int r = ty; r < kJointTile; r += 8) {
        const int i = bi * kJointTile + r, j = bj * kJointTile + tx;
        A[r][tx] = (i < n && j < n) ? C[static_cast<size_t>(i) * ld + j] : 0.f;
        const int i2 = bj * kJointTile + r, j2 = bi * kJointTile + tx;
        B[r][tx] = (i2 < n && j2 < n) ? C[static_cast<size_t>(i2) * ld + j2] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < kJointTile; r += 8) {
        const int i = bi * kJointTile + r, j = bj * kJointTile + tx;
        if (i < n && j < n) {
            const double c = static_cast<double>(A[r][tx]) + static_cast<double>(B[tx][r]);
            C[static_cast<size_t>(i) * ld + j] = i == j ? 0.f : static_cast<float>(fmax(c / denom, kTsneEps));
        }
        const int i2 = bj * kJointTile + r, j2 = bi * kJointTile + tx;
        if (bi != bj && i2 < n && j2 < n) {
            const double c = static_cast<double>(B[r][tx]) + static_cast<double>(A[tx][r]);
            C[static_cast<size_t>(i2) * ld + j2] = static_cast<float>(fmax(c / denom, kTsneEps));
        }
    }
}

// ---- one iteration, first launch: the five partial sums of every row over one slab of columns -----------------------------------------
// part[i][slab] = (Σ P_ij q_ij dx, Σ P_ij q_ij dy, Σ q_ij² dx, Σ q_ij² dy, Σ q_ij) over the slab's j != i, q_ij = 1 / (1 + |y_i − y_j|²).
// A workgroup: 64 rows × one slab of wc columns (a multiple of 256), the slab's Y in LDS. A wave takes 4 rows at a time and
// reads each with 16-byte loads, 4 columns a lane; P is read exactly once per iteration. Sums: a lane's columns in ascending
// order, then the wave's DPP tree.
__global__ __launch_bounds__(256) void tsne_forces_kernel(const float* __restrict__ P, int64_t ld, const float* __restrict__ Y, int n,
                                                          int wc, int slabs, float* __restrict__ part) {
    extern __shared__ float ytile[];      // [wc][2]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int slab = blockIdx.y, c0 = slab * wc;
    for (int e = tid; e < wc; e += 256) {
        const int j = c0 + e;
        const float2 v = j < n ? reinterpret_cast<const float2*>(Y)[j] : make_float2(0.f, 0.f);
        reinterpret_cast<float2*>(ytile)[e] = v;
    }
    __syncthreads();
    const int cend = min(wc, n - c0);      // columns of the slab that exist (> 0 by the launcher's slab count)
    const int base = blockIdx.x * kForceRows + wave * 16;
    for (int g = 0; g < 4; ++g) {
        const int r0 = base + g * 4;
        if (r0 >= n) break;               // (wave-uniform)
        int ri[4];
        float yix[4], yiy[4], acc[4][5];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ri[u] = min(r0 + u, n - 1);   // (a row beyond n repeats the last one and is not written)
            yix[u] = Y[2 * ri[u]];
            yiy[u] = Y[2 * ri[u] + 1];
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[u][k] = 0.f;
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
                float p[4];
                ldv<4>(P + static_cast<size_t>(ri[u]) * ld + c0 + c, p);      // c0 + c <= ld − 4: inside the row
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = c0 + c + e;
                    const bool valid = j < n && j != ri[u];
                    const float dx = yix[u] - yj[2 * e], dy = yiy[u] - yj[2 * e + 1];
                    // the hardware reciprocal (1 ulp) and one Newton step: s >= 1, so nothing can overflow or go subnormal
                    const float s = 1.f + dx * dx + dy * dy;
                    float q = __builtin_amdgcn_rcpf(s);
                    q = fmaf(q, fmaf(-s, q, 1.f), q);
                    q = valid ? q : 0.f;
                    const float pq = (valid ? p[e] : 0.f) * q, qq = q * q;
                    acc[u][0] += pq * dx;
                    acc[u][1] += pq * dy;
                    acc[u][2] += qq * dx;
                    acc[u][3] += qq * dy;
                    acc[u][4] += q;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int k = 0; k < 5; ++k) acc[u][k] = wave_sum(acc[u][k]);
            if (lane == 0 && r0 + u < n) {
                float* o = part + (static_cast<size_t>(r0 + u) * slabs + slab) * 5;
#pragma unroll
                for (int k = 0; k < 5; ++k) o[k] = acc[u][k];
            }
        }
    }
}

// Z = Σ_i Σ_slab part[i][slab][4] in fp64: thread t adds rows t, t + 1024, ... (slabs in order), then the tree. One workgroup.
__global__ __launch_bounds__(kReduceThreads) void tsne_z_kernel(const float* __restrict__ part, int n, int slabs, double* __restrict__ z) {
    __shared__ double sh[kReduceThreads];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kReduceThreads)
        for (int k = 0; k < slabs; ++k) s += static_cast<double>(part[(static_cast<size_t>(i) * slabs + k) * 5 + 4]);
    s = block_sum_f64<kReduceThreads>(s, sh);
    if (threadIdx.x == 0) z[0] = s;
}

// ---- one iteration, second launch: the gradient of every row and sklearn's _gradient_descent step -------------------------------------
// g = 4·(e·Σ attractive − Σ repulsive / Z), slabs added in order in fp64; then per coordinate: gains += 0.2 where update·g < 0,
// else gains *= 0.8; gains >= 0.01; g *= gains; update = momentum·update − learning_rate·g; y += update. gs receives the
// gain-scaled gradient (whose norm the convergence check takes), graw (may be null) the gradient itself.
__global__ __launch_bounds__(256) void tsne_update_kernel(const float* __restrict__ part, int n, int slabs, const double* __restrict__ z,
                                                          float exaggeration, float momentum, float learning_rate, float* __restrict__ Y,
                                                          float* __restrict__ upd, float* __restrict__ gains, float* __restrict__ gs,
                                                          float* __restrict__ graw) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double a[2] = {0.0, 0.0}, r[2] = {0.0, 0.0};
    for (int k = 0; k < slabs; ++k) {
        const float* p = part + (static_cast<size_t>(i) * slabs + k) * 5;
        a[0] += static_cast<double>(p[0]); a[1] += static_cast<double>(p[1]);
        r[0] += static_cast<double>(p[2]); r[1] += static_cast<double>(p[3]);
    }
    const double Z = z[0];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        float g = static_cast<float>(4.0 * (static_cast<double>(exaggeration) * a[c] - r[c] / Z));
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

// ---- convergence check, fp64 throughout and with a Z of its own (the iteration's Z is a sum of fp32 terms), one workgroup a row:
// KL = false: klrow[i] = Σ_{j != i} q_ij;  KL = true: klrow[i] = Σ_{j != i} e·P_ij · log(max(e·P_ij, eps) / max(q_ij / z[0], eps))
template <bool KL>
__global__ __launch_bounds__(256) void tsne_kl_rows_kernel(const float* __restrict__ P, int64_t ld, const float* __restrict__ Y, int n,
                                                           const double* __restrict__ z, float exaggeration, double* __restrict__ klrow) {
    __shared__ double sh[256];
    const int i = blockIdx.x;
    const double yx = static_cast<double>(Y[2 * i]), yy = static_cast<double>(Y[2 * i + 1]), e = static_cast<double>(exaggeration);
    const double Z = KL ? z[0] : 1.0;
    const float* row = P + static_cast<size_t>(i) * ld;
    double s = 0.0;
    for (int j = threadIdx.x; j < n; j += 256) {
        if (j == i) continue;
        const double dx = yx - static_cast<double>(Y[2 * j]), dy = yy - static_cast<double>(Y[2 * j + 1]);
        const double q = 1.0 / (1.0 + dx * dx + dy * dy);
        if (KL) {
            const double p = e * static_cast<double>(row[j]);
            s += p * log(fmax(p, kTsneEps) / fmax(q / Z, kTsneEps));
        } else {
            s += q;
        }
    }
    s = block_sum_f64<256>(s, sh);
    if (threadIdx.x == 0) klrow[i] = s;
}

// out[0] = Σ klrow (rows in the fixed order of tsne_sum_kernel), out[1] = |gs| over the 2n gain-scaled components. One workgroup.
__global__ __launch_bounds__(kReduceThreads) void tsne_check_kernel(const double* __restrict__ klrow, const float* __restrict__ gs, int n,
                                                                    double* __restrict__ out) {
    __shared__ double sh[kReduceThreads];
    double s = 0.0, g = 0.0;
    for (int i = threadIdx.x; i < n; i += kReduceThreads) s += klrow[i];
    for (int i = threadIdx.x; i < 2 * n; i += kReduceThreads) g += static_cast<double>(gs[i]) * static_cast<double>(gs[i]);
    s = block_sum_f64<kReduceThreads>(s, sh);
    g = block_sum_f64<kReduceThreads>(g, sh);
    if (threadIdx.x == 0) { out[0] = s; out[1] = sqrt(g); }
}

// ---- PCA start --------------------------------------------------------------------------------------------------------------------
// mean[c] = Σ_i x_ic / n, one workgroup a column
__global__ __launch_bounds__(256) void tsne_colmean_kernel(const float* __restrict__ X, int n, int d, double* __restrict__ mean) {
    __shared__ double sh[256];
    const int c = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += static_cast<double>(X[static_cast<size_t>(i) * d + c]);
    s = block_sum_f64<256>(s, sh);
    if (threadIdx.x == 0) mean[c] = s / static_cast<double>(n);
}

// cov[a][b] = Σ_i (x_ia − mean_a)(x_ib − mean_b) in ascending i, 16 × 16 cells a workgroup; symmetric bit for bit
__global__ __launch_bounds__(256) void tsne_cov_kernel(const float* __restrict__ X, int n, int d, const double* __restrict__ mean,
                                                       double* __restrict__ cov) {
    __shared__ double xa[16][17], xb[16][17];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int a0 = blockIdx.y * 16, b0 = blockIdx.x * 16;
    double acc = 0.0;
    for (int i0 = 0; i0 < n; i0 += 16) {
        const int i = i0 + ty;      // this thread stages row i0 + ty, columns a0 + tx and b0 + tx
        xa[ty][tx] = (i < n && a0 + tx < d) ? static_cast<double>(X[static_cast<size_t>(i) * d + a0 + tx]) - mean[a0 + tx] : 0.0;
        xb[ty][tx] = (i < n && b0 + tx < d) ? static_cast<double>(X[static_cast<size_t>(i) * d + b0 + tx]) - mean[b0 + tx] : 0.0;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) acc = fma(xa[r][ty], xb[r][tx], acc);
        __syncthreads();
    }
    const int a = a0 + ty, b = b0 + tx;
    if (a < d && b < d) cov[static_cast<size_t>(a) * d + b] = acc;
}

// Y0[i][c] = fp32(Σ_t (x_it − mean_t)·V[c][t]), one wave a row
__global__ __launch_bounds__(64) void tsne_project_kernel(const float* __restrict__ X, int n, int d, const double* __restrict__ mean,
                                                          const double* __restrict__ V, float* __restrict__ Y0) {
    __shared__ double sh[64];
    const int i = blockIdx.x;
    double s0 = 0.0, s1 = 0.0;
    for (int t = threadIdx.x; t < d; t += 64) {
        const double xc = static_cast<double>(X[static_cast<size_t>(i) * d + t]) - mean[t];
        s0 += xc * V[t];
        s1 += xc * V[d + t];
    }
    s0 = block_sum_f64<64>(s0, sh);
    s1 = block_sum_f64<64>(s1, sh);
    if (threadIdx.x == 0) { Y0[2 * i] = static_cast<float>(s0); Y0[2 * i + 1] = static_cast<float>(s1); }
}

}  // namespace

int64_t tsne_ld(int64_t n) { return (n + 3) / 4 * 4; }

void tsne_force_layout(int n, int* wc, int* slabs) {
    // enough workgroups for 256 CUs four times over where n allows it: a small n splits its columns into more slabs
    const int64_t row_blocks = (n + kForceRows - 1) / kForceRows;
    int64_t want = std::max<int64_t>(1, (1024 + row_blocks - 1) / row_blocks);
    int64_t w = (n + want - 1) / want;
    w = std::min<int64_t>(kForceSlabMax, std::max<int64_t>(256, (w + 255) / 256 * 256));
    *wc = static_cast<int>(w);
    *slabs = static_cast<int>((n + w - 1) / w);
}

void launch_tsne_normalize(float* X, int n, int d, hipStream_t s) {
    NVSM_LAUNCH(tsne_normalize_kernel, dim3(static_cast<unsigned>(n)), dim3(256), 0, s, X, d);
}

void launch_tsne_conditionals(const float* X, int n, int d, float perplexity, float* P, double* rowsum, hipStream_t s) {
    const int64_t ld = tsne_ld(n);
    NVSM_LAUNCH(tsne_dist_kernel, dim3(cdiv_u(n, kDistTile), cdiv_u(n, kDistTile)), dim3(kDistTile, kDistTile), 0, s, X, n, d, P, ld);
    NVSM_LAUNCH(tsne_perplexity_kernel, dim3(static_cast<unsigned>(n)), dim3(256), 0, s, P, n, ld, std::log(static_cast<double>(perplexity)),
                rowsum);
}

void launch_tsne_joint(float* P, int n, const double* rowsum, double* total, hipStream_t s) {
    NVSM_LAUNCH(tsne_sum_kernel, dim3(1), dim3(kReduceThreads), 0, s, rowsum, n, total);
    NVSM_LAUNCH(tsne_joint_kernel, dim3(cdiv_u(n, kJointTile), cdiv_u(n, kJointTile)), dim3(kJointTile, 8), 0, s, P, n, tsne_ld(n), total);
}

void launch_tsne_forces(const float* P, const float* Y, int n, float* part, double* z, hipStream_t s) {
    int wc, slabs;
    tsne_force_layout(n, &wc, &slabs);
    NVSM_LAUNCH(tsne_forces_kernel, dim3(cdiv_u(n, kForceRows), static_cast<unsigned>(slabs)), dim3(256),
                static_cast<size_t>(wc) * 2 * sizeof(float), s, P, tsne_ld(n), Y, n, wc, slabs, part);
    NVSM_LAUNCH(tsne_z_kernel, dim3(1), dim3(kReduceThreads), 0, s, part, n, slabs, z);
}

void launch_tsne_update(const float* part, int n, const double* z, float exaggeration, float momentum, float learning_rate, float* Y,
                        float* upd, float* gains, float* gs, float* graw, hipStream_t s) {
    int wc, slabs;
    tsne_force_layout(n, &wc, &slabs);
    NVSM_LAUNCH(tsne_update_kernel, dim3(cdiv_u(n, 256)), dim3(256), 0, s, part, n, slabs, z, exaggeration, momentum, learning_rate, Y, upd,
                gains, gs, graw);
}

void launch_tsne_kl_rows(const float* P, const float* Y, int n, double* z64, float exaggeration, double* klrow, hipStream_t s) {
    // klrow holds the rows of Z first, then, once they are added up, the rows of the KL
    NVSM_LAUNCH(tsne_kl_rows_kernel<false>, dim3(static_cast<unsigned>(n)), dim3(256), 0, s, P, tsne_ld(n), Y, n, z64, exaggeration, klrow);
    NVSM_LAUNCH(tsne_sum_kernel, dim3(1), dim3(kReduceThreads), 0, s, klrow, n, z64);
    NVSM_LAUNCH(tsne_kl_rows_kernel<true>, dim3(static_cast<unsigned>(n)), dim3(256), 0, s, P, tsne_ld(n), Y, n, z64, exaggeration, klrow);
}

void launch_tsne_check(const double* klrow, const float* gs, int n, double* out, hipStream_t s) {
    NVSM_LAUNCH(tsne_check_kernel, dim3(1), dim3(kReduceThreads), 0, s, klrow, gs, n, out);
}

void launch_tsne_covariance(const float* X, int n, int d, double* mean, double* cov, hipStream_t s) {
    NVSM_LAUNCH(tsne_colmean_kernel, dim3(static_cast<unsigned>(d)), dim3(256), 0, s, X, n, d, mean);
    NVSM_LAUNCH(tsne_cov_kernel, dim3(cdiv_u(d, 16), cdiv_u(d, 16)), dim3(16, 16), 0, s, X, n, d, mean, cov);
}

void launch_tsne_project(const float* X, int n, int d, const double* mean, const double* V, float* Y0, hipStream_t s) {
    NVSM_LAUNCH(tsne_project_kernel, dim3(static_cast<unsigned>(n)), dim3(64), 0, s, X, n, d, mean, V, Y0);
}

}  // namespace cunvsm
