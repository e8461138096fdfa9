// Launchers of the hand-written gfx950 kernels of the NVSM / LSE hot path. Host-callable; every
// launcher enqueues on the given stream and returns immediately. See DESIGN.md for the data layout
// and the per-kernel roofline; each kernel cites the reference code it replaces.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>

#include <stdexcept>
#include <string>

#include "tuning.h"

namespace cunvsm {

// what every layer below the C ABI throws; c_api.cpp turns it into an nvsm_status + nvsm_last_error() (status: NVSM_ERR_*)
struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};

// An event recorded behind a kernel is a packet of its own which the stream's next kernel waits for: a bubble of 6-10 us
// per record on the step's critical stream. A kernel launched through NVSM_LAUNCH right after set_launch_events(start, stop)
// carries them as its own start / completion events instead (hipExtLaunchKernelGGL): `stop` means the same for whoever waits
// on it as a record behind the kernel, and a (start, stop) pair made with timing brackets exactly the kernel's execution —
// no packet between the kernel and its neighbours either way. take_launch_events() hands the pending events to the launch
// (or back to the caller, who records them the plain way when the launcher launched nothing). Per host thread.
void set_launch_events(hipEvent_t start, hipEvent_t stop);
hipEvent_t take_launch_events(hipEvent_t* start);      // returns the stop event
#define NVSM_LAUNCH(kernel, grid, block, shmem, stream, ...)                                                       \
    do {                                                                                                          \
        hipEvent_t _start = nullptr;                                                                              \
        hipEvent_t _stop = ::cunvsm::take_launch_events(&_start);                                                 \
        if (_stop || _start)                                                                                      \
            hipExtLaunchKernelGGL(kernel, grid, block, shmem, stream, _start, _stop, 0, __VA_ARGS__);             \
        else                                                                                                      \
            hipLaunchKernelGGL(kernel, grid, block, shmem, stream, __VA_ARGS__);                                  \
    } while (0)

// How a reader brings the rows of a lazily decayed table up to date while it gathers them (see "lazy dense decay" below):
// row r has had `stamp[r]` updates applied, the table `now`; the factors of the updates in between are applied to the
// loaded values one by one, in update order — the roundings of the dense passes — without writing anything back.
constexpr int kLazyHistory = 128;
struct LazyView {
    const int* stamp;               // null: the table is current (no lazy decay)
    int now;
    float decay[kLazyHistory];      // factor of update u + 1 on the table rows at [u % kLazyHistory]
};

// Workspace of the ordered grid-wide sums (device_utils.h grid_sum_ordered): the batch-norm column statistics out of the
// projection GEMM's epilogue and [loss | Σdy | Σdy·x̂] out of the loss kernel are added up in a fixed order — same bits
// every run, no atomics on data. `colgroups` independent sums (column parts / tiles of a GEMM; 1 for the loss kernel), each
// of up to `contrib_cap` contributions of up to `width_cap` values: fp64 from the projection products (their tile sums are
// fp64 — see the pivot in their epilogues), fp32 from the loss kernel (which uses the buffer as floats).
struct GridSumWs {
    double* part;       // [colgroups][contrib_cap][width_cap]
    double* part2;      // [colgroups][groups_cap][width_cap]
    int* arrive;        // [colgroups][groups_cap + 1], zero between launches
    int colgroups, contrib_cap, groups_cap, width_cap, fan;
};
// The bf16 planes of the new T for the next step's projection products, written by the update itself (a thread holds the new
// element anyway: two launches of 5 us less behind the update, on the stream the next forward product waits for).
// kind 0: none; 1: gemm_split.hip's layout (dim = padded columns np); 2: gemm_rsplit.hip's (dim = 32-column tiles).
// transposed 0: the forward product's B (k = row of the stored T = word dimension, n = entity dimension); 1: the backward one's.
struct PlaneTarget { unsigned char* planes; size_t plane_stride; int kind; int dim; int transposed; };
// batch-norm backward (or, pre == null, the bias gradient alone) riding on the backward projection product: see launch_gemm_rows
struct BnDxFused { float* dy; const float* pre; const float* mean; const float* inv_std; const double* sums;
                   float* dbeta; float* dgamma; float* grad_bias; double n_global; };
// the word gather-mean (launch_gather_mean's arguments) riding on the forward projection product's staging of A (gemm_rsplit.hip,
// gemm_split.hip): phrase[b] = (Σ_j wts[b, j] · table[idx[b, j]]) / window is formed as the product stages its rows and written
// out on the way, bit for bit what the gather kernel writes
struct GatherFused { const float* table; const int* idx; const float* wts; int window; const LazyView* lazy; };
// planes of the small operand for the split-bf16 GEMM (gemm_split.hip; see launch_gemm_split)
// ... and for the split-bf16 row-panel kernel of the per-rank batch sizes (gemm_rsplit.hip), which wants them in another order
struct GemmSplitWs { void* planes; size_t bytes; bool ready; void* rplanes; size_t rbytes; bool rready; };
inline int grid_sum_fan(int contributions) { return contributions > 256 ? 32 : 16; }

// ---- gather-mean (F3/F9; replaces average_repr_kernel, cpp/params.cu:75-95) ------------------
void launch_gather_mean(const float* table, int dim, const int* idx, const float* wts, int window,
                        int64_t num_out, float* out, hipStream_t s, const LazyView* lazy = nullptr);

int window_unroll(int window);      // rows of a window in flight per lane in the window-major gathers (gather-mean, adam_u)

// ---- fp32 MFMA GEMM (F5, B6, B7; replaces the cuBLAS calls at cpp/params.cu:417,528, objective.cu:453)
// C[M][N] = alpha * A·B (+ bias[n]).  a_layout 0: A is [M][K] (lda); 1: A is stored [K][M] (lda).
//                                      b_layout 0: B is [K][N] (ldb); 1: B is stored [N][K] (ldb).
// split_k > 1: the K range is cut into split_k slabs, slab z writes C + z * c_split_stride (no bias/alpha fold
// is lost: alpha applied per slab, bias must be null) and the caller reduces with launch_splitk_reduce.
void launch_gemm(int a_layout, int b_layout, const float* A, const float* B, float* C, int M, int N, int K,
                 int lda, int ldb, int ldc, float alpha, const float* bias_n, int split_k, size_t c_split_stride,
                 hipStream_t s, double* colstats = nullptr,     // colstats [2][N] (no split-K): = Σ_rows C, Σ_rows C² (needs `sums`)
                 float* rowsq = nullptr, float rowsq_scale = 0.f, int* rowsq_parts = nullptr,
                 bool busy_chip = false,      // the launch lands next to long-running kernels of other streams (kernel choice)
                 const GridSumWs* sums = nullptr,       // workspace of the ordered column sums (required with colstats)
                 GemmSplitWs* split_ws = nullptr);      // planes of B for the split-bf16 kernel (null: exact-fp32 MFMA kernels)
// rowsq [gemm_rowsq_parts(N)][M]: rowsq_scale · Σ_cols C² per row, split by column tile (128 columns in the tiled kernel,
// 16 in the LDS-stationary one): *rowsq_parts = the number of parts this launch wrote; launch_sum_parts adds them in
// order (a runtime-length loop over the parts inside the row passes' unrolled gather was measured: it halves their
// speed, so the parts are combined once up front)
int gemm_rowsq_parts(int N);             // upper bound of *rowsq_parts: sizes the buffer
// LDS-stationary kernel for the batch-sized projection products (gemm_tstat.hip); false = shape not covered
bool launch_gemm_tstat(int a_layout, int b_layout, const float* A, const float* B, float* C, int M, int N, int K,
                       int lda, int ldb, int ldc, float alpha, const float* bias_n, hipStream_t s, double* colstats,
                       float* rowsq, float rowsq_scale, int* rowsq_parts, bool busy_chip = false, const GridSumWs* sums = nullptr);
// Row-panel kernel for per-rank batch sizes (gemm_rows.hip): a workgroup owns 32 rows and all N <= 320 columns.
// A [M][K] row-major; b_layout as launch_gemm. colstats (+ sums): ordered column sums of the output; rowsq [M]: COMPLETE
// rowsq_scale · Σ_cols C² per row (no parts); bn: the batch-norm backward of launch_bn_dx applied to the rows of A as they are
// loaded, dx written back over dy (b_layout 1 only); bn with pre == null: only grad_bias = (float) sums[k] (no batch-norm: what
// launch_colsum_finalize does). false: shape not covered, nothing launched.
bool launch_gemm_rows(int b_layout, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                      float alpha, const float* bias_n, hipStream_t s, double* colstats, const GridSumWs* sums, float* rowsq,
                      float rowsq_scale, const BnDxFused* bn);
bool gemm_rows_covers(int b_layout, int M, int N, int K, bool colstats, bool rowsq, bool bn);      // what launch_gemm_rows accepts
// The same decomposition on the bf16 matrix pipe (gemm_rsplit.hip; arithmetic of launch_gemm_split below): the workgroup's whole
// 32 x K panel of A cut into bf16 planes in LDS at once, B as planes in MFMA fragment order from L2 (GemmSplitWs::rplanes,
// gemm_rsplit_planes_bytes(N, K) bytes, cut here unless `rready`), a barrier-free K loop. Arguments as launch_gemm_rows.
size_t gemm_rsplit_planes_bytes(int N, int K);
void launch_gemm_rsplit_planes(int b_layout, const float* B, int N, int K, int ldb, void* planes, hipStream_t s);
// gf (forward product, b_layout 0, lda == K): the word gather-mean of launch_gather_mean rides on the staging of A — A is then
// WRITTEN (the phrase matrix [M][K], the gather kernel's bits) instead of read: see GatherFused.
bool launch_gemm_rsplit(int b_layout, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                        float alpha, const float* bias_n, hipStream_t s, double* colstats, const GridSumWs* sums, float* rowsq,
                        float rowsq_scale, GemmSplitWs* ws, const BnDxFused* bn, const GatherFused* gf = nullptr);
bool gemm_rsplit_covers(int b_layout, int M, int N, int K, bool colstats, bool rowsq, bool bn);
bool gemm_rsplit_gather_covers(int M, int N, int K, bool colstats, int window);      // ... with the gather inside
// Split-bf16 kernel for large batches (gemm_split.hip): fp32 operands cut exactly into three bf16 planes, nine (or six) bf16
// MFMAs per product with fp32 accumulation. rowsq [M]: COMPLETE rowsq_scale · Σ_cols C² per row. false: not covered / switched off.
// B travels as its three bf16 planes (GemmSplitWs::planes, gemm_split_planes_bytes(N, K) bytes, owned by the caller): cut by a
// small launch in front of the product unless `ready` says they are current — the caller clears `ready` whenever B changes.
size_t gemm_split_planes_bytes(int N, int K);
PlaneTarget gemm_split_plane_target(int N, int K, void* planes, int transposed);       // for TransformUpdateArgs::pt
PlaneTarget gemm_rsplit_plane_target(int N, int K, void* planes, int transposed);
void launch_gemm_split_planes(int b_layout, const float* B, int N, int K, int ldb, void* planes, hipStream_t s);
bool launch_gemm_split(int b_layout, const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                       float alpha, const float* bias_n, hipStream_t s, double* colstats, const GridSumWs* sums, float* rowsq,
                       float rowsq_scale, GemmSplitWs* ws, const BnDxFused* bn = nullptr);      // bn: as launch_gemm_rows (b_layout 1 only)
bool gemm_split_covers(int b_layout, int M, int N, int K, bool bn);      // shapes launch_gemm_split accepts
// dT = Aᵀ[M x rows] · B[rows x N], split-K over the rows (the batch), split-bf16 arithmetic (gemm_dt.hip): A [rows][M] (lda),
// B [rows][N] (ldb), partial [gemm_dt_slabs(rows, want)][M][N] — never more slabs than `want` —; the caller adds the slabs with
// launch_splitk_reduce. false: shape not covered, nothing launched.
bool gemm_dt_covers(int M, int N, int rows);
int gemm_dt_slabs(int rows, int want);
int gemm_dt_default_slabs(int rows, int cus);      // a slab per two CUs (two workgroups per slab), at least 64 rows each
bool launch_gemm_dt(const float* A, const float* B, float* partial, int M, int N, int rows, int lda, int ldb, int want_slabs, hipStream_t s);
// The same product in workgroups of ONE wave (gemm_dtw.hip, round 6): 32 x 64 tiles of the output per wave and slab, no LDS, no barrier —
// for per-rank batches, where the product runs next to both table passes and a whole-CU (or four-wave) workgroup waits for room.
bool gemm_dtw_covers(int M, int N, int rows);
int gemm_dtw_slabs(int rows, int want);
bool launch_gemm_dtw(const float* A, const float* B, float* partial, int M, int N, int rows, int lda, int ldb, int want_slabs, hipStream_t s);
// What each of the four batch-sized kernels would do with a shape and an epilogue — host arithmetic only, no HIP call, the
// functions the launchers themselves decide by (tests/test_gemm_plans.py reads them through nvsm_debug_gemm_plan). false: refused.
struct TstatPlan { int parts, NT, KG, wide, inst; bool mixed; size_t lds; };      // inst: which compiled (KG, NT, layout, mixed) form
bool gemm_tstat_plan(int b_layout, int M, int N, int K, bool colstats, bool rowsq, bool bias, TstatPlan* plan);
struct RsplitPlan { int waves, rch, ks, ksp, nt; };                               // ks: k steps of 16; ksp: padded to an even number
bool gemm_rsplit_plan(int b_layout, int M, int N, int K, bool colstats, bool rowsq, bool bn, int gather_window, RsplitPlan* plan);
bool gemm_rows_plan(int b_layout, int M, int N, int K, bool colstats, bool rowsq, bool bn, int* tpw, int* waves);
// (bn: a BnDxFused is passed, with or without `pre`; cbs: 16-column blocks, dealt to the eight waves ncb_min to ncb_max each)
struct SplitPlan { int cbs, ncb_min, ncb_max; };
bool gemm_split_plan(int b_layout, int M, int N, int K, bool colstats, bool rowsq, bool bias, bool bn, SplitPlan* plan);
int gemm_split_products();               // NVSM_GEMM_SPLIT: 6 (default), 9, or 0 = exact-fp32 MFMA kernels only
int gemm_rows_max_m();                   // largest M launch_gemm sends to the row-panel kernel (NVSM_GEMM_ROWS_MAX, default 8192; 0 = never): above it the split-bf16 kernel
float* gemm_dump_buffer();               // 256 B per device nobody reads (gemm_tstat.hip): the target of masked-out stores
void gemm_set_tstat_enabled(bool on);    // experiments / tests: force the tiled kernel
void launch_sum_parts(const float* parts, int nparts, int64_t stride, float* out, int64_t n, hipStream_t s);
void gemm_set_panel_enabled(bool on);    // experiments / tests: force the tiled kernel
int gemm_split_k_slabs(int K, int want);   // actual number of slabs launch_gemm will use for `want`
void launch_splitk_reduce(const float* partial, int slabs, size_t stride, float* out, int64_t n, hipStream_t s);

// ---- batch normalisation (F6, B5; replaces cuDNN per-activation BN, cpp/cudnn_utils.cu:82-183) --
// (the forward statistics μ, 1/sqrt(σ²+ε) are evaluated inside the loss kernel from the GEMM's column sums: LossArgs)
// dβ = Σdy, dγ = Σdy·x̂ (double sums [2][dim]) → floats, published together with grad_bias = dβ;
// dx = invσ·(dy − (dβ + x̂·dγ)/N), in place on dy
void launch_bn_dx(float* dy, const float* pre, const float* mean, const float* inv_std, const double* sums, float* dbeta,
                  float* dgamma, float* grad_bias, double n_global, int64_t rows, int dim, hipStream_t s);
void launch_colsum_finalize(const double* sums, int dim, float* out, hipStream_t s);   // no-BN grad_bias = Σdy

// codes a kernel stores into the engine's error word (page-locked host memory, read at the next synchronisation point)
enum { NVSM_BAD_WORD_ID = 1, NVSM_BAD_ENTITY_ID = 2, NVSM_SORT_TIMEOUT = 3, NVSM_BAD_WINDOW_REF = 4, NVSM_NONFINITE_BASE = 16 };
// ids outside [0, limit) become row 0 and raise `code` in *err_flag (err_flag may be null: tests of single kernels)
void launch_narrow_i64(const int64_t* src, int* dst, int64_t n, int64_t limit, int* err_flag, int code, hipStream_t s);
// stamp[list[i]] = value for i < *count (launch_stamp_rows' job, riding on the prologue: list == null: none)
struct StampJob { const int* list; const int* count; int* stamp; int value; };
void launch_step_prologue(const int64_t* words64, int* widx, int64_t nW, const int64_t* labels, int64_t B, int R,
                          int64_t num_words, int64_t num_entities, uint64_t seed, uint64_t step, int* ids, double* stats,
                          int nstats, int* err_flag, hipStream_t s, StampJob stamps = StampJob{nullptr, nullptr, nullptr, 0});
void launch_check_finite(const float* x, int64_t n, int* err_flag, int code, hipStream_t s);   // NVSM_DEBUG (CHECK_MATRIX)
void launch_scale(float* x, int64_t n, float a, hipStream_t s);      // x *= a (replica averaging)
// Host batch → HBM by a kernel that READS page-locked host memory over PCIe (up to four arrays in one launch) instead of
// hipMemcpyAsync: the runtime's copy call held the calling thread for most of a step (0.55-0.8 ms per step measured for the
// four arrays of a 51 200-window batch while the GPU was busy), so the host never got ahead of the GPU and every step began
// with the GPU waiting for its launches. src: device-visible addresses of page-locked memory; bytes: multiples of 4.
struct HostPull { void* dst[4]; const void* src[4]; size_t bytes[4]; int count; };
void launch_host_pull(const HostPull& p, hipStream_t s);
// data parallel, one collective per step (model.cpp dp_fold_): tail = [gb (de floats) | loss as hi, lo floats] behind the projection
// gradient, and back (gather_gemm.hip)
void launch_dp_pack_tail(const float* gb, const double* loss, float* tail, int de, hipStream_t s);
void launch_dp_unpack_tail(const float* tail, float* gb, double* loss, int de, hipStream_t s);
// Window references -> the four arrays of a device batch (corpus.hip; nvsm_step_windows). refs: [B] (document, first token inside
// the document) as interleaved uint32; tokens / doc_offsets / doc_weights / term_weights: the corpus in HBM (the weight arrays may
// be null: the matching output is then not written). A reference whose document is >= num_documents or whose window reaches beyond
// its document becomes word 0 / label 0 and stores NVSM_BAD_WINDOW_REF into *err_flag; nothing is read out of bounds (tokens holds at
// least one element, doc_offsets at least two, doc_weights at least one). words / wwts must be 16-byte aligned.
struct WindowExpandArgs {
    const uint32_t* refs; const int* tokens; const int64_t* doc_offsets; const float* doc_weights; const float* term_weights;
    int64_t num_documents, B; int w;
    int64_t* words; int64_t* labels; float* wwts; float* instw; int* err_flag;
};
void launch_window_expand(const WindowExpandArgs& a, hipStream_t s);
// *bad = 1 if a token is outside [0, num_words) (nvsm_corpus_upload); *bad must be 0 before
void launch_corpus_check_tokens(const int* tokens, int64_t n, int64_t num_words, int* bad, hipStream_t s);
void launch_delay(int microseconds, hipStream_t s);      // one wave spinning on the 100 MHz wall clock (profiling aid)
void launch_iota(int* dst, int64_t n, hipStream_t s);

// ---- fused loss forward + backward (F7–F16, B1–B4; replaces cpp/objective.cu:159-305,354-425 and the
// nonlinearity at cpp/params.cu:430-446,474-491) ------------------------------------------------
struct LossArgs {
    const float* pre;         // [B][de]  T·x (+b when !bn)
    const double* bn_sums;    // [2][de] (bn) Σx, Σx² over the batch, from the projection GEMM's epilogue
    double bn_n;              //      number of rows behind those sums (global batch with synchronised batch-norm)
    float bn_eps;
    float* bn_mean;           // [de] (bn) OUT: μ and 1/sqrt(σ²+ε), written by block 0 for the backward pass
    float* bn_inv_std;        // [de] (bn) OUT
    const float* bias;        // [de] (bn: β)
    const float* E;           // [nD][de]
    int64_t E_rows;           // nD (0: unknown) — which loop the gather runs depends on whether E fits the Infinity Cache
    LazyView lazyE;           // pending decay of E's rows, applied as they are gathered (stamp null: none)
    const int* ids;           // [B*R]
    const float* inst_w;      // [B] or null
    float* proj;              // [B][de]  act(BN(pre))
    float* dy;                // [B][de]  d/d(BN output) = gproj · act'
    float* coef;              // [B*R]   ±m_j  (signed multipliers)
    float* probs;             // [B*R]
    float* pp;                // [B]     mean_t(proj²)
    double* loss_acc;         // [1]     Σ ω·log p                           } written (not accumulated) by the ordered grid-wide sum;
    double* colstats;         // [2][de] Σdy, Σdy·x̂ (x̂ only when bn)      } colstats == loss_acc + 1
    GridSumWs sums;           // its workspace (kernels.h GridSumWs, one column group)
    int64_t B;
    int de, R, k;
    int bn, nonlinearity, rebalance;
    int l2_entity;            // l2_normalize_entity_reprs: gathered rows are divided by their norm (generic kernel only)
    float sig_eps, sig_hi, d_eps;
    double d_hi;              // 1 − d_eps compared in double (include/cuNVSM/cuda_utils.h:230)
    float inv_batch;          // exp(−log(B_global))
    float neg_scale;          // (k+1)/(2k)
    float clip_min, clip_max; // nextafter-widened hard_tanh bounds
    float inv_de;             // exp(−log(de))
};
// What LossArgs and PairArgs share: the sigmoid clamps of the forward and the backward half — float and double mixed as the
// reference mixes them — and 1 / d_e for the rows' mean of squares (updates_adam.cu:238-240)
template <typename Args>
inline void fill_clamps(Args& a, bool clip_sigmoid, int de) {
    a.sig_eps = clip_sigmoid ? 1e-7f : 0.f;
    a.sig_hi = static_cast<float>(1.0 - static_cast<double>(a.sig_eps));
    a.d_eps = clip_sigmoid ? 1e-6f : 0.f;
    a.d_hi = 1.0 - static_cast<double>(a.d_eps);
    a.inv_de = static_cast<float>(std::exp(-std::log(static_cast<double>(de))));
}
// Every constant of LossArgs that follows from the configuration, the number k of negatives and the global batch size (a.de is
// set): what Model::forward hands the loss kernel and what nvsm_debug_loss hands it — one statement of it, so the same bits.
inline void fill_loss_consts(LossArgs& a, bool clip_sigmoid, bool bias_negative_samples, int k, double B_global) {
    a.k = k;
    a.rebalance = (!bias_negative_samples && k > 1);                                      // objective.cu:268
    fill_clamps(a, clip_sigmoid, a.de);                                                     // :245-246, :367-368
    a.inv_batch = static_cast<float>(std::exp(-std::log(B_global)));                        // :354
    a.neg_scale = static_cast<float>((static_cast<double>(static_cast<float>(k)) + 1.0) /
                                     (2.0 * static_cast<double>(static_cast<float>(k))));   // :270-273
    a.clip_min = std::nextafter(-1.0f, -1.0f - 1e-5f);                                      // cuda_utils.h:91-96
    a.clip_max = std::nextafter(1.0f, 1.0f + 1e-5f);
}
// What launch_loss does with a LossArgs — every decision of the dispatch, host arithmetic only: the kernel family and its template
// numbers, the examples a wave walks, the grid and the dynamic LDS. launch_loss launches from this plan and from nothing else.
enum { LOSS_NONE = 0, LOSS_ROWS = 1, LOSS_GENERIC = 2 };
struct LossPlan {
    int family;              // LOSS_NONE (B <= 0: nothing is launched), LOSS_ROWS loss_rows_kernel<rb, lazy, pipe>, LOSS_GENERIC loss_kernel<v, niter, l2e>
    int rb, lazy, pipe;      // rows
    int v, niter, l2e;       // generic
    int epw;                 // examples per wave
    int grid;                // workgroups of four waves
    int shmem;               // bytes of dynamic LDS
};
void loss_plan(const LossArgs& a, LossPlan* plan);
void launch_loss(const LossArgs& a, hipStream_t s);
// true: the kernel launch_loss picks for these shapes applies LossArgs::lazyE itself; false: the rows must be current
bool loss_reads_lazily(int de, int R, bool l2_entity);
bool loss_two_row_sets(int64_t table_rows, int de);      // the row-gathering loss kernel keeps two sets of rows in flight per wave (tables beyond the Infinity Cache)

// ---- entity-entity similarity objective: forward + first half of the backward pass (pairs.hip; replaces
// RepresentationSimilarity::Objective, cpp/objective.cu:485-696) -------------------------------------------------------------
struct PairArgs {
    const float* E;           // [nD][de]
    int64_t E_rows;
    LazyView lazyE;           // pending decay of E's rows, applied as they are read (stamp null: none)
    const int* ids;           // [2M] interleaved a_p, b_p (narrowed: out-of-range ids are row 0)
    const float* w;           // [M] pair weights or null (= all 1.0)
    float* X;                 // [2M][de] OUT gradient source rows: row 2p = E[b_p], row 2p + 1 = E[a_p]
    float* coef;              // OUT coefficient of entry i at coef[i * coef_stride]: mult_p x scale for i = 2p, 2p + 1
    int coef_stride;
    float* sq;                // [2M]  OUT mean of squares of the entry's source row
    float* probs;             // [M]   OUT
    float* mults;             // [M]   OUT mult_p x scale
    double* loss_acc;         // [1]   Σ ω·log prob, written (not accumulated) by the ordered grid-wide sum
    GridSumWs sums;           // its workspace: one column group, pair_loss_blocks(M, de) contributions of one double
    int64_t M;
    int de;
    float sig_eps, sig_hi, d_eps;
    double d_hi;
    float inv_batch;          // exp(−log(M))
    float scale;              // mixture scale w_ee / (w_te + w_ee); 1 for the pair objective alone
    float inv_de;
    int mul_rows;             // the words-table form (pairs.hip): E is the words table, X gets the MULTIPLIED rows mults[p]·E[·], sq the
                              //   means of squares of those stored rows, coef is not written (the entries weigh 1)
};
int pair_loss_blocks(int64_t M, int de);      // workgroups launch_pair_loss uses (sizes GridSumWs::contrib_cap)
void launch_pair_loss(const PairArgs& a, hipStream_t s);
// the entry ids of the merged documents update: vals[i] = i for the n_text text entries, (first_src + j) * R for pair entry j —
// the id whose quotient by R is the entry's source row behind the text objective's (model.cpp compute_cost)
void launch_pair_entry_ids(int* vals, int64_t n_text, int64_t first_src, int R, int64_t n_pair, hipStream_t s);
void launch_pair_scale_weights(const float* w, float scale, float* out, int64_t n, hipStream_t s);      // out[i] = (w ? w[i] : 1) · scale
// the per-entry weights of the merged words update: out[i] = w[i] for the n_text text entries, out[(first_src + j) * R] = 1 for pair entry j
void launch_pair_entry_weights(const float* w, float* out, int64_t n_text, int64_t first_src, int R, int64_t n_pair, hipStream_t s);
void launch_pair_materialize(const float* coef, int coef_stride, const float* X, int64_t n, int de, float* out, hipStream_t s);   // tests

// per-row mean of squares: out[b] = Σ_t G[b][t]² · inv_dim  (cpp/updates_adam.cu:232-240)
void launch_row_meansq(const float* G, int64_t rows, int dim, float inv_dim, float* out, hipStream_t s);
// grad_entity[j][t] = coef[j] · proj[j/R][t]  (tests / gradient checker only)
void launch_materialize_grad_entity(const float* coef, const float* proj, int64_t N, int R, int de, float* out, hipStream_t s);
// ---- optional L2 row normaliser (cpp/cuda_utils.cu:12-130) ----
void launch_l2_rows_forward(const float* x, int64_t rows, int dim, float* y, float* norms, hipStream_t s);
void launch_l2_rows_backward(const float* g, const float* x, const float* norms, int64_t rows, int dim, float scale,
                             float* gin, float* msq, hipStream_t s);
void launch_materialize_grad_entity_l2(const float* coef, const float* proj, const float* E, const int* ids, int64_t N, int R,
                                       int de, float* out, float* msq, hipStream_t s);

// ---- batch → CSR by table row (replaces the atomic scatter of update_repr_kernel, cpp/storage.cu:37-49)
// Stable radix sort of (key, value) pairs by the low `bits` bits of the key (sort.hip). `temp` must be zero-filled ONCE when
// allocated; *epoch (host, starts at 0, one per workspace) is the value its arrival counter has reached. vals_in may be
// null (= 0, 1, 2, …). err_flag: the engine's error word (a grid-wide wait that never completes stores NVSM_SORT_TIMEOUT).
// zero_buf (optional, 16 B aligned, zero_count % 4 == 0): ints the first pass clears on the way (the CSR's per-step counters).
size_t sort_pairs_temp_bytes(int64_t n, int bits);
// gate (optional, device): the launches return at once when *gate == 0 — the outputs are then left as they were (the chunk
// order of a table none of whose rows has chunks this step).
void sort_pairs(void* temp, size_t temp_bytes, uint64_t* epoch, const int* keys_in, int* keys_out, const int* vals_in,
                int* vals_out, int64_t n, int bits, int* err_flag, hipStream_t s, int* zero_buf = nullptr, int64_t zero_count = 0,
                const int* gate = nullptr);
struct Csr {
    int* sorted_key;      // [n]
    int* sorted_entry;    // [n]  entry ids ordered by row (stable)
    int* row_begin;       // [rows]
    int* row_end;         // [rows]
    int* chunk_base;      // [rows]  first level-1 chunk of a long row
    int* chunk_desc;      // [max_chunks][3] row, begin, end
    int* chunk2_base;     // [rows]  first level-2 chunk of a very long row
    int* chunk2_desc;     // [max_chunks2][2] first, last (exclusive) level-1 chunk
    int* chunk_order;     // [max_chunks] level-1 chunks ordered by the position of their first entry in the batch (null: as numbered)
    int* num_chunks;      // [2]  level-1 / level-2 chunks in use
    int* num_touched;     // [1]  rows with at least one entry (num_chunks + 2)
    int* touched;         // [min(rows, max entries)] those rows, in no particular order (rows are independent)
    float* partial;       // [max_chunks][dim]
    float* partial_q;     // [max_chunks]
    float* partial2;      // [max_chunks2][dim]
    float* partial2_q;    // [max_chunks2]
    int* arrive_row;      // [rows]        arrival counters of table_pass_kernel, zero between launches
    int* arrive2;         // [max_chunks2]
    int64_t n;            // entries
    int64_t rows;
    int max_chunks, max_chunks2;
    int chunk;            // entries per level-1 chunk of a long row this step: kChunk, or kChunkSmall (Model::chunk_entries)
};
constexpr int kChunk = 64;    // entries per level-1 chunk of a long row
constexpr int kChunkSmall = 32;       // (48 / 20 / 16: LSE 0.1533 / 0.1506 / 0.1534 ms against 0.1503; 64: 0.1568)      // ... for the small batches of SGD / Adagrad handles (Model::chunk_entries)
constexpr int64_t kChunkSmallMaxEntries = 131072;
constexpr int kFan = 32;      // level-1 partials per level-2 chunk (64 until round 5: a row of 33-64 chunks then ended in one sum of up to 64 partials;
                              //   32 / 128: batch 51 200 and 6 400 the same / +0.4 %, +1.2 %, LSE batch 4 096 0.1473 -> 0.1456 ms / the same)
// Entries per level-1 chunk of a long row in a batch of n entries (Csr::chunk; why 32 for the small batches of SGD / Adagrad handles on
// narrow rows: Model::chunk_entries) and the chunk slots of a workspace for up to max_entries entries. A long row of L > chunk entries
// has ceil(L / chunk) <= 2 L / (chunk + 1) chunks — equality at L = chunk + 1 —, so a batch has fewer than 2 n / chunk of them; the
// level-2 chunks, two at most per kFan · chunk + 1 entries, likewise. Shared by Model::alloc_table_csr and the table-pass test hook
// (test_hooks.cpp), which must size its workspace as the product does: tests/test_gpu_table_pass.py builds the batch of chunk + 1 rows.
inline int csr_chunk_entries(bool adam, int dim, int64_t n) {
    return (!adam && n <= kChunkSmallMaxEntries && dim <= 128) ? kChunkSmall : kChunk;
}
inline void csr_chunk_caps(bool adam, int dim, int64_t max_entries, int* max_chunks, int* max_chunks2) {
    int64_t c1 = 2 * max_entries / kChunk;
    if (!adam && dim <= 128) c1 = std::max<int64_t>(c1, 2 * std::min<int64_t>(max_entries, kChunkSmallMaxEntries) / kChunkSmall);
    *max_chunks = static_cast<int>(c1 + 2);
    *max_chunks2 = static_cast<int>(c1 / kFan + 2);
}

// bounds + long-row chunk list, from sorted_key; counters_cleared: row_begin | row_end | num_chunks | num_touched (one
// allocation of csr_counter_ints(rows) ints) are already zero (sort_pairs cleared them), otherwise a memset does it
// order_key (optional, [max_chunks], with Csr::chunk_order): the chunk fill also writes the keys of launch_chunk_order (keys_written)
void launch_csr_build(const Csr& c, hipStream_t s, bool counters_cleared = false, int* order_key = nullptr);
// Csr::chunk_order: the level-1 chunks by where in the batch their entries start (512 buckets; update.hip table_pass_kernel
// gives each XCD one eighth of the batch so that the chunks of different hot rows over the same windows share an L2).
// key_in / key_out: [max_chunks] scratch; sort_temp: a sort_pairs workspace for max_chunks pairs
void launch_chunk_order(const Csr& c, int* key_in, int* key_out, void* sort_temp, size_t sort_temp_bytes, hipStream_t s, bool keys_written = false);
inline int64_t csr_counter_ints(int64_t rows) { return (2 * rows + 3 + 63) / 64 * 64; }
bool row_pass_split(const Csr& c);                    // rows · ratio >= entries: touched-row list + streaming pass over the rest
double table_split_ratio();                           // that ratio (2 unless NVSM_SPLIT_RATIO says otherwise)

// ---- row passes: gather Σ coef·X[src] per table row, then the optimiser's row-local formula --------
enum RowKind {
    ROW_SGD = 0,               // P = P·decay + lr·g                         (cpp/storage.cu:51-102)
    ROW_ADAGRAD_ENT = 1,       // a += q; P = P·decay + lr·g/sqrt(a+ε)       (cpp/updates_adagrad.cu:99-179, window 1)
    ROW_ADAM_MV = 2,           // m = β1 m + (1−β1) g; v = β2 v + (1−β2) q   (cpp/updates_adam.cu:196-252)
    ROW_ADAM_SPARSE_ENT = 3,   // ROW_ADAM_MV then P = P·decay + lr·cnt·bc·m/(√v+ε)   (:332-384, window 1)
    ROW_ADAM_DENSE = 4,        // ROW_ADAM_MV then P = P·decay + lr·bc·m/(√v+ε)       (:293-311)
    ROW_ADAM_FULL = 5,         // m,v with L2 folded in, v per element; P += lr·bc·m/(√v+ε)  (:203-213,253-282,312-328)
    ROW_SCALAR_ACC = 6         // a += q only (Adagrad, window > 1)           (cpp/updates_adagrad.cu:136-158)
};
struct RowPassArgs {
    int table;                 // 0 = words (entry e: src = e / div, coef = wts[e]), 1 = entities (src = j / div, coef = coefs[j])
    int kind;
    const float* X;            // [num_src][dim]   gradient source rows
    const float* wts;          // words: per-entry weights or null
    const float* coefs;        // entities: signed multipliers
    const float* sq_src;       // words: msq[src]; entities: pp[src]
    const float* src_scale;    // optional per-src scale (Adagrad, window > 1)
    uint32_t div;              // window (words) or R (entities)
    uint64_t div_magic;        // floor(2^37 / div) + 1: src = (entry * div_magic) >> 37, exact for entry < 2^26, div <= 2048
    float* P; float* m; float* v;   // table, first moment [rows][dim], per-element second moment (ROW_ADAM_FULL only)
    const float* sc_in;        // per-row scalar state in  (Adam v / Adagrad a, [rows]); ping-pong with sc_out because
    float* sc_out;             //   every lane of a row's thread group reads the old value
    int dim;
    float lr, decay, lambda;
    float one_m_b1, s_m, one_m_b2, s_v, bc, eps, c_reg;
    int dense;                 // visit rows without entries (decay / dense Adam)
    int max_blocks;            // 0 = one thread group per row; > 0 = cap the grid (rows are grid-strided) so that a kernel
                               //   running concurrently on another stream finds free registers on every CU
    int touched_only;          // set by launch_row_pass: visit the rows of Csr::touched only (see row_pass_split)
    int nt_p;                  // the table rows themselves likewise (experiments)
    int nt_m;                  // first moments with streaming (nt) loads / stores: nobody gathers them (documents table)
    int shallow;               // set by launch_row_pass: two entries in flight per lane instead of eight (rows >= entries)
    int lazy;                  // lazy dense decay (below): rows without entries are NOT visited, their decay stays pending
    int rows_elsewhere;        // set by launch_table_pass: the rows of at most a chunk's entries are done by entry_walk_kernel
    int wide;                  // this ROW_SGD pass belongs to an Adam update (update.hip: the WIDE family of the one-launch pass)
    int untouched_done;        // the streaming pass over the rows WITHOUT entries of a split dense pass has been queued already (launch_untouched_rows)
    LazyView pending;          // lazy: the row's P (and m, by s_m) first get the factors of the updates (stamp[row], now] the
                               //   row sat out, one by one (pending.stamp null: the rows are current)
};
// ---- lazy dense decay, for tables much larger than the batch ------------------------------------------------------------
// The reference rewrites EVERY row of a table on every update (θ·(1 − λ·lr), Adam m·β₁, v·β₂: cpp/storage.cu:65-67,
// cpp/updates_adam.cu:196-252): at |D| = 2 M that is 8 of the 10 GB a step moves. A row without entries only ever gets
// multiplied by those per-update constants, so the multiplications can wait until somebody looks at the row: every row
// carries the number of updates applied to it (stamp), and whoever reads a row applies the factors of the updates it sat
// out ONE BY ONE, in fp32, in update order (the factors of the last kLazyHistory updates travel in the kernel arguments:
// LazyView) — exactly the sequence of roundings the dense passes would have produced, so parameters and optimiser state
// stay bit-identical to the eager path (tests/test_gpu_lazy.py compares them):
//   * the gathers of the forward pass (word gather-mean, loss kernel) do it in registers and write nothing back;
//   * the row passes of the update do it to the rows of the batch before the optimiser's formula and store the result;
//     the per-row scalar (Adam v / Adagrad accumulator) of those rows is brought up to date into a snapshot buffer by a
//     small launch in front of the passes (launch_lazy_refresh, scalars_only), and the rows' stamps are set by a small
//     launch behind the last pass (launch_stamp_rows) — not inside it, where another wave of the row's thread group could
//     still be about to read the old stamp;
//   * every kLazyHistory updates, and before anything else looks at a whole table (get_param, set_param, replica
//     averaging), launch_lazy_refresh brings all rows up to date.
struct LazyRefreshArgs {
    float* P; float* m;                 // table rows, first moments (null: none)
    float* sc;                          // per-row scalar state (Adam v / Adagrad accumulator; null: none)
    float* sc_snapshot;                 // copy of the refreshed scalar the row pass reads while it writes `sc` (null: none)
    int scalars_only;                   // P, m and the stamps are left alone (the row pass refreshes them itself): only the
                                        //   scalar is brought up to date and snapshotted, one thread per row
    int* stamp;                         // [rows] updates applied to the row
    const int* list; const int* list_count;      // rows to refresh (Csr::touched); null = all `rows`
    int64_t rows; int dim;
    int now;                            // updates applied to the table so far
    float s_m, s_v;                     // per-update factors of m and of the scalar (1 = none)
    float decay[kLazyHistory];          // factor of update u on P at [(u - 1) % kLazyHistory]
};
// stamp[row] = value for the rows of c.touched (after the last pass of a lazy table's update)
void launch_stamp_rows(const Csr& c, int* stamp, int value, int64_t max_rows, hipStream_t s);
void launch_lazy_refresh(const LazyRefreshArgs& a, int64_t max_rows, hipStream_t s);

void launch_chunk_pass(const Csr& c, const RowPassArgs& a, hipStream_t s);
// untouched_s: the stream the streaming pass over the rows WITHOUT entries of a split dense pass is queued on (null: `s`).
// Those rows and the rows with entries are disjoint, so the two launches need no order between them — only the CSR bounds
// in front of both and the table's next reader behind both.
void launch_row_pass(const Csr& c, const RowPassArgs& a, hipStream_t s, hipStream_t untouched_s = nullptr);
// The streaming half of a split dense pass on its own: the rows WITHOUT entries of a table much larger than the batch get the
// row formula with g = 0 (the decay). It needs the CSR's row bounds and nothing else of the step, so the fused step queues it
// right behind the CSR build, under the forward pass, instead of in the update's tail; the pass proper is then launched with
// RowPassArgs::untouched_done. true: launched (the pass is split, dense, not lazy, its kind row-local for untouched rows).
bool launch_untouched_rows(const Csr& c, const RowPassArgs& a, hipStream_t s);
// both, in one launch (update.hip). Returns how the rows with entries were walked (tests assert which path a shape took).
enum TablePassPath { TABLE_PASS_DENSE = 0, TABLE_PASS_LIST_WALK = 1, TABLE_PASS_ENTRY_WALK = 2 };
int launch_table_pass(const Csr& c, const RowPassArgs& a, hipStream_t s, hipStream_t untouched_s = nullptr);
void set_table_pass_one_launch(bool on);      // tests / A-B runs: false = the three-launch form (also NVSM_MERGED_PASS=0)
bool table_pass_one_launch();                 // what set_table_pass_one_launch last said (the table-pass test hook puts it back)
// the constants of an Adam row pass (β₁ = 0.9, β₂ = 0.999, ε = 1e-6) for bias correction bc and scaled λ sl (model.cpp)
void fill_adam_consts(RowPassArgs& a, float bc, float sl);

// ---- fold-in (fold.hip; include/cunvsm_amd.h nvsm_step_fold): the documents update on the rows [first, rows) only ----
// Reads row_begin / row_end / sorted_key / sorted_entry of the documents CSR and its own partial buffers; the row formula and its
// constants are RowPassArgs' (kind: ROW_SGD, ROW_ADAGRAD_ENT, ROW_ADAM_SPARSE_ENT, ROW_ADAM_DENSE, ROW_ADAM_FULL). The per-row scalar
// state is updated in place (a wave owns its row). Rows below `first` are neither read nor written.
constexpr int kFoldChunk = 64;      // entries per chunk of a row's sum (a row of more entries is cut over several waves)
constexpr int kFoldGroup = 32;      // chunk sums per second-stage group (rows of more chunks get group sums first)
struct FoldArgs {
    const int* sorted_key; const int* sorted_entry; const int* row_begin; const int* row_end;
    int64_t n, rows, first;             // entries of the batch, rows of the table, first row that trains
    const float* X; const float* coefs; const float* sq_src;      // proj [B][dim], coef [n], pp [B] (null: the kind has no q)
    uint64_t div_magic;                 // as RowPassArgs: src = (entry * div_magic) >> 37
    float* P; float* m; float* v; float* sc;
    int dim, kind, dense;
    float lr, decay, lambda, one_m_b1, s_m, one_m_b2, s_v, bc, eps, c_reg;
    float* partial; float* partial_q;   // [chunk_rows][dim], [chunk_rows]    } fold_partial_rows(max entries)
    float* partial2; float* partial2_q; // [group_rows][dim], [group_rows]    }
};
void fold_partial_rows(int64_t max_entries, size_t* chunk_rows, size_t* group_rows);
void launch_fold_update(const FoldArgs& f, hipStream_t s);

// words, window > 1 (cpp/updates_adagrad.cu:83-97, cpp/updates_adam.cu:132-151)
void launch_adagrad_scale(const float* acc, const int* idx, int window, int64_t B, float eps, float* scale, hipStream_t s);
void launch_adam_u(const float* m, const float* v, int dim, const int* idx, int window, int64_t B, float bc, float eps,
                   float* U, hipStream_t s);

// ---- dense projection optimiser (U4; cpp/updates.cu:24-34, updates_adagrad.cu:33-70, updates_adam.cu:46-105)
struct TransformUpdateArgs {
    PlaneTarget pt[2];
    int de;                          // entity dimension: T is stored [dw][de]
    // the split-K slabs of the dT product, added up here instead of by launch_splitk_reduce in front of the update (null: gT holds
    // the gradient): the same sums in the same order — 16 interleaved groups of slabs, then the groups in order — one launch less
    const float* partial; int slabs; size_t slab_stride;
    float* T; float* b;              // parameters (nT = de*dw, nb = de)
    float* gT; float* gb;            // gradients (overwritten with the applied direction, as the reference does)
    float* s0T; float* s0b; float* s1T; float* s1b;
    int nT, nb, method;
    float lr, lambda, eps, one_m_b1, s_m, one_m_b2, s_v, bc;
};
void launch_transform_update(const TransformUpdateArgs& a, hipStream_t s);
// the scalars of the launch (method, lr, lambda, eps, the Adam factors and the bias correction at step count t) as
// Model::update_transform hands them over; model.cpp
float adam_bias_correction(uint64_t t);
void fill_transform_consts(TransformUpdateArgs& a, int method, float lr, float sl, uint64_t t);

// ---- ranking: query inference and top-k documents (rank.hip; Model::infer, cpp/model.cu:105-133; py/nvsm/base.py:297-430) ----
// query side: ragged weighted gather-mean (ids / wts / offsets on the device; `lazy` as launch_gather_mean), then f(pre + c·b) in place
void launch_rank_query_mean(const float* W, int dw, int64_t num_words, const int64_t* ids, const float* wts, const int64_t* offsets,
                            int64_t Q, float* out, const LazyView& lazy, int* err_flag, hipStream_t s);
void launch_rank_bias_act(float* y, const float* bias, float c, int act, int64_t Q, int de, hipStream_t s);      // act: NVSM_TANH, NVSM_HARD_TANH, else identity
void launch_rank_query_norm(const float* P, int64_t Q, int de, float* inv, int cosine, hipStream_t s);            // 1 / |P[q]|, 0 for a zero row; cosine 0: ones
// scan: scores[q][i] = similarity of query q < Q and document d_begin + i, i < S (cosine: the row norms out of the same pass)
bool rank_scan_uses_mfma(int de);
void launch_rank_scan(const float* E, int de, int64_t d_begin, int S, const float* P, int Q, const float* qinv, float* scores,
                      int64_t ld_scores, int cosine, const LazyView& lazy, hipStream_t s);
// candidate lists (distinct, ascending ids, concatenated; cand_off [Q + 1]): keys[q][j < npad] = sortable (score, id), 0 past the list
void launch_rank_scan_candidates(const float* E, int de, const float* P, const float* qinv, const int* cand, const int64_t* cand_off,
                                 int Q, int64_t npad, unsigned long long* keys, int cosine, const LazyView& lazy, hipStream_t s);
// selection: the min(k, S) best documents of the slab per query as keys[q][key_off ...], in no particular order. ws:
// rank_select_ws_bytes(Q, S) bytes. true: by radix select (k < S); false: every document of the slab (k >= S).
size_t rank_select_ws_bytes(int Q, int S);
bool launch_rank_select(const float* scores, int64_t ld_scores, int S, int64_t d_begin, int Q, int k, void* ws,
                        unsigned long long* keys, int64_t ld_keys, int64_t key_off, hipStream_t s);
void launch_rank_fill_keys(unsigned long long* keys, int64_t ld_keys, int64_t from, int64_t to, int Q, hipStream_t s);   // keys[q][from, to) = 0
// keys[q][0 .. npad) (npad a power of two) descending = score descending, id ascending. true: npad needed the global-memory steps.
bool launch_rank_sort(unsigned long long* keys, int64_t npad, int Q, hipStream_t s);
// ids / scores [Q][k], counts [Q] from the sorted keys; a query has cand_off[q + 1] - cand_off[q] keys (cand_off null: n_all)
void launch_rank_write(const unsigned long long* keys, int64_t npad, int Q, int k, const int64_t* cand_off, int64_t n_all,
                       int64_t* ids, float* scores, int64_t* counts, hipStream_t s);


// ---- nearest neighbours in word, projected-word and document space (rank.hip; py/nvsm/base.py:106-162, 325-353, 362-430) ----
// the scan of nvsm_neighbors: scores as launch_rank_scan; the MFMA kernel wherever dim % 4 == 0 && dim >= 32 (a zero-filled tail
// chunk where dim % 32 != 0), else the plain kernel. set_nbr_scan_force_plain: the plain kernel for every dimension (test hook:
// how tools/bench_neighbors.py holds the two against each other).
bool nbr_scan_uses_mfma(int dim);
void set_nbr_scan_force_plain(bool on);
void launch_nbr_scan(const float* E, int dim, int64_t d_begin, int S, const float* P, int Q, const float* qinv, float* scores,
                     int64_t ld_scores, int cosine, const LazyView& lazy, hipStream_t s);
// out[q][dim] = row ids[q] (ids null: first + q) of `table` at its logical values
void launch_rank_gather_rows(const float* table, int dim, const int64_t* ids, int64_t first, int64_t Q, float* out, const LazyView& lazy, hipStream_t s);
// scores[q][self[q] - d_begin] = -inf where that lies in the slab (self[q] < 0: nothing)
void launch_rank_exclude_self(float* scores, int64_t ld_scores, int64_t d_begin, int S, const int64_t* self, int Q, hipStream_t s);
// out[i] = cosine similarity or dot product of rows a[i] and b[i] (device ids) of one table; one wave per pair
void launch_rank_pair_sim(const float* table, int dim, const int64_t* a, const int64_t* b, int64_t n, float* out, int cosine,
                          const LazyView& lazy, hipStream_t s);

// ---- n-grams of terms in document space (ngram.hip; include/cunvsm_amd.h nvsm_ngram_search; py/nvsm/base.py:106-162) ----
// rows of the stack of phrase projections over m words: m for max_cardinality 1, m + m(m − 1)/2 for 2; -1 where that is not below
// 2^31 (the selection keys' limit), for m < 1 and for any other cardinality. Host arithmetic only.
int64_t ngram_row_count(int64_t m, int max_cardinality);
// out[i][de], i < S = phrase row p0 + i: f(G[a] + c·b) for the 1-gram a = p0 + i < m, f(0.5·(G[a] + G[b]) + c·b) for the 2-gram
// (a, b) of row m + a·(2m − a − 1)/2 + (b − a − 1); G [m][de] = T·W[s_i] on the device, f and c as launch_rank_bias_act (the same
// __device__ expression). The slab may straddle the 1-gram / 2-gram boundary and begin inside a run of one a; rows outside the
// stack throw before anything is launched.
void launch_ngram_rows(const float* G, int m, int de, const float* bias, float c, int act, int64_t p0, int S, float* out, hipStream_t s);

// ---- exact t-SNE of table rows (tsne.hip; include/cunvsm_amd.h nvsm_tsne; py/visualize.py) ----
// The n × n buffer P (squared distances, then conditional probabilities, then joint probabilities) has rows of tsne_ld(n) floats,
// n rounded up to 4; every pointer below is a device pointer, and every sum has a fixed order (no atomics).
int64_t tsne_ld(int64_t n);
// the column slabs of tsne_forces_kernel at n rows: width wc (a multiple of 256, at most 4096) and their number; host arithmetic
void tsne_force_layout(int n, int* wc, int* slabs);
void launch_tsne_normalize(float* X, int n, int d, hipStream_t s);      // rows of X [n][d] divided by their norms, zero rows kept
// X [n][d] -> P: distances (fp64 sums rounded to fp32), then sklearn's perplexity search per row (fp64): the conditional
// probabilities, zero diagonal; rowsum [n] = their row sums (fp64)
void launch_tsne_conditionals(const float* X, int n, int d, float perplexity, float* P, double* rowsum, hipStream_t s);
// P in place: max((C + Cᵀ) / max(2ΣC, eps), eps) with a zero diagonal; total [1]: fp64 scratch
void launch_tsne_joint(float* P, int n, const double* rowsum, double* total, hipStream_t s);
// part [n][slabs][5] = (Σ P q dx, Σ P q dy, Σ q² dx, Σ q² dy, Σ q) per row and column slab, q = 1 / (1 + |y_i − y_j|²); z [1] = Σ q
void launch_tsne_forces(const float* P, const float* Y, int n, float* part, double* z, hipStream_t s);
// g = 4·(exaggeration·attractive − repulsive / Z) and sklearn's _gradient_descent step on Y, upd, gains [n][2]; gs [n][2] = the
// gain-scaled gradient, graw [n][2] (may be null) = g
void launch_tsne_update(const float* part, int n, const double* z, float exaggeration, float momentum, float learning_rate, float* Y,
                        float* upd, float* gains, float* gs, float* graw, hipStream_t s);
// klrow [n] = the rows of KL(e·P ‖ Q) at Y, fp64 throughout, with a Z of their own in z64 [1] (scratch); out [2] = (Σ klrow, |gs|)
void launch_tsne_kl_rows(const float* P, const float* Y, int n, double* z64, float exaggeration, double* klrow, hipStream_t s);
void launch_tsne_check(const double* klrow, const float* gs, int n, double* out, hipStream_t s);
// PCA start: mean [d], cov [d][d] = XcᵀXc (fp64); Y0 [n][2] = fp32(Xc·Vᵀ) for V [2][d] (fp64)
void launch_tsne_covariance(const float* X, int n, int d, double* mean, double* cov, hipStream_t s);
void launch_tsne_project(const float* X, int n, int d, const double* mean, const double* V, float* Y0, hipStream_t s);

// ---- sparse-affinity t-SNE (tsne_sparse.hip; include/cunvsm_amd.h nvsm_tsne_sparse) ----
// sklearn's method='barnes_hut' at angle 0: k neighbours a row, P a CSR matrix (indptr [n + 1] int64, indices / data [nnz]), the
// repulsion over all pairs from Y alone. Every pointer is a device pointer and every sum has a fixed order (no float atomics).
// the column ranges of tsne_sp_repulsion_kernel at n rows: width wr, LDS tile tw (a multiple of 256, at most 4096) and their number, a
// function of n alone; forced_ranges > 0 (the test hooks) asks for that many ranges. Host arithmetic.
void tsne_sparse_layout(int n, int forced_ranges, int* wr, int* tw, int* ranges);
// scores [qn][ld]: row q0 + i against rows j0 .. j0 + S: −fp32(fp64 Σ_t (x_it − x_jt)²), never −0; −inf at the row itself
void launch_tsne_nn_scores(const float* X, int n, int d, int q0, int qn, int j0, int S, float* scores, int64_t ld, hipStream_t s);
// the round's sorted selection keys -> nbr_id / nbr_d2 [n][k] rows q0 .. q0 + qn, nearest first, ties by ascending id
void launch_tsne_nn_write(const unsigned long long* keys, int64_t npad, int qn, int k, int q0, int* nbr_id, float* nbr_d2, hipStream_t s);
// sklearn's perplexity search over each row's k distances (fp64): cond [n][k] (fp32), rowsum [n] their sums (fp64)
void launch_tsne_nn_conditionals(const float* nbr_d2, int n, int k, float perplexity, float* cond, double* rowsum, hipStream_t s);
// out [2nk]: the row (row = true) or column of directed entry perm[t] (perm null: t); entry e < nk is edge e as (i, j), e >= nk as (j, i)
void launch_tsne_sym_keys(const int* nbr_id, int n, int k, const int* perm, bool row, int* out, hipStream_t s);
// data[p] = fp32(Σ cond of the entries head_pos[p] .. head_pos[p + 1] of perm / max(2·total, eps)); total [1] = Σ rowsum
void launch_tsne_sym_values(const int* head_pos, const int* perm, const float* cond, int64_t nnz, int n, int k, const double* total, float* data,
                            hipStream_t s);
// attr [n][2] = Σ_{stored j} P q (y_i − y_j); part [n][ranges][3] = (Σ q² dx, Σ q² dy, Σ q) over the range's j != i; z [1] = Σ q
void launch_tsne_sparse_forces(const int64_t* indptr, const int* indices, const float* data, const float* Y, int n, int forced_ranges, float* attr,
                               float* part, double* z, hipStream_t s);
// launch_tsne_update on attr and part
void launch_tsne_sparse_update(const float* attr, const float* part, int n, int forced_ranges, const double* z, float exaggeration, float momentum,
                               float learning_rate, float* Y, float* upd, float* gains, float* gs, float* graw, hipStream_t s);
// klrow [n] = Σ_{stored j} e·P·log(max(e·P, tiny) / max(q / Z, tiny)), fp64 throughout, with a Z of their own in z64 [1] (scratch: one
// more pass over all pairs, in fp64); launch_tsne_check adds them up
void launch_tsne_sparse_kl_rows(const int64_t* indptr, const int* indices, const float* data, const float* Y, int n, double* z64,
                                float exaggeration, double* klrow, hipStream_t s);

// ---- k-means of table rows (kmeans.hip; include/cunvsm_amd.h nvsm_kmeans) ----
// Every pointer below is a device pointer; every floating-point sum has a fixed order (no float atomics).
// The assignment pass runs on v_mfma_f32_16x16x4_f32 at every dimension (columns beyond d are zeros in LDS): always true today,
// kept as a predicate so that a caller names the route it got, as nbr_scan_uses_mfma does.
bool kmeans_assign_uses_mfma(int d);
int kmeans_stat_slabs(int n);                  // row slabs of launch_kmeans_colstats (part: [slabs][d] doubles)
int64_t kmeans_max_chunks(int64_t n, int k);   // an upper bound of the chunks of launch_kmeans_update (part: [chunks][d] doubles)
int64_t kmeans_prefix_chunks(int64_t n);       // chunks of launch_kmeans_kpp_pick (part: [chunks] doubles)
// mean64 / var [d]: fp64 column mean and population variance of X [n][d]; mean32 its fp32 rounding; *var_mean = mean of var
void launch_kmeans_colstats(const float* X, int n, int d, double* part, double* mean64, float* mean32, double* var, double* var_mean, hipStream_t s);
// cc [rows][d] (may be null) = fp32(x − mean); norm [rows] = the squared norms of those (fp64 sums rounded to fp32)
void launch_kmeans_center_rows(const float* X, int64_t rows, int d, const float* mean, float* cc, float* norm, hipStream_t s);
// label [n] = argmin_j |x_i − c_j|² by the centred expansion (Cc, cn: launch_kmeans_center_rows of the centres; xn: of the rows), the
// lowest j on a tie; dist [n] = that minimum, clamped at 0
void launch_kmeans_assign(const float* X, int n, int d, const float* mean, const float* Cc, const float* cn, const float* xn, int k,
                          int* label, float* dist, hipStream_t s);
// out64 [n] = direct fp64 |x_i − c|², c = C[label[i]] or (label null) the row X[fixed]; min_into: the minimum with what out64 holds;
// out32 (may be null) its fp32 rounding
void launch_kmeans_rowdist(const float* X, int n, int d, const float* C, const int* label, int64_t fixed, bool min_into, double* out64,
                           float* out32, hipStream_t s);
void launch_kmeans_sum(const double* v, int64_t n, double* out, hipStream_t s);      // *out = Σ v, one workgroup, fixed order
void launch_kmeans_iota(int* v, int n, hipStream_t s);
// from the labels sorted ascending: start [k + 1] segment bounds, choff [k + 1] chunk offsets, counts [k], *n_empty
void launch_kmeans_segments(const int* sorted_label, int n, int k, int* start, int* choff, int64_t* counts, int* n_empty, hipStream_t s);
// Cnew [k][d] = fp32 of the fp64 mean of each segment's rows (pos: row positions in sorted order), Cold's row where a segment is
// empty; shift [k] and *shift_total = Σ (Cnew − Cold)² (fp64)
void launch_kmeans_update(const float* X, int n, int d, const int* pos, const int* start, const int* choff, int k, double* part,
                          const float* Cold, float* Cnew, double* shift, double* shift_total, hipStream_t s);
void launch_kmeans_changed(const int* a, const int* b, int n, int* changed, hipStream_t s);      // *changed += 1 per workgroup with a moved label
// out[0] = Σ dmin (two-level sequential prefix); out[1] = the lowest position whose inclusive prefix exceeds u · total, −1 if none
void launch_kmeans_kpp_pick(const double* dmin, int n, double* part, double u, double* out, hipStream_t s);

// ---- retrieval metrics of a round's ranking (eval.hip; include/cunvsm_amd.h nvsm_evaluate) ----
// One wave per query of the round. ids [Q][k] / counts [Q]: what launch_rank_write left. Judged documents of ALL queries of the
// call: jids ascending per query (no -1 entries), jgrades next to them, joff [queries of the call + 1]; consts
// [query][2 + kEvalMaxCutoffs] = R, idcg, idcg@cutoff; metrics [query][NVSM_EVAL_FIXED + 3 num_cutoffs]. q0: the round's first query.
constexpr int kEvalMaxCutoffs = 8;
struct EvalArgs {
    const int64_t* ids; const int64_t* counts; int k;
    const int* jids; const int* jgrades; const int64_t* joff; const double* consts;
    int cutoffs[kEvalMaxCutoffs]; int num_cutoffs;
    double* metrics; int64_t q0;
};
void launch_eval_metrics(const EvalArgs& a, int Q, hipStream_t s);

// ---- query-likelihood ranking over the resident corpus, and run fusion (lexical.hip; include/cunvsm_amd.h nvsm_lexical_rank /
// nvsm_rank_ensemble) ----
constexpr int kLexSlots = 1024;            // distinct query terms of a round: 4 KiB of LDS counters per workgroup
constexpr int kFuseMaxTopK = 1024;         // fuse_lists_kernel: 2 k entries x 20 B of LDS (NVSM_ENSEMBLE_MAX_TOP_K)
void launch_lex_cf(const int* tokens, int64_t n, unsigned long long* cf, hipStream_t s);      // cf[t] += occurrences; cf zeroed by the caller
void launch_lex_fill_int(int* p, int64_t n, int v, hipStream_t s);
// slot_of[terms[i]] = i (set) or -1 (clear), i < n; the terms are distinct
void launch_lex_set_slots(int* slot_of, const int* terms, int n, bool set, hipStream_t s);
// scores[q][d - d0] for q < Q, d in [d0, d0 + S): Σ over the query's terms j in [qoff[q], qoff[q + 1]) — in that order, fp64, narrowed
// once — of log((1 − param)·tf/len + c0[j]) (NVSM_LEX_JM) or log((tf + c0[j]) / (len + param)) (NVSM_LEX_DIRICHLET); -inf when no
// term of q occurs in d. tslot[j]: the term's slot < num_slots <= kLexSlots; base[j] = log(c0[j]).
// weight null: the sum as it stands (nvsm_lexical_rank's bits). weight given (nvsm_lexical_rank_weighted): Σ_j weight[j]·log(...),
// each product rounded on its own, in the same order.
struct LexScoreArgs {
    const int* tokens; const int64_t* doc_offsets; const int* slot_of;
    int64_t d0; int S; int Q; int num_slots; int method; double param;
    const int* qoff; const int* tslot; const double* c0; const double* base;
    float* scores; int64_t ld;
    const double* weight;
};
void launch_lex_score(const LexScoreArgs& a, hipStream_t s);
// relevance model of a round's queries (nvsm_relevance_model). Query q < Q has the feedback documents
// fb_ids[q][0 .. fb_counts[q]) in rank order with the first pass's scores fb_scores[q][...] (rows fb_docs long, fb_docs <= kFeedbackMaxDocs).
// acc [Q][V] doubles and cnt [Q][V] ints are zero before and cnt is zero behind; acc[q][t] = Σ_i ω_i·tf(t, d_i)/len(d_i) added in rank
// order, sum_w[q] = Σ_i ω_i in rank order, ω_i = exp(s_i − s_0). Integer atomics only.
constexpr int kFeedbackMaxDocs = 1024;     // the ω of a query: 8 KiB of LDS (NVSM_FEEDBACK_MAX_DOCS)
struct LexRmArgs {
    const int* tokens; const int64_t* doc_offsets;
    const int* fb_ids; const float* fb_scores; const int* fb_counts; int fb_docs;
    int64_t V; double* acc; int* cnt; double* sum_w;
};
void launch_lex_rm_accumulate(const LexRmArgs& a, int Q, hipStream_t s);
// scores[q][t − t0] = float(acc[q][t] / sum_w[q]) where acc[q][t] > 0 and the narrowed value is > 0, else -inf, for t in [t0, t0 + S);
// acc is zeroed behind
void launch_lex_rm_narrow(double* acc, const double* sum_w, int64_t V, int64_t t0, int S, int Q, float* scores, int64_t ld, hipStream_t s);
// launch_rank_write for keys that may carry -inf scores: ids / scores [Q][k] up to the first -inf or padding key, counts [Q] likewise
void launch_lex_write(const unsigned long long* keys, int64_t npad, int Q, int k, int64_t n_all, int64_t* ids, float* scores,
                      int64_t* counts, hipStream_t s);
// ---- TF-IDF first stage and re-ranking of its candidates (lexical.hip; include/cunvsm_amd.h nvsm_tfidf_rank / nvsm_rerank)
// df[t] += documents d < num_documents with tf(t, d) >= 1, exactly: the documents in slabs of `slab` (1 .. 2^31 − 1), bits
// [num_words][lex_df_row_words(slab)] words, zero before (behind a slab that is not the last they are zero again; behind the last they
// are not). df zeroed by the caller. Integer atomics only.
int64_t lex_df_row_words(int64_t slab);
void launch_lex_df(const int* tokens, const int64_t* doc_offsets, int64_t num_documents, int64_t slab, unsigned* bits,
                   unsigned long long* df, hipStream_t s);
// scores[q][d - d0] as launch_lex_score lays them out: Σ over the query's terms j with tf > 0 — in query order, fp64, every operation
// rounded on its own, narrowed once — of (idf[j]·(tf·(k1 + 1))) / (tf + k1·((1 − b) + b·(len / avgdl))), times weight[j] where weight
// is given; -inf when no term of q occurs in d. idf[j]: evaluated by the host, once per term.
struct TfidfScoreArgs {
    const int* tokens; const int64_t* doc_offsets; const int* slot_of;
    int64_t d0; int S; int Q; int num_slots; double k1, b, avgdl;
    const int* qoff; const int* tslot; const double* idf; const double* weight;
    float* scores; int64_t ld;
};
void launch_tfidf_score(const TfidfScoreArgs& a, hipStream_t s);
// the hand-over of nvsm_rerank: cand[off[q] .. off[q + 1]) = the ids of query q's first off[q + 1] − off[q] sorted keys (rows of
// npad), ascending, for q < Q; off [Q + 1] on the device; nsort: a power of two >= every list, <= kRerankMaxDepth (LDS: 4 B per slot)
constexpr int kRerankMaxDepth = 4096;      // NVSM_RERANK_MAX_DEPTH
void launch_rerank_gather(const unsigned long long* keys, int64_t npad, const int64_t* off, int* cand, int Q, int nsort, hipStream_t s);
// two ranked lists [Q][k] (+ counts) -> their fused list [Q][2 k] (+ counts); npad: a power of two >= 2 k; k <= kFuseMaxTopK
struct FuseArgs {
    const int64_t* ids_a; const float* scores_a; const int64_t* counts_a;
    const int64_t* ids_b; const float* scores_b; const int64_t* counts_b;
    int k; int npad; float alpha; int normalizer;
    int64_t* out_ids; float* out_scores; int64_t* out_counts;
    const float* query_alpha;      // null: every query at `alpha`; given [Q]: query q at query_alpha[q] (nvsm_rank_ensemble_cv)
};
void launch_fuse_lists(const FuseArgs& a, int Q, hipStream_t s);
// the alpha sweep of the fusion (fuse_sweep_kernel; include/cunvsm_amd.h nvsm_ensemble_sweep): the two lists of f
// (f.alpha, f.out_* are not looked at) matched and normalised once per workgroup, then for every alpha of the workgroup's strip the
// fused order of fuse_lists_kernel and eval_metrics_kernel's row of its first min(depth, count) entries (depth 0: all), all in LDS.
// e: the call's judgments as launch_eval_metrics reads them, e.q0 the round's first query; table [num_alphas][total_queries][width]
// doubles on the device, width = NVSM_EVAL_FIXED + 3 e.num_cutoffs. Grid: (queries of the round, strips of kFuseSweepStrip alphas).
constexpr int kFuseSweepStrip = 8;         // alphas one workgroup sweeps behind one id match
constexpr int kFuseSweepMaxAlphas = 1024;  // NVSM_SWEEP_MAX_ALPHAS
struct FuseSweepArgs {
    FuseArgs f; EvalArgs e;
    const float* alphas; int num_alphas; int depth;
    double* table; int64_t total_queries;
};
void launch_fuse_sweep(const FuseSweepArgs& a, int Q, hipStream_t s);

// ---- inverted index of the uploaded corpus (index.hip; include/cunvsm_amd.h nvsm_corpus_index) ----
// The build behind sort_pairs(keys = tokens, vals_in = nullptr): term [n] the sorted tokens, pos [n] their arena positions.
// launch_index_docs: pos[i] -> the document of that position, in place (doc_offsets [num_documents + 1], the last one n).
void launch_index_docs(int* pos, int64_t n, const int64_t* doc_offsets, int64_t num_documents, hipStream_t s);
// heads = entries whose (term, document) differs from their predecessor's. tile_sums [index_tiles(n) + 1]: every tile's heads, then
// (a second launch, one workgroup) their exclusive prefixes with the total P behind them
int64_t index_tiles(int64_t n);
void launch_index_scan(const int* term, const int* doc, int64_t n, int* tile_sums, hipStream_t s);
// post_doc [P], head_pos [P + 1] (a posting's first entry; head_pos[P] = n), post_off / tok_off [V + 1]: a term's first posting and
// first sorted entry (df and cf are their differences). Every element has exactly one writer.
void launch_index_write(const int* term, const int* doc, int64_t n, int64_t V, const int* tile_sums, int* head_pos, int* post_doc,
                        int64_t* post_off, int64_t* tok_off, hipStream_t s);
void launch_index_tf(const int* head_pos, int64_t P, int* post_tf, hipStream_t s);      // post_tf[p] = head_pos[p + 1] − head_pos[p]
// The postings form of launch_lex_score / launch_tfidf_score: the same scores [Q][ld] of the slab [d0, d0 + S), the same bits.
// terms [num_slots]: the round's distinct terms by slot; entries as LexScoreArgs' (qoff, tslot, c0 = idf for TF-IDF, base, weight);
// entry_query [num_entries]: the query of an entry; first [num_entries]: 1 where the entry is the first of its term in its query;
// lo / hi [num_slots]: scratch, a term's postings inside the slab. max_df: the longest list among the round's terms (sizes the grid).
struct PostingsArgs {
    const int64_t* post_off; const int* post_doc; const int* post_tf; const int64_t* doc_offsets;
    const int* terms; int num_slots; int64_t* lo; int64_t* hi;
    int64_t d0; int S; int Q; int num_entries; int method; double param; double k1, b, avgdl;
    const int* qoff; const int* tslot; const int* entry_query; const int* first;
    const double* c0; const double* base; const double* weight;
    float* scores; int64_t ld;
};
void launch_postings_fill(const PostingsArgs& a, int64_t max_df, bool tfidf, hipStream_t s);

// ---- sequential dependence: ordered and unordered term pairs (sdm.hip; include/cunvsm_amd.h nvsm_sdm_rank) ----
constexpr int kSdmTile = 256;              // positions of a document staged at a time: the workgroup
constexpr int kSdmMaxWindow = 64;          // NVSM_SDM_MAX_WINDOW: the halo behind a tile is at most 63 positions
constexpr int kSdmSlots = kLexSlots;       // distinct terms of a round: tf counters, 4 KiB of LDS
constexpr int kSdmPairs = 1024;            // distinct (first, second) pairs of a round: od and uw counters, 8 KiB of LDS
// What the counting reads of a round. slot_of [num_words]: as launch_lex_set_slots leaves it for the round's terms. The pair entries
// of slot s are ent_off[s] .. ent_off[s + 1) (ent_off [num_slots + 1]): ent_other[e] the slot of the pair's other term, ent_pair[e] =
// pair id << 1 | first, first = 1 where s is the pair's first term (the entry that also counts the ordered form). A pair (a, b),
// a != b, has one entry under a (first) and one under b; a pair (a, a) has its first entry alone, so a position counts once.
struct SdmCountArgs {
    const int* tokens; const int64_t* doc_offsets; const int* slot_of;
    const int* ent_off; const int* ent_other; const int* ent_pair;
    int num_slots; int num_pairs; int window;
};
// cf_o[p] += od(pair p; d), cf_u[p] += uw(pair p; d) over every document d < num_documents; both zeroed by the caller
void launch_sdm_collect(const SdmCountArgs& a, int64_t num_documents, unsigned long long* cf_o, unsigned long long* cf_u, hipStream_t s);
// scores[q][d - d0] for q < Q, d in [d0, d0 + S), the layout of launch_lex_score. Group g (0 terms, 1 ordered, 2 unordered) of query q
// has the members goff[g][q] .. goff[g][q + 1) (goff [3][Q + 1], indices into index / c0 / base, query order): index[j] a slot (g = 0)
// or a pair id, c0[j] and base[j] = log(c0[j]) as LexScoreArgs'. score = Σ_g coef[q][g]·(Σ_j log term / members), the groups in the
// order 0, 1, 2, over the groups with members and coef > 0; fp64, every operation rounded on its own, narrowed once; -inf when no
// member of group 0 occurs in d.
struct SdmScoreArgs {
    SdmCountArgs count;
    int64_t d0; int S; int Q; int method; double param;
    const int* goff; const int* index; const double* c0; const double* base; const double* coef;
    float* scores; int64_t ld;
};
void launch_sdm_score(const SdmScoreArgs& a, hipStream_t s);

// ---- the positional layer of the index, and the SDM rounds served from it (index.hip, sdm.hip; include/cunvsm_amd.h
// nvsm_corpus_index_positions) ----
// Behind sort_pairs(keys = tokens, vals_in = nullptr): pos [n] the sorted entries' arena positions -> doc[i] their document, pos[i] the
// offset inside it (position − doc_offsets[document]). One writer per element.
void launch_index_positions(int* pos, int* doc, int64_t n, const int64_t* doc_offsets, int64_t num_documents, hipStream_t s);
// what launch_postings_fill does before its scorer: p[0 .. n) = -inf; lo / hi [n]: the postings of terms[s] inside [d0, d0 + S)
void launch_index_fill(float* p, int64_t n, hipStream_t s);
void launch_index_bounds(const int64_t* post_off, const int* post_doc, const int* terms, int n, int64_t d0, int S, int64_t* lo, int64_t* hi,
                         hipStream_t s);
// The postings with positions: post_first [P + 1] a posting's first entry of pos [N], its in-document offsets, ascending.
// pair_a / pair_b [num_pairs]: the slots of a pair's first and second term; terms [num_slots]: the round's terms by slot.
struct SdmPostingsArgs {
    const int64_t* post_off; const int* post_doc; const int* post_tf; const int* post_first; const int* pos;
    const int* terms; const int* pair_a; const int* pair_b; int num_slots; int num_pairs; int window;
};
// launch_sdm_collect's sums from the postings: cf_o[p] += Σ_d od(pair p; d), cf_u[p] += Σ_d uw(pair p; d); both zeroed by the caller
void launch_sdm_postings_collect(const SdmPostingsArgs& a, int64_t max_df, unsigned long long* cf_o, unsigned long long* cf_u, hipStream_t s);
// launch_sdm_score's slab from the postings, the same bits. `score` as launch_sdm_score reads it (of score.count only doc_offsets);
// entry_query / first [goff[0][Q]]: the query of a member of group 0, and 1 where it is the first of its slot in its query;
// lo / hi [num_slots]: scratch, a term's postings inside the slab. max_df: the longest list among the round's terms.
struct SdmPostingsScoreArgs {
    SdmScoreArgs score; SdmPostingsArgs post;
    const int* entry_query; const int* first; int num_entries; int64_t* lo; int64_t* hi;
};
void launch_sdm_postings_score(const SdmPostingsScoreArgs& a, int64_t max_df, hipStream_t s);


}  // namespace cunvsm
