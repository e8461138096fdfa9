/* Unit-test and profiling hooks of the MI355X NVSM / LSE engine — libcunvsm_amd_testhooks.so.
 *
 * NOT part of the drop-in surface (include/cunvsm_amd.h) and not exported by libcunvsm_amd.so: tests/, bench.py's --gate-us
 * profiling aid and tools/exp/ load this library behind the product library (cunvsm_amd/_lib.py does it on first use of a hook);
 * it calls the product's own kernel launchers and carries no kernels of its own. */
#ifndef CUNVSM_AMD_TEST_HOOKS_H
#define CUNVSM_AMD_TEST_HOOKS_H

#include "cunvsm_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Debug / unit-test hooks for individual kernels (tests only; not part of the drop-in surface). */
int nvsm_debug_gemm(int variant, int M, int N, int K, const float* hostA, const float* hostB, float* hostC);
/* ONE of the batch-sized projection products C[M][N] = alpha * A[M][K] * B (+ bias) by its own launcher - not launch_gemm's
 * dispatch - with any of the epilogues the kernels fuse into the product. Everything past B is optional (null / 0 = absent).
 * Every output buffer starts as 0xFF bytes on the device (NaN as float and as double): a refused launch leaves all of them so,
 * a launch must have written every element it owns. The planes of B are cut fresh on every call. */
enum { NVSM_DEBUG_GEMM_ROWS = 0, NVSM_DEBUG_GEMM_RSPLIT = 1, NVSM_DEBUG_GEMM_SPLIT = 2, NVSM_DEBUG_GEMM_TSTAT = 3,
       NVSM_DEBUG_GEMM_TILED = 4 /* the tiled kernel through launch_gemm, the four others switched off */ };
typedef struct nvsm_debug_gemm_epilogue_args {
    int kernel, b_layout, M, N, K;   /* b_layout 0: B is [K][N]; 1: B is stored [N][K] */
    const float* A;                  /* host [M][K]; ignored with the gather (A is then made, not read) */
    const float* B;
    float* C;                        /* out [M][N] */
    float alpha;
    const float* bias;               /* [N] */
    double* colstats;                /* out [2][N]: ordered column sums of C and of its squares */
    float* rowsq; float rowsq_scale; /* out [M]: rowsq_scale * sum over the columns of C squared (parts added by launch_sum_parts) */
    /* batch-norm backward on the rows of A on the way in; sums non-null alone (pre null) = the bias gradient only */
    const float* pre; const float* mean; const float* inv_std; const double* sums; double n_global;
    float* dbeta; float* dgamma; float* grad_bias;   /* out [K] */
    /* word gather-mean on the staging of A (rsplit only): table [table_rows][K], idx [M][window], wts [M][window] or null */
    const float* table; int64_t table_rows; const int64_t* idx; const float* wts; int window;
    float* A_out;                    /* out [M][K]: A after the launch (dx with the batch-norm backward, the phrases with the gather) */
    int* launched;                   /* out: 1 = the launcher launched, 0 = it refused */
} nvsm_debug_gemm_epilogue_args;
int nvsm_debug_gemm_epilogue(const nvsm_debug_gemm_epilogue_args* args);
/* Host-only (never touches the GPU): whether that launcher covers (shape, epilogue flags, gather window), and its plan word:
 *   rows    waves | tpw << 8
 *   rsplit  waves | rch << 8 | (odd number of k steps: one step of padding) << 16 | columns of the last 32-column tile << 24
 *   split   16-column blocks | fewest blocks of a wave << 8 | most blocks of a wave << 16
 *   tstat   parts | NT << 8 | mixed << 16 | KG << 24 */
enum { NVSM_DEBUG_EPI_COLSTATS = 1, NVSM_DEBUG_EPI_ROWSQ = 2, NVSM_DEBUG_EPI_BN = 4, NVSM_DEBUG_EPI_BIAS = 8, NVSM_DEBUG_EPI_GATHER = 16,
       NVSM_DEBUG_EPI_BIAS_GRAD = 32 };
int nvsm_debug_gemm_plan(int kernel, int b_layout, int M, int N, int K, int flags, int window, int* covers, unsigned* plan);
/* Host-only (never touches the GPU): the layout of the first round of a retrieval call that searches `rows` rows for the top k of
 * `queries` queries with a score slab of slab_mb MB (NVSM_RANK_SLAB_MB) and at most slab_cap rows per slab (0: no cap) - the
 * function the rounds of nvsm_rank, nvsm_lexical_rank and nvsm_neighbors call. out[5] = queries of the round, rows per slab, leading
 * dimension of the slab, keys selected per query, keys per query padded to a power of two. With lengths[queries] (the candidate
 * lists' lengths) the candidate form: rows, k, slab_mb and slab_cap are not read, out = round, 0, 0, 0, padded longest list. */
int nvsm_debug_rank_layout(int64_t rows, int64_t k, int64_t queries, int64_t slab_mb, int64_t slab_cap, const int64_t* lengths, int64_t* out);
/* Queues a kernel on the handle's stream that spins for `microseconds` of GPU wall clock: profiling runs put it in
 * front of a step so that the host has queued the whole step before the GPU starts it (tools/rocprof_summary.py timeline). */
int nvsm_debug_delay(nvsm_model* m, int microseconds);
/* table passes of the update in one launch (1, the default) or as the three launches chunk / level-2 / rows (0): the two
 * forms are bit-identical (tests/test_gpu_parity.py); process-wide */
int nvsm_debug_set_table_pass_form(int one_launch);
/* ONE table pass of the update on caller-supplied inputs (tests/test_gpu_table_pass.py): the host arrays are uploaded, then the
 * product's own launchers run in the order model.cpp calls them - sort_pairs, launch_csr_build, launch_chunk_order when the
 * chunks get an order, launch_table_pass - on a workspace sized by the product's own arithmetic (csr_chunk_caps /
 * csr_chunk_entries, kernels.h), and the state is copied back.
 * Lazy decay (tests/test_gpu_lazy_rows.py): with `stamp` given the hook does what Model::update_entities / update_words do for a
 * lazy table, in their order - RowPassArgs::lazy = 1 and ::pending = (stamp, lazy_decay, now); for the kinds with a per-row scalar
 * launch_lazy_refresh with scalars_only on the CSR's touched list into a snapshot buffer of the hook's own (0xFF bytes to begin
 * with; s_v from fill_adam_consts for the Adam kinds, 1 otherwise), which the pass reads as sc_in while it writes the stored
 * scalar in place (no ping-pong flip); launch_table_pass; launch_stamp_rows(now + 1). The stored scalar is what sc_in uploads, and
 * sc_out receives it back for every row, visited or not; stamp_out receives the stamps. prev_keys must be null.
 * Refused: NVSM_ERR_INVALID_ARGUMENT for a stamp that is negative, ahead of `now` or more than 128 updates (kLazyHistory) behind
 * it - the row pass does not clamp, such a row would read a stale slot of the ring -; NVSM_ERR_UNSUPPORTED for the kinds the
 * model never makes lazy (4 dense Adam, 5 full Adam) and for 6, the accumulator pass, which runs in front of the lazy pass proper.
 * The form of the pass comes from the fields below alone - a Tuning of the hook's own with every other switch at its default, and
 * the process-wide launch form put back on exit -, never from the environment.
 * Entry e (its position in `keys`) reads source row e / div of X and coefficient coef[e]: num_src * div >= max(n, prev_n), and
 * coef, where given, has max(n, prev_n) elements. The partial sums of the chunk tree start as 0xFF bytes (NaN). */
typedef struct nvsm_debug_table_pass_args {
    int table;                       /* 0 words (q += coef * sq_src, src_scale applies), 1 entities (q += coef^2 * sq_src) */
    int kind;                        /* RowKind (kernels.h): 0 SGD, 1 Adagrad, 2 Adam m/v, 3 sparse Adam, 4 dense Adam, 5 full Adam, 6 accumulator */
    int64_t rows; int dim;
    int64_t n; const int32_t* keys;  /* the table row of every entry, in batch order, each in [0, rows) */
    int div; int64_t num_src;
    const float* X;                  /* [num_src][dim] */
    const float* coef;               /* per entry: wts (words) / coefs (entities); null = 1 */
    const float* sq_src;             /* [num_src] or null */
    const float* src_scale;          /* [num_src] or null (words only) */
    float* P; float* m; float* v;    /* in / out [rows][dim]; m and v may be null for the kinds that do not use them */
    const float* sc_in; float* sc_out;   /* per-row scalar [rows]: sc_out is uploaded too (rows the pass does not visit keep what it held);
                                            sc_out == sc_in: updated in place, as the accumulator pass of Adagrad's words update does */
    float lr, lambda, decay, bc; int dense;
    int wide;                        /* RowPassArgs::wide (a ROW_SGD pass of an Adam update) */
    int nt;                          /* bit 0: RowPassArgs::nt_m, bit 1: nt_p */
    int64_t max_entries; int adam;   /* what the workspace is sized for (>= n, >= prev_n); the handle's update method is Adam */
    int one_launch, chunk_order, fill_in_bounds; int64_t entry_walk_min;
    int64_t prev_n; const int32_t* prev_keys;   /* optional: a batch run first through the same workspace, on scratch copies of the state */
    /* out (each may be null) */
    int* path;                       /* TablePassPath: 0 dense, 1 list walk, 2 entry walk */
    int* chunk;                      /* entries per level-1 chunk */
    int* num_chunks;                 /* [2]: level-1 / level-2 chunks the CSR build reserved */
    int* max_chunks; int* max_chunks2;
    int* arrive_left;                /* arrival counters of the one-launch pass that are not back at zero after it */
    /* lazy decay (null / 0 = none: the rows are current) */
    const int32_t* stamp;            /* [rows]: updates applied to each row */
    const float* lazy_decay;         /* [128]: factor of update u + 1 at [u % 128] */
    int now;                         /* updates applied to the table */
    int32_t* stamp_out;              /* out [rows]: the stamps after launch_stamp_rows(now + 1) */
} nvsm_debug_table_pass_args;
int nvsm_debug_table_pass(const nvsm_debug_table_pass_args* args);
/* ONE launch_loss (csrc/loss_bn.hip) on caller-supplied inputs (tests/test_gpu_loss_shapes.py): the host arrays are uploaded, the
 * constants of the kernel's arguments come from the function Model::forward fills them with (kernels.h fill_loss_consts, batch-norm
 * epsilon 1e-4), the product's own launch_loss runs `repeats` times on ONE grid-sum workspace - sized as the model sizes it for a
 * batch of B, ceil(B / 4) contributions, its arrival counters zeroed once in front of the first launch - and everything is copied
 * back. The dispatch follows its rules alone - a Tuning of the hook's own at its defaults -, never the environment.
 * Every output buffer starts as 0xFF bytes in front of every launch and carries a guard behind what the kernel owns, which comes
 * back too: one more row for proj, dy ([B + 1][de]), bn_mean, bn_inv_std ([2][de]) and colstats ([3][de]), one more element for
 * pp ([B + 1]), R more for coef and probs ([(B + 1) * R]). Output pointers may be null.
 * Refused: NVSM_ERR_UNSUPPORTED for a lazy view (stamp non-null) where the kernel of the shape does not apply one
 * (loss_reads_lazily false: the model refreshes the rows instead); NVSM_ERR_INVALID_ARGUMENT for a row whose stamp is negative,
 * ahead of `now` or more than 128 updates (kLazyHistory, the length of the factor ring) behind it, and for ids outside the table. */
typedef struct nvsm_debug_loss_args {
    int64_t B; int de, R, k;
    const float* pre;                /* [B][de] */
    int bn; const double* bn_sums;   /* [2][de]: column sums of pre and of its squares over bn_n rows */
    double bn_n; const float* bias;  /* [de] (read with bn only: without it pre holds the bias already) */
    const float* E; int64_t rows;    /* [rows][de] */
    const int32_t* ids;              /* [B * R], each in [0, rows) */
    const float* inst_w;             /* [B] or null */
    int nonlinearity;                /* 0 tanh, 1 hard_tanh */
    int clip_sigmoid, bias_negative_samples, l2_entity;
    double b_global;                 /* the global batch size behind 1 / B in the multipliers */
    const int32_t* stamp;            /* [rows] or null: updates applied to each row of E (a lazy view) */
    const float* decay;              /* [128]: factor of update u + 1 at [u % 128] */
    int now;                         /* updates applied to the table */
    int64_t rows_for_dispatch;       /* 0: rows. Stands in for LossArgs::E_rows, which only the choice of the two-row-set form reads */
    int repeats;
    /* out */
    float* proj; float* dy; float* coef; float* probs; float* pp; float* bn_mean; float* bn_inv_std;
    double* loss;                    /* [1] */
    double* colstats;                /* [3][de]: sums of dy, sums of dy * xhat (written with bn only), guard */
    int* plan;                       /* [10], LossPlan (kernels.h): family (1 rows, 2 generic), rb, lazy, pipe, v, niter, l2e, examples per wave, grid, LDS bytes */
    int* arrive_left;                /* arrival counters that are not back at zero after the last launch */
} nvsm_debug_loss_args;
int nvsm_debug_loss(const nvsm_debug_loss_args* args);
/* nvsm_neighbors' scan through the plain kernel whatever the dimension (1) or by its own dispatch (0, the default): how
 * tools/bench_neighbors.py holds the MFMA scan with the tail chunk against the plain scan on the same table; process-wide */
int nvsm_debug_neighbors_force_plain(int on);
/* ONE launch of nvsm_ngram_search's phrase-row generator (csrc/ngram.hip launch_ngram_rows) on caller-supplied inputs: G [m][de]
 * host (what the call makes as T·W[S]), bias [de], c and act (NVSM_TANH, NVSM_HARD_TANH, else identity) as launch_rank_bias_act
 * takes them. The rows [p0, p0 + S) of the 1- and 2-gram stack over m words are written to out[out_row0 .. out_row0 + S); out
 * [out_rows][de] is uploaded whole before the launch and comes back whole, so whatever the caller filled the other rows with must
 * still be there.
 * Refused with NVSM_ERR_INVALID_ARGUMENT: m outside [1, 65 535], rows outside the stack or outside out. */
int nvsm_debug_ngram_rows(const float* G, int64_t m, int de, const float* bias, float c, int act, int64_t p0, int64_t S, float* out,
                          int64_t out_rows, int64_t out_row0);
/* nvsm_tsne's stages on caller-supplied host inputs, through the product's own launchers (csrc/tsne.hip) and host functions
 * (csrc/ranking.cpp tsne_pca_start / tsne_descent). Sizes: 2 <= n <= NVSM_TSNE_MAX_ROWS, 1 <= d <= 4096, else
 * NVSM_ERR_INVALID_ARGUMENT.
 * affinities: X [n][d] -> the joint probabilities P in rows 1 .. n of P_out [n + 2][n]; P_out is uploaded whole before the launches
 *   and comes back whole, so rows 0 and n + 1 must return as the caller filled them. cond_out [n][n] (may be NULL): the
 *   conditional probabilities the perplexity search left, which the symmetrised P no longer shows.
 * gradient: for P [n][n] and Y [n][2], grad_out [n][2] = 4·(e·attractive − repulsive / Z) as tsne_update_kernel forms it and
 *   *kl_out = KL(e·P ‖ Q) as the convergence check evaluates it; Y is left as it is.
 * pca: Y0_out [n][2] = nvsm_tsne's NVSM_TSNE_INIT_PCA start of the rows X [n][d]; identical rows are refused.
 * descent: the two-phase loop on P [n][n] from Y [n][2] (overwritten with the result): opt's early_exaggeration, learning_rate
 *   (> 0: no 'auto' here), min_grad_norm, max_iter and n_iter_without_progress, and `exploration` (1 .. max_iter) iterations in the
 *   first phase, which the C ABI fixes at min(250, max_iter). */
int nvsm_debug_tsne_affinities(const float* X, int64_t n, int d, float perplexity, float* P_out, float* cond_out);
int nvsm_debug_tsne_gradient(const float* P, const float* Y, int64_t n, float exaggeration, float* grad_out, double* kl_out);
int nvsm_debug_tsne_pca(const float* X, int64_t n, int d, float* Y0_out);
int nvsm_debug_tsne_descent(const float* P, float* Y, int64_t n, const nvsm_tsne_options* opt, int exploration, double* kl_out,
                            int32_t* n_iter_out);
/* nvsm_tsne_sparse's stages on caller-supplied host inputs, through the product's own launchers (csrc/tsne_sparse.hip) and host
 * functions (csrc/ranking.cpp tsne_sparse_knn / tsne_sparse_affinities / tsne_sparse_descent). Sizes: 2 <= n <=
 * NVSM_TSNE_SPARSE_MAX_ROWS, 1 <= d <= 4096, 1 <= k <= min(n − 1, NVSM_TSNE_SPARSE_MAX_NEIGHBORS), 2·n·k < 2^31, else
 * NVSM_ERR_INVALID_ARGUMENT.
 * knn: ids_out / d2_out [n][k] = every row's k nearest other rows of X [n][d] and their squared distances, nearest first, ties by
 *   ascending id. round_rows > 0 forces that many query rows per round (0: the product's layout), so that a small n crosses
 *   several rounds.
 * sparse_affinities: knn, then the perplexity search and the symmetrisation: the CSR matrix P as indptr_out [n + 1], indices_out /
 *   data_out [indptr_out[n]] — give both room for 2·n·k entries — and cond_out [n][k] (may be NULL), the conditional probabilities
 *   beside the neighbour lists.
 * sparse_gradient: for a CSR matrix P (columns inside [0, n) or the hook refuses) and Y [n][2], grad_out [n][2] = 4·(e·attractive −
 *   repulsive / Z) and *kl_out = the error as the convergence check evaluates it; Y is left as it is. ranges > 0 forces the number
 *   of column ranges of the repulsion (0: the product's layout; at most 4096).
 * sparse_descent: nvsm_debug_tsne_descent on a CSR matrix. */
int nvsm_debug_tsne_knn(const float* X, int64_t n, int d, int k, int64_t round_rows, int32_t* ids_out, float* d2_out);
int nvsm_debug_tsne_sparse_affinities(const float* X, int64_t n, int d, float perplexity, int k, int64_t* indptr_out, int32_t* indices_out,
                                      float* data_out, float* cond_out);
int nvsm_debug_tsne_sparse_gradient(const int64_t* indptr, const int32_t* indices, const float* data, const float* Y, int64_t n,
                                    float exaggeration, int ranges, float* grad_out, double* kl_out);
int nvsm_debug_tsne_sparse_descent(const int64_t* indptr, const int32_t* indices, const float* data, float* Y, int64_t n,
                                   const nvsm_tsne_options* opt, int exploration, double* kl_out, int32_t* n_iter_out);
/* nvsm_kmeans' passes on caller-supplied host inputs, through the product's own launchers (csrc/kmeans.hip) and host functions
 * (csrc/ranking.cpp kmeans_prepare / kmeans_assign_pass / kmeans_update_pass / kmeans_plusplus). Sizes: 1 <= n < 2^31, 1 <= d <= 4096,
 * 1 <= k <= min(n, NVSM_KMEANS_MAX_CLUSTERS), else NVSM_ERR_INVALID_ARGUMENT.
 * assign: one assignment pass of X [n][d] against C [k][d]: labels_out [n], dist_out [n] (may be NULL) = the kernel's own fp32
 *   squared distance of each row to its centre.
 * update: one centre update from labels [n] (in: values in [0, k); out: relocated rows rewritten) with empty clusters settled against
 *   C_old [k][d]: C_new [k][d], counts_out [k], *shift_out = Σ (C_new − C_old)².
 * plusplus: the k-means++ start: rows_out [k] the chosen positions, centers_out [k][d] (may be NULL) their rows. seed >= 1. */
int nvsm_debug_kmeans_assign(const float* X, int64_t n, int d, const float* C, int k, int32_t* labels_out, float* dist_out);
int nvsm_debug_kmeans_update(const float* X, int64_t n, int d, int32_t* labels, const float* C_old, int k, float* C_new,
                             int64_t* counts_out, double* shift_out);
int nvsm_debug_kmeans_plusplus(const float* X, int64_t n, int d, int k, int64_t seed, int64_t* rows_out, float* centers_out);
/* the stable (row, entry) radix sort alone: keys of `bits` significant bits in, sorted keys + their original positions out */
/* average ms per launch of a batch-sized projection product on device operands (extras: 1 = column statistics, 2 = row sums of squares) */
int nvsm_debug_gemm_time(int b_layout, int M, int N, int K, int extras, int repeats, float* avg_ms);
/* the projection-gradient product alone (which 0 = the split-bf16 split-K kernel, 1 = its wave-sized form gemm_dtw.hip, 2 = tiled exact-fp32 kernel): average ms of the product and of its slab reduce */
int nvsm_debug_dt_time(int M, int N, int rows, int slabs, int repeats, int which, float* kernel_ms, float* reduce_ms);
int nvsm_debug_sort(int64_t n, int bits, const int32_t* keys, int32_t* keys_out, int32_t* vals_out, int repeats, float* avg_ms);
int nvsm_debug_gather_mean(int64_t num_rows, int dim, const float* table, const int64_t* idx, const float* wts,
                           int window, int64_t num_out, float* out);
/* ... through a LazyView (stamp [num_rows], decay [128]: factor of update u + 1 at [u % 128], now): launch_gather_mean applies the
 * factors a row sat out as it gathers the row and writes nothing back - table_out [num_rows][dim] receives the table after the
 * launch. Refused as in nvsm_debug_loss: a stamp that is negative, ahead of `now` or more than 128 behind it; ids outside the table. */
int nvsm_debug_gather_mean_lazy(int64_t num_rows, int dim, const float* table, const int64_t* idx, const float* wts,
                                int window, int64_t num_out, const int32_t* stamp, const float* decay, int now,
                                float* out, float* table_out);
/* ONE launch_lazy_refresh (csrc/update.hip: lazy_refresh_kernel<1 / 4>, or lazy_scalar_snapshot_kernel with scalars_only) on
 * caller-supplied inputs. P and m carry one guard row behind the table ([rows + 1][dim]), sc and sc_snapshot one guard element
 * ([rows + 1]); everything is uploaded, the snapshot starts as 0xFF bytes, and everything comes back. `list` (n_list row ids, each
 * in [0, rows), no id twice) goes to the device with its count, as Csr::touched / num_touched do; null = all rows.
 * Refused with NVSM_ERR_INVALID_ARGUMENT: a stamp that is negative, ahead of `now` or more than 128 behind it. */
typedef struct nvsm_debug_lazy_refresh_args {
    int64_t rows; int dim;
    float* P;                        /* in / out [rows + 1][dim] */
    float* m;                        /* in / out [rows + 1][dim] or null */
    float* sc;                       /* in / out [rows + 1] or null */
    float* sc_snapshot;              /* out [rows + 1] or null */
    const int32_t* stamp;            /* [rows] */
    int32_t* stamp_out;              /* out [rows] */
    const int32_t* list; int64_t n_list;
    int now; float s_m, s_v;
    const float* decay;              /* [128]: factor of update u + 1 at [u % 128] */
    int scalars_only;
} nvsm_debug_lazy_refresh_args;
int nvsm_debug_lazy_refresh(const nvsm_debug_lazy_refresh_args* args);
/* The document-frequency pass of nvsm_tfidf_rank alone (csrc/lexical.hip: launch_lex_df) on a caller-supplied corpus, the documents in
 * slabs of `slab` (1 .. 2^31 - 1; it need not be a multiple of 32 nor divide num_documents): df_out [num_words] = documents that
 * hold each word. The bit table [num_words][(slab + 31) / 32] is the hook's own. Refused with NVSM_ERR_INVALID_ARGUMENT: offsets that
 * do not start at 0, decrease or do not end at num_tokens; a token outside [0, num_words). */
int nvsm_debug_lex_df(const int32_t* tokens, int64_t num_tokens, const int64_t* doc_offsets, int64_t num_documents, int64_t num_words,
                      int64_t slab, int64_t* df_out);

/* ---- the streaming kernels of a training step, one launcher each (tests/test_gpu_step_kernels.py) ----
 * As nvsm_debug_loss and nvsm_debug_table_pass: host arrays go up, the product's own launcher runs once, everything comes back. Every
 * output starts as 0xFF bytes and carries a guard behind what the kernel owns (one more row or element), which comes back too. Bad
 * sizes and ids outside the table are refused with NVSM_ERR_INVALID_ARGUMENT on the host and never reach the device. */
/* launch_adam_u (csrc/update.hip): m [rows][dim], v [rows], idx [B][window] each in [0, rows); U_out [B + 1][dim].
 * B * (dim / 4 where dim is a multiple of 4, else dim) must stay below 2^32: the kernel counts its work items in 32 bits. */
int nvsm_debug_adam_u(int64_t rows, int dim, const float* m, const float* v, const int32_t* idx, int window, int64_t B, float bc,
                      float eps, float* U_out);
/* launch_adagrad_scale: acc [rows], idx [B][window]; scale_out [B + 1] */
int nvsm_debug_adagrad_scale(int64_t rows, const float* acc, const int32_t* idx, int window, int64_t B, float eps, float* scale_out);
/* launch_bn_dx (csrc/loss_bn.hip) on dy, pre [rows][dim], mean, inv_std [dim], sums [2][dim] (column sums of dy and of dy * xhat) and
 * n_global; with pre == NULL launch_colsum_finalize(sums, dim, grad_bias) instead, which reads the first row of sums only: dbeta and
 * dgamma come back as the 0xFF bytes they started as, dy_out is not written. rows * (dim / 4 or dim, as above) below 2^32. */
typedef struct nvsm_debug_bn_dx_args {
    int64_t rows; int dim;
    const float* dy; const float* pre; const float* mean; const float* inv_std;
    const double* sums; double n_global;
    float* dy_out;                               /* out [rows + 1][dim]: dy after the launch (dx) */
    float* dbeta; float* dgamma; float* grad_bias;   /* out [dim + 1] */
} nvsm_debug_bn_dx_args;
int nvsm_debug_bn_dx(const nvsm_debug_bn_dx_args* args);
/* ONE of the wave-per-row launchers of csrc/loss_bn.hip:
 *   MEANSQ          launch_row_meansq(x, rows, dim, scale)                      -> out_scalar
 *   L2_FORWARD      launch_l2_rows_forward(x, rows, dim)                        -> out (y), out_scalar (norms)
 *   L2_BACKWARD     launch_l2_rows_backward(g, x, norms, rows, dim, scale)      -> out (gin), out_scalar (msq; NULL: the launcher gets none).
 *                   in_place: ONE device buffer [rows + 1][dim] holding g is passed as g and as gin, as Model::backward does.
 *   MATERIALIZE     launch_materialize_grad_entity(coef, x = proj, rows, R, dim)               -> out
 *   MATERIALIZE_L2  launch_materialize_grad_entity_l2(coef, x = proj, E, ids, rows, R, dim)    -> out, out_scalar (msq; NULL: none)
 * For the two materialise ops `rows` counts gathered rows (entries j), x is proj [(rows + R - 1) / R][dim], coef [rows], ids [rows]
 * each in [0, table_rows), E [table_rows][dim]. out is [rows + 1][dim], out_scalar [rows + 1]. */
enum { NVSM_DEBUG_ROW_MEANSQ = 0, NVSM_DEBUG_ROW_L2_FORWARD = 1, NVSM_DEBUG_ROW_L2_BACKWARD = 2, NVSM_DEBUG_ROW_MATERIALIZE = 3,
       NVSM_DEBUG_ROW_MATERIALIZE_L2 = 4 };
typedef struct nvsm_debug_row_op_args {
    int op; int64_t rows; int dim;
    const float* x; const float* g; const float* norms; const float* coef;
    const float* E; int64_t table_rows; const int32_t* ids; int R;
    float scale; int in_place;
    float* out; float* out_scalar;
} nvsm_debug_row_op_args;
int nvsm_debug_row_op(const nvsm_debug_row_op_args* args);
/* The two ordered sums of csrc/gather_gemm.hip over parts [nparts][stride], n <= stride elements of each: which 0 =
 * launch_splitk_reduce, 1 = launch_sum_parts; out [n + 1]. Both buffers come from the device allocator (16-byte aligned), so
 * launch_splitk_reduce takes its float4 kernel exactly where n and stride are multiples of 4. */
int nvsm_debug_slab_sum(int which, const float* parts, int nparts, int64_t stride, int64_t n, float* out);
/* Host-only (never touches the GPU): gemm_split_planes_bytes / gemm_rsplit_planes_bytes (kind 1 / 2) of an N x K operand and the
 * plane_stride of its gemm_*_plane_target. */
int nvsm_debug_plane_sizes(int kind, int N, int K, int64_t* bytes, int64_t* plane_stride);
/* ONE launch_transform_update (csrc/update.hip) on T [dw][de] and b [de]. The kernel's scalars come from fill_transform_consts
 * (kernels.h), the function Model::update_transform derives them by, from (method, lr, lambda, t_transform: the Adam step count the
 * bias correction is taken at, 1 for the first update). T, gT, s0T, s1T are [dw * de + 1] and b, gb, s0b, s1b [de + 1]: all but the
 * last element go up, all come back, the last one being the 0xFF guard. s0* are required by Adagrad and Adam, s1* by Adam.
 * partial [slabs][dw * de] (or NULL): the dT product's slabs, added up by the update in place of gT's content.
 * plane_kind[i] (0 none, 1 gemm_split_plane_target, 2 gemm_rsplit_plane_target) for pt[0] = (N = de, K = dw, transposed 0) and
 * pt[1] = (N = dw, K = de, transposed 1): planes[i] receives the whole buffer (nvsm_debug_plane_sizes bytes; zero-filled in front
 * of the launch, as the model's are) the update wrote its bf16 pieces into, and fresh[i] the buffer launch_gemm_split_planes /
 * launch_gemm_rsplit_planes cut from the updated T with the model's arguments, into memory that started as 0xFF bytes. */
typedef struct nvsm_debug_transform_update_args {
    int method; int dw, de;
    float lr, lambda; uint64_t t_transform;
    float* T; float* b; float* gT; float* gb;
    float* s0T; float* s0b; float* s1T; float* s1b;
    const float* partial; int slabs;
    int plane_kind[2];
    unsigned char* planes[2]; unsigned char* fresh[2];
} nvsm_debug_transform_update_args;
int nvsm_debug_transform_update(const nvsm_debug_transform_update_args* args);

#ifdef __cplusplus
}
#endif
#endif /* CUNVSM_AMD_TEST_HOOKS_H */
