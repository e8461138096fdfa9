// Host side of the MI355X NVSM / LSE engine: owns the parameters, optimiser state and per-step
// workspaces in HBM and sequences the gfx950 kernels of kernels.h on one HIP stream.
// Mirrors Model<TextEntity::Objective> (include/cuNVSM/model.h:75-131): initialize / compute_cost /
// compute_gradients / update / get_cost, same argument meaning.
#pragma once

#include <cstdlib>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <map>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cunvsm_amd.h"
#include "kernels.h"

namespace cunvsm {

#define NVSM_HIP_CHECK(expr)                                                                         \
    do {                                                                                             \
        hipError_t _e = (expr);                                                                      \
        if (_e != hipSuccess)                                                                        \
            throw ::cunvsm::Error(NVSM_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

inline bool devbuf_poison() { return tuning().poison; }

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void alloc(size_t count, bool zero = false) {
        release();
        n = count;
        if (count == 0) return;
        NVSM_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)));
        // NVSM_POISON=1 (tests): buffers that are not cleared start as 0xFF bytes (NaN floats, -1 ints) instead of whatever
        // the allocator hands back — a kernel that reads one before it is written shows up at once
        if (!zero && !devbuf_poison()) return;
        NVSM_HIP_CHECK(hipMemset(p, zero ? 0 : 0xFF, count * sizeof(T)));
        // hipMemset of device memory returns once the fill is queued on the null stream, and the handle's streams are
        // non-blocking (no implicit order with the null stream): without this wait a kernel of the handle could read the
        // buffer before it was cleared (seen as a memory fault of lazy_refresh_kernel on a recycled, not yet zeroed stamp array)
        NVSM_HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// RCCL entry points resolved at run time (dlopen) so that single-GPU use never loads librccl and a
// process that already holds PyTorch's RCCL shares it.
struct RcclApi;

class Profiler {
 public:
    bool enabled = false;
    std::string only;          // when not empty, only these kernel groups (comma-separated) are timed (a few events per step instead of ~50)
    void begin(const char* name, hipStream_t s);
    void end(hipStream_t s);
    // the next event pair of group `name`, NOT recorded: the caller hands it to a single launch as that kernel's start / stop
    // events (kernels.h set_launch_events) — the group's time is then the kernel's own execution time, and nothing is queued
    // in front of or behind the kernel. false: the group is not being timed.
    bool bind(const char* name, hipEvent_t* start, hipEvent_t* stop);
    bool selected(const char* name) const;
    void note(const char* name) { if (enabled) ++notes_[name]; }      // a counter without events: which code path a launch took
    void reset();
    std::vector<std::string> names() const;
    bool get(const std::string& name, double* ms, int64_t* launches);
    ~Profiler();
 private:
    struct Slot { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; size_t used = 0; };
    std::map<std::string, Slot> slots_;
    std::map<std::string, int64_t> notes_;
    Slot* cur_ = nullptr;
};

struct TableState {           // one embedding table + its optimiser state + its per-step CSR workspace
    int64_t rows = 0;
    int dim = 0;
    DevBuf<float> P, m, vfull, sc[2];
    int sc_cur = 0;
    uint64_t t = 1;           // Adam step counter (cpp/updates_adam.cu:130)
    // CSR workspace. What the build writes and the update reads comes in two sets for the documents table: the build
    // of step k+1 (side stream, at the start of the step) then does not have to wait for the documents update of step k,
    // which trails into step k+1 and still reads the arrays of step k.
    struct CsrIndex {
        DevBuf<int> sorted_key, sorted_entry, chunk_base, chunk_desc, chunk2_base, chunk2_desc;
        DevBuf<int> touched;      // rows with entries (Csr::touched)
        DevBuf<int> chunk_order;  // Csr::chunk_order (large batches only)
        DevBuf<int> csr_zeroed;   // [row_begin (rows) | row_end (rows) | num_chunks (2) | num_touched | pad]: cleared by the sort's first launch
    };
    CsrIndex idx[2];
    int idx_sets = 1, idx_cur = 0;
    DevBuf<int> arrive_row, arrive2;      // arrival counters of the one-launch table pass (Csr)
    DevBuf<float> partial, partial_q, partial2, partial2_q;
    DevBuf<int> chunk_key, chunk_key_sorted;      // scratch of launch_chunk_order
    DevBuf<char> sort_temp;
    size_t sort_temp_bytes = 0;
    uint64_t sort_epoch = 0;      // (unused by the two-launch sort)
    int sort_bits = 1;
    int max_chunks = 0, max_chunks2 = 0;
    int64_t max_entries = 0;
    // lazy dense decay (kernels.h): for tables with at least as many rows as a batch has entries
    bool lazy = false;
    bool lazy_scalar = false;     // the per-row scalar state takes part (Adam v, document Adagrad accumulator)
    DevBuf<int> stamp;            // [rows] updates applied to the row
    int updates_done = 0;
    float decay_hist[kLazyHistory];
};

// The layout of one round of a retrieval call (ranking.cpp, DESIGN.md §9 "Dispatch by Q and k"), host arithmetic only: qn queries,
// slabs of S rows at leading dimension ld, n_keys selected keys per query padded to npad. Candidate lists (offsets of the queries on
// offer) have no slabs: S, ld and n_keys stay 0.
struct RankLayout { int64_t qn, S, ld, n_keys, npad; };
RankLayout rank_layout(int64_t rows, int64_t k, int64_t queries, int64_t score_floats, int64_t slab_cap = 0);      // slab_cap 0: none
RankLayout rank_layout_candidates(const int64_t* offsets, int64_t queries);

// ---- exact t-SNE (ranking.cpp; kernels: tsne.hip): the host side the product call and the test hooks share ----
// device scratch of a run over n rows; P [n][tsne_ld(n)] is filled by launch_tsne_conditionals + launch_tsne_joint
struct TsneScratch {
    DevBuf<float> x, p, y, upd, gains, gs, part;
    DevBuf<double> rows, pca;      // rows: rowsum [n] | klrow [n] | total, z, kl, |g|, the check's own z; pca: mean [d] | cov [d][d] | V [2][d]
    DevBuf<int64_t> ids;
    void grow_for(int64_t n, int d);
};
// Y0 [n][2] (device) = the rows X [n][d] (device) on their two leading principal axes, scaled to a standard deviation of 1e-4 in
// column 0: covariance on the device in fp64, cyclic Jacobi on the host, signs by each axis' entry of largest magnitude (the lower
// index on a tie). Throws NVSM_ERR_INVALID_ARGUMENT when that standard deviation is 0. Synchronous on s.
void tsne_pca_start(const float* X, int n, int d, TsneScratch& w, float* Y0, hipStream_t s);
// sklearn's two-phase _gradient_descent on Y [n][2] (device) for P in w.p: `exploration` iterations (momentum 0.5, P times
// early_exaggeration, n_iter_without_progress 250), then up to max_iter (momentum 0.8). learning_rate resolved by the caller.
// kl / n_iter: the error of the last evaluation and the index of the last iteration run. Synchronous on s.
void tsne_descent(TsneScratch& w, int n, const nvsm_tsne_options& opt, float learning_rate, int exploration, double* kl, int32_t* n_iter,
                  Profiler* prof, hipStream_t s);

// ---- sparse-affinity t-SNE (ranking.cpp; kernels: tsne_sparse.hip): the host side nvsm_tsne_sparse and the test hooks share
struct TsneSparseScratch {
    TsneScratch base;                      // x, y, upd, gains, gs, rows, pca, ids as nvsm_tsne uses them; its p and part stay empty
    DevBuf<int> nbr_id, indices;           // [n][k]; [nnz]
    DevBuf<float> nbr_d2, cond, data, attr, part;      // [n][k] twice; [nnz]; [n][2]; [n][ranges][3]
    DevBuf<int64_t> indptr;                // [n + 1]
    DevBuf<float> scores;                  // a neighbour round's slab
    DevBuf<unsigned long long> keys;
    DevBuf<char> sel_ws;
    int64_t nnz = 0;
    int forced_ranges = 0;                 // > 0 (test hooks): that many column ranges in the repulsion
    void grow_rows(int64_t n, int d);      // everything sized by n and d alone
};
// w.nbr_id / w.nbr_d2 [n][k]: every row's k nearest other rows of X [n][d] (device), nearest first, ties by ascending id; rounds of
// query rows as the retrieval calls run them (score slab of score_floats floats; round_rows > 0: that many rows a round)
void tsne_sparse_knn(const float* X, int n, int d, int k, int64_t round_rows, int64_t score_floats, TsneSparseScratch& w, Profiler* prof,
                     hipStream_t s);
// w.cond [n][k] and the CSR matrix P (w.indptr, w.indices, w.data, w.nnz) from w.nbr_id / w.nbr_d2. Synchronous on s.
void tsne_sparse_affinities(int n, int k, float perplexity, TsneSparseScratch& w, Profiler* prof, hipStream_t s);
// tsne_descent on the CSR matrix in w and w.base.y
void tsne_sparse_descent(TsneSparseScratch& w, int n, const nvsm_tsne_options& opt, float learning_rate, int exploration, double* kl,
                         int32_t* n_iter, Profiler* prof, hipStream_t s);

// ---- k-means (ranking.cpp; kernels: kmeans.hip): the host side the product call and the test hooks share ----
struct KmeansScratch {
    DevBuf<float> x, mean32, xn, c, c2, cc, cn, dist32;
    DevBuf<double> stats;      // column partials [slabs][d] | mean [d] | var [d] | mean variance, shift total, inertia, the draw's (total, position)
    DevBuf<double> part, shift, dist64, kpp_part;
    DevBuf<int> lab_a, lab_b, sorted_lab, pos, iota, start, choff, meta;      // meta: empty clusters, workgroups with a moved label
    DevBuf<int64_t> counts, ids;
    DevBuf<char> sort_temp;
    size_t sort_temp_bytes = 0;
    void grow_for(int64_t n, int d, int k);
    double* mean64(int n, int d) { return stats.p + static_cast<size_t>(kmeans_stat_slabs(n)) * d; }
    double* var(int n, int d) { return mean64(n, d) + d; }
    double* scalars(int n, int d) { return var(n, d) + d; }      // [0] mean variance [1] shift total [2] inertia [3..4] the draw
};
// column statistics of w.x [n][d] (w.mean32, the variances) and the centred rows' norms w.xn; queued on s
void kmeans_prepare(KmeansScratch& w, int n, int d, hipStream_t s);
// label [n], w.dist32 [n]: one assignment pass of w.x against C [k][d] (both device); queued on s
void kmeans_assign_pass(KmeansScratch& w, int n, int d, int k, const float* C, int* label, hipStream_t s);
// one centre update from label [n] (device; relocated rows are rewritten): empty clusters settled by nvsm_kmeans' rule against Cold,
// then Cnew [k][d], w.counts [k], the shift total in w.scalars()[1]. relocate false: empty clusters keep Cold's row (the final pass's
// counts). Returns the number of clusters that were empty. Synchronises s once (twice when a cluster was empty).
int kmeans_update_pass(KmeansScratch& w, int n, int d, int k, int* label, const float* Cold, float* Cnew, bool relocate, hipStream_t s);
// the k-means++ start of w.x: C [k][d] (device) and rows [k] (host) the chosen positions. Synchronous on s.
void kmeans_plusplus(KmeansScratch& w, int n, int d, int k, int64_t seed, float* C, int64_t* rows, hipStream_t s);

class Model {
 public:
    explicit Model(const nvsm_config& cfg);
    ~Model();

    void initialize(uint64_t seed);
    void initialize_from_rng_state();      // Glorot draws continue from the generator's current state
    uint64_t rng_get_state();
    void rng_set_state(uint64_t s);

    void compute_cost(const nvsm_batch& batch, const int64_t* entity_ids);
    void compute_gradients();
    void update(float lr, float scaled_lambda);
    float get_cost();
    double cost_f64() const { return cost_; }      // valid after get_cost()
    float scaled_regularization_lambda() const;
    void step(const nvsm_batch& batch, const int64_t* entity_ids, float lr, float* cost);
    // fold-in (include/cunvsm_amd.h nvsm_step_fold; fold.hip): compute_cost, then the documents update on the rows
    // [first_document, num_entities) alone — W, T, b and the rows below keep their logical values bit for bit
    void step_fold(const nvsm_batch& batch, const int64_t* entity_ids, int64_t first_document, float lr, float* cost);
    // the entity-entity similarity objective alone (text null) or mixed into the text objective (TextEntityEntityEntity,
    // cpp/objective.cu:698-745): see "entity-entity pairs" below
    void compute_cost_mixed(const nvsm_batch* text, const int64_t* entity_ids, const nvsm_pair_batch& pairs, const nvsm_mixture* mix);
    void step_mixed(const nvsm_batch* text, const int64_t* entity_ids, const nvsm_pair_batch& pairs, const nvsm_mixture* mix, float lr, float* cost);
    // the term-term similarity objective on the words table, alone or mixed into the text objective (TextEntityTermTerm,
    // cpp/objective.cu:747-794): see "term-term pairs" below
    void compute_cost_term_mixed(const nvsm_batch* text, const int64_t* entity_ids, const nvsm_pair_batch& pairs, const nvsm_mixture* mix);
    void step_term_mixed(const nvsm_batch* text, const int64_t* entity_ids, const nvsm_pair_batch& pairs, const nvsm_mixture* mix, float lr, float* cost);

    // training from an HBM-resident corpus (include/cunvsm_amd.h; corpus.hip): see "window references" below
    void corpus_upload(const nvsm_corpus* corpus);      // null: free it
    void compute_cost_windows(const nvsm_window_batch& wb, const int64_t* entity_ids);
    void step_windows(const nvsm_window_batch& wb, const int64_t* entity_ids, float lr, float* cost);
    int64_t step_windows_deferred(const nvsm_window_batch& wb, const int64_t* entity_ids, float lr);

    int64_t param_size(const std::string& name);
    void get_param(const std::string& name, float* dst, int64_t count);
    void set_param(const std::string& name, const float* src, int64_t count);
    // rows [first_row, first_row + rows) of an embedding table or of its per-row optimiser state
    void get_param_rows(const std::string& name, int64_t first_row, int64_t rows, float* dst);
    void set_param_rows(const std::string& name, int64_t first_row, int64_t rows, const float* src);
    void increment_param(const std::string& name, int64_t index, float delta);
    int64_t tensor_size(const std::string& name);
    void get_tensor(const std::string& name, float* dst, int64_t count);

    // Model::infer (cpp/model.cu:105-133) for ragged queries, and the ranking of py/nvsm/base.py:362-430 (rank.cpp)
    void infer(const nvsm_queries& q, const nvsm_rank_options& opt, float* out);
    void rank(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t* doc_ids, float* scores, int64_t* counts);
    // the same ranking plus per-query retrieval metrics computed on the device (eval.hip); doc_ids / scores / counts may be null
    // query-likelihood ranking over the resident corpus and its fusion with rank's list (include/cunvsm_amd.h; lexical.hip)
    void lexical_rank(const nvsm_queries& q, const nvsm_lexical_options& lex, int64_t* doc_ids, float* scores, int64_t* counts);
    void rank_ensemble(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_ensemble_options& ens,
                       const nvsm_judgments* j, double* metrics, int64_t* doc_ids, float* scores, int64_t* counts);
    // weighted queries and pseudo-relevance feedback (include/cunvsm_amd.h; lexical.hip)
    void lexical_rank_weighted(const nvsm_queries& q, const nvsm_lexical_options& lex, int64_t* doc_ids, float* scores, int64_t* counts);
    void relevance_model(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, int64_t* term_ids,
                         float* term_probs, int64_t* counts);
    void lexical_rank_prf(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, int64_t* doc_ids,
                          float* scores, int64_t* counts);
    void rank_ensemble_prf(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb,
                           const nvsm_ensemble_options& ens, const nvsm_judgments* j, double* metrics, int64_t* doc_ids, float* scores,
                           int64_t* counts);
    void evaluate(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_judgments& j, double* metrics, int64_t* doc_ids,
                  float* scores, int64_t* counts);
    // sequential dependence: terms, ordered pairs and unordered pairs in a window (include/cunvsm_amd.h; sdm.hip)
    void sdm_rank(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_sdm_options& sdm, int64_t* doc_ids, float* scores,
                  int64_t* counts);
    void sdm_pair_counts(const nvsm_queries& q, const nvsm_sdm_options& sdm, uint64_t* ordered, uint64_t* unordered);
    void rank_ensemble_sdm(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_sdm_options& sdm,
                           const nvsm_ensemble_options& ens, const nvsm_judgments* j, double* metrics, int64_t* doc_ids, float* scores,
                           int64_t* counts);
    // TF-IDF first stage over the resident corpus, and nvsm_rank over its candidates handed over on the device (include/cunvsm_amd.h;
    // lexical.hip); j and metrics both null or both given
    void tfidf_rank(const nvsm_queries& q, const nvsm_tfidf_options& opt, int64_t* doc_ids, float* scores, int64_t* counts);
    void rerank(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_rerank_options& rr, const nvsm_judgments* j, double* metrics,
                int64_t* doc_ids, float* scores, int64_t* counts);
    // supervised fusion (include/cunvsm_amd.h; lexical.hip fuse_sweep_kernel); fb null: list B is lexical_rank's
    void ensemble_sweep(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                        const nvsm_sweep_options& sw, const nvsm_judgments& j, double* table);
    void rank_ensemble_cv(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                          const nvsm_sweep_options& sw, const nvsm_cv_options& cv, const nvsm_judgments& j, float* fold_alpha,
                          double* fold_train_measure, int64_t* doc_ids, float* scores, int64_t* counts, double* metrics, double* sweep_metrics);
    // nearest neighbours among the word rows, the projected vocabulary or the document rows (py/nvsm/base.py:106-162, 325-353,
    // 362-430), and the similarity of pairs of rows (ranking.cpp)
    void neighbors(const nvsm_neighbor_queries& q, const nvsm_neighbor_options& opt, int64_t* ids, float* scores, int64_t* counts);
    // phrase_rows / scores [Q][top_k], terms [Q][top_k][max_cardinality], counts [Q], host (nvsm_ngram_search)
    void ngram_search(const nvsm_neighbor_queries& q, const nvsm_ngram_options& opt, int64_t* phrase_rows, int64_t* terms, float* scores,
                      int64_t* counts);
    void similarity(int space, const int64_t* a, const int64_t* b, int64_t n, int similarity, float* out);
    // exact t-SNE of rows of E or W (py/visualize.py; nvsm_tsne): embedding [num_rows][2] host
    void tsne(const nvsm_tsne_options& opt, float* embedding, double* kl_divergence, int32_t* n_iter);
    // the same picture from sparse affinities (nvsm_tsne_sparse): sklearn's barnes_hut at angle 0, no n × n memory
    void tsne_sparse(const nvsm_tsne_options& opt, const nvsm_tsne_sparse_options& sparse, float* embedding, double* kl_divergence,
                     int32_t* n_iter);
    // Lloyd's k-means of rows of E or W (nvsm_kmeans): labels [num_rows], centers [k][dim], counts [k], distances [num_rows] or null: host
    void kmeans(const nvsm_kmeans_options& opt, int32_t* labels, float* centers, int64_t* counts, float* distances, double* inertia, int32_t* n_iter);

    void set_stream(hipStream_t s);
    int64_t step_deferred(const nvsm_batch& batch, const int64_t* entity_ids, float lr);
    float deferred_cost(int64_t ticket);
    void wait_inputs();
    void synchronize();
    void debug_delay(int microseconds);
    void draw_reference_negatives(const int64_t* labels, int64_t B, int64_t* ids);
    void join_T();
    void join_E();
    void join_aux() { join_T(); join_E(); }
    void comm_init(const char id[128]);
    void average_tables();                 // data parallel: mean of the replicas' embedding tables (nvsm_dp_average_tables)
    int comm_ranks() const { return comm_ranks_; }
    bool dp_single_stream() const { return dp_single_stream_; }
    void set_allreduce_callback(nvsm_allreduce_fn fn, void* user) { ar_fn_ = fn; ar_user_ = user; }

    Profiler prof;
    const nvsm_config& config() const { return cfg_; }
    const Tuning& tune() const { return tune_; }
    // the inverted index of the uploaded corpus (include/cunvsm_amd.h nvsm_corpus_index; ranking.cpp)
    void corpus_index(const nvsm_index_options& opt, nvsm_index_info* info);
    void corpus_index_free();
    void corpus_postings(int64_t word_id, int64_t capacity, int64_t* doc_ids, int32_t* tfs, int64_t* count);
    // its positional layer (include/cunvsm_amd.h nvsm_corpus_index_positions; ranking.cpp)
    void corpus_index_positions(nvsm_positions_info* info);
    void corpus_index_positions_free();
    void corpus_positions(int64_t word_id, int64_t doc_id, int64_t capacity, int64_t* positions, int64_t* count);
    std::string describe(int64_t batch) const;      // which kernel each product of a step takes at `batch` windows, table modes, switches off their defaults

 private:
    struct ParamRef { float* p; int64_t n; };
    ParamRef find_param(const std::string& name);
    struct RowsRef { float* p; int64_t rows, width; };
    RowsRef find_param_rows(const std::string& name, int64_t first_row, int64_t rows);      // throws unless a table's rows, in range
    DevBuf<float> fold_partial_, fold_partial_q_, fold_partial2_, fold_partial2_q_;          // fold.hip's partial sums: allocated by the first fold step
    int fold_current_at_ = -1;            // ents_.updates_done when a fold step last brought the lazily decayed documents table up to date
    void build_csr(TableState& t, const int* keys, int64_t n, hipStream_t s, int64_t n_pair_entries = 0);
    void alloc_table_csr(TableState& t, int64_t max_entries, bool chunk_order);
    Csr csr_of(TableState& t, int64_t n);
    void backward_dx(hipStream_t dx_follower);           // B5, B7, B9 on the main stream; dx_follower (or null): the stream that waits for dx
    void backward_T(hipStream_t s, bool slab_sum_in_update);      // B6 (+ its all-reduce); true: the slab sum is left to the projection update behind it
    void update_entities(float lr, float sl, hipStream_t s, hipEvent_t row_pass_after = nullptr);
    void update_words(float lr, float sl, hipStream_t untouched_stream);      // (kernels.h launch_table_pass untouched_s; null: the main stream)
    void update_transform(float lr, float sl, hipStream_t s);
    void allreduce_f64(double* dev, int64_t n);
    void allreduce_f32(float* dev, int64_t n, hipStream_t s);
    void lazy_refresh(TableState& t, const Csr* touched, hipStream_t s);     // null = every row of the table
    void lazy_flush_all();                 // before anything reads or writes whole tables (get / set_param, averaging)
    LazyView lazy_view(const TableState& t) const;      // what a reader needs to bring the rows it gathers up to date on the fly
    void lazy_scalar_snapshot(TableState& t, const Csr& c, hipStream_t s);   // the touched rows' scalar state, before an update's passes
    void lazy_begin_update(TableState& t, RowPassArgs& a, bool scalar_pingpong);
    void lazy_end_update(TableState& t, const Csr& c, hipStream_t s);
    RowPassArgs final_words_pass_args(float lr, float sl);
    hipEvent_t ev_untouched_ = nullptr;
    void settle_words_stamp();            // the words table's pending stamps, now (see lazy_end_update)
    bool words_stamp_pending_ = false;    // the last words update's stamps have not been set yet
    int64_t words_stamp_n_ = 0;           //   ... entries of that update's CSR
    void raise_device_error();             // throws when a kernel has flagged bad ids / non-finite values since the last check
    void debug_check(const float* x, int64_t n, int which);
    void alloc_table(TableState& t, int64_t rows, int dim, int64_t max_entries);
    float adam_bc(uint64_t t) const;

    // ---- one call's request. Built on the public method's stack and passed down by const reference: nothing a call is asked to do
    // lives in a member, so nothing has to be cleared again when the call returns or throws.
    struct ForwardRequest {
        const nvsm_batch* batch = nullptr;              // the text batch, or
        const nvsm_window_batch* windows = nullptr;     // ... the window references F1 expands into one (neither: the pair objective alone)
        const int64_t* entity_ids = nullptr;
        const nvsm_pair_batch* pairs = nullptr;         // the pair objective rides along (or stands alone)
        const nvsm_mixture* mix = nullptr;              // ... with these shares
        bool term_pairs = false;                        // ... on the words table (pairs of word ids) instead of the documents table
        // what only a fused step knows up front
        hipEvent_t loss_event = nullptr;                // the loss kernel carries it as its completion event
        bool hoist = false;                             // queue the decay of the words rows without entries behind the CSR build,
        float lr = 0.f, sl = 0.f;                       // ... with this learning rate and scaled lambda
        bool text() const { return batch || windows; }
        int64_t num_instances() const { return windows ? windows->num_instances : batch->num_instances; }
        bool on_device() const { return (windows ? windows->on_device : batch->on_device) != 0; }
    };
    // what the stages of one forward pass share: filled by forward() and by the stage that produces the value, never a member
    struct ForwardCall {
        const ForwardRequest& req;
        int64_t B = 0, N = 0, M2 = 0;                   // windows, document ids (B * R), pair ids (2 M) of this rank
        int64_t T2 = 0;                                 // term-pair ids (2 M) behind the word ids (M2 is 0 then)
        bool terms = false;
        int64_t Bu = 0;                                 // windows of the table updates (exact tables: of all ranks)
        bool mixed = false, fused_prologue = false;
        int sort_layout = 0;
        bool any_lazy = false, csr_first = false, words_csr_late = false, pair_on_main = false;
        const int64_t* words_dev = nullptr;             // F1: the word ids in HBM
        const int* csr_ids = nullptr;                   // F2: the ids the CSR builds sort (exact tables: the gathered ones)
        const int* csr_widx = nullptr;
    };
    void forward(const ForwardRequest& req);
    void step(const ForwardRequest& req, float lr, float* cost);
    int64_t step_deferred(const ForwardRequest& req, float lr);
    void finish_unfused(float lr, float* cost);         // compute_gradients; update(scaled lambda); get_cost — behind a forward pass
    void step_transform_tail(float lr, float sl);       // a fused step's dT product and projection update (side stream 2)
    // the stages of forward(), in its order
    void begin_forward(int mode, int64_t B, int64_t M, const nvsm_mixture* mix);      // the preamble (shared with the pairs-only pass)
    void forward_pairs_only(const ForwardRequest& req);
    void stage_inputs(ForwardCall& c);                  // F1
    void stage_ids(ForwardCall& c);                     // F2
    void launch_csr_builds(const ForwardCall& c, hipEvent_t after, int which = 3);
    void forward_product(const ForwardCall& c);         // F3 + F5
    void forward_loss(const ForwardCall& c);            // F6 + the loss launch

    // ---- state carried from one call to the next (everything else a call needs is in its ForwardRequest / ForwardCall)
    //   item                              written by                                      consumed by
    //   words_untouched_hoisted_          launch_csr_builds (a fused step's hoisted pass)  update_words of the same step (skips that pass)
    //   hoisted_lr_, hoisted_sl_          ... with the values the pass was queued with     update_words: other values are NVSM_ERR_STATE
    //   words_untouched_pending_          launch_csr_builds (hoist_untouched == 2)         the next forward(): the main stream follows ev_untouched_
    //   words_untouched_stream_prev_      launch_csr_builds (hoist_untouched == 2)         the next launch_csr_builds: the words CSR stream must not change
    //   words_snapshot_early_             launch_csr_builds (lazy words, scalar state)     update_words: the snapshot is taken already
    //   words_tail_pending_               step (streaming decay on side stream 2)          the next forward_product: join_T in front of the word gather
    //   E_pending_, T_pending_            step (side-stream tails not yet joined)          join_E / join_T; forward_product (which phrase matrix to write)
    //   last_csr_layout_                  forward                                          the next stage_inputs (host-batch copies lean on it)
    // A call that throws half way leaves these as they are, which is what they mean: the *_pending_ flags name work that IS queued, and
    // so does words_untouched_hoisted_ — the next words CSR build resets it. Where a forward pass throws behind its launches and leaves
    // have_forward_ set (NVSM_DEBUG: raise_device_error), compute_gradients; update on that pass skip the decay that is queued already,
    // and another lr / lambda is NVSM_ERR_STATE. (step() used to clear the flag on that path; the decay would then have run twice.)
    bool words_untouched_hoisted_ = false;      // the decay of the words rows without entries is queued behind the CSR build already
    float hoisted_lr_ = 0.f, hoisted_sl_ = 0.f;
    bool words_untouched_pending_ = false;      // ... and not yet followed by the main stream (the next word gather does)
    hipStream_t words_untouched_stream_prev_ = nullptr;      // the stream the hoisted words decay of the last step ran on (hoist_untouched == 2)
    bool words_snapshot_early_ = false;   // this step's words scalar snapshot was taken behind the CSR build
    bool words_tail_pending_ = false;                   // side stream 2 still decays words rows: the next word gather joins it
    bool E_pending_ = false, T_pending_ = false;      // side-stream tails of the last nvsm_step not yet joined
    int last_csr_layout_ = -1;          // the layout of the previous step's builds (host-batch copies lean on it)

    Tuning tune_;                     // the switches of this handle: read from the environment once, by the constructor (tuning.h)
    nvsm_config cfg_;
    int R_;
    hipStream_t stream_ = nullptr;
    bool own_stream_ = false;
    // The batch → CSR builds depend only on the indices, so they run on a side stream concurrently with the
    // forward / backward kernels and are joined right before the row passes.
    hipStream_t aux_stream_ = nullptr;
    hipStream_t aux2_stream_ = nullptr;   // the words CSR build: next to the documents CSR build instead of behind it
    hipStream_t aux3_stream_ = nullptr;   // host-batch copies, then the documents CSR build (NVSM_SORT_LAYOUT 4)
    hipEvent_t ev_csr_ents_ = nullptr;
    hipEvent_t ev_inputs_ = nullptr, ev_csr_ = nullptr;
    // fused step(): the documents update (HBM bound) and the dT GEMM (MFMA bound) run on the side stream next to the
    // dx GEMM and the words update on the main stream
    hipEvent_t ev_gathered_ = nullptr;
    hipEvent_t ev_loss_ = nullptr, ev_dx_ = nullptr, ev_bwdx_ = nullptr, ev_E_done_ = nullptr, ev_T_done_ = nullptr, ev_words_late_ = nullptr;
    hipEvent_t ev_cost_ready_ = nullptr, ev_cost_copied_ = nullptr;      // step(cost): the loss word copied out behind the loss kernel
    double* cost_host_ = nullptr;                                         // ... into this page-locked word
    hipStream_t words_csr_stream_ = nullptr;            // the side stream that built this step's words CSR (NVSM_SORT_LAYOUT)
    std::minstd_rand0 rng_;           // include/cuNVSM/base.h:36
    uint64_t device_seed_ = 1, step_count_ = 0;

    TableState words_, ents_;
    DevBuf<float> T_, b_, s0T_, s0b_, s1T_, s1b_;
    uint64_t t_transform_ = 1;

    // per-step inputs
    DevBuf<int64_t> in_words_[2], in_labels_[2], in_ids64_;      // host batches: two staging sets (see compute_cost)
    DevBuf<float> in_wwts_[2], in_instw_[2];
    int in_parity_ = 0;
    hipStream_t copy_stream_ = nullptr;   // alias of aux3_stream_
    hipEvent_t ev_copied_ = nullptr, ev_step_begin_[2] = {nullptr, nullptr};
    bool copied_recorded_ = false, last_batch_on_host_ = false;
    DevBuf<int> widx_, ids_buf_[2];
    int* ids_p_ = nullptr;            // this step's document ids: the two buffers alternate, so that a step's prologue never
                                      //   rewrites the ids the previous step's documents CSR build may still be reading
    const float* wwts_ = nullptr;     // device pointer or null
    const float* instw_ = nullptr;
    const int64_t* labels_dev_ = nullptr;
    std::vector<int64_t> host_labels_;
    // host sampler: two page-locked id buffers, each guarded by the event of the copy that last read it, so that
    // compute_cost never waits for the stream (the step before last has long released the buffer it reuses)
    int64_t* host_ids_pin_[2] = {nullptr, nullptr};
    hipEvent_t ev_host_ids_[2] = {nullptr, nullptr};
    bool host_ids_used_[2] = {false, false};
    int host_ids_parity_ = 0;
    int* err_host_ = nullptr;         // page-locked error word written by kernels (kernels.h: NVSM_BAD_*, NVSM_NONFINITE_BASE)
    bool debug_ = false;              // NVSM_DEBUG=1: finite checks of every intermediate + a sync after each call
    int64_t B_ = 0;                   // instances of the current batch (this rank)

    // intermediates
    DevBuf<float> phrase_raw_, phrase_norms_, ge_msq_;      // optional L2 normalisers: cached raw phrase means + norms; per-entry mean of squares
    DevBuf<float> phrase_alt_;            // second phrase matrix (see compute_cost)
    float* phrase_p_ = nullptr;           // the one the current forward result lives in
    DevBuf<float> phrase_, pre_, proj_, dy_, gphrase_, coef_, probs_, pp_, msq_w_, msq_parts_, U_, scale_w_, grad_entity_;
    DevBuf<double> stats_;                   // [2 de | 1 + 2 de] = Σx Σx² | loss Σdy Σdy·x̂ — written by the ordered grid sums
    // workspaces of those sums (kernels.h GridSumWs): projection GEMM epilogue / loss kernel
    struct SumsBufs { DevBuf<double> part; DevBuf<double> part2; DevBuf<int> arrive; GridSumWs ws{}; };
    SumsBufs sums_fwd_, sums_bwd_;
    // the projection matrix cut into bf16 planes for the split-bf16 GEMM (gemm_split.hip), in the forward and the backward
    // product's layout; `ready` is cleared by everything that writes T
    DevBuf<char> planes_fwd_, planes_bwd_, rplanes_fwd_, rplanes_bwd_;
    int pending_slabs_ = 0;              // backward_T left the slab sum to the projection update behind it: that many slabs in gT_partial_
    void planes_stale();                 // T changed: every set of planes is out of date
    GemmSplitWs split_fwd_{}, split_bwd_{};
    void cut_transform_planes(hipStream_t strm);
    bool dt_on_main() const;
    bool dt_on_main_at(int64_t B) const;
    bool use_dt_at(int64_t B) const;
    bool use_dtw_at(int64_t B) const;    // ... on the wave-sized kernel (gemm_dtw.hip: per-rank batches)
    int csr_stream_layout() const;
    bool slab_sum_fusable() const;     // the projection update's own slab sum is launch_splitk_reduce's (vector order, alignment)
    bool dp_fold() const;              // data parallel: [db | loss] ride on the dT all-reduce (one collective per step)
    bool gather_fused_at(int64_t B) const;      // the forward product at this batch size forms the phrase rows itself
    void alloc_sums(SumsBufs& b, int colgroups, int contrib_cap, int width_cap);
    bool csr_joined_words_ = true, csr_joined_ents_ = true;      // the main stream is behind the current CSR builds
    double* stats_fwd_ = nullptr;
    double* stats_bwd_ = nullptr;
    DevBuf<float> bn_mean_, bn_inv_std_, dbeta_, dgamma_;
    DevBuf<float> gT_, gb_, gT_partial_;
    int gemm_slabs_want_ = 128;        // split-K slabs of the exact-fp32 dT product (shapes / settings gemm_dt.hip does not cover)
    bool dt_ok_ = false;               // the split-K dT kernel (gemm_dt.hip) covers this model's shapes
    int num_cus_ = 256;
    bool table_decays_lazily(bool documents, int64_t rows, int dim, int64_t max_entries) const;
    static constexpr int kDtwSlabs = 12;                    // split-K slabs of the wave-sized dT kernel (gemm_dtw.hip; backward_T)
    static constexpr int64_t kDtMainMinBatch = 16384;      // eager tables, one rank: the dT product on the split-bf16 kernel, on the main stream, from here
    int chunk_entries(const TableState& t, int64_t n) const;      // entries per level-1 chunk of a long row for a batch of n entries of table t
    bool use_dt() const;               // this step's dT product runs on it (else: the exact-fp32 tiled / panel kernels)

    // ---- entity-entity pairs (pairs.hip). The pair entries ride in the documents table's ONE sorted pass: the 2M gradient source
    // rows sit behind the text objective's in proj_ (rows B .. B + 2M - 1), pair entry i carries the entry id (B + i) * R — so the
    // pass's src = entry / R finds its row, coef_[entry] its coefficient, pp_[src] its mean of squares — and the CSR is built from the
    // step's B * R document ids followed by the 2M pair ids. Everything here is allocated by the first pair call.
    enum { MODE_TEXT = 0, MODE_PAIRS = 1, MODE_MIXED = 2 };
    int mode_ = MODE_TEXT;                      // what the current forward result is
    int64_t M_ = 0;                             // its pairs
    float text_scale_ = 1.f, pair_scale_ = 1.f; // w / (w_te + w_ee) (MergeGradientsFn, cpp/intermediate_results.cu:19-38): set by begin_forward
    bool pairs_ready_ = false;
    DevBuf<int64_t> pair_ids64_;
    DevBuf<float> pair_w_, pair_probs_, pair_mults_, instw_scaled_;
    DevBuf<int> pair_vals_[2];                  // entry ids of the merged CSR, one per set of CSR arrays
    DevBuf<double> pair_loss_;
    const float* pair_wdev_ = nullptr;
    SumsBufs sums_pair_;
    hipEvent_t ev_pair_ = nullptr, ev_pair_copied_ = nullptr;
    hipStream_t pair_stream_ = nullptr;         // the stream the last pair kernel ran on
    bool pair_pending_ = false;                 // ... which the main stream has not followed yet
    bool pair_copy_pending_ = false;
    double pair_cost_ = 0.0, text_cost_ = 0.0;
    void check_pair_request(const nvsm_batch* text, const nvsm_pair_batch& pairs, const nvsm_mixture* mix) const;
    void ensure_pair_workspace();
    // ids narrowed into ids_dst, weights on the device (main stream); ids outside [0, limit) become row 0 and flag `code`
    void stage_pairs(const nvsm_pair_batch& pairs, int* ids_dst, int64_t limit, int code);
    void launch_pairs(hipStream_t s, hipEvent_t after);                // the pair kernel of the current forward result
    int64_t ents_entries(int64_t text_windows) const { return text_windows * R_ + (mode_ != MODE_TEXT && pair_table_ == 0 ? 2 * M_ : 0); }
    float scaled_lambda_for(int mode, int64_t B, int64_t M) const;

    // ---- term-term pairs (pairs.hip, the words-table form). The pair entries ride in the words table's sorted passes:
    // the 2M MULTIPLIED gradient rows sit behind the text objective's in gphrase_ (rows B .. B + 2M - 1), their means of squares at
    // msq_w_[B + i], pair entry i carries the entry id (B + i) * w and weighs 1, and the words CSR is built from the step's B * w word
    // ids followed by the 2M pair ids (widx_). The pair objective alone: entries = 2M, div = 1, widx_ = the pair ids. With feature
    // weights the B * w weights are copied into wts_ext_ ((B + 2M) * w floats) and slot (B + i) * w is 1. Allocated by the first
    // term-pair call (ensure_term_workspace), beyond what a handle without one holds:
    //   gphrase_ +2Mx·d_w floats, msq_w_ +2Mx, widx_ +2Mx ints, term_vals_ B·w + 2Mx ints, wts_ext_ (B + 2Mx)·w floats, the words CSR
    //   workspace again for B·w + 2Mx entries, U_ / scale_w_ (sparse Adam / Adagrad) for max(B, 2Mx) source rows, sums_term_, and — unless
    //   an entity-pair call made them — pair_ids64_ 2Mx int64, pair_w_ / pair_probs_ / pair_mults_ Mx floats, instw_scaled_ B floats
    // with B = Mx = max_batch_size.
    int pair_table_ = 0;                        // the current forward result's pairs are 0: document pairs, 1: term pairs
    bool terms_ready_ = false;
    DevBuf<int> term_vals_;                     // entry ids of the merged words CSR
    DevBuf<float> wts_ext_;
    SumsBufs sums_term_;
    void check_term_request(const nvsm_batch* text, const nvsm_pair_batch& pairs, const nvsm_mixture* mix) const;
    void ensure_term_workspace();
    void launch_term_pairs();                   // the words-table pair kernel of the current forward result, on the main stream
    void forward_terms_only(const ForwardRequest& req);
    bool term_result() const { return mode_ != MODE_TEXT && pair_table_ == 1; }
    // entries of the words update of the current forward result for `text_windows` windows
    int64_t words_entries(int64_t text_windows) const { return text_windows * cfg_.window_size + (term_result() ? 2 * M_ : 0); }

    // ---- window references (corpus.hip). The corpus lives in HBM from nvsm_corpus_upload on; a *_windows call is compute_cost / step
    // on a batch that window_expand_kernel writes into a host batch's staging set (compute_cost F1). Everything here is allocated by
    // the upload.
    struct Corpus {
        DevBuf<int> tokens;                 // at least one element
        DevBuf<int64_t> offsets;            // at least two
        DevBuf<float> doc_weights, term_weights;      // empty: none
        std::vector<int64_t> host_offsets;  // host sampler: which references are bad (their label is 0, as on the device)
        int64_t num_tokens = 0, num_documents = 0;
        bool with_doc_weights = false, with_term_weights = false;
        size_t bytes = 0;
        std::vector<int64_t> cf;            // lexical ranking: occurrences of every word, made by the first lexical call (empty: not yet)
        std::vector<int64_t> df;            // TF-IDF: documents holding every word, made by the first call that needs it (empty: not yet)
        // the inverted index (index.hip), made by nvsm_corpus_index and dropped with the corpus: post_off [V + 1],
        // post_doc / post_tf [P] (at least one element)
        bool indexed = false;
        int index_use = 0;                  // NVSM_INDEX_*
        DevBuf<int64_t> post_off;
        DevBuf<int> post_doc, post_tf;
        std::vector<int64_t> host_post_off; // post_off on the host: df, and the bounds nvsm_corpus_postings copies between
        int64_t num_postings = 0, index_bytes = 0, max_df = 0;
        // the positional layer of the index, made by nvsm_corpus_index_positions and dropped with the index:
        // post_first [P + 1], a posting's first entry of pos [N] (at least one element), its in-document offsets, ascending
        bool positional = false;
        DevBuf<int> post_first, pos;
        int64_t positions_bytes = 0;
    };
    Corpus* corpus_ = nullptr;
    DevBuf<uint32_t> in_refs_[2];               // host references, one per staging set
    std::vector<uint32_t> host_refs_;           // host sampler: device references read back
    void check_window_request(const nvsm_window_batch& wb) const;

    // ranking scratch: allocated by the first infer / rank call (training-only handles never pay for it), grown on demand
    struct RankScratch {
        DevBuf<int64_t> ids, offsets, cand_off, out_ids, out_counts;
        DevBuf<float> wts, phrase, proj, qinv, scores, out_scores;
        DevBuf<int> cand;
        DevBuf<unsigned long long> keys;
        DevBuf<char> sel_ws;
        DevBuf<float> panel, pslab, pair_out;      // neighbours: the query panel [round][dim], one slab of the projected vocabulary
        DevBuf<int64_t> self;                      //             ... the queries' own rows (exclude_self)
        DevBuf<float> ngram_g;                     // n-grams: G [m][de] = T·W[S] of the call,
        DevBuf<int64_t> ngram_vocab;               //          ... and S on the device
        DevBuf<int> jids, jgrades;                 // evaluate: the call's judged ids (ascending per query) and grades,
        DevBuf<int64_t> joff;                      //           ... their offsets,
        DevBuf<double> jconst, metrics;            //           ... R / idcg / idcg@c per query, and the metric rows
        DevBuf<int> lex_slot_of, lex_terms, lex_qoff, lex_tslot;      // lexical: term -> slot [num_words] (-1 between rounds), a round's terms
        DevBuf<double> lex_c0, lex_base, lex_weight;                  //          ... and their constants (lex_weight: weighted queries only)
        DevBuf<int> sdm_ent_off, sdm_ent_other, sdm_ent_pair, sdm_goff, sdm_index;      // sequential dependence: a round's pair entries by slot, its groups
        DevBuf<double> sdm_c0, sdm_base, sdm_coef;                    //          ... their members' constants, every query's group coefficients
        DevBuf<unsigned long long> sdm_cf;                            //          ... and the round's collection counts [2][kSdmPairs]
        DevBuf<int> post_query, post_first;                           // postings fill (indexed corpora only): an entry's query, first-of-its-term flag
        DevBuf<int64_t> post_lo, post_hi;                             //          ... and a term's postings inside the slab
        DevBuf<int> sdm_pair_a, sdm_pair_b;                           // SDM from positional postings: a round's pairs as slots
        DevBuf<double> rm_acc, rm_sum;                                // relevance model: acc [round][num_words] and cnt likewise (zero between
        DevBuf<int> rm_cnt, rm_ids, rm_counts;                        //   rounds), Σω [round], a round's feedback lists [round][fb_docs]
        DevBuf<float> rm_scores;
        DevBuf<int64_t> fuse_ids, fuse_counts, fuse_out_ids, fuse_out_counts;      // ensemble: both lists of a round [2][round][k], the fused list
        DevBuf<float> fuse_scores, fuse_out_scores;
        DevBuf<float> fuse_alpha, sweep_alphas;    // supervised fusion: a round's per-query alphas; the call's grid
        DevBuf<double> sweep_table;                //                    ... and its metric table [alphas][queries][width]
    };
    RankScratch rank_;
    TsneScratch tsne_;      // allocated by the first nvsm_tsne, grown by a later call with more rows
    TsneSparseScratch tsne_sparse_;      // likewise for nvsm_tsne_sparse
    void tsne_check(const nvsm_tsne_options& opt, int64_t max_rows, const char* too_many, int64_t* n_out) const;      // the refusals both calls share
    KmeansScratch kmeans_;  // likewise for nvsm_kmeans
    int64_t score_floats() const { return static_cast<int64_t>(tune_.rank_slab_mb) << 18; }      // the score slab: 256 MB unless NVSM_RANK_SLAB_MB says otherwise
    // one round behind its layout (ranking.cpp): scratch, the slabs through the caller's fill step, sort + the caller's write, results
    void round_grow(const RankLayout& l, int k);
    template <typename Fill> void round_slabs(const RankLayout& l, int64_t rows, int k, Fill fill);
    template <typename Write> void round_sort(const RankLayout& l, Write write);
    void round_results(int64_t q0, int64_t qn, int k, int64_t* ids, float* scores, int64_t* counts);      // null pointers are not copied to
    void rank_check(const nvsm_queries& q, const nvsm_rank_options& opt);      // the refusals of nvsm_infer, before anything runs
    struct EvalPlan;                        // evaluate: the judgments as the kernel reads them (ranking.cpp)
    void eval_plan(EvalPlan& p, int64_t Q) const;                                 // checks, sorts, R / idcg / idcg@c
    EvalArgs eval_upload(const EvalPlan& p, int64_t Q, int width);                // ... on the device; width: the length of the ranked lists
    // the rounds of rank and evaluate (ev null: rank); null result pointers are not copied to
    void rank_rounds(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t* doc_ids, float* scores, int64_t* counts, EvalPlan* ev);
    void lexical_check(const nvsm_queries& q, const nvsm_lexical_options& lex) const;      // the refusals of nvsm_lexical_rank, before anything runs
    // weights null: nvsm_lexical_rank's rounds; given ([offsets[num_queries]] floats next to word_ids): the weighted scorer
    // tfidf given: nvsm_tfidf_rank's scorer at lex.top_k (lex's method and param are not looked at). hand given: the round's retrieved
    // ids go, ascending, where the candidate scan reads them (nvsm_rerank); counts must then be given
    struct TfidfPlan { double k1, b, avgdl; int idf; };
    struct Handover;                        // the candidate arrays of nvsm_rerank while the first stage fills them (ranking.cpp)
    void lexical_rounds(const nvsm_queries& q, const nvsm_lexical_options& lex, const float* weights, int64_t* doc_ids, float* scores, int64_t* counts,
                        const TfidfPlan* tfidf = nullptr, Handover* hand = nullptr);
    void tfidf_check(const nvsm_queries& q, const nvsm_tfidf_options& opt) const;          // the refusals of nvsm_tfidf_rank, before anything runs
    TfidfPlan tfidf_plan(const nvsm_tfidf_options& opt) const;
    void corpus_cf();                       // the cf table of the corpus, made once (lex_cf_kernel)
    void corpus_df();                       // the df table of the corpus, made once (lex_df_kernel)
    // the refusals of the sequential-dependence calls that are their own (behind lexical_check where there is a ranking), and their
    // rounds: lex null: the pair counts alone into ordered / unordered; given: the ranking (ordered / unordered may still be given)
    void sdm_check(const nvsm_queries& q, const nvsm_sdm_options& sdm) const;
    void sdm_rounds(const nvsm_queries& q, const nvsm_lexical_options* lex, const nvsm_sdm_options& sdm, int64_t* doc_ids, float* scores,
                    int64_t* counts, uint64_t* ordered, uint64_t* unordered);
    void index_build(Corpus& c);            // the postings of the corpus and, where still empty, its cf and df (ranking.cpp; index.hip)
    void positions_build(Corpus& c);        // the positional layer of an indexed corpus (ranking.cpp; index.hip)
    // one round of nvsm_rank over candidate lists that lie on the device as launch_rank_scan_candidates reads them
    void rank_candidates_round(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t q0, const RankLayout& l, const int* cand,
                               const int64_t* cand_off, EvalArgs* ea, int64_t* doc_ids, float* scores, int64_t* counts);
    // a query without words retrieves nothing: its result rows blanked, its metric row zero (metrics null: none)
    void blank_wordless(const nvsm_queries& q, int k, int64_t* doc_ids, float* scores, int64_t* counts, double* metrics, int width) const;
    void weights_check(const nvsm_queries& q) const;
    void feedback_check(const nvsm_feedback_options& fb) const;                   // behind lexical_check: the corpus is there
    // first pass + relevance model into host lists [Q][fb_terms] (the rounds of nvsm_relevance_model, behind its checks and rank_join)
    void relevance_rounds(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, int64_t* term_ids,
                          float* term_probs, int64_t* counts);
    struct ExpandedQueries;                 // the RM3 queries of a call, built on the host in fp64 (ranking.cpp)
    void expand_queries(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, ExpandedQueries& out);
    void ensemble_rounds(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                         const nvsm_ensemble_options& ens, const nvsm_judgments* j, double* metrics, int64_t* doc_ids, float* scores,
                         int64_t* counts, const nvsm_sdm_options* sdm = nullptr);      // sdm given (fb null): list B is nvsm_sdm_rank's
    // what the fused calls share (ranking.cpp): the refusals of nvsm_rank_ensemble(_prf) for every alpha of the call, both rankings
    // once, a round's lists on the device, and the fusion of the call's queries at one alpha or at one alpha per query
    struct EnsembleLists;
    void ensemble_check(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                        int normalizer, const float* alphas, int64_t num_alphas, const nvsm_sdm_options* sdm = nullptr);
    void ensemble_lists(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                        EnsembleLists& l, const nvsm_sdm_options* sdm = nullptr);
    FuseArgs ensemble_upload(const EnsembleLists& l, int64_t q0, int64_t qn, int normalizer);
    void fuse_rounds(const nvsm_queries& q, const EnsembleLists& l, int normalizer, float alpha, const float* query_alpha, const EvalPlan* plan,
                     int64_t* doc_ids, float* scores, int64_t* counts);
    void sweep_check(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                     const nvsm_sweep_options& sw, const nvsm_judgments& j, double* table, EvalPlan& plan);
    void sweep_rounds(const nvsm_queries& q, const EnsembleLists& l, const nvsm_sweep_options& sw, const EvalPlan& plan, double* table);
    void rank_join();                       // the handle's four streams waited for on the host; the words table's pending stamps settled
    struct RowSpace { const float* rows; int64_t count; int dim; const TableState* table; };      // rows null: the projected vocabulary
    RowSpace row_space(int space) const;
    void project_words(const int64_t* ids_dev, int64_t first, int64_t n, float c, int act, float* out);      // out [n][de] = f(T·W[id] + c·b)
    void neighbor_queries_check(const nvsm_neighbor_queries& q, int dim) const;      // the query refusals nvsm_neighbors and nvsm_ngram_search share
    void neighbor_panel(const nvsm_neighbor_queries& q, int64_t q0, int64_t qn, int dim, float c, int act, int cosine);      // rank_.panel, rank_.qinv of a round
    void rank_project(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t q0, int64_t qn);      // rank_.proj [qn][de], on the main stream

    bool have_forward_ = false, have_grads_ = false;
    struct DeferredCost { double* host = nullptr; hipEvent_t ev = nullptr; double batch = 1.0; int64_t ticket = -1; };
    DeferredCost deferred_[NVSM_MAX_DEFERRED];
    int64_t next_ticket_ = 0;
    bool inputs_recorded_ = false;
    double cost_ = 0.0;
    bool cost_valid_ = false;
    bool loss_reduced_ = false;       // data parallel: the loss word has been all-reduced (by the backward pass)

    // data parallel
    RcclApi* rccl_ = nullptr;
    void* comm_ = nullptr;
    int comm_ranks_ = 0;              // ncclCommCount of the communicator (0 = none)
    // the step's three collectives: on two event-ordered streams (dT all-reduce + projection update on side stream 2, next to
    // the words update) or all on the main stream — NVSM_DP_T_ON_MAIN=1, or chosen by comm_init when the communicator does not
    // return the right sums with the two-stream order
    bool dp_single_stream_ = false;
    bool comm_order_check(bool two_streams);      // all-reduces of known values in the step's order; every rank gets the same verdict
    DevBuf<double> loss_tmp_;         // data parallel get_cost before compute_gradients: all-reduced copy of the loss word
    DevBuf<double> loss_red_;         // ... with the folded collective (dp_fold): the summed loss word, written behind the dT all-reduce
    bool loss_folded_ = false;        //     this step's summed loss is in loss_red_, final on loss_stream_
    hipStream_t loss_stream_ = nullptr;
    nvsm_allreduce_fn ar_fn_ = nullptr;
    void* ar_user_ = nullptr;
    std::vector<double> ar_host_;

    // Data parallel with exact tables (nvsm_config.dp_exact_tables): what the table updates read — ids, projected phrases,
    // multipliers, phrase gradients — of ALL ranks, rank-major, all-gathered on the main stream; the CSR builds and the table
    // passes then run on world_size x B windows, i.e. every rank performs the single-GPU update of the global batch.
    bool exact_ = false;
    struct UpdateInputs {
        const float* proj; const float* coef; const float* pp; const int* ids; const float* gphrase; const float* wwts;
        const float* msq_w; const int* widx; int64_t B;
    };
    UpdateInputs update_inputs() const;      // the rank's own buffers, or the gathered ones
    DevBuf<int> xg_ids_[2], xg_widx_;
    int* xg_ids_p_ = nullptr;                // alternates like ids_p_
    DevBuf<float> xg_proj_, xg_coef_, xg_pp_, xg_gphrase_, xg_msq_w_, xg_wwts_;
    void allgather(const void* send, void* recv, size_t bytes, hipStream_t s);      // recv: world_size x bytes, rank-major
    void gather_update_inputs();
};

// The k-fold choice of nvsm_rank_ensemble_cv (ranking.cpp): a pure host function of the sweep table [A][Q][width]. Per fold f the
// alpha whose column `measure`, averaged over the queries with fold_of[q] != f (added in ascending q, divided once), is largest, on
// a tie the largest alpha; fold_index[f] its position in `alphas`. A fold nobody is in: (NaN, 0, -1).
void cv_select(const double* table, int64_t A, int64_t Q, int width, int measure, const float* alphas, const int32_t* fold_of, int F,
               float* fold_alpha, double* fold_train, int* fold_index);

}  // namespace cunvsm
