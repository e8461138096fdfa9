/*
 * cunvsm_amd — C ABI of the MI355X-native NVSM / LSE training hot path.
 *
 * Drop-in boundary for cuNVSM's `Model<TextEntity::Objective>` (include/cuNVSM/model.h:75-131):
 * the per-batch compute_cost → compute_gradients → update → get_cost sequence driven by
 * iterate_data (cpp/main.cu:400-444) and ModelTest::train (include/cuNVSM/tests_base_cuda.h:161-190).
 * Plain pointers and sizes only; the library owns every device-side object, the caller owns its
 * host buffers; nothing but the opaque handle crosses the boundary. Every entry point returns an
 * nvsm_status (0 = OK) instead of aborting (the reference CHECK()s / LOG(FATAL)s).
 *
 * Layouts are the reference's raw buffers:
 *   embedding tables   [num_objects][dim] row-major  (device_matrix dim x n, column-major)
 *   projection         entity_dim x word_dim column-major: T[r + entity_dim * c]
 *   bias               [entity_dim]
 *   indices            int64 (include/cuNVSM/base.h:28  `typedef long int32`)
 *   floating point     float32 (release build, cpp/CMakeLists.txt:17)
 */
#ifndef CUNVSM_AMD_H
#define CUNVSM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nvsm_model nvsm_model;

typedef enum {
    NVSM_OK = 0,
    NVSM_ERR_INVALID_ARGUMENT = 1,
    NVSM_ERR_UNSUPPORTED = 2,      /* configuration outside the kernels' limits (entity_repr_size > 1024, the reference's own limit) */
    NVSM_ERR_DEVICE = 3,           /* HIP / RCCL error, see nvsm_last_error() */
    NVSM_ERR_STATE = 4,            /* call sequence violated (e.g. compute_gradients before compute_cost) */
    NVSM_ERR_NO_DEVICE = 5         /* no MI355X visible: there is NO CPU fallback */
} nvsm_status;

/* proto/nvsm.proto:11-14 (ModelDesc.TransformDesc.Nonlinearity) */
enum { NVSM_TANH = 0, NVSM_HARD_TANH = 1 };
/* proto/nvsm.proto:40-44 (TrainConfig.UpdateMethod) */
enum { NVSM_SGD = 0, NVSM_ADAGRAD = 1, NVSM_ADAM = 2 };
/* proto/nvsm.proto:50-55 (AdamConf.AdamMode); NONE behaves as SPARSE (cpp/updates_adam.cu:289,332) */
enum { NVSM_ADAM_NONE = 0, NVSM_ADAM_SPARSE = 1, NVSM_ADAM_DENSE_UPDATE = 2, NVSM_ADAM_DENSE_UPDATE_DENSE_VARIANCE = 3 };
/* negative sampling: F2, cpp/objective.cu:5-28 → cpp/labels.cu:4-22 */
enum {
    NVSM_SAMPLER_HOST_MINSTD = 0,  /* std::minstd_rand0 + fresh uniform_int_distribution<long> per draw: draw-for-draw the reference */
    NVSM_SAMPLER_DEVICE = 1        /* counter-based hash on the GPU, same distribution (uniform over all documents) */
};

/*
 * Replaces the constructor arguments Model(num_words, num_entities, ModelDesc, TrainConfig)
 * (cpp/model.cu:95-103); field names follow proto/nvsm.proto:7-71.
 */
typedef struct {
    int64_t num_words;
    int64_t num_entities;
    /* ModelDesc */
    int32_t word_repr_size;
    int32_t entity_repr_size;
    int32_t batch_normalization;       /* transform_desc.batch_normalization */
    int32_t nonlinearity;              /* transform_desc.nonlinearity */
    int32_t clip_sigmoid;              /* forced true by the reference CLI (cpp/main.cu:645) */
    int32_t bias_negative_samples;
    int32_t l2_normalize_phrase_reprs; /* objective.cu:99-103,136-142,461-468: optional; separate normaliser passes */
    int32_t l2_normalize_entity_reprs; /* objective.cu:104-107,168-174,405-412: optional; generic loss kernel, gradient rows materialised */
    /* TrainConfig */
    int32_t window_size;
    int32_t num_random_entities;
    float   regularization_lambda;
    int32_t update_method;
    int32_t adam_mode;
    int32_t max_batch_size;            /* TrainConfig.batch_size: capacity of the per-step device buffers (per rank) */
    /* runtime */
    int32_t device;                    /* HIP device ordinal */
    int32_t sampler;                   /* NVSM_SAMPLER_* */
    /* data parallelism (new). world_size 1 = single GPU. */
    int32_t world_size;
    int32_t rank;
    int32_t sync_batch_norm;           /* 1: global batch statistics (exact single-GPU maths); 0: per-shard */
    int32_t dp_exact_tables;           /* world_size > 1 — 0: embedding tables are updated from the rank's own windows (replicas drift);
                                          1: every rank applies the sparse gradients of ALL ranks' windows (all-gather of the update's
                                          inputs in front of the table passes): replicas stay bit-identical and follow the single-GPU
                                          trajectory on the global batch, at world_size x the table-update work per rank (see below) */
    int32_t reserved[4];
} nvsm_config;

/* Fills the reference CLI defaults (cpp/main.cu:15-76,637-721; scripts/functions.sh:380-399). */
void nvsm_config_default(nvsm_config* cfg);

/*
 * Replaces TextEntity::Batch (include/cuNVSM/data.h:114-177, cpp/data.cu:8-124): four flat arrays.
 * on_device = 0: host pointers (the reference's pinned-host batch). Page-locked arrays (nvsm_host_alloc, hipHostMalloc,
 *                hipHostRegister) are read over PCIe by a kernel on the engine's copy stream, a step ahead of their use, and
 *                the call never holds the calling thread; pageable arrays are staged by hipMemcpyAsync, which does;
 * on_device = 1: device pointers already resident in HBM (no copy).
 */
typedef struct {
    const int64_t* features;          /* [num_instances * window_size] word ids */
    const float*   feature_weights;   /* [num_instances * window_size] or NULL (= all 1.0) */
    const int64_t* labels;            /* [num_instances] document ids */
    const float*   weights;           /* [num_instances] or NULL (= all 1.0) */
    int64_t        num_instances;
    int32_t        on_device;
} nvsm_batch;

const char* nvsm_last_error(void);
const char* nvsm_version(void);
/* number of visible HIP devices (0 ⇒ nvsm_create fails with NVSM_ERR_NO_DEVICE) */
int nvsm_device_count(void);

/* Bind the CALLING host thread (and the threads it creates afterwards) to the CPUs of the NUMA node the device hangs off
 * (/sys/bus/pci/devices/<bus id>/local_cpulist, intersected with the thread's present affinity mask; left as it is when the
 * intersection is empty or the node is unknown). The steps of a small batch are a chain of ~45 launches and event calls per
 * 0.15 ms: queued from the far socket they take the host LONGER than they take the GPU (LSE recipe, batch 4096, two-socket
 * host: 0.159 ms per step unbound or on the far node, 0.150 on the device's node). The reference has no counterpart (one
 * GPU, one thread, cpp/main.cu:623-767); the trainer and bench.py call it once per process, right after choosing the device.
 * Call it BEFORE the first HIP call of the process where possible: the device is then found through sysfs (the AMD render nodes the
 * process may open, in order; nvsm_create re-checks the guess against hipDeviceGetPCIBusId and re-binds if it was wrong), and the
 * runtime's own threads and host allocations land on the device's node as well (LSE: 0.1495 ms in every process against
 * 0.150-0.162 when bound after the runtime came up). Where sysfs does not identify the device the runtime is asked (and comes up).
 * *numa_node (may be null): the device's node, -1 if unknown. NVSM_BIND_HOST=0 in the environment makes it a no-op. */
int nvsm_bind_host_thread(int device, int* numa_node);

/* Model::Model (cpp/model.cu:95-103) / ~Model */
int nvsm_create(const nvsm_config* cfg, nvsm_model** out);
void nvsm_destroy(nvsm_model* m);

/* ModelBase::initialize(RNG*) (cpp/model.cu:37-43): Glorot-uniform words → entities → transform, bias = 0,
 * drawn from std::minstd_rand0(seed) exactly as include/cuNVSM/cuda_utils.h:35-56; the same generator then
 * feeds the host negative sampler (as `rng` does in cpp/main.cu:729-730,405). */
int nvsm_initialize(nvsm_model* m, uint64_t seed);
int nvsm_rng_get_state(nvsm_model* m, uint64_t* state);   /* `rng_state << *rng`  (cpp/main.cu:401-402) */
int nvsm_rng_set_state(nvsm_model* m, uint64_t state);
/* model.initialize(&rng) with a generator that has ALREADY been consumed: the reference seeds one RNG in main()
 * (cpp/main.cu:729-730), lets the data source draw from it first (document shuffling, cpp/main.cu:497-499) and only
 * then initialises the parameters (cpp/main.cu:520). The caller installs that state with nvsm_rng_set_state and
 * calls this instead of nvsm_initialize(seed). */
int nvsm_initialize_from_rng_state(nvsm_model* m);

/* Pinned host memory for batches handed over with on_device = 0 — what TextEntity::Batch allocates with
 * cudaHostAlloc (cpp/data.cu:16-27), so that bringing a batch into HBM is truly asynchronous (see nvsm_batch). */
int nvsm_host_alloc(size_t bytes, void** out);
int nvsm_host_free(void* p);

/* ModelBase::get_data() (cpp/model.cu:64-93) — the four tensors write_to_hdf5 dumps. Names:
 *   "word_representations-representations"   [num_words][word_repr_size]
 *   "entity_representations-representations" [num_entities][entity_repr_size]
 *   "word_entity_mapping-transform"          entity_repr_size x word_repr_size, column-major
 *   "word_entity_mapping-bias"               [entity_repr_size]
 * nvsm_set_param is the test hook that replaces Storage::increment_parameter / initialize_with_constant
 * (cpp/storage.cu:108-131,252-264). Optimiser state is reachable under "<param>/m", "<param>/v", "<param>/a". */
int nvsm_param_size(nvsm_model* m, const char* name, int64_t* count);
int nvsm_get_param(nvsm_model* m, const char* name, float* host_dst, int64_t count);
int nvsm_set_param(nvsm_model* m, const char* name, const float* host_src, int64_t count);
/* Storage::increment_parameter(idx, epsilon) (cpp/storage.cu:123-131,252-264): the gradient checker's poke. */
int nvsm_increment_parameter(nvsm_model* m, const char* name, int64_t index, float delta);

/* Index contract (the reference indexes its tables with these ids unchecked, cpp/params.cu:75-95, cpp/storage.cu:37-49):
 * every word id must be in [0, num_words), every label / entity id in [0, num_entities). The arrays must hold
 * num_instances * window_size (features, feature_weights), num_instances (labels, weights) and
 * num_instances * (num_random_entities + 1) (entity_ids) elements. Ids are checked ON THE DEVICE when they are narrowed
 * to 32 bits: an id out of range is replaced by row 0 (nothing is ever read or written out of bounds) and the NEXT
 * host-side wait of the handle — nvsm_get_cost, nvsm_deferred_cost, nvsm_synchronize, nvsm_get_param / nvsm_get_tensor —
 * returns NVSM_ERR_INVALID_ARGUMENT once; the numbers of that step are meaningless. With the environment variable
 * NVSM_DEBUG=1 (the reference's debug build: CHECK_MATRIX, cpp/objective.cu:134,152) compute_cost / compute_gradients
 * additionally verify that every intermediate and parameter is finite and report at once (NVSM_ERR_DEVICE). */
/* Model::compute_cost(batch, rng) (cpp/model.cu:135-143 → cpp/objective.cu:30-313).
 * entity_ids: optional [num_instances * (num_random_entities + 1)] int64 HOST array laid out as
 * generate_labels does ([label, neg_1..neg_k] per instance); NULL ⇒ sampled per cfg.sampler. */
int nvsm_compute_cost(nvsm_model* m, const nvsm_batch* batch, const int64_t* entity_ids);
/* Model::compute_gradients(result) (cpp/model.cu:145-152 → cpp/objective.cu:315-481) */
int nvsm_compute_gradients(nvsm_model* m);
/* Model::update(gradients, learning_rate, scaled_regularization_lambda) (cpp/model.cu:187-220) */
int nvsm_update(nvsm_model* m, float learning_rate, float scaled_regularization_lambda);
/* ForwardResult::get_cost() (cpp/intermediate_results.cu:80-124) — synchronises the stream, like the reference. */
int nvsm_get_cost(nvsm_model* m, float* cost);
/* the same value before it is narrowed to FloatT: the device accumulates Σ ω·log p in fp64, which is what lets the
 * gradient checker difference two costs that agree to seven digits */
int nvsm_get_cost_f64(nvsm_model* m, double* cost);
/* ForwardResult::scaled_regularization_lambda() (cpp/intermediate_results.cu:126-129): lambda / (global) batch */
float nvsm_scaled_regularization_lambda(nvsm_model* m);

/* One iterate_data loop body (cpp/main.cu:400-444): compute_cost + compute_gradients + update with
 * scaled lambda; fully asynchronous. cost may be NULL (no read-back, no sync). With a cost pointer the call returns once
 * the step's loss kernel has run and its loss word has been copied out (single GPU: the backward pass and the updates
 * are still running then, and the caller can queue the next step); under data parallelism, where the word is summed
 * over the ranks in the backward pass, it waits for the step as nvsm_get_cost does.
 * LIFETIME of a device-resident batch (batch->on_device): the word update reads batch->feature_weights — and the loss
 * kernel batch->weights — long after the prologue has consumed the ids, and nvsm_step(cost) returns BEFORE the updates have
 * run: the caller must leave all four arrays untouched until nvsm_synchronize — or, when the handle runs on the caller's own
 * stream (nvsm_set_stream), order the refill on that stream behind the step (everything that reads the batch is on that stream
 * or joined to it by the next call on the handle). Double-buffer device batches otherwise. nvsm_wait_inputs covers host batches
 * only. Errors flagged by the backward and update kernels of a step surface at the next call that waits. */
int nvsm_step(nvsm_model* m, const nvsm_batch* batch, const int64_t* entity_ids, float learning_rate, float* cost);

/*
 * DOCUMENT FOLD-IN (nvsm_step_fold). The model is transductive: a document exists for nvsm_rank only if it had a
 * row of E when training started. Folding new documents in trains THEIR rows against a frozen model: the word table, the
 * projection, the bias and rows [0, first_document) of the documents table stay as they are; rows [first_document, num_entities)
 * train with the configured objective, sampler and optimiser. (The caller creates the handle with the grown num_entities and loads
 * it: old rows copied, new rows drawn — nvsm_set_param_rows below. A live handle's tables do not grow.)
 *   forward, loss  exactly nvsm_compute_cost(batch, entity_ids): the same kernels, the same sampler — negatives are drawn over all
 *                  documents, frozen and new alike — and *cost is bit for bit what nvsm_compute_cost + nvsm_get_cost return from the
 *                  same state.
 *   not run        batch-norm backward, the dx and dT products, the words update, the projection update, the re-cut of T's planes.
 *   update         row r >= first_document gets nvsm_step's documents update restricted to those rows: g_r = Σ coef·proj and q_r
 *                  over the entries of the batch whose id is r, then the optimiser's row formula with the constants nvsm_step would
 *                  use (decay 1 − λ/B·lr, Adam's bias correction at the documents table's step counter, which advances by one). A new
 *                  row without entries gets what a dense pass gives it (decay of the row, of m and of the row's scalar under Adam).
 *                  Entries with id < first_document contribute to the loss and to nothing else.
 *   frozen state   rows < first_document of E and of its m / v / a, all of W, T, b and their optimiser state keep their LOGICAL
 *                  values (what nvsm_get_param returns) bit for bit, whatever λ and the Adam mode. On a lazily decayed documents table
 *                  the first fold step behind an ordinary one brings the table up to date; fold steps add no pending factors.
 *                  Ordinary steps and fold steps may be interleaved freely.
 *   reproducible   no float atomics. A row's sum runs over its entries in ascending entry order in an association that depends on
 *                  the row's entry count alone (nvsm_fold_summation: chunks of chunk_entries entries, each an fma chain from 0;
 *                  the chunk sums of a row added left to right; rows of more than group_chunks chunks: groups of group_chunks chunk
 *                  sums first, then the group sums left to right) — not on the grid, on max_batch_size or on the other rows.
 * NVSM_ERR_UNSUPPORTED (the handle stays usable): world_size > 1; l2_normalize_entity_reprs. NVSM_ERR_INVALID_ARGUMENT: first_document
 * outside [0, num_entities]; a negative learning rate. first_document == num_entities is valid: nothing trains, the cost is produced.
 * cost may be NULL (the call then does not wait). The index contract above holds for ids.
 */
typedef struct {
    int64_t first_document;   /* rows [0, first_document) of the documents table are frozen; rows [first_document, num_entities) train */
    int32_t reserved[6];
} nvsm_fold_options;
void nvsm_fold_options_default(nvsm_fold_options* opt);          /* first_document = 0 */
int nvsm_step_fold(nvsm_model* m, const nvsm_batch* batch, const int64_t* entity_ids, const nvsm_fold_options* opt, float learning_rate,
                   float* cost);
void nvsm_fold_summation(int32_t* chunk_entries, int32_t* group_chunks);      /* the constants of the summation order; either may be NULL */
/* Rows [first_row, first_row + rows) of an embedding table ("word_representations-representations",
 * "entity_representations-representations") or of its per-row optimiser state ("<param>/m", "/v", "/a"): host arrays of rows x width
 * floats, width the table's dimension or 1 for a per-row scalar. Same waits and the same flush of a lazily decayed table as
 * nvsm_get_param / nvsm_set_param. A range outside the table, or any other parameter name, is NVSM_ERR_INVALID_ARGUMENT. */
int nvsm_get_param_rows(nvsm_model* m, const char* name, int64_t first_row, int64_t rows, float* host_dst);
int nvsm_set_param_rows(nvsm_model* m, const char* name, int64_t first_row, int64_t rows, const float* host_src);

/*
 * The entity-entity similarity objective (RepresentationSimilarity::Objective on ENTITY_REPRS, cpp/objective.cu:485-696) and its
 * mixture with the text objective (TextEntityEntityEntity, cpp/objective.cu:698-745) — what the reference trains when
 * cuNVSMTrainModel gets document-document similarities as its second argument (PRODUCT_SUBSTITUTABILITY.md).
 *   pair objective   a batch is M pairs (a_p, b_p, ω_p) of document ids, interleaved as pairs[2p], pairs[2p + 1] (cpp/data.cu:316-334).
 *                    s_p = E[a_p]·E[b_p]; prob_p = clip(σ(s_p), 1e-7, 1 − 1e-7) in float32 (objective.cu:546-550, the two-branch sigmoid
 *                    of include/cuNVSM/cuda_utils.h:193-214); cost = −(1/M)·Σ ω_p·log prob_p (:553-567, intermediate_results.cu:81-124).
 *                    No negative samples, no projection. mult_p = ω_p·d(prob_p)/M with d(x) = 0 for x ≥ 1 − 1e-6 or x ≤ 1e-6, else 1 − x
 *                    (:607-626, cuda_utils.h:218-235); the gradient of entry 2p is mult_p·E[b_p], that of entry 2p + 1 mult_p·E[a_p]
 *                    (flip_adjacent_columns, :643-661), both from the rows as they were at compute_cost (:519-521); window 1, no
 *                    per-entry weights (intermediate_results.cu:300-307); gradient ascent. a_p == b_p and repeated pairs simply add.
 *                    scaled lambda = lambda / M. Only the documents table is updated (the other parameters have no gradient:
 *                    cpp/params.cu:304-307), with any of the five update methods.
 *   mixed objective  cost = (cost_text + cost_pairs) / 2 — an unweighted mean (AverageFn) —; scaled lambda = (lambda/B + lambda/M) / 2;
 *                    every text gradient is scaled by w_te / (w_te + w_ee), the pair gradient by w_ee / (w_te + w_ee)
 *                    (MergeGradientsFn, intermediate_results.cu:3-60); the documents table is updated ONCE from both entry lists — one
 *                    decay, both scatters (CompositeGradients, cpp/storage.cu:65-99), Adam's m from both lists (updates_adam.cu:196-200),
 *                    dense_update's per-row v from the per-entry means of squares of both lists (:216-252), full Adam squares the summed
 *                    gradient (:253-282). Exists for sgd, dense_update and full Adam; the reference refuses Adagrad
 *                    (updates_adagrad.cu:108) and sparse Adam (updates_adam.cu:348) with more than one gradient list, and so does this.
 * text == NULL: the pair objective alone (entity_ids and mix are ignored). Pair ids follow the index contract above (checked on the
 * device, row 0, NVSM_ERR_INVALID_ARGUMENT at the next wait). on_device = 0: host arrays, copied by the call (nvsm_wait_inputs also
 * covers them); 1: device arrays, which must stay untouched until nvsm_synchronize. weights NULL = all 1.0.
 * nvsm_compute_gradients / nvsm_update / nvsm_get_cost / nvsm_get_cost_f64 / nvsm_scaled_regularization_lambda act on whichever
 * forward result is current. nvsm_get_tensor additionally knows "pair_probs" [M], "pair_multipliers" [M] (mixture scale included),
 * "grad_pair_entity" [2M][entity_repr_size], "pair_cost" and "text_cost" [1]; in a mixed result the text tensors carry the
 * w_te / (w_te + w_ee) scale, as the reference's do after merging.
 * NVSM_ERR_UNSUPPORTED (the handle stays usable): mixed with Adagrad or sparse Adam; world_size > 1; l2_normalize_entity_reprs.
 * NVSM_ERR_INVALID_ARGUMENT: a mixture weight <= 0, num_pairs < 1 or > max_batch_size.
 * The pair workspaces (and the larger CSR workspace of the documents table) are allocated by the first of these calls; a handle that
 * never makes one allocates and launches exactly what it did before they existed. nvsm_step_mixed equals
 * nvsm_compute_cost_mixed; nvsm_compute_gradients; nvsm_update(scaled lambda) bit for bit; cost may be NULL.
 */
typedef struct {
    const int64_t* pairs;         /* [2 * num_pairs] document ids, interleaved */
    const float*   weights;       /* [num_pairs] or NULL (= all 1.0) */
    int64_t        num_pairs;
    int32_t        on_device;
    int32_t        reserved[3];
} nvsm_pair_batch;
typedef struct {
    float   text_weight;          /* w_te: TrainConfig.text_entity_weight */
    float   pair_weight;          /* w_ee: TrainConfig.entity_entity_weight */
    int32_t reserved[2];
} nvsm_mixture;
int nvsm_compute_cost_mixed(nvsm_model* m, const nvsm_batch* text /* NULL: pairs only */, const int64_t* entity_ids,
                            const nvsm_pair_batch* pairs, const nvsm_mixture* mix /* ignored when text is NULL */);
int nvsm_step_mixed(nvsm_model* m, const nvsm_batch* text, const int64_t* entity_ids, const nvsm_pair_batch* pairs,
                    const nvsm_mixture* mix, float learning_rate, float* cost);

/*
 * The term-term similarity objective (RepresentationSimilarity::Objective with param_id_ == WORD_REPRS, cpp/objective.cu:485-696) and
 * its mixture with the text objective (TextEntityTermTerm, cpp/objective.cu:747-794, cpp/main.cu:742-750). Both calls take the
 * structs of the entity-pair calls unchanged; nvsm_pair_batch::pairs holds MODEL WORD IDS here, nvsm_mixture::pair_weight is w_tt.
 *   pair objective   a batch is M pairs (a_p, b_p, ω_p) of model word ids, interleaved. s_p = W[a_p]·W[b_p];
 *                    prob_p = clip(σ(s_p), 1e-7, 1 − 1e-7) in float32 with the two-branch sigmoid; cost = −(1/M)·Σ ω_p·log prob_p;
 *                    mult_p = ω_p·d(prob_p)·exp(−log M), the derivative clamp at 1e-6. The gradient of entry 2p is mult_p·W[b_p], that
 *                    of entry 2p + 1 mult_p·W[a_p], both from the rows as they were at compute_cost. Window 1, no per-entry weights
 *                    (include/cuNVSM/intermediate_results.h:328-334), gradient ascent, scaled lambda = lambda / M. Only the words
 *                    table has a gradient: T, b, E, the batch-norm parameters and their step counters are left alone
 *                    (cpp/params.cu:304-307). All five update methods: sparse Adam runs with window 1, Adagrad uses the per-entry
 *                    accumulator and scale of updates_adagrad.cu:136-158 with window 1.
 *   mixed objective  cost = (cost_text + cost_pairs) / 2; scaled lambda = (lambda/B + lambda/M) / 2; text gradients are scaled by
 *                    w_te / (w_te + w_tt), the pair gradient by w_tt / (w_te + w_tt) (MergeGradientsFn, cpp/intermediate_results.cu:3-60).
 *                    The WORDS table is updated once from both gradient lists (CompositeGradients, cpp/storage.cu:65-99): one decay, the
 *                    text list's scatter with window w and the feature weights, then the pair list's with window 1 and weight 1. Adam's m
 *                    comes from both lists (updates_adam.cu:196-200), dense_update's per-row v from both lists' per-source means of
 *                    squares, scattered with the same window and weights (:216-252), full Adam squares the summed gradient (:253-282).
 *                    The documents table and the projection see the text objective only, at its share. Refused, as the reference
 *                    refuses them: Adagrad (updates_adagrad.cu:108) and sparse Adam (updates_adam.cu:348).
 * The words table pass weighs an entry's mean of squares linearly by its coefficient (the reference scatters v with the gradient's
 * repr_weights), so a pair entry carries its MULTIPLIED row c_p·W[other] (c_p = mult_p x the mixture scale), weight 1, and the mean of
 * squares of that row (pairs.hip).
 * nvsm_compute_gradients / nvsm_update / nvsm_get_cost(_f64) / nvsm_scaled_regularization_lambda act on the current forward result.
 * nvsm_get_tensor additionally knows "term_pair_probs" [M], "term_pair_multipliers" [M] (mixture scale included), "grad_pair_word"
 * [2M][word_repr_size] (the rows as stored: multiplied), "term_pair_msq" [2M] (their means of squares, as the words update reads
 * them), "pair_cost" and "text_cost" [1]. A word id outside [0, num_words) follows the index contract: row 0, and
 * NVSM_ERR_INVALID_ARGUMENT at the next call that waits.
 * NVSM_ERR_UNSUPPORTED (the handle stays usable): mixed with Adagrad or sparse Adam; world_size > 1; word_repr_size above 1024, or
 * above 256 and no multiple of 4; 3 x max_batch_size x window_size >= 2^26. NVSM_ERR_INVALID_ARGUMENT: a mixture weight <= 0,
 * num_pairs outside [1, max_batch_size], null pairs. A handle may make entity-pair and term-pair calls at different times; one call
 * takes one kind (the reference excludes both at once, cpp/main.cu:733-745).
 * Allocated by the first of these calls (B = Mx = max_batch_size, w = window_size): 2Mx more gradient rows (2Mx·word_repr_size floats),
 * 2Mx means of squares, 2Mx word ids, B·w + 2Mx entry ids, (B + 2Mx)·w entry weights, the words CSR workspace again for B·w + 2Mx
 * entries, the per-source buffers of sparse Adam / Adagrad for max(B, 2Mx) rows, and the pair kernel's ids, weights, probabilities and
 * multipliers (2Mx int64 + 3Mx floats + B floats) where no entity-pair call made them. nvsm_describe says whether this has happened.
 * A handle that never makes one of these calls allocates and launches exactly what it did before they existed.
 * nvsm_step_term_mixed equals nvsm_compute_cost_term_mixed; nvsm_compute_gradients; nvsm_update(scaled lambda) bit for bit.
 */
int nvsm_compute_cost_term_mixed(nvsm_model* m, const nvsm_batch* text /* NULL: pairs only */, const int64_t* entity_ids,
                                 const nvsm_pair_batch* pairs /* word ids */, const nvsm_mixture* mix /* pair_weight = w_tt */);
int nvsm_step_term_mixed(nvsm_model* m, const nvsm_batch* text, const int64_t* entity_ids, const nvsm_pair_batch* pairs,
                         const nvsm_mixture* mix, float learning_rate, float* cost);

/*
 * Training from an HBM-resident corpus: window references instead of batches. A host nvsm_batch carries 12·w + 12 bytes per window
 * (132 at w = 10); the windows of a collection are all slices of one token arena, so a window is fully named by 8 bytes — its
 * document and the position of its first token inside the document. nvsm_corpus_upload puts the arena, the document offsets and
 * the two weight tables into HBM once; the *_windows calls then take [num_instances] references and a kernel on the copy stream
 * writes the batch they denote into the staging set a host batch would have been copied into. No reference counterpart.
 * SEMANTICS — the contract. With w = window_size, window i of a batch of references (doc_i, pos_i) is the nvsm_batch instance
 *   features[i·w + j]        = tokens[doc_offsets[doc_i] + pos_i + j]          j = 0 .. w − 1
 *   feature_weights[i·w + j] = term_weights[that token]                        (term_weights NULL: feature_weights NULL)
 *   labels[i]                = doc_i
 *   weights[i]               = doc_weights[doc_i]                               (doc_weights NULL: weights NULL)
 * and every *_windows call equals its nvsm_batch twin on that batch BIT FOR BIT: the cost, every tensor of nvsm_get_tensor, every
 * parameter, the optimiser state, the RNG state and the lazy-decay bookkeeping (everything behind the expansion is the twin's code
 * on an ordinary device batch). Document i of the corpus is document id i of the model, hence num_documents <= num_entities.
 * LIFETIME of refs is that of nvsm_batch.features: nvsm_wait_inputs covers host refs; device refs must stay untouched until
 * nvsm_synchronize or be ordered behind the step on the caller's stream (nvsm_set_stream). With NVSM_SAMPLER_HOST_MINSTD the host
 * needs the labels: it takes them from refs[2i], or reads device refs back on the copy stream as device labels are read back.
 * nvsm_corpus_upload is synchronous (it waits for everything the handle has queued first), copies the four host arrays — the
 * caller may free them when it returns —, replaces an earlier corpus, and frees it when corpus is NULL. The new corpus is built and
 * checked next to the earlier one and takes its place only when every check has passed: a refused upload leaves the handle with the
 * corpus it had. NVSM_ERR_INVALID_ARGUMENT,
 * each with a sentence naming the field, before the call ends: doc_offsets that do not start at 0 or that decrease; a last offset
 * that is not num_tokens; num_documents > num_entities; a token outside [0, num_words) (checked on the device in one pass).
 * AT STEP TIME the index contract above holds: a reference whose document is >= num_documents, or whose pos + w reaches beyond its
 * document, becomes a window of word id 0 and label 0 (with their weights) — nothing is read out of bounds — and the next call of
 * the handle that waits returns NVSM_ERR_INVALID_ARGUMENT once. A *_windows call on a handle without a corpus is
 * NVSM_ERR_INVALID_ARGUMENT before anything runs; num_instances outside (0, max_batch_size] likewise. world_size > 1 is
 * NVSM_ERR_UNSUPPORTED (the handle stays usable): the materialised batch would pass through the data-parallel path unchanged, but
 * that is untested. The mixed / pair step takes no references.
 * MEMORY: the corpus (4 B per token, 8 per document + 4 with doc_weights, 4 per word with term_weights) and two staging buffers of
 * 8 B x max_batch_size for host refs are allocated by the upload, not by nvsm_create: a handle that never uploads a corpus allocates
 * and launches exactly what it did before these calls existed. nvsm_describe reports " corpus=<bytes>B" only when there is one.
 */
typedef struct {
    const int32_t* tokens;        /* [num_tokens] model word ids, documents back to back (host) */
    const int64_t* doc_offsets;   /* [num_documents + 1], offsets[0] = 0, non-decreasing, last = num_tokens (host) */
    const float*   doc_weights;   /* [num_documents] instance weight of every window of the document, or NULL (= nvsm_batch.weights NULL) */
    const float*   term_weights;  /* [num_words] feature weight of every occurrence of the word, or NULL (= feature_weights NULL) */
    int64_t num_tokens, num_documents;
    int32_t reserved[4];
} nvsm_corpus;
typedef struct {
    const uint32_t* refs;         /* [2 * num_instances]: document, first token inside the document; interleaved */
    int64_t num_instances;
    int32_t on_device;            /* as nvsm_batch: 0 host (page-locked: pulled by the copy-stream kernel; pageable: hipMemcpyAsync), 1 device */
    int32_t reserved[3];
} nvsm_window_batch;
int nvsm_corpus_upload(nvsm_model* m, const nvsm_corpus* corpus);   /* synchronous; replaces an earlier corpus; NULL corpus frees it */
int nvsm_compute_cost_windows(nvsm_model* m, const nvsm_window_batch* windows, const int64_t* entity_ids);
int nvsm_step_windows(nvsm_model* m, const nvsm_window_batch* windows, const int64_t* entity_ids, float learning_rate, float* cost);
int nvsm_step_windows_deferred(nvsm_model* m, const nvsm_window_batch* windows, const int64_t* entity_ids, float learning_rate, int64_t* ticket);

/* The same step for training loops that want the loss of EVERY batch, as cpp/main.cu:427-444 does, without putting the
 * GPU behind the host: nvsm_step_deferred queues the step plus a device→host copy of its loss word and hands back a
 * ticket; nvsm_deferred_cost(ticket) waits for that copy only (not for the step's updates). At most
 * NVSM_MAX_DEFERRED tickets may be outstanding (older ones are overwritten). nvsm_wait_inputs returns once the last
 * queued step has copied its host batch to the device, i.e. once the caller may refill those host buffers; a loop that
 * calls it before refilling and reads each loss one step late keeps one whole step queued ahead of the GPU. */
#define NVSM_MAX_DEFERRED 8
int nvsm_step_deferred(nvsm_model* m, const nvsm_batch* batch, const int64_t* entity_ids, float learning_rate, int64_t* ticket);
int nvsm_deferred_cost(nvsm_model* m, int64_t ticket, float* cost);
int nvsm_wait_inputs(nvsm_model* m);

/* Intermediates / gradients of the last compute_cost / compute_gradients, for parity tests and the
 * gradient checker (Parameters::get_parameter_gradient, cpp/storage.cu:133-183,264-283). Names:
 *   "phrase" [B][dw], "pre" [B][de], "proj" [B][de], "probs" [B*R], "entity_ids" [B*R] (as float),
 *   "bn_mean" [de], "bn_inv_std" [de], "multipliers" [B*R] (signed),
 *   "grad_transform" (de x dw col-major), "grad_bias" [de], "grad_phrase" [B][dw], "grad_entity" [B*R][de],
 *   "grad_proj" [B][de]. */
int nvsm_tensor_size(nvsm_model* m, const char* name, int64_t* count);
int nvsm_get_tensor(nvsm_model* m, const char* name, float* host_dst, int64_t count);

/*
 * Query inference and top-k document ranking — what the reference does with a trained model (no counterpart in its
 * training loop). Semantics, pinned by the reference:
 *   query        a list of model word ids of any length >= 1 (ragged: the queries of one call differ in length) with optional
 *                per-word weights. Representation = Σ wᵢ·W[idᵢ] / Σ wᵢ (np.average, py/nvsm/base.py:305-307); word_weights
 *                NULL = the plain mean, which is Model::infer's gather-mean over a fixed window (cpp/model.cu:105-133,
 *                cpp/params.cu:75-95). Mapping index term ids to model ids, dropping out-of-vocabulary terms and computing
 *                self-information weights (-log(tf / total), base.py:297-301) are the caller's job.
 *   projection   f(T·x + c·b). NO batch normalisation, even on a handle created with batch_normalization = 1: the reference
 *                passes nullptr statistics (cpp/model.cu:125-128, cpp/params.cu:396-428) and so does base.py:311-323.
 *                bias_coefficient c = 1 with the handle's nonlinearity is Model::infer (the default here); c = 0 with tanh is
 *                what py/query.py computes by default — base.py:228-233 multiplies the bias by a coefficient that is 0 whenever
 *                the bias is kept (a quirk of the reference, reproduced by passing 0, not "fixed"); NVSM_ACT_IDENTITY is --linear.
 *                l2_normalize_phrase_reprs / l2_normalize_entity_reprs of the handle are ignored: the reference's normalisers
 *                belong to the objective (cpp/objective.cu:99-107), not to Model::infer, and base.py has none.
 *   score        NVSM_SIM_COSINE: cosine similarity of the projected query and a document row, larger is better (the reference
 *                returns the cosine DISTANCE, base.py:362-430, and py/query.py negates it); NVSM_SIM_DOT: the plain dot
 *                product. A document row or a projected query of norm 0 has inverse norm 0: score 0, never NaN.
 *   ranking      the top_k best documents per query, 1 <= top_k <= num_entities, by score descending, ties by ASCENDING
 *                document id: a pure function of the parameters and the query (a repeated call returns the same bits). With
 *                candidates (base.py's document_set: re-ranking judged documents) only those rows are scored and
 *                counts[q] = min(top_k, number of distinct candidates of q). A query without words has counts[q] = 0 (the
 *                reference returns None). Slots beyond counts[q] hold id -1 and score -inf.
 * Word ids follow the index contract above: an id out of range reads row 0 and the call (it waits for its own results)
 * returns NVSM_ERR_INVALID_ARGUMENT. Candidate ids out of range, decreasing offsets, word weights that sum to 0, unknown
 * enums and top_k outside [1, num_entities] are NVSM_ERR_INVALID_ARGUMENT before anything runs.
 * Both calls are synchronous and return host results; they run behind everything earlier steps have queued (the side
 * streams' tails included) and leave parameters, optimiser state and the lazy-decay bookkeeping untouched: lazily decayed
 * tables are read through their view (the values nvsm_get_param would return), nothing is flushed. The number of queries is
 * independent of max_batch_size (chunked internally); device scratch is allocated by the first call, not by nvsm_create.
 */
enum { NVSM_SIM_COSINE = 0, NVSM_SIM_DOT = 1 };
enum { NVSM_ACT_MODEL = -1, NVSM_ACT_IDENTITY = -2 };   /* or NVSM_TANH / NVSM_HARD_TANH */
typedef struct {
    const int64_t* word_ids;      /* [offsets[num_queries]] host */
    const float*   word_weights;  /* same length, or NULL */
    const int64_t* offsets;       /* [num_queries + 1], non-decreasing, offsets[0] = 0 */
    int64_t        num_queries;
} nvsm_queries;
typedef struct {
    float   bias_coefficient;     /* 1 = Model::infer, 0 = py/query.py's default */
    int32_t activation;           /* NVSM_ACT_MODEL, NVSM_ACT_IDENTITY, NVSM_TANH, NVSM_HARD_TANH */
    int32_t similarity;           /* NVSM_SIM_* */
    int32_t top_k;
    const int64_t* candidates;         /* optional: concatenated per-query document ids (duplicates and any order allowed) */
    const int64_t* candidate_offsets;  /* [num_queries + 1] when candidates != NULL */
    int32_t reserved[4];
} nvsm_rank_options;
/* bias_coefficient 1, NVSM_ACT_MODEL, NVSM_SIM_COSINE, top_k 1000 (py/query.py --top_k), no candidates */
void nvsm_rank_options_default(nvsm_rank_options* opt);
/* out [num_queries][entity_repr_size] host; top_k, similarity and candidates are not looked at */
int nvsm_infer(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* opt, float* out);
/* doc_ids, scores [num_queries][top_k], counts [num_queries], all host */
int nvsm_rank(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* opt,
              int64_t* doc_ids, float* scores, int64_t* counts);

/*
 * Ranking and retrieval metrics in one call: nvsm_evaluate ranks exactly as nvsm_rank does (same arguments, same checks with
 * the same sentences, same ids / scores / counts bit for bit) and computes each query's metrics ON THE DEVICE from the ranked
 * ids of every round, so that validation over thousands of topics at top_k = 1000 brings back a few doubles per query
 * instead of num_queries x top_k ids and scores. doc_ids / scores / counts are still returned where the caller passes
 * buffers (a run file needs them); each of the three may be NULL.
 * The metrics are trec_eval's num_ret, num_rel, num_rel_ret, map, Rprec, recip_rank, ndcg, P_c, recall_c and ndcg_cut_c AS FAR AS
 * WRITTEN HERE — these formulas are the contract. For one query, r_1 .. r_n is the ranking nvsm_rank returns, n = counts[q]; its
 * order is the library's: score descending, ties by ASCENDING DOCUMENT ID (trec_eval would break ties by docno). g(d) is the
 * judged grade of d, 0 if d is unjudged; rel(d) means g(d) >= 1; R is the number of judged entries with grade >= 1, entries with
 * id -1 (judged documents the model does not hold) included: they can never be retrieved, as in trec_eval;
 * c_i = sum over j <= i of rel(r_j). Then
 *   num_ret = n, num_rel = R, num_rel_ret = c_n
 *   ap         = (1 / R) · sum over i with rel(r_i) of c_i / i
 *   rprec      = c_min(R, n) / R
 *   recip_rank = 1 / min{i : rel(r_i)}, 0 if there is none
 *   P@c        = c_min(c, n) / c          (always divided by c)
 *   recall@c   = c_min(c, n) / R
 *   dcg@c      = sum over i <= min(c, n) with g(r_i) > 0 of g(r_i) / log2(i + 1)
 *   idcg@c     = the same sum over the query's judged grades > 0 sorted descending, the first c of them (-1 entries included)
 *   ndcg@c     = dcg@c / idcg@c;  ndcg = ndcg@c with c = infinity
 * Every ratio with a zero denominator is 0. A query without words gets all zeros. All arithmetic is fp64; sums are taken in a
 * fixed order (a repeated call returns the same bits).
 * Judgments: per query a list of (model document id, grade), ids in [-1, num_entities), an id >= 0 at most once per query, any
 * order. Decreasing offsets or offsets[0] != 0, an id out of range, a repeated id, cutoffs that are not ascending, are < 1 or
 * number more than NVSM_EVAL_MAX_CUTOFFS, and a NULL metrics are NVSM_ERR_INVALID_ARGUMENT before anything runs.
 * Like nvsm_rank the call is synchronous, runs behind everything queued, reads lazily decayed tables through their view and
 * leaves parameters, optimiser state and the lazy bookkeeping bit-identical.
 */
#define NVSM_EVAL_MAX_CUTOFFS 8
typedef struct {
    const int64_t* doc_ids;    /* concatenated per query: judged model document ids; -1 = a judged document the model does not hold */
    const int32_t* grades;     /* same length; >= 1 relevant, <= 0 judged non-relevant */
    const int64_t* offsets;    /* [num_queries + 1], offsets[0] = 0, non-decreasing */
    const int32_t* cutoffs;    /* ascending, each >= 1 */
    int32_t num_cutoffs;       /* 0 .. NVSM_EVAL_MAX_CUTOFFS */
    int32_t reserved[3];
} nvsm_judgments;
enum { NVSM_EVAL_NUM_RET, NVSM_EVAL_NUM_REL, NVSM_EVAL_NUM_REL_RET, NVSM_EVAL_AP, NVSM_EVAL_RPREC, NVSM_EVAL_RECIP_RANK,
       NVSM_EVAL_NDCG, NVSM_EVAL_FIXED };      /* then per cutoff j: P, recall, ndcg at NVSM_EVAL_FIXED + 3 j + {0, 1, 2} */
/* metrics [num_queries][NVSM_EVAL_FIXED + 3 * num_cutoffs] doubles, host; doc_ids / scores / counts as nvsm_rank, each may be NULL */
int nvsm_evaluate(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* opt, const nvsm_judgments* judgments,
                  double* metrics, int64_t* doc_ids, float* scores, int64_t* counts);

/*
 * Query-likelihood ranking over the HBM-resident corpus, and the fusion of that run with nvsm_rank's — the last stage of the
 * reference's rank-cranfield-collection.sh, which takes its lexical run from Indri and fuses with py/combine_runs.py --alpha.
 * SEMANTICS — the contract. The lexical model is defined on the corpus AS UPLOADED (nvsm_corpus_upload): model word ids, with
 * out-of-vocabulary positions already dropped or mapped by whoever built the arena. It is a model over the uploaded vocabulary, not
 * over Indri's. With D_c = num_documents, N = num_tokens, len(d) = doc_offsets[d + 1] − doc_offsets[d], tf(t, d) = occurrences of
 * word t in document d, cf(t) = occurrences of t in the arena and p(t) = cf(t) / N, a query is the nvsm_queries list of word ids
 * t_1 .. t_L:
 *   duplicates      a word repeated in a query contributes once per occurrence. word_weights are not looked at
 *                   (nvsm_lexical_rank_weighted, below, honours them).
 *   absent terms    a query term with cf(t) = 0 is dropped. A query with no remaining terms, or without words, retrieves nothing:
 *                   counts[q] = 0, ids -1, scores -inf, as in nvsm_rank.
 *   NVSM_LEX_JM         s(q, d) = Σ_j log((1 − λ)·tf(t_j, d) / len(d) + λ·p(t_j)), λ in (0, 1) the weight of the collection model
 *   NVSM_LEX_DIRICHLET  s(q, d) = Σ_j log((tf(t_j, d) + μ·p(t_j)) / (len(d) + μ)), μ > 0
 *   param = 0       "auto": λ = 0.5, μ = N / D_c (the average document length).
 *   retrieved set   a document is retrieved if it contains at least one remaining query term; a document with len(d) = 0 never is.
 *                   counts[q] = min(top_k, matching documents), 1 <= top_k <= num_documents.
 *   order           score descending, ties by ASCENDING document id; a pure function of corpus and query (a repeated call returns
 *                   the same bits). Document i of the corpus is model document i.
 *   accuracy        scores are float32. With a_j the fp64 value of term j, |score − the fp64 sum| <= 2^-23 · Σ_j (8 + (L + 2)·|a_j|):
 *                   the argument of a log takes at most seven fp32 roundings from exact integers, an accurate logf adds about one
 *                   ulp of |a_j|, an fp32 sum of L terms about (L − 1) ulps of Σ|a_j|. (The kernel evaluates in fp64 and narrows the
 *                   sum once, which is well inside that bound; no fast-math log.)
 * A query of more than NVSM_LEXICAL_MAX_QUERY_TERMS DISTINCT word ids is NVSM_ERR_UNSUPPORTED (the per-document counters of
 * a round's terms live in LDS).
 * FUSION (nvsm_rank_ensemble). Inputs per query: list A, the nvsm_rank result, and list B, the lexical result, with weights
 * w_A = alpha and w_B = 1 − alpha. Each list's scores are normalised over THAT LIST'S RETURNED ENTRIES (its first counts[q]):
 *   NVSM_NORM_STANDARDIZE  (x − mean) / population standard deviation        NVSM_NORM_MINMAX  (x − min) / (max − min)
 *   NVSM_NORM_NONE         x
 * The fused score of a document is the MEAN OVER THE LISTS THAT CONTAIN IT of w·normalised score: (w_A·n_A + w_B·n_B) / 2 for a
 * document in both, w·n UNDIVIDED for a document in one list only — the reference's behaviour, reproduced as it is. Two deviations
 * from the reference, which raises an exception in the first case and produces NaN in the second: a list whose scores are all equal
 * (standard deviation 0, or max = min) normalises to 0 everywhere; a query with one empty list is fused from the other list alone.
 * The result is the union of both lists, at most 2·top_k entries, by fused score descending, ties by ascending id; slots beyond
 * counts[q] hold (-1, -inf). Arithmetic is fp64 in a fixed order (sums in index order; mean, then Σ(x − mean)² / n), the order is
 * decided on the fp64 values, and the fused scores are returned narrowed to float32.
 * With judgments and metrics the call also returns nvsm_evaluate's metrics of the fused list (the same kernel on the fused ids,
 * width 2·top_k). rank_opt->top_k and lex->top_k must be equal, rank_opt->candidates must be NULL, and top_k may not exceed
 * NVSM_ENSEMBLE_MAX_TOP_K (NVSM_ERR_UNSUPPORTED: a query's 2·top_k entries are matched and sorted in LDS).
 * Both calls are synchronous, run behind everything queued, and touch no parameter, optimiser state, RNG state or lazy bookkeeping.
 * Scratch, and the cf table (one histogram pass over the arena at the first lexical call after an upload, kept with the corpus:
 * uploading or freeing a corpus drops it), are allocated on first use: a handle that never makes these calls allocates and launches
 * what it did before they existed, and its nvsm_describe text is unchanged. NVSM_ERR_INVALID_ARGUMENT before anything runs, each
 * with a sentence: no corpus uploaded; unknown method or normaliser; λ outside (0, 1); μ < 0; alpha outside [0, 1]; top_k out of
 * range; unequal top_ks; candidates given; null arguments, by name. A word id outside [0, num_words) follows the index contract:
 * it matches nothing and the call returns NVSM_ERR_INVALID_ARGUMENT.
 *
 * WEIGHTED QUERIES AND PSEUDO-RELEVANCE FEEDBACK (nvsm_lexical_rank_weighted, nvsm_relevance_model, nvsm_lexical_rank_prf,
 * nvsm_rank_ensemble_prf) — the "QLM w/ PRF" runs of rank-cranfield-collection.sh, which the reference takes from Indri (--prf)
 * through a package outside its tree. There is no program text to follow: the contract is this one, after Lavrenko's relevance model
 * in its RM3 form. cf, p(t), len(d), tf, the smoothing methods and "auto" mean what they mean above.
 *   weighted query likelihood   the query terms t_1 .. t_L carry float32 weights w_j >= 0 in queries->word_weights (required). A term
 *                   with cf = 0 or w_j = 0 is dropped; a query with nothing left retrieves nothing. s(q, d) = Σ_j w_j·a_j(d), a_j the
 *                   Jelinek-Mercer or Dirichlet log term above; the sum runs in query order in fp64 (every product rounded on its own)
 *                   and is narrowed to float32 ONCE. Retrieved set: the documents that hold at least one remaining term. Order: score
 *                   descending, ties by ascending id; a repeated call returns the same bits. Accuracy: every a_j <= 0 and w_j >= 0, so
 *                   nothing cancels: |score − the fp64 sum| <= 2^-23·|the fp64 sum| — tighter than nvsm_lexical_rank's bound on
 *                   purpose: fp64 evaluation is part of THIS contract. nvsm_lexical_rank keeps its own bound and its bits. (Weights all
 *                   1 return nvsm_lexical_rank's bits; a power-of-two weight on every term scales its scores exactly.)
 *   relevance model  per query: (1) the UNWEIGHTED first pass (nvsm_lexical_rank; queries->word_weights are not looked at) with
 *                   top_k = fb_docs returns d_0 .. d_{n−1} with float32 scores s_0 >= ..., n <= fb_docs; (2) ω_i = exp(double(s_i) −
 *                   double(s_0)); (3) π(t) = (Σ_i ω_i·tf(t, d_i) / len(d_i)) / Σ_i ω_i, both sums over the documents in rank order in
 *                   fp64, no document smoothing; π is narrowed to float32; (4) the expansion terms are the fb_terms terms with the
 *                   largest float32 π > 0, ties by ascending word id; counts[q] says how many there are, slots behind hold (-1, -inf).
 *                   Accuracy: |π − its fp64 value| <= 2^-23·π + 2^-149 (the narrowing; the fp64 sum of at most fb_docs positive terms
 *                   is right to a few of its own ulps). With n = 1 no exp is involved (ω = 1) and π(t) is float32(tf / len) exactly.
 *   expanded query  with o64 = double(orig_weight) and L the number of the query's remaining terms (cf > 0; repeated words count once
 *                   per occurrence): those terms first, in query order, each with weight float32(o64 / L); then the expansion terms in
 *                   rank order, each with weight float32(((1.0 − o64)·double(π_i)) / S), S = Σ_i double(π_i) summed in rank order.
 *                   A term in both groups appears twice. Plain fp64 operations. (Indri's #combine is a mean and its #weight normalises:
 *                   hence o / L and π_i / S.) Expansion terms are not filtered against the original query nor against a stop list: the
 *                   vocabulary is the model's. A query without remaining terms has no feedback documents and stays empty.
 *   nvsm_lexical_rank_prf   is BY DEFINITION nvsm_lexical_rank_weighted of the expanded query at lex->top_k: the same bits.
 *   nvsm_rank_ensemble_prf  is nvsm_rank_ensemble with list B taken from nvsm_lexical_rank_prf; everything else is the same code path.
 * Document smoothing inside the relevance model (Indri's fbMu) is out of scope. nvsm_relevance_model checks lex->top_k as the other
 * calls do but ranks at fb_docs. All four calls are synchronous, touch no parameter, optimiser state, RNG state or lazy bookkeeping,
 * allocate on first use (the relevance model's scratch, 12 bytes per word and query of a round, comes out of the same budget as the
 * score slab), and leave nvsm_describe unchanged. NVSM_ERR_INVALID_ARGUMENT before anything runs, each with a sentence: what
 * nvsm_lexical_rank refuses; null arguments by name, queries->word_weights among them for the weighted call; a weight that is negative
 * or not finite; fb_docs outside [1, min(num_documents, NVSM_FEEDBACK_MAX_DOCS)]; fb_terms outside [1, num_words]; orig_weight outside
 * [0, 1]. An EXPANDED query of more than NVSM_LEXICAL_MAX_QUERY_TERMS distinct terms is NVSM_ERR_UNSUPPORTED; it is known behind the
 * relevance model and refused there, before the second pass and before any result is written. A word id out of range fails the PRF
 * calls behind their first pass, with nothing written.
 */
enum { NVSM_LEX_JM = 0, NVSM_LEX_DIRICHLET = 1 };
enum { NVSM_NORM_STANDARDIZE = 0, NVSM_NORM_MINMAX = 1, NVSM_NORM_NONE = 2 };
#define NVSM_LEXICAL_MAX_QUERY_TERMS 1024
#define NVSM_ENSEMBLE_MAX_TOP_K 1024
typedef struct {
    int32_t method;               /* NVSM_LEX_* */
    float   param;                /* λ (JM) or μ (Dirichlet); 0 = auto */
    int32_t top_k;
    int32_t reserved[5];
} nvsm_lexical_options;
typedef struct {
    float   alpha;                /* weight of nvsm_rank's list; the lexical list weighs 1 − alpha */
    int32_t normalizer;           /* NVSM_NORM_* */
    int32_t reserved[6];
} nvsm_ensemble_options;
/* NVSM_LEX_JM, auto, top_k 1000 */
void nvsm_lexical_options_default(nvsm_lexical_options* opt);
/* alpha 0.5, NVSM_NORM_STANDARDIZE: what rank-cranfield-collection.sh passes */
void nvsm_ensemble_options_default(nvsm_ensemble_options* opt);
/* doc_ids, scores [num_queries][top_k], counts [num_queries], all host */
int nvsm_lexical_rank(nvsm_model* m, const nvsm_queries* queries, const nvsm_lexical_options* lex,
                      int64_t* doc_ids, float* scores, int64_t* counts);
/* doc_ids, scores [num_queries][2 * top_k], counts [num_queries], all host; judgments and metrics both given or both NULL:
 * metrics [num_queries][NVSM_EVAL_FIXED + 3 * num_cutoffs] */
int nvsm_rank_ensemble(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* rank_opt, const nvsm_lexical_options* lex,
                       const nvsm_ensemble_options* ens, const nvsm_judgments* judgments, double* metrics,
                       int64_t* doc_ids, float* scores, int64_t* counts);
#define NVSM_FEEDBACK_MAX_DOCS 1024
typedef struct {
    int32_t fb_docs;              /* feedback documents per query: 1 .. min(num_documents, NVSM_FEEDBACK_MAX_DOCS) */
    int32_t fb_terms;             /* expansion terms per query: 1 .. num_words */
    float   orig_weight;          /* weight of the original query in the expanded one, in [0, 1] */
    int32_t reserved[5];
} nvsm_feedback_options;
/* fb_docs 10, fb_terms 10, orig_weight 0.5 */
void nvsm_feedback_options_default(nvsm_feedback_options* opt);
/* nvsm_lexical_rank with queries->word_weights honoured (required); results as nvsm_lexical_rank */
int nvsm_lexical_rank_weighted(nvsm_model* m, const nvsm_queries* queries, const nvsm_lexical_options* lex,
                               int64_t* doc_ids, float* scores, int64_t* counts);
/* term_ids, term_probs [num_queries][fb_terms], counts [num_queries], all host; (-1, -inf) beyond counts[q] */
int nvsm_relevance_model(nvsm_model* m, const nvsm_queries* queries, const nvsm_lexical_options* lex, const nvsm_feedback_options* fb,
                         int64_t* term_ids, float* term_probs, int64_t* counts);
/* results as nvsm_lexical_rank */
int nvsm_lexical_rank_prf(nvsm_model* m, const nvsm_queries* queries, const nvsm_lexical_options* lex, const nvsm_feedback_options* fb,
                          int64_t* doc_ids, float* scores, int64_t* counts);
/* arguments and results as nvsm_rank_ensemble */
int nvsm_rank_ensemble_prf(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* rank_opt, const nvsm_lexical_options* lex,
                           const nvsm_feedback_options* fb, const nvsm_ensemble_options* ens, const nvsm_judgments* judgments,
                           double* metrics, int64_t* doc_ids, float* scores, int64_t* counts);

/*
 * SEQUENTIAL DEPENDENCE (nvsm_sdm_rank, nvsm_sdm_pair_counts, nvsm_rank_ensemble_sdm) — Metzler & Croft's sequential dependence model,
 * the Indri query #weight(w_T #combine(t_1 .. t_L) w_O #combine(#1(t_1 t_2) ..) w_U #combine(#uwW(t_1 t_2) ..)): the unigram score,
 * plus exact adjacent pairs of query terms, plus pairs that co-occur inside a small window. The reference has no program text for it;
 * the contract is this one. It is defined over the corpus AS UPLOADED: where the arena's builder dropped out-of-vocabulary positions,
 * adjacency means adjacency in the arena. cf, p(t), len(d), tf, N, the smoothing methods and "auto" mean what they mean for
 * nvsm_lexical_rank. For a query t_1 .. t_L as given and a window W, 2 <= W <= NVSM_SDM_MAX_WINDOW:
 *   pairs           (t_j, t_{j+1}), j = 1 .. L − 1, from the query as given (before any term is dropped); a repeated pair counts once per
 *                   occurrence. A query of one term has no pairs and ranks as its T group alone.
 *   ordered count   od(a, b; d) = #{i : tok_i = a and tok_{i+1} = b}, both positions inside d.
 *   unordered count uw(a, b; d) = #{i : tok_i in {a, b} and there is a j, i < j < i + W, j inside d, with tok_j = the OTHER term}; for
 *                   a = b the other term is a. Every position counts at most once per pair: an existence test, not a count of matches.
 *                   uw(a, b) = uw(b, a).
 *   collection      cf_o(a, b) and cf_u(a, b) are those counts summed over all documents, as integers.
 *   dropped         a term with cf = 0 is dropped from T, as in nvsm_lexical_rank; an ordered pair with cf_o = 0 is dropped from O; an
 *                   unordered pair with cf_u = 0 is dropped from U. (A pair with a term of cf = 0, or out of range, has no occurrence.)
 *   features        the unigram term a_j(d) is the log term of nvsm_lexical_rank. A pair feature uses the same formula with its count c
 *                   in place of tf and cf_x / N in place of p: Dirichlet log((c + μ·cf_x / N) / (len + μ)), JM log((1 − λ)·c / len +
 *                   λ·cf_x / N).
 *   score           three groups: T (terms), O (ordered pairs), U (unordered pairs), each in query order. With n_G remaining members
 *                   g_G = (Σ members in order, fp64) / n_G (Indri's #combine is a mean), and s(q, d) = Σ_G (w_G / Σ_{present G'} w_G')·g_G
 *                   over the PRESENT groups, those with n_G > 0 and w_G > 0 (Indri's #weight normalises). The weights are float32
 *                   widened to fp64 and added in the order T, O, U; every product and quotient is rounded on its own; the groups are
 *                   added in the order T, O, U; the sum is narrowed to float32 ONCE. With no group present (w_T = 0 and no pair left)
 *                   the score of a retrieved document is 0.
 *   retrieved set, order, ties, empty queries, counts   exactly nvsm_lexical_rank's: a document is retrieved if it holds at least one
 *                   remaining TERM, whatever the weights are.
 *   accuracy        every log term is <= 0 and every coefficient >= 0, so nothing cancels: |score − the fp64 value| <= 2^-23·|the fp64
 *                   value|, the weighted call's bound.
 *   reproducibility a repeated call returns the same bits (integer atomics only).
 * nvsm_sdm_pair_counts writes cf_o and cf_u of every pair (t_j, t_{j+1}) of every query, laid out [Σ_q max(L_q − 1, 0)] in query order:
 * exact integers, 0 for a pair that holds a term nobody holds. Only sdm->window is looked at beyond the refusals.
 * nvsm_rank_ensemble_sdm is nvsm_rank_ensemble with list B taken from nvsm_sdm_rank; everything behind list B is the same code path.
 * The postings of nvsm_corpus_index hold counts and no positions: without the positional layer (nvsm_corpus_index_positions, below)
 * these calls scan the arena whatever `use` says; with it their rounds may be served from the postings, the same bits either way.
 * All three calls are synchronous, touch no parameter, optimiser state, RNG state or lazy bookkeeping, allocate on first use and leave
 * nvsm_describe unchanged. NVSM_ERR_INVALID_ARGUMENT before anything runs, each with a sentence: what nvsm_lexical_rank refuses (and
 * nvsm_rank_ensemble, for the fused call); null arguments, by name; a weight that is negative or not finite, or all three weights
 * zero; a window outside [2, NVSM_SDM_MAX_WINDOW]. A round whose distinct terms or distinct pairs exceed the LDS counters is split by
 * the driver; a single query of more than NVSM_LEXICAL_MAX_QUERY_TERMS distinct terms or NVSM_SDM_MAX_QUERY_PAIRS distinct pairs is
 * NVSM_ERR_UNSUPPORTED. A word id out of range follows the index contract, as in nvsm_lexical_rank.
 */
#define NVSM_SDM_MAX_WINDOW 64
#define NVSM_SDM_MAX_QUERY_PAIRS 1024
typedef struct {
    float   w_term, w_ordered, w_unordered;      /* >= 0, not all zero; normalised over the groups that are present */
    int32_t window;               /* W of the unordered pairs: 2 .. NVSM_SDM_MAX_WINDOW */
    int32_t reserved[4];
} nvsm_sdm_options;
/* 0.85, 0.10, 0.05, window 8: Metzler & Croft's weights with #uw8 for pairs */
void nvsm_sdm_options_default(nvsm_sdm_options* opt);
/* results as nvsm_lexical_rank */
int nvsm_sdm_rank(nvsm_model* m, const nvsm_queries* queries, const nvsm_lexical_options* lex, const nvsm_sdm_options* sdm,
                  int64_t* doc_ids, float* scores, int64_t* counts);
/* ordered, unordered [Σ_q max(L_q − 1, 0)], host */
int nvsm_sdm_pair_counts(nvsm_model* m, const nvsm_queries* queries, const nvsm_sdm_options* sdm, uint64_t* ordered, uint64_t* unordered);
/* arguments and results as nvsm_rank_ensemble */
int nvsm_rank_ensemble_sdm(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* rank_opt, const nvsm_lexical_options* lex,
                           const nvsm_sdm_options* sdm, const nvsm_ensemble_options* ens, const nvsm_judgments* judgments,
                           double* metrics, int64_t* doc_ids, float* scores, int64_t* counts);

/*
 * SUPERVISED FUSION (nvsm_ensemble_sweep, nvsm_rank_ensemble_cv) — py/combine_runs.py --qrel --num_folds --alpha_stepsize, the mode
 * rank-cranfield-collection.sh takes its "NVSM + QLM" figures from: the fusion is evaluated on a grid of weights alpha, and for each of
 * k folds of the queries the alpha with the best training measure fuses the held-out queries.
 *   sweep      list A and list B are made ONCE per call, exactly as nvsm_rank_ensemble makes them (fb NULL: list B is
 *              nvsm_lexical_rank's) or as nvsm_rank_ensemble_prf does (fb given), with the same refusals and the same bits.
 *              metrics[a][q][:] is nvsm_evaluate's row of the list fused at alpha = alphas[a], over its first min(depth, count)
 *              entries; depth = 0: the whole list. With a cut, num_ret is the cut length and every other formula applies to the cut
 *              list unchanged (depth 1000: ap is trec_eval's map_cut_1000). With depth = 0 or depth >= 2·top_k every row equals BIT FOR
 *              BIT the row nvsm_rank_ensemble(_prf) returns for that alpha. Alphas are float32 in [0, 1], in any order, repeats
 *              allowed (equal alphas give equal rows), 1 <= num_alphas <= NVSM_SWEEP_MAX_ALPHAS. A query without words has all-zero
 *              rows. judgments are required.
 *   folds      cv->fold_of[q] in [0, num_folds) names the fold of query q. NULL: contiguous folds in query order, fold f holding
 *              num_queries / num_folds + 1 queries when f < num_queries % num_folds, else num_queries / num_folds (sklearn's KFold
 *              without shuffling). 2 <= num_folds <= num_queries. With fold_of given a fold may be empty: its outputs are
 *              (NaN, 0). A fold that holds every query (its training set is empty) is refused.
 *   choice     the training measure of (fold f, alpha a) is the mean over the queries NOT in f of column cv->measure of the sweep row
 *              (NVSM_EVAL_AP, NVSM_EVAL_NDCG, a cutoff column, ...; num_ret, num_rel and num_rel_ret are refused): the queries are added
 *              in ascending query index as plain sequential fp64 additions, then divided once by their number. A pure host function
 *              of the sweep table's bits. The alpha of the largest training measure is chosen; on an exact tie the LARGEST alpha value
 *              (Python's max() over (value, alpha) tuples).
 *   result     every query's list is what nvsm_rank_ensemble(_prf) returns for alpha = fold_alpha[fold of q], bit for bit in ids,
 *              scores and counts; metrics (may be NULL) [num_queries][width] are the sweep's rows of those lists, cut at depth;
 *              sweep_metrics (may be NULL) receives the sweep table.
 * Both calls are synchronous, touch no parameter, optimiser state, RNG state or lazy bookkeeping, and allocate on first use
 * (nvsm_describe of a handle that never makes them is unchanged). NVSM_ERR_INVALID_ARGUMENT before anything runs, each with a
 * sentence: everything nvsm_rank_ensemble(_prf) refuses; NULL alphas, judgments, metrics (and the cv call's required outputs), by name;
 * num_alphas out of range; an alpha outside [0, 1] or not finite; depth < 0; num_folds out of range; a fold_of entry out of range; an
 * unknown or not offered measure. top_k > NVSM_ENSEMBLE_MAX_TOP_K is NVSM_ERR_UNSUPPORTED.
 */
#define NVSM_SWEEP_MAX_ALPHAS 1024
typedef struct {
    const float* alphas;          /* [num_alphas], each in [0, 1] */
    int32_t num_alphas;           /* 1 .. NVSM_SWEEP_MAX_ALPHAS */
    int32_t normalizer;           /* NVSM_NORM_* */
    int32_t depth;                /* the metrics look at the first depth entries of a fused list; 0 = all */
    int32_t reserved[5];
} nvsm_sweep_options;
typedef struct {
    int32_t measure;              /* a column of the metric row: NVSM_EVAL_AP, ..., NVSM_EVAL_FIXED + 3 j + {0, 1, 2} */
    int32_t num_folds;            /* 2 .. num_queries */
    const int32_t* fold_of;       /* [num_queries], or NULL: contiguous folds in query order */
    int32_t reserved[4];
} nvsm_cv_options;
/* alphas NULL (the caller sets them), NVSM_NORM_STANDARDIZE, depth 0 */
void nvsm_sweep_options_default(nvsm_sweep_options* opt);
/* NVSM_EVAL_AP, 20 folds, fold_of NULL: what rank-cranfield-collection.sh passes */
void nvsm_cv_options_default(nvsm_cv_options* opt);
/* metrics [num_alphas][num_queries][NVSM_EVAL_FIXED + 3 * num_cutoffs] doubles, host; fb may be NULL */
int nvsm_ensemble_sweep(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* rank_opt, const nvsm_lexical_options* lex,
                        const nvsm_feedback_options* fb, const nvsm_sweep_options* sweep, const nvsm_judgments* judgments, double* metrics);
/* fold_alpha, fold_train_measure [num_folds]; doc_ids / scores [num_queries][2 * top_k], counts [num_queries]; metrics
 * [num_queries][width] or NULL; sweep_metrics as nvsm_ensemble_sweep's metrics or NULL; all host; fb may be NULL */
int nvsm_rank_ensemble_cv(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* rank_opt, const nvsm_lexical_options* lex,
                          const nvsm_feedback_options* fb, const nvsm_sweep_options* sweep, const nvsm_cv_options* cv,
                          const nvsm_judgments* judgments, float* fold_alpha, double* fold_train_measure,
                          int64_t* doc_ids, float* scores, int64_t* counts, double* metrics, double* sweep_metrics);

/*
 * TF-IDF FIRST-STAGE RETRIEVAL AND RE-RANKING OF ITS CANDIDATES (nvsm_tfidf_rank, nvsm_rerank) — py/query.py
 * --rerank_exact_matching_documents (query.py:186-205): Indri's TF-IDF query environment returns each topic's best 1000 documents and
 * the neural model ranks only those (base.py's document_set). Indri is outside the reference's tree: there is no program text to
 * follow, and the formula written here is the contract. D_c, N, len(d), tf and the corpus mean what they mean for nvsm_lexical_rank;
 * df(t) is the number of documents d with tf(t, d) >= 1; avgdl = N / D_c, empty documents counted (as μ auto does).
 *   term value      a_j(d) = idf(t_j) · tf·(k1 + 1) / (tf + k1·(1 − b + b·len(d) / avgdl)), tf = tf(t_j, d): BM25's saturating tf.
 *   NVSM_IDF_ROBERTSON  idf = ln((D_c + 1) / (df + 0.5)): Robertson's tf × idf, which Indri's tfidf baseline documents. Always > 0.
 *   NVSM_IDF_OKAPI      idf = ln((D_c − df + 0.5) / (df + 0.5)): negative for df > D_c / 2, reproduced as it is. Finite for every df in
 *                   [1, D_c], so -inf stays free to mark "no term of the query in this document".
 *   score           s(q, d) = Σ_j w_j·a_j(d) in query order; a repeated word contributes once per occurrence. w_j = 1 when
 *                   queries->word_weights is NULL, else the float32 weights, each finite and >= 0 (refused otherwise); a term of
 *                   weight 0 is dropped, and so is a term with df = 0. A query with nothing left, or without words, retrieves nothing.
 *   retrieved set   the documents that hold at least one remaining term; counts[q] = min(top_k, matches), 1 <= top_k <= num_documents.
 *   order           float32 score descending, ties by ascending id; slots behind hold (-1, -inf); a repeated call returns the same bits.
 *   arithmetic      fp64 plain operations without contraction, every product rounded on its own:
 *                   (idf·(tf·(k1 + 1))) / (tf + k1·((1 − b) + b·(len / avgdl))); the sum is narrowed to float32 ONCE. idf is evaluated
 *                   once per term by the host, the length norm once per document: no log per (document, term) pair.
 *   accuracy        |score − the exact value| <= 2^-23 · Σ_j |w_j·a_j|: one narrowing of an fp64 sum whose own error is orders of
 *                   magnitude smaller. (Weights all 1 return the unweighted bits; a power-of-two weight on every term scales exactly.)
 *   parameters      k1 finite and > 0, or 0 for auto 1.2; b in (0, 1], or 0 for auto 0.75.
 * The df table is made by one pass over the arena at the first call that needs it after an upload (integer atomics only: exact,
 * whatever their order) and kept with the corpus exactly as the cf table is: uploading or freeing a corpus drops it. A handle that
 * never makes these calls allocates and launches nothing new, and its nvsm_describe text is unchanged. More than
 * NVSM_LEXICAL_MAX_QUERY_TERMS distinct terms in a query is NVSM_ERR_UNSUPPORTED. NVSM_ERR_INVALID_ARGUMENT before anything runs, each
 * with a sentence: no corpus uploaded; unknown idf; k1 or b out of range or NaN; top_k outside [1, num_documents]; a weight that is
 * negative or not finite; null arguments by name; decreasing offsets. A word id out of range follows the index contract: it matches
 * nothing and the call returns NVSM_ERR_INVALID_ARGUMENT.
 *
 * nvsm_rerank returns BY DEFINITION, bit for bit, what nvsm_rank returns with `candidates` set to the ids the first stage returns at
 * top_k = depth, and with rank_opt's remaining fields. The first stage is nvsm_tfidf_rank (NVSM_STAGE_TFIDF, options rr->tfidf) or
 * nvsm_lexical_rank (NVSM_STAGE_LEXICAL, options rr->lexical); a NULL pointer means that stage's defaults, and the stage's own top_k
 * field is not looked at. The first stage is UNWEIGHTED: queries->word_weights shape only the neural stage's query representation
 * (query.py builds a plain query string). Results are [num_queries][rank_opt->top_k], counts[q] = min(top_k, first-stage count). With
 * judgments and metrics (both given or both NULL) the metrics are nvsm_evaluate's for those candidates; doc_ids, scores and counts may
 * each be NULL when metrics are asked for. The candidate ids never leave the device: per round of the first stage only the per-query
 * counts come back to the host (they size the second stage's rounds), and a kernel writes the retrieved ids, ascending, where the
 * candidate scan reads them. Refusals, before anything runs: rank_opt->candidates must be NULL; depth in [1, min(num_documents,
 * NVSM_RERANK_MAX_DEPTH)] (above the cap with enough documents: NVSM_ERR_UNSUPPORTED; a query's candidates are ordered in LDS);
 * depth >= rank_opt->top_k; an unknown first stage; and everything either stage would refuse, in its words. Synchronous, behind
 * everything queued, lazily decayed tables read through their view, no parameter, optimiser state, RNG state or lazy bookkeeping touched.
 */
enum { NVSM_IDF_ROBERTSON = 0, NVSM_IDF_OKAPI = 1 };
typedef struct {
    float   k1;                   /* > 0; 0 = auto 1.2 */
    float   b;                    /* in (0, 1]; 0 = auto 0.75 */
    int32_t idf;                  /* NVSM_IDF_* */
    int32_t top_k;
    int32_t reserved[4];
} nvsm_tfidf_options;
/* k1 0 (auto 1.2), b 0 (auto 0.75), NVSM_IDF_ROBERTSON, top_k 1000 */
void nvsm_tfidf_options_default(nvsm_tfidf_options* opt);
/* doc_ids, scores [num_queries][top_k], counts [num_queries], all host */
int nvsm_tfidf_rank(nvsm_model* m, const nvsm_queries* queries, const nvsm_tfidf_options* opt,
                    int64_t* doc_ids, float* scores, int64_t* counts);
#define NVSM_RERANK_MAX_DEPTH 4096
enum { NVSM_STAGE_TFIDF = 0, NVSM_STAGE_LEXICAL = 1 };
typedef struct {
    int32_t first_stage;          /* NVSM_STAGE_* */
    int32_t depth;                /* candidates per query: 1 .. min(num_documents, NVSM_RERANK_MAX_DEPTH), >= rank_opt->top_k */
    const nvsm_tfidf_options* tfidf;        /* NVSM_STAGE_TFIDF; NULL = defaults; its top_k is not looked at */
    const nvsm_lexical_options* lexical;    /* NVSM_STAGE_LEXICAL; NULL = defaults; its top_k is not looked at */
    int32_t reserved[4];
} nvsm_rerank_options;
/* NVSM_STAGE_TFIDF, depth 1000 (query.py:201), both pointers NULL */
void nvsm_rerank_options_default(nvsm_rerank_options* opt);
/* doc_ids, scores [num_queries][rank_opt->top_k], counts [num_queries], all host; judgments and metrics both given or both NULL:
 * metrics [num_queries][NVSM_EVAL_FIXED + 3 * num_cutoffs]; with metrics each of doc_ids / scores / counts may be NULL */
int nvsm_rerank(nvsm_model* m, const nvsm_queries* queries, const nvsm_rank_options* rank_opt, const nvsm_rerank_options* rr,
                const nvsm_judgments* judgments, double* metrics, int64_t* doc_ids, float* scores, int64_t* counts);

/*
 * INVERTED INDEX OF THE UPLOADED CORPUS (nvsm_corpus_index) — DESIGN.md §22
 *
 * A CSR of postings in HBM: per word its documents, ascending and each once, with the word's count in each. Once it exists, the
 * lexical rounds — nvsm_lexical_rank, its weighted form, nvsm_tfidf_rank, the first stage of nvsm_rerank, both passes of the
 * feedback calls, list B of the fused calls — may fill their score slabs from the postings of the query words instead of
 * re-reading the whole token arena. Both fills return THE SAME BITS: ids, scores and counts do not depend on `use`.
 *   NVSM_INDEX_NEVER   the arena scan           NVSM_INDEX_ALWAYS  the postings, in every lexical round
 *   NVSM_INDEX_AUTO    chosen per round on the host from the round's Σ df, its entries per query and the corpus size
 * nvsm_corpus_index is synchronous, runs behind everything queued and touches no parameter, optimiser state, RNG state or lazy
 * bookkeeping. On a corpus that is indexed already it only sets `use` and refills `info`. The layout is a function of the corpus
 * alone: a second build gives the same bytes. nvsm_corpus_upload, with a new corpus or NULL, drops the index with the corpus. A
 * handle that never calls it allocates and launches exactly what it did before, and its nvsm_describe text is unchanged.
 * NVSM_ERR_INVALID_ARGUMENT, each with a sentence, the handle staying usable: no corpus; no index (nvsm_corpus_postings); a null
 * argument, by name; an unknown `use`; a word id outside [0, num_words). NVSM_ERR_UNSUPPORTED: a corpus of 2^31 tokens or more;
 * world_size > 1. The index describes the corpus as uploaded; there are no incremental updates.
 */
enum { NVSM_INDEX_AUTO = 0, NVSM_INDEX_ALWAYS = 1, NVSM_INDEX_NEVER = 2 };
typedef struct {
    int32_t use;                  /* NVSM_INDEX_* */
    int32_t reserved[7];
} nvsm_index_options;
typedef struct {
    int64_t num_postings;         /* P = Σ_t df(t) */
    int64_t bytes;                /* HBM the index holds */
    int64_t max_df;               /* the longest list */
    int32_t use;                  /* NVSM_INDEX_* in force */
    int32_t reserved[9];
} nvsm_index_info;
/* NVSM_INDEX_AUTO */
void nvsm_index_options_default(nvsm_index_options* opt);
/* info may be NULL */
int nvsm_corpus_index(nvsm_model* m, const nvsm_index_options* opt, nvsm_index_info* info);
/* frees the index (the corpus stays); no index: success */
int nvsm_corpus_index_free(nvsm_model* m);
/* one word's list to the host: *count = df(word_id), always written; doc_ids / tfs [capacity] receive the list when
 * capacity >= *count, else nothing else is written and the call returns NVSM_ERR_INVALID_ARGUMENT */
int nvsm_corpus_postings(nvsm_model* m, int64_t word_id, int64_t capacity, int64_t* doc_ids, int32_t* tfs, int64_t* count);

/*
 * POSITIONAL LAYER OF THE INVERTED INDEX (nvsm_corpus_index_positions) — DESIGN.md §26
 *
 * Beside every posting (word, document) of nvsm_corpus_index, the word's positions in that document: in-document offsets, 0-based
 * from the document's first token, ascending, tf of them; N int32 in all plus a posting's first entry (P + 1 int32). It replaces no
 * reference function: the reference has no program text for an index; the contract is this one. With the layer, an index and a
 * `use` other than NVSM_INDEX_NEVER, the rounds of nvsm_sdm_rank, nvsm_sdm_pair_counts and list B of nvsm_rank_ensemble_sdm may count
 * their pairs and fill their slabs from the postings of the query words instead of scanning the arena; both forms return THE SAME
 * BITS (NVSM_INDEX_ALWAYS: the postings in every such round; NVSM_INDEX_AUTO: a host rule per round).
 * nvsm_corpus_index_positions needs an index, is synchronous, runs behind everything queued and touches no parameter, optimiser
 * state, RNG state or lazy bookkeeping. On a corpus that has the layer already it only refills `info`. The layout is a function of
 * the corpus alone: a second build gives the same bytes. nvsm_corpus_index_free and nvsm_corpus_upload (a new corpus or NULL) drop
 * the layer with the index; nvsm_corpus_index_positions_free drops the layer alone. nvsm_index_info and nvsm_describe are unchanged
 * by it, and a handle that never calls it allocates and launches exactly what it did before.
 * NVSM_ERR_INVALID_ARGUMENT, each with a sentence, the handle staying usable: a null handle or `count`; no corpus; no index; no
 * layer (nvsm_corpus_positions); a word id outside [0, num_words); a document id outside [0, num_documents).
 * NVSM_ERR_UNSUPPORTED: world_size > 1.
 */
typedef struct {
    int64_t num_positions;        /* N: one per token of the corpus */
    int64_t bytes;                /* HBM the layer holds beyond nvsm_index_info.bytes */
    int32_t reserved[12];
} nvsm_positions_info;
/* info may be NULL */
int nvsm_corpus_index_positions(nvsm_model* m, nvsm_positions_info* info);
/* frees the layer (the index stays); no layer: success */
int nvsm_corpus_index_positions_free(nvsm_model* m);
/* the in-document offsets of word_id in doc_id to the host: *count = tf, 0 when the document does not hold the word, always
 * written; positions [capacity] receives them when capacity >= *count, else nothing else is written and the call returns
 * NVSM_ERR_INVALID_ARGUMENT */
int nvsm_corpus_positions(nvsm_model* m, int64_t word_id, int64_t doc_id, int64_t capacity, int64_t* positions, int64_t* count);

/*
 * Nearest-neighbour search in word, projected-word and document space — the three other things the reference's query
 * library does with the same parameters (py/nvsm/base.py). Semantics, pinned by the reference:
 *   space        NVSM_SPACE_WORDS: the rows of W, dimension word_repr_size — NVSM.related_terms (base.py:325-342) and
 *                term_similarity (:344-353), cosine neighbours of a word among the word rows.
 *                NVSM_SPACE_PROJECTED_WORDS: row w is f(T·W[w] + c·b), dimension entity_repr_size — the vocabulary projected
 *                into document space, which TermBruteforcer (base.py:106-162) searches for the terms closest to a document
 *                vector ("which terms describe this document"); its n-grams of more than one term are nvsm_ngram_search's,
 *                further down. NO batch normalisation;
 *                bias_coefficient and activation mean exactly what they mean in nvsm_rank_options, with the same defaults
 *                and the same quirk (c = 0 is what py/query.py computes; not "fixed" here).
 *                NVSM_SPACE_ENTITIES: the rows of E, dimension entity_repr_size — query_using_projected_query
 *                (base.py:362-430) called with a vector that is not a projected query: documents near a document.
 *   queries      one vector of the searched space's dimension per query, given EITHER as row ids of a source space (ids,
 *                source_space; vectors NULL) OR as host floats [num_queries][dim] (vectors, dim; ids NULL). A source whose
 *                dimension differs from the searched space's is NVSM_ERR_INVALID_ARGUMENT before anything runs, and so are
 *                ids out of range, unknown enums, top_k outside [1, rows of the space], both or neither of ids / vectors.
 *   exclude_self only with row ids of the searched space itself: the query's own row is left out and
 *                counts[q] = min(top_k, rows - 1). Default 0: the reference does not exclude — related_terms returns the
 *                term itself among its 30.
 *   score        NVSM_SIM_COSINE or NVSM_SIM_DOT. A zero row or a zero query has inverse norm 0: score 0, never NaN.
 *   result       as nvsm_rank: the top_k rows by score descending, ties by ASCENDING id; slots beyond counts[q] hold
 *                (-1, -inf); a pure function of the parameters and the arguments (a repeated call returns the same bits).
 * nvsm_neighbors is synchronous and returns host results; it runs behind everything earlier steps have queued (the side
 * streams' tails included) and leaves parameters, optimiser state and the lazy-decay bookkeeping untouched: tables are read
 * through their view, nothing is flushed. The projected vocabulary is produced one slab of at most 64 MB at a time, never as
 * the whole [num_words][entity_repr_size] matrix. Device scratch is allocated by the first call, not by nvsm_create.
 * nvsm_similarity: out[i] = the score of row a[i] against row b[i] of one space for n pairs (term_similarity batched), the
 * same lazy view; in NVSM_SPACE_PROJECTED_WORDS the rows are projected with nvsm_rank_options_default's c and activation.
 */
enum { NVSM_SPACE_WORDS = 0, NVSM_SPACE_PROJECTED_WORDS = 1, NVSM_SPACE_ENTITIES = 2 };
typedef struct {
    const int64_t* ids;           /* [num_queries] host: row ids of source_space, or NULL */
    const float*   vectors;       /* [num_queries][dim] host, or NULL */
    int64_t        num_queries;
    int32_t        source_space;  /* NVSM_SPACE_*: what ids index (ignored with vectors) */
    int32_t        dim;           /* floats per vector (ignored with ids) */
} nvsm_neighbor_queries;
typedef struct {
    int32_t space;                /* NVSM_SPACE_*: the rows searched */
    int32_t similarity;           /* NVSM_SIM_* */
    int32_t top_k;
    int32_t exclude_self;
    float   bias_coefficient;     /* projected words, searched or as the source: as nvsm_rank_options */
    int32_t activation;
    int32_t reserved[6];
} nvsm_neighbor_options;
/* NVSM_SPACE_WORDS, NVSM_SIM_COSINE, top_k 30 (related_terms' default), exclude_self 0, bias_coefficient 1, NVSM_ACT_MODEL */
void nvsm_neighbor_options_default(nvsm_neighbor_options* opt);
/* ids, scores [num_queries][top_k], counts [num_queries], all host */
int nvsm_neighbors(nvsm_model* m, const nvsm_neighbor_queries* queries, const nvsm_neighbor_options* opt,
                   int64_t* ids, float* scores, int64_t* counts);
/* a, b [n] host row ids of `space`; out [n] host */
int nvsm_similarity(nvsm_model* m, int32_t space, const int64_t* a, const int64_t* b, int64_t n, int32_t similarity, float* out);

/*
 * N-grams of terms in document space — TermBruteforcer (py/nvsm/base.py:106-162) with max_ngram_cardinality up to 2: which
 * terms, and which PAIRS of terms, describe a document or a query vector. Semantics, pinned by the reference:
 *   vocabulary   S: vocabulary_size strictly ascending model word ids (host); NULL: all num_words words, which is what the
 *                reference always takes. The subset is this library's addition: C(|V|, 2) phrases fit no other way.
 *   phrase rows  the rows of the reference's np.vstack(reprs): first the m = |S| 1-grams in order, then the 2-grams (a, b),
 *                a < b positions in S, in itertools.combinations order: row of (a, b) = m + a·(2m − a − 1)/2 + (b − a − 1).
 *                R = m rows for max_cardinality 1, m + m(m − 1)/2 for 2 (nvsm_ngram_rows). R must stay below 2^31, the
 *                selection keys' limit, i.e. m <= 65 535 for 2-grams: beyond it NVSM_ERR_UNSUPPORTED before anything runs.
 *   row vector   f(T·mean(W[s_a], W[s_b]) + c·b) — Model::infer of the mean word vector, NO batch normalisation;
 *                bias_coefficient and activation mean exactly what they mean in nvsm_rank_options, the c = 0 quirk included.
 *                Evaluated as f(0.5·(G[a] + G[b]) + c·b) with G[i] = T·W[s_i] computed once per call (the projection is
 *                linear in front of the bias); the 1-gram row is f(G[a] + c·b).
 *   queries      a nvsm_neighbor_queries of dimension entity_repr_size: entity ids, projected-word ids or host vectors; the
 *                dimension rule and the refusals are nvsm_neighbors' (projected-word queries take this call's c and activation).
 *   score        NVSM_SIM_COSINE (the reference's 1 − cosine distance) or NVSM_SIM_DOT; a zero phrase or a zero query scores
 *                0, never NaN.
 *   result       per query the top_k phrase rows by score descending, ties by ASCENDING phrase row; terms[q][j][0 ..
 *                max_cardinality) holds the model word ids of row phrase_rows[q][j], -1 in unused slots (the second of a
 *                1-gram); slots beyond counts[q] hold (-1, -1 ..., -inf). A repeated call returns the same bits.
 * Refused with a status code, in this order, the handle usable afterwards: max_cardinality outside {1, 2}; unknown
 * similarity / activation; a bias_coefficient that is not finite; vocabulary_size < 1 (with a vocabulary), a vocabulary that
 * is not strictly ascending or holds an id outside [0, num_words); the row limit; nvsm_neighbors' query refusals; top_k
 * outside [1, R]. The call is synchronous; it runs behind everything earlier steps have queued (the side streams' tails
 * included), flushes nothing and moves no stamp of a lazily decayed table: training goes on from exactly the same state.
 */
typedef struct {
    int32_t        max_cardinality;   /* 1 or 2 */
    int32_t        similarity;        /* NVSM_SIM_* */
    int32_t        top_k;
    float          bias_coefficient;  /* as nvsm_rank_options */
    int32_t        activation;
    int32_t        reserved0;
    const int64_t* vocabulary;        /* [vocabulary_size] host, strictly ascending word ids, or NULL: every word */
    int64_t        vocabulary_size;   /* ignored with vocabulary NULL */
    int32_t        reserved[4];
} nvsm_ngram_options;
/* max_cardinality 1, NVSM_SIM_COSINE, top_k 20 (the reference's n_neighbors), bias_coefficient 1, NVSM_ACT_MODEL, vocabulary NULL */
void nvsm_ngram_options_default(nvsm_ngram_options* opt);
/* rows of the phrase stack over vocabulary_size words; -1 where that is not below 2^31, for vocabulary_size < 1 and for a
 * max_cardinality outside {1, 2}. Host arithmetic only. */
int64_t nvsm_ngram_rows(int64_t vocabulary_size, int32_t max_cardinality);
/* phrase_rows, scores [num_queries][top_k], terms [num_queries][top_k][max_cardinality], counts [num_queries], all host */
int nvsm_ngram_search(nvsm_model* m, const nvsm_neighbor_queries* queries, const nvsm_ngram_options* opt,
                      int64_t* phrase_rows, int64_t* terms, float* scores, int64_t* counts);

/*
 * Exact t-SNE of document or word rows — what py/visualize.py asks sklearn.manifold.TSNE(n_components=2, init='pca',
 * random_state=0) for, with the EXACT gradient (sklearn's method='exact'; its default is the Barnes-Hut approximation) on the
 * device. Semantics, pinned by scikit-learn 1.7:
 *   rows         ids: num_rows host row ids of `space`, any order (--filter_unclassified passes the sorted indices of the
 *                classified documents), or NULL: rows 0 .. num_rows − 1 (--limit); num_rows 0 with ids NULL: every row.
 *                Gathered through the lazy view; with l2_normalize every row is divided by its norm (a zero row stays zero).
 *   affinities   squared Euclidean distances (fp64 sums rounded to fp32, as sklearn hands them on), sklearn's
 *                _binary_search_perplexity per row in fp64 (at most 100 steps, tolerance 1e-5), then
 *                P = max((C + Cᵀ) / max(ΣC + ΣCᵀ, eps), eps), eps = 2.220446049250313e-16, zero diagonal, stored as fp32.
 *   start        NVSM_TSNE_INIT_PCA: the centred rows on their two leading principal axes, each axis' sign chosen so that its
 *                entry of largest magnitude is positive (svd_flip on V; the lower index on a tie), scaled to a standard
 *                deviation of 1e-4 in the first column. The axes come from an fp64 covariance and a Jacobi eigensolver, NOT
 *                from sklearn's randomised SVD: the start agrees with sklearn's to rounding, not bit for bit.
 *                NVSM_TSNE_INIT_GIVEN: init_embedding as it is (sklearn's 'random' is 1e-4 · standard normal draws).
 *   descent      sklearn's _gradient_descent twice: min(250, max_iter) iterations with momentum 0.5 and P times
 *                early_exaggeration (n_iter_without_progress 250), then up to max_iter with momentum 0.8; gains, update and
 *                the best error start afresh in the second phase. The error is evaluated every 50th iteration of a phase and
 *                on its last; a phase ends when i − best_iter > n_iter_without_progress or the norm of the gain-scaled gradient
 *                is <= min_grad_norm. Y is never re-centred.
 *   result       kl_divergence: the error of the last evaluation (sklearn's kl_divergence_); n_iter: the index of the last
 *                iteration that ran (sklearn's n_iter_: max_iter − 1 for a run that max_iter ends). Where the second phase has
 *                no iteration left (max_iter <= 250, which sklearn refuses) both are the first phase's.
 * NVSM_SPACE_PROJECTED_WORDS is not served: a caller can project words with nvsm_neighbors' machinery but pass no vectors through
 * this call yet.
 * Refused with a status code before anything runs, in this order, the handle usable afterwards: a space other than entities or
 * words; num_rows < 2 (after the default is resolved) or, with ids NULL, beyond the space's rows; an id out of range; num_rows >
 * NVSM_TSNE_MAX_ROWS (NVSM_ERR_UNSUPPORTED); a perplexity that is not finite, not positive or not below num_rows; a non-finite or
 * non-positive early_exaggeration; a non-finite learning_rate, min_grad_norm or init_embedding entry; max_iter < 1 or
 * n_iter_without_progress < 0; an unknown init, or NVSM_TSNE_INIT_GIVEN without an array. Rows that are all identical have no
 * principal axes: NVSM_TSNE_INIT_PCA then fails with NVSM_ERR_INVALID_ARGUMENT.
 * The call is synchronous; it runs behind everything earlier steps have queued (the side streams' tails included), flushes
 * nothing and moves no stamp of a lazily decayed table: training goes on from exactly the same state. A repeated call returns
 * the same bits. Device scratch (n² floats for P) is allocated by the first call and grown by a later one with more rows.
 */
#define NVSM_TSNE_MAX_ROWS 32768          /* P is n*n floats: 4 GiB at the cap */
enum { NVSM_TSNE_INIT_PCA = 0, NVSM_TSNE_INIT_GIVEN = 1 };
typedef struct {
    int32_t        space;                    /* NVSM_SPACE_ENTITIES (visualize.py) or NVSM_SPACE_WORDS */
    int32_t        l2_normalize;             /* --l2_normalize */
    const int64_t* ids;                      /* [num_rows] host row ids, any order, or NULL: rows 0 .. num_rows-1 (--limit) */
    int64_t        num_rows;
    float          perplexity;               /* 30 */
    float          early_exaggeration;       /* 12 */
    float          learning_rate;            /* <= 0: sklearn's 'auto', max(n / early_exaggeration / 4, 50) */
    float          min_grad_norm;            /* 1e-7 */
    int32_t        max_iter;                 /* 1000; >= 1 (exploration = min(250, max_iter)) */
    int32_t        n_iter_without_progress;  /* 300 */
    int32_t        init;                     /* NVSM_TSNE_INIT_* */
    int32_t        reserved0;
    const float*   init_embedding;           /* [num_rows][2] host, with NVSM_TSNE_INIT_GIVEN */
    int32_t        reserved[6];
} nvsm_tsne_options;
/* entities, no normalisation, ids NULL, num_rows 0 = every row, the values above, PCA */
void nvsm_tsne_options_default(nvsm_tsne_options* opt);
/* embedding [num_rows][2] host; kl_divergence and n_iter as sklearn's kl_divergence_ and n_iter_ */
int nvsm_tsne(nvsm_model* m, const nvsm_tsne_options* opt, float* embedding, double* kl_divergence, int32_t* n_iter);

/*
 * Sparse-affinity t-SNE of document or word rows, for collections beyond NVSM_TSNE_MAX_ROWS: sklearn.manifold.TSNE with its
 * default method='barnes_hut' at angle = 0, where the tree summarises nothing and the repulsion is the exact sum over all
 * pairs. No n × n values are held: the affinities take O(n · n_neighbors) memory and the repulsion reads the embedding alone.
 * Rows, normalisation, start, descent, results and synchrony are nvsm_tsne's (same options struct). What differs, pinned by
 * scikit-learn 1.7 (sklearn/manifold/_t_sne.py):
 *   neighbours   k = n_neighbors, or with 0 sklearn's min(n − 1, int(3 · perplexity + 1)) (TSNE._fit). Per row the k OTHER rows of
 *                smallest squared Euclidean distance (nvsm_tsne's distance: an fp64 sum rounded to fp32), ties by ascending row
 *                id. A row is never its own neighbour; a duplicate of it is one, at distance 0.
 *   affinities   _binary_search_perplexity over each row's k distances in fp64, stored as fp32; _joint_probabilities_nn:
 *                P = (C + Cᵀ) / max(ΣC + ΣCᵀ, eps) as a CSR matrix over the union of both directions of every edge, with no
 *                clamp per cell (the sparse path has none), no diagonal, columns ascending, P_ij and P_ji the same bits.
 *   gradient     _kl_divergence_bh at angle 0: g_i = 4·(e·Σ_{j stored} P_ij q_ij (y_i − y_j) − Σ_{j != i} q_ij² (y_i − y_j) / Z),
 *                q = 1 / (1 + |y_i − y_j|²), Z = Σ_{i != j} q_ij over all pairs.
 *   error        Σ_{stored} e·P_ij · log(max(e·P_ij, tiny) / max(q_ij / Z, tiny)), tiny = FLT_MIN (_barnes_hut_tsne.pyx), in fp64
 *                throughout and with an fp64 Z of its own, as nvsm_tsne's: a check costs one more pass over all pairs.
 * Refused as nvsm_tsne refuses and in its order, with these changes: the row limit is NVSM_TSNE_SPARSE_MAX_ROWS
 * (NVSM_ERR_UNSUPPORTED); behind all of nvsm_tsne's checks, n_neighbors outside [1, min(num_rows − 1, NVSM_TSNE_SPARSE_MAX_NEIGHBORS)]
 * is NVSM_ERR_INVALID_ARGUMENT, a default k above NVSM_TSNE_SPARSE_MAX_NEIGHBORS is NVSM_ERR_UNSUPPORTED, and so is
 * 2 · num_rows · k >= 2^31 (the directed entries are numbered in 32 bits).
 * A repeated call returns the same bits. Device scratch is allocated by the first call and grown by a later, larger one.
 */
#define NVSM_TSNE_SPARSE_MAX_ROWS 1048576     /* row ids fit 20 bits: two passes of the 32-bit pair sort order (row, column) */
#define NVSM_TSNE_SPARSE_MAX_NEIGHBORS 1024   /* perplexity up to 341 */
typedef struct {
    int32_t n_neighbors;                     /* 0: sklearn's min(n - 1, int(3 * perplexity + 1)) */
    int32_t reserved[7];
} nvsm_tsne_sparse_options;
void nvsm_tsne_sparse_options_default(nvsm_tsne_sparse_options* opt);      /* n_neighbors 0 */
/* sparse: NULL = the defaults; embedding, kl_divergence and n_iter as nvsm_tsne's */
int nvsm_tsne_sparse(nvsm_model* m, const nvsm_tsne_options* opt, const nvsm_tsne_sparse_options* sparse, float* embedding,
                     double* kl_divergence, int32_t* n_iter);

/*
 * k-means (Lloyd's algorithm) of document or word rows on the device — what a caller would otherwise ask
 * sklearn.cluster.KMeans(n_clusters=k, n_init=1, algorithm='lloyd') for after pulling the table to the host. Semantics, pinned by
 * scikit-learn 1.7 where it specifies them:
 *   rows         nvsm_tsne_options' selection: ids (num_rows host row ids of `space`, any order, duplicates allowed), or NULL: rows
 *                0 .. num_rows − 1; num_rows 0 with ids NULL: every row. Gathered through the lazy view; with l2_normalize every
 *                row is divided by its norm (a zero row stays zero). X below is these rows, fp32.
 *   assignment   label[i] = the j that minimises |x_i − c_j|² in the kernel's arithmetic, the lowest j on a tie. The kernel evaluates
 *                |x|² − 2 x·c + |c|² in fp32 on rows and centres centred by the column mean of X (an fp64 sum rounded to fp32), as
 *                sklearn centres X: without that the cancellation is not fp32-accurate for rows far from the origin.
 *   empty        settled before the sums are taken: empty clusters in ascending id each take the row with the largest squared
 *                distance (direct fp64) to the centre it is assigned to, the lower row position on a tie, among rows whose cluster
 *                has at least two members at that moment; counts are updated as it goes and the row's label CHANGES. (sklearn
 *                relocates the same kind of rows but hands them out in argpartition's unspecified order and keeps the labels.)
 *   update       c_j = fp32((Σ_{label i = j} x_i) / count_j), the sum in fp64 over the fp32 rows as gathered (not the centred
 *                copy), in an order that depends on the member count and ascending row position alone. No float atomics.
 *   stopping     sklearn's _kmeans_single_lloyd: stop at iteration i when its labels equal those of iteration i − 1 ("strict"),
 *                or when the fp64 sum of squared centre shifts is <= tol · mean_c(var(X[:, c])) (fp64 population variances);
 *                n_iter is the number of iterations run. After a stop that was not strict — max_iter included — one more
 *                assignment pass runs against the final centres (no relocation). labels, counts, distances and inertia describe
 *                that final assignment; centers are the last update's.
 *   inertia      an fp64 sum in a fixed order of directly evaluated fp64 (x − c)²; distances[i] = the fp32 rounding of row i's.
 *   k-means++    u_t = (x_t − 1) / 2147483646.0 in fp64, x_t the t-th output (t = 0, 1, …) of std::minstd_rand0(seed). Centre 0 is
 *                row floor(u_0 · n). Centre t is the lowest row position p whose inclusive fp64 prefix sum, over ascending
 *                positions, of min_{s<t} |x_p − c_s|² (direct fp64) exceeds u_t · total; where total is 0, the lowest position not
 *                yet chosen. ONE candidate per draw: sklearn's greedy local trials (2 + log k candidates, the best kept) are NOT
 *                reproduced, so a seed does not give sklearn's start.
 *                NVSM_KMEANS_INIT_GIVEN: init_centers as they are.
 * Out of scope: spherical k-means, mini-batches, n_init > 1 (loop over seeds and keep the lowest inertia),
 * NVSM_SPACE_PROJECTED_WORDS, world_size > 1.
 * Refused with a status code before anything runs, in this order, nothing written to the outputs, the handle usable afterwards:
 * a space other than entities or words; num_rows < 1 (after the default is resolved) or, with ids NULL, beyond the space's rows;
 * an id out of range; num_clusters < 1 or > num_rows; num_clusters > NVSM_KMEANS_MAX_CLUSTERS (NVSM_ERR_UNSUPPORTED); max_iter < 1;
 * a tol that is negative or not finite; an unknown init; NVSM_KMEANS_INIT_GIVEN without an array or with an entry that is not
 * finite; seed < 1 with NVSM_KMEANS_INIT_PLUSPLUS.
 * Every dimension the model accepts is served by the same matrix-pipe kernel. The call is synchronous; it runs behind everything
 * earlier steps have queued (the side streams' tails included), flushes nothing and moves no stamp of a lazily decayed table, and
 * touches no parameter, optimiser state or RNG state: training goes on from exactly the same state. A repeated call returns the
 * same bits. Device scratch (the gathered rows and a few arrays of n or k entries) is allocated by the first call and grown later.
 */
#define NVSM_KMEANS_MAX_CLUSTERS 4096     /* the chunk scan of the update is one workgroup and k-means++ costs a host round trip per centre */
enum { NVSM_KMEANS_INIT_PLUSPLUS = 0, NVSM_KMEANS_INIT_GIVEN = 1 };
typedef struct {
    int32_t        space;                    /* NVSM_SPACE_ENTITIES or NVSM_SPACE_WORDS */
    int32_t        l2_normalize;
    const int64_t* ids;                      /* [num_rows] host row ids, any order, or NULL: rows 0 .. num_rows-1 */
    int64_t        num_rows;
    int32_t        num_clusters;             /* k: 1 .. min(num_rows, NVSM_KMEANS_MAX_CLUSTERS) */
    int32_t        max_iter;                 /* 300 */
    double         tol;                      /* 1e-4, relative to the mean column variance */
    int32_t        init;                     /* NVSM_KMEANS_INIT_* */
    int32_t        reserved0;
    const float*   init_centers;             /* [num_clusters][dim] host, with NVSM_KMEANS_INIT_GIVEN */
    int64_t        seed;                     /* >= 1 with NVSM_KMEANS_INIT_PLUSPLUS */
    int32_t        reserved[6];
} nvsm_kmeans_options;
/* entities, no normalisation, ids NULL, num_rows 0 = every row, num_clusters 8, max_iter 300, tol 1e-4, k-means++, seed 1 */
void nvsm_kmeans_options_default(nvsm_kmeans_options* opt);
/* labels [num_rows], centers [k][dim], counts [k], distances [num_rows] (may be NULL): host */
int nvsm_kmeans(nvsm_model* m, const nvsm_kmeans_options* opt, int32_t* labels, float* centers, int64_t* counts, float* distances,
                double* inertia, int32_t* n_iter);

/* Streams. A handle issues its work on FOUR HIP streams of its own device: the main stream (highest priority: the step's
 * critical chain), two side streams (lowest priority: the batch → row-order sorts, and — in nvsm_step — the documents
 * update and the ∂T GEMM + projection update, which keep running after nvsm_step has returned and are joined by the next
 * step where it needs their results) and a copy stream (host batches → HBM). The reference collapses to one stream,
 * cpp/model.cu:13-14. nvsm_set_stream replaces the MAIN stream only (the caller's stream keeps its own priority; the
 * side streams still order themselves against it with events); NULL = a fresh highest-priority stream of the handle's
 * own. nvsm_synchronize waits for all four and reports any error a kernel has flagged since the last wait. */
int nvsm_set_stream(nvsm_model* m, void* hip_stream);
int nvsm_synchronize(nvsm_model* m);
/* One line of text: which kernel each of a step's three projection products takes at `batch` windows on this handle, where the
 * dT product and the CSR builds run, whether the tables decay lazily, and every NVSM_* switch that is off its default (the
 * switches are read from the environment ONCE, by nvsm_create: INTEGRATION.md §6). No reference counterpart. */
int nvsm_describe(nvsm_model* m, int64_t batch, char* buf, int64_t buf_bytes);

/* Data parallelism over RCCL / xGMI: one all-reduce of [grad_transform | grad_bias] per
 * step (+ two of the batch-norm statistics when sync_batch_norm). The 128-byte id is ncclUniqueId.
 * SEMANTICS — read before training with world_size > 1: only the dense projection, its bias and the batch-norm
 * statistics are reduced; the word and document tables (and their optimiser state) are updated from each rank's own
 * shard ("sparse embedding rows stay GPU-local"), so the replicas of the tables drift apart and an N-rank run does
 * NOT follow the single-GPU trajectory (the loss and the dense gradients of a step given equal tables do, exactly).
 * nvsm_dp_average_tables replaces every replica's tables by their mean over the ranks; cuNVSMTrainModel calls it at the
 * end of every epoch and before every model dump, so that what rank 0 writes carries every rank's updates. A caller
 * that checkpoints one rank without it drops the other ranks' embedding updates.
 * EXACT TABLES (nvsm_config.dp_exact_tables = 1): the window ids, document ids, projected phrases, multipliers and phrase
 * gradients of every rank are all-gathered (ncclAllGather on the main stream, 2 x B x (d_e + d_w) floats per rank and step)
 * and every rank runs the table updates of the whole global batch in rank order — exactly the single-GPU update on the
 * concatenated batch, so the tables of all ranks are bit-identical after every step and equal the single-GPU tables up to the
 * summation order of the all-reduced dense statistics. Every rank must pass the same num_instances and agree on whether
 * feature_weights is NULL. The step's collectives all run on the main stream in this mode, the table passes are not
 * overlapped with the backward products, and nvsm_dp_average_tables has nothing to do (it returns at once). The update work
 * per rank is that of the global batch: the mode buys the single-GPU trajectory, not update throughput.
 * nvsm_get_cost with world_size > 1 is a collective when called before nvsm_compute_gradients (it all-reduces a copy of
 * the loss word); every rank must make the same sequence of calls.
 * NEGATIVES with world_size > 1: rank r is taken to hold instances [r·B, (r+1)·B) of a global batch of world_size·B.
 * NVSM_SAMPLER_HOST_MINSTD: every rank replays the draws of the WHOLE global batch from its copy of the shared generator
 * (nvsm_rng_set_state: the same state on every rank, as cuNVSMTrainModel hands it over) and keeps its own slice's — the
 * negatives of an instance are those of the single-GPU run, ranks never share a negative set, and the generator states
 * stay equal across ranks (world_size x the host draws per rank: this is the parity sampler). NVSM_SAMPLER_DEVICE: the
 * counter-based sampler is keyed by (seed, rank, step, slot), so ranks draw independent streams. */
int nvsm_comm_unique_id(char id[128]);
int nvsm_comm_init(nvsm_model* m, const char id[128]);
/* ncclCommCount of the handle's communicator (0 = none was built) */
int nvsm_comm_size(nvsm_model* m, int* ranks);
/* collective: W, E ← mean over ranks (synchronises the handle) */
int nvsm_dp_average_tables(nvsm_model* m);
/* Alternative transport for tests: the library hands a HOST double buffer to the callback, which must
 * sum it in place across ranks (e.g. torch.distributed gloo). */
typedef int (*nvsm_allreduce_fn)(double* host_buf, int64_t count, void* user);
int nvsm_set_allreduce_callback(nvsm_model* m, nvsm_allreduce_fn fn, void* user);
/* Single-process check of the RCCL plumbing (dlopen, symbols, enum values, stream use): builds a 1-rank communicator
 * on `device` and all-reduces an f32 and an f64 buffer through the same code path nvsm_step uses with world_size > 1. */
int nvsm_comm_selftest(int device);
/* The three collectives of a data-parallel step (all-reduce of [Σx | Σx²]: 2·entity_dim doubles; of [loss | Σdy | Σdy·x̂]:
 * 1 + 2·entity_dim doubles; of the projection gradient: entity_dim·word_dim floats) on a 1-rank communicator, each on a stream of
 * its own, `repeats` times back to back: average microseconds per call in us[0..2] and the payload bytes in bytes[0..2] — the
 * latency floor of each collective on this GPU (what a rank of the N-GPU job pays per step before any wire time), for
 * bench.py's `--gpus 1` line. */
int nvsm_comm_latency(int device, int entity_dim, int word_dim, int repeats, float us[3], int64_t bytes[3]);

/* Per-kernel timing of the hot path, measured with HIP events on the handle's stream (bench.py's
 * roofline leg). enable=1 records around every launch of subsequent steps (adds sync points at
 * read-out only). nvsm_profile_get returns accumulated milliseconds and launch counts per kernel name;
 * names are listed by nvsm_profile_names (NUL-separated, double-NUL terminated). The ~50 event records of a fully
 * profiled step cost ≈5 % of its time (measured); nvsm_profile_select(names) restricts recording to the comma-separated kernel groups
 * (NULL or "" = all) so that a timed region can carry the roofline kernel's events only. */
int nvsm_profile_enable(nvsm_model* m, int enable);
int nvsm_profile_select(nvsm_model* m, const char* kernel);
int nvsm_profile_reset(nvsm_model* m);
int nvsm_profile_names(nvsm_model* m, char* buf, int64_t buf_bytes);
int nvsm_profile_get(nvsm_model* m, const char* kernel, double* total_ms, int64_t* launches);

/* roctx ranges (the reference's nvtxRangePush / nvtxRangePop, cpp/main.cu:386-431): forwarded to
 * librocprofiler-sdk-roctx when it can be loaded, no-ops otherwise. The library itself brackets ComputeCost /
 * ComputeGradients / UpdateParameters and every kernel group; the trainer adds Epoch / Batch / FetchData. */
void nvsm_range_push(const char* name);
void nvsm_range_pop(void);

/* (The unit-test hooks for single kernels — nvsm_debug_* — are NOT in this library: include/cunvsm_amd_test_hooks.h,
 * libcunvsm_amd_testhooks.so.) */

#ifdef __cplusplus
}
#endif
#endif /* CUNVSM_AMD_H */
