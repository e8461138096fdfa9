// C++ host-side wrapper over the C ABI (include/cunvsm_amd.h) with the shape of cuNVSM's
// Model<TextEntity::Objective> (include/cuNVSM/model.h:75-131): what a maintainer of the reference would
// instantiate in cpp/main.cu:515-520 instead of `Model<ObjectiveT>`. Header-only; link -lcunvsm_amd.
//
//   reference                                         here
//   Model(num_words, num_entities, desc, train_cfg)   cunvsm_amd::Model(nvsm_config)
//   model.initialize(&rng)                            model.initialize(seed)   |   model.initialize(rng) with the caller's
//                                                     std::minstd_rand0, whose state is handed over and taken back
//   ForwardResult* r = model.compute_cost(batch,&rng) model.compute_cost(batch)            (result lives in the handle)
//   Gradients* g = model.compute_gradients(*r)        model.compute_gradients()
//   model.update(*g, lr, r->scaled_regularization_lambda())   model.update(lr, model.scaled_regularization_lambda())
//   r->get_cost()                                     model.get_cost()
//   model.get_data()                                  model.get_data()
//
// Error behaviour: the reference CHECK()s and aborts; here every failure throws cunvsm_amd::Error carrying the
// nvsm_status (never aborts the process).
#pragma once

#include <map>
#include <random>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../cunvsm_amd.h"

namespace cunvsm_amd {

struct Error : std::runtime_error {
    int status;
    Error(int st, const char* what) : std::runtime_error(what), status(st) {}
};

inline void check(int st) {
    if (st != NVSM_OK) throw Error(st, nvsm_last_error());
}

// TextEntity::Batch (include/cuNVSM/data.h:114-177) — a view over the caller's four arrays.
struct Batch {
    nvsm_batch raw{};
    Batch(const int64_t* features, const float* feature_weights, const int64_t* labels, const float* weights,
          int64_t num_instances, bool on_device = false) {
        raw.features = features; raw.feature_weights = feature_weights; raw.labels = labels; raw.weights = weights;
        raw.num_instances = num_instances; raw.on_device = on_device ? 1 : 0;
    }
    int64_t num_instances() const { return raw.num_instances; }
};

// RepresentationSimilarity::Batch (cpp/data.cu:316-334) — a view over the caller's interleaved pair ids and optional weights.
struct PairBatch {
    nvsm_pair_batch raw{};
    PairBatch(const int64_t* pairs, const float* weights, int64_t num_pairs, bool on_device = false) {
        raw.pairs = pairs; raw.weights = weights; raw.num_pairs = num_pairs; raw.on_device = on_device ? 1 : 0;
    }
    int64_t num_pairs() const { return raw.num_pairs; }
};

class Model {
 public:
    explicit Model(const nvsm_config& cfg) : cfg_(cfg) { check(nvsm_create(&cfg, &h_)); }
    ~Model() { nvsm_destroy(h_); }
    Model(const Model&) = delete;
    Model& operator=(const Model&) = delete;

    void initialize(uint64_t seed) { check(nvsm_initialize(h_, seed)); }
    // model.initialize(&rng) (cpp/model.cu:37-43) with the reference's own generator object: the Glorot draws continue
    // from *rng's state and *rng is advanced past them, exactly as if the reference had consumed it (cpp/main.cu:520)
    void initialize(std::minstd_rand0* rng) {
        check(nvsm_rng_set_state(h_, state_of(*rng)));
        check(nvsm_initialize_from_rng_state(h_));
        sync_rng(rng);
    }
    // after compute_cost with the host sampler: advance the caller's generator past the negatives that were drawn
    void sync_rng(std::minstd_rand0* rng) {
        uint64_t s = 0;
        check(nvsm_rng_get_state(h_, &s));
        std::stringstream ss; ss << s; ss >> *rng;
    }
    void push_rng(const std::minstd_rand0& rng) { check(nvsm_rng_set_state(h_, state_of(rng))); }

    // entity_ids: optional output of the caller's own label generator; nullptr = sample as configured
    void compute_cost(const Batch& batch, const int64_t* entity_ids = nullptr) { check(nvsm_compute_cost(h_, &batch.raw, entity_ids)); }
    void compute_gradients() { check(nvsm_compute_gradients(h_)); }
    void update(float learning_rate, float scaled_regularization_lambda) { check(nvsm_update(h_, learning_rate, scaled_regularization_lambda)); }
    float get_cost() { float c = 0.f; check(nvsm_get_cost(h_, &c)); return c; }
    float scaled_regularization_lambda() { return nvsm_scaled_regularization_lambda(h_); }
    // backprop(result, lr) (cpp/model.cu:176-185)
    void backprop(float learning_rate) { compute_gradients(); update(learning_rate, scaled_regularization_lambda()); }
    // one iterate_data loop body (cpp/main.cu:400-444)
    float step(const Batch& batch, float learning_rate, bool want_cost = true) {
        float c = 0.f;
        check(nvsm_step(h_, &batch.raw, nullptr, learning_rate, want_cost ? &c : nullptr));
        return c;
    }

    // document fold-in (nvsm_step_fold): compute_cost, then the documents update on rows [first_document, num_entities) alone
    float step_fold(const Batch& batch, float learning_rate, int64_t first_document, bool want_cost = true) {
        nvsm_fold_options opt;
        nvsm_fold_options_default(&opt);
        opt.first_document = first_document;
        float c = 0.f;
        check(nvsm_step_fold(h_, &batch.raw, nullptr, &opt, learning_rate, want_cost ? &c : nullptr));
        return c;
    }

    // the entity-entity similarity objective mixed into the text objective with weights (text_weight, pair_weight)
    // (TextEntityEntityEntity, cpp/objective.cu:698-745), or alone (text == nullptr): compute_gradients / update / get_cost follow
    void compute_cost_mixed(const Batch* text, const PairBatch& pairs, float text_weight = 0.5f, float pair_weight = 0.5f,
                            const int64_t* entity_ids = nullptr) {
        nvsm_mixture mix{};
        mix.text_weight = text_weight; mix.pair_weight = pair_weight;
        check(nvsm_compute_cost_mixed(h_, text ? &text->raw : nullptr, entity_ids, &pairs.raw, &mix));
    }
    float step_mixed(const Batch* text, const PairBatch& pairs, float learning_rate, float text_weight = 0.5f, float pair_weight = 0.5f,
                     bool want_cost = true) {
        nvsm_mixture mix{};
        mix.text_weight = text_weight; mix.pair_weight = pair_weight;
        float c = 0.f;
        check(nvsm_step_mixed(h_, text ? &text->raw : nullptr, nullptr, &pairs.raw, &mix, learning_rate, want_cost ? &c : nullptr));
        return c;
    }
    // the term-term similarity objective on the words table (TextEntityTermTerm, cpp/objective.cu:747-794): `pairs` holds model word
    // ids, pair_weight is w_tt; alone with text == nullptr
    void compute_cost_term_mixed(const Batch* text, const PairBatch& pairs, float text_weight = 0.5f, float pair_weight = 0.5f,
                                 const int64_t* entity_ids = nullptr) {
        nvsm_mixture mix{};
        mix.text_weight = text_weight; mix.pair_weight = pair_weight;
        check(nvsm_compute_cost_term_mixed(h_, text ? &text->raw : nullptr, entity_ids, &pairs.raw, &mix));
    }
    float step_term_mixed(const Batch* text, const PairBatch& pairs, float learning_rate, float text_weight = 0.5f, float pair_weight = 0.5f,
                          bool want_cost = true) {
        nvsm_mixture mix{};
        mix.text_weight = text_weight; mix.pair_weight = pair_weight;
        float c = 0.f;
        check(nvsm_step_term_mixed(h_, text ? &text->raw : nullptr, nullptr, &pairs.raw, &mix, learning_rate, want_cost ? &c : nullptr));
        return c;
    }

    // training from an HBM-resident corpus (cunvsm_amd.h): the corpus goes to the device once, a batch is then [n] window
    // references — (document, first token inside the document) as interleaved uint32, 8 bytes per window — and every call below
    // equals its Batch twin on the batch the references denote bit for bit. upload_corpus(nullptr) frees the corpus.
    void upload_corpus(const nvsm_corpus* corpus) { check(nvsm_corpus_upload(h_, corpus)); }
    static nvsm_window_batch windows_of(const uint32_t* refs, int64_t num_instances, bool on_device = false) {
        nvsm_window_batch wb{};
        wb.refs = refs; wb.num_instances = num_instances; wb.on_device = on_device ? 1 : 0;
        return wb;
    }
    void compute_cost_windows(const nvsm_window_batch& windows, const int64_t* entity_ids = nullptr) {
        check(nvsm_compute_cost_windows(h_, &windows, entity_ids));
    }
    float step_windows(const nvsm_window_batch& windows, float learning_rate, bool want_cost = true) {
        float c = 0.f;
        check(nvsm_step_windows(h_, &windows, nullptr, learning_rate, want_cost ? &c : nullptr));
        return c;
    }
    int64_t step_windows_deferred(const nvsm_window_batch& windows, float learning_rate) {
        int64_t t = 0;
        check(nvsm_step_windows_deferred(h_, &windows, nullptr, learning_rate, &t));
        return t;
    }

    // the same loop body with the loss read back one step late (cpp/main.cu:427-444 without the per-step stall):
    //   wait_inputs(); refill the host batch; t = step_deferred(batch, lr); cost of the PREVIOUS step = deferred_cost(t_prev)
    int64_t step_deferred(const Batch& batch, float learning_rate) {
        int64_t t = 0;
        check(nvsm_step_deferred(h_, &batch.raw, nullptr, learning_rate, &t));
        return t;
    }
    float deferred_cost(int64_t ticket) { float c = 0.f; check(nvsm_deferred_cost(h_, ticket, &c)); return c; }
    void wait_inputs() { check(nvsm_wait_inputs(h_)); }

    // ModelBase::get_data() (cpp/model.cu:64-93): name → host copy, in the layout write_to_hdf5 expects
    std::map<std::string, std::vector<float>> get_data() {
        static const char* names[] = {"word_representations-representations", "entity_representations-representations",
                                      "word_entity_mapping-transform", "word_entity_mapping-bias"};
        std::map<std::string, std::vector<float>> out;
        for (const char* n : names) {
            int64_t cnt = 0;
            check(nvsm_param_size(h_, n, &cnt));
            std::vector<float> v(static_cast<size_t>(cnt));
            check(nvsm_get_param(h_, n, v.data(), cnt));
            out.emplace(n, std::move(v));
        }
        return out;
    }
    // rows [first_row, first_row + rows) of an embedding table or of its per-row optimiser state; v holds rows x width floats
    void get_param_rows(const std::string& name, int64_t first_row, int64_t rows, std::vector<float>* v) { check(nvsm_get_param_rows(h_, name.c_str(), first_row, rows, v->data())); }
    void set_param_rows(const std::string& name, int64_t first_row, int64_t rows, const std::vector<float>& v) { check(nvsm_set_param_rows(h_, name.c_str(), first_row, rows, v.data())); }
    void set_param(const std::string& name, const std::vector<float>& v) { check(nvsm_set_param(h_, name.c_str(), v.data(), static_cast<int64_t>(v.size()))); }

    // Storage::increment_parameter (cpp/storage.cu:123-131) — the gradient checker's poke
    void increment_parameter(const std::string& name, int64_t index, float epsilon) { check(nvsm_increment_parameter(h_, name.c_str(), index, epsilon)); }
    double get_cost_f64() { double c = 0.0; check(nvsm_get_cost_f64(h_, &c)); return c; }

    // Model::infer (cpp/model.cu:105-133) for ragged queries: word ids of query q are word_ids[offsets[q] .. offsets[q + 1]);
    // returns [num_queries][entity_repr_size]. opt == nullptr: nvsm_rank_options_default (c = 1, the model's nonlinearity).
    std::vector<float> infer(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets,
                             const std::vector<float>* word_weights = nullptr, const nvsm_rank_options* opt = nullptr) {
        nvsm_rank_options o;
        if (opt) o = *opt; else nvsm_rank_options_default(&o);
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        std::vector<float> out(static_cast<size_t>(q.num_queries) * static_cast<size_t>(cfg_.entity_repr_size));
        check(nvsm_infer(h_, &q, &o, out.data()));
        return out;
    }
    // the ranking of py/nvsm/base.py:362-430: the opt.top_k best documents per query, score descending, ties by ascending id
    struct Ranking { std::vector<int64_t> doc_ids; std::vector<float> scores; std::vector<int64_t> counts; int32_t top_k; };
    Ranking rank(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_rank_options& opt,
                 const std::vector<float>* word_weights = nullptr) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        Ranking r;
        r.top_k = opt.top_k;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        r.doc_ids.resize(n ? n : 1); r.scores.resize(n ? n : 1); r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_rank(h_, &q, &opt, r.doc_ids.data(), r.scores.data(), r.counts.data()));
        r.doc_ids.resize(n); r.scores.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    // nvsm_evaluate: the same ranking plus, per query, NVSM_EVAL_FIXED + 3 * judgments.num_cutoffs metrics computed on the device
    // (layout and formulas: cunvsm_amd.h). with_ranking false: only the metrics come back from the device.
    struct Evaluation { std::vector<double> metrics; int32_t width; Ranking ranking; };
    Evaluation evaluate(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_rank_options& opt,
                        const nvsm_judgments& judgments, const std::vector<float>* word_weights = nullptr, bool with_ranking = true) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        Evaluation e;
        e.width = NVSM_EVAL_FIXED + 3 * (judgments.num_cutoffs > 0 ? judgments.num_cutoffs : 0);
        e.ranking.top_k = opt.top_k;
        const size_t Q = static_cast<size_t>(q.num_queries);
        const size_t n = with_ranking ? Q * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0) : 0;
        e.metrics.resize(Q * static_cast<size_t>(e.width) + 1);
        if (with_ranking) { e.ranking.doc_ids.resize(n ? n : 1); e.ranking.scores.resize(n ? n : 1); e.ranking.counts.resize(Q + 1); }
        check(nvsm_evaluate(h_, &q, &opt, &judgments, e.metrics.data(), with_ranking ? e.ranking.doc_ids.data() : nullptr,
                            with_ranking ? e.ranking.scores.data() : nullptr, with_ranking ? e.ranking.counts.data() : nullptr));
        e.metrics.resize(Q * static_cast<size_t>(e.width));
        if (with_ranking) { e.ranking.doc_ids.resize(n); e.ranking.scores.resize(n); e.ranking.counts.resize(Q); }
        return e;
    }

    // nvsm_lexical_rank: query-likelihood ranking over the uploaded corpus (cunvsm_amd.h has the model); a Ranking as rank() returns
    Ranking lexical_rank(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_lexical_options& lex) {
        const nvsm_queries q = queries_of(word_ids, offsets, nullptr);
        Ranking r;
        r.top_k = lex.top_k;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(lex.top_k > 0 ? lex.top_k : 0);
        r.doc_ids.resize(n ? n : 1); r.scores.resize(n ? n : 1); r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_lexical_rank(h_, &q, &lex, r.doc_ids.data(), r.scores.data(), r.counts.data()));
        r.doc_ids.resize(n); r.scores.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    // nvsm_rank_ensemble: rank()'s and lexical_rank()'s lists fused; the ranking is [num_queries][2 * top_k] (its top_k field says
    // 2 * top_k). judgments null: no metrics (width 0).
    Evaluation rank_ensemble(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_rank_options& opt,
                             const nvsm_lexical_options& lex, const nvsm_ensemble_options& ens, const nvsm_judgments* judgments = nullptr,
                             const std::vector<float>* word_weights = nullptr) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        Evaluation e;
        e.width = judgments ? NVSM_EVAL_FIXED + 3 * (judgments->num_cutoffs > 0 ? judgments->num_cutoffs : 0) : 0;
        e.ranking.top_k = 2 * opt.top_k;
        const size_t Q = static_cast<size_t>(q.num_queries);
        const size_t n = Q * 2 * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        e.metrics.resize(Q * static_cast<size_t>(e.width) + 1);
        e.ranking.doc_ids.resize(n ? n : 1); e.ranking.scores.resize(n ? n : 1); e.ranking.counts.resize(Q + 1);
        check(nvsm_rank_ensemble(h_, &q, &opt, &lex, &ens, judgments, judgments ? e.metrics.data() : nullptr, e.ranking.doc_ids.data(),
                                 e.ranking.scores.data(), e.ranking.counts.data()));
        e.metrics.resize(Q * static_cast<size_t>(e.width));
        e.ranking.doc_ids.resize(n); e.ranking.scores.resize(n); e.ranking.counts.resize(Q);
        return e;
    }

    // nvsm_tfidf_rank: TF-IDF / BM25 ranking over the uploaded corpus (cunvsm_amd.h has the formula); word_weights null: every weight 1
    Ranking tfidf_rank(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_tfidf_options& opt,
                       const std::vector<float>* word_weights = nullptr) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        Ranking r;
        r.top_k = opt.top_k;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        r.doc_ids.resize(n ? n : 1); r.scores.resize(n ? n : 1); r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_tfidf_rank(h_, &q, &opt, r.doc_ids.data(), r.scores.data(), r.counts.data()));
        r.doc_ids.resize(n); r.scores.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    // the inverted index of the uploaded corpus (cunvsm_amd.h nvsm_corpus_index): built once, a later call only sets `use`; the
    // lexical rankings return the same bits whichever fill they take
    nvsm_index_info index_corpus(int32_t use = NVSM_INDEX_AUTO) {
        nvsm_index_options opt;
        nvsm_index_options_default(&opt);
        opt.use = use;
        nvsm_index_info info;
        check(nvsm_corpus_index(h_, &opt, &info));
        return info;
    }
    void free_index() { check(nvsm_corpus_index_free(h_)); }
    struct Postings { std::vector<int64_t> doc_ids; std::vector<int32_t> tfs; };
    Postings postings(int64_t word_id) {      // one word's list, documents ascending
        Postings p;
        int64_t n = 0;
        const int st = nvsm_corpus_postings(h_, word_id, 0, nullptr, nullptr, &n);
        if (n == 0) { check(st); return p; }      // (an empty list is a success; a refusal leaves the count 0)
        p.doc_ids.resize(static_cast<size_t>(n)); p.tfs.resize(static_cast<size_t>(n));
        check(nvsm_corpus_postings(h_, word_id, n, p.doc_ids.data(), p.tfs.data(), &n));
        return p;
    }
    // the positional layer of the index (cunvsm_amd.h nvsm_corpus_index_positions): built once behind index_corpus(); with it the
    // SDM rankings may be served from the postings, the same bits
    nvsm_positions_info index_positions() {
        nvsm_positions_info info;
        check(nvsm_corpus_index_positions(h_, &info));
        return info;
    }
    void drop_positions() { check(nvsm_corpus_index_positions_free(h_)); }
    std::vector<int64_t> positions(int64_t word_id, int64_t doc_id) {      // the word's offsets inside the document, ascending
        std::vector<int64_t> p;
        int64_t n = 0;
        const int st = nvsm_corpus_positions(h_, word_id, doc_id, 0, nullptr, &n);
        if (n == 0) { check(st); return p; }      // (an empty run is a success; a refusal leaves the count 0)
        p.resize(static_cast<size_t>(n));
        check(nvsm_corpus_positions(h_, word_id, doc_id, n, p.data(), &n));
        return p;
    }
    // nvsm_rerank: rank() over the candidates the first stage retrieves at top_k = rr.depth, handed over on the device. judgments
    // null: no metrics (width 0).
    Evaluation rerank(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_rank_options& opt,
                      const nvsm_rerank_options& rr, const nvsm_judgments* judgments = nullptr, const std::vector<float>* word_weights = nullptr) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        Evaluation e;
        e.width = judgments ? NVSM_EVAL_FIXED + 3 * (judgments->num_cutoffs > 0 ? judgments->num_cutoffs : 0) : 0;
        e.ranking.top_k = opt.top_k;
        const size_t Q = static_cast<size_t>(q.num_queries);
        const size_t n = Q * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        e.metrics.resize(Q * static_cast<size_t>(e.width) + 1);
        e.ranking.doc_ids.resize(n ? n : 1); e.ranking.scores.resize(n ? n : 1); e.ranking.counts.resize(Q + 1);
        check(nvsm_rerank(h_, &q, &opt, &rr, judgments, judgments ? e.metrics.data() : nullptr, e.ranking.doc_ids.data(),
                          e.ranking.scores.data(), e.ranking.counts.data()));
        e.metrics.resize(Q * static_cast<size_t>(e.width));
        e.ranking.doc_ids.resize(n); e.ranking.scores.resize(n); e.ranking.counts.resize(Q);
        return e;
    }

    // nvsm_lexical_rank_weighted: lexical_rank with a float32 weight >= 0 per query word (one per word id; a weight 0 drops its term)
    Ranking lexical_rank_weighted(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const std::vector<float>& word_weights,
                                  const nvsm_lexical_options& lex) {
        static const float none = 0.f;      // (the ABI wants a pointer even where there is nothing to read)
        nvsm_queries q = queries_of(word_ids, offsets, &word_weights);
        if (!q.word_weights) q.word_weights = &none;
        Ranking r;
        r.top_k = lex.top_k;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(lex.top_k > 0 ? lex.top_k : 0);
        r.doc_ids.resize(n ? n : 1); r.scores.resize(n ? n : 1); r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_lexical_rank_weighted(h_, &q, &lex, r.doc_ids.data(), r.scores.data(), r.counts.data()));
        r.doc_ids.resize(n); r.scores.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    // nvsm_relevance_model: per query the fb.fb_terms most probable words under the relevance model of its fb.fb_docs best documents
    struct RelevanceModel { std::vector<int64_t> term_ids; std::vector<float> term_probs; std::vector<int64_t> counts; int32_t fb_terms; };
    RelevanceModel relevance_model(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_lexical_options& lex,
                                   const nvsm_feedback_options& fb) {
        const nvsm_queries q = queries_of(word_ids, offsets, nullptr);
        RelevanceModel r;
        r.fb_terms = fb.fb_terms;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(fb.fb_terms > 0 ? fb.fb_terms : 0);
        r.term_ids.resize(n ? n : 1); r.term_probs.resize(n ? n : 1); r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_relevance_model(h_, &q, &lex, &fb, r.term_ids.data(), r.term_probs.data(), r.counts.data()));
        r.term_ids.resize(n); r.term_probs.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    // nvsm_lexical_rank_prf: lexical_rank of the RM3 query (cunvsm_amd.h has the expansion)
    Ranking lexical_rank_prf(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_lexical_options& lex,
                             const nvsm_feedback_options& fb) {
        const nvsm_queries q = queries_of(word_ids, offsets, nullptr);
        Ranking r;
        r.top_k = lex.top_k;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(lex.top_k > 0 ? lex.top_k : 0);
        r.doc_ids.resize(n ? n : 1); r.scores.resize(n ? n : 1); r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_lexical_rank_prf(h_, &q, &lex, &fb, r.doc_ids.data(), r.scores.data(), r.counts.data()));
        r.doc_ids.resize(n); r.scores.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    // nvsm_rank_ensemble_prf: rank_ensemble with the lexical list taken from lexical_rank_prf
    Evaluation rank_ensemble_prf(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_rank_options& opt,
                                 const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, const nvsm_ensemble_options& ens,
                                 const nvsm_judgments* judgments = nullptr, const std::vector<float>* word_weights = nullptr) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        Evaluation e;
        e.width = judgments ? NVSM_EVAL_FIXED + 3 * (judgments->num_cutoffs > 0 ? judgments->num_cutoffs : 0) : 0;
        e.ranking.top_k = 2 * opt.top_k;
        const size_t Q = static_cast<size_t>(q.num_queries);
        const size_t n = Q * 2 * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        e.metrics.resize(Q * static_cast<size_t>(e.width) + 1);
        e.ranking.doc_ids.resize(n ? n : 1); e.ranking.scores.resize(n ? n : 1); e.ranking.counts.resize(Q + 1);
        check(nvsm_rank_ensemble_prf(h_, &q, &opt, &lex, &fb, &ens, judgments, judgments ? e.metrics.data() : nullptr, e.ranking.doc_ids.data(),
                                     e.ranking.scores.data(), e.ranking.counts.data()));
        e.metrics.resize(Q * static_cast<size_t>(e.width));
        e.ranking.doc_ids.resize(n); e.ranking.scores.resize(n); e.ranking.counts.resize(Q);
        return e;
    }

    // nvsm_sdm_rank: lexical_rank's retrieved set ranked by the sequential dependence model (cunvsm_amd.h has the formula)
    Ranking sdm_rank(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_lexical_options& lex,
                     const nvsm_sdm_options& sdm) {
        const nvsm_queries q = queries_of(word_ids, offsets, nullptr);
        Ranking r;
        r.top_k = lex.top_k;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(lex.top_k > 0 ? lex.top_k : 0);
        r.doc_ids.resize(n ? n : 1); r.scores.resize(n ? n : 1); r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_sdm_rank(h_, &q, &lex, &sdm, r.doc_ids.data(), r.scores.data(), r.counts.data()));
        r.doc_ids.resize(n); r.scores.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    // nvsm_sdm_pair_counts: the collection counts of every adjacent pair of every query, concatenated in query order
    struct PairCounts { std::vector<uint64_t> ordered, unordered; };
    PairCounts sdm_pair_counts(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_sdm_options& sdm) {
        const nvsm_queries q = queries_of(word_ids, offsets, nullptr);
        size_t n = 0;
        for (size_t i = 0; i + 1 < offsets.size(); ++i)
            if (offsets[i + 1] - offsets[i] > 1) n += static_cast<size_t>(offsets[i + 1] - offsets[i] - 1);
        PairCounts p;
        p.ordered.resize(n + 1); p.unordered.resize(n + 1);
        check(nvsm_sdm_pair_counts(h_, &q, &sdm, p.ordered.data(), p.unordered.data()));
        p.ordered.resize(n); p.unordered.resize(n);
        return p;
    }
    // nvsm_rank_ensemble_sdm: rank_ensemble with the lexical list taken from sdm_rank
    Evaluation rank_ensemble_sdm(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_rank_options& opt,
                                 const nvsm_lexical_options& lex, const nvsm_sdm_options& sdm, const nvsm_ensemble_options& ens,
                                 const nvsm_judgments* judgments = nullptr, const std::vector<float>* word_weights = nullptr) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        Evaluation e;
        e.width = judgments ? NVSM_EVAL_FIXED + 3 * (judgments->num_cutoffs > 0 ? judgments->num_cutoffs : 0) : 0;
        e.ranking.top_k = 2 * opt.top_k;
        const size_t Q = static_cast<size_t>(q.num_queries);
        const size_t n = Q * 2 * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        e.metrics.resize(Q * static_cast<size_t>(e.width) + 1);
        e.ranking.doc_ids.resize(n ? n : 1); e.ranking.scores.resize(n ? n : 1); e.ranking.counts.resize(Q + 1);
        check(nvsm_rank_ensemble_sdm(h_, &q, &opt, &lex, &sdm, &ens, judgments, judgments ? e.metrics.data() : nullptr, e.ranking.doc_ids.data(),
                                     e.ranking.scores.data(), e.ranking.counts.data()));
        e.metrics.resize(Q * static_cast<size_t>(e.width));
        e.ranking.doc_ids.resize(n); e.ranking.scores.resize(n); e.ranking.counts.resize(Q);
        return e;
    }

    // nvsm_ensemble_sweep: both rankings once, then the metric rows [alphas][num_queries][width] of their fusion at every alpha over
    // the first `depth` entries of the fused lists (0: all). fb null: the lexical list is lexical_rank's, else lexical_rank_prf's.
    struct Sweep { std::vector<double> metrics; int32_t width; int32_t num_alphas; };
    Sweep ensemble_sweep(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_rank_options& opt,
                         const nvsm_lexical_options& lex, const std::vector<float>& alphas, const nvsm_judgments& judgments,
                         int32_t normalizer = NVSM_NORM_STANDARDIZE, int32_t depth = 0, const nvsm_feedback_options* fb = nullptr,
                         const std::vector<float>* word_weights = nullptr) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        nvsm_sweep_options sw;
        nvsm_sweep_options_default(&sw);
        sw.alphas = alphas.data(); sw.num_alphas = static_cast<int32_t>(alphas.size()); sw.normalizer = normalizer; sw.depth = depth;
        Sweep s;
        s.width = NVSM_EVAL_FIXED + 3 * (judgments.num_cutoffs > 0 ? judgments.num_cutoffs : 0);
        s.num_alphas = sw.num_alphas;
        const size_t n = alphas.size() * static_cast<size_t>(q.num_queries) * static_cast<size_t>(s.width);
        s.metrics.resize(n + 1);
        check(nvsm_ensemble_sweep(h_, &q, &opt, &lex, fb, &sw, &judgments, s.metrics.data()));
        s.metrics.resize(n);
        return s;
    }
    // nvsm_rank_ensemble_cv: the sweep, per fold the alpha with the best training measure, and every query fused at its fold's alpha.
    // fold_of null: contiguous folds in query order. The evaluation holds the fused lists and their metric rows cut at `depth`.
    struct CrossValidation { std::vector<float> fold_alpha; std::vector<double> fold_train_measure; Evaluation evaluation; Sweep sweep; };
    CrossValidation rank_ensemble_cv(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const nvsm_rank_options& opt,
                                     const nvsm_lexical_options& lex, const std::vector<float>& alphas, const nvsm_judgments& judgments,
                                     int32_t num_folds = 20, int32_t measure = NVSM_EVAL_AP, int32_t normalizer = NVSM_NORM_STANDARDIZE,
                                     int32_t depth = 1000, const std::vector<int32_t>* fold_of = nullptr,
                                     const nvsm_feedback_options* fb = nullptr, const std::vector<float>* word_weights = nullptr) {
        const nvsm_queries q = queries_of(word_ids, offsets, word_weights);
        nvsm_sweep_options sw;
        nvsm_sweep_options_default(&sw);
        sw.alphas = alphas.data(); sw.num_alphas = static_cast<int32_t>(alphas.size()); sw.normalizer = normalizer; sw.depth = depth;
        nvsm_cv_options cv;
        nvsm_cv_options_default(&cv);
        cv.measure = measure; cv.num_folds = num_folds; cv.fold_of = fold_of ? fold_of->data() : nullptr;
        CrossValidation c;
        Evaluation& e = c.evaluation;
        e.width = c.sweep.width = NVSM_EVAL_FIXED + 3 * (judgments.num_cutoffs > 0 ? judgments.num_cutoffs : 0);
        c.sweep.num_alphas = sw.num_alphas;
        e.ranking.top_k = 2 * opt.top_k;
        const size_t Q = static_cast<size_t>(q.num_queries);
        const size_t n = Q * 2 * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        const size_t F = static_cast<size_t>(num_folds > 0 ? num_folds : 0);
        c.fold_alpha.resize(F + 1); c.fold_train_measure.resize(F + 1);
        e.metrics.resize(Q * static_cast<size_t>(e.width) + 1);
        c.sweep.metrics.resize(alphas.size() * Q * static_cast<size_t>(e.width) + 1);
        e.ranking.doc_ids.resize(n ? n : 1); e.ranking.scores.resize(n ? n : 1); e.ranking.counts.resize(Q + 1);
        check(nvsm_rank_ensemble_cv(h_, &q, &opt, &lex, fb, &sw, &cv, &judgments, c.fold_alpha.data(), c.fold_train_measure.data(),
                                    e.ranking.doc_ids.data(), e.ranking.scores.data(), e.ranking.counts.data(), e.metrics.data(),
                                    c.sweep.metrics.data()));
        c.fold_alpha.resize(F); c.fold_train_measure.resize(F);
        e.metrics.resize(Q * static_cast<size_t>(e.width));
        c.sweep.metrics.resize(alphas.size() * Q * static_cast<size_t>(e.width));
        e.ranking.doc_ids.resize(n); e.ranking.scores.resize(n); e.ranking.counts.resize(Q);
        return c;
    }

    // nearest neighbours among the word rows, the projected vocabulary or the document rows (py/nvsm/base.py:106-162, 325-353,
    // 362-430): queries are row ids of `source_space`, or vectors [n][dim] of the searched space (neighbors_of_vectors)
    struct Neighbors { std::vector<int64_t> ids; std::vector<float> scores; std::vector<int64_t> counts; int32_t top_k; };
    Neighbors neighbors(const std::vector<int64_t>& row_ids, int32_t source_space, const nvsm_neighbor_options& opt) {
        nvsm_neighbor_queries q;
        q.ids = row_ids.data(); q.vectors = nullptr; q.num_queries = static_cast<int64_t>(row_ids.size());
        q.source_space = source_space; q.dim = 0;
        return neighbors_of(q, opt);
    }
    Neighbors neighbors_of_vectors(const std::vector<float>& vectors, int32_t dim, const nvsm_neighbor_options& opt) {
        if (dim < 1 || vectors.size() % static_cast<size_t>(dim) != 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "vectors: a whole number of rows of dim floats");
        nvsm_neighbor_queries q;
        q.ids = nullptr; q.vectors = vectors.data(); q.num_queries = static_cast<int64_t>(vectors.size() / static_cast<size_t>(dim));
        q.source_space = opt.space; q.dim = dim;
        return neighbors_of(q, opt);
    }
    // NVSM.term_similarity (base.py:344-353) batched: the score of row a[i] against row b[i] of one space
    std::vector<float> similarity(int32_t space, const std::vector<int64_t>& a, const std::vector<int64_t>& b, int32_t sim = NVSM_SIM_COSINE) {
        if (a.size() != b.size()) throw Error(NVSM_ERR_INVALID_ARGUMENT, "similarity: a and b differ in length");
        std::vector<float> out(a.size() + 1);
        check(nvsm_similarity(h_, space, a.data(), b.data(), static_cast<int64_t>(a.size()), sim, out.data()));
        out.resize(a.size());
        return out;
    }

    // TermBruteforcer up to 2-grams (py/nvsm/base.py:106-162; nvsm_ngram_search): the phrases of opt.vocabulary (NULL: every word)
    // nearest to rows of `source_space` (entities or projected words), or to vectors [n][entity_repr_size] (ngram_search_of_vectors)
    struct Ngrams {
        std::vector<int64_t> phrase_rows, terms; std::vector<float> scores; std::vector<int64_t> counts;
        int32_t top_k, max_cardinality;      // terms [n][top_k][max_cardinality], -1 in unused slots
    };
    Ngrams ngram_search(const std::vector<int64_t>& row_ids, int32_t source_space, const nvsm_ngram_options& opt) {
        nvsm_neighbor_queries q;
        q.ids = row_ids.data(); q.vectors = nullptr; q.num_queries = static_cast<int64_t>(row_ids.size());
        q.source_space = source_space; q.dim = 0;
        return ngrams_of(q, opt);
    }
    Ngrams ngram_search_of_vectors(const std::vector<float>& vectors, const nvsm_ngram_options& opt) {
        const int32_t dim = cfg_.entity_repr_size;
        if (dim < 1 || vectors.size() % static_cast<size_t>(dim) != 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "vectors: a whole number of rows of entity_repr_size floats");
        nvsm_neighbor_queries q;
        q.ids = nullptr; q.vectors = vectors.data(); q.num_queries = static_cast<int64_t>(vectors.size() / static_cast<size_t>(dim));
        q.source_space = NVSM_SPACE_ENTITIES; q.dim = dim;
        return ngrams_of(q, opt);
    }

    // exact t-SNE of document or word rows (py/visualize.py; nvsm_tsne): opt.ids / opt.num_rows choose the rows (nvsm_tsne_options_default:
    // every document); embedding [rows][2], kl_divergence and n_iter as sklearn's kl_divergence_ and n_iter_
    struct Tsne { std::vector<float> embedding; double kl_divergence; int32_t n_iter; };
    Tsne tsne(const nvsm_tsne_options& opt) {
        int64_t n = opt.num_rows;
        if (!opt.ids && n == 0) n = opt.space == NVSM_SPACE_WORDS ? cfg_.num_words : cfg_.num_entities;
        Tsne r;
        r.embedding.resize(static_cast<size_t>(n > 0 ? 2 * n : 0) + 1);
        r.kl_divergence = 0.0; r.n_iter = 0;
        check(nvsm_tsne(h_, &opt, r.embedding.data(), &r.kl_divergence, &r.n_iter));
        r.embedding.resize(static_cast<size_t>(2 * n));
        return r;
    }
    Tsne tsne(const std::vector<int64_t>& row_ids, nvsm_tsne_options opt) {
        opt.ids = row_ids.data(); opt.num_rows = static_cast<int64_t>(row_ids.size());
        return tsne(opt);
    }
    // sparse-affinity t-SNE (nvsm_tsne_sparse: sklearn's barnes_hut at angle 0) for collections beyond NVSM_TSNE_MAX_ROWS; n_neighbors 0:
    // sklearn's min(n − 1, int(3·perplexity + 1))
    Tsne tsne_sparse(const nvsm_tsne_options& opt, int32_t n_neighbors = 0) {
        int64_t n = opt.num_rows;
        if (!opt.ids && n == 0) n = opt.space == NVSM_SPACE_WORDS ? cfg_.num_words : cfg_.num_entities;
        nvsm_tsne_sparse_options sp;
        nvsm_tsne_sparse_options_default(&sp);
        sp.n_neighbors = n_neighbors;
        Tsne r;
        r.embedding.resize(static_cast<size_t>(n > 0 ? 2 * n : 0) + 1);
        r.kl_divergence = 0.0; r.n_iter = 0;
        check(nvsm_tsne_sparse(h_, &opt, &sp, r.embedding.data(), &r.kl_divergence, &r.n_iter));
        r.embedding.resize(static_cast<size_t>(2 * n));
        return r;
    }
    Tsne tsne_sparse(const std::vector<int64_t>& row_ids, nvsm_tsne_options opt, int32_t n_neighbors = 0) {
        opt.ids = row_ids.data(); opt.num_rows = static_cast<int64_t>(row_ids.size());
        return tsne_sparse(opt, n_neighbors);
    }

    // Lloyd's k-means of document or word rows (nvsm_kmeans): opt.ids / opt.num_rows choose the rows (nvsm_kmeans_options_default: every
    // document), opt.num_clusters the centres; labels [rows], centers [k][dim], counts [k], distances [rows] (squared, to the own centre)
    struct Kmeans { std::vector<int32_t> labels; std::vector<float> centers; std::vector<int64_t> counts; std::vector<float> distances;
                    double inertia; int32_t n_iter; };
    Kmeans kmeans(const nvsm_kmeans_options& opt) {
        int64_t n = opt.num_rows;
        if (!opt.ids && n == 0) n = opt.space == NVSM_SPACE_WORDS ? cfg_.num_words : cfg_.num_entities;
        const int64_t dim = opt.space == NVSM_SPACE_WORDS ? cfg_.word_repr_size : cfg_.entity_repr_size;
        const size_t rows = static_cast<size_t>(n > 0 ? n : 0), k = static_cast<size_t>(opt.num_clusters > 0 ? opt.num_clusters : 0);
        Kmeans r;
        r.labels.resize(rows + 1); r.distances.resize(rows + 1);
        r.centers.resize(k * static_cast<size_t>(dim) + 1); r.counts.resize(k + 1);
        r.inertia = 0.0; r.n_iter = 0;
        check(nvsm_kmeans(h_, &opt, r.labels.data(), r.centers.data(), r.counts.data(), r.distances.data(), &r.inertia, &r.n_iter));
        r.labels.resize(rows); r.distances.resize(rows);
        r.centers.resize(k * static_cast<size_t>(dim)); r.counts.resize(k);
        return r;
    }
    Kmeans kmeans(const std::vector<int64_t>& row_ids, nvsm_kmeans_options opt) {
        opt.ids = row_ids.data(); opt.num_rows = static_cast<int64_t>(row_ids.size());
        return kmeans(opt);
    }

    void synchronize() { check(nvsm_synchronize(h_)); }
    void comm_init(const char id[128]) { check(nvsm_comm_init(h_, id)); }
    nvsm_model* handle() { return h_; }
    const nvsm_config& config() const { return cfg_; }

 private:
    Neighbors neighbors_of(const nvsm_neighbor_queries& q, const nvsm_neighbor_options& opt) {
        Neighbors r;
        r.top_k = opt.top_k;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        r.ids.resize(n ? n : 1); r.scores.resize(n ? n : 1); r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_neighbors(h_, &q, &opt, r.ids.data(), r.scores.data(), r.counts.data()));
        r.ids.resize(n); r.scores.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    Ngrams ngrams_of(const nvsm_neighbor_queries& q, const nvsm_ngram_options& opt) {
        Ngrams r;
        r.top_k = opt.top_k; r.max_cardinality = opt.max_cardinality;
        const size_t n = static_cast<size_t>(q.num_queries) * static_cast<size_t>(opt.top_k > 0 ? opt.top_k : 0);
        const size_t c = static_cast<size_t>(opt.max_cardinality > 0 ? opt.max_cardinality : 0);
        r.phrase_rows.resize(n ? n : 1); r.terms.resize(n * c + 1); r.scores.resize(n ? n : 1);
        r.counts.resize(static_cast<size_t>(q.num_queries) + 1);
        check(nvsm_ngram_search(h_, &q, &opt, r.phrase_rows.data(), r.terms.data(), r.scores.data(), r.counts.data()));
        r.phrase_rows.resize(n); r.terms.resize(n * c); r.scores.resize(n); r.counts.resize(static_cast<size_t>(q.num_queries));
        return r;
    }
    static nvsm_queries queries_of(const std::vector<int64_t>& word_ids, const std::vector<int64_t>& offsets, const std::vector<float>* word_weights) {
        if (offsets.empty() || offsets.back() != static_cast<int64_t>(word_ids.size()) || (word_weights && word_weights->size() != word_ids.size()))
            throw Error(NVSM_ERR_INVALID_ARGUMENT, "queries: offsets must end at word_ids.size(), weights must match word_ids");
        nvsm_queries q;
        q.word_ids = word_ids.data(); q.word_weights = word_weights ? word_weights->data() : nullptr;
        q.offsets = offsets.data(); q.num_queries = static_cast<int64_t>(offsets.size()) - 1;
        return q;
    }
    static uint64_t state_of(const std::minstd_rand0& rng) { std::stringstream ss; ss << rng; uint64_t s = 0; ss >> s; return s; }
    nvsm_config cfg_;
    nvsm_model* h_ = nullptr;
};

}  // namespace cunvsm_amd
