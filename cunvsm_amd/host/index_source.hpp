// IndexSource — the data source of cuNVSMTrainModel: n-gram windows of the documents of an index, as
// TextEntity::Batch rows. Same constructor arguments, vocabulary / document selection and — given the same seed — the
// same instances in the same order as the reference's TextEntity::IndriSource (include/cuNVSM/data.h:383-529,
// cpp/data_indri.cpp:412-915), which its own tests pin (cpp/data_tests.cpp:365-683, restated in
// tests/cpp/host_tests.cpp). Built differently:
//   * the collection is mapped to model term ids ONCE into a flat token arena (32-bit ids + one offset per document)
//     through a dense index-term → model-term table;
//   * an epoch is a flat array of (document, position) references — all windows in document order, all windows
//     shuffled, or `samples per document` sampled positions shuffled — consumed by a cursor;
//   * next() copies windows from the arena straight into the batch's rows. There is no per-instance object, no
//     intermediate queue and no generator class hierarchy.
// What has to be the reference's is the random stream: one uniform_int_distribution<int> draw per sampled position, in
// document order, then the one-draw-per-element shuffle libstdc++ shipped before GCC 7 (the permutation the reference's
// seed-pinned test expects), all on the caller's minstd_rand0.
#pragma once

#include <map>
#include <memory>
#include <set>

#include "data.hpp"
#include "index.hpp"
#include "metadata.hpp"

namespace nvsm_host {

enum SamplingStrategy { AUTOMATIC_SAMPLING, NONE, NGRAM_FREQUENCY };                 // data.h:371-373
enum WeightingStrategy { AUTOMATIC_WEIGHTING, UNIFORM, INV_DOC_FREQUENCY };          // :375-377
enum TermWeightingStrategy { UNIFORM_TERM_WEIGHTING, SELF_INFORMATION_TERM_WEIGHTING };  // :379-381

class IndexSource : public DataSource {
 public:
    typedef std::map<TERMID_T, size_t> TermIdMapping;
    typedef std::map<size_t, DOCID_T> DocumentIdMapping;
    typedef std::set<std::string> TermBlacklist;

    // Takes ownership of `index` (as IndriSource(DiskIndex*, ...) does, data.h:405-418).
    IndexSource(IndexInterface* index, size_t window_size, RNG* rng, size_t max_vocabulary_size = 0,
                size_t min_document_frequency = 0, size_t max_document_frequency = 0, size_t documents_cutoff = 0,
                bool include_oov = false, bool include_digits = false,
                const std::vector<std::string>* document_list = nullptr, const TermBlacklist* term_blacklist = nullptr,
                bool shuffle = false, SamplingStrategy sampling_strategy = AUTOMATIC_SAMPLING,
                WeightingStrategy weighting_strategy = AUTOMATIC_WEIGHTING,
                TermWeightingStrategy term_weighting_strategy = UNIFORM_TERM_WEIGHTING);
    // Fold-in (cuNVSMTrainModel --fold_in): windows of a CHOSEN set of documents under a FIXED term mapping. Nothing is selected: the
    // vocabulary is `terms` (a checkpoint's meta file: the same model term ids, its term frequencies and total_terms for the
    // self-information weights; the out-of-vocabulary token exists exactly when index term 0 is mapped), the documents are
    // `documents` (index ids, each at least a window long), and document i carries the label label_offset + i. Weighting, sampling
    // and shuffling are what the constructor above does for a collection that consists of these documents. Takes ownership of `index`.
    struct FoldIn {
        std::vector<Metadata::TermInfo> terms;
        int64_t total_terms = 0;
        std::vector<DOCID_T> documents;
        size_t label_offset = 0;
    };
    IndexSource(IndexInterface* index, size_t window_size, RNG* rng, const FoldIn& fold, bool shuffle = false,
                SamplingStrategy sampling_strategy = AUTOMATIC_SAMPLING, WeightingStrategy weighting_strategy = AUTOMATIC_WEIGHTING,
                TermWeightingStrategy term_weighting_strategy = UNIFORM_TERM_WEIGHTING);
    ~IndexSource() override;

    void reset() override;                 // next epoch: re-draws / re-shuffles with the shared generator
    void next(Batch* batch) override;
    bool has_next() const override;
    float progress() const override;       // windows handed out / windows of this epoch
    void extract_metadata(Metadata* metadata) const override;

    int64_t term_id(const std::string& term) const;            // model term id or -1
    std::string term(int64_t model_term_id) const;
    const TermIdMapping& term_id_mapping() const { return model_term_of_; }
    const DocumentIdMapping& document_id_mapping() const { return index_doc_of_; }      // keyed without the fold-in's label offset
    size_t label_offset() const { return label_offset_; }
    const std::map<size_t, int64_t>& term_frequencies() const { return frequency_of_model_term_; }
    size_t window_size() const { return window_; }
    size_t total_num_terms() const { return corpus_term_occurrences_; }
    std::map<std::string, int64_t> build_term_identifiers_map() const;
    std::map<std::string, int64_t> build_document_identifiers_map() const;

    // ---- the collection as the GPU can train from it (nvsm_corpus_upload / nvsm_step_windows, include/cunvsm_amd.h) ----
    // What next(Batch*) copies windows out of, read-only and valid as long as the source lives: the flat arena of model term
    // ids, one offset per model document (+ 1), the instance weight of every window of a document, and the feature weight of
    // every occurrence of a term (null under uniform term weighting: every weight is 1).
    struct CorpusView {
        const int32_t* tokens; size_t num_tokens;
        const uint64_t* first_token; size_t num_documents;      // first_token[num_documents] == num_tokens
        const WeightType* instance_weight;                      // [num_documents]
        const WeightType* term_weight; size_t num_term_weights; // [num_term_weights] or null
    };
    CorpusView corpus_view() const;
    // A second way to draw an epoch: the next at most `max` entries of the epoch plan as they lie in memory — (model document,
    // first token inside the document) as interleaved uint32, *count of them at *refs, valid until the next reset(). The plan,
    // the cursor and the shared generator are the ones next(Batch*) uses: has_next(), progress() and reset() behave the same,
    // and an epoch drawn this way consumes the random stream exactly as one drawn through batches. hold_plan_in(alloc, free)
    // moves the plan (this epoch's and every later one's) into memory from `alloc` — the trainer passes the page-locked
    // allocator, so that slices of the plan are read by the GPU where they lie.
    void next_refs(size_t max, const uint32_t** refs, size_t* count);
    void hold_plan_in(BatchAllocFn alloc, BatchFreeFn free_fn);

    // −log(term frequency / total term occurrences) per term; empty under uniform term weighting (data.h:465-490)
    std::vector<WeightType> compute_term_weights(const std::vector<WordIdxType>& terms) const;

 private:
    class WindowFeeder;                    // index_source.cpp
    void choose_documents(size_t documents_cutoff, const std::vector<std::string>* document_list);
    void choose_vocabulary(size_t max_vocabulary_size, size_t min_document_frequency, size_t max_document_frequency,
                           bool include_digits, const TermBlacklist* term_blacklist);
    size_t occurrences_in_chosen_documents(TERMID_T term_id);

    std::unique_ptr<IndexInterface> index_;
    const size_t window_;
    const bool oov_token_;                 // out-of-vocabulary positions become model term 0 instead of being dropped
    const TermWeightingStrategy term_weighting_;
    size_t corpus_term_occurrences_ = 0;
    WeightType mean_index_document_length_ = 0;
    TermIdMapping model_term_of_;                          // index term id → model term id
    std::map<size_t, TERMID_T> index_term_of_;             // model term id → index term id
    std::map<size_t, int64_t> frequency_of_model_term_;
    DocumentIdMapping index_doc_of_;                       // model document id → index document id
    std::vector<int64_t> index_document_length_;           // by model document id
    std::map<TERMID_T, size_t> occurrences_;               // term occurrences inside the chosen documents (built on demand)
    bool occurrences_counted_ = false;
    size_t label_offset_ = 0;              // fold-in: added to every label (and to the model ids of extract_metadata and the docno map)
    void start_feeder(bool shuffle, SamplingStrategy sampling_strategy, WeightingStrategy weighting_strategy, RNG* rng);
    std::unique_ptr<WindowFeeder> feeder_;
};

// --fold_in: the documents a model is grown by — of `document_list` (docnos; null: every document of the index) those the meta file
// does not name and that are at least a window long, in INDEX order whatever the list's. A docno the index does not know is fatal, and so is a result without documents.
std::vector<DOCID_T> fold_in_new_documents(IndexInterface* index, const Metadata& meta, const std::vector<std::string>* document_list,
                                           size_t window_size);

}  // namespace nvsm_host
