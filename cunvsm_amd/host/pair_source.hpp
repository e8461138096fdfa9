// The entity-entity similarity objective's data: RepresentationSimilarity::Batch / LoadSimilarities / DataSource
// (include/cuNVSM/data.h, cpp/data.cu:234-344) and the RepeatingSource(-1) the trainer wraps it in (cpp/main.cu:240-259,
// cpp/data_repeating.cpp). A similarity file holds lines of `docno docno weight`; a pair that names a document the model does not
// hold is skipped with the reference's warning. The source hands the pairs out in a shuffled order — shuffled with the caller's
// generator when it is constructed and at every reset(), by the one-draw-per-element shuffle libstdc++ shipped before GCC 7, the
// permutation index_source.cpp's windows get —, a pass ends with a short batch, and the repeating wrapper starts the next pass.
#pragma once

#include <deque>
#include <istream>
#include <map>
#include <memory>
#include <tuple>

#include "data.hpp"

namespace nvsm_host {

typedef std::tuple<ObjectIdxType, ObjectIdxType, WeightType> PairInstanceT;
typedef std::map<std::string, int64_t> IdentifiersMapT;

std::vector<PairInstanceT>* LoadSimilarities(std::istream& file, const IdentifiersMapT& identifiers_map);      // cpp/data.cu:234-276
std::vector<PairInstanceT>* LoadSimilarities(const std::string& path, const IdentifiersMapT& identifiers_map);  // :278-287

// RepresentationSimilarity::Batch: features [2 * batch_size] interleaved ids, weights [batch_size] — the two arrays of
// nvsm_pair_batch, from the installed batch allocator (page-locked in the trainer)
class PairBatch {
 public:
    explicit PairBatch(size_t batch_size);
    ~PairBatch();
    PairBatch(const PairBatch&) = delete;
    PairBatch& operator=(const PairBatch&) = delete;

    void clear() { num_instances_ = 0; }
    bool full() const { return num_instances_ == batch_size_; }
    bool empty() const { return num_instances_ == 0; }
    size_t num_instances() const { return num_instances_; }
    size_t maximum_size() const { return batch_size_; }
    const ObjectIdxType* features() const { return features_; }
    const WeightType* weights() const { return weights_; }

 private:
    friend class PairSource;
    const size_t batch_size_;
    ObjectIdxType* features_;
    WeightType* weights_;
    size_t num_instances_;
};

// RepresentationSimilarity::DataSource (cpp/data.cu:289-344). Takes ownership of `data`.
class PairSource {
 public:
    PairSource(const std::vector<PairInstanceT>* data, RNG* rng);
    PairSource(const std::string& path, const IdentifiersMapT& identifiers_map, RNG* rng);
    void reset();                              // :300-314: a fresh shuffled order of ALL pairs, drawn from the shared generator
    void next(PairBatch* batch);               // :316-334: until the batch is full or the pass is over
    bool has_next() const { return !instance_order_.empty(); }
    float progress() const;
    size_t size() const { return data_->size(); }
 private:
    std::unique_ptr<const std::vector<PairInstanceT>> data_;
    RNG* const rng_;
    std::deque<size_t> instance_order_;
};

// RepeatingSource<RepresentationSimilarity::Batch> (cpp/data_repeating.cpp): num_repeats size_t(-1) = for ever. Takes ownership.
class RepeatingPairSource {
 public:
    RepeatingPairSource(size_t num_repeats, PairSource* source) : num_repeats_(num_repeats), source_(source) {}
    void reset() { current_iteration_ = 0; source_->reset(); }
    void next(PairBatch* batch);
    bool has_next() const;
    bool next_reshuffles() const { return !source_->has_next(); }      // the next next() starts a pass: it draws from the generator
    size_t current_iteration() const { return current_iteration_; }
 private:
    const size_t num_repeats_;
    std::unique_ptr<PairSource> source_;
    size_t current_iteration_ = 0;
};

}  // namespace nvsm_host
