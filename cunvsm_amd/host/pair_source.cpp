#include "pair_source.hpp"

#include <fstream>
#include <numeric>
#include <sstream>

namespace nvsm_host {

std::vector<PairInstanceT>* LoadSimilarities(std::istream& file, const IdentifiersMapT& identifiers_map) {
    NVSM_CHECK(file.good());
    NVSM_CHECK(!identifiers_map.empty());
    std::vector<PairInstanceT>* const data = new std::vector<PairInstanceT>;
    std::string line;
    while (file.good() && std::getline(file, line)) {
        std::istringstream iss(line);
        std::string first_entity_id, second_entity_id;
        WeightType weight = 0;
        iss >> first_entity_id >> second_entity_id >> weight;
        // (the first unknown name is the one reported, as the reference's two tests in a row do)
        const auto first = identifiers_map.find(first_entity_id);
        if (first == identifiers_map.end()) {
            NVSM_LOG(WARNING) << "Entity '" << first_entity_id << "' not found; skipping pair.";
            continue;
        }
        const auto second = identifiers_map.find(second_entity_id);
        if (second == identifiers_map.end()) {
            NVSM_LOG(WARNING) << "Entity '" << second_entity_id << "' not found; skipping pair.";
            continue;
        }
        data->push_back(std::make_tuple(static_cast<ObjectIdxType>(first->second), static_cast<ObjectIdxType>(second->second), weight));
    }
    return data;
}

std::vector<PairInstanceT>* LoadSimilarities(const std::string& path, const IdentifiersMapT& identifiers_map) {
    NVSM_CHECK(!path.empty());
    std::ifstream file(path);
    NVSM_CHECK(file.good()) << "cannot read " << path;
    return LoadSimilarities(file, identifiers_map);
}

PairBatch::PairBatch(size_t batch_size) : batch_size_(batch_size), features_(nullptr), weights_(nullptr), num_instances_(0) {
    NVSM_CHECK(batch_size_ > 0);
    features_ = static_cast<ObjectIdxType*>(batch_alloc(2 * batch_size_ * sizeof(ObjectIdxType)));
    weights_ = static_cast<WeightType*>(batch_alloc(batch_size_ * sizeof(WeightType)));
}

PairBatch::~PairBatch() { batch_free(features_); batch_free(weights_); }

PairSource::PairSource(const std::vector<PairInstanceT>* data, RNG* rng) : data_(data), rng_(rng) { reset(); }

PairSource::PairSource(const std::string& path, const IdentifiersMapT& identifiers_map, RNG* rng)
    : PairSource(LoadSimilarities(path, identifiers_map), rng) {}

void PairSource::reset() {
    if (!instance_order_.empty()) {
        NVSM_LOG(WARNING) << "Resetting instance generator while there are still instances to consume.";
        instance_order_.clear();
    }
    std::vector<size_t> order(data_->size());
    std::iota(order.begin(), order.end(), size_t(0));
    NVSM_LOG(INFO) << "Shuffling " << order.size() << " instance pointers.";
    // std::shuffle as libstdc++ shipped it before GCC 7 (index_source.cpp shuffle_pre_gcc7): element i is swapped with the element
    // at a position drawn uniformly from [0, i], one generator-backed draw per element
    typedef std::uniform_int_distribution<uint64_t> Draw;
    Draw draw;
    for (size_t i = 1; i < order.size(); ++i) std::swap(order[i], order[draw(*rng_, Draw::param_type(0, i))]);
    instance_order_.assign(order.begin(), order.end());
}

void PairSource::next(PairBatch* batch) {
    NVSM_CHECK(batch->empty());
    while (!batch->full() && !instance_order_.empty()) {
        const PairInstanceT& instance = data_->at(instance_order_.front());
        const size_t offset = 2 * batch->num_instances_;
        batch->features_[offset] = std::get<0>(instance);
        batch->features_[offset + 1] = std::get<1>(instance);
        batch->weights_[batch->num_instances_] = std::get<2>(instance);
        instance_order_.pop_front();
        ++batch->num_instances_;
    }
}

float PairSource::progress() const {
    return 1.0f - static_cast<float>(instance_order_.size()) / static_cast<float>(data_->size());
}

void RepeatingPairSource::next(PairBatch* batch) {
    if (!source_->has_next()) {
        source_->reset();
        ++current_iteration_;
        NVSM_CHECK(current_iteration_ < num_repeats_);
    }
    source_->next(batch);
}

bool RepeatingPairSource::has_next() const {
    if (current_iteration_ + 1 < num_repeats_) return true;
    return source_->has_next();
}

}  // namespace nvsm_host
