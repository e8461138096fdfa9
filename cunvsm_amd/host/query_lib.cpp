#include "query_lib.hpp"

#include <sys/stat.h>

#include <cmath>
#include <cstdlib>
#include <random>
#include <sstream>

#include "base.hpp"
#include "trectext_index.hpp"

namespace nvsm_host {

namespace {
bool exists(const std::string& path) { struct stat st; return stat(path.c_str(), &st) == 0; }
}  // namespace

ModelPath split_model_path(const std::string& model_path) {
    ModelPath p;
    const size_t cut = model_path.rfind('_');                              // model.rsplit('_', 1)
    if (cut == std::string::npos) NVSM_LOG(FATAL) << model_path << " is not named <model>_<epoch>.hdf5";
    p.model_base = model_path.substr(0, cut);
    const std::string epoch_and_ext = model_path.substr(cut + 1);
    const std::string epoch = epoch_and_ext.substr(0, epoch_and_ext.find('.'));
    char* end = nullptr;
    p.epoch = std::strtol(epoch.c_str(), &end, 10);
    if (epoch.empty() || *end != '\0') NVSM_LOG(FATAL) << model_path << " is not named <model>_<epoch>.hdf5: '" << epoch << "' is no epoch number";
    p.meta_path = p.model_base + "_meta";
    if (!exists(p.meta_path)) {                                            // a dump of --dump_every: <model>_<epoch>_<batch>.hdf5
        const size_t cut2 = p.model_base.rfind('_');
        if (cut2 == std::string::npos || !exists(p.model_base.substr(0, cut2) + "_meta"))
            NVSM_LOG(FATAL) << "no meta file for " << model_path << ": " << p.meta_path << " does not exist";
        p.meta_path = p.model_base.substr(0, cut2) + "_meta";
    }
    return p;
}

ModelMappings build_mappings(const Metadata& meta, int64_t num_terms, int64_t num_objects) {
    ModelMappings m;
    m.total_terms = meta.total_terms;
    m.term_frequency.assign(static_cast<size_t>(num_terms), -1);
    m.index_object_of.assign(static_cast<size_t>(num_objects), -1);
    for (const Metadata::TermInfo& t : meta.term) {
        if (t.model_term_id < 0 || t.model_term_id >= num_terms)
            NVSM_LOG(FATAL) << "meta file: model term id " << t.model_term_id << " is outside the " << num_terms << " word representations";
        if (!m.model_term_of.emplace(t.index_term_id, t.model_term_id).second)
            NVSM_LOG(FATAL) << "meta file: index term id " << t.index_term_id << " is named twice";
        if (m.term_frequency[static_cast<size_t>(t.model_term_id)] != -1)
            NVSM_LOG(FATAL) << "meta file: model term id " << t.model_term_id << " is named twice";
        if (t.term_frequency < 0) NVSM_LOG(FATAL) << "meta file: model term id " << t.model_term_id << " has a negative term frequency";
        m.term_frequency[static_cast<size_t>(t.model_term_id)] = t.term_frequency;
    }
    for (const Metadata::ObjectInfo& o : meta.object) {
        if (o.model_object_id < 0 || o.model_object_id >= num_objects)
            NVSM_LOG(FATAL) << "meta file: model object id " << o.model_object_id << " is outside the " << num_objects << " entity representations";
        if (m.index_object_of[static_cast<size_t>(o.model_object_id)] != -1)
            NVSM_LOG(FATAL) << "meta file: model object id " << o.model_object_id << " is named twice";
        if (o.index_object_id < 0) NVSM_LOG(FATAL) << "meta file: model object id " << o.model_object_id << " has a negative index object id";
        if (!m.model_object_of.emplace(o.index_object_id, o.model_object_id).second)
            NVSM_LOG(FATAL) << "meta file: index object id " << o.index_object_id << " is named twice";
        m.index_object_of[static_cast<size_t>(o.model_object_id)] = o.index_object_id;
    }
    return m;
}

std::vector<Topic> parse_topics(std::istream& in, const std::string& origin) {
    std::vector<Topic> topics;
    std::string line;
    size_t number = 0;
    while (std::getline(in, line)) {
        ++number;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.find_first_not_of(" \t") == std::string::npos) continue;
        const size_t cut = line.find(';');
        if (cut == std::string::npos) NVSM_LOG(FATAL) << origin << ":" << number << ": no ';' between the topic id and its text";
        Topic t;
        t.id = line.substr(0, cut);
        t.text = line.substr(cut + 1);
        topics.push_back(t);
    }
    return topics;
}

void parse_qrels(std::istream& in, const std::string& origin, Qrels* qrels) {
    std::string line;
    size_t number = 0;
    while (std::getline(in, line)) {
        ++number;
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.find_first_not_of(" \t") == std::string::npos) continue;
        std::istringstream cols(line);
        std::string topic, iteration, docno, grade, more;
        cols >> topic >> iteration >> docno >> grade;
        char* end = nullptr;
        const long g = std::strtol(grade.c_str(), &end, 10);
        if (grade.empty() || *end != '\0' || (cols >> more))
            NVSM_LOG(FATAL) << origin << ":" << number << ": expected '<topic> <iteration> <docno> <grade>'";
        std::vector<std::pair<std::string, int>>& judged = (*qrels)[topic];
        bool known = false;
        for (std::pair<std::string, int>& j : judged)
            if (j.first == docno) { j.second = static_cast<int>(g); known = true; break; }
        if (!known) judged.emplace_back(docno, static_cast<int>(g));
    }
}

bool query_terms(IndexInterface* index, const ModelMappings& maps, const std::string& text, bool strict, std::vector<int64_t>* model_terms) {
    model_terms->clear();
    size_t tokens = 0;
    for (const std::string& token : TrectextIndex::tokenize(text)) {
        ++tokens;
        const TERMID_T index_term = index->term(token);
        const auto hit = index_term == 0 ? maps.model_term_of.end() : maps.model_term_of.find(index_term);
        if (hit == maps.model_term_of.end()) {
            NVSM_VLOG(1) << "Term " << token << " is out of vocabulary; skipping " << (strict ? "query." : "term.");
            continue;
        }
        model_terms->push_back(hit->second);
    }
    return !model_terms->empty() && !(strict && model_terms->size() < tokens);
}

std::vector<float> self_information(const ModelMappings& maps, const std::vector<int64_t>& model_terms) {
    std::vector<float> w;
    w.reserve(model_terms.size());
    for (const int64_t t : model_terms) {
        const int64_t tf = maps.term_frequency.at(static_cast<size_t>(t));
        w.push_back(static_cast<float>(-std::log(static_cast<double>(tf) / static_cast<double>(maps.total_terms))));
    }
    return w;
}

std::vector<int32_t> ensemble_folds(int64_t n, int64_t num_folds, uint64_t seed) {
    std::vector<int64_t> order(static_cast<size_t>(n > 0 ? n : 0));
    for (size_t i = 0; i < order.size(); ++i) order[i] = static_cast<int64_t>(i);
    if (seed > 0) {
        std::minstd_rand0 rng(static_cast<std::minstd_rand0::result_type>(seed));
        for (int64_t i = n - 1; i >= 1; --i) {
            const int64_t j = static_cast<int64_t>(rng() % static_cast<uint64_t>(i + 1));
            std::swap(order[static_cast<size_t>(i)], order[static_cast<size_t>(j)]);
        }
    }
    std::vector<int32_t> fold_of(order.size(), 0);
    if (num_folds < 1) return fold_of;
    int64_t at = 0;
    for (int64_t f = 0; f < num_folds; ++f)
        for (int64_t c = n / num_folds + (f < n % num_folds ? 1 : 0); c > 0 && at < n; --c) fold_of[static_cast<size_t>(order[static_cast<size_t>(at++)])] = static_cast<int32_t>(f);
    return fold_of;
}

bool ensemble_measure(const std::string& name, const std::vector<std::string>& names, int32_t* column, int32_t* depth) {
    *depth = 0;
    for (size_t i = 3; i < names.size(); ++i)
        if (names[i] == name) { *column = static_cast<int32_t>(i); return true; }
    static const std::string kCut = "map_cut_";
    if (name.compare(0, kCut.size(), kCut) != 0 || name.size() == kCut.size() || name.size() > kCut.size() + 9) return false;
    if (name.find_first_not_of("0123456789", kCut.size()) != std::string::npos) return false;
    const long d = std::strtol(name.c_str() + kCut.size(), nullptr, 10);
    if (d < 1) return false;
    for (size_t i = 3; i < names.size(); ++i)
        if (names[i] == "map") { *column = static_cast<int32_t>(i); *depth = static_cast<int32_t>(d); return true; }
    return false;
}

}  // namespace nvsm_host
