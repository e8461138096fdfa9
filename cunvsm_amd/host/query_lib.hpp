// What cuNVSMQuery (query_main.cpp) does on the host around nvsm_evaluate — py/query.py and the loader of py/nvsm/base.py on top
// of the C ABI: where a checkpoint's meta file lies, the id mappings of the meta file, topic and qrel files, out-of-vocabulary
// handling and self-information weights. No device code; tests/cpp/query_tests.cpp drives every piece.
#pragma once

#include <cstdint>
#include <istream>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "index.hpp"
#include "metadata.hpp"

namespace nvsm_host {

// "<model_base>_<epoch>.hdf5" (py/query.py:145-151): the epoch is what follows the last '_' up to the first '.'; the meta file is
// "<model_base>_meta" and, where that does not exist, "<model_base minus one more _<batch> suffix>_meta" (the dumps of --dump_every).
struct ModelPath {
    std::string model_base, meta_path;
    long epoch = 0;
};
ModelPath split_model_path(const std::string& model_path);      // FatalError: no '_', no epoch number, no meta file

// The mappings of py/nvsm/base.py:188-222 with its asserts as FatalErrors: index term id -> model term id -> term frequency,
// model object id -> index object id (and back). Ids must be unique on both sides and model ids inside the tables.
struct ModelMappings {
    std::unordered_map<int64_t, int64_t> model_term_of;           // index term id -> model term id
    std::vector<int64_t> term_frequency;                          // by model term id (-1: the meta file names no such term)
    std::vector<int64_t> index_object_of;                         // by model object id (-1: not named)
    std::unordered_map<int64_t, int64_t> model_object_of;         // index object id -> model object id
    int64_t total_terms = 0;
};
ModelMappings build_mappings(const Metadata& meta, int64_t num_terms, int64_t num_objects);

// One query per line, "<topic id>;<text>" (resources/product-substitutability/*/topics); the text is everything behind the FIRST
// ';'. Empty lines are skipped, a trailing '\r' is dropped, a line without ';' is a FatalError. File order is kept.
struct Topic {
    std::string id, text;
};
std::vector<Topic> parse_topics(std::istream& in, const std::string& origin);

// "<topic> <iteration> <docno> <grade>" per line, any blanks between the columns; empty lines are skipped, anything else that
// does not have four columns with an integer grade is a FatalError. Per topic the judgments in file order; a docno judged twice
// for a topic keeps its LAST grade (one entry).
typedef std::map<std::string, std::vector<std::pair<std::string, int>>> Qrels;
void parse_qrels(std::istream& in, const std::string& origin, Qrels* qrels);

// A topic's text as model term ids (py/nvsm/base.py:274-295 behind pyndri's tokenisation): a token the index does not know or has
// stopped (id 0), or one that is not in the model, is out of vocabulary and skipped; with `strict` the whole query is. False: the
// query is to be skipped (no term left, or strict and a term missing).
bool query_terms(IndexInterface* index, const ModelMappings& maps, const std::string& text, bool strict, std::vector<int64_t>* model_terms);

// -log(tf / total_terms) in double, then float (py/nvsm/base.py:297-301)
std::vector<float> self_information(const ModelMappings& maps, const std::vector<int64_t>& model_terms);

// The folds of --ensemble_qrel: fold_of[i] of the i-th kept topic. The topics are permuted — seed > 0: a Fisher-Yates pass driven by
// std::minstd_rand0(seed), for i = n - 1 down to 1: j = rng() % (i + 1), swap positions i and j; seed 0: topic-file order — and
// the permuted sequence is cut into num_folds contiguous folds, the first n % num_folds of them one topic longer.
std::vector<int32_t> ensemble_folds(int64_t n, int64_t num_folds, uint64_t seed);

// --ensemble_measure: a name of `names` (the printed metrics; not num_ret, num_rel, num_rel_ret) -> its column, depth 0; or
// map_cut_<d> -> the column of map, depth d. false: neither.
bool ensemble_measure(const std::string& name, const std::vector<std::string>& names, int32_t* column, int32_t* depth);

}  // namespace nvsm_host
