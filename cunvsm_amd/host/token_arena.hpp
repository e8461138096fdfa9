// The token arena of a collection: every chosen document's term list as MODEL term ids, documents back to back in ascending
// model document id, with the offset of every document's first token. One loop, two users: IndexSource (index_source.cpp) trains
// from it and hands it to nvsm_corpus_upload as its corpus_view(); cuNVSMQuery --qlm (query_main.cpp) builds it from a
// checkpoint's meta file and uploads it for nvsm_lexical_rank. The out-of-vocabulary rule is the reference's
// (cpp/data_indri.cpp:112-136): an index term the model does not hold becomes the OoV token 0 where the model has one, and is
// dropped otherwise.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "index.hpp"

namespace nvsm_host {

struct TokenArena {
    std::vector<int32_t> tokens;           // model term ids of all kept documents, back to back
    std::vector<uint64_t> first_token;     // [documents + 1] offsets into tokens; a document that is not named, or not kept, is empty
};

// index term id -> model term id as a table (-1: the model does not hold the term), from any map of (index term id, model term id)
template <typename TermMap>
std::vector<int32_t> model_term_table(const TermMap& model_term_of) {
    int64_t max_index_term = 0;
    for (const auto& m : model_term_of) max_index_term = std::max<int64_t>(max_index_term, static_cast<int64_t>(m.first));
    std::vector<int32_t> table(static_cast<size_t>(max_index_term) + 1, -1);
    for (const auto& m : model_term_of) table[static_cast<size_t>(m.first)] = static_cast<int32_t>(m.second);
    return table;
}

// documents: (model document id, index document id) pairs in ASCENDING model id, all below num_documents. keep(model document,
// index document, tokens appended) decides behind each document whether its tokens stay (false: the document is left empty).
template <typename Documents, typename Keep>
void build_token_arena(IndexInterface* index, const std::vector<int32_t>& model_term, bool oov_token, const Documents& documents,
                       size_t num_documents, Keep keep, TokenArena* out) {
    out->tokens.clear();
    out->first_token.assign(num_documents + 1, 0);
    size_t next_doc = 0;
    for (const auto& d : documents) {
        const size_t model_doc = static_cast<size_t>(d.first);
        for (; next_doc < model_doc; ++next_doc) out->first_token[next_doc + 1] = out->tokens.size();
        const size_t before = out->tokens.size();
        for (const TERMID_T t : index->termList(static_cast<DOCID_T>(d.second))) {
            const int32_t m = (t >= 0 && static_cast<size_t>(t) < model_term.size()) ? model_term[static_cast<size_t>(t)] : -1;
            if (m >= 0) out->tokens.push_back(m);
            else if (oov_token) out->tokens.push_back(0);
        }
        if (!keep(model_doc, static_cast<DOCID_T>(d.second), out->tokens.size() - before)) out->tokens.resize(before);
        out->first_token[model_doc + 1] = out->tokens.size();
        next_doc = model_doc + 1;
    }
    for (; next_doc < num_documents; ++next_doc) out->first_token[next_doc + 1] = out->tokens.size();
}

}  // namespace nvsm_host
