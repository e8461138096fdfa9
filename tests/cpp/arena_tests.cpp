// CPU test of the factored arena builder (cunvsm_amd/host/token_arena.hpp): built from what a checkpoint's meta file carries — the
// term and document id mappings of an IndexSource, as cuNVSMQuery --qlm reads them back — it must give the bytes of
// IndexSource::corpus_view(), the arena the trainer uploads: on the Cranfield collection (argv[1]) and on the mock index of
// tests/cpp/host_tests.cpp, with and without the out-of-vocabulary token, for the document order and for a shuffled order (which
// leaves documents shorter than a window empty: there the builder is told which documents the source kept).
// A stand-alone program: tests/test_arena_host.py builds it with the host sources (and once more with -fsanitize=address,undefined).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <unordered_map>

#include "../../cunvsm_amd/host/data.hpp"
#include "../../cunvsm_amd/host/index_source.hpp"
#include "../../cunvsm_amd/host/token_arena.hpp"
#include "../../cunvsm_amd/host/trectext_index.hpp"

using namespace nvsm_host;

static int g_failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("    EXPECT failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_failures; } } while (0)
#define EXPECT_EQ(a, b) do { if (!((a) == (b))) { std::ostringstream os_; os_ << (a) << " vs " << (b); \
    std::printf("    EXPECT_EQ failed %s:%d: %s == %s (%s)\n", __FILE__, __LINE__, #a, #b, os_.str().c_str()); ++g_failures; } } while (0)

// the MockDiskIndex of the reference's data tests as a plain IndexInterface (as in host_tests.cpp)
class FakeIndex : public IndexInterface {
 public:
    explicit FakeIndex(bool add_oov) {
        const int tf[7] = {2, 3, 2, 1, 1, 1, 1};
        const TERMID_T ids[7] = {1, 2, 3, 4, 5, 10, 111};
        for (int i = 0; i < 7; ++i) { VocabularyEntry e; e.term_id = ids[i]; e.term = "test"; e.total_count = tf[i]; vocab_.push_back(e); }
        d0_ = {1, 2, 3, 4};
        if (add_oov) d0_.insert(d0_.end(), {0, 0, 0});
        d0_.insert(d0_.end(), {3, 2, 1});
        d1_ = {10, 2};
        if (add_oov) d1_.insert(d1_.end(), {0, 0, 0, 0, 0});
        d1_.insert(d1_.end(), {111, 5});
        len0_ = 7 + (add_oov ? 3 : 0);
        len1_ = 4 + (add_oov ? 5 : 0);
    }
    DOCID_T documentBase() override { return 0; }
    DOCID_T documentMaximum() override { return 2; }
    uint64_t documentCount() override { return 2; }
    int64_t documentLength(DOCID_T d) override { return d == 0 ? len0_ : len1_; }
    uint64_t uniqueTermCount() override { return 7; }
    std::vector<VocabularyEntry> vocabulary() override { return vocab_; }
    std::vector<TERMID_T> termList(DOCID_T d) override { return d == 0 ? d0_ : d1_; }
    std::string term(TERMID_T) override { return "test"; }
    TERMID_T term(const std::string&) override { return 0; }
    std::vector<DOCID_T> documentIDsFromDocno(const std::vector<std::string>&) override { return {}; }
    std::string docno(DOCID_T d) override { return std::to_string(d); }
 private:
    std::vector<VocabularyEntry> vocab_;
    std::vector<TERMID_T> d0_, d1_;
    int64_t len0_, len1_;
};

template <typename MakeIndex>
static void compare(const char* collection, MakeIndex make_index, size_t window, size_t max_vocabulary, size_t min_df, double max_df_ratio,
                    size_t cutoff, bool include_oov, bool shuffle) {
    const int before = g_failures;
    RNG rng;
    rng.seed(1);
    IndexInterface* owned = make_index();
    const uint64_t max_df = max_df_ratio > 0 ? static_cast<uint64_t>(std::ceil(owned->documentCount() * max_df_ratio)) : 0;
    IndexSource source(owned, window, &rng, max_vocabulary, min_df, max_df, cutoff, include_oov, false, nullptr, nullptr, shuffle,
                       shuffle ? NONE : AUTOMATIC_SAMPLING);
    const IndexSource::CorpusView v = source.corpus_view();

    // what the meta file carries, in the container types cuNVSMQuery reads it into
    Metadata meta;
    source.extract_metadata(&meta);
    std::unordered_map<int64_t, int64_t> model_term_of;
    for (const auto& t : meta.term) model_term_of.emplace(t.index_term_id, t.model_term_id);
    std::vector<std::pair<size_t, DOCID_T>> documents;
    for (const auto& o : meta.object) documents.emplace_back(static_cast<size_t>(o.model_object_id), static_cast<DOCID_T>(o.index_object_id));
    std::sort(documents.begin(), documents.end());
    const bool oov_token = model_term_of.count(0) != 0;      // the model holds the OoV token exactly when index term 0 is mapped
    EXPECT_EQ(oov_token, include_oov);

    std::unique_ptr<IndexInterface> second(make_index());
    TokenArena arena;
    size_t kept = 0;
    build_token_arena(second.get(), model_term_table(model_term_of), oov_token, documents, source.corpus_size(),
                      [&](size_t model_doc, DOCID_T, size_t n) {      // the source's own rule: a shuffled order holds no document shorter than a window
                          const bool keep = !shuffle || n >= window;
                          EXPECT_EQ(keep, v.first_token[model_doc + 1] > v.first_token[model_doc] || n == 0);
                          kept += keep;
                          return keep;
                      },
                      &arena);
    EXPECT_EQ(arena.first_token.size(), v.num_documents + 1);
    EXPECT_EQ(arena.tokens.size(), v.num_tokens);
    if (arena.first_token.size() == v.num_documents + 1 && arena.tokens.size() == v.num_tokens) {
        EXPECT_TRUE(std::memcmp(arena.first_token.data(), v.first_token, (v.num_documents + 1) * sizeof(uint64_t)) == 0);
        EXPECT_TRUE(v.num_tokens == 0 || std::memcmp(arena.tokens.data(), v.tokens, v.num_tokens * sizeof(int32_t)) == 0);
    }
    EXPECT_TRUE(v.num_tokens > 0 && kept > 0);
    for (const int32_t t : arena.tokens) if (t < 0 || static_cast<size_t>(t) >= source.vocabulary_size()) { EXPECT_TRUE(false); break; }
    std::printf("  [%s] %s: %s, %s (%lu documents, %lu tokens)\n", g_failures == before ? "ok" : "FAIL", collection,
                include_oov ? "OoV token" : "OoV dropped", shuffle ? "shuffled" : "document order",
                static_cast<unsigned long>(v.num_documents), static_cast<unsigned long>(v.num_tokens));
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: arena_tests <cranfield.trectext>\n"); return 2; }
    verbosity() = 0;
    log_to_stderr() = false;
    const std::string cranfield = argv[1];
    try {
        for (const bool oov : {false, true})
            for (const bool shuffle : {false, true}) {
                compare("mock index", [&] { return static_cast<IndexInterface*>(new FakeIndex(oov)); }, 3, 0, 0, 0.0, 0, oov, shuffle);
                // (a vocabulary cap and a document-frequency band: many index terms are out of the model's vocabulary)
                compare("Cranfield", [&] { return static_cast<IndexInterface*>(TrectextIndex::from_file(cranfield)); }, 8, 2000, 2, 0.5, 300, oov, shuffle);
            }
        // an empty document list and a gap in the model ids: unnamed documents are empty, before, between and behind
        FakeIndex index(false);
        const std::vector<std::pair<size_t, DOCID_T>> some = {{1, 1}, {3, 0}};
        const std::unordered_map<int64_t, int64_t> terms = {{2, 0}, {111, 1}};
        TokenArena arena;
        build_token_arena(&index, model_term_table(terms), false, some, 5, [](size_t, DOCID_T, size_t) { return true; }, &arena);
        EXPECT_TRUE((arena.first_token == std::vector<uint64_t>{0, 0, 2, 2, 4, 4}));
        EXPECT_TRUE((arena.tokens == std::vector<int32_t>{0, 1, 0, 0}));
        build_token_arena(&index, model_term_table(terms), false, std::vector<std::pair<size_t, DOCID_T>>(), 2, [](size_t, DOCID_T, size_t) { return true; }, &arena);
        EXPECT_TRUE((arena.first_token == std::vector<uint64_t>{0, 0, 0}) && arena.tokens.empty());
        std::printf("  [%s] gaps and the empty list\n", g_failures == 0 ? "ok" : "FAIL");
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("%d failed\n", g_failures);
    return g_failures == 0 ? 0 : 1;
}
