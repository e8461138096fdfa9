// CPU test of the second way to draw an epoch from IndexSource (cunvsm_amd/host/index_source.hpp): next_refs + corpus_view —
// what cuNVSMTrainModel --device_corpus hands to nvsm_corpus_upload / nvsm_step_windows_deferred — against next(Batch*).
// For each of the three orders (document order, all windows shuffled, sampled positions shuffled) x {uniform, self_information}
// feature weighting x {uniform, inv_doc_frequency} instance weighting at seed 1, two epochs drawn as window references and expanded
// here, on the CPU, by the definition in include/cunvsm_amd.h must be the same instances with the same weights in the same order as
// two epochs drawn as batches from a second source built the same way, and the shared generator must be in the same state after
// each epoch. On the Cranfield collection (argv[1]) and on the mock index of tests/cpp/host_tests.cpp.
// A stand-alone program: tests/test_corpus_host.py builds it next to host_tests (and once more with -fsanitize=address,undefined).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>

#include "../../cunvsm_amd/host/data.hpp"
#include "../../cunvsm_amd/host/index_source.hpp"
#include "../../cunvsm_amd/host/trectext_index.hpp"

using namespace nvsm_host;

static int g_failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("    EXPECT failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_failures; } } while (0)
#define EXPECT_EQ(a, b) do { if (!((a) == (b))) { std::ostringstream os_; os_ << (a) << " vs " << (b); \
    std::printf("    EXPECT_EQ failed %s:%d: %s == %s (%s)\n", __FILE__, __LINE__, #a, #b, os_.str().c_str()); ++g_failures; } } while (0)

// the MockDiskIndex of the reference's data tests as a plain IndexInterface (as in host_tests.cpp)
class FakeIndex : public IndexInterface {
 public:
    FakeIndex(bool add_oov, bool actual_tf) {
        const int tf[7] = {2, 3, 2, 1, 1, 1, 1};
        const TERMID_T ids[7] = {1, 2, 3, 4, 5, 10, 111};
        for (int i = 0; i < 7; ++i) { VocabularyEntry e; e.term_id = ids[i]; e.term = "test"; e.total_count = actual_tf ? tf[i] : 5; vocab_.push_back(e); }
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

struct Epoch {
    std::vector<WordIdxType> features;
    std::vector<WeightType> feature_weights, weights;
    std::vector<ObjectIdxType> labels;
    std::string rng_after;
    size_t calls = 0;
};

static std::string state(const RNG& rng) { std::ostringstream os; os << rng; return os.str(); }
static bool same_bits(const std::vector<WeightType>& a, const std::vector<WeightType>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(WeightType)) == 0);
}

static Epoch through_batches(IndexSource* source, RNG* rng, size_t batch_size) {
    Epoch e;
    Batch batch(batch_size, source->window_size());
    const size_t w = source->window_size();
    while (source->has_next()) {
        batch.clear();
        source->next(&batch);
        const size_t n = batch.num_instances();
        e.features.insert(e.features.end(), batch.features(), batch.features() + n * w);
        e.feature_weights.insert(e.feature_weights.end(), batch.feature_weights(), batch.feature_weights() + n * w);
        e.labels.insert(e.labels.end(), batch.labels(), batch.labels() + n);
        e.weights.insert(e.weights.end(), batch.weights(), batch.weights() + n);
        ++e.calls;
    }
    source->reset();
    e.rng_after = state(*rng);
    return e;
}

// the four lines of include/cunvsm_amd.h ("window i of the batch is the nvsm_batch instance ..."), with all-1 feature weights where
// the source has none, as the batches carry them and as the trainer uploads them
static Epoch through_refs(IndexSource* source, RNG* rng, size_t batch_size) {
    Epoch e;
    const size_t w = source->window_size();
    const IndexSource::CorpusView v = source->corpus_view();
    EXPECT_EQ(v.first_token[0], 0u);
    EXPECT_EQ(v.first_token[v.num_documents], v.num_tokens);
    EXPECT_EQ(v.num_documents, source->corpus_size());
    if (v.term_weight) EXPECT_EQ(v.num_term_weights, source->vocabulary_size());
    float last_progress = 0.f;
    while (source->has_next()) {
        const uint32_t* refs = nullptr;
        size_t n = 0;
        source->next_refs(batch_size, &refs, &n);
        EXPECT_TRUE(n > 0 && n <= batch_size);
        if (n == 0) break;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t doc = refs[2 * i], pos = refs[2 * i + 1];
            EXPECT_TRUE(doc < v.num_documents);
            if (doc >= v.num_documents) continue;
            EXPECT_TRUE(v.first_token[doc] + pos + w <= v.first_token[doc + 1]);
            for (size_t j = 0; j < w; ++j) {
                const int32_t t = v.tokens[v.first_token[doc] + pos + j];
                EXPECT_TRUE(t >= 0 && static_cast<size_t>(t) < source->vocabulary_size());
                e.features.push_back(static_cast<WordIdxType>(t));
                e.feature_weights.push_back(v.term_weight ? v.term_weight[t] : static_cast<WeightType>(1));
            }
            e.labels.push_back(static_cast<ObjectIdxType>(doc));
            e.weights.push_back(v.instance_weight[doc]);
        }
        EXPECT_TRUE(source->progress() >= last_progress);
        last_progress = source->progress();
        ++e.calls;
    }
    EXPECT_EQ(last_progress, 1.0f);
    source->reset();
    e.rng_after = state(*rng);
    return e;
}

static void plain_free(void* p) { std::free(p); }
static size_t g_held = 0;
static void* counting_alloc(size_t bytes) { ++g_held; return std::malloc(bytes); }

struct Setting { const char* name; bool shuffle; SamplingStrategy sampling; };
static const Setting kOrders[3] = {{"document order", false, NONE}, {"all windows shuffled", true, NONE}, {"sampled positions shuffled", true, NGRAM_FREQUENCY}};

template <typename MakeIndex>
static void compare(const char* collection, MakeIndex make_index, size_t window, size_t batch_size, size_t max_vocabulary, size_t min_df,
                    double max_df_ratio, size_t cutoff) {
    for (const Setting& order : kOrders)
        for (const TermWeightingStrategy tw : {UNIFORM_TERM_WEIGHTING, SELF_INFORMATION_TERM_WEIGHTING})
            for (const WeightingStrategy iw : {UNIFORM, INV_DOC_FREQUENCY}) {
                const int before = g_failures;
                RNG rng_a, rng_b;
                rng_a.seed(1); rng_b.seed(1);
                IndexInterface* ia = make_index();
                IndexInterface* ib = make_index();
                const uint64_t max_df = max_df_ratio > 0 ? static_cast<uint64_t>(std::ceil(ia->documentCount() * max_df_ratio)) : 0;
                IndexSource a(ia, window, &rng_a, max_vocabulary, min_df, max_df, cutoff, false, false, nullptr, nullptr, order.shuffle, order.sampling, iw, tw);
                IndexSource b(ib, window, &rng_b, max_vocabulary, min_df, max_df, cutoff, false, false, nullptr, nullptr, order.shuffle, order.sampling, iw, tw);
                EXPECT_EQ(state(rng_a), state(rng_b));
                g_held = 0;
                b.hold_plan_in(counting_alloc, plain_free);          // as the trainer does, with the page-locked allocator
                EXPECT_EQ(g_held, 1u);
                EXPECT_EQ(state(rng_a), state(rng_b));               // moving the plan draws nothing
                size_t instances = 0;
                for (int epoch = 0; epoch < 2; ++epoch) {
                    const Epoch ea = through_batches(&a, &rng_a, batch_size);
                    const Epoch eb = through_refs(&b, &rng_b, batch_size);
                    EXPECT_TRUE(!ea.labels.empty());
                    EXPECT_EQ(ea.labels.size(), eb.labels.size());
                    EXPECT_TRUE(ea.features == eb.features);
                    EXPECT_TRUE(ea.labels == eb.labels);
                    EXPECT_TRUE(same_bits(ea.feature_weights, eb.feature_weights));
                    EXPECT_TRUE(same_bits(ea.weights, eb.weights));
                    EXPECT_EQ(ea.calls, eb.calls);                   // the same batches, the last one short
                    EXPECT_EQ(ea.rng_after, eb.rng_after);
                    instances = ea.labels.size();
                }
                // ... and a source whose plan is held elsewhere still fills batches (one cursor, one plan)
                const Epoch ea = through_batches(&a, &rng_a, batch_size), eb = through_batches(&b, &rng_b, batch_size);
                EXPECT_TRUE(ea.features == eb.features && ea.labels == eb.labels && same_bits(ea.weights, eb.weights));
                EXPECT_EQ(ea.rng_after, eb.rng_after);
                std::printf("  [%s] %s: %s, feature weighting %s, weighting %s (%lu instances per epoch)\n", g_failures == before ? "ok" : "FAIL",
                            collection, order.name, tw == UNIFORM_TERM_WEIGHTING ? "uniform" : "self_information",
                            iw == UNIFORM ? "uniform" : "inv_doc_frequency", static_cast<unsigned long>(instances));
            }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: corpus_tests <cranfield.trectext>\n"); return 2; }
    verbosity() = 0;
    log_to_stderr() = false;
    const std::string cranfield = argv[1];
    try {
        compare("mock index", [] { return static_cast<IndexInterface*>(new FakeIndex(true, true)); }, 3, 4, 0, 0, 0.0, 0);
        compare("Cranfield", [&] { return static_cast<IndexInterface*>(TrectextIndex::from_file(cranfield)); }, 8, 1000, 60000, 2, 0.5, 300);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 1;
    }
    std::printf("%d failed\n", g_failures);
    return g_failures == 0 ? 0 : 1;
}
