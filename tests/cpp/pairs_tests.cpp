// CPU unit tests of the entity-entity pair source (cunvsm_amd/host/pair_source.hpp). The first two cases restate the reference's
// RepresentationSimilarityTest.LoadSimilarities and .DataSource (cpp/data_tests.cpp:687-746) with the same identifiers and pairs;
// the others add what the trainer leans on: the skip warning for unknown documents, repetition across passes with a short last
// batch, and the instance order for a pinned seed (recorded from a written-out minstd_rand0 and pre-GCC-7 shuffle; numbers only).
// Driven by tests/test_pairs_host.py.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iostream>
#include <set>
#include <sstream>

#include "../../cunvsm_amd/host/pair_source.hpp"

using namespace nvsm_host;

static int g_failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("    EXPECT failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_failures; } } while (0)
#define EXPECT_EQ(a, b) do { if (!((a) == (b))) { std::ostringstream os_; os_ << (a) << " vs " << (b); \
    std::printf("    EXPECT_EQ failed %s:%d: %s == %s (%s)\n", __FILE__, __LINE__, #a, #b, os_.str().c_str()); ++g_failures; } } while (0)

typedef std::pair<long, long> P;
static std::vector<P> pairs_of(const PairBatch& b) {
    std::vector<P> v;
    for (size_t i = 0; i < b.num_instances(); ++i) v.push_back(P(b.features()[2 * i], b.features()[2 * i + 1]));
    return v;
}
static std::multiset<P> as_set(const std::vector<P>& v) { return std::multiset<P>(v.begin(), v.end()); }

static const IdentifiersMapT kIdentifiers = {{"apple", 0}, {"pen", 1}, {"pineapple", 2}, {"apple-pen", 3}, {"pineapple-pen", 4},
                                             {"pen-pineapple-apple-pen", 5}};
static const char* kSimilarities =
    "pen apple 1.0\n"
    "pen apple-pen 1.0\n"
    "apple apple-pen 1.0\n"
    "pen pineapple-pen 1.0\n"
    "pineapple pineapple-pen 1.0\n"
    "apple-pen pen-pineapple-apple-pen 1.0\n"
    "pineapple-pen pen-pineapple-apple-pen 1.0\n";

// cpp/data_tests.cpp:687-719
static void test_LoadSimilarities() {
    std::istringstream stream{std::string(kSimilarities)};
    std::unique_ptr<std::vector<PairInstanceT>> data(LoadSimilarities(stream, kIdentifiers));
    std::multiset<std::tuple<long, long, float>> got, want = {std::make_tuple(1, 0, 1.0f), std::make_tuple(1, 3, 1.0f), std::make_tuple(0, 3, 1.0f),
                                                              std::make_tuple(1, 4, 1.0f), std::make_tuple(2, 4, 1.0f), std::make_tuple(3, 5, 1.0f),
                                                              std::make_tuple(4, 5, 1.0f)};
    for (const PairInstanceT& t : *data) got.insert(std::make_tuple(long(std::get<0>(t)), long(std::get<1>(t)), float(std::get<2>(t))));
    EXPECT_TRUE(got == want);
}

static std::vector<PairInstanceT>* reference_pairs() {      // cpp/data_tests.cpp:724-730
    return new std::vector<PairInstanceT>({std::make_tuple(0, 10, 1.0f), std::make_tuple(2, 1, 1.0f), std::make_tuple(5, 20, 1.0f),
                                           std::make_tuple(1, 6, 1.0f), std::make_tuple(12, 9, 1.0f)});
}

// cpp/data_tests.cpp:721-746
static void test_DataSource() {
    RNG rng;
    PairSource source(reference_pairs(), &rng);
    PairBatch batch(1024);
    source.next(&batch);
    EXPECT_EQ(batch.num_instances(), 5u);
    EXPECT_TRUE(as_set(pairs_of(batch)) == as_set({P(0, 10), P(2, 1), P(5, 20), P(1, 6), P(12, 9)}));
    EXPECT_TRUE(!source.has_next());
    for (size_t i = 0; i < 5; ++i) EXPECT_EQ(batch.weights()[i], 1.0f);
}

// cpp/data.cu:255-267: a pair naming an unknown document is skipped with a warning that names it (the first unknown of the line)
static void test_LoadSimilarities_skips_unknown_documents() {
    std::istringstream stream{std::string("pen apple 0.5\nbanana pen 1.0\npen cherry 2.0\ndurian elderberry 1.0\napple pineapple 0.25\n")};
    std::ostringstream captured;
    std::streambuf* old = std::cerr.rdbuf(captured.rdbuf());
    const bool logged = log_to_stderr();
    log_to_stderr() = true;
    std::unique_ptr<std::vector<PairInstanceT>> data(LoadSimilarities(stream, kIdentifiers));
    log_to_stderr() = logged;
    std::cerr.rdbuf(old);
    EXPECT_EQ(data->size(), 2u);
    if (data->size() == 2) {
        EXPECT_TRUE((*data)[0] == std::make_tuple(ObjectIdxType(1), ObjectIdxType(0), 0.5f));
        EXPECT_TRUE((*data)[1] == std::make_tuple(ObjectIdxType(0), ObjectIdxType(2), 0.25f));
    }
    const std::string log = captured.str();
    for (const char* name : {"banana", "cherry", "durian"})
        EXPECT_TRUE(log.find(std::string("Entity '") + name + "' not found; skipping pair.") != std::string::npos);
    EXPECT_TRUE(log.find("elderberry") == std::string::npos);
}

// RepeatingSource(-1) over the pair source (cpp/main.cu:256-258, cpp/data_repeating.cpp): passes follow each other for ever, the
// last batch of a pass is short, every pass hands out every pair once
static void test_repetition_with_a_short_last_batch() {
    RNG rng;
    RepeatingPairSource source(size_t(-1), new PairSource(reference_pairs(), &rng));
    PairBatch batch(2);
    std::vector<size_t> sizes;
    std::vector<P> pass;
    for (int b = 0; b < 9; ++b) {
        EXPECT_TRUE(source.has_next());
        EXPECT_EQ(source.next_reshuffles(), b > 0 && b % 3 == 0);
        batch.clear();
        source.next(&batch);
        sizes.push_back(batch.num_instances());
        for (const P& p : pairs_of(batch)) pass.push_back(p);
        if (b % 3 == 2) {
            EXPECT_TRUE(as_set(pass) == as_set({P(0, 10), P(2, 1), P(5, 20), P(1, 6), P(12, 9)}));
            pass.clear();
        }
    }
    EXPECT_TRUE(sizes == std::vector<size_t>({2, 2, 1, 2, 2, 1, 2, 2, 1}));
    EXPECT_EQ(source.current_iteration(), 2u);
}

// the order for the default seed (1): the one-draw-per-element shuffle of index_source.cpp on minstd_rand0, one shuffle at
// construction and one per reset, all from the ONE generator the caller shares with the model
static void test_seed_pinned_order() {
    RNG rng;
    PairSource source(reference_pairs(), &rng);
    PairBatch batch(1024);
    source.next(&batch);
    // order [2, 0, 4, 3, 1] of the five pairs
    EXPECT_TRUE(pairs_of(batch) == std::vector<P>({P(5, 20), P(0, 10), P(12, 9), P(1, 6), P(2, 1)}));
    std::stringstream ss; ss << rng;
    EXPECT_EQ(ss.str(), std::string("984943658"));          // four draws in
    source.reset();
    batch.clear();
    source.next(&batch);
    // order [3, 1, 0, 4, 2]
    EXPECT_TRUE(pairs_of(batch) == std::vector<P>({P(1, 6), P(2, 1), P(0, 10), P(12, 9), P(5, 20)}));
    std::stringstream ss2; ss2 << rng;
    EXPECT_EQ(ss2.str(), std::string("1457850878"));
    // resetting with instances left warns and starts over (cpp/data.cu:300-305)
    PairBatch small(2);
    source.reset();
    source.next(&small);
    EXPECT_TRUE(source.has_next());
    source.reset();
    EXPECT_EQ(source.progress(), 0.0f);
}

int main(int argc, char** argv) {
    log_to_stderr() = false;
    const std::vector<std::pair<const char*, std::function<void()>>> tests = {
        {"RepresentationSimilarityTest.LoadSimilarities", test_LoadSimilarities},
        {"RepresentationSimilarityTest.DataSource", test_DataSource},
        {"RepresentationSimilarityTest.LoadSimilarities_skips_unknown_documents", test_LoadSimilarities_skips_unknown_documents},
        {"RepresentationSimilarityTest.repetition_with_a_short_last_batch", test_repetition_with_a_short_last_batch},
        {"RepresentationSimilarityTest.seed_pinned_order", test_seed_pinned_order},
    };
    int failed_tests = 0;
    for (const auto& t : tests) {
        if (argc > 1 && std::string(argv[1]) != t.first) continue;
        const int before = g_failures;
        try { t.second(); }
        catch (const std::exception& e) { std::printf("    exception: %s\n", e.what()); ++g_failures; }
        const bool ok = g_failures == before;
        std::printf("[%s] %s\n", ok ? "PASS" : "FAIL", t.first);
        failed_tests += !ok;
    }
    std::printf("%d failed\n", failed_tests);
    return failed_tests ? 1 : 0;
}
