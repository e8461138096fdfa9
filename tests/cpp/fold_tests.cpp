// CPU unit tests of what cuNVSMTrainModel --fold_in does on the host (cunvsm_amd/host/index_source.hpp: fold_in_new_documents and
// the IndexSource constructor that takes a fixed term mapping, a chosen document set and a label offset), on the Cranfield
// collection given as argv[1]. Driven by tests/test_fold_host.py: `fold_tests <collection> [<case>]`.
// `fold_tests --dump-hdf5 <checkpoint> <outbase>` writes the four datasets of a checkpoint as raw float32 files <outbase>.{W,E,T,b}.f32
// and prints their shapes (read_hdf5 of hdf5_writer.hpp): how tests/test_trainer_fold_gpu.py compares checkpoints byte for byte.
#include <cmath>
#include <cstdio>
#include <fstream>
#include <functional>
#include <iostream>
#include <map>
#include <memory>
#include <set>
#include <sstream>

#include "../../cunvsm_amd/host/base.hpp"
#include "../../cunvsm_amd/host/hdf5_writer.hpp"
#include "../../cunvsm_amd/host/index_source.hpp"
#include "../../cunvsm_amd/host/trectext_index.hpp"

using namespace nvsm_host;

static int g_failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("    EXPECT failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_failures; } } while (0)
#define EXPECT_EQ(a, b) do { if (!((a) == (b))) { std::ostringstream os_; os_ << (a) << " vs " << (b); \
    std::printf("    EXPECT_EQ failed %s:%d: %s == %s (%s)\n", __FILE__, __LINE__, #a, #b, os_.str().c_str()); ++g_failures; } } while (0)

static void expect_fatal(const std::function<void()>& call, const char* word, int line) {
    try {
        call();
    } catch (const FatalError& e) {
        if (std::string(e.what()).find(word) == std::string::npos) { std::printf("    line %d: FatalError without '%s': %s\n", line, word, e.what()); ++g_failures; }
        return;
    }
    std::printf("    line %d: no FatalError (expected one about '%s')\n", line, word);
    ++g_failures;
}
#define EXPECT_FATAL(word, ...) expect_fatal([&] { __VA_ARGS__; }, word, __LINE__)

static std::string g_collection;
static const size_t kWindow = 10, kOld = 1300;

static IndexInterface* open_index() { return TrectextIndex::from_file(g_collection, ""); }

// the meta file of a model trained on the first kOld documents of the collection (what the trainer writes for --document_list)
static Metadata old_model_meta(std::vector<std::string>* old_docnos = nullptr) {
    std::unique_ptr<IndexInterface> probe(open_index());
    std::vector<std::string> docnos;
    for (DOCID_T d = probe->documentBase(); docnos.size() < kOld; ++d) docnos.push_back(probe->docno(d));
    RNG rng(1);
    IndexSource source(open_index(), kWindow, &rng, 65536, 2, 700, 0, false, false, &docnos, nullptr, false);
    Metadata meta;
    source.extract_metadata(&meta);
    if (old_docnos) *old_docnos = docnos;
    return meta;
}

static void test_new_documents() {
    std::vector<std::string> old_docnos;
    const Metadata meta = old_model_meta(&old_docnos);
    EXPECT_TRUE(meta.object_size() > 1200 && meta.object_size() <= kOld);
    for (size_t i = 0; i < meta.object.size(); ++i) EXPECT_EQ(meta.object[i].model_object_id, static_cast<int32_t>(i));      // old ids keep their order
    std::unique_ptr<IndexInterface> index(open_index());
    std::set<DOCID_T> known;
    for (const auto& o : meta.object) known.insert(o.index_object_id);
    // every document of the index: the ones the meta file does not name, ascending, none shorter than a window
    const std::vector<DOCID_T> fresh = fold_in_new_documents(index.get(), meta, nullptr, kWindow);
    EXPECT_TRUE(fresh.size() >= 90 && fresh.size() <= 100 + (kOld - meta.object_size()));
    for (size_t i = 0; i < fresh.size(); ++i) {
        EXPECT_TRUE(known.count(fresh[i]) == 0);
        EXPECT_TRUE(index->documentLength(fresh[i]) >= static_cast<int64_t>(kWindow));
        if (i) EXPECT_TRUE(fresh[i - 1] < fresh[i]);
    }
    size_t expected = 0;
    for (DOCID_T d = index->documentBase(); d < index->documentMaximum(); ++d)
        expected += known.count(d) == 0 && index->documentLength(d) >= static_cast<int64_t>(kWindow);
    EXPECT_EQ(fresh.size(), expected);
    // a document list: new and old documents mixed, the new ones in reverse and one of them twice -> index order, once each
    std::vector<std::string> list = {index->docno(fresh[5]), old_docnos[3], index->docno(fresh[2]), index->docno(fresh[5]), old_docnos[0], index->docno(fresh[0])};
    const std::vector<DOCID_T> some = fold_in_new_documents(index.get(), meta, &list, kWindow);
    EXPECT_EQ(some.size(), 3u);
    if (some.size() == 3) { EXPECT_EQ(some[0], fresh[0]); EXPECT_EQ(some[1], fresh[2]); EXPECT_EQ(some[2], fresh[5]); }
    // only old documents: fatal; a docno the index does not know: fatal
    std::vector<std::string> only_old = {old_docnos[1], old_docnos[2]};
    EXPECT_FATAL("no new documents", fold_in_new_documents(index.get(), meta, &only_old, kWindow));
    std::vector<std::string> unknown = {"no-such-docno"};
    EXPECT_FATAL("Check failed", fold_in_new_documents(index.get(), meta, &unknown, kWindow));
}

static void test_source() {
    Metadata meta = old_model_meta();
    const size_t n_old = meta.object_size();
    std::unique_ptr<IndexInterface> index(open_index());
    IndexSource::FoldIn fold;
    fold.terms = meta.term; fold.total_terms = meta.total_terms;
    fold.documents = fold_in_new_documents(index.get(), meta, nullptr, kWindow);
    fold.label_offset = n_old;
    // a frequency only the meta file can have given: the weight of that term must follow it
    const int32_t marked_model_term = fold.terms[fold.terms.size() / 2].model_term_id;
    fold.terms[fold.terms.size() / 2].term_frequency = 7777;
    const std::vector<DOCID_T> documents = fold.documents;
    RNG rng(1);
    IndexSource source(index.release(), kWindow, &rng, fold, false, AUTOMATIC_SAMPLING, AUTOMATIC_WEIGHTING, SELF_INFORMATION_TERM_WEIGHTING);
    EXPECT_EQ(source.vocabulary_size(), meta.term_size());
    EXPECT_EQ(source.corpus_size(), documents.size());
    EXPECT_EQ(source.label_offset(), n_old);
    EXPECT_EQ(source.total_num_terms(), static_cast<size_t>(meta.total_terms));
    // the vocabulary is exactly the meta file's: same index term -> model term pairs
    for (const auto& t : meta.term) {
        const auto hit = source.term_id_mapping().find(t.index_term_id);
        EXPECT_TRUE(hit != source.term_id_mapping().end() && hit->second == static_cast<size_t>(t.model_term_id));
    }
    EXPECT_EQ(source.term_id_mapping().size(), meta.term_size());
    // metadata: the terms as given, the objects numbered from n_old on in the given (index) order
    Metadata got;
    source.extract_metadata(&got);
    EXPECT_EQ(got.term_size(), meta.term_size());
    EXPECT_EQ(got.total_terms, meta.total_terms);
    EXPECT_EQ(got.object_size(), documents.size());
    for (size_t i = 0; i < got.object.size(); ++i) {
        EXPECT_EQ(got.object[i].model_object_id, static_cast<int32_t>(n_old + i));
        EXPECT_EQ(got.object[i].index_object_id, static_cast<int32_t>(documents[i]));
    }
    // windows in document order: labels carry the offset and never name an old document; features are model term ids of the meta
    // file; feature weights are -log(tf / total_terms) of the META file's frequencies
    std::map<int64_t, int64_t> tf_of;      // straight from the (marked) meta data, not from the source under test
    for (const auto& t : fold.terms) tf_of[t.model_term_id] = t.term_frequency;
    Batch batch(4096, kWindow);
    size_t windows = 0, marked_seen = 0;
    int64_t last_label = -1;
    std::set<int64_t> labels;
    while (source.has_next()) {
        batch.clear();
        source.next(&batch);
        for (size_t i = 0; i < batch.num_instances(); ++i, ++windows) {
            const int64_t label = static_cast<int64_t>(batch.labels()[i]);
            EXPECT_TRUE(label >= static_cast<int64_t>(n_old) && label < static_cast<int64_t>(n_old + documents.size()));
            EXPECT_TRUE(label >= last_label);
            last_label = label;
            labels.insert(label);
            for (size_t j = 0; j < kWindow; ++j) {
                const int64_t term = static_cast<int64_t>(batch.features()[i * kWindow + j]);
                EXPECT_TRUE(term >= 0 && term < static_cast<int64_t>(meta.term_size()));
                const int64_t tf = tf_of.count(term) ? tf_of[term] : -1;
                const float want = -std::log(static_cast<WeightType>(tf) / static_cast<size_t>(meta.total_terms));
                EXPECT_TRUE(batch.feature_weights()[i * kWindow + j] == want);
                if (term == marked_model_term) { ++marked_seen; EXPECT_EQ(tf, 7777); }
            }
        }
        if (g_failures > 20) return;
    }
    EXPECT_TRUE(windows > 1000);
    EXPECT_TRUE(labels.size() > documents.size() * 9 / 10);      // (a document may hold fewer than a window of in-vocabulary tokens)
    std::printf("    %zu windows of %zu documents, the marked term %zu times\n", windows, labels.size(), marked_seen);
}

static void test_existing_constructor_is_unchanged() {
    // label offset 0 and the model ids of the meta data as before
    RNG rng(1);
    IndexSource source(open_index(), kWindow, &rng, 65536, 2, 700, 50, false, false, nullptr, nullptr, false);
    EXPECT_EQ(source.label_offset(), 0u);
    Metadata meta;
    source.extract_metadata(&meta);
    EXPECT_EQ(meta.object_size(), 50u);
    for (size_t i = 0; i < meta.object.size(); ++i) EXPECT_EQ(meta.object[i].model_object_id, static_cast<int32_t>(i));
    Batch batch(64, kWindow);
    source.next(&batch);
    EXPECT_EQ(batch.num_instances(), 64u);
    EXPECT_EQ(static_cast<int64_t>(batch.labels()[0]), 0);
}

static int dump_hdf5(const std::string& checkpoint, const std::string& outbase) {
    const std::vector<Hdf5Array> arrays = read_hdf5(checkpoint, {"word_representations-representations", "entity_representations-representations",
                                                                 "word_entity_mapping-transform", "word_entity_mapping-bias"});
    const char* suffix[4] = {"W", "E", "T", "b"};
    for (size_t i = 0; i < arrays.size(); ++i) {
        std::ofstream f(outbase + "." + suffix[i] + ".f32", std::ios::binary);
        f.write(reinterpret_cast<const char*>(arrays[i].data.data()), static_cast<std::streamsize>(arrays[i].data.size() * sizeof(float)));
        if (!f.good()) { std::fprintf(stderr, "cannot write %s.%s.f32\n", outbase.c_str(), suffix[i]); return 1; }
        std::printf("%s %llu %llu\n", suffix[i], arrays[i].dim0, arrays[i].dim1);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "--dump-hdf5") {
        try { return dump_hdf5(argv[2], argv[3]); }
        catch (const std::exception& e) { std::fprintf(stderr, "dump-hdf5: %s\n", e.what()); return 1; }
    }
    if (argc < 2) { std::fprintf(stderr, "usage: fold_tests <collection.trectext> [<case>]\n"); return 2; }
    g_collection = argv[1];
    log_to_stderr() = false;
    const std::vector<std::pair<const char*, std::function<void()>>> tests = {
        {"FoldIn.new_documents_in_index_order_and_refusals", test_new_documents},
        {"FoldIn.source_vocabulary_labels_and_weights", test_source},
        {"FoldIn.existing_constructor_is_unchanged", test_existing_constructor_is_unchanged},
    };
    int failed_tests = 0;
    for (const auto& t : tests) {
        if (argc > 2 && std::string(argv[2]) != t.first) continue;
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
