// CPU unit tests of what cuNVSMQuery does on the host (cunvsm_amd/host/query_lib.hpp, read_hdf5 of hdf5_writer.hpp), and — with
// `--make-model <collection> <outbase> [<stop list> [<dataset to leave out>]]` — the writer of a small checkpoint in the trainer's formats whose parameters
// follow a closed formula of the index, for tests/test_query_cli_gpu.py. Driven by tests/test_query_host.py.
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <memory>
#include <sstream>

#include "../../cunvsm_amd/host/base.hpp"
#include "../../cunvsm_amd/host/hdf5_writer.hpp"
#include "../../cunvsm_amd/host/query_lib.hpp"
#include "../../cunvsm_amd/host/trectext_index.hpp"

using namespace nvsm_host;

static int g_failures = 0;
#define EXPECT_TRUE(c) do { if (!(c)) { std::printf("    EXPECT failed %s:%d: %s\n", __FILE__, __LINE__, #c); ++g_failures; } } while (0)
#define EXPECT_EQ(a, b) do { if (!((a) == (b))) { std::ostringstream os_; os_ << (a) << " vs " << (b); \
    std::printf("    EXPECT_EQ failed %s:%d: %s == %s (%s)\n", __FILE__, __LINE__, #a, #b, os_.str().c_str()); ++g_failures; } } while (0)

// the call must end in a FatalError whose message holds `word`
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

struct TempDir {
    std::string path;
    TempDir() {
        char name[] = "/tmp/nvsm_query_tests_XXXXXX";
        if (!mkdtemp(name)) throw std::runtime_error("mkdtemp failed");
        path = name;
    }
    ~TempDir() { const std::string cmd = "rm -rf '" + path + "'"; if (std::system(cmd.c_str()) != 0) std::printf("    could not remove %s\n", path.c_str()); }
};

static const std::vector<std::string> kNames = {"word_representations-representations", "entity_representations-representations",
                                                "word_entity_mapping-transform", "word_entity_mapping-bias"};

// ---- read_hdf5 ------------------------------------------------------------------------------------------------------------------------
static void test_hdf5_round_trip_is_bit_exact() {
    TempDir dir;
    std::vector<float> W(7 * 5), E(3 * 4), T(5 * 4), b(4);
    uint32_t bits = 0x12345678u;
    auto fill = [&](std::vector<float>& v) { for (float& x : v) { bits = bits * 1664525u + 1013904223u; std::memcpy(&x, &bits, 4); } };      // any bit pattern: NaNs, denormals
    fill(W); fill(E); fill(T); fill(b);
    W[0] = -0.0f; W[1] = std::numeric_limits<float>::denorm_min(); W[2] = std::numeric_limits<float>::infinity();
    const std::string file = dir.path + "/m_1.hdf5";
    write_hdf5(file, {{kNames[1], 3, 4, E.data()}, {kNames[3], 1, 4, b.data()}, {kNames[2], 5, 4, T.data()}, {kNames[0], 7, 5, W.data()}});
    const std::vector<Hdf5Array> got = read_hdf5(file, kNames);
    EXPECT_EQ(got.size(), 4u);
    if (got.size() != 4) return;
    const std::vector<float>* want[4] = {&W, &E, &T, &b};
    const unsigned long long dims[4][2] = {{7, 5}, {3, 4}, {5, 4}, {1, 4}};
    for (int i = 0; i < 4; ++i) {
        EXPECT_EQ(got[i].name, kNames[i]);
        EXPECT_EQ(got[i].dim0, dims[i][0]);
        EXPECT_EQ(got[i].dim1, dims[i][1]);
        EXPECT_EQ(got[i].data.size(), want[i]->size());
        EXPECT_TRUE(got[i].data.size() == want[i]->size() && std::memcmp(got[i].data.data(), want[i]->data(), want[i]->size() * 4) == 0);
    }
}

static void test_hdf5_refusals() {
    TempDir dir;
    std::vector<float> x(12, 1.f);
    const std::string three = dir.path + "/three_1.hdf5", flat = dir.path + "/flat_1.hdf5";
    write_hdf5(three, {{kNames[1], 3, 4, x.data()}, {kNames[3], 1, 4, x.data()}, {kNames[0], 3, 4, x.data()}});
    EXPECT_FATAL("holds no dataset word_entity_mapping-transform", read_hdf5(three, kNames));
    write_hdf5(flat, {{kNames[1], 3, 4, x.data()}, {kNames[3], 1, 4, x.data(), 1}, {kNames[2], 3, 4, x.data()}, {kNames[0], 3, 4, x.data()}});
    EXPECT_FATAL("word_entity_mapping-bias is not two-dimensional", read_hdf5(flat, kNames));
    EXPECT_EQ(read_hdf5(flat, {kNames[0], kNames[1]}).size(), 2u);
    EXPECT_FATAL("unable to open", read_hdf5(dir.path + "/absent_1.hdf5", kNames));
    { std::ofstream f(dir.path + "/text_1.hdf5"); f << "not an HDF5 file\n"; }
    EXPECT_FATAL("unable to open", read_hdf5(dir.path + "/text_1.hdf5", kNames));
}

// ---- where the meta file lies ---------------------------------------------------------------------------------------------------------
static void test_model_path() {
    TempDir dir;
    { std::ofstream f(dir.path + "/run_a_meta"); f << "x"; }
    ModelPath p = split_model_path(dir.path + "/run_a_12.hdf5");
    EXPECT_EQ(p.model_base, dir.path + "/run_a");
    EXPECT_EQ(p.meta_path, dir.path + "/run_a_meta");
    EXPECT_EQ(p.epoch, 12);
    p = split_model_path(dir.path + "/run_a_3_40.hdf5");              // a --dump_every dump: <model>_<epoch>_<batch>.hdf5
    EXPECT_EQ(p.model_base, dir.path + "/run_a_3");
    EXPECT_EQ(p.meta_path, dir.path + "/run_a_meta");
    EXPECT_EQ(p.epoch, 40);                                           // (py/query.py:145-146 reads the last number, whatever it counts)
    EXPECT_FATAL("no meta file", split_model_path(dir.path + "/other_1.hdf5"));
    EXPECT_FATAL("no epoch number", split_model_path(dir.path + "/run_a_final.hdf5"));
    EXPECT_FATAL("is not named", split_model_path("model.hdf5"));
}

// ---- topics and qrels -----------------------------------------------------------------------------------------------------------------
static void test_topic_parser() {
    std::istringstream in("7;boundary layer; laminar flow\r\n\r\n  \nq-2;\nthree;x\n9; wing ;\n");
    const std::vector<Topic> t = parse_topics(in, "topics");
    EXPECT_EQ(t.size(), 4u);
    if (t.size() != 4) return;
    EXPECT_EQ(t[0].id, std::string("7"));
    EXPECT_EQ(t[0].text, std::string("boundary layer; laminar flow"));          // only the FIRST ';' separates; the CR is gone
    EXPECT_EQ(t[1].id, std::string("q-2"));
    EXPECT_EQ(t[1].text, std::string(""));                                      // an empty text is a topic (it will have no terms)
    EXPECT_EQ(t[2].id, std::string("three"));
    EXPECT_EQ(t[3].text, std::string(" wing ;"));
    std::istringstream bad("1;fine\nno separator here\n");
    EXPECT_FATAL("topics:2", parse_topics(bad, "topics"));
}

static void test_qrel_parser() {
    Qrels q;
    std::istringstream in("1 0 d1 2\n1 Q0 d2 0\r\n\n2\t0\td1\t-1\n1 0 d3 1\n1 0 d1 3\n");
    parse_qrels(in, "qrels", &q);
    std::istringstream more("3 0 d9 1\n2 0 d2 1\n");
    parse_qrels(more, "qrels2", &q);                                  // several files accumulate
    EXPECT_EQ(q.size(), 3u);
    typedef std::vector<std::pair<std::string, int>> J;
    EXPECT_TRUE(q["1"] == J({{"d1", 3}, {"d2", 0}, {"d3", 1}}));     // file order; a docno judged twice keeps its last grade
    EXPECT_TRUE(q["2"] == J({{"d1", -1}, {"d2", 1}}));
    EXPECT_TRUE(q["3"] == J({{"d9", 1}}));
    for (const char* bad : {"1 0 d1\n", "1 0 d1 x\n", "1 0 d1 1 extra\n", "1 0 d1 1.5\n"}) {
        std::istringstream b(bad);
        Qrels scratch;
        EXPECT_FATAL("qrels:1", parse_qrels(b, "qrels", &scratch));
    }
}

// ---- the mappings of the meta file ----------------------------------------------------------------------------------------------------
static Metadata small_meta() {
    Metadata m;
    m.total_terms = 100;
    for (int i = 0; i < 3; ++i) { Metadata::TermInfo t; t.index_term_id = 10 + i; t.model_term_id = i; t.term_frequency = 5 * (i + 1); m.term.push_back(t); }
    for (int i = 0; i < 2; ++i) { Metadata::ObjectInfo o; o.index_object_id = 7 - i; o.model_object_id = i; m.object.push_back(o); }
    return m;
}

static void test_meta_mappings() {
    Metadata parsed;
    EXPECT_TRUE(parsed.ParseFromString(small_meta().SerializeAsString()));
    const ModelMappings maps = build_mappings(parsed, 4, 2);
    EXPECT_EQ(maps.total_terms, 100);
    EXPECT_EQ(maps.model_term_of.size(), 3u);
    EXPECT_EQ(maps.model_term_of.at(11), 1);
    EXPECT_TRUE(maps.term_frequency == std::vector<int64_t>({5, 10, 15, -1}));
    EXPECT_TRUE(maps.index_object_of == std::vector<int64_t>({7, 6}));
    EXPECT_EQ(maps.model_object_of.at(6), 1);
    const std::vector<float> w = self_information(maps, {0, 2, 2});
    EXPECT_EQ(w.size(), 3u);
    EXPECT_EQ(w[0], static_cast<float>(-std::log(5.0 / 100.0)));
    EXPECT_EQ(w[2], static_cast<float>(-std::log(15.0 / 100.0)));
    Metadata m = small_meta(); m.term[2].index_term_id = 10;
    EXPECT_FATAL("index term id 10 is named twice", build_mappings(m, 4, 2));
    m = small_meta(); m.term[2].model_term_id = 0;
    EXPECT_FATAL("model term id 0 is named twice", build_mappings(m, 4, 2));
    m = small_meta();
    EXPECT_FATAL("model term id 2 is outside", build_mappings(m, 2, 2));
    m = small_meta(); m.object[1].model_object_id = 0;
    EXPECT_FATAL("model object id 0 is named twice", build_mappings(m, 4, 2));
    m = small_meta(); m.object[1].index_object_id = 7;
    EXPECT_FATAL("index object id 7 is named twice", build_mappings(m, 4, 2));
    m = small_meta();
    EXPECT_FATAL("model object id 1 is outside", build_mappings(m, 4, 1));
}

// ---- a topic's text as model terms ----------------------------------------------------------------------------------------------------
static void test_query_terms() {
    TrectextIndex index;
    std::istringstream collection("<DOC>\n<DOCNO> a </DOCNO>\n<TEXT>\nthe wing of the aircraft\n</TEXT>\n</DOC>\n"
                                  "<DOC>\n<DOCNO> b </DOCNO>\n<TEXT>\nboundary layer flow\n</TEXT>\n</DOC>\n");
    index.load(collection, {"the", "of"});
    Metadata meta;
    meta.total_terms = 5;
    int next = 0;
    for (const char* word : {"wing", "boundary", "flow"}) {           // "aircraft" and "layer" are in the index, not in the model
        Metadata::TermInfo t; t.index_term_id = static_cast<int32_t>(index.term(std::string(word))); t.model_term_id = next++; t.term_frequency = 1;
        meta.term.push_back(t);
    }
    const ModelMappings maps = build_mappings(meta, 3, 1);
    std::vector<int64_t> terms;
    EXPECT_TRUE(query_terms(&index, maps, "The WING, the flow; wing!", false, &terms));
    EXPECT_TRUE(terms == std::vector<int64_t>({0, 2, 0}));           // stopped words skipped, a repeated word kept twice
    EXPECT_TRUE(query_terms(&index, maps, "wing aircraft zeppelin", false, &terms));
    EXPECT_TRUE(terms == std::vector<int64_t>({0}));
    EXPECT_TRUE(!query_terms(&index, maps, "wing aircraft", true, &terms));       // strict: a term outside the model skips the query
    EXPECT_TRUE(!query_terms(&index, maps, "the wing", true, &terms));            // ... and so does a stopped one (index id 0)
    EXPECT_TRUE(query_terms(&index, maps, "flow wing", true, &terms));
    EXPECT_TRUE(terms == std::vector<int64_t>({2, 0}));
    EXPECT_TRUE(!query_terms(&index, maps, "aircraft layer zeppelin", false, &terms) && terms.empty());
    EXPECT_TRUE(!query_terms(&index, maps, "", false, &terms));
    EXPECT_TRUE(!query_terms(&index, maps, " ;,", true, &terms));
}

// ---- --make-model ---------------------------------------------------------------------------------------------------------------------
static void write_raw(const std::string& path, const std::vector<float>& v) {
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(v.data()), static_cast<std::streamsize>(v.size() * sizeof(float)));
    if (!f.good()) throw std::runtime_error("cannot write " + path);
}

// <outbase>_meta, <outbase>_3.hdf5, <outbase>.{W,E,T,b}.f32 (the arrays as written) and <outbase>.map.txt. Every 7th index term and
// every 9th document stay outside the model; parameters are closed formulas of the model ids. `leave_out` names a dataset the
// checkpoint is to lack (what a reader must refuse).
static int make_model(const std::string& collection, const std::string& outbase, const std::string& stopwords, const std::string& leave_out) {
    std::unique_ptr<TrectextIndex> index(TrectextIndex::from_file(collection, stopwords));
    const int dw = 12, de = 36;
    Metadata meta;
    meta.total_terms = static_cast<int32_t>(index->termCount());
    std::ofstream dump(outbase + ".map.txt");
    dump << "total_terms " << meta.total_terms << "\n";
    for (const VocabularyEntry& v : index->vocabulary()) {
        if (v.term_id % 7 == 0) continue;
        Metadata::TermInfo t;
        t.index_term_id = static_cast<int32_t>(v.term_id); t.model_term_id = static_cast<int32_t>(meta.term.size());
        t.term_frequency = static_cast<int32_t>(v.total_count);
        meta.term.push_back(t);
        dump << "term " << t.index_term_id << " " << t.model_term_id << " " << t.term_frequency << " " << v.term << "\n";
    }
    for (DOCID_T d = index->documentBase(); d < index->documentMaximum(); ++d) {
        if (d % 9 == 0) continue;
        Metadata::ObjectInfo o;
        o.index_object_id = static_cast<int32_t>(d); o.model_object_id = static_cast<int32_t>(meta.object.size());
        meta.object.push_back(o);
        dump << "object " << o.index_object_id << " " << o.model_object_id << " " << index->docno(d) << "\n";
    }
    dump.close();
    const size_t V = meta.term_size(), D = meta.object_size();
    std::vector<float> W(V * dw), E(D * de), T(static_cast<size_t>(dw) * de), b(de);
    for (size_t t = 0; t < V; ++t) for (int j = 0; j < dw; ++j) W[t * dw + j] = static_cast<float>(std::sin(0.37 * (t + 1) + 1.3 * j));
    for (size_t d = 0; d < D; ++d) for (int j = 0; j < de; ++j) E[d * de + j] = static_cast<float>(std::cos(0.11 * (d + 1) * (j + 1) + 0.5 * j));
    for (int i = 0; i < dw; ++i) for (int j = 0; j < de; ++j) T[static_cast<size_t>(i) * de + j] = static_cast<float>(0.3 * std::sin(0.7 * i - 0.2 * j + 0.1));
    for (int j = 0; j < de; ++j) b[j] = static_cast<float>(0.05 * j - 0.4);
    {
        std::ofstream f(outbase + "_meta", std::ios::binary);
        const std::string wire = meta.SerializeAsString();
        f.write(wire.data(), static_cast<std::streamsize>(wire.size()));
    }
    std::vector<Hdf5Dataset> datasets = {{kNames[1], D, static_cast<unsigned long long>(de), E.data()}, {kNames[3], 1ull, static_cast<unsigned long long>(de), b.data()},
                                         {kNames[2], static_cast<unsigned long long>(dw), static_cast<unsigned long long>(de), T.data()},
                                         {kNames[0], V, static_cast<unsigned long long>(dw), W.data()}};
    for (size_t i = datasets.size(); i-- > 0;)
        if (datasets[i].name == leave_out) datasets.erase(datasets.begin() + static_cast<long>(i));
    write_hdf5(outbase + "_3.hdf5", datasets);
    write_raw(outbase + ".W.f32", W); write_raw(outbase + ".E.f32", E); write_raw(outbase + ".T.f32", T); write_raw(outbase + ".b.f32", b);
    std::printf("model %zu words x %d, %zu documents x %d\n", V, dw, D, de);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && std::string(argv[1]) == "--make-model") {
        try { return make_model(argv[2], argv[3], argc >= 5 ? argv[4] : "", argc >= 6 ? argv[5] : ""); }
        catch (const std::exception& e) { std::fprintf(stderr, "make-model: %s\n", e.what()); return 1; }
    }
    log_to_stderr() = false;
    const std::vector<std::pair<const char*, std::function<void()>>> tests = {
        {"Hdf5Reader.round_trip_is_bit_exact", test_hdf5_round_trip_is_bit_exact},
        {"Hdf5Reader.refusals", test_hdf5_refusals},
        {"ModelPath.meta_file_and_batch_fallback", test_model_path},
        {"Topics.parser", test_topic_parser},
        {"Qrels.parser", test_qrel_parser},
        {"Meta.mappings_and_their_refusals", test_meta_mappings},
        {"Topics.terms_out_of_vocabulary_and_strict", test_query_terms},
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
