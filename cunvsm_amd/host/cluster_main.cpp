// cuNVSMCluster — k-means of a checkpoint's document rows on the device (nvsm_kmeans), written in the classification format that
// cuNVSMVisualize reads: a collection without classes gets its picture coloured by
//   cuNVSMCluster --num_clusters K --clusters_out c.txt model_3.hdf5 index
//   cuNVSMVisualize --object_classification c.txt --filter_unclassified --plot_out plot model_3.hdf5 index
//
//   cuNVSMCluster --num_clusters K [--limit N] [--l2_normalize] [--max_iter I] [--tol T] [--seed S] [--object_classification F]
//                 --clusters_out PATH  <model>_<epoch>.hdf5  <index>
//
// Without --object_classification the documents of the model are clustered in model order (the first --limit of them). With it
// only the classified documents the model knows are, chosen as cuNVSMVisualize --filter_unclassified chooses them, and purity,
// NMI and ARI of the clusters against the classes are printed. Output: "<docno> <cluster>" lines in model order in --clusters_out;
// on stdout one line per cluster (its size and the docno nearest its centre), then inertia and the iteration count.
// The index is the one the trainer reads; with a TREC-text collection pass the training run's --stopwords.
#include <sys/stat.h>

#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>

#include "../../include/cunvsm_amd.h"
#include "base.hpp"
#include "cluster_lib.hpp"
#include "flags.hpp"
#include "hdf5_writer.hpp"
#include "indri_index.hpp"
#include "query_lib.hpp"
#include "trectext_index.hpp"
#include "visualize_lib.hpp"

using namespace nvsm_host;

namespace {

std::string FLAGS_object_classification, FLAGS_clusters_out, FLAGS_stopwords;
bool FLAGS_l2_normalize, FLAGS_help, FLAGS_logtostderr;
int64_t FLAGS_num_clusters, FLAGS_limit, FLAGS_device, FLAGS_v, FLAGS_max_iter, FLAGS_seed;
double FLAGS_tol;

void define_flags(Flags* f) {
    f->define_int64("num_clusters", &FLAGS_num_clusters, 0, "Number of clusters K (required).");
    f->define_string("clusters_out", &FLAGS_clusters_out, "", "Where the <docno> <cluster> lines go (required).");
    f->define_string("object_classification", &FLAGS_object_classification, "", "Classification file, one document per line: <docno> <class>. "
                     "Cluster the classified documents only and print purity, NMI and ARI against the classes.");
    f->define_int64("limit", &FLAGS_limit, 0, "Keep the first N of the chosen rows (default: all).");
    f->define_bool("l2_normalize", &FLAGS_l2_normalize, false, "Divide every row by its norm first.");
    f->define_int64("max_iter", &FLAGS_max_iter, 300, "Lloyd iterations at most (sklearn's default).");
    f->define_double("tol", &FLAGS_tol, 1e-4, "Stop when the squared centre shift is at most tol times the mean column variance (sklearn's default).");
    f->define_int64("seed", &FLAGS_seed, 1, "Seed of the k-means++ start, at least 1.");
    f->define_string("stopwords", &FLAGS_stopwords, "", "Stop list applied while indexing a TREC-text collection: the training run's.");
    f->define_int64("device", &FLAGS_device, 0, "HIP device ordinal.");
    f->define_bool("help", &FLAGS_help, false, "Print the options and exit.");
    f->define_bool("logtostderr", &FLAGS_logtostderr, true, "Log to stderr (there is no log-file sink).");
    f->define_int64("v", &FLAGS_v, 0, "Verbosity of VLOG messages.");
}

void check_status(int status, const char* what) {
    if (status != NVSM_OK) NVSM_LOG(FATAL) << what << ": " << nvsm_last_error();
}
#define NVSM_CALL(expr) check_status((expr), #expr)

bool is_directory(const std::string& path) { struct stat st; return stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }
bool is_file(const std::string& path) { struct stat st; return stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode); }

int run(int argc, char** argv) {
    Flags flags;
    define_flags(&flags);
    const std::vector<std::string> args = flags.parse(argc, argv);
    verbosity() = static_cast<int>(FLAGS_v);
    log_to_stderr() = FLAGS_logtostderr;
    const std::string usage = "Usage: " + args[0] + " --num_clusters K [OPTIONS] --clusters_out <path> "
                              "<model>_<epoch>.hdf5 <TREC-text collection | Indri repository>\n" + flags.usage();
    if (FLAGS_help) { std::cout << usage; return 0; }
    if (args.size() != 3 || FLAGS_clusters_out.empty() || FLAGS_num_clusters == 0) {
        std::cerr << usage;
        NVSM_LOG(FATAL) << "--num_clusters, --clusters_out, the model and the index are required.";
    }
    NVSM_CHECK(FLAGS_num_clusters >= 1 && FLAGS_num_clusters <= NVSM_KMEANS_MAX_CLUSTERS) << "--num_clusters must be in [1, " << NVSM_KMEANS_MAX_CLUSTERS << "].";
    NVSM_CHECK(FLAGS_limit >= 0) << "--limit must not be negative.";
    NVSM_CHECK(FLAGS_max_iter >= 1 && FLAGS_max_iter <= 2147483647) << "--max_iter must be at least 1.";
    NVSM_CHECK(std::isfinite(FLAGS_tol) && FLAGS_tol >= 0.0) << "--tol must be finite and not negative.";
    NVSM_CHECK(FLAGS_seed >= 1) << "--seed must be at least 1.";
    const std::string model_path = args[1], index_path = args[2];
    const bool classified = !FLAGS_object_classification.empty();
    NVSM_CHECK(!classified || is_file(FLAGS_object_classification)) << "cannot read the classification file " << FLAGS_object_classification;
    NVSM_CHECK(is_file(model_path)) << "cannot read the model " << model_path;

    std::unique_ptr<IndexInterface> index;
    if (is_directory(index_path)) {
        if (!IndriDiskIndex::looks_like_repository(index_path)) NVSM_LOG(FATAL) << "Unable to open Indri parameters: " << index_path << " holds no manifest / index.";
        index.reset(IndriDiskIndex::open(index_path));
    } else {
        NVSM_CHECK(is_file(index_path)) << "cannot read collection " << index_path;
        NVSM_LOG(INFO) << "Indexing " << index_path << ".";
        index.reset(TrectextIndex::from_file(index_path, FLAGS_stopwords));
    }

    NVSM_LOG(INFO) << "Loading model.";
    const ModelPath where = split_model_path(model_path);
    Metadata meta;
    {
        std::ifstream f(where.meta_path, std::ios::binary);
        std::stringstream wire;
        wire << f.rdbuf();
        NVSM_CHECK(f.good() && meta.ParseFromString(wire.str())) << "cannot parse " << where.meta_path;
    }
    static const char* kNames[4] = {"word_representations-representations", "entity_representations-representations",
                                    "word_entity_mapping-transform", "word_entity_mapping-bias"};
    const std::vector<Hdf5Array> arrays = read_hdf5(model_path, {kNames[0], kNames[1], kNames[2], kNames[3]});
    const Hdf5Array &W = arrays[0], &E = arrays[1];
    const int64_t num_words = static_cast<int64_t>(W.dim0), dw = static_cast<int64_t>(W.dim1);
    const int64_t num_entities = static_cast<int64_t>(E.dim0), de = static_cast<int64_t>(E.dim1);
    if (num_words < 1 || num_entities < 1 || dw < 1 || de < 1 || dw > 2147483647 || de > 2147483647) NVSM_LOG(FATAL) << model_path << " holds an empty table";
    const ModelMappings maps = build_mappings(meta, num_words, num_entities);

    // the rows: the classified documents as cuNVSMVisualize chooses them, or every document of the model the index names
    std::vector<VisualRow> rows;
    if (classified) {
        std::unordered_map<std::string, int64_t> model_doc_of_docno;
        for (int64_t d = 0; d < num_entities; ++d)
            if (maps.index_object_of[static_cast<size_t>(d)] >= 0) model_doc_of_docno.emplace(index->docno(maps.index_object_of[static_cast<size_t>(d)]), d);
        std::ifstream in(FLAGS_object_classification);
        rows = select_rows(parse_classification(in, FLAGS_object_classification), model_doc_of_docno, true, FLAGS_limit);
    } else {
        for (int64_t d = 0; d < num_entities; ++d) {
            if (maps.index_object_of[static_cast<size_t>(d)] < 0) continue;
            if (FLAGS_limit > 0 && static_cast<int64_t>(rows.size()) >= FLAGS_limit) break;
            rows.push_back(VisualRow{d, index->docno(maps.index_object_of[static_cast<size_t>(d)]), ""});
        }
    }
    NVSM_LOG(INFO) << rows.size() << " documents to cluster.";
    NVSM_CHECK(static_cast<int64_t>(rows.size()) >= FLAGS_num_clusters) << "fewer documents (" << rows.size() << ") than clusters (" << FLAGS_num_clusters << ").";

    if (nvsm_device_count() < 1) NVSM_LOG(FATAL) << "no HIP device visible: cuNVSMCluster has no CPU path.";
    nvsm_model* model = nullptr;
    nvsm_config cfg;
    nvsm_config_default(&cfg);      // a handle for reading the tables only: plain SGD (no optimiser state), a token batch capacity
    cfg.num_words = num_words; cfg.num_entities = num_entities;
    cfg.word_repr_size = static_cast<int32_t>(dw); cfg.entity_repr_size = static_cast<int32_t>(de);
    cfg.window_size = 1; cfg.num_random_entities = 1; cfg.max_batch_size = 8;
    cfg.update_method = NVSM_SGD; cfg.adam_mode = NVSM_ADAM_NONE; cfg.nonlinearity = NVSM_TANH; cfg.batch_normalization = 0;
    cfg.device = static_cast<int32_t>(FLAGS_device);
    NVSM_CALL(nvsm_create(&cfg, &model));
    for (int i = 0; i < 4; ++i)
        NVSM_CALL(nvsm_set_param(model, kNames[i], arrays[static_cast<size_t>(i)].data.data(), static_cast<int64_t>(arrays[static_cast<size_t>(i)].data.size())));

    std::vector<int64_t> ids;
    for (const VisualRow& r : rows) ids.push_back(r.model_id);
    const int32_t k = static_cast<int32_t>(FLAGS_num_clusters);
    nvsm_kmeans_options opt;
    nvsm_kmeans_options_default(&opt);
    opt.ids = ids.data(); opt.num_rows = static_cast<int64_t>(ids.size());
    opt.l2_normalize = FLAGS_l2_normalize ? 1 : 0;
    opt.num_clusters = k; opt.max_iter = static_cast<int32_t>(FLAGS_max_iter); opt.tol = FLAGS_tol; opt.seed = FLAGS_seed;
    std::vector<int32_t> labels(ids.size());
    std::vector<float> centers(static_cast<size_t>(k) * static_cast<size_t>(de)), distances(ids.size());
    std::vector<int64_t> counts(static_cast<size_t>(k));
    double inertia = 0.0;
    int32_t n_iter = 0;
    NVSM_CALL(nvsm_kmeans(model, &opt, labels.data(), centers.data(), counts.data(), distances.data(), &inertia, &n_iter));
    nvsm_destroy(model);

    {
        std::ofstream out(FLAGS_clusters_out);
        write_clusters(out, rows, labels);
        out.flush();
        NVSM_CHECK(out.good()) << "cannot write " << FLAGS_clusters_out;
    }
    const std::vector<int64_t> nearest = nearest_members(labels, distances, k);
    for (int32_t j = 0; j < k; ++j)
        std::cout << "cluster " << j << ": " << counts[static_cast<size_t>(j)] << " documents, nearest "
                  << (nearest[static_cast<size_t>(j)] < 0 ? std::string("-") : rows[static_cast<size_t>(nearest[static_cast<size_t>(j)])].docno) << "\n";
    char buf[160];
    std::snprintf(buf, sizeof(buf), "inertia %.17g after %d iterations", inertia, static_cast<int>(n_iter));
    std::cout << buf << "\n";
    if (classified) {
        std::vector<std::string> classes;
        for (const VisualRow& r : rows) classes.push_back(r.label);
        const Contingency t = contingency(labels, classes);
        std::snprintf(buf, sizeof(buf), "purity %.17g nmi %.17g ari %.17g", cluster_purity(t), cluster_nmi(t), cluster_ari(t));
        std::cout << buf << "\n";
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return run(argc, argv);
    } catch (const FatalError& e) {
        std::cerr << e.what() << std::endl;      // (NVSM_LOG(FATAL) has logged its own; the library functions' have not been)
        return 1;
    } catch (const std::exception& e) {
        std::cerr << "Exception: " << e.what() << std::endl;
        return 1;
    }
}
