// cuNVSMVisualize — the reference's py/visualize.py (the body of visualize-reuters-collection.sh) on top of libcunvsm_amd.so's
// C ABI: the document rows of a checkpoint, restricted to the classified documents, as a two-dimensional t-SNE picture
// (nvsm_tsne: sklearn's exact method on the device; --tsne_method sparse: nvsm_tsne_sparse, sklearn's barnes_hut method at angle 0,
// for more than NVSM_TSNE_MAX_ROWS documents) or as TSV files for the embedding projector.
//
//   cuNVSMVisualize --object_classification f1 [f2 ...] --filter_unclassified [--limit N] [--l2_normalize]
//                   [--mode tsne|embedding_projector] [--tsne_method exact|sparse] [--tsne_neighbors N]
//                   --plot_out PATH  <model>_<epoch>.hdf5  <index>
//
// Each classification file has lines "<docno> <class>". The rows are the ascending model indices of the classified documents
// the model knows. Differences from py/visualize.py:
//   * mode tsne writes "<root>-<basename(classification)>.tsv" with lines docno<TAB>class<TAB>x<TAB>y (%.9g) instead of a
//     matplotlib figure (tools outside this tree can plot it); root is --plot_out without its extension.
//   * mode embedding_projector writes <plot_out>_vectors.tsv (%.5f) and <plot_out>_meta.tsv (header document_id<TAB>class),
//     class by class; it takes one classification file and needs no device.
//   * the index is the one the trainer reads; with a TREC-text collection pass the training run's --stopwords.
#include <sys/stat.h>

#include <fstream>
#include <memory>
#include <sstream>

#include "../../include/cunvsm_amd.h"
#include "base.hpp"
#include "flags.hpp"
#include "hdf5_writer.hpp"
#include "indri_index.hpp"
#include "query_lib.hpp"
#include "trectext_index.hpp"
#include "visualize_lib.hpp"

using namespace nvsm_host;

namespace {

std::string FLAGS_object_classification, FLAGS_mode, FLAGS_plot_out, FLAGS_stopwords, FLAGS_tsne_method;
bool FLAGS_filter_unclassified, FLAGS_l2_normalize, FLAGS_help, FLAGS_logtostderr;
int64_t FLAGS_limit, FLAGS_device, FLAGS_v, FLAGS_max_iter, FLAGS_tsne_neighbors;
double FLAGS_perplexity;

void define_flags(Flags* f) {
    f->define_string("object_classification", &FLAGS_object_classification, "", "Classification file, one document per line: <docno> <class>. "
                     "Further files follow as positional arguments in front of the model.");
    f->define_bool("filter_unclassified", &FLAGS_filter_unclassified, false, "Keep the classified documents only. Required, as in the "
                   "reference, which fails without it.");
    f->define_int64("limit", &FLAGS_limit, 0, "Keep the first N of the chosen rows (default: all).");
    f->define_bool("l2_normalize", &FLAGS_l2_normalize, false, "Divide every row by its norm first.");
    f->define_string("mode", &FLAGS_mode, "tsne", "tsne | embedding_projector.");
    f->define_string("plot_out", &FLAGS_plot_out, "", "Where the output goes (see the modes).");
    f->define_string("stopwords", &FLAGS_stopwords, "", "Stop list applied while indexing a TREC-text collection: the training run's.");
    f->define_double("perplexity", &FLAGS_perplexity, 30.0, "t-SNE perplexity (sklearn's default); must be below the number of rows.");
    f->define_int64("max_iter", &FLAGS_max_iter, 1000, "t-SNE iterations (sklearn's default).");
    f->define_string("tsne_method", &FLAGS_tsne_method, "exact", "exact | sparse: sparse keeps --tsne_neighbors affinities per document "
                     "(sklearn's barnes_hut method at angle 0) and serves more than 32768 documents.");
    f->define_int64("tsne_neighbors", &FLAGS_tsne_neighbors, 0, "Neighbours per document with --tsne_method sparse (0: sklearn's 3 * perplexity + 1).");
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
    const std::string usage = "Usage: " + args[0] + " --object_classification <file> [<file> ...] --filter_unclassified [OPTIONS] --plot_out <path> "
                              "<model>_<epoch>.hdf5 <TREC-text collection | Indri repository>\n" + flags.usage();
    if (FLAGS_help) { std::cout << usage; return 0; }
    if (args.size() < 3 || FLAGS_object_classification.empty() || FLAGS_plot_out.empty()) {
        std::cerr << usage;
        NVSM_LOG(FATAL) << "--object_classification, --plot_out, the model and the index are required.";
    }
    const bool projector = FLAGS_mode == "embedding_projector";
    if (!projector && FLAGS_mode != "tsne") NVSM_LOG(FATAL) << "--mode: '" << FLAGS_mode << "' is neither tsne nor embedding_projector.";
    NVSM_CHECK(FLAGS_filter_unclassified) << "without --filter_unclassified every document needs a class, which py/visualize.py does not "
                                             "handle either: pass --filter_unclassified.";
    NVSM_CHECK(FLAGS_limit >= 0) << "--limit must not be negative.";
    NVSM_CHECK(FLAGS_max_iter >= 1 && FLAGS_max_iter <= 2147483647) << "--max_iter must be at least 1.";
    const bool sparse = FLAGS_tsne_method == "sparse";
    if (!sparse && FLAGS_tsne_method != "exact") NVSM_LOG(FATAL) << "--tsne_method: '" << FLAGS_tsne_method << "' is neither exact nor sparse.";
    NVSM_CHECK(FLAGS_tsne_neighbors >= 0 && FLAGS_tsne_neighbors <= NVSM_TSNE_SPARSE_MAX_NEIGHBORS)
        << "--tsne_neighbors must be in [0, " << NVSM_TSNE_SPARSE_MAX_NEIGHBORS << "].";
    NVSM_CHECK(sparse || FLAGS_tsne_neighbors == 0) << "--tsne_neighbors belongs to --tsne_method sparse.";
    std::vector<std::string> class_paths = {FLAGS_object_classification};
    for (size_t i = 1; i + 2 < args.size(); ++i) class_paths.push_back(args[i]);
    const std::string model_path = args[args.size() - 2], index_path = args[args.size() - 1];
    for (const std::string& c : class_paths) NVSM_CHECK(is_file(c)) << "cannot read the classification file " << c;
    NVSM_CHECK(is_file(model_path)) << "cannot read the model " << model_path;
    NVSM_CHECK(!projector || class_paths.size() == 1) << "--mode embedding_projector writes one pair of files: give one classification file.";

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
    std::unordered_map<std::string, int64_t> model_doc_of_docno;
    for (int64_t d = 0; d < num_entities; ++d)
        if (maps.index_object_of[static_cast<size_t>(d)] >= 0) model_doc_of_docno.emplace(index->docno(maps.index_object_of[static_cast<size_t>(d)]), d);

    nvsm_model* model = nullptr;
    for (const std::string& class_path : class_paths) {
        std::ifstream in(class_path);
        const std::vector<VisualRow> rows = select_rows(parse_classification(in, class_path), model_doc_of_docno, FLAGS_filter_unclassified, FLAGS_limit);
        NVSM_LOG(INFO) << class_path << ": " << rows.size() << " classified documents of the model.";
        if (projector) {
            NVSM_CHECK(!rows.empty()) << class_path << " names no document of the model.";
            std::ofstream vectors(FLAGS_plot_out + "_vectors.tsv"), metadata(FLAGS_plot_out + "_meta.tsv");
            write_projector(vectors, metadata, rows, gather_rows(E.data, de, rows, FLAGS_l2_normalize), de);
            NVSM_CHECK(vectors.good() && metadata.good()) << "cannot write " << FLAGS_plot_out << "_vectors.tsv / _meta.tsv";
            continue;
        }
        NVSM_CHECK(rows.size() >= 2) << class_path << " names fewer than two documents of the model: nothing to embed.";
        if (!model) {
            if (nvsm_device_count() < 1) NVSM_LOG(FATAL) << "no HIP device visible: cuNVSMVisualize --mode tsne has no CPU path.";
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
        }
        std::vector<int64_t> ids;
        for (const VisualRow& r : rows) ids.push_back(r.model_id);
        nvsm_tsne_options opt;
        nvsm_tsne_options_default(&opt);      // TSNE(n_components=2, init='pca', random_state=0)
        opt.ids = ids.data(); opt.num_rows = static_cast<int64_t>(ids.size());
        opt.l2_normalize = FLAGS_l2_normalize ? 1 : 0;
        opt.perplexity = static_cast<float>(FLAGS_perplexity);
        opt.max_iter = static_cast<int32_t>(FLAGS_max_iter);
        std::vector<float> Y(2 * ids.size());
        double kl = 0.0;
        int32_t n_iter = 0;
        if (sparse) {
            nvsm_tsne_sparse_options sp;
            nvsm_tsne_sparse_options_default(&sp);
            sp.n_neighbors = static_cast<int32_t>(FLAGS_tsne_neighbors);
            NVSM_CALL(nvsm_tsne_sparse(model, &opt, &sp, Y.data(), &kl, &n_iter));
        } else {
            NVSM_CALL(nvsm_tsne(model, &opt, Y.data(), &kl, &n_iter));
        }
        NVSM_LOG(INFO) << "t-SNE of " << ids.size() << " documents: KL divergence " << kl << " after " << (n_iter + 1) << " iterations.";
        const std::string out_path = tsne_out_path(FLAGS_plot_out, class_path);
        std::ofstream out(out_path);
        write_tsne_tsv(out, rows, Y);
        out.flush();
        NVSM_CHECK(out.good()) << "cannot write " << out_path;
    }
    if (model) nvsm_destroy(model);
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
