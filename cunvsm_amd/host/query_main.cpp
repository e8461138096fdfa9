// cuNVSMQuery — the reference's py/query.py on top of libcunvsm_amd.so's C ABI: from what cuNVSMTrainModel writes
// ("<output>_meta", "<output>_<epoch>[_<batch>].hdf5") to one TREC run per topic file and, with --qrels, the retrieval metrics
// that pick the epoch (rank-cranfield-collection.sh), computed on the device by nvsm_evaluate in the same call that ranks.
//
//   cuNVSMQuery --index <trectext file | Indri repository> --topics f1 [f2 ...] [OPTIONS] <model>_<epoch>.hdf5 <run_out>
//
// Differences from py/query.py, all forced by what exists on this platform:
//   * the index is the one the trainer reads (host/trectext_index.hpp, host/indri_index.hpp); topics are tokenised with the
//     trectext tokenizer. With a TREC-text collection the SAME --stopwords as at training time is needed, or the term ids differ.
//   * the written score is the cosine similarity nvsm_rank returns; the reference writes cos - 1 through an external writer —
//     the same ranking.
//   * ties in a ranking are broken by ascending model document id, not by docno.
//   * not offered: --rerank_exact_matching_documents (its place is taken by --rerank tfidf, below), --num_workers, --l2norm_phrase
//     (see --help).
// The last stage of rank-cranfield-collection.sh — a query-likelihood run and its fusion with the NVSM run (py/combine_runs.py
// --alpha) — is --qlm / --ensemble_alpha: the collection goes to HBM as the token arena the trainer would upload (token_arena.hpp:
// IndexSource's term mapping and out-of-vocabulary rule, documents in model id order) and nvsm_lexical_rank / nvsm_rank_ensemble do
// the rest. The lexical model is over the MODEL's vocabulary, not Indri's. --qlm_prf makes the lexical run, and with it
// the fusion, the reference's "QLM w/ PRF": nvsm_lexical_rank_prf / nvsm_rank_ensemble_prf (RM3). --qlm_sdm makes it the
// sequential dependence model's — terms, exact adjacent pairs, pairs in a window: nvsm_sdm_rank / nvsm_rank_ensemble_sdm.
// py/combine_runs.py's supervised mode (--qrel --num_folds --alpha_stepsize) is --ensemble_qrel: the fusion's weight is chosen per fold
// of the topics on a grid by nvsm_rank_ensemble_cv.
// py/query.py's --rerank_exact_matching_documents — a lexical first stage names each topic's candidates and the model ranks only those —
// is --rerank tfidf | okapi | jm | dirichlet with --rerank_depth: nvsm_rerank over the same uploaded collection, the candidates handed
// over on the device. --tfidf_run_out writes the TF-IDF first stage's own run (nvsm_tfidf_rank).
#include <sys/stat.h>

#include <cmath>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <memory>
#include <set>
#include <sstream>

#include "../../include/cunvsm_amd.h"
#include "base.hpp"
#include "flags.hpp"
#include "hdf5_writer.hpp"
#include "indri_index.hpp"
#include "query_lib.hpp"
#include "token_arena.hpp"
#include "trectext_index.hpp"

using namespace nvsm_host;

namespace {

std::string FLAGS_index, FLAGS_topics, FLAGS_stopwords, FLAGS_top_k, FLAGS_qrels, FLAGS_cutoffs, FLAGS_qlm, FLAGS_qlm_param, FLAGS_qlm_run_out,
    FLAGS_ensemble_alpha, FLAGS_score_normalizer, FLAGS_ensemble_qrel, FLAGS_ensemble_measure, FLAGS_rerank, FLAGS_tfidf_run_out, FLAGS_lexical_index, FLAGS_sdm_weights;
bool FLAGS_linear, FLAGS_self_information, FLAGS_strict, FLAGS_per_query, FLAGS_logtostderr, FLAGS_rerank_exact_matching_documents,
    FLAGS_l2norm_phrase, FLAGS_help, FLAGS_qlm_prf, FLAGS_qlm_sdm, FLAGS_lexical_positions;
double FLAGS_bias_coefficient, FLAGS_qlm_fb_orig_weight, FLAGS_alpha_stepsize;
int64_t FLAGS_num_queries, FLAGS_device, FLAGS_v, FLAGS_num_workers, FLAGS_qlm_fb_docs, FLAGS_qlm_fb_terms, FLAGS_num_folds, FLAGS_ensemble_seed,
    FLAGS_rerank_depth, FLAGS_sdm_window;

void define_flags(Flags* f) {
    f->define_string("index", &FLAGS_index, "", "TREC-text collection file or Indri repository directory, as given to cuNVSMTrainModel.");
    f->define_string("topics", &FLAGS_topics, "", "Topic file, one query per line: <topic id>;<text>. Further topic files follow as "
                     "positional arguments in front of the model.");
    f->define_string("stopwords", &FLAGS_stopwords, "", "Stop list applied while indexing a TREC-text collection. Must be the one used at "
                     "training time: term ids are assigned while indexing, and the meta file maps THOSE ids to the model's.");
    f->define_string("top_k", &FLAGS_top_k, "", "Documents per topic: a number (default 1000, clipped to the number of documents of the "
                     "model), 'all', or qrel file names (blank-separated): each topic is then ranked among its judged documents only.");
    f->define_bool("linear", &FLAGS_linear, false, "No nonlinearity behind the projection (default: tanh).");
    f->define_double("bias_coefficient", &FLAGS_bias_coefficient, 0.0, "Accepted as by the reference, which never applies the bias: "
                     "py/nvsm/base.py keeps the bias only where the coefficient is 0. Not fixed here.");
    f->define_bool("self_information", &FLAGS_self_information, false, "Weight query terms by -log(term frequency / total terms).");
    f->define_bool("strict", &FLAGS_strict, false, "Skip a topic when any of its terms is out of vocabulary (default: skip the term).");
    f->define_int64("num_queries", &FLAGS_num_queries, 0, "Keep the first n topics of every topic file (default: all).");
    f->define_string("qrels", &FLAGS_qrels, "", "Qrel file names (blank-separated, lines of <topic> <iteration> <docno> <grade>): evaluates "
                     "every topic file's ranking on the device and prints the means in trec_eval's layout.");
    f->define_string("cutoffs", &FLAGS_cutoffs, "5,10,20,100,1000", "Rank cutoffs of P, recall and ndcg_cut (ascending, at most 8).");
    f->define_bool("per_query", &FLAGS_per_query, false, "With --qrels: also print every evaluated topic's metrics.");
    f->define_int64("device", &FLAGS_device, 0, "HIP device ordinal.");
    f->define_bool("rerank_exact_matching_documents", &FLAGS_rerank_exact_matching_documents, false, "NOT OFFERED: it needs Indri's TF-IDF "
                   "query environment, which does not exist here. --rerank tfidf is the same retrieve-then-rerank over the model's vocabulary.");
    f->define_int64("num_workers", &FLAGS_num_workers, 0, "NOT OFFERED (accepted and ignored): every topic file is one GPU pass.");
    f->define_bool("l2norm_phrase", &FLAGS_l2norm_phrase, false, "NOT OFFERED: py/nvsm/base.py has no such argument (the reference's "
                   "py/query.py fails when it is given).");
    f->define_string("qlm", &FLAGS_qlm, "", "jm | dirichlet: also rank every topic with the query-likelihood model (Jelinek-Mercer or Dirichlet "
                     "smoothing) over the collection in the model's vocabulary, uploaded to the device. Needs --qlm_run_out or --ensemble_alpha.");
    f->define_string("qlm_param", &FLAGS_qlm_param, "auto", "auto | <number>: lambda in (0, 1) for jm (auto: 0.5), mu > 0 for dirichlet (auto: the "
                     "average document length).");
    f->define_string("qlm_run_out", &FLAGS_qlm_run_out, "", "With --qlm: prefix of the query-likelihood runs, written as <prefix>-<topic file> in TREC format.");
    f->define_string("ensemble_alpha", &FLAGS_ensemble_alpha, "", "With --qlm: <run_out> holds the fusion of the NVSM ranking (weight alpha in [0, 1]) and "
                     "the query-likelihood ranking (weight 1 - alpha), up to 2 x top_k documents per topic, and the printed means are the fused list's.");
    f->define_string("score_normalizer", &FLAGS_score_normalizer, "standardize", "standardize | minmax | none: how --ensemble_alpha normalises each "
                     "list's scores per topic before mixing them.");
    f->define_string("ensemble_qrel", &FLAGS_ensemble_qrel, "", "With --qlm, instead of --ensemble_alpha (the two exclude each other): qrel file names "
                     "(blank-separated). The weight alpha is chosen by cross-validation over the topics: every alpha of the grid 0, stepsize, "
                     "2 x stepsize, ... < 1 is evaluated, and each fold's topics are fused with the alpha whose mean --ensemble_measure over the "
                     "OTHER folds' topics is largest (ties: the largest alpha). <run_out> holds the fused lists; the printed means are theirs.");
    f->define_int64("num_folds", &FLAGS_num_folds, 20, "With --ensemble_qrel: folds of the ranked topics, 2 .. their number.");
    f->define_double("alpha_stepsize", &FLAGS_alpha_stepsize, 0.05, "With --ensemble_qrel: step of the alpha grid; at most 1024 points.");
    f->define_string("ensemble_measure", &FLAGS_ensemble_measure, "map_cut_1000", "With --ensemble_qrel: the training measure, a name of the printed "
                     "metrics (map, ndcg, P_5, ...) or map_cut_<d>: map over the first d entries of the fused list, and the printed metrics are then "
                     "those of the lists cut at d.");
    f->define_int64("ensemble_seed", &FLAGS_ensemble_seed, 1, "With --ensemble_qrel: the folds are contiguous runs of the ranked topics after a "
                    "permutation. seed s > 0: a Fisher-Yates pass driven by std::minstd_rand0(s) — for i = n - 1 down to 1, j = rng() % (i + 1), "
                    "swap topics i and j. seed 0: topic-file order. (The reference shuffles with an unseeded generator.)");
    f->define_bool("qlm_prf", &FLAGS_qlm_prf, false, "With --qlm: pseudo-relevance feedback (RM3). Every topic is expanded with the most probable "
                   "terms of its best documents' relevance model; the --qlm_run_out runs and the --ensemble_alpha fusion use the expanded ranking.");
    f->define_int64("qlm_fb_docs", &FLAGS_qlm_fb_docs, 10, "With --qlm_prf: feedback documents per topic.");
    f->define_int64("qlm_fb_terms", &FLAGS_qlm_fb_terms, 10, "With --qlm_prf: expansion terms per topic.");
    f->define_double("qlm_fb_orig_weight", &FLAGS_qlm_fb_orig_weight, 0.5, "With --qlm_prf: weight of the original query in the expanded one, in [0, 1].");
    f->define_string("rerank", &FLAGS_rerank, "", "tfidf | okapi | jm | dirichlet: retrieve-then-rerank. A lexical first stage over the collection in the "
                     "model's vocabulary (TF-IDF with Robertson's or Okapi's idf, or the query-likelihood model at its automatic parameter) retrieves "
                     "--rerank_depth documents per topic and the model ranks only those; <run_out> and the printed means are the re-ranked lists. "
                     "Excludes --ensemble_alpha, --ensemble_qrel and qrel files as --top_k.");
    f->define_int64("rerank_depth", &FLAGS_rerank_depth, 1000, "With --rerank: candidates per topic, clipped to the collection; at most 4096.");
    f->define_string("tfidf_run_out", &FLAGS_tfidf_run_out, "", "Prefix of the TF-IDF runs (Robertson's idf; Okapi's with --rerank okapi), written as "
                     "<prefix>-<topic file> in TREC format, --top_k documents per topic (with --rerank: the --rerank_depth candidates).");
    f->define_bool("qlm_sdm", &FLAGS_qlm_sdm, false, "With --qlm: the sequential dependence model. Every topic is ranked by its terms, its adjacent pairs "
                   "of terms as exact phrases and those pairs within a window; the --qlm_run_out runs and the --ensemble_alpha fusion use that ranking. "
                   "Not together with --qlm_prf or --ensemble_qrel.");
    f->define_string("sdm_weights", &FLAGS_sdm_weights, "0.85,0.10,0.05", "With --qlm_sdm: t,o,u, the weights of the terms, the ordered pairs and the unordered "
                     "pairs; not negative, not all zero.");
    f->define_int64("sdm_window", &FLAGS_sdm_window, 8, "With --qlm_sdm: the window of the unordered pairs, in [2, 64].");
    f->define_string("lexical_index", &FLAGS_lexical_index, "", "auto | always | never, with --qlm or --rerank: build the inverted index of the uploaded "
                     "collection and let the lexical rankings fill their scores from its postings (always), from the token arena (never) or "
                     "whichever is cheaper per round (auto). Every run file is byte for byte the one written without the flag.");
    f->define_bool("lexical_positions", &FLAGS_lexical_positions, false, "With --lexical_index and --qlm_sdm: build the positional layer of the inverted "
                   "index behind it, so that the dependence model's rounds may be served from the postings. Every run file is byte for byte the "
                   "one written without the flag.");
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
bool exists(const std::string& path) { struct stat st; return stat(path.c_str(), &st) == 0; }
std::string basename_of(const std::string& path) { const size_t cut = path.rfind('/'); return cut == std::string::npos ? path : path.substr(cut + 1); }

std::vector<std::string> split_blanks(const std::string& s) {
    std::istringstream in(s);
    std::vector<std::string> out;
    for (std::string w; in >> w;) out.push_back(w);
    return out;
}

Qrels read_qrels(const std::vector<std::string>& paths) {
    Qrels qrels;
    for (const std::string& path : paths) {
        std::ifstream f(path);
        NVSM_CHECK(f.good()) << "cannot read " << path;
        parse_qrels(f, path, &qrels);
    }
    return qrels;
}

std::vector<int32_t> parse_cutoffs(const std::string& s) {
    std::vector<int32_t> cutoffs;
    std::istringstream in(s);
    for (std::string item; std::getline(in, item, ',');) {
        char* end = nullptr;
        const long c = std::strtol(item.c_str(), &end, 10);
        if (item.empty() || *end != '\0' || c < 1 || c > 2147483647L) NVSM_LOG(FATAL) << "--cutoffs: '" << item << "' is no rank cutoff";
        if (!cutoffs.empty() && c <= cutoffs.back()) NVSM_LOG(FATAL) << "--cutoffs must ascend";
        cutoffs.push_back(static_cast<int32_t>(c));
    }
    if (cutoffs.size() > NVSM_EVAL_MAX_CUTOFFS) NVSM_LOG(FATAL) << "--cutoffs: at most " << NVSM_EVAL_MAX_CUTOFFS;
    return cutoffs;
}

std::vector<std::string> metric_names(const std::vector<int32_t>& cutoffs) {      // trec_eval's, in the order of a metric row
    std::vector<std::string> names = {"num_ret", "num_rel", "num_rel_ret", "map", "Rprec", "recip_rank", "ndcg"};
    for (const int32_t c : cutoffs)
        for (const char* m : {"P_", "recall_", "ndcg_cut_"}) names.push_back(m + std::to_string(c));
    return names;
}

void print_metric(const std::string& name, const std::string& topic, double value, bool integral) {      // "map<TAB>all<TAB>0.1234"
    if (integral) std::printf("%s\t%s\t%lld\n", name.c_str(), topic.c_str(), static_cast<long long>(value));
    else std::printf("%s\t%s\t%.4f\n", name.c_str(), topic.c_str(), value);
}

int run(int argc, char** argv) {
    Flags flags;
    define_flags(&flags);
    const std::vector<std::string> args = flags.parse(argc, argv);
    verbosity() = static_cast<int>(FLAGS_v);
    log_to_stderr() = FLAGS_logtostderr;
    const std::string usage = "Usage: " + args[0] + " --index <TREC-text collection | Indri repository> --topics <file> [<file> ...] [OPTIONS] "
                              "<model>_<epoch>.hdf5 <run_out>\n" + flags.usage();
    if (FLAGS_help) { std::cout << usage; return 0; }
    if (args.size() < 3 || FLAGS_index.empty() || FLAGS_topics.empty()) {
        std::cerr << usage;
        NVSM_LOG(FATAL) << "--index, --topics, the model and the run's name are required.";
    }
    NVSM_CHECK(!FLAGS_rerank_exact_matching_documents) << "--rerank_exact_matching_documents is not offered: it needs Indri's TF-IDF query environment. "
                                                          "--rerank tfidf re-ranks a TF-IDF first stage over the model's vocabulary.";
    NVSM_CHECK(!FLAGS_l2norm_phrase) << "--l2norm_phrase is not offered: py/nvsm/base.py has no such argument.";
    if (FLAGS_num_workers != 0) NVSM_LOG(WARNING) << "--num_workers is ignored: every topic file is one GPU pass.";
    if (FLAGS_bias_coefficient != 0.0)
        NVSM_LOG(WARNING) << "--bias_coefficient " << FLAGS_bias_coefficient << ": as in the reference, the bias is never applied "
                             "(py/nvsm/base.py:228-233 keeps it only where the coefficient is 0).";
    NVSM_CHECK(FLAGS_num_queries >= 0) << "--num_queries must not be negative.";
    std::vector<std::string> topic_paths = {FLAGS_topics};
    for (size_t i = 1; i + 2 < args.size(); ++i) topic_paths.push_back(args[i]);
    const std::string model_path = args[args.size() - 2], run_out = args[args.size() - 1];
    for (const std::string& t : topic_paths) NVSM_CHECK(is_file(t)) << "cannot read the topic file " << t;
    NVSM_CHECK(is_file(model_path)) << "cannot read the model " << model_path;
    const std::vector<int32_t> cutoffs = parse_cutoffs(FLAGS_cutoffs);

    // ---- --qlm / --ensemble_alpha (rank-cranfield-collection.sh's last stage)
    const bool with_qlm = !FLAGS_qlm.empty(), with_ensemble = !FLAGS_ensemble_alpha.empty(), with_cv = !FLAGS_ensemble_qrel.empty();
    const bool with_fusion = with_ensemble || with_cv;
    NVSM_CHECK(!(with_ensemble && with_cv)) << "--ensemble_alpha and --ensemble_qrel are mutually exclusive: the weight is either given or chosen by cross-validation.";
    nvsm_lexical_options lex;
    nvsm_lexical_options_default(&lex);
    nvsm_ensemble_options ens;
    nvsm_ensemble_options_default(&ens);
    if (with_qlm) {
        if (FLAGS_qlm == "jm") lex.method = NVSM_LEX_JM;
        else if (FLAGS_qlm == "dirichlet") lex.method = NVSM_LEX_DIRICHLET;
        else NVSM_LOG(FATAL) << "--qlm: '" << FLAGS_qlm << "' is neither jm nor dirichlet.";
        if (FLAGS_qlm_param != "auto") {
            char* end = nullptr;
            const double v = std::strtod(FLAGS_qlm_param.c_str(), &end);
            if (FLAGS_qlm_param.empty() || *end != '\0' || !(v > 0.0) || (lex.method == NVSM_LEX_JM && !(v < 1.0)))
                NVSM_LOG(FATAL) << "--qlm_param: '" << FLAGS_qlm_param << "' is neither auto, nor a lambda in (0, 1) (jm), nor a mu > 0 (dirichlet).";
            lex.param = static_cast<float>(v);
        }
        NVSM_CHECK(with_fusion || !FLAGS_qlm_run_out.empty()) << "--qlm needs --qlm_run_out, --ensemble_alpha or --ensemble_qrel: nothing would be written.";
    } else {
        NVSM_CHECK(!with_fusion && FLAGS_qlm_run_out.empty() && FLAGS_qlm_param == "auto" && FLAGS_score_normalizer == "standardize")
            << "--qlm_param, --qlm_run_out, --ensemble_alpha, --ensemble_qrel and --score_normalizer need --qlm.";
    }
    std::vector<float> cv_alphas;
    int32_t cv_measure = NVSM_EVAL_AP, cv_depth = 0;
    if (with_cv) {
        NVSM_CHECK(FLAGS_qrels.empty()) << "--ensemble_qrel evaluates the fused lists with its own judgments: leave --qrels out.";
        NVSM_CHECK(FLAGS_num_folds >= 2 && FLAGS_num_folds <= 2147483647) << "--num_folds must be at least 2.";
        NVSM_CHECK(FLAGS_ensemble_seed >= 0 && FLAGS_ensemble_seed <= 2147483646) << "--ensemble_seed must be in [0, 2147483646].";
        NVSM_CHECK(FLAGS_alpha_stepsize > 0.0 && FLAGS_alpha_stepsize <= 1.0 && std::ceil(1.0 / FLAGS_alpha_stepsize) <= NVSM_SWEEP_MAX_ALPHAS)
            << "--alpha_stepsize must be in (0, 1] and give at most " << NVSM_SWEEP_MAX_ALPHAS << " alphas.";
        // np.arange(0.0, 1.0, stepsize): ceil(1 / stepsize) points i * stepsize in double, narrowed to float32
        const int64_t points = static_cast<int64_t>(std::ceil(1.0 / FLAGS_alpha_stepsize));
        for (int64_t i = 0; i < points; ++i) cv_alphas.push_back(static_cast<float>(static_cast<double>(i) * FLAGS_alpha_stepsize));
        if (!ensemble_measure(FLAGS_ensemble_measure, metric_names(cutoffs), &cv_measure, &cv_depth))
            NVSM_LOG(FATAL) << "--ensemble_measure: '" << FLAGS_ensemble_measure << "' is neither a printed metric (num_ret, num_rel and num_rel_ret "
                               "are not offered) nor map_cut_<depth>.";
    } else {
        NVSM_CHECK(FLAGS_num_folds == 20 && FLAGS_alpha_stepsize == 0.05 && FLAGS_ensemble_measure == "map_cut_1000" && FLAGS_ensemble_seed == 1)
            << "--num_folds, --alpha_stepsize, --ensemble_measure and --ensemble_seed need --ensemble_qrel.";
    }
    nvsm_feedback_options fb;
    nvsm_feedback_options_default(&fb);
    const bool with_prf = FLAGS_qlm_prf;
    if (with_prf) {
        NVSM_CHECK(with_qlm) << "--qlm_prf needs --qlm.";
        NVSM_CHECK(FLAGS_qlm_fb_docs >= 1 && FLAGS_qlm_fb_docs <= NVSM_FEEDBACK_MAX_DOCS) << "--qlm_fb_docs must be in [1, " << NVSM_FEEDBACK_MAX_DOCS << "].";
        NVSM_CHECK(FLAGS_qlm_fb_terms >= 1 && FLAGS_qlm_fb_terms <= 2147483647) << "--qlm_fb_terms must be at least 1.";
        NVSM_CHECK(FLAGS_qlm_fb_orig_weight >= 0.0 && FLAGS_qlm_fb_orig_weight <= 1.0) << "--qlm_fb_orig_weight must be in [0, 1].";
        fb.fb_docs = static_cast<int32_t>(FLAGS_qlm_fb_docs);
        fb.fb_terms = static_cast<int32_t>(FLAGS_qlm_fb_terms);
        fb.orig_weight = static_cast<float>(FLAGS_qlm_fb_orig_weight);
    } else {
        NVSM_CHECK(FLAGS_qlm_fb_docs == 10 && FLAGS_qlm_fb_terms == 10 && FLAGS_qlm_fb_orig_weight == 0.5)
            << "--qlm_fb_docs, --qlm_fb_terms and --qlm_fb_orig_weight need --qlm_prf.";
    }
    nvsm_sdm_options sdm;
    nvsm_sdm_options_default(&sdm);
    const bool with_sdm = FLAGS_qlm_sdm;
    if (with_sdm) {
        NVSM_CHECK(with_qlm) << "--qlm_sdm needs --qlm.";
        NVSM_CHECK(!with_prf) << "--qlm_sdm and --qlm_prf are mutually exclusive: the lexical run is either the dependence model's or the expanded query's.";
        NVSM_CHECK(!with_cv) << "--qlm_sdm is not offered with --ensemble_qrel: the cross-validated fusion takes the query-likelihood run.";
        float w[3];
        size_t n = 0;
        std::istringstream in(FLAGS_sdm_weights);
        bool good = !FLAGS_sdm_weights.empty() && FLAGS_sdm_weights.back() != ',';
        for (std::string item; good && std::getline(in, item, ',');) {
            char* end = nullptr;
            const double v = std::strtod(item.c_str(), &end);
            good = !item.empty() && *end == '\0' && v >= 0.0 && v <= 3.0e38 && n < 3;
            if (good) w[n++] = static_cast<float>(v);
        }
        if (!good || n != 3 || (w[0] == 0.f && w[1] == 0.f && w[2] == 0.f))
            NVSM_LOG(FATAL) << "--sdm_weights: '" << FLAGS_sdm_weights << "' is not three weights t,o,u that are not negative and not all zero.";
        NVSM_CHECK(FLAGS_sdm_window >= 2 && FLAGS_sdm_window <= NVSM_SDM_MAX_WINDOW) << "--sdm_window must be in [2, " << NVSM_SDM_MAX_WINDOW << "].";
        sdm.w_term = w[0]; sdm.w_ordered = w[1]; sdm.w_unordered = w[2];
        sdm.window = static_cast<int32_t>(FLAGS_sdm_window);
    } else {
        NVSM_CHECK(FLAGS_sdm_weights == "0.85,0.10,0.05" && FLAGS_sdm_window == 8) << "--sdm_weights and --sdm_window need --qlm_sdm.";
    }
    if (with_ensemble) {
        char* end = nullptr;
        const double a = std::strtod(FLAGS_ensemble_alpha.c_str(), &end);
        if (*end != '\0' || !(a >= 0.0 && a <= 1.0)) NVSM_LOG(FATAL) << "--ensemble_alpha: '" << FLAGS_ensemble_alpha << "' is no weight in [0, 1].";
        ens.alpha = static_cast<float>(a);
    }
    if (FLAGS_score_normalizer == "standardize") ens.normalizer = NVSM_NORM_STANDARDIZE;
    else if (FLAGS_score_normalizer == "minmax") ens.normalizer = NVSM_NORM_MINMAX;
    else if (FLAGS_score_normalizer == "none") ens.normalizer = NVSM_NORM_NONE;
    else NVSM_LOG(FATAL) << "--score_normalizer: '" << FLAGS_score_normalizer << "' is none of standardize, minmax, none.";

    // ---- --rerank / --tfidf_run_out (py/query.py:186-205, over the model's vocabulary)
    const bool with_rerank = !FLAGS_rerank.empty(), with_tfidf_run = !FLAGS_tfidf_run_out.empty();
    nvsm_tfidf_options tfidf;
    nvsm_tfidf_options_default(&tfidf);
    nvsm_lexical_options rerank_lex;
    nvsm_lexical_options_default(&rerank_lex);
    nvsm_rerank_options rerank;
    nvsm_rerank_options_default(&rerank);
    rerank.tfidf = &tfidf; rerank.lexical = &rerank_lex;
    if (with_rerank) {
        NVSM_CHECK(!with_fusion) << "--rerank and --ensemble_alpha / --ensemble_qrel are mutually exclusive: <run_out> holds either the re-ranked or the fused lists.";
        if (FLAGS_rerank == "tfidf") { rerank.first_stage = NVSM_STAGE_TFIDF; tfidf.idf = NVSM_IDF_ROBERTSON; }
        else if (FLAGS_rerank == "okapi") { rerank.first_stage = NVSM_STAGE_TFIDF; tfidf.idf = NVSM_IDF_OKAPI; }
        else if (FLAGS_rerank == "jm") { rerank.first_stage = NVSM_STAGE_LEXICAL; rerank_lex.method = NVSM_LEX_JM; }
        else if (FLAGS_rerank == "dirichlet") { rerank.first_stage = NVSM_STAGE_LEXICAL; rerank_lex.method = NVSM_LEX_DIRICHLET; }
        else NVSM_LOG(FATAL) << "--rerank: '" << FLAGS_rerank << "' is none of tfidf, okapi, jm, dirichlet.";
        NVSM_CHECK(FLAGS_rerank_depth >= 1 && FLAGS_rerank_depth <= NVSM_RERANK_MAX_DEPTH) << "--rerank_depth must be in [1, " << NVSM_RERANK_MAX_DEPTH << "].";
    } else {
        NVSM_CHECK(FLAGS_rerank_depth == 1000) << "--rerank_depth needs --rerank.";
    }
    const bool with_collection = with_qlm || with_rerank || with_tfidf_run;      // the token arena goes to the device
    // ---- --lexical_index: the inverted index of that arena
    nvsm_index_options index_opt;
    nvsm_index_options_default(&index_opt);
    const bool with_index = !FLAGS_lexical_index.empty();
    if (with_index) {
        NVSM_CHECK(with_qlm || with_rerank) << "--lexical_index needs --qlm or --rerank.";
        if (FLAGS_lexical_index == "auto") index_opt.use = NVSM_INDEX_AUTO;
        else if (FLAGS_lexical_index == "always") index_opt.use = NVSM_INDEX_ALWAYS;
        else if (FLAGS_lexical_index == "never") index_opt.use = NVSM_INDEX_NEVER;
        else NVSM_LOG(FATAL) << "--lexical_index: '" << FLAGS_lexical_index << "' is none of auto, always, never.";
    }
    if (FLAGS_lexical_positions) {      // the positional layer of that index
        NVSM_CHECK(with_index) << "--lexical_positions needs --lexical_index.";
        NVSM_CHECK(with_sdm) << "--lexical_positions needs --qlm_sdm: only the dependence model reads positions.";
    }

    // ---- --top_k (py/query.py:118-139)
    int64_t top_k = 1000;
    bool top_k_all = false;
    std::unique_ptr<Qrels> candidate_qrels;
    if (FLAGS_top_k == "all") {
        top_k_all = true;
    } else if (!FLAGS_top_k.empty() && FLAGS_top_k.find_first_not_of("0123456789") == std::string::npos) {
        top_k = std::atoll(FLAGS_top_k.c_str());
        NVSM_CHECK(top_k >= 1) << "--top_k must be at least 1.";
    } else if (!FLAGS_top_k.empty()) {
        const std::vector<std::string> paths = split_blanks(FLAGS_top_k);
        for (const std::string& p : paths)
            if (!exists(p)) NVSM_LOG(FATAL) << "--top_k: '" << FLAGS_top_k << "' is neither a number, nor 'all', nor existing qrel files (" << p << ").";
        candidate_qrels.reset(new Qrels(read_qrels(paths)));
    }
    NVSM_CHECK(!(with_qlm && candidate_qrels)) << "--qlm ranks every document: with it --top_k is a number or 'all', not qrel files.";
    NVSM_CHECK(!((with_rerank || with_tfidf_run) && candidate_qrels))
        << "--rerank and --tfidf_run_out take their candidates from the collection: with them --top_k is a number or 'all', not qrel files.";
    std::unique_ptr<Qrels> qrels;
    if (!FLAGS_qrels.empty()) qrels.reset(new Qrels(read_qrels(split_blanks(FLAGS_qrels))));
    if (with_cv) qrels.reset(new Qrels(read_qrels(split_blanks(FLAGS_ensemble_qrel))));

    // ---- the index
    std::unique_ptr<IndexInterface> index;
    if (is_directory(FLAGS_index)) {
        if (!IndriDiskIndex::looks_like_repository(FLAGS_index)) NVSM_LOG(FATAL) << "Unable to open Indri parameters: " << FLAGS_index << " holds no manifest / index.";
        if (!FLAGS_stopwords.empty()) NVSM_LOG(WARNING) << "--stopwords is not used with an Indri repository (its stop list was applied when it was built).";
        index.reset(IndriDiskIndex::open(FLAGS_index));
    } else {
        NVSM_CHECK(is_file(FLAGS_index)) << "cannot read collection " << FLAGS_index;
        NVSM_LOG(INFO) << "Indexing " << FLAGS_index << ".";
        index.reset(TrectextIndex::from_file(FLAGS_index, FLAGS_stopwords));
    }

    // ---- the model (py/query.py:144-169, py/nvsm/base.py:165-240)
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
    const Hdf5Array &W = arrays[0], &E = arrays[1], &T = arrays[2], &b = arrays[3];
    const int64_t num_words = static_cast<int64_t>(W.dim0), dw = static_cast<int64_t>(W.dim1);
    const int64_t num_entities = static_cast<int64_t>(E.dim0), de = static_cast<int64_t>(E.dim1);
    if (num_words < 1 || num_entities < 1 || dw < 1 || de < 1 || dw > 2147483647 || de > 2147483647) NVSM_LOG(FATAL) << model_path << " holds an empty table";
    if (static_cast<int64_t>(T.dim0) != dw || static_cast<int64_t>(T.dim1) != de)
        NVSM_LOG(FATAL) << model_path << ": the transform is " << T.dim0 << " x " << T.dim1 << ", expected " << dw << " x " << de;
    if (b.dim0 * b.dim1 != static_cast<unsigned long long>(de)) NVSM_LOG(FATAL) << model_path << ": the bias holds " << b.dim0 * b.dim1 << " values, expected " << de;
    const ModelMappings maps = build_mappings(meta, num_words, num_entities);
    NVSM_LOG(INFO) << "<NVSM with " << num_words << " words (" << dw << "-dimensional) and " << num_entities << " entities (" << de
                   << "-dimensional), epoch " << where.epoch << ">";
    // docno -> model document id, of the documents the model holds (judged docnos the index or the model lacks find nothing here)
    std::unordered_map<std::string, int64_t> model_doc_of_docno;
    for (int64_t d = 0; d < num_entities; ++d)
        if (maps.index_object_of[static_cast<size_t>(d)] >= 0) model_doc_of_docno.emplace(index->docno(maps.index_object_of[static_cast<size_t>(d)]), d);

    if (nvsm_device_count() < 1) NVSM_LOG(FATAL) << "no HIP device visible: cuNVSMQuery has no CPU path.";
    nvsm_config cfg;
    nvsm_config_default(&cfg);      // a handle for ranking only: plain SGD (no optimiser state), a token batch capacity
    cfg.num_words = num_words; cfg.num_entities = num_entities;
    cfg.word_repr_size = static_cast<int32_t>(dw); cfg.entity_repr_size = static_cast<int32_t>(de);
    cfg.window_size = 1; cfg.num_random_entities = 1; cfg.max_batch_size = 8;
    cfg.update_method = NVSM_SGD; cfg.adam_mode = NVSM_ADAM_NONE; cfg.nonlinearity = NVSM_TANH; cfg.batch_normalization = 0;
    cfg.device = static_cast<int32_t>(FLAGS_device);
    nvsm_model* model = nullptr;
    NVSM_CALL(nvsm_create(&cfg, &model));
    for (int i = 0; i < 4; ++i)
        NVSM_CALL(nvsm_set_param(model, kNames[i], arrays[static_cast<size_t>(i)].data.data(), static_cast<int64_t>(arrays[static_cast<size_t>(i)].data.size())));

    if (with_collection) {      // the collection as the trainer would upload it: model term ids, documents in model id order
        NVSM_LOG(INFO) << "Uploading the collection for the lexical models.";
        std::vector<std::pair<size_t, DOCID_T>> documents;
        for (int64_t d = 0; d < num_entities; ++d)
            if (maps.index_object_of[static_cast<size_t>(d)] >= 0)
                documents.emplace_back(static_cast<size_t>(d), static_cast<DOCID_T>(maps.index_object_of[static_cast<size_t>(d)]));
        TokenArena arena;
        // (the model holds the out-of-vocabulary token exactly when the meta file maps index term 0)
        build_token_arena(index.get(), model_term_table(maps.model_term_of), maps.model_term_of.count(0) != 0, documents,
                          static_cast<size_t>(num_entities), [](size_t, DOCID_T, size_t) { return true; }, &arena);
        const std::vector<int64_t> offsets(arena.first_token.begin(), arena.first_token.end());
        nvsm_corpus corpus{};
        corpus.tokens = arena.tokens.data(); corpus.doc_offsets = offsets.data();
        corpus.num_tokens = static_cast<int64_t>(arena.tokens.size()); corpus.num_documents = num_entities;
        NVSM_CALL(nvsm_corpus_upload(model, &corpus));
        NVSM_LOG(INFO) << "<collection of " << corpus.num_documents << " documents and " << corpus.num_tokens << " in-vocabulary tokens>";
        if (with_index) {
            nvsm_index_info info;
            NVSM_CALL(nvsm_corpus_index(model, &index_opt, &info));
            NVSM_LOG(INFO) << "<inverted index of " << info.num_postings << " postings, " << info.bytes << " bytes, longest list " << info.max_df << ">";
            if (FLAGS_lexical_positions) {
                nvsm_positions_info layer;
                NVSM_CALL(nvsm_corpus_index_positions(model, &layer));
                NVSM_LOG(INFO) << "<positional layer of " << layer.num_positions << " positions, " << layer.bytes << " bytes>";
            }
        }
    }

    nvsm_rank_options opt;
    nvsm_rank_options_default(&opt);
    opt.bias_coefficient = 0.f;                                           // (see --bias_coefficient)
    opt.activation = FLAGS_linear ? static_cast<int32_t>(NVSM_ACT_IDENTITY) : static_cast<int32_t>(NVSM_TANH);
    opt.similarity = NVSM_SIM_COSINE;
    const std::vector<std::string> names = metric_names(cutoffs);
    const size_t width = names.size();

    for (const std::string& topic_path : topic_paths) {
        const std::string run_out_path = run_out + "-" + basename_of(topic_path);
        if (exists(run_out_path)) {
            NVSM_LOG(WARNING) << "Run for topics " << topic_path << " already exists (" << run_out_path << "); skipping.";
            continue;
        }
        std::vector<Topic> topics;
        {
            std::ifstream f(topic_path);
            topics = parse_topics(f, topic_path);
        }
        if (FLAGS_num_queries > 0 && topics.size() > static_cast<size_t>(FLAGS_num_queries)) topics.resize(static_cast<size_t>(FLAGS_num_queries));

        // ---- the topics that are ranked, in file order
        std::vector<std::string> ranked;                                   // topic ids
        std::vector<int64_t> word_ids, word_off = {0}, cand, cand_off = {0}, judged_ids, judged_off = {0};
        std::vector<float> word_weights;
        std::vector<int32_t> judged_grades;
        std::vector<int64_t> terms;
        int64_t most_candidates = 0;
        for (const Topic& topic : topics) {
            if (!query_terms(index.get(), maps, topic.text, FLAGS_strict, &terms)) {
                NVSM_LOG(WARNING) << "Skipping topic " << topic.id << ": " << (terms.empty() ? "no term of it is in the model's vocabulary." : "a term is out of vocabulary (--strict).");
                continue;
            }
            if (candidate_qrels) {
                const auto hit = candidate_qrels->find(topic.id);
                if (hit == candidate_qrels->end() || hit->second.empty()) {
                    NVSM_LOG(WARNING) << "Skipping topic " << topic.id << " as there are no judged documents.";
                    continue;
                }
                std::set<int64_t> docs;
                for (const auto& j : hit->second) {
                    const auto d = model_doc_of_docno.find(j.first);
                    if (d != model_doc_of_docno.end()) docs.insert(d->second);
                }
                cand.insert(cand.end(), docs.begin(), docs.end());
                cand_off.push_back(static_cast<int64_t>(cand.size()));
                most_candidates = std::max<int64_t>(most_candidates, static_cast<int64_t>(hit->second.size()));
            }
            ranked.push_back(topic.id);
            word_ids.insert(word_ids.end(), terms.begin(), terms.end());
            word_off.push_back(static_cast<int64_t>(word_ids.size()));
            if (FLAGS_self_information) {
                const std::vector<float> w = self_information(maps, terms);
                word_weights.insert(word_weights.end(), w.begin(), w.end());
            }
            if (qrels) {
                const auto hit = qrels->find(topic.id);
                if (hit != qrels->end())
                    for (const auto& j : hit->second) {
                        const auto d = model_doc_of_docno.find(j.first);
                        judged_ids.push_back(d == model_doc_of_docno.end() ? -1 : d->second);
                        judged_grades.push_back(j.second);
                    }
            }
            judged_off.push_back(static_cast<int64_t>(judged_ids.size()));
        }
        const int64_t Q = static_cast<int64_t>(ranked.size());
        // results_requested: --top_k clipped to the model's documents (py/nvsm/base.py:379-381); with qrel candidates the number of
        // judged documents of the topic — one call ranks every topic, so it asks for the largest and counts[] cuts each topic's list
        int64_t k = top_k_all ? num_entities : std::min(top_k, num_entities);
        if (candidate_qrels) k = std::max<int64_t>(1, std::min(most_candidates, num_entities));
        if (with_rerank) {      // the depth clipped to the collection, as --top_k is; a topic has no more results than candidates
            rerank.depth = static_cast<int32_t>(std::min<int64_t>(FLAGS_rerank_depth, num_entities));
            k = std::min<int64_t>(k, rerank.depth);
        }
        NVSM_CHECK(k <= 2147483647) << "--top_k is too large.";
        opt.top_k = static_cast<int32_t>(k);
        opt.candidates = candidate_qrels && !cand.empty() ? cand.data() : nullptr;
        opt.candidate_offsets = candidate_qrels ? cand_off.data() : nullptr;
        nvsm_queries queries;
        queries.word_ids = word_ids.data(); queries.word_weights = FLAGS_self_information ? word_weights.data() : nullptr;
        queries.offsets = word_off.data(); queries.num_queries = Q;
        const int64_t run_width = with_fusion ? 2 * k : k;               // entries per topic of <run_out>: the fused list is a union
        std::vector<int64_t> doc_ids(static_cast<size_t>(Q * run_width) + 1), counts(static_cast<size_t>(Q) + 1);
        std::vector<float> scores(static_cast<size_t>(Q * run_width) + 1);
        std::vector<double> metrics(static_cast<size_t>(Q) * width + 1);
        // "<topic> Q0 <docno> <rank from 1> <score> cuNVSM"; %.9g round-trips a float32
        auto write_run = [&](const std::string& path, const std::vector<int64_t>& ids, const std::vector<float>& sc, const std::vector<int64_t>& n,
                             int64_t per_topic) {
            std::ofstream run(path);
            NVSM_CHECK(run.good()) << "cannot write " << path;
            char score[32];
            for (int64_t q = 0; q < Q; ++q)
                for (int64_t r = 0; r < n[static_cast<size_t>(q)]; ++r) {
                    const size_t at = static_cast<size_t>(q * per_topic + r);
                    std::snprintf(score, sizeof(score), "%.9g", static_cast<double>(sc[at]));
                    run << ranked[static_cast<size_t>(q)] << " Q0 " << index->docno(maps.index_object_of[static_cast<size_t>(ids[at])]) << " " << r + 1
                        << " " << score << " cuNVSM\n";
                }
            run.close();
            NVSM_CHECK(run.good()) << "cannot write " << path;
            NVSM_LOG(INFO) << "Run outputted to " << path << ".";
        };
        lex.top_k = static_cast<int32_t>(k);
        fb.fb_docs = static_cast<int32_t>(std::min<int64_t>(fb.fb_docs, num_entities));      // clipped to the collection, as --top_k is
        if (with_qlm && !FLAGS_qlm_run_out.empty()) {
            const std::string qlm_path = FLAGS_qlm_run_out + "-" + basename_of(topic_path);
            if (exists(qlm_path)) {
                NVSM_LOG(WARNING) << "Run for topics " << topic_path << " already exists (" << qlm_path << "); skipping.";
            } else {
                std::vector<int64_t> lex_ids(static_cast<size_t>(Q * k) + 1), lex_counts(static_cast<size_t>(Q) + 1);
                std::vector<float> lex_scores(static_cast<size_t>(Q * k) + 1);
                if (with_prf) NVSM_CALL(nvsm_lexical_rank_prf(model, &queries, &lex, &fb, lex_ids.data(), lex_scores.data(), lex_counts.data()));
                else if (with_sdm) NVSM_CALL(nvsm_sdm_rank(model, &queries, &lex, &sdm, lex_ids.data(), lex_scores.data(), lex_counts.data()));
                else NVSM_CALL(nvsm_lexical_rank(model, &queries, &lex, lex_ids.data(), lex_scores.data(), lex_counts.data()));
                write_run(qlm_path, lex_ids, lex_scores, lex_counts, k);
            }
        }
        if (with_tfidf_run) {
            const std::string tfidf_path = FLAGS_tfidf_run_out + "-" + basename_of(topic_path);
            if (exists(tfidf_path)) {
                NVSM_LOG(WARNING) << "Run for topics " << topic_path << " already exists (" << tfidf_path << "); skipping.";
            } else {
                const int64_t kt = with_rerank ? rerank.depth : k;      // with --rerank the run is the first stage's: its candidates
                std::vector<int64_t> tf_ids(static_cast<size_t>(Q * kt) + 1), tf_counts(static_cast<size_t>(Q) + 1);
                std::vector<float> tf_scores(static_cast<size_t>(Q * kt) + 1);
                nvsm_tfidf_options own = tfidf;
                own.top_k = static_cast<int32_t>(kt);
                nvsm_queries plain = queries;      // a plain query string: --self_information shapes the model's query only
                plain.word_weights = nullptr;
                NVSM_CALL(nvsm_tfidf_rank(model, &plain, &own, tf_ids.data(), tf_scores.data(), tf_counts.data()));
                write_run(tfidf_path, tf_ids, tf_scores, tf_counts, kt);
            }
        }
        if (with_rerank) {      // first stage, hand-over, the model's ranking of the candidates and, with --qrels, its metrics in ONE call
            nvsm_judgments judgments{};
            judgments.doc_ids = judged_ids.data(); judgments.grades = judged_grades.data(); judgments.offsets = judged_off.data();
            judgments.cutoffs = cutoffs.data(); judgments.num_cutoffs = static_cast<int32_t>(cutoffs.size());
            NVSM_CALL(nvsm_rerank(model, &queries, &opt, &rerank, qrels ? &judgments : nullptr, qrels ? metrics.data() : nullptr, doc_ids.data(),
                                  scores.data(), counts.data()));
        } else if (with_cv) {      // both rankings once, the sweep of the grid, the choice per fold and the fused lists in ONE call
            nvsm_judgments judgments{};
            judgments.doc_ids = judged_ids.data(); judgments.grades = judged_grades.data(); judgments.offsets = judged_off.data();
            judgments.cutoffs = cutoffs.data(); judgments.num_cutoffs = static_cast<int32_t>(cutoffs.size());
            nvsm_sweep_options sweep;
            nvsm_sweep_options_default(&sweep);
            sweep.alphas = cv_alphas.data(); sweep.num_alphas = static_cast<int32_t>(cv_alphas.size());
            sweep.normalizer = ens.normalizer; sweep.depth = cv_depth;
            const std::vector<int32_t> fold_of = ensemble_folds(Q, FLAGS_num_folds, static_cast<uint64_t>(FLAGS_ensemble_seed));
            nvsm_cv_options cv;
            nvsm_cv_options_default(&cv);
            cv.measure = cv_measure; cv.num_folds = static_cast<int32_t>(FLAGS_num_folds); cv.fold_of = fold_of.data();
            std::vector<float> fold_alpha(static_cast<size_t>(FLAGS_num_folds));
            std::vector<double> fold_train(static_cast<size_t>(FLAGS_num_folds));
            NVSM_CALL(nvsm_rank_ensemble_cv(model, &queries, &opt, &lex, with_prf ? &fb : nullptr, &sweep, &cv, &judgments, fold_alpha.data(),
                                            fold_train.data(), doc_ids.data(), scores.data(), counts.data(), metrics.data(), nullptr));
            char line[160];
            for (int64_t f = 0; f < FLAGS_num_folds; ++f) {
                std::snprintf(line, sizeof(line), "Fold %lld: best_alpha=%.2f train %s=%.4f", static_cast<long long>(f),
                              static_cast<double>(fold_alpha[static_cast<size_t>(f)]), FLAGS_ensemble_measure.c_str(), fold_train[static_cast<size_t>(f)]);
                NVSM_LOG(INFO) << line;
            }
        } else if (with_ensemble) {      // both rankings, their fusion and, with --qrels, the fused list's metrics in ONE call
            nvsm_judgments judgments{};
            judgments.doc_ids = judged_ids.data(); judgments.grades = judged_grades.data(); judgments.offsets = judged_off.data();
            judgments.cutoffs = cutoffs.data(); judgments.num_cutoffs = static_cast<int32_t>(cutoffs.size());
            if (with_prf)
                NVSM_CALL(nvsm_rank_ensemble_prf(model, &queries, &opt, &lex, &fb, &ens, qrels ? &judgments : nullptr, qrels ? metrics.data() : nullptr,
                                                 doc_ids.data(), scores.data(), counts.data()));
            else if (with_sdm)
                NVSM_CALL(nvsm_rank_ensemble_sdm(model, &queries, &opt, &lex, &sdm, &ens, qrels ? &judgments : nullptr, qrels ? metrics.data() : nullptr,
                                                 doc_ids.data(), scores.data(), counts.data()));
            else
                NVSM_CALL(nvsm_rank_ensemble(model, &queries, &opt, &lex, &ens, qrels ? &judgments : nullptr, qrels ? metrics.data() : nullptr,
                                             doc_ids.data(), scores.data(), counts.data()));
        } else if (qrels) {      // ranking and metrics in ONE call: the metrics are computed from each round's ranked ids where they lie
            nvsm_judgments judgments{};
            judgments.doc_ids = judged_ids.data(); judgments.grades = judged_grades.data(); judgments.offsets = judged_off.data();
            judgments.cutoffs = cutoffs.data(); judgments.num_cutoffs = static_cast<int32_t>(cutoffs.size());
            NVSM_CALL(nvsm_evaluate(model, &queries, &opt, &judgments, metrics.data(), doc_ids.data(), scores.data(), counts.data()));
        } else {
            NVSM_CALL(nvsm_rank(model, &queries, &opt, doc_ids.data(), scores.data(), counts.data()));
        }

        write_run(run_out_path, doc_ids, scores, counts, run_width);

        if (qrels) {      // means over the topics that are in the run and have relevant judged documents, in trec_eval's layout
            std::vector<double> sums(width, 0.0);
            int64_t num_q = 0;
            for (int64_t q = 0; q < Q; ++q) {
                const double* row = metrics.data() + static_cast<size_t>(q) * width;
                if (counts[static_cast<size_t>(q)] < 1 || !(row[NVSM_EVAL_NUM_REL] > 0.0)) continue;
                ++num_q;
                for (size_t i = 0; i < width; ++i) {
                    sums[i] += row[i];
                    if (FLAGS_per_query) print_metric(names[i], ranked[static_cast<size_t>(q)], row[i], i < 3);
                }
            }
            std::printf("runid\tall\tcuNVSM\n");
            std::printf("topics\tall\t%s\n", basename_of(topic_path).c_str());
            std::printf("num_q\tall\t%lld\n", static_cast<long long>(num_q));
            for (size_t i = 0; i < width; ++i) print_metric(names[i], "all", i < 3 ? sums[i] : (num_q > 0 ? sums[i] / static_cast<double>(num_q) : 0.0), i < 3);
            std::fflush(stdout);
        }
    }
    nvsm_destroy(model);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return run(argc, argv);
    } catch (const FatalError&) {
        return 1;                       // the message has been logged
    } catch (const std::exception& e) {
        std::cerr << "Exception: " << e.what() << std::endl;
        return 1;
    }
}
