// What cuNVSMVisualize (visualize_main.cpp) does on the host around nvsm_tsne — py/visualize.py on top of the C ABI: classification
// files, the choice of rows, and the files it writes. No device code.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <istream>
#include <map>
#include <ostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "base.hpp"

namespace nvsm_host {

// "<docno> <class>" per line, any blanks between the two columns; empty lines are skipped, a trailing '\r' is dropped, a line with
// another number of columns is a FatalError. A docno classified twice keeps its LAST class.
inline std::map<std::string, std::string> parse_classification(std::istream& in, const std::string& origin) {
    std::map<std::string, std::string> out;
    std::string line;
    for (int64_t number = 1; std::getline(in, line); ++number) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        std::istringstream columns(line);
        std::vector<std::string> c;
        for (std::string t; columns >> t;) c.push_back(t);
        if (c.empty()) continue;
        if (c.size() != 2) throw FatalError(origin + ":" + std::to_string(number) + ": expected '<docno> <class>'");
        out[c[0]] = c[1];
    }
    return out;
}

struct VisualRow {
    int64_t model_id;
    std::string docno, label;
};

// The rows of py/visualize.py: the model indices of the classified documents that the model knows, ascending; with limit > 0 the
// first `limit` of them. Without filter_unclassified the reference fails (it indexes the class list with every document): so
// does this.
inline std::vector<VisualRow> select_rows(const std::map<std::string, std::string>& classes,
                                          const std::unordered_map<std::string, int64_t>& model_doc_of_docno, bool filter_unclassified,
                                          int64_t limit) {
    if (!filter_unclassified)
        throw FatalError("without --filter_unclassified every document needs a class, which py/visualize.py does not handle either: pass --filter_unclassified");
    if (limit < 0) throw FatalError("--limit must not be negative");
    std::vector<VisualRow> rows;
    for (const auto& kv : classes) {
        const auto it = model_doc_of_docno.find(kv.first);
        if (it != model_doc_of_docno.end()) rows.push_back(VisualRow{it->second, kv.first, kv.second});
    }
    std::sort(rows.begin(), rows.end(), [](const VisualRow& a, const VisualRow& b) { return a.model_id < b.model_id; });
    if (limit > 0 && static_cast<int64_t>(rows.size()) > limit) rows.resize(static_cast<size_t>(limit));
    return rows;
}

inline std::string basename_of_path(const std::string& path) {
    const size_t cut = path.rfind('/');
    return cut == std::string::npos ? path : path.substr(cut + 1);
}

// "<root>-<basename(classification)>.tsv", root = plot_out without its extension (os.path.splitext)
inline std::string tsne_out_path(const std::string& plot_out, const std::string& classification_path) {
    const size_t slash = plot_out.rfind('/'), dot = plot_out.rfind('.');
    const bool has_ext = dot != std::string::npos && (slash == std::string::npos || dot > slash + 1) && dot != 0;
    return (has_ext ? plot_out.substr(0, dot) : plot_out) + "-" + basename_of_path(classification_path) + ".tsv";
}

// mode tsne: "docno<TAB>class<TAB>x<TAB>y", floats as %.9g (a float32 survives the round trip); Y [rows][2]
inline void write_tsne_tsv(std::ostream& out, const std::vector<VisualRow>& rows, const std::vector<float>& Y) {
    char buf[64];
    for (size_t i = 0; i < rows.size(); ++i) {
        std::snprintf(buf, sizeof(buf), "%.9g\t%.9g", static_cast<double>(Y[2 * i]), static_cast<double>(Y[2 * i + 1]));
        out << rows[i].docno << '\t' << rows[i].label << '\t' << buf << '\n';
    }
}

// rows of the table E [.][dim] for the chosen documents, each divided by its norm with l2_normalize (a zero row kept)
inline std::vector<float> gather_rows(const std::vector<float>& E, int64_t dim, const std::vector<VisualRow>& rows, bool l2_normalize) {
    std::vector<float> out(rows.size() * static_cast<size_t>(dim));
    for (size_t i = 0; i < rows.size(); ++i) {
        const float* x = &E[static_cast<size_t>(rows[i].model_id) * dim];
        double s = 0.0;
        for (int64_t t = 0; t < dim; ++t) s += static_cast<double>(x[t]) * static_cast<double>(x[t]);
        const double inv = !l2_normalize ? 1.0 : (s > 0.0 ? 1.0 / std::sqrt(s) : 0.0);
        for (int64_t t = 0; t < dim; ++t) out[i * dim + t] = static_cast<float>(static_cast<double>(x[t]) * inv);
    }
    return out;
}

// mode embedding_projector: vectors (values %.5f, tab-separated, one row a line) and metadata (header "document_id<TAB>class"),
// class by class in ascending class name, a class's documents by ascending model index — the same order in both files
inline void write_projector(std::ostream& vectors, std::ostream& meta, const std::vector<VisualRow>& rows, const std::vector<float>& X,
                            int64_t dim) {
    std::vector<size_t> order(rows.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return rows[a].label < rows[b].label; });
    meta << "document_id\tclass\n";
    char buf[64];
    for (size_t i : order) {
        for (int64_t t = 0; t < dim; ++t) {
            std::snprintf(buf, sizeof(buf), "%.5f", static_cast<double>(X[i * dim + t]));
            vectors << (t ? "\t" : "") << buf;
        }
        vectors << '\n';
        meta << rows[i].docno << '\t' << rows[i].label << '\n';
    }
}

}  // namespace nvsm_host
