// What cuNVSMCluster (cluster_main.cpp) does on the host around nvsm_kmeans: the agreement of a clustering with a labelling
// (purity, NMI, ARI — cunvsm_amd.cluster_agreement in Python) and the file it writes. No device code.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <map>
#include <ostream>
#include <string>
#include <vector>

#include "base.hpp"
#include "visualize_lib.hpp"

namespace nvsm_host {

// n_jc: members of cluster j that carry class c; clusters and classes renumbered densely in ascending order of their values
struct Contingency {
    std::vector<std::vector<double>> table;      // [clusters][classes]
    std::vector<double> a, b;                    // row sums (clusters), column sums (classes)
    double n = 0.0;
};

inline Contingency contingency(const std::vector<int32_t>& labels, const std::vector<std::string>& classes) {
    if (labels.size() != classes.size() || labels.empty()) throw FatalError("cluster agreement: labels and classes must have the same, non-zero length");
    std::map<int32_t, size_t> cluster_of;
    std::map<std::string, size_t> class_of;
    for (int32_t l : labels) cluster_of.emplace(l, 0);
    for (const std::string& c : classes) class_of.emplace(c, 0);
    size_t next = 0;
    for (auto& kv : cluster_of) kv.second = next++;
    next = 0;
    for (auto& kv : class_of) kv.second = next++;
    Contingency t;
    t.table.assign(cluster_of.size(), std::vector<double>(class_of.size(), 0.0));
    t.a.assign(cluster_of.size(), 0.0);
    t.b.assign(class_of.size(), 0.0);
    for (size_t i = 0; i < labels.size(); ++i) {
        const size_t j = cluster_of[labels[i]], c = class_of[classes[i]];
        t.table[j][c] += 1.0; t.a[j] += 1.0; t.b[c] += 1.0;
    }
    t.n = static_cast<double>(labels.size());
    return t;
}

// Σ_j max_c n_jc / n
inline double cluster_purity(const Contingency& t) {
    double s = 0.0;
    for (const auto& row : t.table) s += *std::max_element(row.begin(), row.end());
    return s / t.n;
}

// mutual information over the arithmetic mean of the two entropies, natural logarithms (sklearn's normalized_mutual_info_score)
inline double cluster_nmi(const Contingency& t) {
    if (t.a.size() == 1 && t.b.size() == 1) return 1.0;
    auto entropy = [&](const std::vector<double>& c) {
        double h = 0.0;
        for (double v : c) if (v > 0.0) h -= v / t.n * (std::log(v) - std::log(t.n));
        return h;
    };
    double mi = 0.0;
    for (size_t j = 0; j < t.a.size(); ++j)
        for (size_t c = 0; c < t.b.size(); ++c)
            if (t.table[j][c] > 0.0) mi += t.table[j][c] / t.n * std::log(t.n * t.table[j][c] / (t.a[j] * t.b[c]));
    const double eps = std::numeric_limits<double>::epsilon();
    mi = std::max(mi, 0.0);
    if (mi < eps) return 0.0;
    return mi / std::max(0.5 * (entropy(t.a) + entropy(t.b)), eps);
}

// sklearn's adjusted_rand_score, from the pair confusion matrix
inline double cluster_ari(const Contingency& t) {
    double sum_sq = 0.0, ta = 0.0, tb = 0.0;
    for (size_t j = 0; j < t.a.size(); ++j)
        for (size_t c = 0; c < t.b.size(); ++c) {
            sum_sq += t.table[j][c] * t.table[j][c];
            tb += t.table[j][c] * t.b[c];
            ta += t.table[j][c] * t.a[j];
        }
    const double n11 = sum_sq - t.n, n01 = tb - sum_sq, n10 = ta - sum_sq, n00 = t.n * t.n - n01 - n10 - sum_sq;
    if (n10 == 0.0 && n01 == 0.0) return 1.0;
    return 2.0 * (n11 * n00 - n10 * n01) / ((n11 + n10) * (n10 + n00) + (n11 + n01) * (n01 + n00));
}

// "<docno> <cluster>" per clustered document, in the order given (model order): the classification format parse_classification reads
inline void write_clusters(std::ostream& out, const std::vector<VisualRow>& rows, const std::vector<int32_t>& labels) {
    for (size_t i = 0; i < rows.size(); ++i) out << rows[i].docno << ' ' << labels[i] << '\n';
}

// per cluster, the position (into the clustered rows) of the row nearest its centre — the lowest position among equals; −1: no member
inline std::vector<int64_t> nearest_members(const std::vector<int32_t>& labels, const std::vector<float>& distances, int32_t k) {
    std::vector<int64_t> best(static_cast<size_t>(k), -1);
    for (size_t i = 0; i < labels.size(); ++i) {
        int64_t& b = best[static_cast<size_t>(labels[i])];
        if (b < 0 || distances[i] < distances[static_cast<size_t>(b)]) b = static_cast<int64_t>(i);
    }
    return best;
}

}  // namespace nvsm_host
