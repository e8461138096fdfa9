// CPU unit tests of what cuNVSMQuery --ensemble_qrel decides on the host (cunvsm_amd/host/query_lib.hpp): the folds of the ranked topics
// behind the seeded permutation, and the reading of --ensemble_measure.
//   fusion_folds_tests                       runs the cases; one "[PASS] name" or "[FAIL] name" line each, then "<n> failed"
//   fusion_folds_tests --folds n F seed      prints fold_of[0 .. n) on one line (tests/test_fusion_folds_host.py holds it against its
//                                            own restatement of the permutation)
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../cunvsm_amd/host/query_lib.hpp"

using namespace nvsm_host;

namespace {

int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("  %s:%d: %s\n", __FILE__, __LINE__, #cond); ok = false; } } while (0)

typedef std::vector<int32_t> V;

bool topic_file_order() {
    bool ok = true;
    EXPECT(ensemble_folds(7, 3, 0) == (V{0, 0, 0, 1, 1, 2, 2}));             // n / F + 1 topics in the first n % F folds
    EXPECT(ensemble_folds(5, 5, 0) == (V{0, 1, 2, 3, 4}));
    EXPECT(ensemble_folds(6, 2, 0) == (V{0, 0, 0, 1, 1, 1}));
    EXPECT(ensemble_folds(0, 3, 0).empty());
    const V f = ensemble_folds(23, 5, 0);
    int size[5] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < f.size(); ++i) { ++size[f[i]]; EXPECT(i == 0 || f[i] >= f[i - 1]); }
    EXPECT(size[0] == 5 && size[1] == 5 && size[2] == 5 && size[3] == 4 && size[4] == 4);
    return ok;
}

bool seeded_permutation_by_hand() {
    bool ok = true;
    // minstd_rand0(1) yields 16807, 282475249, 1622650073, ...: x' = 16807 x mod (2^31 - 1)
    std::minstd_rand0 rng(1);
    EXPECT(rng() == 16807u && rng() == 282475249u && rng() == 1622650073u);
    // n = 3: i = 2 takes j = 16807 % 3 = 1 -> order 0, 2, 1; i = 1 takes j = 282475249 % 2 = 1 -> unchanged.
    // Position p of the order is fold p: topic 0 -> 0, topic 2 -> 1, topic 1 -> 2
    EXPECT(ensemble_folds(3, 3, 1) == (V{0, 2, 1}));
    // n = 4, two folds: i = 3: j = 16807 % 4 = 3 (no move); i = 2: j = 282475249 % 3 = 1 -> order 0, 2, 1, 3; i = 1: j = 1622650073 % 2 = 1.
    // folds of the positions 0, 0, 1, 1: topics 0 and 2 -> 0, topics 1 and 3 -> 1
    EXPECT(ensemble_folds(4, 2, 1) == (V{0, 1, 0, 1}));
    return ok;
}

bool seeded_permutation_against_its_rule() {
    bool ok = true;
    for (const uint64_t seed : {1ull, 2ull, 7ull, 2147483646ull})
        for (const int64_t n : {1, 2, 23, 225})
            for (const int64_t F : {2, 5, 20}) {
                if (F > n) continue;
                std::vector<int64_t> order(static_cast<size_t>(n));
                for (int64_t i = 0; i < n; ++i) order[static_cast<size_t>(i)] = i;
                uint64_t x = seed;                                          // the generator written out
                for (int64_t i = n - 1; i >= 1; --i) {
                    x = x * 16807ull % 2147483647ull;
                    const int64_t j = static_cast<int64_t>(x % static_cast<uint64_t>(i + 1));
                    std::swap(order[static_cast<size_t>(i)], order[static_cast<size_t>(j)]);
                }
                V want(static_cast<size_t>(n));
                int64_t at = 0;
                for (int64_t f = 0; f < F; ++f)
                    for (int64_t c = n / F + (f < n % F ? 1 : 0); c > 0; --c) want[static_cast<size_t>(order[static_cast<size_t>(at++)])] = static_cast<int32_t>(f);
                EXPECT(ensemble_folds(n, F, seed) == want);
            }
    EXPECT(ensemble_folds(225, 20, 1) != ensemble_folds(225, 20, 0));
    EXPECT(ensemble_folds(225, 20, 1) != ensemble_folds(225, 20, 2));
    return ok;
}

bool measure_names() {
    bool ok = true;
    const std::vector<std::string> names = {"num_ret", "num_rel", "num_rel_ret", "map", "Rprec", "recip_rank", "ndcg", "P_5", "recall_5", "ndcg_cut_5"};
    int32_t column = -1, depth = -1;
    EXPECT(ensemble_measure("map", names, &column, &depth) && column == 3 && depth == 0);
    EXPECT(ensemble_measure("ndcg_cut_5", names, &column, &depth) && column == 9 && depth == 0);
    EXPECT(ensemble_measure("map_cut_1000", names, &column, &depth) && column == 3 && depth == 1000);
    EXPECT(ensemble_measure("map_cut_1", names, &column, &depth) && column == 3 && depth == 1);
    for (const char* bad : {"num_ret", "num_rel", "num_rel_ret", "bpref", "", "map_cut_", "map_cut_0", "map_cut_-3", "map_cut_1e3", "map_cut_12345678901", "P_10"})
        EXPECT(!ensemble_measure(bad, names, &column, &depth));
    return ok;
}

struct Case { const char* name; bool (*run)(); };
const Case kCases[] = {
    {"Folds.topic_file_order", topic_file_order},
    {"Folds.seeded_permutation_by_hand", seeded_permutation_by_hand},
    {"Folds.seeded_permutation_against_its_rule", seeded_permutation_against_its_rule},
    {"Measure.names_and_map_cut", measure_names},
};

}  // namespace

int main(int argc, char** argv) {
    if (argc == 5 && std::string(argv[1]) == "--folds") {
        const V f = ensemble_folds(std::atoll(argv[2]), std::atoll(argv[3]), static_cast<uint64_t>(std::atoll(argv[4])));
        for (size_t i = 0; i < f.size(); ++i) std::printf("%s%d", i ? " " : "", f[i]);
        std::printf("\n");
        return 0;
    }
    for (const Case& c : kCases) {
        if (argc > 1 && std::string(argv[1]) != c.name) continue;
        const bool ok = c.run();
        std::printf("[%s] %s\n", ok ? "PASS" : "FAIL", c.name);
        failures += ok ? 0 : 1;
    }
    std::printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
