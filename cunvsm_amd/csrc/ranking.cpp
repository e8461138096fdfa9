// Host side of query inference and top-k document ranking (include/cunvsm_amd.h nvsm_infer / nvsm_rank; kernels: rank.hip).
// Both calls are synchronous. They first wait for the handle's four streams on the host — everything earlier steps queued
// that writes W, E, T or b, the side streams' tails included — and then run on the main stream, so the next step is ordered
// behind them. Lazily decayed tables are read through their LazyView, as the loss kernel and the word gather read them: no
// flush, no stamp moves, and training goes on from exactly the state it was in.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "model.h"

namespace cunvsm {

namespace {

struct RankProf {      // a profiler group around a few launches of the main stream; no profiler (the test hooks have none): nothing
    Profiler* p; hipStream_t s;
    RankProf(Profiler& p_, const char* name, hipStream_t s_) : p(&p_), s(s_) { p->begin(name, s); }
    RankProf(Profiler* p_, const char* name, hipStream_t s_) : p(p_), s(s_) { if (p) p->begin(name, s); }
    ~RankProf() { if (p) p->end(s); }
};

template <typename T>
void grow(DevBuf<T>& b, size_t count) { if (b.n < count) b.alloc(count); }

constexpr int64_t kInferChunk = 4096;                       // queries projected per launch group
constexpr int64_t kRankChunk = 256;                         // queries scanned together
constexpr int64_t kKeyCount = int64_t(32) << 20;            // sort keys: at most 256 MB (one query's keys may exceed it)
constexpr int64_t kSlabAlign = 4096;                        // rank.hip kSelPart

int64_t pow2_at_least(int64_t n) { int64_t p = 1; while (p < n) p <<= 1; return p; }

// ---- refusals several entry points share; every entry point runs its checks in an order of its own, which decides the message
// of a call that is wrong in two ways
void check_queries(const nvsm_queries& q) {
    if (q.num_queries < 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "num_queries is negative");
    if (!q.offsets) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: queries->offsets");
    if (q.offsets[0] != 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "queries->offsets[0] must be 0");
    for (int64_t i = 0; i < q.num_queries; ++i)
        if (q.offsets[i + 1] < q.offsets[i]) throw Error(NVSM_ERR_INVALID_ARGUMENT, "queries->offsets decrease");
    if (q.offsets[q.num_queries] > 0 && !q.word_ids) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: queries->word_ids");
}
void check_similarity(int s) { if (s != NVSM_SIM_COSINE && s != NVSM_SIM_DOT) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown similarity"); }
void check_activation(int a) {
    if (a != NVSM_ACT_MODEL && a != NVSM_ACT_IDENTITY && a != NVSM_TANH && a != NVSM_HARD_TANH) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown activation");
}
void check_top_k(int64_t k, int64_t rows, const char* refusal) { if (k < 1 || k > rows) throw Error(NVSM_ERR_INVALID_ARGUMENT, refusal); }
void check_row_count(int64_t rows, const char* refusal) { if (rows >= (int64_t(1) << 31)) throw Error(NVSM_ERR_UNSUPPORTED, refusal); }

// NVSM_INDEX_AUTO's rule for one round (DESIGN.md §22 "AUTO"): the postings fill costs about one binary search per (posting of a
// query's distinct terms, entry of that query) — `work` — and the scan costs one workgroup visit per document whatever the queries
// are: in the measurements its time went with D_c (x 20 for x 20 documents and x 5 tokens), so N dropped out of the rule. The
// slab's -inf fill, selection and sort are the same on both sides. The constants — how many searches one scanned document is worth,
// the TF-IDF scan being the cheaper one (no log per pair) — are fitted to the cells of tools/bench_index.py
// (profiles/index_bench.jsonl): below them the postings won every measured cell, above them the first cell they lost.
constexpr double kIndexAutoSearchesPerDocument = 200.0, kIndexAutoSearchesPerDocumentTfidf = 100.0;
bool index_auto_takes_postings(double work, int64_t num_documents, bool tfidf) {
    return work <= (tfidf ? kIndexAutoSearchesPerDocumentTfidf : kIndexAutoSearchesPerDocument) * static_cast<double>(num_documents);
}

// NVSM_INDEX_AUTO's rule for one SDM round over positional postings (DESIGN.md §26 "AUTO"): `work`, the entries the postings form
// searches and merges, against the tokens the scan reads (both of its passes walk the whole arena whatever the queries are). The
// constant comes from the cells of tools/bench_sdm_index.py (profiles/sdm_index_bench_fit.jsonl): the postings won every measured
// cell, up to 79.8 entries per token (256 queries of five words on 2·10⁶ documents), so no losing cell bounds it from above; it
// stands at the edge of what was measured, and a round beyond it — queries far longer than five words — keeps the scan.
constexpr double kSdmAutoEntriesPerToken = 80.0;
bool sdm_auto_takes_postings(double work, int64_t num_tokens) { return work <= kSdmAutoEntriesPerToken * static_cast<double>(num_tokens); }

}  // namespace

// ---- the layout of a round (DESIGN.md §9 "Dispatch by Q and k"): host arithmetic only -------------------------------------------
RankLayout rank_layout(int64_t rows, int64_t k, int64_t queries, int64_t score_floats, int64_t slab_cap) {
    RankLayout l{};
    for (l.qn = std::min(kRankChunk, queries);; l.qn = (l.qn + 1) / 2) {
        l.S = std::min(rows, std::max(kSlabAlign, score_floats / l.qn / kSlabAlign * kSlabAlign));
        if (slab_cap > 0) l.S = std::min(l.S, slab_cap);
        const int64_t last = rows % l.S;                    // every slab gives its min(k, slab size) best
        l.n_keys = rows / l.S * std::min(k, l.S) + std::min(k, last);
        l.npad = pow2_at_least(l.n_keys);
        if (l.qn * l.npad <= kKeyCount || l.qn == 1) break;
    }
    l.ld = (l.S + 3) / 4 * 4;                               // rows of the slab start 16-byte aligned (rank.hip rank_keys4)
    return l;
}

RankLayout rank_layout_candidates(const int64_t* offsets, int64_t queries) {
    RankLayout l{};
    for (l.qn = std::min(kInferChunk, queries);; l.qn = (l.qn + 1) / 2) {
        int64_t most = 1;                                   // the longest list of the queries that remain
        for (int64_t i = 0; i < l.qn; ++i) most = std::max(most, offsets[i + 1] - offsets[i]);
        l.npad = pow2_at_least(most);
        if (l.qn * l.npad <= kKeyCount || l.qn == 1) break;
    }
    return l;
}

void Model::rank_check(const nvsm_queries& q, const nvsm_rank_options& opt) {
    check_queries(q);
    if (q.word_weights) {
        for (int64_t i = 0; i < q.num_queries; ++i) {
            double sum = 0.0;
            for (int64_t j = q.offsets[i]; j < q.offsets[i + 1]; ++j) sum += q.word_weights[j];
            if (q.offsets[i + 1] > q.offsets[i] && !(std::fabs(sum) > 0.0))
                throw Error(NVSM_ERR_INVALID_ARGUMENT, "the word weights of a query sum to zero (np.average: weights sum to zero)");
        }
    }
    check_activation(opt.activation);
    if (!std::isfinite(opt.bias_coefficient)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "bias_coefficient is not finite");
}

void Model::rank_join() {
    NVSM_HIP_CHECK(hipSetDevice(cfg_.device));
    settle_words_stamp();      // (what the next step's prologue would do: the stamps of the last words update)
    synchronize();             // reports what earlier kernels have flagged, as every wait of the handle does
}

void Model::rank_project(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t q0, int64_t qn) {
    const int dw = cfg_.word_repr_size, de = cfg_.entity_repr_size;
    RankScratch& r = rank_;
    const int64_t w0 = q.offsets[q0], nw = q.offsets[q0 + qn] - w0;
    std::vector<int64_t> off(static_cast<size_t>(qn) + 1);
    for (int64_t i = 0; i <= qn; ++i) off[static_cast<size_t>(i)] = q.offsets[q0 + i] - w0;
    grow(r.offsets, static_cast<size_t>(kInferChunk) + 1);
    grow(r.ids, static_cast<size_t>(std::max<int64_t>(nw, 1)));
    grow(r.phrase, static_cast<size_t>(kInferChunk) * dw);
    grow(r.proj, static_cast<size_t>(kInferChunk) * de);
    // (the main stream is idle here: rank_join, and every chunk, end with a wait)
    NVSM_HIP_CHECK(hipMemcpy(r.offsets.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nw > 0) NVSM_HIP_CHECK(hipMemcpy(r.ids.p, q.word_ids + w0, static_cast<size_t>(nw) * sizeof(int64_t), hipMemcpyHostToDevice));
    const float* wts = nullptr;
    if (q.word_weights) {
        grow(r.wts, static_cast<size_t>(std::max<int64_t>(nw, 1)));
        if (nw > 0) NVSM_HIP_CHECK(hipMemcpy(r.wts.p, q.word_weights + w0, static_cast<size_t>(nw) * sizeof(float), hipMemcpyHostToDevice));
        wts = r.wts.p;
    }
    RankProf scope(prof, "rank_query", stream_);
    launch_rank_query_mean(words_.P.p, dw, cfg_.num_words, r.ids.p, wts, r.offsets.p, qn, r.phrase.p, lazy_view(words_), err_host_, stream_);
    // T·x on the exact-fp32 MFMA kernels, without the bias (it enters with its coefficient) and without batch-norm statistics
    launch_gemm(0, 0, r.phrase.p, T_.p, r.proj.p, static_cast<int>(qn), de, dw, dw, de, de, 1.f, nullptr, 1, 0, stream_);
    const int act = opt.activation == NVSM_ACT_MODEL ? cfg_.nonlinearity : opt.activation;
    launch_rank_bias_act(r.proj.p, b_.p, opt.bias_coefficient, act, qn, de, stream_);
}

void Model::infer(const nvsm_queries& q, const nvsm_rank_options& opt, float* out) {
    rank_check(q, opt);
    rank_join();
    const int de = cfg_.entity_repr_size;
    for (int64_t q0 = 0; q0 < q.num_queries; q0 += kInferChunk) {
        const int64_t qn = std::min(kInferChunk, q.num_queries - q0);
        rank_project(q, opt, q0, qn);
        NVSM_HIP_CHECK(hipMemcpyAsync(out + q0 * de, rank_.proj.p, static_cast<size_t>(qn) * de * sizeof(float), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    }
    prof.note("rank_infer");
    raise_device_error();
}

// ---- one round of rank / evaluate, lexical_rank and neighbors behind its layout: round_grow; round_slabs with the caller's "fill this
// slab of r.scores" step; round_sort with the caller's write kernel; round_results ---------------------------------------------------
void Model::round_grow(const RankLayout& l, int k) {
    RankScratch& r = rank_;
    grow(r.keys, static_cast<size_t>(l.qn * l.npad));
    grow(r.out_ids, static_cast<size_t>(l.qn) * k);
    grow(r.out_scores, static_cast<size_t>(l.qn) * k);
    grow(r.out_counts, static_cast<size_t>(kInferChunk));
}

// every slab of `rows`: fill(d0, rows of the slab) writes its scores [qn][ld], the selection adds each query's min(k, slab) best keys
template <typename Fill>
void Model::round_slabs(const RankLayout& l, int64_t rows, int k, Fill fill) {
    RankScratch& r = rank_;
    const int qn = static_cast<int>(l.qn);
    grow(r.scores, static_cast<size_t>(l.qn * l.ld));
    grow(r.sel_ws, rank_select_ws_bytes(qn, static_cast<int>(l.S)));
    int64_t key_off = 0;
    for (int64_t d0 = 0; d0 < rows; d0 += l.S) {
        const int Ss = static_cast<int>(std::min(l.S, rows - d0));
        fill(d0, Ss);
        {
            RankProf scope(prof, "rank_select", stream_);
            const bool radix = launch_rank_select(r.scores.p, l.ld, Ss, d0, qn, k, r.sel_ws.p, r.keys.p, l.npad, key_off, stream_);
            prof.note(radix ? "rank_select_radix" : "rank_select_all");
        }
        key_off += std::min<int64_t>(k, Ss);
    }
}

// the keys behind the slabs' (n_keys 0, candidate lists: the scan wrote and padded them) filled up to npad, the sort, and the caller's
// write kernel inside the sort's profiler group
template <typename Write>
void Model::round_sort(const RankLayout& l, Write write) {
    RankScratch& r = rank_;
    if (l.n_keys > 0) launch_rank_fill_keys(r.keys.p, l.npad, l.n_keys, l.npad, static_cast<int>(l.qn), stream_);
    RankProf scope(prof, "rank_sort", stream_);
    const bool global_steps = launch_rank_sort(r.keys.p, l.npad, static_cast<int>(l.qn), stream_);
    prof.note(global_steps ? "rank_sort_global" : "rank_sort_lds");
    write();
}

// a round's results to the host where the caller wants them, and the wait that ends the round
void Model::round_results(int64_t q0, int64_t qn, int k, int64_t* ids, float* scores, int64_t* counts) {
    RankScratch& r = rank_;
    if (ids) NVSM_HIP_CHECK(hipMemcpyAsync(ids + q0 * k, r.out_ids.p, static_cast<size_t>(qn) * k * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
    if (scores) NVSM_HIP_CHECK(hipMemcpyAsync(scores + q0 * k, r.out_scores.p, static_cast<size_t>(qn) * k * sizeof(float), hipMemcpyDeviceToHost, stream_));
    if (counts) NVSM_HIP_CHECK(hipMemcpyAsync(counts + q0, r.out_counts.p, static_cast<size_t>(qn) * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
}

void Model::rank(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t* doc_ids, float* scores, int64_t* counts) {
    rank_rounds(q, opt, doc_ids, scores, counts, nullptr);
}

// ---- retrieval metrics (include/cunvsm_amd.h nvsm_evaluate; kernel: eval.hip) ------------------------------------
// What the host prepares once per call: every query's judged list sorted by id with the -1 entries (judged documents the model
// does not hold) dropped, and the constants of the formulas that do not depend on the ranking — R, idcg, idcg@c — in double.
struct Model::EvalPlan {
    const nvsm_judgments* request = nullptr;
    double* metrics = nullptr;                  // host [Q][width]
    int width = 0, num_cutoffs = 0;
    int cutoffs[kEvalMaxCutoffs] = {};
    std::vector<int> ids, grades;               // concatenated, per query ascending by id
    std::vector<int64_t> off;                   // [Q + 1]
    std::vector<double> consts;                 // [Q][2 + kEvalMaxCutoffs]
};

void Model::evaluate(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_judgments& j, double* metrics, int64_t* doc_ids,
                     float* scores, int64_t* counts) {
    EvalPlan plan;
    plan.request = &j;      // (looked at by rank_rounds, behind nvsm_rank's own checks)
    plan.metrics = metrics;
    rank_rounds(q, opt, doc_ids, scores, counts, &plan);
}

void Model::eval_plan(EvalPlan& p, int64_t Q) const {
    const nvsm_judgments& j = *p.request;
    const int64_t D = cfg_.num_entities;
    if (!p.metrics) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: metrics");
    if (!j.offsets) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: judgments->offsets");
    if (j.offsets[0] != 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "judgments->offsets[0] must be 0");
    for (int64_t i = 0; i < Q; ++i)
        if (j.offsets[i + 1] < j.offsets[i]) throw Error(NVSM_ERR_INVALID_ARGUMENT, "judgments->offsets decrease");
    if (j.offsets[Q] > 0 && !j.doc_ids) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: judgments->doc_ids");
    if (j.offsets[Q] > 0 && !j.grades) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: judgments->grades");
    if (j.num_cutoffs < 0 || j.num_cutoffs > NVSM_EVAL_MAX_CUTOFFS)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "judgments->num_cutoffs must be in [0, NVSM_EVAL_MAX_CUTOFFS]");
    if (j.num_cutoffs > 0 && !j.cutoffs) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: judgments->cutoffs");
    for (int c = 0; c < j.num_cutoffs; ++c) {
        if (j.cutoffs[c] < 1) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a cutoff is smaller than 1");
        if (c > 0 && j.cutoffs[c] <= j.cutoffs[c - 1]) throw Error(NVSM_ERR_INVALID_ARGUMENT, "judgments->cutoffs must ascend");
        p.cutoffs[c] = j.cutoffs[c];
    }
    p.num_cutoffs = j.num_cutoffs;
    p.width = NVSM_EVAL_FIXED + 3 * j.num_cutoffs;
    p.off.assign(static_cast<size_t>(Q) + 1, 0);
    p.consts.assign(static_cast<size_t>(Q) * (2 + kEvalMaxCutoffs), 0.0);
    std::vector<std::pair<int, int>> one;       // (id, grade) of one query
    std::vector<int> gains;
    for (int64_t i = 0; i < Q; ++i) {
        one.clear();
        gains.clear();
        int64_t R = 0;
        for (int64_t t = j.offsets[i]; t < j.offsets[i + 1]; ++t) {
            const int64_t id = j.doc_ids[t];
            const int g = j.grades[t];
            if (id < -1 || id >= D) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a judged document id is outside [-1, num_entities)");
            if (g >= 1) { ++R; gains.push_back(g); }
            if (id >= 0) one.emplace_back(static_cast<int>(id), g);
        }
        std::sort(one.begin(), one.end());
        for (size_t t = 1; t < one.size(); ++t)
            if (one[t].first == one[t - 1].first) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a document id is judged twice for one query");
        for (const auto& e : one) { p.ids.push_back(e.first); p.grades.push_back(e.second); }
        p.off[static_cast<size_t>(i) + 1] = static_cast<int64_t>(p.ids.size());
        // idcg: the grades > 0 in descending order, gain g / log2(rank + 1), summed in rank order
        std::sort(gains.begin(), gains.end(), [](int x, int y) { return x > y; });
        double* c = p.consts.data() + static_cast<size_t>(i) * (2 + kEvalMaxCutoffs);
        c[0] = static_cast<double>(R);
        double sum = 0.0;
        int next = 0;
        for (size_t t = 0; t < gains.size(); ++t) {
            while (next < p.num_cutoffs && static_cast<int64_t>(t) >= p.cutoffs[next]) c[2 + next++] = sum;
            sum += static_cast<double>(gains[t]) / std::log2(static_cast<double>(t) + 2.0);
        }
        while (next < p.num_cutoffs) c[2 + next++] = sum;
        c[1] = sum;
    }
}

// the judgments and their constants go up once per call, not per round; `width` is the length of the lists the kernel will read
EvalArgs Model::eval_upload(const EvalPlan& p, int64_t Q, int width) {
    RankScratch& r = rank_;
    grow(r.jids, std::max<size_t>(p.ids.size(), 1));
    grow(r.jgrades, std::max<size_t>(p.ids.size(), 1));
    grow(r.joff, static_cast<size_t>(Q) + 1);
    grow(r.jconst, std::max<size_t>(p.consts.size(), 1));
    grow(r.metrics, std::max<size_t>(static_cast<size_t>(Q) * p.width, 1));
    if (!p.ids.empty()) {
        NVSM_HIP_CHECK(hipMemcpy(r.jids.p, p.ids.data(), p.ids.size() * sizeof(int), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(r.jgrades.p, p.grades.data(), p.grades.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    NVSM_HIP_CHECK(hipMemcpy(r.joff.p, p.off.data(), p.off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (!p.consts.empty()) NVSM_HIP_CHECK(hipMemcpy(r.jconst.p, p.consts.data(), p.consts.size() * sizeof(double), hipMemcpyHostToDevice));
    EvalArgs ea{};
    ea.k = width;
    ea.jids = r.jids.p; ea.jgrades = r.jgrades.p; ea.joff = r.joff.p; ea.consts = r.jconst.p;
    for (int c = 0; c < kEvalMaxCutoffs; ++c) ea.cutoffs[c] = p.cutoffs[c];
    ea.num_cutoffs = p.num_cutoffs;
    ea.metrics = r.metrics.p;
    return ea;
}

void Model::rank_rounds(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t* doc_ids, float* scores, int64_t* counts, EvalPlan* ev) {
    const int64_t D = cfg_.num_entities, Q = q.num_queries;
    const int de = cfg_.entity_repr_size;
    check_similarity(opt.similarity);
    check_top_k(opt.top_k, D, "top_k must be in [1, num_entities]");
    check_row_count(D, "ranking supports fewer than 2^31 documents");
    const int k = opt.top_k;
    const int cosine = opt.similarity == NVSM_SIM_COSINE;
    // candidate lists: distinct, ascending (base.py ranks a document_set: a set)
    std::vector<int> cand;
    std::vector<int64_t> cand_off;
    if (opt.candidates || opt.candidate_offsets) {
        if (!opt.candidate_offsets) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: options->candidate_offsets");
        const int64_t* co = opt.candidate_offsets;
        if (co[0] != 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "options->candidate_offsets[0] must be 0");
        for (int64_t i = 0; i < Q; ++i)
            if (co[i + 1] < co[i]) throw Error(NVSM_ERR_INVALID_ARGUMENT, "options->candidate_offsets decrease");
        if (co[Q] > 0 && !opt.candidates) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: options->candidates");
        cand_off.assign(static_cast<size_t>(Q) + 1, 0);
        std::vector<int> one;
        for (int64_t i = 0; i < Q; ++i) {
            one.clear();
            for (int64_t j = co[i]; j < co[i + 1]; ++j) {
                const int64_t id = opt.candidates[j];
                if (id < 0 || id >= D) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a candidate document id is outside [0, num_entities)");
                one.push_back(static_cast<int>(id));
            }
            std::sort(one.begin(), one.end());
            one.erase(std::unique(one.begin(), one.end()), one.end());
            cand.insert(cand.end(), one.begin(), one.end());
            cand_off[static_cast<size_t>(i) + 1] = static_cast<int64_t>(cand.size());
        }
    }
    const bool by_candidates = !cand_off.empty();
    rank_check(q, opt);
    if (ev) eval_plan(*ev, Q);      // (host work only: refusals come before anything runs)
    rank_join();
    RankScratch& r = rank_;
    const LazyView view = lazy_view(ents_);
    EvalArgs ea{};
    if (ev) ea = eval_upload(*ev, Q, k);

    for (int64_t q0 = 0; q0 < Q;) {
        const RankLayout l = by_candidates ? rank_layout_candidates(cand_off.data() + q0, Q - q0) : rank_layout(D, k, Q - q0, score_floats());
        const int64_t qn = l.qn;
        if (by_candidates) {      // the round's lists go up, then the round that nvsm_rerank shares
            const int64_t c0 = cand_off[q0], nc = cand_off[q0 + qn] - c0;
            std::vector<int64_t> off(static_cast<size_t>(qn) + 1);
            for (int64_t i = 0; i <= qn; ++i) off[static_cast<size_t>(i)] = cand_off[q0 + i] - c0;
            grow(r.cand_off, static_cast<size_t>(kInferChunk) + 1);
            grow(r.cand, static_cast<size_t>(std::max<int64_t>(nc, 1)));
            NVSM_HIP_CHECK(hipMemcpyAsync(r.cand_off.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
            if (nc > 0) NVSM_HIP_CHECK(hipMemcpyAsync(r.cand.p, cand.data() + c0, static_cast<size_t>(nc) * sizeof(int), hipMemcpyHostToDevice, stream_));
            NVSM_HIP_CHECK(hipStreamSynchronize(stream_));      // (`off` goes out of scope)
            rank_candidates_round(q, opt, q0, l, r.cand.p, r.cand_off.p, ev ? &ea : nullptr, doc_ids, scores, counts);
            q0 += qn;
            continue;
        }
        rank_project(q, opt, q0, qn);
        grow(r.qinv, static_cast<size_t>(kInferChunk));
        round_grow(l, k);
        { RankProf scope(prof, "rank_query", stream_); launch_rank_query_norm(r.proj.p, qn, de, r.qinv.p, cosine, stream_); }
        round_slabs(l, D, k, [&](int64_t d0, int Ss) {
            RankProf scope(prof, "rank_scan", stream_);
            prof.note(rank_scan_uses_mfma(de) ? "rank_scan_mfma" : "rank_scan_plain");
            launch_rank_scan(ents_.P.p, de, d0, Ss, r.proj.p, static_cast<int>(qn), r.qinv.p, r.scores.p, l.ld, cosine, view, stream_);
        });
        round_sort(l, [&] {
            launch_rank_write(r.keys.p, l.npad, static_cast<int>(qn), k, nullptr, l.n_keys, r.out_ids.p, r.out_scores.p, r.out_counts.p, stream_);
        });
        if (ev) {      // the round's metrics from the ranked ids where they lie: one wave per query
            RankProf scope(prof, "rank_eval", stream_);
            ea.ids = r.out_ids.p; ea.counts = r.out_counts.p; ea.q0 = q0;
            launch_eval_metrics(ea, static_cast<int>(qn), stream_);
        }
        round_results(q0, qn, k, doc_ids, scores, counts);
        q0 += qn;
    }
    if (ev && Q > 0)
        NVSM_HIP_CHECK(hipMemcpy(ev->metrics, r.metrics.p, static_cast<size_t>(Q) * ev->width * sizeof(double), hipMemcpyDeviceToHost));
    blank_wordless(q, k, doc_ids, scores, counts, ev ? ev->metrics : nullptr, ev ? ev->width : 0);
    raise_device_error();
}

// a query without words retrieves nothing (the reference returns None)
void Model::blank_wordless(const nvsm_queries& q, int k, int64_t* doc_ids, float* scores, int64_t* counts, double* metrics, int width) const {
    for (int64_t i = 0; i < q.num_queries; ++i) {
        if (q.offsets[i + 1] > q.offsets[i]) continue;
        if (counts) counts[i] = 0;
        for (int j = 0; j < k; ++j) {
            if (doc_ids) doc_ids[i * k + j] = -1;
            if (scores) scores[i * k + j] = -INFINITY;
        }
        if (metrics) std::fill(metrics + i * width, metrics + (i + 1) * width, 0.0);
    }
}

// no slabs: the scan writes every list's keys, padded to npad; then the sort, the write, the metrics and the results of the round
void Model::rank_candidates_round(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t q0, const RankLayout& l, const int* cand,
                                  const int64_t* cand_off, EvalArgs* ea, int64_t* doc_ids, float* scores, int64_t* counts) {
    RankScratch& r = rank_;
    const int de = cfg_.entity_repr_size, k = opt.top_k;
    const int cosine = opt.similarity == NVSM_SIM_COSINE;
    const int64_t qn = l.qn;
    rank_project(q, opt, q0, qn);
    grow(r.qinv, static_cast<size_t>(kInferChunk));
    round_grow(l, k);
    { RankProf scope(prof, "rank_query", stream_); launch_rank_query_norm(r.proj.p, qn, de, r.qinv.p, cosine, stream_); }
    {
        RankProf scope(prof, "rank_scan", stream_);
        prof.note("rank_scan_candidates");
        launch_rank_scan_candidates(ents_.P.p, de, r.proj.p, r.qinv.p, cand, cand_off, static_cast<int>(qn), l.npad, r.keys.p, cosine,
                                    lazy_view(ents_), stream_);
    }
    round_sort(l, [&] {
        launch_rank_write(r.keys.p, l.npad, static_cast<int>(qn), k, cand_off, l.n_keys, r.out_ids.p, r.out_scores.p, r.out_counts.p, stream_);
    });
    if (ea) {      // the round's metrics from the ranked ids where they lie: one wave per query
        RankProf scope(prof, "rank_eval", stream_);
        ea->ids = r.out_ids.p; ea->counts = r.out_counts.p; ea->q0 = q0;
        launch_eval_metrics(*ea, static_cast<int>(qn), stream_);
    }
    round_results(q0, qn, k, doc_ids, scores, counts);
}

// ---- query-likelihood ranking over the resident corpus (include/cunvsm_amd.h nvsm_lexical_rank; kernels: lexical.hip) ----
// Rounds, slabs, selection and sort are nvsm_rank's; what differs is who fills the score slab (launch_lex_score from the token arena)
// and that a slab entry may be -inf — a document without any of the query's terms — which launch_lex_write leaves out and counts.
// A round takes queries while their distinct remaining terms fit kLexSlots counters.
//
// nvsm_rerank's first stage hands every round over on the device: the round's counts are on the host behind round_results, the
// offsets of its queries follow from them and go up behind those of the rounds before, and rerank_gather_kernel takes the retrieved
// ids out of the round's sorted keys. `off` is sized for the chunk up front, so what the queued copies read stays where it is.
struct Model::Handover {
    int* cand = nullptr;                  // device: every query of the chunk has room for `depth` ids
    int64_t* off_dev = nullptr;           // device [queries of the chunk + 1]; off_dev[0] = 0 is there already
    std::vector<int64_t> off;             // the same on the host
    int64_t done = 0;                     // queries handed over so far
    int nsort = 1;                        // a power of two >= depth
    void take(Model& m, const RankLayout& l, const int64_t* counts, int64_t qn) {
        for (int64_t i = 0; i < qn; ++i) off[static_cast<size_t>(done + i + 1)] = off[static_cast<size_t>(done + i)] + counts[i];
        NVSM_HIP_CHECK(hipMemcpyAsync(off_dev + done + 1, off.data() + done + 1, static_cast<size_t>(qn) * sizeof(int64_t), hipMemcpyHostToDevice, m.stream_));
        RankProf scope(m.prof, "rerank_gather", m.stream_);
        launch_rerank_gather(m.rank_.keys.p, l.npad, off_dev + done, cand, static_cast<int>(qn), nsort, m.stream_);
        done += qn;
    }
};

void Model::lexical_check(const nvsm_queries& q, const nvsm_lexical_options& lex) const {
    if (!corpus_) throw Error(NVSM_ERR_INVALID_ARGUMENT, "lexical ranking needs a corpus: call nvsm_corpus_upload first");
    if (lex.method != NVSM_LEX_JM && lex.method != NVSM_LEX_DIRICHLET) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown lexical method");
    if (!std::isfinite(lex.param)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "lexical param is not finite");
    if (lex.method == NVSM_LEX_JM && lex.param != 0.f && !(lex.param > 0.f && lex.param < 1.f))
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "lambda (lexical param, Jelinek-Mercer) must be in (0, 1), or 0 for auto");
    if (lex.method == NVSM_LEX_DIRICHLET && lex.param < 0.f)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "mu (lexical param, Dirichlet) must not be negative (0 is auto)");
    check_top_k(lex.top_k, corpus_->num_documents, "lexical top_k must be in [1, num_documents of the corpus]");
    check_row_count(corpus_->num_documents, "ranking supports fewer than 2^31 documents");
    check_queries(q);
    std::vector<int64_t> one;
    for (int64_t i = 0; i < q.num_queries; ++i) {
        if (q.offsets[i + 1] - q.offsets[i] <= kLexSlots) continue;
        one.assign(q.word_ids + q.offsets[i], q.word_ids + q.offsets[i + 1]);
        std::sort(one.begin(), one.end());
        if (std::unique(one.begin(), one.end()) - one.begin() > kLexSlots)
            throw Error(NVSM_ERR_UNSUPPORTED, "a query has more than NVSM_LEXICAL_MAX_QUERY_TERMS distinct terms");
    }
}

void Model::lexical_rank(const nvsm_queries& q, const nvsm_lexical_options& lex, int64_t* doc_ids, float* scores, int64_t* counts) {
    lexical_check(q, lex);
    rank_join();
    lexical_rounds(q, lex, nullptr, doc_ids, scores, counts);
}

// the cf table of the corpus: one histogram pass over the arena, kept with the corpus (a new upload is a new Corpus)
void Model::corpus_cf() {
    Corpus& c = *corpus_;
    if (!c.cf.empty()) return;
    const int64_t V = cfg_.num_words;
    DevBuf<unsigned long long> cf;
    cf.alloc(static_cast<size_t>(V), true);
    { RankProf scope(prof, "lex_cf", stream_); launch_lex_cf(c.tokens.p, c.num_tokens, cf.p, stream_); }
    std::vector<int64_t> host(static_cast<size_t>(V));
    NVSM_HIP_CHECK(hipMemcpyAsync(host.data(), cf.p, static_cast<size_t>(V) * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    c.cf.swap(host);
}

void Model::lexical_rounds(const nvsm_queries& q, const nvsm_lexical_options& lex, const float* weights, int64_t* doc_ids, float* scores,
                           int64_t* counts, const TfidfPlan* tfidf, Handover* hand) {
    Corpus& c = *corpus_;
    const int64_t Dc = c.num_documents, N = c.num_tokens, Q = q.num_queries, V = cfg_.num_words;
    const int k = lex.top_k;
    RankScratch& r = rank_;
    if (tfidf) {
        corpus_df();
    } else {
        corpus_cf();
    }
    if (r.lex_slot_of.n < static_cast<size_t>(V)) {
        r.lex_slot_of.alloc(static_cast<size_t>(V));
        launch_lex_fill_int(r.lex_slot_of.p, V, -1, stream_);
    }
    const double param = lex.method == NVSM_LEX_JM ? (lex.param == 0.f ? 0.5 : static_cast<double>(lex.param))
                                                   : (lex.param == 0.f ? static_cast<double>(N) / static_cast<double>(Dc) : static_cast<double>(lex.param));
    const std::vector<int64_t>& held = tfidf ? c.df : c.cf;      // a term nobody holds is dropped: df = 0 exactly where cf = 0
    bool bad_word = false;
    std::vector<int> terms, qoff, tslot;
    std::vector<double> c0, base, wt;
    std::vector<std::pair<int64_t, int>> slot_of;      // (term, slot) of the round, kept sorted by term
    // an indexed corpus: every entry's query and whether it is the first of its term there, the round's postings work
    const bool indexed = c.indexed && c.index_use != NVSM_INDEX_NEVER;
    std::vector<int> entry_query, entry_first;

    for (int64_t q0 = 0; q0 < Q;) {
        RankLayout l = rank_layout(Dc, k, Q - q0, score_floats());
        // ---- the round's queries: as many of the l.qn as their distinct remaining terms leave room for (at least one: lexical_check);
        // the slabs stay those of the layout, the scratch is sized by the queries taken
        terms.clear(); tslot.clear(); c0.clear(); base.clear(); wt.clear(); slot_of.clear(); entry_query.clear(); entry_first.clear();
        qoff.assign(1, 0);
        int64_t taken = 0;
        double postings_work = 0.0;      // Σ over the queries of (Σ df of the query's distinct terms) · (its entries): the searches of the fill
        int64_t round_max_df = 0;
        for (; taken < l.qn; ++taken) {
            const size_t terms_before = terms.size(), entries_before = tslot.size();
            bool fits = true;
            double query_df = 0.0;
            for (int64_t j = q.offsets[q0 + taken]; j < q.offsets[q0 + taken + 1]; ++j) {
                const int64_t t = q.word_ids[j];
                if (t < 0 || t >= V) { bad_word = true; continue; }      // the index contract: matches nothing, reported at the end
                if (held[static_cast<size_t>(t)] == 0) continue;
                if (weights && weights[j] == 0.f) continue;               // a weighted query: a term of weight 0 is dropped
                auto it = std::lower_bound(slot_of.begin(), slot_of.end(), std::make_pair(t, -1));
                int slot;
                if (it != slot_of.end() && it->first == t) {
                    slot = it->second;
                } else {
                    if (terms.size() == static_cast<size_t>(kLexSlots)) { fits = false; break; }
                    slot = static_cast<int>(terms.size());
                    slot_of.insert(it, std::make_pair(t, slot));
                    terms.push_back(static_cast<int>(t));
                }
                if (indexed) {
                    const bool first = std::find(tslot.begin() + static_cast<std::ptrdiff_t>(entries_before), tslot.end(), slot) == tslot.end();
                    entry_query.push_back(static_cast<int>(taken));
                    entry_first.push_back(first ? 1 : 0);
                    if (first) {
                        query_df += static_cast<double>(c.df[static_cast<size_t>(t)]);
                        round_max_df = std::max(round_max_df, c.df[static_cast<size_t>(t)]);
                    }
                }
                tslot.push_back(slot);
                if (tfidf) {    // the term's idf, once per term by the host, where the lexical scorer has c0 (base is not read)
                    const double df = static_cast<double>(c.df[static_cast<size_t>(t)]), docs = static_cast<double>(Dc);
                    c0.push_back(tfidf->idf == NVSM_IDF_OKAPI ? std::log((docs - df + 0.5) / (df + 0.5)) : std::log((docs + 1.0) / (df + 0.5)));
                    base.push_back(0.0);
                } else {
                    const double p = static_cast<double>(c.cf[static_cast<size_t>(t)]) / static_cast<double>(N);
                    c0.push_back(param * p);
                    base.push_back(std::log(param * p));
                }
                if (weights) wt.push_back(static_cast<double>(weights[j]));
            }
            if (!fits) {      // this query opens the next round: take back what it added
                for (size_t s = terms_before; s < terms.size(); ++s) {
                    auto it = std::lower_bound(slot_of.begin(), slot_of.end(), std::make_pair(static_cast<int64_t>(terms[s]), -1));
                    slot_of.erase(it);
                }
                terms.resize(terms_before); tslot.resize(entries_before); c0.resize(entries_before); base.resize(entries_before);
                if (weights) wt.resize(entries_before);
                if (indexed) { entry_query.resize(entries_before); entry_first.resize(entries_before); }
                break;
            }
            postings_work += query_df * static_cast<double>(tslot.size() - entries_before);
            qoff.push_back(static_cast<int>(tslot.size()));
        }
        const int64_t qn = l.qn = taken;
        const int nslots = static_cast<int>(terms.size());
        const size_t nent = tslot.size();
        grow(r.lex_terms, static_cast<size_t>(kLexSlots));
        grow(r.lex_qoff, static_cast<size_t>(kRankChunk) + 1);
        grow(r.lex_tslot, std::max<size_t>(nent, 1));
        grow(r.lex_c0, std::max<size_t>(nent, 1));
        grow(r.lex_base, std::max<size_t>(nent, 1));
        if (weights) grow(r.lex_weight, std::max<size_t>(nent, 1));
        // (the main stream is idle here: every round ends with a wait)
        if (nslots > 0) NVSM_HIP_CHECK(hipMemcpy(r.lex_terms.p, terms.data(), static_cast<size_t>(nslots) * sizeof(int), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(r.lex_qoff.p, qoff.data(), qoff.size() * sizeof(int), hipMemcpyHostToDevice));
        if (nent > 0) {
            NVSM_HIP_CHECK(hipMemcpy(r.lex_tslot.p, tslot.data(), nent * sizeof(int), hipMemcpyHostToDevice));
            NVSM_HIP_CHECK(hipMemcpy(r.lex_c0.p, c0.data(), nent * sizeof(double), hipMemcpyHostToDevice));
            NVSM_HIP_CHECK(hipMemcpy(r.lex_base.p, base.data(), nent * sizeof(double), hipMemcpyHostToDevice));
            if (weights) NVSM_HIP_CHECK(hipMemcpy(r.lex_weight.p, wt.data(), nent * sizeof(double), hipMemcpyHostToDevice));
        }
        round_grow(l, k);
        LexScoreArgs a{};
        a.tokens = c.tokens.p; a.doc_offsets = c.offsets.p; a.slot_of = r.lex_slot_of.p;
        a.Q = static_cast<int>(qn); a.num_slots = nslots; a.method = lex.method; a.param = param;
        a.qoff = r.lex_qoff.p; a.tslot = r.lex_tslot.p; a.c0 = r.lex_c0.p; a.base = r.lex_base.p;
        a.ld = l.ld;
        a.weight = weights ? r.lex_weight.p : nullptr;
        TfidfScoreArgs ta{};
        if (tfidf) {
            ta.tokens = a.tokens; ta.doc_offsets = a.doc_offsets; ta.slot_of = a.slot_of;
            ta.Q = a.Q; ta.num_slots = nslots; ta.k1 = tfidf->k1; ta.b = tfidf->b; ta.avgdl = tfidf->avgdl;
            ta.qoff = a.qoff; ta.tslot = a.tslot; ta.idf = a.c0; ta.weight = a.weight; ta.ld = l.ld;
        }
        // the fill of this round's slabs: the arena scan, or the postings of the round's terms. Both give the same bits, so the
        // choice — the caller's, or under NVSM_INDEX_AUTO index_auto_takes_postings' — is invisible in the results
        const bool postings = indexed && (c.index_use == NVSM_INDEX_ALWAYS || index_auto_takes_postings(postings_work, Dc, tfidf != nullptr));
        PostingsArgs pa{};
        if (postings) {
            grow(r.post_query, std::max<size_t>(nent, 1));
            grow(r.post_first, std::max<size_t>(nent, 1));
            grow(r.post_lo, static_cast<size_t>(kLexSlots));
            grow(r.post_hi, static_cast<size_t>(kLexSlots));
            if (nent > 0) {
                NVSM_HIP_CHECK(hipMemcpy(r.post_query.p, entry_query.data(), nent * sizeof(int), hipMemcpyHostToDevice));
                NVSM_HIP_CHECK(hipMemcpy(r.post_first.p, entry_first.data(), nent * sizeof(int), hipMemcpyHostToDevice));
            }
            pa.post_off = c.post_off.p; pa.post_doc = c.post_doc.p; pa.post_tf = c.post_tf.p; pa.doc_offsets = c.offsets.p;
            pa.terms = r.lex_terms.p; pa.num_slots = nslots; pa.lo = r.post_lo.p; pa.hi = r.post_hi.p;
            pa.Q = static_cast<int>(qn); pa.num_entries = static_cast<int>(nent); pa.method = lex.method; pa.param = param;
            if (tfidf) { pa.k1 = tfidf->k1; pa.b = tfidf->b; pa.avgdl = tfidf->avgdl; }
            pa.qoff = r.lex_qoff.p; pa.tslot = r.lex_tslot.p; pa.entry_query = r.post_query.p; pa.first = r.post_first.p;
            pa.c0 = r.lex_c0.p; pa.base = r.lex_base.p; pa.weight = a.weight; pa.ld = l.ld;
        }
        round_slabs(l, Dc, k, [&](int64_t d0, int Ss) {
            if (postings) {
                pa.scores = r.scores.p; pa.d0 = d0; pa.S = Ss;
                RankProf scope(prof, tfidf ? "tfidf_postings" : (weights ? "lex_postings_weighted" : "lex_postings"), stream_);
                launch_postings_fill(pa, round_max_df, tfidf != nullptr, stream_);
                return;
            }
            if (d0 == 0) launch_lex_set_slots(r.lex_slot_of.p, r.lex_terms.p, nslots, true, stream_);      // (behind round_slabs' grows)
            if (tfidf) {
                ta.scores = r.scores.p; ta.d0 = d0; ta.S = Ss;
                RankProf scope(prof, "tfidf_score", stream_);
                launch_tfidf_score(ta, stream_);
                return;
            }
            a.scores = r.scores.p; a.d0 = d0; a.S = Ss;
            RankProf scope(prof, weights ? "lex_score_weighted" : "lex_score", stream_);
            launch_lex_score(a, stream_);
        });
        if (!postings) launch_lex_set_slots(r.lex_slot_of.p, r.lex_terms.p, nslots, false, stream_);
        round_sort(l, [&] { launch_lex_write(r.keys.p, l.npad, static_cast<int>(qn), k, l.n_keys, r.out_ids.p, r.out_scores.p, r.out_counts.p, stream_); });
        round_results(q0, qn, k, doc_ids, scores, counts);
        if (hand) hand->take(*this, l, counts + q0, qn);      // (the round's sorted keys still lie in r.keys)
        q0 += qn;
    }
    raise_device_error();
    if (bad_word) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a query word id is outside [0, num_words)");
}

// ---- TF-IDF first stage and re-ranking of its candidates (include/cunvsm_amd.h nvsm_tfidf_rank / nvsm_rerank; kernels: lexical.hip;
// DESIGN.md §20) -------------------------------------------------------------------------------------------------------------------------
// nvsm_tfidf_rank is lexical_rounds with another scorer: the same rounds, slot table, slabs, selection, sort and write.
void Model::tfidf_check(const nvsm_queries& q, const nvsm_tfidf_options& opt) const {
    if (!corpus_) throw Error(NVSM_ERR_INVALID_ARGUMENT, "lexical ranking needs a corpus: call nvsm_corpus_upload first");
    if (opt.idf != NVSM_IDF_ROBERTSON && opt.idf != NVSM_IDF_OKAPI) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown idf");
    if (!std::isfinite(opt.k1) || opt.k1 < 0.f) throw Error(NVSM_ERR_INVALID_ARGUMENT, "k1 must be finite and positive, or 0 for auto");
    if (!(opt.b >= 0.f && opt.b <= 1.f)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "b must be in (0, 1], or 0 for auto");
    check_top_k(opt.top_k, corpus_->num_documents, "tfidf top_k must be in [1, num_documents of the corpus]");
    check_row_count(corpus_->num_documents, "ranking supports fewer than 2^31 documents");
    check_queries(q);
    if (q.word_weights) weights_check(q);
    std::vector<int64_t> one;
    for (int64_t i = 0; i < q.num_queries; ++i) {
        if (q.offsets[i + 1] - q.offsets[i] <= kLexSlots) continue;
        one.assign(q.word_ids + q.offsets[i], q.word_ids + q.offsets[i + 1]);
        std::sort(one.begin(), one.end());
        if (std::unique(one.begin(), one.end()) - one.begin() > kLexSlots)
            throw Error(NVSM_ERR_UNSUPPORTED, "a query has more than NVSM_LEXICAL_MAX_QUERY_TERMS distinct terms");
    }
}

Model::TfidfPlan Model::tfidf_plan(const nvsm_tfidf_options& opt) const {
    TfidfPlan p{};
    p.k1 = opt.k1 == 0.f ? 1.2 : static_cast<double>(opt.k1);
    p.b = opt.b == 0.f ? 0.75 : static_cast<double>(opt.b);
    p.avgdl = static_cast<double>(corpus_->num_tokens) / static_cast<double>(corpus_->num_documents);      // (top_k >= 1: there are documents)
    p.idf = opt.idf;
    return p;
}

// One pass over the arena, kept with the corpus as the cf table is (a new upload is a new Corpus). The bit table comes out of the score
// slab's budget: as many documents per slab as fit, at least 32.
void Model::corpus_df() {
    Corpus& c = *corpus_;
    if (!c.df.empty()) return;
    const int64_t V = cfg_.num_words, Dc = c.num_documents;
    const int64_t slab = std::max<int64_t>(1, std::min(Dc, std::max<int64_t>(1, score_floats() / V) * 32));
    DevBuf<unsigned long long> df;
    DevBuf<unsigned> bits;
    df.alloc(static_cast<size_t>(V), true);
    bits.alloc(static_cast<size_t>(V * lex_df_row_words(slab)), true);
    { RankProf scope(prof, "lex_df", stream_); launch_lex_df(c.tokens.p, c.offsets.p, Dc, slab, bits.p, df.p, stream_); }
    std::vector<int64_t> host(static_cast<size_t>(V));
    NVSM_HIP_CHECK(hipMemcpyAsync(host.data(), df.p, static_cast<size_t>(V) * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    c.df.swap(host);
}

// ---- the inverted index of the uploaded corpus (include/cunvsm_amd.h nvsm_corpus_index; kernels: index.hip) ---------
// The arena is in document order and sort_pairs is stable: sorted by token with the positions as values, every term's positions
// ascend, hence its documents. Heads — where (term, document) changes — are the postings; their scan is three launches. All the
// build's scratch is local to this function: freed before the call returns.
void Model::index_build(Corpus& c) {
    const int64_t N = c.num_tokens, Dc = c.num_documents, V = cfg_.num_words;
    if (N >= (int64_t(1) << 31)) throw Error(NVSM_ERR_UNSUPPORTED, "the inverted index supports fewer than 2^31 tokens");
    RankProf scope(prof, "index_build", stream_);
    c.post_off.alloc(static_cast<size_t>(V) + 1, true);
    std::vector<int64_t> post_off(static_cast<size_t>(V) + 1, 0), tok_off(static_cast<size_t>(V) + 1, 0);
    int64_t P = 0;
    if (N > 0) {
        int bits = 1;
        while (bits < 31 && (int64_t(1) << bits) < V) ++bits;
        DevBuf<int> term, doc, sums;
        term.alloc(static_cast<size_t>(N));
        doc.alloc(static_cast<size_t>(N));
        {
            DevBuf<char> temp;
            const size_t temp_bytes = sort_pairs_temp_bytes(N, bits);
            temp.alloc(temp_bytes, true);
            sort_pairs(temp.p, temp_bytes, nullptr, c.tokens.p, term.p, nullptr, doc.p, N, bits, nullptr, stream_);
            launch_index_docs(doc.p, N, c.offsets.p, Dc, stream_);
            NVSM_HIP_CHECK(hipStreamSynchronize(stream_));      // (the sort's workspace goes before the postings come)
        }
        const int64_t tiles = index_tiles(N);
        sums.alloc(static_cast<size_t>(tiles) + 1);
        launch_index_scan(term.p, doc.p, N, sums.p, stream_);
        int total = 0;
        NVSM_HIP_CHECK(hipMemcpyAsync(&total, sums.p + tiles, sizeof(int), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
        P = total;
        DevBuf<int> head;
        DevBuf<int64_t> tok;
        head.alloc(static_cast<size_t>(P) + 1);
        tok.alloc(static_cast<size_t>(V) + 1);
        c.post_doc.alloc(static_cast<size_t>(P));
        c.post_tf.alloc(static_cast<size_t>(P));
        launch_index_write(term.p, doc.p, N, V, sums.p, head.p, c.post_doc.p, c.post_off.p, tok.p, stream_);
        launch_index_tf(head.p, P, c.post_tf.p, stream_);
        NVSM_HIP_CHECK(hipMemcpyAsync(post_off.data(), c.post_off.p, post_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipMemcpyAsync(tok_off.data(), tok.p, tok_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    } else {
        c.post_doc.alloc(1, true);
        c.post_tf.alloc(1, true);
    }
    c.max_df = 0;
    for (int64_t t = 0; t < V; ++t) c.max_df = std::max(c.max_df, post_off[static_cast<size_t>(t) + 1] - post_off[static_cast<size_t>(t)]);
    if (c.cf.empty()) {      // what lex_cf_kernel counts: a term's sorted entries
        c.cf.resize(static_cast<size_t>(V));
        for (int64_t t = 0; t < V; ++t) c.cf[static_cast<size_t>(t)] = tok_off[static_cast<size_t>(t) + 1] - tok_off[static_cast<size_t>(t)];
    }
    if (c.df.empty()) {      // what lex_df_kernel counts: a term's postings
        c.df.resize(static_cast<size_t>(V));
        for (int64_t t = 0; t < V; ++t) c.df[static_cast<size_t>(t)] = post_off[static_cast<size_t>(t) + 1] - post_off[static_cast<size_t>(t)];
    }
    c.host_post_off.swap(post_off);
    c.num_postings = P;
    c.index_bytes = static_cast<int64_t>(c.post_off.n * sizeof(int64_t) + (c.post_doc.n + c.post_tf.n) * sizeof(int));
    c.indexed = true;
}

void Model::corpus_index(const nvsm_index_options& opt, nvsm_index_info* info) {
    if (!corpus_) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the inverted index needs a corpus: call nvsm_corpus_upload first");
    if (opt.use != NVSM_INDEX_AUTO && opt.use != NVSM_INDEX_ALWAYS && opt.use != NVSM_INDEX_NEVER)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown index use (NVSM_INDEX_AUTO, NVSM_INDEX_ALWAYS or NVSM_INDEX_NEVER)");
    if (cfg_.world_size > 1) throw Error(NVSM_ERR_UNSUPPORTED, "the inverted index is not implemented under data parallelism (world_size > 1)");
    Corpus& c = *corpus_;
    if (!c.indexed) {
        rank_join();
        try {
            index_build(c);
        } catch (...) {      // a refused or failed build leaves the corpus without an index
            c.post_off.release(); c.post_doc.release(); c.post_tf.release();
            throw;
        }
    }
    c.index_use = opt.use;
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->num_postings = c.num_postings; info->bytes = c.index_bytes; info->max_df = c.max_df; info->use = c.index_use;
    }
}

void Model::corpus_index_free() {
    if (!corpus_ || !corpus_->indexed) return;
    rank_join();      // whatever is queued may still read the postings
    Corpus& c = *corpus_;
    c.post_off.release(); c.post_doc.release(); c.post_tf.release();
    c.post_first.release(); c.pos.release();
    c.host_post_off.clear();
    c.indexed = c.positional = false; c.index_use = NVSM_INDEX_AUTO;
    c.num_postings = c.index_bytes = c.max_df = c.positions_bytes = 0;
}

// ---- the positional layer of the index (include/cunvsm_amd.h nvsm_corpus_index_positions; kernels: index.hip) -------
// index_build's sort once more, in a call of its own so that a plain nvsm_corpus_index keeps its scratch and its launches: the sorted
// entries' arena positions ARE the layer once every one is taken relative to its document, and the heads of index_build's scan are
// post_first. The scan's other outputs (post_doc, post_off, tok_off, rewritten with the values they hold already) go to scratch.
void Model::positions_build(Corpus& c) {
    const int64_t N = c.num_tokens, Dc = c.num_documents, V = cfg_.num_words, P = c.num_postings;
    RankProf scope(prof, "index_positions", stream_);
    c.post_first.alloc(static_cast<size_t>(P) + 1, true);      // (no token: post_first[0] = 0 = N)
    c.pos.alloc(static_cast<size_t>(std::max<int64_t>(N, 1)), true);
    if (N > 0) {
        int bits = 1;
        while (bits < 31 && (int64_t(1) << bits) < V) ++bits;
        DevBuf<int> term, doc, sums, post_doc;
        DevBuf<int64_t> post_off, tok;
        term.alloc(static_cast<size_t>(N));
        doc.alloc(static_cast<size_t>(N));
        {
            DevBuf<char> temp;
            const size_t temp_bytes = sort_pairs_temp_bytes(N, bits);
            temp.alloc(temp_bytes, true);
            sort_pairs(temp.p, temp_bytes, nullptr, c.tokens.p, term.p, nullptr, c.pos.p, N, bits, nullptr, stream_);
            launch_index_positions(c.pos.p, doc.p, N, c.offsets.p, Dc, stream_);
            NVSM_HIP_CHECK(hipStreamSynchronize(stream_));      // (the sort's workspace goes before the scan's comes)
        }
        const int64_t tiles = index_tiles(N);
        sums.alloc(static_cast<size_t>(tiles) + 1);
        post_doc.alloc(static_cast<size_t>(P));
        post_off.alloc(static_cast<size_t>(V) + 1);
        tok.alloc(static_cast<size_t>(V) + 1);
        launch_index_scan(term.p, doc.p, N, sums.p, stream_);
        int total = 0;
        NVSM_HIP_CHECK(hipMemcpyAsync(&total, sums.p + tiles, sizeof(int), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
        if (total != P) throw Error(NVSM_ERR_STATE,"the positional layer counted other postings than the index holds");
        launch_index_write(term.p, doc.p, N, V, sums.p, c.post_first.p, post_doc.p, post_off.p, tok.p, stream_);
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    }
    c.positions_bytes = static_cast<int64_t>((c.post_first.n + c.pos.n) * sizeof(int));
    c.positional = true;
}

void Model::corpus_index_positions(nvsm_positions_info* info) {
    if (!corpus_) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the positional layer needs a corpus: call nvsm_corpus_upload first");
    if (cfg_.world_size > 1) throw Error(NVSM_ERR_UNSUPPORTED, "the inverted index is not implemented under data parallelism (world_size > 1)");
    Corpus& c = *corpus_;
    if (!c.indexed) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the positional layer needs an inverted index: call nvsm_corpus_index first");
    if (!c.positional) {
        rank_join();
        try {
            positions_build(c);
        } catch (...) {      // a failed build leaves the index without the layer
            c.post_first.release(); c.pos.release();
            throw;
        }
    }
    if (info) {
        std::memset(info, 0, sizeof(*info));
        info->num_positions = c.num_tokens; info->bytes = c.positions_bytes;
    }
}

void Model::corpus_index_positions_free() {
    if (!corpus_ || !corpus_->positional) return;
    rank_join();      // whatever is queued may still read the layer
    Corpus& c = *corpus_;
    c.post_first.release(); c.pos.release();
    c.positional = false;
    c.positions_bytes = 0;
}

void Model::corpus_positions(int64_t word_id, int64_t doc_id, int64_t capacity, int64_t* positions, int64_t* count) {
    *count = 0;
    if (!corpus_) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the positional layer needs a corpus: call nvsm_corpus_upload first");
    if (!corpus_->indexed) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the corpus has no inverted index: call nvsm_corpus_index first");
    if (!corpus_->positional) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the index has no positional layer: call nvsm_corpus_index_positions first");
    if (word_id < 0 || word_id >= cfg_.num_words) throw Error(NVSM_ERR_INVALID_ARGUMENT, "word_id is outside [0, num_words)");
    const Corpus& c = *corpus_;
    if (doc_id < 0 || doc_id >= c.num_documents) throw Error(NVSM_ERR_INVALID_ARGUMENT, "doc_id is outside [0, num_documents of the corpus)");
    const int64_t lo = c.host_post_off[static_cast<size_t>(word_id)], n = c.host_post_off[static_cast<size_t>(word_id) + 1] - lo;
    if (n == 0) return;
    NVSM_HIP_CHECK(hipSetDevice(cfg_.device));
    std::vector<int> docs(static_cast<size_t>(n));
    NVSM_HIP_CHECK(hipMemcpy(docs.data(), c.post_doc.p + lo, static_cast<size_t>(n) * sizeof(int), hipMemcpyDeviceToHost));
    const auto it = std::lower_bound(docs.begin(), docs.end(), static_cast<int>(doc_id));
    if (it == docs.end() || *it != doc_id) return;
    const int64_t p = lo + (it - docs.begin());
    int first[2];
    NVSM_HIP_CHECK(hipMemcpy(first, c.post_first.p + p, sizeof(first), hipMemcpyDeviceToHost));
    const int64_t tf = first[1] - first[0];
    *count = tf;
    if (capacity < tf) throw Error(NVSM_ERR_INVALID_ARGUMENT, "capacity is below the word's count in the document (returned in count)");
    if (!positions) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: positions");
    std::vector<int> run(static_cast<size_t>(tf));
    NVSM_HIP_CHECK(hipMemcpy(run.data(), c.pos.p + first[0], static_cast<size_t>(tf) * sizeof(int), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < tf; ++i) positions[i] = run[static_cast<size_t>(i)];
}

void Model::corpus_postings(int64_t word_id, int64_t capacity, int64_t* doc_ids, int32_t* tfs, int64_t* count) {
    *count = 0;
    if (!corpus_) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the inverted index needs a corpus: call nvsm_corpus_upload first");
    if (!corpus_->indexed) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the corpus has no inverted index: call nvsm_corpus_index first");
    if (word_id < 0 || word_id >= cfg_.num_words) throw Error(NVSM_ERR_INVALID_ARGUMENT, "word_id is outside [0, num_words)");
    const Corpus& c = *corpus_;
    const int64_t lo = c.host_post_off[static_cast<size_t>(word_id)], n = c.host_post_off[static_cast<size_t>(word_id) + 1] - lo;
    *count = n;
    if (capacity < n) throw Error(NVSM_ERR_INVALID_ARGUMENT, "capacity is below the word's document frequency (returned in count)");
    if (n == 0) return;
    if (!doc_ids) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: doc_ids");
    if (!tfs) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: tfs");
    NVSM_HIP_CHECK(hipSetDevice(cfg_.device));
    std::vector<int> docs(static_cast<size_t>(n));
    NVSM_HIP_CHECK(hipMemcpy(docs.data(), c.post_doc.p + lo, static_cast<size_t>(n) * sizeof(int), hipMemcpyDeviceToHost));
    NVSM_HIP_CHECK(hipMemcpy(tfs, c.post_tf.p + lo, static_cast<size_t>(n) * sizeof(int), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; ++i) doc_ids[i] = docs[static_cast<size_t>(i)];
}

void Model::tfidf_rank(const nvsm_queries& q, const nvsm_tfidf_options& opt, int64_t* doc_ids, float* scores, int64_t* counts) {
    tfidf_check(q, opt);
    rank_join();
    const TfidfPlan plan = tfidf_plan(opt);
    nvsm_lexical_options rounds{};      // (what lexical_rounds reads of it in this form: top_k)
    rounds.top_k = opt.top_k;
    lexical_rounds(q, rounds, q.word_weights, doc_ids, scores, counts, &plan);
}

// nvsm_rerank: chunks of at most kInferChunk queries. The first stage's rounds of a chunk leave its candidate arrays on the device
// (Handover), then the rounds of nvsm_rank over candidate lists run on them: their layout needs the lists' lengths, which are the
// counts the first stage brought back. Both stages' rounds decide nothing about the bits: every (query, candidate) score and every
// query's sort are on their own.
void Model::rerank(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_rerank_options& rr, const nvsm_judgments* j, double* metrics,
                   int64_t* doc_ids, float* scores, int64_t* counts) {
    const int64_t D = cfg_.num_entities, Q = q.num_queries;
    if (opt.candidates || opt.candidate_offsets)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "rank_opt->candidates must be NULL: the first stage names the candidates");
    if (rr.first_stage != NVSM_STAGE_TFIDF && rr.first_stage != NVSM_STAGE_LEXICAL) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown first stage");
    if (!corpus_) throw Error(NVSM_ERR_INVALID_ARGUMENT, "lexical ranking needs a corpus: call nvsm_corpus_upload first");
    if (rr.depth < 1 || rr.depth > corpus_->num_documents)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "depth must be in [1, min(num_documents of the corpus, NVSM_RERANK_MAX_DEPTH)]");
    if (rr.depth > kRerankMaxDepth) throw Error(NVSM_ERR_UNSUPPORTED, "depth exceeds NVSM_RERANK_MAX_DEPTH");
    if (rr.depth < opt.top_k) throw Error(NVSM_ERR_INVALID_ARGUMENT, "depth must not be smaller than rank_opt->top_k");
    const bool by_tfidf = rr.first_stage == NVSM_STAGE_TFIDF;
    nvsm_queries plain = q;      // the first stage is unweighted
    plain.word_weights = nullptr;
    nvsm_tfidf_options tf{};
    nvsm_lexical_options lex{};
    if (by_tfidf) {
        if (rr.tfidf) tf = *rr.tfidf; else nvsm_tfidf_options_default(&tf);
        tf.top_k = rr.depth;
        tfidf_check(plain, tf);
        lex.top_k = rr.depth;
    } else {
        if (rr.lexical) lex = *rr.lexical; else nvsm_lexical_options_default(&lex);
        lex.top_k = rr.depth;
        lexical_check(plain, lex);
    }
    check_similarity(opt.similarity);
    check_top_k(opt.top_k, D, "top_k must be in [1, num_entities]");
    check_row_count(D, "ranking supports fewer than 2^31 documents");
    rank_check(q, opt);
    EvalPlan plan;
    EvalPlan* ev = nullptr;
    if (j) {
        plan.request = j;
        plan.metrics = metrics;
        eval_plan(plan, Q);
        ev = &plan;
    }
    rank_join();
    const TfidfPlan tplan = by_tfidf ? tfidf_plan(tf) : TfidfPlan{};
    RankScratch& r = rank_;
    const int k = opt.top_k;
    EvalArgs ea{};
    if (ev) ea = eval_upload(*ev, Q, k);
    std::vector<int64_t> sub_off, first_counts;
    for (int64_t c0 = 0; c0 < Q; c0 += kInferChunk) {
        const int64_t cn = std::min(kInferChunk, Q - c0);
        // ---- the first stage over the chunk's queries, handed over round by round
        grow(r.cand_off, static_cast<size_t>(kInferChunk) + 1);
        grow(r.cand, static_cast<size_t>(cn) * rr.depth);
        Handover hand;
        hand.cand = r.cand.p; hand.off_dev = r.cand_off.p;
        hand.off.assign(static_cast<size_t>(cn) + 1, 0);
        hand.nsort = static_cast<int>(pow2_at_least(rr.depth));
        NVSM_HIP_CHECK(hipMemcpy(r.cand_off.p, hand.off.data(), sizeof(int64_t), hipMemcpyHostToDevice));      // off[0] = 0
        sub_off.resize(static_cast<size_t>(cn) + 1);
        for (int64_t i = 0; i <= cn; ++i) sub_off[static_cast<size_t>(i)] = q.offsets[c0 + i] - q.offsets[c0];
        nvsm_queries sub{};
        sub.word_ids = q.word_ids ? q.word_ids + q.offsets[c0] : nullptr;
        sub.offsets = sub_off.data();
        sub.num_queries = cn;
        first_counts.assign(static_cast<size_t>(cn), 0);
        lexical_rounds(sub, lex, nullptr, nullptr, nullptr, first_counts.data(), by_tfidf ? &tplan : nullptr, &hand);
        // ---- nvsm_rank's rounds over the candidate lists where they lie: cand_off holds the chunk's absolute offsets, so a round
        // that begins at query s reads them from cand_off + s against the one cand array
        for (int64_t s = 0; s < cn;) {
            const RankLayout l = rank_layout_candidates(hand.off.data() + s, cn - s);
            rank_candidates_round(q, opt, c0 + s, l, r.cand.p, r.cand_off.p + s, ev ? &ea : nullptr, doc_ids, scores, counts);
            s += l.qn;
        }
    }
    if (ev && Q > 0)
        NVSM_HIP_CHECK(hipMemcpy(ev->metrics, r.metrics.p, static_cast<size_t>(Q) * ev->width * sizeof(double), hipMemcpyDeviceToHost));
    blank_wordless(q, k, doc_ids, scores, counts, ev ? ev->metrics : nullptr, ev ? ev->width : 0);
    raise_device_error();
}

// ---- weighted queries and pseudo-relevance feedback (include/cunvsm_amd.h nvsm_lexical_rank_weighted / nvsm_relevance_model /
// nvsm_lexical_rank_prf; kernels: lexical.hip) -------------------------------------------------------------------------
// The first pass is nvsm_lexical_rank's rounds at top_k = fb_docs into host lists. A round of the relevance model takes the lists of as
// many queries as 12·num_words bytes each fit the score slab's budget (at least one), accumulates them (one workgroup per query),
// narrows the accumulators slab by slab into the score slab and selects over the vocabulary with nvsm_rank's selection, sort and
// launch_lex_write: rows = num_words, top_k = fb_terms. The expanded queries are built on the host and go through the weighted rounds.
void Model::weights_check(const nvsm_queries& q) const {
    if (!q.word_weights) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: queries->word_weights");
    for (int64_t j = 0; j < q.offsets[q.num_queries]; ++j) {
        if (!std::isfinite(q.word_weights[j])) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a word weight is not finite");
        if (q.word_weights[j] < 0.f) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a word weight is negative");
    }
}

void Model::feedback_check(const nvsm_feedback_options& fb) const {
    if (fb.fb_docs < 1 || fb.fb_docs > std::min<int64_t>(corpus_->num_documents, kFeedbackMaxDocs))
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "fb_docs must be in [1, min(num_documents of the corpus, NVSM_FEEDBACK_MAX_DOCS)]");
    if (fb.fb_terms < 1 || fb.fb_terms > cfg_.num_words) throw Error(NVSM_ERR_INVALID_ARGUMENT, "fb_terms must be in [1, num_words]");
    if (!(fb.orig_weight >= 0.f && fb.orig_weight <= 1.f)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "orig_weight must be in [0, 1]");
    check_row_count(cfg_.num_words, "the relevance model supports fewer than 2^31 words");
}

void Model::lexical_rank_weighted(const nvsm_queries& q, const nvsm_lexical_options& lex, int64_t* doc_ids, float* scores, int64_t* counts) {
    lexical_check(q, lex);
    weights_check(q);
    rank_join();
    lexical_rounds(q, lex, q.word_weights, doc_ids, scores, counts);
}

void Model::relevance_model(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, int64_t* term_ids,
                            float* term_probs, int64_t* counts) {
    lexical_check(q, lex);
    feedback_check(fb);
    rank_join();
    relevance_rounds(q, lex, fb, term_ids, term_probs, counts);
}

void Model::relevance_rounds(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, int64_t* term_ids,
                             float* term_probs, int64_t* counts) {
    Corpus& c = *corpus_;
    const int64_t Q = q.num_queries, V = cfg_.num_words;
    const int nd = fb.fb_docs, kt = fb.fb_terms;
    // ---- the first pass: nvsm_lexical_rank at top_k = fb_docs (a word id out of range ends the call here)
    nvsm_lexical_options first = lex;
    first.top_k = nd;
    const size_t cells = static_cast<size_t>(std::max<int64_t>(Q, 1)) * nd;
    std::vector<int64_t> ids(cells), cnt(static_cast<size_t>(Q) + 1);
    std::vector<float> sc(cells);
    lexical_rounds(q, first, nullptr, ids.data(), sc.data(), cnt.data());

    RankScratch& r = rank_;
    const int64_t fit = std::max<int64_t>(1, score_floats() * 4 / (12 * V));      // queries whose acc and cnt fit the slab's budget
    std::vector<int> ids32, cnt32;
    for (int64_t q0 = 0; q0 < Q;) {
        RankLayout l = rank_layout(V, kt, Q - q0, score_floats());
        const int64_t qn = l.qn = std::min(l.qn, fit);       // (the slabs stay those of the layout, the scratch is sized by the queries taken)
        if (r.rm_acc.n < static_cast<size_t>(qn * V)) {      // zeroed once: the kernels leave both zero behind them
            r.rm_acc.alloc(static_cast<size_t>(qn * V), true);
            r.rm_cnt.alloc(static_cast<size_t>(qn * V), true);
        }
        grow(r.rm_sum, static_cast<size_t>(kRankChunk));
        grow(r.rm_counts, static_cast<size_t>(kRankChunk));
        grow(r.rm_ids, static_cast<size_t>(qn) * nd);
        grow(r.rm_scores, static_cast<size_t>(qn) * nd);
        ids32.resize(static_cast<size_t>(qn) * nd);
        cnt32.resize(static_cast<size_t>(qn));
        for (int64_t i = 0; i < qn; ++i) {
            const int n = static_cast<int>(cnt[static_cast<size_t>(q0 + i)]);
            cnt32[static_cast<size_t>(i)] = n;
            for (int t = 0; t < nd; ++t) ids32[static_cast<size_t>(i) * nd + t] = t < n ? static_cast<int>(ids[static_cast<size_t>(q0 + i) * nd + t]) : 0;
        }
        // (the main stream is idle here: the first pass, and every round, end with a wait)
        NVSM_HIP_CHECK(hipMemcpy(r.rm_ids.p, ids32.data(), ids32.size() * sizeof(int), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(r.rm_scores.p, sc.data() + q0 * nd, static_cast<size_t>(qn) * nd * sizeof(float), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(r.rm_counts.p, cnt32.data(), cnt32.size() * sizeof(int), hipMemcpyHostToDevice));
        LexRmArgs a{};
        a.tokens = c.tokens.p; a.doc_offsets = c.offsets.p;
        a.fb_ids = r.rm_ids.p; a.fb_scores = r.rm_scores.p; a.fb_counts = r.rm_counts.p; a.fb_docs = nd;
        a.V = V; a.acc = r.rm_acc.p; a.cnt = r.rm_cnt.p; a.sum_w = r.rm_sum.p;
        { RankProf scope(prof, "lex_rm", stream_); launch_lex_rm_accumulate(a, static_cast<int>(qn), stream_); }
        round_grow(l, kt);
        round_slabs(l, V, kt, [&](int64_t t0, int Ss) {
            RankProf scope(prof, "lex_rm_narrow", stream_);
            launch_lex_rm_narrow(r.rm_acc.p, r.rm_sum.p, V, t0, Ss, static_cast<int>(qn), r.scores.p, l.ld, stream_);
        });
        round_sort(l, [&] { launch_lex_write(r.keys.p, l.npad, static_cast<int>(qn), kt, l.n_keys, r.out_ids.p, r.out_scores.p, r.out_counts.p, stream_); });
        round_results(q0, qn, kt, term_ids, term_probs, counts);
        q0 += qn;
    }
    raise_device_error();
}

struct Model::ExpandedQueries {
    std::vector<int64_t> word_ids, offsets;
    std::vector<float> weights;
    nvsm_queries view() const {
        nvsm_queries x{};
        x.word_ids = word_ids.data(); x.word_weights = weights.data(); x.offsets = offsets.data();
        x.num_queries = static_cast<int64_t>(offsets.size()) - 1;
        return x;
    }
};

// the RM3 queries of the call: first pass, relevance model, and the weights in plain fp64 (a division, a difference, a product, a
// division: nothing a compiler could contract, so the numpy restatement produces the same float32 weights); refuses an expanded query of more than kLexSlots distinct terms
void Model::expand_queries(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, ExpandedQueries& out) {
    const int64_t Q = q.num_queries, V = cfg_.num_words;
    const int kt = fb.fb_terms;
    const size_t cells = static_cast<size_t>(std::max<int64_t>(Q, 1)) * kt;
    std::vector<int64_t> terms(cells), n_terms(static_cast<size_t>(Q) + 1);
    std::vector<float> probs(cells);
    relevance_rounds(q, lex, fb, terms.data(), probs.data(), n_terms.data());
    const std::vector<int64_t>& cf = corpus_->cf;      // (made by the first pass at the latest)
    const double o64 = static_cast<double>(fb.orig_weight);
    out.word_ids.clear(); out.weights.clear();
    out.offsets.assign(1, 0);
    for (int64_t i = 0; i < Q; ++i) {
        int64_t L = 0;
        for (int64_t j = q.offsets[i]; j < q.offsets[i + 1]; ++j) {
            const int64_t t = q.word_ids[j];
            if (t >= 0 && t < V && cf[static_cast<size_t>(t)] > 0) ++L;
        }
        if (L > 0) {
            const double each = o64 / static_cast<double>(L);
            for (int64_t j = q.offsets[i]; j < q.offsets[i + 1]; ++j) {
                const int64_t t = q.word_ids[j];
                if (!(t >= 0 && t < V && cf[static_cast<size_t>(t)] > 0)) continue;
                out.word_ids.push_back(t);
                out.weights.push_back(static_cast<float>(each));
            }
            const int64_t n = n_terms[static_cast<size_t>(i)];
            const float* pi = probs.data() + static_cast<size_t>(i) * kt;
            double S = 0.0;
            for (int64_t e = 0; e < n; ++e) S += static_cast<double>(pi[e]);
            for (int64_t e = 0; e < n; ++e) {
                const double num = (1.0 - o64) * static_cast<double>(pi[e]);
                out.word_ids.push_back(terms[static_cast<size_t>(i) * kt + e]);
                out.weights.push_back(static_cast<float>(num / S));
            }
        }
        out.offsets.push_back(static_cast<int64_t>(out.word_ids.size()));
    }
    const nvsm_queries x = out.view();
    lexical_check(x, lex);      // the distinct terms of every expanded query against the round's counters
}

void Model::lexical_rank_prf(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb, int64_t* doc_ids,
                             float* scores, int64_t* counts) {
    lexical_check(q, lex);
    feedback_check(fb);
    rank_join();
    ExpandedQueries x;
    expand_queries(q, lex, fb, x);
    lexical_rounds(x.view(), lex, x.weights.data(), doc_ids, scores, counts);
}

// ---- fusion of nvsm_rank's list with the lexical one (include/cunvsm_amd.h nvsm_rank_ensemble; fuse_lists_kernel) ----------------
// Both rankings are made by their own calls' rounds (whose sizes differ) into host lists; a round of fusion takes kRankChunk queries'
// lists back up, fuses them on the device and, with judgments, runs nvsm_evaluate's kernel on the fused ids where they lie.
void Model::rank_ensemble(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_ensemble_options& ens,
                          const nvsm_judgments* j, double* metrics, int64_t* doc_ids, float* scores, int64_t* counts) {
    ensemble_rounds(q, opt, lex, nullptr, ens, j, metrics, doc_ids, scores, counts);
}

void Model::rank_ensemble_prf(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options& fb,
                              const nvsm_ensemble_options& ens, const nvsm_judgments* j, double* metrics, int64_t* doc_ids, float* scores,
                              int64_t* counts) {
    ensemble_rounds(q, opt, lex, &fb, ens, j, metrics, doc_ids, scores, counts);
}

// both host lists of a call [Q][k] (+ counts), as the two rankings returned them
struct Model::EnsembleLists {
    int k = 0;
    std::vector<int64_t> ids_a, ids_b, cnt_a, cnt_b;
    std::vector<float> sc_a, sc_b;
};

// the refusals of nvsm_rank_ensemble(_prf), in their order, for every fused call; alphas [num_alphas]: the weights the call fuses with
void Model::ensemble_check(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                           int normalizer, const float* alphas, int64_t num_alphas, const nvsm_sdm_options* sdm) {
    lexical_check(q, lex);
    if (fb) feedback_check(*fb);
    if (sdm) sdm_check(q, *sdm);
    if (normalizer != NVSM_NORM_STANDARDIZE && normalizer != NVSM_NORM_MINMAX && normalizer != NVSM_NORM_NONE)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown score normalizer");
    for (int64_t i = 0; i < num_alphas; ++i)
        if (!(alphas[i] >= 0.f && alphas[i] <= 1.f)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "alpha must be in [0, 1]");
    if (opt.top_k != lex.top_k) throw Error(NVSM_ERR_INVALID_ARGUMENT, "rank_opt->top_k and lex->top_k must be equal");
    if (opt.candidates || opt.candidate_offsets) throw Error(NVSM_ERR_INVALID_ARGUMENT, "rank_opt->candidates must be NULL: the ensemble ranks every document");
    check_similarity(opt.similarity);
    check_top_k(opt.top_k, cfg_.num_entities, "top_k must be in [1, num_entities]");
    rank_check(q, opt);
    if (opt.top_k > kFuseMaxTopK) throw Error(NVSM_ERR_UNSUPPORTED, "the ensemble supports top_k up to NVSM_ENSEMBLE_MAX_TOP_K");
}

// list A: nvsm_rank's; list B: nvsm_lexical_rank's (fb null) or nvsm_lexical_rank_prf's — once per call
void Model::ensemble_lists(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                           EnsembleLists& l, const nvsm_sdm_options* sdm) {
    const int64_t Q = q.num_queries;
    l.k = opt.top_k;
    const size_t cells = static_cast<size_t>(std::max<int64_t>(Q, 1)) * l.k;
    l.ids_a.resize(cells); l.ids_b.resize(cells); l.sc_a.resize(cells); l.sc_b.resize(cells);
    l.cnt_a.resize(static_cast<size_t>(Q) + 1); l.cnt_b.resize(static_cast<size_t>(Q) + 1);
    rank_rounds(q, opt, l.ids_a.data(), l.sc_a.data(), l.cnt_a.data(), nullptr);
    if (fb) {
        ExpandedQueries x;
        expand_queries(q, lex, *fb, x);
        lexical_rounds(x.view(), lex, x.weights.data(), l.ids_b.data(), l.sc_b.data(), l.cnt_b.data());
    } else if (sdm) {
        sdm_rounds(q, &lex, *sdm, l.ids_b.data(), l.sc_b.data(), l.cnt_b.data(), nullptr, nullptr);
    } else {
        lexical_rounds(q, lex, nullptr, l.ids_b.data(), l.sc_b.data(), l.cnt_b.data());
    }
}

// the lists of queries [q0, q0 + qn) of a round (qn <= kRankChunk) on the device, as the fusion kernels read them
FuseArgs Model::ensemble_upload(const EnsembleLists& l, int64_t q0, int64_t qn, int normalizer) {
    RankScratch& r = rank_;
    const int k = l.k;
    const size_t chunk_cells = static_cast<size_t>(kRankChunk) * k;
    grow(r.fuse_ids, 2 * chunk_cells);
    grow(r.fuse_scores, 2 * chunk_cells);
    grow(r.fuse_counts, static_cast<size_t>(2 * kRankChunk));
    const size_t n = static_cast<size_t>(qn) * k;
    // (the main stream is idle here: both rankings, and every round, end with a wait)
    NVSM_HIP_CHECK(hipMemcpy(r.fuse_ids.p, l.ids_a.data() + q0 * k, n * sizeof(int64_t), hipMemcpyHostToDevice));
    NVSM_HIP_CHECK(hipMemcpy(r.fuse_ids.p + chunk_cells, l.ids_b.data() + q0 * k, n * sizeof(int64_t), hipMemcpyHostToDevice));
    NVSM_HIP_CHECK(hipMemcpy(r.fuse_scores.p, l.sc_a.data() + q0 * k, n * sizeof(float), hipMemcpyHostToDevice));
    NVSM_HIP_CHECK(hipMemcpy(r.fuse_scores.p + chunk_cells, l.sc_b.data() + q0 * k, n * sizeof(float), hipMemcpyHostToDevice));
    NVSM_HIP_CHECK(hipMemcpy(r.fuse_counts.p, l.cnt_a.data() + q0, static_cast<size_t>(qn) * sizeof(int64_t), hipMemcpyHostToDevice));
    NVSM_HIP_CHECK(hipMemcpy(r.fuse_counts.p + kRankChunk, l.cnt_b.data() + q0, static_cast<size_t>(qn) * sizeof(int64_t), hipMemcpyHostToDevice));
    FuseArgs f{};
    f.ids_a = r.fuse_ids.p; f.scores_a = r.fuse_scores.p; f.counts_a = r.fuse_counts.p;
    f.ids_b = r.fuse_ids.p + chunk_cells; f.scores_b = r.fuse_scores.p + chunk_cells; f.counts_b = r.fuse_counts.p + kRankChunk;
    f.k = k; f.npad = static_cast<int>(pow2_at_least(2 * k)); f.normalizer = normalizer;
    return f;
}

// the fused lists of the call, round by round. query_alpha null: every query at `alpha`; given [Q]: query i at query_alpha[i].
// plan given: nvsm_evaluate's kernel on the fused ids where they lie, the rows into plan->metrics.
void Model::fuse_rounds(const nvsm_queries& q, const EnsembleLists& l, int normalizer, float alpha, const float* query_alpha, const EvalPlan* plan,
                        int64_t* doc_ids, float* scores, int64_t* counts) {
    const int64_t Q = q.num_queries;
    const int k = l.k;
    RankScratch& r = rank_;
    const size_t chunk_cells = static_cast<size_t>(kRankChunk) * k;
    grow(r.fuse_out_ids, 2 * chunk_cells);
    grow(r.fuse_out_scores, 2 * chunk_cells);
    grow(r.fuse_out_counts, static_cast<size_t>(kRankChunk));
    if (query_alpha) grow(r.fuse_alpha, static_cast<size_t>(kRankChunk));
    EvalArgs ea{};
    if (plan) ea = eval_upload(*plan, Q, 2 * k);
    for (int64_t q0 = 0; q0 < Q; q0 += kRankChunk) {
        const int64_t qn = std::min(kRankChunk, Q - q0);
        const size_t n = static_cast<size_t>(qn) * 2 * k;      // entries of the round's fused lists
        FuseArgs f = ensemble_upload(l, q0, qn, normalizer);
        f.alpha = alpha;
        if (query_alpha) {
            NVSM_HIP_CHECK(hipMemcpy(r.fuse_alpha.p, query_alpha + q0, static_cast<size_t>(qn) * sizeof(float), hipMemcpyHostToDevice));
            f.query_alpha = r.fuse_alpha.p;
        }
        f.out_ids = r.fuse_out_ids.p; f.out_scores = r.fuse_out_scores.p; f.out_counts = r.fuse_out_counts.p;
        { RankProf scope(prof, "fuse_lists", stream_); launch_fuse_lists(f, static_cast<int>(qn), stream_); }
        if (plan) {
            RankProf scope(prof, "rank_eval", stream_);
            ea.ids = r.fuse_out_ids.p; ea.counts = r.fuse_out_counts.p; ea.q0 = q0;
            launch_eval_metrics(ea, static_cast<int>(qn), stream_);
        }
        NVSM_HIP_CHECK(hipMemcpyAsync(doc_ids + q0 * 2 * k, r.fuse_out_ids.p, n * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipMemcpyAsync(scores + q0 * 2 * k, r.fuse_out_scores.p, n * sizeof(float), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipMemcpyAsync(counts + q0, r.fuse_out_counts.p, static_cast<size_t>(qn) * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    }
    if (plan && Q > 0) {
        double* metrics = plan->metrics;
        NVSM_HIP_CHECK(hipMemcpy(metrics, r.metrics.p, static_cast<size_t>(Q) * plan->width * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < Q; ++i)      // a query without words gets all zeros, as in nvsm_evaluate
            if (q.offsets[i + 1] == q.offsets[i]) std::fill(metrics + i * plan->width, metrics + (i + 1) * plan->width, 0.0);
    }
    raise_device_error();
}

// fb null: list B is nvsm_lexical_rank's; given: nvsm_lexical_rank_prf's
void Model::ensemble_rounds(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                            const nvsm_ensemble_options& ens, const nvsm_judgments* j, double* metrics, int64_t* doc_ids, float* scores,
                            int64_t* counts, const nvsm_sdm_options* sdm) {
    ensemble_check(q, opt, lex, fb, ens.normalizer, &ens.alpha, 1, sdm);
    EvalPlan plan;
    if (j) { plan.request = j; plan.metrics = metrics; eval_plan(plan, q.num_queries); }
    EnsembleLists l;
    ensemble_lists(q, opt, lex, fb, l, sdm);
    fuse_rounds(q, l, ens.normalizer, ens.alpha, nullptr, j ? &plan : nullptr, doc_ids, scores, counts);
}

// ---- sequential dependence: terms, ordered pairs, unordered pairs in a window (include/cunvsm_amd.h nvsm_sdm_rank / nvsm_sdm_pair_counts
// / nvsm_rank_ensemble_sdm; kernels: sdm.hip) ---------------------------------------------------------------------------
// lexical_rounds' frame: a round takes queries while their distinct remaining terms fit kSdmSlots counters AND their distinct pairs
// fit kSdmPairs; the terms go into the slot table, the pairs into a small CSR by slot. One counting pass over ALL documents gives the
// round's collection counts (integers, read back: the host drops what has none and evaluates log(c0) once per member), then the
// slabs are filled by launch_sdm_score and selection, sort, write and results are those of every other round.
void Model::sdm_check(const nvsm_queries& q, const nvsm_sdm_options& sdm) const {
    if (!corpus_) throw Error(NVSM_ERR_INVALID_ARGUMENT, "lexical ranking needs a corpus: call nvsm_corpus_upload first");
    check_row_count(corpus_->num_documents, "ranking supports fewer than 2^31 documents");
    check_queries(q);
    const float w[3] = {sdm.w_term, sdm.w_ordered, sdm.w_unordered};
    for (float x : w)
        if (!std::isfinite(x) || x < 0.f) throw Error(NVSM_ERR_INVALID_ARGUMENT, "an sdm weight (w_term, w_ordered, w_unordered) is negative or not finite");
    if (w[0] == 0.f && w[1] == 0.f && w[2] == 0.f) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the three sdm weights are all zero");
    if (sdm.window < 2 || sdm.window > kSdmMaxWindow) throw Error(NVSM_ERR_INVALID_ARGUMENT, "sdm->window must be in [2, NVSM_SDM_MAX_WINDOW]");
    std::vector<int64_t> one;
    std::vector<std::pair<int64_t, int64_t>> two;
    for (int64_t i = 0; i < q.num_queries; ++i) {
        const int64_t L = q.offsets[i + 1] - q.offsets[i];
        if (L <= kSdmSlots && L - 1 <= kSdmPairs) continue;
        one.assign(q.word_ids + q.offsets[i], q.word_ids + q.offsets[i + 1]);
        two.clear();
        for (int64_t j = 0; j + 1 < L; ++j) two.emplace_back(one[static_cast<size_t>(j)], one[static_cast<size_t>(j) + 1]);
        std::sort(one.begin(), one.end());
        if (std::unique(one.begin(), one.end()) - one.begin() > kSdmSlots)
            throw Error(NVSM_ERR_UNSUPPORTED, "a query has more than NVSM_LEXICAL_MAX_QUERY_TERMS distinct terms");
        std::sort(two.begin(), two.end());
        if (std::unique(two.begin(), two.end()) - two.begin() > kSdmPairs)
            throw Error(NVSM_ERR_UNSUPPORTED, "a query has more than NVSM_SDM_MAX_QUERY_PAIRS distinct term pairs");
    }
}

void Model::sdm_rank(const nvsm_queries& q, const nvsm_lexical_options& lex, const nvsm_sdm_options& sdm, int64_t* doc_ids, float* scores,
                     int64_t* counts) {
    lexical_check(q, lex);
    sdm_check(q, sdm);
    rank_join();
    sdm_rounds(q, &lex, sdm, doc_ids, scores, counts, nullptr, nullptr);
}

void Model::sdm_pair_counts(const nvsm_queries& q, const nvsm_sdm_options& sdm, uint64_t* ordered, uint64_t* unordered) {
    sdm_check(q, sdm);
    rank_join();
    sdm_rounds(q, nullptr, sdm, nullptr, nullptr, nullptr, ordered, unordered);
}

void Model::rank_ensemble_sdm(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_sdm_options& sdm,
                              const nvsm_ensemble_options& ens, const nvsm_judgments* j, double* metrics, int64_t* doc_ids, float* scores,
                              int64_t* counts) {
    ensemble_rounds(q, opt, lex, nullptr, ens, j, metrics, doc_ids, scores, counts, &sdm);
}

void Model::sdm_rounds(const nvsm_queries& q, const nvsm_lexical_options* lex, const nvsm_sdm_options& sdm, int64_t* doc_ids, float* scores,
                       int64_t* counts, uint64_t* ordered, uint64_t* unordered) {
    Corpus& c = *corpus_;
    const int64_t Dc = c.num_documents, N = c.num_tokens, Q = q.num_queries, V = cfg_.num_words;
    const int k = lex ? lex->top_k : 1;
    RankScratch& r = rank_;
    corpus_cf();
    if (r.lex_slot_of.n < static_cast<size_t>(V)) {
        r.lex_slot_of.alloc(static_cast<size_t>(V));
        launch_lex_fill_int(r.lex_slot_of.p, V, -1, stream_);
    }
    double param = 0.0;
    if (lex)
        param = lex->method == NVSM_LEX_JM ? (lex->param == 0.f ? 0.5 : static_cast<double>(lex->param))
                                           : (lex->param == 0.f ? static_cast<double>(N) / static_cast<double>(Dc) : static_cast<double>(lex->param));
    const double w[3] = {static_cast<double>(sdm.w_term), static_cast<double>(sdm.w_ordered), static_cast<double>(sdm.w_unordered)};
    bool bad_word = false;
    std::vector<int> terms, pair_a, pair_b;              // the round's distinct terms by slot, its distinct pairs by id (slots)
    std::vector<std::pair<int64_t, int>> slot_of;        // (term, slot), sorted by term
    std::vector<std::pair<int64_t, int>> pair_of;        // (first slot · kSdmSlots + second slot, pair id), sorted
    std::vector<int> qslot, qpair, qfirst;               // every query position's slot, the pair id of (position, position + 1); -1: dropped
    std::vector<int> ent_off, ent_other, ent_pair, goff, index;
    std::vector<double> c0, base, coef;
    std::vector<unsigned long long> cf(2 * static_cast<size_t>(kSdmPairs));
    int64_t pairs_out = 0;                               // pairs of the queries before this round, in the layout of ordered / unordered
    const bool layered = c.indexed && c.positional && c.index_use != NVSM_INDEX_NEVER;      // the rounds may be served from the postings

    for (int64_t q0 = 0; q0 < Q;) {
        RankLayout l{};
        if (lex) l = rank_layout(Dc, k, Q - q0, score_floats());
        else l.qn = std::min(kRankChunk, Q - q0);
        terms.clear(); pair_a.clear(); pair_b.clear(); slot_of.clear(); pair_of.clear(); qslot.clear(); qpair.clear();
        qfirst.assign(1, 0);
        int64_t taken = 0;
        for (; taken < l.qn; ++taken) {
            const size_t terms_before = terms.size(), pairs_before = pair_a.size(), cells_before = qslot.size();
            bool fits = true;
            const int64_t j0 = q.offsets[q0 + taken], j1 = q.offsets[q0 + taken + 1];
            for (int64_t j = j0; j < j1 && fits; ++j) {
                const int64_t t = q.word_ids[j];
                int slot = -1;
                if (t < 0 || t >= V) {
                    bad_word = true;      // the index contract: matches nothing, reported at the end
                } else if (c.cf[static_cast<size_t>(t)] != 0) {
                    auto it = std::lower_bound(slot_of.begin(), slot_of.end(), std::make_pair(t, -1));
                    if (it != slot_of.end() && it->first == t) {
                        slot = it->second;
                    } else if (terms.size() == static_cast<size_t>(kSdmSlots)) {
                        fits = false;
                    } else {
                        slot = static_cast<int>(terms.size());
                        slot_of.insert(it, std::make_pair(t, slot));
                        terms.push_back(static_cast<int>(t));
                    }
                }
                qslot.push_back(slot);
            }
            // the pairs of the query as given: qpair[cell] is the pair (cell, cell + 1), -1 at the query's last position
            for (size_t i = cells_before; fits && i < qslot.size(); ++i) {
                int pair = -1;
                if (i + 1 < qslot.size() && qslot[i] >= 0 && qslot[i + 1] >= 0) {      // (a pair with a term nobody holds has no occurrence: dropped)
                    const int64_t key = static_cast<int64_t>(qslot[i]) * kSdmSlots + qslot[i + 1];
                    auto it = std::lower_bound(pair_of.begin(), pair_of.end(), std::make_pair(key, -1));
                    if (it != pair_of.end() && it->first == key) {
                        pair = it->second;
                    } else if (pair_a.size() == static_cast<size_t>(kSdmPairs)) {
                        fits = false;
                    } else {
                        pair = static_cast<int>(pair_a.size());
                        pair_of.insert(it, std::make_pair(key, pair));
                        pair_a.push_back(qslot[i]); pair_b.push_back(qslot[i + 1]);
                    }
                }
                qpair.push_back(pair);
            }
            if (!fits) {      // this query opens the next round (alone it fits: sdm_check): take back what it added
                slot_of.erase(std::remove_if(slot_of.begin(), slot_of.end(), [&](const std::pair<int64_t, int>& e) { return e.second >= static_cast<int>(terms_before); }),
                              slot_of.end());
                pair_of.erase(std::remove_if(pair_of.begin(), pair_of.end(), [&](const std::pair<int64_t, int>& e) { return e.second >= static_cast<int>(pairs_before); }),
                              pair_of.end());
                terms.resize(terms_before); pair_a.resize(pairs_before); pair_b.resize(pairs_before);
                qslot.resize(cells_before);
                qpair.resize(cells_before);
                break;
            }
            qfirst.push_back(static_cast<int>(qslot.size()));
        }
        const int64_t qn = l.qn = taken;
        const int nslots = static_cast<int>(terms.size()), npairs = static_cast<int>(pair_a.size());

        // ---- the pair entries by slot, the slot table, the collection counts of the round's pairs
        ent_off.assign(static_cast<size_t>(nslots) + 1, 0);
        for (int p = 0; p < npairs; ++p) {
            ++ent_off[static_cast<size_t>(pair_a[p]) + 1];
            if (pair_b[p] != pair_a[p]) ++ent_off[static_cast<size_t>(pair_b[p]) + 1];
        }
        for (int s = 0; s < nslots; ++s) ent_off[static_cast<size_t>(s) + 1] += ent_off[static_cast<size_t>(s)];
        const size_t nentries = static_cast<size_t>(ent_off[static_cast<size_t>(nslots)]);
        ent_other.assign(std::max<size_t>(nentries, 1), 0);
        ent_pair.assign(std::max<size_t>(nentries, 1), 0);
        {
            std::vector<int> at(ent_off.begin(), ent_off.end() - 1);
            for (int p = 0; p < npairs; ++p) {
                const int a = pair_a[p], b = pair_b[p];
                ent_other[static_cast<size_t>(at[a])] = b; ent_pair[static_cast<size_t>(at[a]++)] = (p << 1) | 1;
                if (b != a) { ent_other[static_cast<size_t>(at[b])] = a; ent_pair[static_cast<size_t>(at[b]++)] = p << 1; }
            }
        }
        grow(r.lex_terms, static_cast<size_t>(kLexSlots));
        grow(r.sdm_ent_off, static_cast<size_t>(kSdmSlots) + 1);
        grow(r.sdm_ent_other, static_cast<size_t>(2 * kSdmPairs));
        grow(r.sdm_ent_pair, static_cast<size_t>(2 * kSdmPairs));
        grow(r.sdm_cf, cf.size());
        // (the main stream is idle here: every round ends with a wait)
        if (nslots > 0) NVSM_HIP_CHECK(hipMemcpy(r.lex_terms.p, terms.data(), static_cast<size_t>(nslots) * sizeof(int), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(r.sdm_ent_off.p, ent_off.data(), ent_off.size() * sizeof(int), hipMemcpyHostToDevice));
        if (nentries > 0) {
            NVSM_HIP_CHECK(hipMemcpy(r.sdm_ent_other.p, ent_other.data(), nentries * sizeof(int), hipMemcpyHostToDevice));
            NVSM_HIP_CHECK(hipMemcpy(r.sdm_ent_pair.p, ent_pair.data(), nentries * sizeof(int), hipMemcpyHostToDevice));
        }
        SdmScoreArgs a{};
        a.count.tokens = c.tokens.p; a.count.doc_offsets = c.offsets.p; a.count.slot_of = r.lex_slot_of.p;
        a.count.ent_off = r.sdm_ent_off.p; a.count.ent_other = r.sdm_ent_other.p; a.count.ent_pair = r.sdm_ent_pair.p;
        a.count.num_slots = nslots; a.count.num_pairs = npairs; a.count.window = sdm.window;
        // both phases of this round: the arena scan, or the positional postings of the round's terms. Both give the
        // same bits, so the choice — the caller's, or under NVSM_INDEX_AUTO sdm_auto_takes_postings' — is invisible in the results
        bool postings = layered && c.index_use == NVSM_INDEX_ALWAYS;
        int64_t round_max_df = 0;
        SdmPostingsScoreArgs pa{};
        if (layered) {
            // the fill's searched and merged entries: every pair merges at most the occurrences of its two terms, and every posting of
            // a query's distinct terms searches once per member of that query
            double work = 0.0;
            for (int p = 0; p < npairs; ++p)
                work += static_cast<double>(c.cf[static_cast<size_t>(terms[static_cast<size_t>(pair_a[p])])] + c.cf[static_cast<size_t>(terms[static_cast<size_t>(pair_b[p])])]);
            std::vector<char> seen(static_cast<size_t>(std::max(nslots, 1)));
            for (int64_t i = 0; i < qn; ++i) {
                std::fill(seen.begin(), seen.end(), 0);
                double query_df = 0.0, members = 0.0;
                for (int cell = qfirst[static_cast<size_t>(i)]; cell < qfirst[static_cast<size_t>(i) + 1]; ++cell) {
                    const int s = qslot[static_cast<size_t>(cell)];
                    if (s < 0) continue;
                    members += qpair[static_cast<size_t>(cell)] >= 0 ? 3.0 : 1.0;      // the term, and its pair in O and in U
                    if (!seen[static_cast<size_t>(s)]) { seen[static_cast<size_t>(s)] = 1; query_df += static_cast<double>(c.df[static_cast<size_t>(terms[static_cast<size_t>(s)])]); }
                }
                work += query_df * members;
            }
            for (int s = 0; s < nslots; ++s) round_max_df = std::max(round_max_df, c.df[static_cast<size_t>(terms[static_cast<size_t>(s)])]);
            if (c.index_use == NVSM_INDEX_AUTO) postings = sdm_auto_takes_postings(work, N);
        }
        if (postings) {
            grow(r.sdm_pair_a, static_cast<size_t>(kSdmPairs));
            grow(r.sdm_pair_b, static_cast<size_t>(kSdmPairs));
            if (npairs > 0) {
                NVSM_HIP_CHECK(hipMemcpy(r.sdm_pair_a.p, pair_a.data(), static_cast<size_t>(npairs) * sizeof(int), hipMemcpyHostToDevice));
                NVSM_HIP_CHECK(hipMemcpy(r.sdm_pair_b.p, pair_b.data(), static_cast<size_t>(npairs) * sizeof(int), hipMemcpyHostToDevice));
            }
            pa.post.post_off = c.post_off.p; pa.post.post_doc = c.post_doc.p; pa.post.post_tf = c.post_tf.p;
            pa.post.post_first = c.post_first.p; pa.post.pos = c.pos.p;
            pa.post.terms = r.lex_terms.p; pa.post.pair_a = r.sdm_pair_a.p; pa.post.pair_b = r.sdm_pair_b.p;
            pa.post.num_slots = nslots; pa.post.num_pairs = npairs; pa.post.window = sdm.window;
        }
        std::fill(cf.begin(), cf.end(), 0ull);
        if (!postings) launch_lex_set_slots(r.lex_slot_of.p, r.lex_terms.p, nslots, true, stream_);
        if (npairs > 0) {
            NVSM_HIP_CHECK(hipMemsetAsync(r.sdm_cf.p, 0, cf.size() * sizeof(unsigned long long), stream_));
            if (postings) {
                RankProf scope(prof, "sdm_postings_collect", stream_);
                launch_sdm_postings_collect(pa.post, round_max_df, r.sdm_cf.p, r.sdm_cf.p + kSdmPairs, stream_);
            } else {
                RankProf scope(prof, "sdm_collect", stream_);
                launch_sdm_collect(a.count, Dc, r.sdm_cf.p, r.sdm_cf.p + kSdmPairs, stream_);
            }
            NVSM_HIP_CHECK(hipMemcpyAsync(cf.data(), r.sdm_cf.p, cf.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream_));
            NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
        }
        const unsigned long long* cf_o = cf.data();
        const unsigned long long* cf_u = cf.data() + kSdmPairs;
        if (ordered || unordered) {
            for (int64_t i = 0; i < qn; ++i) {
                for (int cell = qfirst[static_cast<size_t>(i)]; cell + 1 < qfirst[static_cast<size_t>(i) + 1]; ++cell) {
                    const int p = qpair[static_cast<size_t>(cell)];
                    if (ordered) ordered[pairs_out] = p >= 0 ? cf_o[p] : 0;
                    if (unordered) unordered[pairs_out] = p >= 0 ? cf_u[p] : 0;
                    ++pairs_out;
                }
            }
        }
        if (!lex) {
            if (!postings) launch_lex_set_slots(r.lex_slot_of.p, r.lex_terms.p, nslots, false, stream_);
            NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
            q0 += qn;
            continue;
        }

        // ---- the members of every query's three groups, in query order, and the queries' group coefficients
        goff.assign(3 * (static_cast<size_t>(qn) + 1), 0);
        index.clear(); c0.clear(); base.clear();
        coef.assign(3 * static_cast<size_t>(std::max<int64_t>(qn, 1)), 0.0);
        auto member = [&](int idx, double held) {
            const double v = param * (held / static_cast<double>(N));
            index.push_back(idx); c0.push_back(v); base.push_back(std::log(v));
        };
        for (int g = 0; g < 3; ++g) {
            int* off = goff.data() + static_cast<size_t>(g) * (static_cast<size_t>(qn) + 1);
            for (int64_t i = 0; i < qn; ++i) {
                off[i] = static_cast<int>(index.size());
                for (int cell = qfirst[static_cast<size_t>(i)]; cell < qfirst[static_cast<size_t>(i) + 1]; ++cell) {
                    if (g == 0) {
                        const int s = qslot[static_cast<size_t>(cell)];
                        if (s >= 0) member(s, static_cast<double>(c.cf[static_cast<size_t>(terms[static_cast<size_t>(s)])]));
                    } else {
                        const int p = qpair[static_cast<size_t>(cell)];
                        const unsigned long long held = p >= 0 ? (g == 1 ? cf_o[p] : cf_u[p]) : 0ull;
                        if (held > 0) member(p, static_cast<double>(held));
                    }
                }
            }
            off[qn] = static_cast<int>(index.size());
        }
        for (int64_t i = 0; i < qn; ++i) {
            double total = 0.0;
            bool present[3];
            for (int g = 0; g < 3; ++g) {
                const int* off = goff.data() + static_cast<size_t>(g) * (static_cast<size_t>(qn) + 1);
                present[g] = off[i + 1] > off[i] && w[g] > 0.0;
                if (present[g]) total += w[g];
            }
            for (int g = 0; g < 3; ++g) coef[static_cast<size_t>(i) * 3 + g] = present[g] ? w[g] / total : 0.0;
        }
        const size_t nmem = index.size();
        grow(r.sdm_goff, 3 * (static_cast<size_t>(kRankChunk) + 1));
        grow(r.sdm_coef, 3 * static_cast<size_t>(kRankChunk));
        grow(r.sdm_index, std::max<size_t>(nmem, 1));
        grow(r.sdm_c0, std::max<size_t>(nmem, 1));
        grow(r.sdm_base, std::max<size_t>(nmem, 1));
        NVSM_HIP_CHECK(hipMemcpy(r.sdm_goff.p, goff.data(), goff.size() * sizeof(int), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(r.sdm_coef.p, coef.data(), coef.size() * sizeof(double), hipMemcpyHostToDevice));
        if (nmem > 0) {
            NVSM_HIP_CHECK(hipMemcpy(r.sdm_index.p, index.data(), nmem * sizeof(int), hipMemcpyHostToDevice));
            NVSM_HIP_CHECK(hipMemcpy(r.sdm_c0.p, c0.data(), nmem * sizeof(double), hipMemcpyHostToDevice));
            NVSM_HIP_CHECK(hipMemcpy(r.sdm_base.p, base.data(), nmem * sizeof(double), hipMemcpyHostToDevice));
        }
        round_grow(l, k);
        a.Q = static_cast<int>(qn); a.method = lex->method; a.param = param;
        a.goff = r.sdm_goff.p; a.index = r.sdm_index.p; a.c0 = r.sdm_c0.p; a.base = r.sdm_base.p; a.coef = r.sdm_coef.p;
        a.ld = l.ld;
        if (postings) {      // every member of group 0: its query, and whether it is the first of its slot there (index.hip's ownership)
            const size_t nent = static_cast<size_t>(goff[static_cast<size_t>(qn)]);
            std::vector<int> entry_query(nent), entry_first(nent);
            for (int64_t i = 0; i < qn; ++i)
                for (int j = goff[static_cast<size_t>(i)]; j < goff[static_cast<size_t>(i) + 1]; ++j) {
                    entry_query[static_cast<size_t>(j)] = static_cast<int>(i);
                    entry_first[static_cast<size_t>(j)] =
                        std::find(index.begin() + goff[static_cast<size_t>(i)], index.begin() + j, index[static_cast<size_t>(j)]) == index.begin() + j ? 1 : 0;
                }
            grow(r.post_query, std::max<size_t>(nent, 1));
            grow(r.post_first, std::max<size_t>(nent, 1));
            grow(r.post_lo, static_cast<size_t>(kLexSlots));
            grow(r.post_hi, static_cast<size_t>(kLexSlots));
            if (nent > 0) {
                NVSM_HIP_CHECK(hipMemcpy(r.post_query.p, entry_query.data(), nent * sizeof(int), hipMemcpyHostToDevice));
                NVSM_HIP_CHECK(hipMemcpy(r.post_first.p, entry_first.data(), nent * sizeof(int), hipMemcpyHostToDevice));
            }
            pa.entry_query = r.post_query.p; pa.first = r.post_first.p; pa.num_entries = static_cast<int>(nent);
            pa.lo = r.post_lo.p; pa.hi = r.post_hi.p;
        }
        round_slabs(l, Dc, k, [&](int64_t d0, int Ss) {
            a.scores = r.scores.p; a.d0 = d0; a.S = Ss;
            if (postings) {
                pa.score = a;
                RankProf scope(prof, "sdm_postings_score", stream_);
                launch_sdm_postings_score(pa, round_max_df, stream_);
                return;
            }
            RankProf scope(prof, "sdm_score", stream_);
            launch_sdm_score(a, stream_);
        });
        if (!postings) launch_lex_set_slots(r.lex_slot_of.p, r.lex_terms.p, nslots, false, stream_);
        round_sort(l, [&] { launch_lex_write(r.keys.p, l.npad, static_cast<int>(qn), k, l.n_keys, r.out_ids.p, r.out_scores.p, r.out_counts.p, stream_); });
        round_results(q0, qn, k, doc_ids, scores, counts);
        q0 += qn;
    }
    raise_device_error();
    if (bad_word) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a query word id is outside [0, num_words)");
}

// ---- supervised fusion: the alpha sweep and the k-fold choice (include/cunvsm_amd.h nvsm_ensemble_sweep / nvsm_rank_ensemble_cv;
// fuse_sweep_kernel) ------------------------------------------------------------------------------------------------
// Both rankings once; a round takes kRankChunk queries' lists up once and one launch sweeps every alpha over them; the table
// [num_alphas][Q][width] stays on the device until the last round.
void Model::sweep_check(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                        const nvsm_sweep_options& sw, const nvsm_judgments& j, double* table, EvalPlan& plan) {
    if (!sw.alphas) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: sweep->alphas");
    if (sw.num_alphas < 1 || sw.num_alphas > NVSM_SWEEP_MAX_ALPHAS)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "sweep->num_alphas must be in [1, NVSM_SWEEP_MAX_ALPHAS]");
    if (sw.depth < 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "sweep->depth is negative");
    ensemble_check(q, opt, lex, fb, sw.normalizer, sw.alphas, sw.num_alphas);
    plan.request = &j;
    plan.metrics = table;
    eval_plan(plan, q.num_queries);
}

void Model::sweep_rounds(const nvsm_queries& q, const EnsembleLists& l, const nvsm_sweep_options& sw, const EvalPlan& plan, double* table) {
    const int64_t Q = q.num_queries, A = sw.num_alphas;
    if (Q == 0) return;
    RankScratch& r = rank_;
    const size_t cells = static_cast<size_t>(A) * Q * plan.width;
    grow(r.sweep_alphas, static_cast<size_t>(kFuseSweepMaxAlphas));
    grow(r.sweep_table, cells);
    NVSM_HIP_CHECK(hipMemcpy(r.sweep_alphas.p, sw.alphas, static_cast<size_t>(A) * sizeof(float), hipMemcpyHostToDevice));
    FuseSweepArgs s{};
    // the judgments and their constants as launch_eval_metrics reads them. Of what eval_upload returns the sweep kernel looks at jids,
    // jgrades, joff, consts, the cutoffs and q0 only: its ids are in LDS and its rows go to `table`, so ids, counts, k and metrics stay
    // unused here (eval_upload also makes sure rank_.metrics holds Q rows, which this call never writes)
    s.e = eval_upload(plan, Q, 2 * l.k);
    s.alphas = r.sweep_alphas.p; s.num_alphas = static_cast<int>(A); s.depth = sw.depth;
    s.table = r.sweep_table.p; s.total_queries = Q;
    for (int64_t q0 = 0; q0 < Q; q0 += kRankChunk) {
        const int64_t qn = std::min(kRankChunk, Q - q0);
        s.f = ensemble_upload(l, q0, qn, sw.normalizer);
        s.e.q0 = q0;
        { RankProf scope(prof, "fuse_sweep", stream_); launch_fuse_sweep(s, static_cast<int>(qn), stream_); }
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));      // (the next round's lists overwrite this one's)
    }
    NVSM_HIP_CHECK(hipMemcpy(table, r.sweep_table.p, cells * sizeof(double), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < Q; ++i) {      // a query without words gets all zeros, as in nvsm_evaluate
        if (q.offsets[i + 1] != q.offsets[i]) continue;
        for (int64_t a = 0; a < A; ++a) std::fill(table + (a * Q + i) * plan.width, table + (a * Q + i + 1) * plan.width, 0.0);
    }
    raise_device_error();
}

void Model::ensemble_sweep(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                           const nvsm_sweep_options& sw, const nvsm_judgments& j, double* table) {
    EvalPlan plan;
    sweep_check(q, opt, lex, fb, sw, j, table, plan);
    EnsembleLists l;
    ensemble_lists(q, opt, lex, fb, l);
    sweep_rounds(q, l, sw, plan, table);
}

// the k-fold choice: a pure host function of the sweep table (DESIGN.md §17 "Selection"; declared in model.h)
void cv_select(const double* table, int64_t A, int64_t Q, int width, int measure, const float* alphas, const int32_t* fold_of, int F,
               float* fold_alpha, double* fold_train, int* fold_index) {
    for (int f = 0; f < F; ++f) {
        int64_t held = 0;
        for (int64_t i = 0; i < Q; ++i) held += fold_of[i] == f;
        fold_index[f] = -1;
        if (held == 0) { fold_alpha[f] = std::nanf(""); fold_train[f] = 0.0; continue; }
        const double n_train = static_cast<double>(Q - held);
        double best = 0.0;
        for (int64_t a = 0; a < A; ++a) {
            double sum = 0.0;      // ascending query index, plain sequential additions, one division
            for (int64_t i = 0; i < Q; ++i)
                if (fold_of[i] != f) sum += table[(a * Q + i) * width + measure];
            const double mean = sum / n_train;
            // Python's max() over (value, alpha) tuples: the larger value, on a tie the larger alpha
            if (fold_index[f] < 0 || mean > best || (mean == best && alphas[a] > alphas[fold_index[f]])) { best = mean; fold_index[f] = static_cast<int>(a); }
        }
        fold_alpha[f] = alphas[fold_index[f]];
        fold_train[f] = best;
    }
}

void Model::rank_ensemble_cv(const nvsm_queries& q, const nvsm_rank_options& opt, const nvsm_lexical_options& lex, const nvsm_feedback_options* fb,
                             const nvsm_sweep_options& sw, const nvsm_cv_options& cv, const nvsm_judgments& j, float* fold_alpha,
                             double* fold_train_measure, int64_t* doc_ids, float* scores, int64_t* counts, double* metrics, double* sweep_metrics) {
    const int64_t Q = q.num_queries;
    EvalPlan plan;
    double none = 0.0;            // (eval_plan asks for a pointer; the table's size is known behind the checks)
    sweep_check(q, opt, lex, fb, sw, j, sweep_metrics ? sweep_metrics : &none, plan);
    const int F = cv.num_folds;
    if (F < 2 || F > Q) throw Error(NVSM_ERR_INVALID_ARGUMENT, "cv->num_folds must be in [2, num_queries]");
    if (cv.measure < 0 || cv.measure >= plan.width) throw Error(NVSM_ERR_INVALID_ARGUMENT, "cv->measure is no column of the metric row");
    if (cv.measure == NVSM_EVAL_NUM_RET || cv.measure == NVSM_EVAL_NUM_REL || cv.measure == NVSM_EVAL_NUM_REL_RET)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "cv->measure: num_ret, num_rel and num_rel_ret are not offered as training measures");
    std::vector<int32_t> fold(static_cast<size_t>(Q));
    if (cv.fold_of) {
        std::vector<int64_t> size(static_cast<size_t>(F), 0);
        for (int64_t i = 0; i < Q; ++i) {
            if (cv.fold_of[i] < 0 || cv.fold_of[i] >= F) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a cv->fold_of entry is outside [0, num_folds)");
            fold[static_cast<size_t>(i)] = cv.fold_of[i];
            ++size[static_cast<size_t>(cv.fold_of[i])];
        }
        for (int f = 0; f < F; ++f)
            if (size[static_cast<size_t>(f)] == Q) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a fold holds every query: its training set is empty");
    } else {      // sklearn's un-shuffled KFold: contiguous, the first Q % F folds one query longer
        int64_t i = 0;
        for (int f = 0; f < F; ++f)
            for (int64_t c = Q / F + (f < Q % F ? 1 : 0); c > 0; --c) fold[static_cast<size_t>(i++)] = f;
    }
    const int64_t A = sw.num_alphas;
    std::vector<double> own;      // the table, where the caller does not want it
    if (!sweep_metrics) {
        own.resize(static_cast<size_t>(A) * Q * plan.width);
        sweep_metrics = own.data();
    }
    EnsembleLists l;
    ensemble_lists(q, opt, lex, fb, l);
    sweep_rounds(q, l, sw, plan, sweep_metrics);
    std::vector<int> index(static_cast<size_t>(F));
    cv_select(sweep_metrics, A, Q, plan.width, cv.measure, sw.alphas, fold.data(), F, fold_alpha, fold_train_measure, index.data());
    std::vector<float> query_alpha(static_cast<size_t>(Q));
    for (int64_t i = 0; i < Q; ++i) query_alpha[static_cast<size_t>(i)] = fold_alpha[fold[static_cast<size_t>(i)]];
    fuse_rounds(q, l, sw.normalizer, 0.f, query_alpha.data(), nullptr, doc_ids, scores, counts);
    if (metrics)      // the returned lists cut at depth: by definition the sweep's rows at the chosen alphas
        for (int64_t i = 0; i < Q; ++i) {
            const int64_t a = index[static_cast<size_t>(fold[static_cast<size_t>(i)])];
            std::copy(sweep_metrics + (a * Q + i) * plan.width, sweep_metrics + (a * Q + i + 1) * plan.width, metrics + i * plan.width);
        }
}

// ---- nearest neighbours (include/cunvsm_amd.h nvsm_neighbors / nvsm_similarity) ---------------------------------
// The searched matrix is a pointer, a row count and a dimension: W or E directly (through their LazyView), or, for the projected
// vocabulary, a scratch slab that is produced with the query side's own kernels right before it is scanned. Rounds, slabs,
// selection, sort and write are nvsm_rank's.
namespace {
constexpr int64_t kProjSlabBytes = int64_t(64) << 20;       // one slab of the projected vocabulary
constexpr int64_t kProjChunk = 16384;                       // words gathered and projected per launch group
constexpr int64_t kPairChunk = 2048;                        // pairs per round of nvsm_similarity
bool known_space(int s) { return s == NVSM_SPACE_WORDS || s == NVSM_SPACE_PROJECTED_WORDS || s == NVSM_SPACE_ENTITIES; }
}  // namespace

Model::RowSpace Model::row_space(int space) const {
    if (space == NVSM_SPACE_WORDS) return RowSpace{words_.P.p, cfg_.num_words, cfg_.word_repr_size, &words_};
    if (space == NVSM_SPACE_ENTITIES) return RowSpace{ents_.P.p, cfg_.num_entities, cfg_.entity_repr_size, &ents_};
    return RowSpace{nullptr, cfg_.num_words, cfg_.entity_repr_size, nullptr};
}

// out [n][de] = f(T·W[id] + c·b) for the words ids_dev[0 .. n) (null: first, first + 1, ...): the query side of nvsm_rank with
// one word per query — launch_rank_query_mean (which applies the words table's lazy view), launch_gemm, launch_rank_bias_act
void Model::project_words(const int64_t* ids_dev, int64_t first, int64_t n, float c, int act, float* out) {
    const int dw = cfg_.word_repr_size, de = cfg_.entity_repr_size;
    RankScratch& r = rank_;
    grow(r.offsets, static_cast<size_t>(kProjChunk) + 1);
    grow(r.phrase, static_cast<size_t>(kProjChunk) * dw);
    std::vector<int64_t> iota(static_cast<size_t>(kProjChunk) + 1);
    for (size_t i = 0; i < iota.size(); ++i) iota[i] = static_cast<int64_t>(i);
    NVSM_HIP_CHECK(hipMemcpy(r.offsets.p, iota.data(), iota.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (!ids_dev) grow(r.ids, static_cast<size_t>(kProjChunk));
    for (int64_t i0 = 0; i0 < n; i0 += kProjChunk) {
        const int64_t cn = std::min(kProjChunk, n - i0);
        const int64_t* ids = ids_dev ? ids_dev + i0 : r.ids.p;
        if (!ids_dev) {
            for (int64_t i = 0; i < cn; ++i) iota[static_cast<size_t>(i)] = first + i0 + i;
            NVSM_HIP_CHECK(hipMemcpyAsync(r.ids.p, iota.data(), static_cast<size_t>(cn) * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
            NVSM_HIP_CHECK(hipStreamSynchronize(stream_));      // (`iota` is rewritten by the next chunk)
        }
        RankProf scope(prof, "nbr_project", stream_);
        launch_rank_query_mean(words_.P.p, dw, cfg_.num_words, ids, nullptr, r.offsets.p, cn, r.phrase.p, lazy_view(words_), err_host_, stream_);
        float* y = out + static_cast<size_t>(i0) * de;
        launch_gemm(0, 0, r.phrase.p, T_.p, y, static_cast<int>(cn), de, dw, dw, de, de, 1.f, nullptr, 1, 0, stream_);
        launch_rank_bias_act(y, b_.p, c, act, cn, de, stream_);
    }
}

// the refusals of a nvsm_neighbor_queries against a searched space of dimension `dim`, in nvsm_neighbors' order
void Model::neighbor_queries_check(const nvsm_neighbor_queries& q, int dim) const {
    const int64_t Q = q.num_queries;
    if (Q < 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "num_queries is negative");
    if ((q.ids != nullptr) == (q.vectors != nullptr)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "queries: exactly one of ids and vectors must be given");
    if (q.ids) {
        if (!known_space(q.source_space)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown source space");
        const RowSpace src = row_space(q.source_space);
        if (src.dim != dim) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the source space's dimension differs from the searched space's");
        for (int64_t i = 0; i < Q; ++i)
            if (q.ids[i] < 0 || q.ids[i] >= src.count) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a query row id is outside the source space");
    } else if (q.dim != dim) {
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "queries->dim differs from the searched space's dimension");
    }
}

// a round's query panel rank_.panel [qn][dim] from the queries q0 .. q0 + qn of the call — host vectors, gathered rows of a table
// (through its lazy view) or projected words (c, act) — and its inverse norms rank_.qinv
void Model::neighbor_panel(const nvsm_neighbor_queries& q, int64_t q0, int64_t qn, int dim, float c, int act, int cosine) {
    RankScratch& r = rank_;
    grow(r.panel, static_cast<size_t>(kRankChunk) * dim);
    grow(r.ids, static_cast<size_t>(kInferChunk));
    grow(r.qinv, static_cast<size_t>(kInferChunk));
    if (q.ids) NVSM_HIP_CHECK(hipMemcpy(r.ids.p, q.ids + q0, static_cast<size_t>(qn) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (q.vectors) {
        NVSM_HIP_CHECK(hipMemcpy(r.panel.p, q.vectors + q0 * dim, static_cast<size_t>(qn) * dim * sizeof(float), hipMemcpyHostToDevice));
    } else if (q.source_space == NVSM_SPACE_PROJECTED_WORDS) {
        project_words(r.ids.p, 0, qn, c, act, r.panel.p);
    } else {
        const RowSpace src = row_space(q.source_space);
        RankProf scope(prof, "nbr_gather", stream_);
        launch_rank_gather_rows(src.rows, dim, r.ids.p, 0, qn, r.panel.p, lazy_view(*src.table), stream_);
    }
    { RankProf scope(prof, "nbr_gather", stream_); launch_rank_query_norm(r.panel.p, qn, dim, r.qinv.p, cosine, stream_); }
}

void Model::neighbors(const nvsm_neighbor_queries& q, const nvsm_neighbor_options& opt, int64_t* ids, float* scores, int64_t* counts) {
    if (!known_space(opt.space)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown space");
    check_similarity(opt.similarity);
    check_activation(opt.activation);
    if (!std::isfinite(opt.bias_coefficient)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "bias_coefficient is not finite");
    const RowSpace sp = row_space(opt.space);
    const int64_t R = sp.count, Q = q.num_queries;
    const int dim = sp.dim;
    neighbor_queries_check(q, dim);
    if (opt.exclude_self && !(q.ids && q.source_space == opt.space))
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "exclude_self needs queries given as row ids of the searched space");
    check_top_k(opt.top_k, R, "top_k must be in [1, rows of the searched space]");
    check_row_count(R, "neighbour search supports fewer than 2^31 rows");
    const int k = opt.top_k;
    const int cosine = opt.similarity == NVSM_SIM_COSINE;
    const int act = opt.activation == NVSM_ACT_MODEL ? cfg_.nonlinearity : opt.activation;
    const bool exclude = opt.exclude_self != 0;
    const int64_t n_out = exclude ? R - 1 : R;               // rows a query can retrieve
    const int64_t proj_rows = std::max<int64_t>(kSlabAlign, kProjSlabBytes / (static_cast<int64_t>(dim) * 4) / kSlabAlign * kSlabAlign);
    rank_join();
    RankScratch& r = rank_;
    LazyView none{};
    none.stamp = nullptr;
    const LazyView view = sp.table ? lazy_view(*sp.table) : none;

    for (int64_t q0 = 0; q0 < Q;) {
        const RankLayout l = rank_layout(R, k, Q - q0, score_floats(), sp.rows ? 0 : proj_rows);      // (a projected slab is scratch of its own)
        const int64_t qn = l.qn;
        // ---- the round's query panel [qn][dim]
        const int64_t* self = nullptr;
        if (exclude) {      // (a copy of its own: r.ids serves project_words' identity lists further down)
            grow(r.self, static_cast<size_t>(2 * kPairChunk));
            NVSM_HIP_CHECK(hipMemcpy(r.self.p, q.ids + q0, static_cast<size_t>(qn) * sizeof(int64_t), hipMemcpyHostToDevice));
            self = r.self.p;
        }
        neighbor_panel(q, q0, qn, dim, opt.bias_coefficient, act, cosine);
        round_grow(l, k);
        round_slabs(l, R, k, [&](int64_t d0, int Ss) {
            const float* rows = sp.rows;
            int64_t begin = d0;
            if (!sp.rows) {      // this slab of the projected vocabulary, then scanned as rows 0 .. Ss of the scratch
                grow(r.pslab, static_cast<size_t>(l.S) * dim);
                project_words(nullptr, d0, Ss, opt.bias_coefficient, act, r.pslab.p);
                rows = r.pslab.p;
                begin = 0;
            }
            RankProf scope(prof, "nbr_scan", stream_);
            prof.note(nbr_scan_uses_mfma(dim) ? "nbr_scan_mfma" : "nbr_scan_plain");
            launch_nbr_scan(rows, dim, begin, Ss, r.panel.p, static_cast<int>(qn), r.qinv.p, r.scores.p, l.ld, cosine, view, stream_);
            if (self) launch_rank_exclude_self(r.scores.p, l.ld, d0, Ss, self, static_cast<int>(qn), stream_);
        });
        round_sort(l, [&] {
            launch_rank_write(r.keys.p, l.npad, static_cast<int>(qn), k, nullptr, std::min<int64_t>(l.n_keys, n_out), r.out_ids.p, r.out_scores.p,
                              r.out_counts.p, stream_);
        });
        round_results(q0, qn, k, ids, scores, counts);
        q0 += qn;
    }
    raise_device_error();
}

// ---- n-grams of terms in document space (include/cunvsm_amd.h nvsm_ngram_search; kernel: ngram.hip) ---------------
// TermBruteforcer (base.py:106-162) up to 2-grams. G = T·W[S] is made once per call with project_words (c = 0, identity: the words
// table's lazy view applies as it does to the projected vocabulary); a slab of phrase rows is generated from G into the projected
// slab's scratch and scanned there. Rounds, slabs, selection, sort and write are nvsm_neighbors'.
namespace {
// (a, b) of phrase row p >= m over m words: the run of a begins at a·(2m − a − 1)/2 behind the 1-grams
void ngram_pair_of_row(int64_t p, int64_t m, int64_t* a_out, int64_t* b_out) {
    const int64_t t = p - m;
    auto start = [m](int64_t a) { return a * (2 * m - a - 1) / 2; };
    const double w = static_cast<double>(2 * m - 1);
    int64_t a = static_cast<int64_t>((w - std::sqrt(w * w - 8.0 * static_cast<double>(t))) * 0.5);
    a = std::max<int64_t>(0, std::min(a, m - 2));
    while (a > 0 && start(a) > t) --a;
    while (a < m - 2 && start(a + 1) <= t) ++a;
    *a_out = a;
    *b_out = a + 1 + (t - start(a));
}
}  // namespace

void Model::ngram_search(const nvsm_neighbor_queries& q, const nvsm_ngram_options& opt, int64_t* phrase_rows, int64_t* terms, float* scores,
                         int64_t* counts) {
    const int de = cfg_.entity_repr_size;
    const int64_t V = cfg_.num_words, Q = q.num_queries;
    if (opt.max_cardinality != 1 && opt.max_cardinality != 2) throw Error(NVSM_ERR_INVALID_ARGUMENT, "max_cardinality must be 1 or 2");
    check_similarity(opt.similarity);
    check_activation(opt.activation);
    if (!std::isfinite(opt.bias_coefficient)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "bias_coefficient is not finite");
    const int64_t* S = opt.vocabulary;
    if (S) {
        if (opt.vocabulary_size < 1) throw Error(NVSM_ERR_INVALID_ARGUMENT, "vocabulary_size must be at least 1");
        for (int64_t i = 0; i < opt.vocabulary_size; ++i) {
            if (S[i] < 0 || S[i] >= V) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a vocabulary word id is outside [0, num_words)");
            if (i > 0 && S[i] <= S[i - 1]) throw Error(NVSM_ERR_INVALID_ARGUMENT, "the vocabulary must be strictly ascending");
        }
    }
    const int64_t m = S ? opt.vocabulary_size : V;
    const int card = opt.max_cardinality;
    const int64_t R = ngram_row_count(m, card);
    if (R < 0) throw Error(NVSM_ERR_UNSUPPORTED, "n-gram search supports fewer than 2^31 phrase rows: at most 65535 words for 2-grams");
    neighbor_queries_check(q, de);
    check_top_k(opt.top_k, R, "top_k must be in [1, rows of the phrase stack (nvsm_ngram_rows)]");
    const int k = opt.top_k;
    const int cosine = opt.similarity == NVSM_SIM_COSINE;
    const int act = opt.activation == NVSM_ACT_MODEL ? cfg_.nonlinearity : opt.activation;
    const int64_t proj_rows = std::max<int64_t>(kSlabAlign, kProjSlabBytes / (static_cast<int64_t>(de) * 4) / kSlabAlign * kSlabAlign);
    rank_join();
    RankScratch& r = rank_;
    LazyView none{};
    none.stamp = nullptr;
    // ---- G [m][de] = T·W[S], whole: what every phrase row of the call is made from
    grow(r.ngram_g, static_cast<size_t>(m) * de);
    if (S) {
        grow(r.ngram_vocab, static_cast<size_t>(m));
        NVSM_HIP_CHECK(hipMemcpy(r.ngram_vocab.p, S, static_cast<size_t>(m) * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    project_words(S ? r.ngram_vocab.p : nullptr, 0, m, 0.f, NVSM_ACT_IDENTITY, r.ngram_g.p);

    for (int64_t q0 = 0; q0 < Q;) {
        const RankLayout l = rank_layout(R, k, Q - q0, score_floats(), proj_rows);
        const int64_t qn = l.qn;
        neighbor_panel(q, q0, qn, de, opt.bias_coefficient, act, cosine);
        round_grow(l, k);
        round_slabs(l, R, k, [&](int64_t p0, int Ss) {
            grow(r.pslab, static_cast<size_t>(l.S) * de);
            {
                RankProf scope(prof, "ngram_rows", stream_);
                launch_ngram_rows(r.ngram_g.p, static_cast<int>(m), de, b_.p, opt.bias_coefficient, act, p0, Ss, r.pslab.p, stream_);
            }
            RankProf scope(prof, "ngram_scan", stream_);
            prof.note(nbr_scan_uses_mfma(de) ? "ngram_scan_mfma" : "ngram_scan_plain");
            launch_nbr_scan(r.pslab.p, de, 0, Ss, r.panel.p, static_cast<int>(qn), r.qinv.p, r.scores.p, l.ld, cosine, none, stream_);
        });
        round_sort(l, [&] {
            launch_rank_write(r.keys.p, l.npad, static_cast<int>(qn), k, nullptr, std::min<int64_t>(l.n_keys, R), r.out_ids.p, r.out_scores.p,
                              r.out_counts.p, stream_);
        });
        round_results(q0, qn, k, phrase_rows, scores, counts);
        q0 += qn;
    }
    raise_device_error();
    // ---- the words of every returned row: positions in S by the row formula, then model word ids
    for (int64_t i = 0; i < Q * k; ++i) {
        int64_t* t = terms + i * card;
        const int64_t p = phrase_rows[i];
        int64_t a = -1, b = -1;
        if (p >= m) ngram_pair_of_row(p, m, &a, &b);
        else if (p >= 0) a = p;
        t[0] = a < 0 ? -1 : (S ? S[a] : a);
        if (card == 2) t[1] = b < 0 ? -1 : (S ? S[b] : b);
    }
}

void Model::similarity(int space, const int64_t* a, const int64_t* b, int64_t n, int similarity, float* out) {
    if (!known_space(space)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown space");
    check_similarity(similarity);
    if (n < 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "n is negative");
    const RowSpace sp = row_space(space);
    for (int64_t i = 0; i < n; ++i)
        if (a[i] < 0 || a[i] >= sp.count || b[i] < 0 || b[i] >= sp.count) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a row id is outside the space");
    rank_join();
    RankScratch& r = rank_;
    const int cosine = similarity == NVSM_SIM_COSINE;
    LazyView none{};
    none.stamp = nullptr;
    grow(r.ids, static_cast<size_t>(kInferChunk));
    grow(r.self, static_cast<size_t>(2 * kPairChunk));
    grow(r.pair_out, static_cast<size_t>(kPairChunk));
    if (!sp.rows) {      // where the projected rows of a round's pairs lie in the panel: a at i, b at cn + i
        std::vector<int64_t> pos(static_cast<size_t>(2 * kPairChunk));
        for (size_t i = 0; i < pos.size(); ++i) pos[i] = static_cast<int64_t>(i);
        NVSM_HIP_CHECK(hipMemcpy(r.self.p, pos.data(), pos.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    for (int64_t i0 = 0; i0 < n; i0 += kPairChunk) {
        const int64_t cn = std::min(kPairChunk, n - i0);
        // r.ids = [a | b] of the round
        NVSM_HIP_CHECK(hipMemcpy(r.ids.p, a + i0, static_cast<size_t>(cn) * sizeof(int64_t), hipMemcpyHostToDevice));
        NVSM_HIP_CHECK(hipMemcpy(r.ids.p + cn, b + i0, static_cast<size_t>(cn) * sizeof(int64_t), hipMemcpyHostToDevice));
        if (sp.rows) {
            RankProf scope(prof, "nbr_pairs", stream_);
            launch_rank_pair_sim(sp.rows, sp.dim, r.ids.p, r.ids.p + cn, cn, r.pair_out.p, cosine, lazy_view(*sp.table), stream_);
        } else {      // both rows of every pair projected (nvsm_rank_options_default's c and activation), then scored where they lie
            grow(r.panel, static_cast<size_t>(2 * kPairChunk) * sp.dim);
            project_words(r.ids.p, 0, 2 * cn, 1.f, cfg_.nonlinearity, r.panel.p);
            RankProf scope(prof, "nbr_pairs", stream_);
            launch_rank_pair_sim(r.panel.p, sp.dim, r.self.p, r.self.p + cn, cn, r.pair_out.p, cosine, none, stream_);
        }
        NVSM_HIP_CHECK(hipMemcpyAsync(out + i0, r.pair_out.p, static_cast<size_t>(cn) * sizeof(float), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    }
    raise_device_error();
}

// ---- exact t-SNE of table rows (include/cunvsm_amd.h nvsm_tsne; kernels: tsne.hip) --------------------------------
// py/visualize.py's sklearn.manifold.TSNE with the exact gradient. The host keeps sklearn's control flow — two phases of
// _gradient_descent, the error every 50th iteration, the stopping rules — and reads two doubles back at every check; everything
// else stays on the device. tsne_pca_start and tsne_descent are free functions so that the test hooks run the same code.
namespace {
// eigenvectors of the symmetric A [d][d] (destroyed; its diagonal ends as the eigenvalues) as the COLUMNS of V: cyclic Jacobi
void jacobi_eigen(std::vector<double>& A, int d, std::vector<double>& V) {
    V.assign(static_cast<size_t>(d) * d, 0.0);
    for (int i = 0; i < d; ++i) V[static_cast<size_t>(i) * d + i] = 1.0;
    double fro = 0.0;
    for (double a : A) fro += a * a;
    for (int sweep = 0; sweep < 100; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < d; ++p)
            for (int q = p + 1; q < d; ++q) off += A[static_cast<size_t>(p) * d + q] * A[static_cast<size_t>(p) * d + q];
        if (off <= 1e-32 * fro) return;
        for (int p = 0; p < d - 1; ++p)
            for (int q = p + 1; q < d; ++q) {
                const double apq = A[static_cast<size_t>(p) * d + q];
                if (apq == 0.0) continue;
                const double theta = (A[static_cast<size_t>(q) * d + q] - A[static_cast<size_t>(p) * d + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < d; ++k) {
                    double* r = &A[static_cast<size_t>(k) * d];
                    const double akp = r[p], akq = r[q];
                    r[p] = c * akp - sn * akq;
                    r[q] = sn * akp + c * akq;
                }
                double* rp = &A[static_cast<size_t>(p) * d];
                double* rq = &A[static_cast<size_t>(q) * d];
                for (int k = 0; k < d; ++k) {
                    const double apk = rp[k], aqk = rq[k];
                    rp[k] = c * apk - sn * aqk;
                    rq[k] = sn * apk + c * aqk;
                }
                for (int k = 0; k < d; ++k) {
                    double* r = &V[static_cast<size_t>(k) * d];
                    const double vkp = r[p], vkq = r[q];
                    r[p] = c * vkp - sn * vkq;
                    r[q] = sn * vkp + c * vkq;
                }
            }
    }
    // cyclic Jacobi converges quadratically (a dozen sweeps at d = 1024); a matrix that is still not diagonal holds non-finite entries
    throw Error(NVSM_ERR_INVALID_ARGUMENT, "PCA initialisation: the covariance of the rows has no eigen-decomposition (non-finite values?)");
}
}  // namespace

void TsneScratch::grow_for(int64_t n, int d) {
    int wc, slabs;
    tsne_force_layout(static_cast<int>(n), &wc, &slabs);
    grow(x, static_cast<size_t>(n) * d);
    grow(p, static_cast<size_t>(n) * tsne_ld(n));
    grow(y, static_cast<size_t>(2 * n)); grow(upd, static_cast<size_t>(2 * n)); grow(gains, static_cast<size_t>(2 * n)); grow(gs, static_cast<size_t>(2 * n));
    grow(part, static_cast<size_t>(n) * slabs * 5);
    grow(rows, static_cast<size_t>(2 * n + 5));
    grow(pca, static_cast<size_t>(d) * (d + 3));
    grow(ids, static_cast<size_t>(n));
}

void tsne_pca_start(const float* X, int n, int d, TsneScratch& w, float* Y0, hipStream_t s) {
    double* mean = w.pca.p;
    double* cov = mean + d;
    double* V = cov + static_cast<size_t>(d) * d;
    launch_tsne_covariance(X, n, d, mean, cov, s);
    std::vector<double> A(static_cast<size_t>(d) * d), vecs;
    NVSM_HIP_CHECK(hipMemcpyAsync(A.data(), cov, A.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    NVSM_HIP_CHECK(hipStreamSynchronize(s));
    jacobi_eigen(A, d, vecs);
    // the two largest eigenvalues (the lower index on a tie); with d = 1 the second axis is zero
    int first = 0, second = -1;
    for (int i = 1; i < d; ++i) if (A[static_cast<size_t>(i) * d + i] > A[static_cast<size_t>(first) * d + first]) first = i;
    for (int i = 0; i < d; ++i) {
        if (i == first) continue;
        if (second < 0 || A[static_cast<size_t>(i) * d + i] > A[static_cast<size_t>(second) * d + second]) second = i;
    }
    std::vector<double> axes(static_cast<size_t>(2) * d, 0.0);
    const int pick[2] = {first, second};
    for (int c = 0; c < 2; ++c) {
        if (pick[c] < 0) continue;
        int big = 0;
        for (int t = 0; t < d; ++t) {
            axes[static_cast<size_t>(c) * d + t] = vecs[static_cast<size_t>(t) * d + pick[c]];
            if (std::fabs(axes[static_cast<size_t>(c) * d + t]) > std::fabs(axes[static_cast<size_t>(c) * d + big])) big = t;
        }
        if (axes[static_cast<size_t>(c) * d + big] < 0.0)
            for (int t = 0; t < d; ++t) axes[static_cast<size_t>(c) * d + t] = -axes[static_cast<size_t>(c) * d + t];
    }
    NVSM_HIP_CHECK(hipMemcpyAsync(V, axes.data(), axes.size() * sizeof(double), hipMemcpyHostToDevice, s));
    launch_tsne_project(X, n, d, mean, V, Y0, s);
    std::vector<float> y(static_cast<size_t>(2) * n);
    NVSM_HIP_CHECK(hipMemcpyAsync(y.data(), Y0, y.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    NVSM_HIP_CHECK(hipStreamSynchronize(s));
    // np.std of column 0 (population), then Y0 / std · 1e-4
    double m = 0.0, var = 0.0;
    for (int i = 0; i < n; ++i) m += static_cast<double>(y[static_cast<size_t>(2) * i]);
    m /= n;
    for (int i = 0; i < n; ++i) { const double c = static_cast<double>(y[static_cast<size_t>(2) * i]) - m; var += c * c; }
    const double sd = std::sqrt(var / n);
    if (!(sd > 0.0) || !std::isfinite(sd))
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "PCA initialisation: the rows have no spread along their first principal axis (all rows identical?)");
    for (float& v : y) v = static_cast<float>(static_cast<double>(v) / sd * 1e-4);
    NVSM_HIP_CHECK(hipMemcpyAsync(Y0, y.data(), y.size() * sizeof(float), hipMemcpyHostToDevice, s));
    NVSM_HIP_CHECK(hipStreamSynchronize(s));
}

namespace {
// sklearn's two-phase _gradient_descent over the device steps of one method (exact: tsne.hip; sparse: tsne_sparse.hip). w holds y, upd,
// gains, gs and rows = rowsum [n] | klrow [n] | total, z, kl, |g|, a z of the check's own. forces(z): the iteration's sums and its Z;
// kl_rows(z, z64, e, klrow): the rows of the error; update(z, e, momentum): the step.
template <typename Forces, typename KlRows, typename Update>
void tsne_descent_loop(TsneScratch& w, int n, const nvsm_tsne_options& opt, int exploration, double* kl, int32_t* n_iter, Profiler* prof,
                       hipStream_t s, Forces forces, KlRows kl_rows, Update update) {
    double* klrow = w.rows.p + n;
    double* z = w.rows.p + 2 * static_cast<size_t>(n) + 1;
    double* out = z + 1;
    const std::vector<float> ones(static_cast<size_t>(2) * n, 1.f);
    double error = std::numeric_limits<double>::max();
    // one _gradient_descent: iterations it0 .. max_iter − 1; returns the index of the last one that ran (it0 − 1: none did)
    auto phase = [&](int it0, int max_iter, float momentum, float exaggeration, int without_progress) {
        NVSM_HIP_CHECK(hipMemsetAsync(w.upd.p, 0, ones.size() * sizeof(float), s));
        NVSM_HIP_CHECK(hipMemcpyAsync(w.gains.p, ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice, s));
        double best_error = std::numeric_limits<double>::max();
        int best_iter = it0, last = it0 - 1;
        for (int i = it0; i < max_iter; ++i) {
            last = i;
            const bool check = (i + 1) % 50 == 0, compute = check || i == max_iter - 1;
            { RankProf scope(prof, "tsne_forces", s); forces(z); }
            if (compute) { RankProf scope(prof, "tsne_kl", s); kl_rows(z, out + 2, exaggeration, klrow); }
            { RankProf scope(prof, "tsne_update", s); update(z, exaggeration, momentum); }
            if (!compute) continue;
            double host[2];
            { RankProf scope(prof, "tsne_kl", s); launch_tsne_check(klrow, w.gs.p, n, out, s); }
            NVSM_HIP_CHECK(hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, s));
            NVSM_HIP_CHECK(hipStreamSynchronize(s));
            error = host[0];
            if (!check) continue;
            if (error < best_error) { best_error = error; best_iter = i; }
            else if (i - best_iter > without_progress) break;
            if (host[1] <= static_cast<double>(opt.min_grad_norm)) break;
        }
        NVSM_HIP_CHECK(hipStreamSynchronize(s));      // (`ones` and `host` are this frame's)
        return last;
    };
    int it = phase(0, exploration, 0.5f, opt.early_exaggeration, 250);
    if (it + 1 < opt.max_iter) it = phase(it + 1, opt.max_iter, 0.8f, 1.f, opt.n_iter_without_progress);
    *kl = error;
    *n_iter = it;
}
}  // namespace

void tsne_descent(TsneScratch& w, int n, const nvsm_tsne_options& opt, float learning_rate, int exploration, double* kl, int32_t* n_iter,
                  Profiler* prof, hipStream_t s) {
    tsne_descent_loop(
        w, n, opt, exploration, kl, n_iter, prof, s, [&](double* z) { launch_tsne_forces(w.p.p, w.y.p, n, w.part.p, z, s); },
        [&](double*, double* z64, float e, double* klrow) { launch_tsne_kl_rows(w.p.p, w.y.p, n, z64, e, klrow, s); },
        [&](double* z, float e, float momentum) {
            launch_tsne_update(w.part.p, n, z, e, momentum, learning_rate, w.y.p, w.upd.p, w.gains.p, w.gs.p, nullptr, s);
        });
}

void Model::tsne_check(const nvsm_tsne_options& opt, int64_t max_rows, const char* too_many, int64_t* n_out) const {
    if (opt.space != NVSM_SPACE_ENTITIES && opt.space != NVSM_SPACE_WORDS)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown space: t-SNE takes the rows of NVSM_SPACE_ENTITIES or NVSM_SPACE_WORDS");
    const RowSpace sp = row_space(opt.space);
    const int64_t n = (!opt.ids && opt.num_rows == 0) ? sp.count : opt.num_rows;
    if (n < 2) throw Error(NVSM_ERR_INVALID_ARGUMENT, "num_rows must be at least 2");
    if (!opt.ids && n > sp.count) throw Error(NVSM_ERR_INVALID_ARGUMENT, "num_rows exceeds the rows of the space");
    if (opt.ids)
        for (int64_t i = 0; i < n; ++i)
            if (opt.ids[i] < 0 || opt.ids[i] >= sp.count) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a row id is outside the space");
    if (n > max_rows) throw Error(NVSM_ERR_UNSUPPORTED, too_many);
    if (!std::isfinite(opt.perplexity) || !(opt.perplexity > 0.f) || !(opt.perplexity < static_cast<float>(n)))
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "perplexity must be finite, positive and below num_rows");
    if (!std::isfinite(opt.early_exaggeration) || !(opt.early_exaggeration > 0.f))
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "early_exaggeration must be finite and positive");
    if (!std::isfinite(opt.learning_rate)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "learning_rate is not finite");
    if (!std::isfinite(opt.min_grad_norm)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "min_grad_norm is not finite");
    if (opt.init == NVSM_TSNE_INIT_GIVEN && opt.init_embedding)
        for (int64_t i = 0; i < 2 * n; ++i)
            if (!std::isfinite(opt.init_embedding[i])) throw Error(NVSM_ERR_INVALID_ARGUMENT, "init_embedding holds a value that is not finite");
    if (opt.max_iter < 1) throw Error(NVSM_ERR_INVALID_ARGUMENT, "max_iter must be at least 1");
    if (opt.n_iter_without_progress < 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "n_iter_without_progress is negative");
    if (opt.init != NVSM_TSNE_INIT_PCA && opt.init != NVSM_TSNE_INIT_GIVEN) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown init");
    if (opt.init == NVSM_TSNE_INIT_GIVEN && !opt.init_embedding)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "NVSM_TSNE_INIT_GIVEN needs init_embedding");
    *n_out = n;
}

void Model::tsne(const nvsm_tsne_options& opt, float* embedding, double* kl_divergence, int32_t* n_iter) {
    int64_t n;
    tsne_check(opt, NVSM_TSNE_MAX_ROWS, "t-SNE supports at most NVSM_TSNE_MAX_ROWS (32768) rows", &n);
    const RowSpace sp = row_space(opt.space);
    const int d = sp.dim, rows = static_cast<int>(n);
    rank_join();
    TsneScratch& w = tsne_;
    w.grow_for(n, d);
    if (opt.ids) NVSM_HIP_CHECK(hipMemcpy(w.ids.p, opt.ids, static_cast<size_t>(n) * sizeof(int64_t), hipMemcpyHostToDevice));
    {
        RankProf scope(prof, "tsne_rows", stream_);
        launch_rank_gather_rows(sp.rows, d, opt.ids ? w.ids.p : nullptr, 0, n, w.x.p, lazy_view(*sp.table), stream_);
        if (opt.l2_normalize) launch_tsne_normalize(w.x.p, rows, d, stream_);
    }
    {
        RankProf scope(prof, "tsne_affinities", stream_);
        launch_tsne_conditionals(w.x.p, rows, d, opt.perplexity, w.p.p, w.rows.p, stream_);
        launch_tsne_joint(w.p.p, rows, w.rows.p, w.rows.p + 2 * n, stream_);
    }
    if (opt.init == NVSM_TSNE_INIT_GIVEN) {
        NVSM_HIP_CHECK(hipMemcpyAsync(w.y.p, opt.init_embedding, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyHostToDevice, stream_));
    } else {
        RankProf scope(prof, "tsne_pca", stream_);
        tsne_pca_start(w.x.p, rows, d, w, w.y.p, stream_);
    }
    // sklearn's learning_rate='auto'
    const float lr = opt.learning_rate > 0.f ? opt.learning_rate : std::max(static_cast<float>(n) / opt.early_exaggeration / 4.f, 50.f);
    tsne_descent(w, rows, opt, lr, std::min(250, opt.max_iter), kl_divergence, n_iter, &prof, stream_);
    NVSM_HIP_CHECK(hipMemcpyAsync(embedding, w.y.p, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    raise_device_error();
}

// ---- sparse-affinity t-SNE (include/cunvsm_amd.h nvsm_tsne_sparse; kernels: tsne_sparse.hip) -----------------------
// sklearn's method='barnes_hut' at angle 0. Neighbour rounds as the retrieval calls run them (a block of query rows against all
// rows, slab by slab, then the selection and the sort of rank.hip); the symmetrisation on index.hip's scan behind two passes of
// the stable pair sort; the descent is tsne_descent's loop over the sparse kernels. Free functions, so the test hooks run them.
void TsneSparseScratch::grow_rows(int64_t n, int d) {
    int wr, tw, ranges;
    tsne_sparse_layout(static_cast<int>(n), forced_ranges, &wr, &tw, &ranges);
    const size_t n2 = static_cast<size_t>(2 * n);
    grow(base.x, static_cast<size_t>(n) * d);
    grow(base.y, n2); grow(base.upd, n2); grow(base.gains, n2); grow(base.gs, n2); grow(attr, n2);
    grow(part, static_cast<size_t>(n) * ranges * 3);
    grow(base.rows, n2 + 5);
    grow(base.pca, static_cast<size_t>(d) * (d + 3));
    grow(base.ids, static_cast<size_t>(n));
    grow(indptr, static_cast<size_t>(n) + 1);
}

void tsne_sparse_knn(const float* X, int n, int d, int k, int64_t round_rows, int64_t score_floats, TsneSparseScratch& w, Profiler* prof,
                     hipStream_t s) {
    grow(w.nbr_id, static_cast<size_t>(n) * k);
    grow(w.nbr_d2, static_cast<size_t>(n) * k);
    for (int64_t q0 = 0; q0 < n;) {
        const int64_t left = round_rows > 0 ? std::min<int64_t>(round_rows, n - q0) : n - q0;
        const RankLayout l = rank_layout(n, k, left, score_floats);
        const int qn = static_cast<int>(l.qn);
        grow(w.scores, static_cast<size_t>(l.qn * l.ld));
        grow(w.sel_ws, rank_select_ws_bytes(qn, static_cast<int>(l.S)));
        grow(w.keys, static_cast<size_t>(l.qn * l.npad));
        int64_t key_off = 0;
        for (int64_t j0 = 0; j0 < n; j0 += l.S) {
            const int Ss = static_cast<int>(std::min<int64_t>(l.S, n - j0));
            { RankProf scope(prof, "tsne_nn_scan", s); launch_tsne_nn_scores(X, n, d, static_cast<int>(q0), qn, static_cast<int>(j0), Ss, w.scores.p, l.ld, s); }
            RankProf scope(prof, "rank_select", s);
            launch_rank_select(w.scores.p, l.ld, Ss, j0, qn, k, w.sel_ws.p, w.keys.p, l.npad, key_off, s);
            key_off += std::min<int64_t>(k, Ss);
        }
        launch_rank_fill_keys(w.keys.p, l.npad, l.n_keys, l.npad, qn, s);
        RankProf scope(prof, "rank_sort", s);
        launch_rank_sort(w.keys.p, l.npad, qn, s);
        launch_tsne_nn_write(w.keys.p, l.npad, qn, k, static_cast<int>(q0), w.nbr_id.p, w.nbr_d2.p, s);
        q0 += qn;
    }
}

void tsne_sparse_affinities(int n, int k, float perplexity, TsneSparseScratch& w, Profiler* prof, hipStream_t s) {
    const int64_t nk = static_cast<int64_t>(n) * k, n2 = 2 * nk;
    double* rowsum = w.base.rows.p;
    double* total = rowsum + 2 * static_cast<size_t>(n);
    grow(w.cond, static_cast<size_t>(nk));
    {
        RankProf scope(prof, "tsne_conditionals", s);
        launch_tsne_nn_conditionals(w.nbr_d2.p, n, k, perplexity, w.cond.p, rowsum, s);
        launch_kmeans_sum(rowsum, n, total, s);
    }
    RankProf scope(prof, "tsne_symmetrize", s);
    // the directed entries by (row, column): the stable sort by column, then by row; a row id has at most 20 bits
    int bits = 1;
    while (bits < 31 && (int64_t(1) << bits) < n) ++bits;
    DevBuf<int> a, b, perm, sums, head;
    DevBuf<int64_t> tok;
    a.alloc(static_cast<size_t>(n2)); b.alloc(static_cast<size_t>(n2)); perm.alloc(static_cast<size_t>(n2));
    {
        DevBuf<int> perm1;
        DevBuf<char> temp;
        perm1.alloc(static_cast<size_t>(n2));
        const size_t temp_bytes = sort_pairs_temp_bytes(n2, bits);
        temp.alloc(temp_bytes, true);
        launch_tsne_sym_keys(w.nbr_id.p, n, k, nullptr, false, a.p, s);
        sort_pairs(temp.p, temp_bytes, nullptr, a.p, b.p, nullptr, perm1.p, n2, bits, nullptr, s);
        launch_tsne_sym_keys(w.nbr_id.p, n, k, perm1.p, true, a.p, s);
        sort_pairs(temp.p, temp_bytes, nullptr, a.p, b.p, perm1.p, perm.p, n2, bits, nullptr, s);      // b: the rows, sorted
        launch_tsne_sym_keys(w.nbr_id.p, n, k, perm.p, false, a.p, s);                                   // a: their columns
        NVSM_HIP_CHECK(hipStreamSynchronize(s));      // (the sort's workspace goes before the matrix comes)
    }
    // heads = entries whose (row, column) differs from their predecessor's: one per stored cell, both directions of an edge merged
    const int64_t tiles = index_tiles(n2);
    sums.alloc(static_cast<size_t>(tiles) + 1);
    launch_index_scan(b.p, a.p, n2, sums.p, s);
    int nnz = 0;
    NVSM_HIP_CHECK(hipMemcpyAsync(&nnz, sums.p + tiles, sizeof(int), hipMemcpyDeviceToHost, s));
    NVSM_HIP_CHECK(hipStreamSynchronize(s));
    w.nnz = nnz;
    head.alloc(static_cast<size_t>(nnz) + 1);
    tok.alloc(static_cast<size_t>(n) + 1);
    grow(w.indices, static_cast<size_t>(nnz));
    grow(w.data, static_cast<size_t>(nnz));
    grow(w.indptr, static_cast<size_t>(n) + 1);
    launch_index_write(b.p, a.p, n2, n, sums.p, head.p, w.indices.p, w.indptr.p, tok.p, s);
    launch_tsne_sym_values(head.p, perm.p, w.cond.p, nnz, n, k, total, w.data.p, s);
    NVSM_HIP_CHECK(hipStreamSynchronize(s));
}

void tsne_sparse_descent(TsneSparseScratch& w, int n, const nvsm_tsne_options& opt, float learning_rate, int exploration, double* kl,
                         int32_t* n_iter, Profiler* prof, hipStream_t s) {
    TsneScratch& b = w.base;
    tsne_descent_loop(
        b, n, opt, exploration, kl, n_iter, prof, s,
        [&](double* z) { launch_tsne_sparse_forces(w.indptr.p, w.indices.p, w.data.p, b.y.p, n, w.forced_ranges, w.attr.p, w.part.p, z, s); },
        [&](double*, double* z64, float e, double* klrow) { launch_tsne_sparse_kl_rows(w.indptr.p, w.indices.p, w.data.p, b.y.p, n, z64, e, klrow, s); },
        [&](double* z, float e, float momentum) {
            launch_tsne_sparse_update(w.attr.p, w.part.p, n, w.forced_ranges, z, e, momentum, learning_rate, b.y.p, b.upd.p, b.gains.p, b.gs.p,
                                      nullptr, s);
        });
}

void Model::tsne_sparse(const nvsm_tsne_options& opt, const nvsm_tsne_sparse_options& sparse, float* embedding, double* kl_divergence,
                        int32_t* n_iter) {
    int64_t n;
    tsne_check(opt, NVSM_TSNE_SPARSE_MAX_ROWS, "sparse t-SNE supports at most NVSM_TSNE_SPARSE_MAX_ROWS (1048576) rows", &n);
    int64_t k = sparse.n_neighbors;
    if (k == 0) {      // TSNE._fit: n_neighbors = min(n_samples - 1, int(3.0 * self.perplexity + 1))
        k = std::min<int64_t>(n - 1, static_cast<int64_t>(3.0 * static_cast<double>(opt.perplexity) + 1.0));
        if (k > NVSM_TSNE_SPARSE_MAX_NEIGHBORS)
            throw Error(NVSM_ERR_UNSUPPORTED, "the perplexity asks for more than NVSM_TSNE_SPARSE_MAX_NEIGHBORS (1024) neighbours");
    } else if (k < 1 || k > std::min<int64_t>(n - 1, NVSM_TSNE_SPARSE_MAX_NEIGHBORS)) {
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "n_neighbors must be in [1, min(num_rows - 1, NVSM_TSNE_SPARSE_MAX_NEIGHBORS)]");
    }
    if (2 * n * k >= (int64_t(1) << 31)) throw Error(NVSM_ERR_UNSUPPORTED, "sparse t-SNE supports fewer than 2^31 directed entries (2 * num_rows * n_neighbors)");
    const RowSpace sp = row_space(opt.space);
    const int d = sp.dim, rows = static_cast<int>(n), kk = static_cast<int>(k);
    rank_join();
    TsneSparseScratch& w = tsne_sparse_;
    w.grow_rows(n, d);
    TsneScratch& b = w.base;
    if (opt.ids) NVSM_HIP_CHECK(hipMemcpy(b.ids.p, opt.ids, static_cast<size_t>(n) * sizeof(int64_t), hipMemcpyHostToDevice));
    {
        RankProf scope(prof, "tsne_rows", stream_);
        launch_rank_gather_rows(sp.rows, d, opt.ids ? b.ids.p : nullptr, 0, n, b.x.p, lazy_view(*sp.table), stream_);
        if (opt.l2_normalize) launch_tsne_normalize(b.x.p, rows, d, stream_);
    }
    tsne_sparse_knn(b.x.p, rows, d, kk, 0, score_floats(), w, &prof, stream_);
    tsne_sparse_affinities(rows, kk, opt.perplexity, w, &prof, stream_);
    if (opt.init == NVSM_TSNE_INIT_GIVEN) {
        NVSM_HIP_CHECK(hipMemcpyAsync(b.y.p, opt.init_embedding, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyHostToDevice, stream_));
    } else {
        RankProf scope(prof, "tsne_pca", stream_);
        tsne_pca_start(b.x.p, rows, d, b, b.y.p, stream_);
    }
    const float lr = opt.learning_rate > 0.f ? opt.learning_rate : std::max(static_cast<float>(n) / opt.early_exaggeration / 4.f, 50.f);
    tsne_sparse_descent(w, rows, opt, lr, std::min(250, opt.max_iter), kl_divergence, n_iter, &prof, stream_);
    NVSM_HIP_CHECK(hipMemcpyAsync(embedding, b.y.p, static_cast<size_t>(2 * n) * sizeof(float), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    raise_device_error();
}

// ---- k-means of table rows (include/cunvsm_amd.h nvsm_kmeans; kernels: kmeans.hip) ---------------------------------
// sklearn's _kmeans_single_lloyd. The host keeps the control flow and reads a few words back per iteration (the number of empty
// clusters behind the sort, then the moved-label count and the centre shift); rows, labels, centres and every sum stay on the
// device. An empty cluster — rare — costs a round trip of the fp64 distances and the labels. The passes are free functions so
// that the test hooks run the same code.
void KmeansScratch::grow_for(int64_t n, int d, int k) {
    const size_t nn = static_cast<size_t>(n), dd = static_cast<size_t>(d), kk = static_cast<size_t>(k);
    grow(x, nn * dd); grow(mean32, dd); grow(xn, nn); grow(dist32, nn);
    grow(c, kk * dd); grow(c2, kk * dd); grow(cc, kk * dd); grow(cn, kk);
    grow(stats, static_cast<size_t>(kmeans_stat_slabs(static_cast<int>(n))) * dd + 2 * dd + 8);
    grow(part, static_cast<size_t>(kmeans_max_chunks(n, k)) * dd);
    grow(shift, kk); grow(dist64, nn); grow(kpp_part, static_cast<size_t>(kmeans_prefix_chunks(n)));
    grow(lab_a, nn); grow(lab_b, nn); grow(sorted_lab, nn); grow(pos, nn);
    grow(start, kk + 1); grow(choff, kk + 1); grow(meta, 4);
    grow(counts, kk); grow(ids, nn);
    if (iota.n < nn) {
        iota.alloc(nn);
        launch_kmeans_iota(iota.p, static_cast<int>(iota.n), nullptr);
        NVSM_HIP_CHECK(hipStreamSynchronize(nullptr));
    }
    const size_t tb = sort_pairs_temp_bytes(n, 31);
    if (sort_temp_bytes < tb) { sort_temp.alloc(tb, true); sort_temp_bytes = tb; }
}

void kmeans_prepare(KmeansScratch& w, int n, int d, hipStream_t s) {
    double* sc = w.scalars(n, d);
    launch_kmeans_colstats(w.x.p, n, d, w.stats.p, w.mean64(n, d), w.mean32.p, w.var(n, d), sc, s);
    launch_kmeans_center_rows(w.x.p, n, d, w.mean32.p, nullptr, w.xn.p, s);
}

void kmeans_assign_pass(KmeansScratch& w, int n, int d, int k, const float* C, int* label, hipStream_t s) {
    launch_kmeans_center_rows(C, k, d, w.mean32.p, w.cc.p, w.cn.p, s);
    launch_kmeans_assign(w.x.p, n, d, w.mean32.p, w.cc.p, w.cn.p, w.xn.p, k, label, w.dist32.p, s);
}

namespace {
// labels sorted (stable: positions ascend inside a label), segment bounds, chunk offsets, counts, the number of empty clusters
int kmeans_sort_segments(KmeansScratch& w, int n, int k, const int* label, hipStream_t s) {
    int bits = 1;
    while (bits < 31 && (int64_t(1) << bits) < k) ++bits;
    sort_pairs(w.sort_temp.p, w.sort_temp_bytes, nullptr, label, w.sorted_lab.p, w.iota.p, w.pos.p, n, bits, nullptr, s);
    launch_kmeans_segments(w.sorted_lab.p, n, k, w.start.p, w.choff.p, w.counts.p, w.meta.p, s);
    int empty = 0;
    NVSM_HIP_CHECK(hipMemcpyAsync(&empty, w.meta.p, sizeof(int), hipMemcpyDeviceToHost, s));
    NVSM_HIP_CHECK(hipStreamSynchronize(s));
    return empty;
}
}  // namespace

int kmeans_update_pass(KmeansScratch& w, int n, int d, int k, int* label, const float* Cold, float* Cnew, bool relocate, hipStream_t s) {
    const int empty = kmeans_sort_segments(w, n, k, label, s);
    if (empty > 0 && relocate) {
        // nvsm_kmeans' rule, on the host: the fp64 distances of the rows to the centres they are assigned to
        launch_kmeans_rowdist(w.x.p, n, d, Cold, label, 0, false, w.dist64.p, nullptr, s);
        std::vector<double> dist(static_cast<size_t>(n));
        std::vector<int> lab(static_cast<size_t>(n));
        std::vector<int64_t> cnt(static_cast<size_t>(k));
        NVSM_HIP_CHECK(hipMemcpyAsync(dist.data(), w.dist64.p, dist.size() * sizeof(double), hipMemcpyDeviceToHost, s));
        NVSM_HIP_CHECK(hipMemcpyAsync(lab.data(), label, lab.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        NVSM_HIP_CHECK(hipMemcpyAsync(cnt.data(), w.counts.p, cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        NVSM_HIP_CHECK(hipStreamSynchronize(s));
        for (int j = 0; j < k; ++j) {
            if (cnt[static_cast<size_t>(j)] != 0) continue;
            int far = -1;
            for (int i = 0; i < n; ++i) {
                if (cnt[static_cast<size_t>(lab[static_cast<size_t>(i)])] < 2) continue;
                if (far < 0 || dist[static_cast<size_t>(i)] > dist[static_cast<size_t>(far)]) far = i;
            }
            if (far < 0) break;      // (k <= n: some cluster has two members while one is empty; only non-finite labels get here)
            --cnt[static_cast<size_t>(lab[static_cast<size_t>(far)])];
            lab[static_cast<size_t>(far)] = j;
            cnt[static_cast<size_t>(j)] = 1;
        }
        NVSM_HIP_CHECK(hipMemcpyAsync(label, lab.data(), lab.size() * sizeof(int), hipMemcpyHostToDevice, s));
        kmeans_sort_segments(w, n, k, label, s);      // (synchronises: `lab` is this frame's)
    }
    launch_kmeans_update(w.x.p, n, d, w.pos.p, w.start.p, w.choff.p, k, w.part.p, Cold, Cnew, w.shift.p, w.scalars(n, d) + 1, s);
    return empty;
}

void kmeans_plusplus(KmeansScratch& w, int n, int d, int k, int64_t seed, float* C, int64_t* rows, hipStream_t s) {
    std::minstd_rand0 gen(static_cast<std::minstd_rand0::result_type>(seed % 2147483647));
    auto draw = [&] { return (static_cast<double>(gen()) - 1.0) / 2147483646.0; };
    double* out = w.scalars(n, d) + 3;
    std::vector<char> chosen(static_cast<size_t>(n), 0);
    int64_t lowest_free = 0;
    for (int t = 0; t < k; ++t) {
        const double u = draw();
        int64_t p;
        if (t == 0) {
            p = std::min<int64_t>(static_cast<int64_t>(std::floor(u * n)), n - 1);
        } else {
            double host[2];
            launch_kmeans_kpp_pick(w.dist64.p, n, w.kpp_part.p, u, out, s);
            NVSM_HIP_CHECK(hipMemcpyAsync(host, out, sizeof(host), hipMemcpyDeviceToHost, s));
            NVSM_HIP_CHECK(hipStreamSynchronize(s));
            p = static_cast<int64_t>(host[1]);
            if (p < 0 || p >= n) {      // total is 0 (or not finite): the lowest position not yet chosen (t < k <= n: there is one)
                while (chosen[static_cast<size_t>(lowest_free)]) ++lowest_free;
                p = lowest_free;
            }
        }
        chosen[static_cast<size_t>(p)] = 1;
        rows[t] = p;
        NVSM_HIP_CHECK(hipMemcpyAsync(C + static_cast<size_t>(t) * d, w.x.p + static_cast<size_t>(p) * d, static_cast<size_t>(d) * sizeof(float),
                                      hipMemcpyDeviceToDevice, s));
        if (t + 1 < k) launch_kmeans_rowdist(w.x.p, n, d, nullptr, nullptr, p, t > 0, w.dist64.p, nullptr, s);
    }
    NVSM_HIP_CHECK(hipStreamSynchronize(s));
}

void Model::kmeans(const nvsm_kmeans_options& opt, int32_t* labels, float* centers, int64_t* counts, float* distances, double* inertia,
                   int32_t* n_iter) {
    if (opt.space != NVSM_SPACE_ENTITIES && opt.space != NVSM_SPACE_WORDS)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown space: k-means takes the rows of NVSM_SPACE_ENTITIES or NVSM_SPACE_WORDS");
    const RowSpace sp = row_space(opt.space);
    const int64_t n = (!opt.ids && opt.num_rows == 0) ? sp.count : opt.num_rows;
    if (n < 1) throw Error(NVSM_ERR_INVALID_ARGUMENT, "num_rows must be at least 1");
    if (!opt.ids && n > sp.count) throw Error(NVSM_ERR_INVALID_ARGUMENT, "num_rows exceeds the rows of the space");
    if (opt.ids)
        for (int64_t i = 0; i < n; ++i)
            if (opt.ids[i] < 0 || opt.ids[i] >= sp.count) throw Error(NVSM_ERR_INVALID_ARGUMENT, "a row id is outside the space");
    if (opt.num_clusters < 1 || opt.num_clusters > n) throw Error(NVSM_ERR_INVALID_ARGUMENT, "num_clusters must be in [1, num_rows]");
    if (opt.num_clusters > NVSM_KMEANS_MAX_CLUSTERS) throw Error(NVSM_ERR_UNSUPPORTED, "k-means supports at most NVSM_KMEANS_MAX_CLUSTERS (4096) clusters");
    if (n >= (int64_t(1) << 31)) throw Error(NVSM_ERR_UNSUPPORTED, "k-means supports fewer than 2^31 rows");
    if (opt.max_iter < 1) throw Error(NVSM_ERR_INVALID_ARGUMENT, "max_iter must be at least 1");
    if (!std::isfinite(opt.tol) || opt.tol < 0.0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "tol must be finite and not negative");
    if (opt.init != NVSM_KMEANS_INIT_PLUSPLUS && opt.init != NVSM_KMEANS_INIT_GIVEN) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown init");
    const int d = sp.dim, rows = static_cast<int>(n), k = opt.num_clusters;
    if (opt.init == NVSM_KMEANS_INIT_GIVEN) {
        if (!opt.init_centers) throw Error(NVSM_ERR_INVALID_ARGUMENT, "NVSM_KMEANS_INIT_GIVEN needs init_centers");
        for (int64_t i = 0; i < static_cast<int64_t>(k) * d; ++i)
            if (!std::isfinite(opt.init_centers[i])) throw Error(NVSM_ERR_INVALID_ARGUMENT, "init_centers holds a value that is not finite");
    } else if (opt.seed < 1) {
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "seed must be at least 1");
    }
    rank_join();
    KmeansScratch& w = kmeans_;
    w.grow_for(n, d, k);
    if (opt.ids) NVSM_HIP_CHECK(hipMemcpy(w.ids.p, opt.ids, static_cast<size_t>(n) * sizeof(int64_t), hipMemcpyHostToDevice));
    {
        RankProf scope(prof, "kmeans_rows", stream_);
        launch_rank_gather_rows(sp.rows, d, opt.ids ? w.ids.p : nullptr, 0, n, w.x.p, lazy_view(*sp.table), stream_);
        if (opt.l2_normalize) launch_tsne_normalize(w.x.p, rows, d, stream_);
        kmeans_prepare(w, rows, d, stream_);
    }
    float* C = w.c.p;
    float* Cnext = w.c2.p;
    if (opt.init == NVSM_KMEANS_INIT_GIVEN) {
        NVSM_HIP_CHECK(hipMemcpyAsync(C, opt.init_centers, static_cast<size_t>(k) * d * sizeof(float), hipMemcpyHostToDevice, stream_));
    } else {
        RankProf scope(prof, "kmeans_plusplus", stream_);
        std::vector<int64_t> chosen(static_cast<size_t>(k));
        kmeans_plusplus(w, rows, d, k, opt.seed, C, chosen.data(), stream_);
    }
    double* sc = w.scalars(rows, d);
    double var_mean = 0.0;
    NVSM_HIP_CHECK(hipMemcpyAsync(&var_mean, sc, sizeof(double), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    const double tol = opt.tol * var_mean;
    int* lab = w.lab_a.p;
    int* lab_old = w.lab_b.p;
    NVSM_HIP_CHECK(hipMemsetAsync(lab_old, 0xFF, static_cast<size_t>(n) * sizeof(int), stream_));      // −1: no row keeps it
    bool strict = false;
    int iterations = 0;
    prof.note(kmeans_assign_uses_mfma(d) ? "kmeans_assign_mfma" : "kmeans_assign_plain");
    for (int it = 0; it < opt.max_iter; ++it) {
        { RankProf scope(prof, "kmeans_assign", stream_); kmeans_assign_pass(w, rows, d, k, C, lab, stream_); }
        double shift = 0.0;
        int moved = 0;
        {
            RankProf scope(prof, "kmeans_update", stream_);
            kmeans_update_pass(w, rows, d, k, lab, C, Cnext, true, stream_);
            NVSM_HIP_CHECK(hipMemsetAsync(w.meta.p + 1, 0, sizeof(int), stream_));
            launch_kmeans_changed(lab, lab_old, rows, w.meta.p + 1, stream_);
            NVSM_HIP_CHECK(hipMemcpyAsync(&moved, w.meta.p + 1, sizeof(int), hipMemcpyDeviceToHost, stream_));
            NVSM_HIP_CHECK(hipMemcpyAsync(&shift, sc + 1, sizeof(double), hipMemcpyDeviceToHost, stream_));
            NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
        }
        std::swap(C, Cnext);
        iterations = it + 1;
        if (moved == 0) { strict = true; break; }
        if (shift <= tol) break;
        if (it + 1 < opt.max_iter) std::swap(lab, lab_old);
    }
    if (!strict) {      // sklearn: one more E-step against the final centres; counts are then plain member counts
        RankProf scope(prof, "kmeans_assign", stream_);
        kmeans_assign_pass(w, rows, d, k, C, lab, stream_);
        kmeans_sort_segments(w, rows, k, lab, stream_);
    }
    {
        RankProf scope(prof, "kmeans_inertia", stream_);
        launch_kmeans_rowdist(w.x.p, rows, d, C, lab, 0, false, w.dist64.p, w.dist32.p, stream_);
        launch_kmeans_sum(w.dist64.p, n, sc + 2, stream_);
    }
    NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    raise_device_error();
    static_assert(sizeof(int) == sizeof(int32_t), "labels are copied out as they are");
    NVSM_HIP_CHECK(hipMemcpyAsync(labels, lab, static_cast<size_t>(n) * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipMemcpyAsync(centers, C, static_cast<size_t>(k) * d * sizeof(float), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipMemcpyAsync(counts, w.counts.p, static_cast<size_t>(k) * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
    if (distances) NVSM_HIP_CHECK(hipMemcpyAsync(distances, w.dist32.p, static_cast<size_t>(n) * sizeof(float), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipMemcpyAsync(inertia, sc + 2, sizeof(double), hipMemcpyDeviceToHost, stream_));
    NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
    *n_iter = iterations;
}

}  // namespace cunvsm
