// Host side of query inference and top-k document ranking (include/cunvsm_amd.h nvsm_infer / nvsm_rank; kernels: rank.hip).
// Both calls are synchronous. They first wait for the handle's four streams on the host — everything earlier steps queued
// that writes W, E, T or b, the side streams' tails included — and then run on the main stream, so the next step is ordered
// behind them. Lazily decayed tables are read through their LazyView, as the loss kernel and the word gather read them: no
// flush, no stamp moves, and training goes on from exactly the state it was in.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "model.h"

namespace cunvsm {

namespace {

struct RankProf {      // a profiler group around a few launches of the main stream
    Profiler& p; hipStream_t s;
    RankProf(Profiler& p_, const char* name, hipStream_t s_) : p(p_), s(s_) { p.begin(name, s); }
    ~RankProf() { p.end(s); }
};

template <typename T>
void grow(DevBuf<T>& b, size_t count) { if (b.n < count) b.alloc(count); }

constexpr int64_t kInferChunk = 4096;                       // queries projected per launch group
constexpr int64_t kRankChunk = 256;                         // queries scanned together
constexpr int64_t kKeyCount = int64_t(32) << 20;            // sort keys: at most 256 MB (one query's keys may exceed it)
constexpr int64_t kSlabAlign = 4096;                        // rank.hip kSelPart

int64_t pow2_at_least(int64_t n) { int64_t p = 1; while (p < n) p <<= 1; return p; }

}  // namespace

void Model::rank_begin(const nvsm_queries& q, const nvsm_rank_options& opt) {
    if (q.num_queries < 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "num_queries is negative");
    if (!q.offsets) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: queries->offsets");
    if (q.offsets[0] != 0) throw Error(NVSM_ERR_INVALID_ARGUMENT, "queries->offsets[0] must be 0");
    for (int64_t i = 0; i < q.num_queries; ++i)
        if (q.offsets[i + 1] < q.offsets[i]) throw Error(NVSM_ERR_INVALID_ARGUMENT, "queries->offsets decrease");
    if (q.offsets[q.num_queries] > 0 && !q.word_ids) throw Error(NVSM_ERR_INVALID_ARGUMENT, "null argument: queries->word_ids");
    if (q.word_weights) {
        for (int64_t i = 0; i < q.num_queries; ++i) {
            double sum = 0.0;
            for (int64_t j = q.offsets[i]; j < q.offsets[i + 1]; ++j) sum += q.word_weights[j];
            if (q.offsets[i + 1] > q.offsets[i] && !(std::fabs(sum) > 0.0))
                throw Error(NVSM_ERR_INVALID_ARGUMENT, "the word weights of a query sum to zero (np.average: weights sum to zero)");
        }
    }
    const int act = opt.activation;
    if (act != NVSM_ACT_MODEL && act != NVSM_ACT_IDENTITY && act != NVSM_TANH && act != NVSM_HARD_TANH)
        throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown activation");
    if (!std::isfinite(opt.bias_coefficient)) throw Error(NVSM_ERR_INVALID_ARGUMENT, "bias_coefficient is not finite");
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
    // (the main stream is idle here: rank_begin, and every chunk, end with a wait)
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
    rank_begin(q, opt);
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

void Model::rank(const nvsm_queries& q, const nvsm_rank_options& opt, int64_t* doc_ids, float* scores, int64_t* counts) {
    const int64_t D = cfg_.num_entities, Q = q.num_queries;
    const int de = cfg_.entity_repr_size;
    if (opt.similarity != NVSM_SIM_COSINE && opt.similarity != NVSM_SIM_DOT) throw Error(NVSM_ERR_INVALID_ARGUMENT, "unknown similarity");
    if (opt.top_k < 1 || opt.top_k > D) throw Error(NVSM_ERR_INVALID_ARGUMENT, "top_k must be in [1, num_entities]");
    if (D >= (int64_t(1) << 31)) throw Error(NVSM_ERR_UNSUPPORTED, "ranking supports fewer than 2^31 documents");
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
    const int64_t kScoreFloats = static_cast<int64_t>(tune_.rank_slab_mb) * (int64_t(1) << 18);      // score slab: 256 MB unless NVSM_RANK_SLAB_MB says otherwise
    rank_begin(q, opt);
    RankScratch& r = rank_;
    const LazyView view = lazy_view(ents_);

    for (int64_t q0 = 0; q0 < Q;) {
        // ---- how many queries this round, and the layout of their scratch
        int64_t qn = std::min(by_candidates ? kInferChunk : kRankChunk, Q - q0);
        int64_t S = 0, npad = 1, n_keys = 0;
        if (by_candidates) {
            for (;;) {
                int64_t most = 1;
                for (int64_t i = 0; i < qn; ++i) most = std::max(most, cand_off[q0 + i + 1] - cand_off[q0 + i]);
                npad = pow2_at_least(most);
                if (qn * npad <= kKeyCount || qn == 1) break;
                qn = (qn + 1) / 2;
            }
        } else {
            for (;;) {
                S = std::min<int64_t>(D, std::max<int64_t>(kSlabAlign, kScoreFloats / qn / kSlabAlign * kSlabAlign));
                n_keys = 0;
                for (int64_t d0 = 0; d0 < D; d0 += S) n_keys += std::min<int64_t>(k, std::min(S, D - d0));
                npad = pow2_at_least(n_keys);
                if (qn * npad <= kKeyCount || qn == 1) break;
                qn = (qn + 1) / 2;
            }
        }
        rank_project(q, opt, q0, qn);
        grow(r.qinv, static_cast<size_t>(kInferChunk));
        grow(r.keys, static_cast<size_t>(qn * npad));
        grow(r.out_ids, static_cast<size_t>(qn) * k);
        grow(r.out_scores, static_cast<size_t>(qn) * k);
        grow(r.out_counts, static_cast<size_t>(kInferChunk));
        const int64_t* cand_off_dev = nullptr;
        { RankProf scope(prof, "rank_query", stream_); launch_rank_query_norm(r.proj.p, qn, de, r.qinv.p, cosine, stream_); }
        if (by_candidates) {
            const int64_t c0 = cand_off[q0], nc = cand_off[q0 + qn] - c0;
            std::vector<int64_t> off(static_cast<size_t>(qn) + 1);
            for (int64_t i = 0; i <= qn; ++i) off[static_cast<size_t>(i)] = cand_off[q0 + i] - c0;
            grow(r.cand_off, static_cast<size_t>(kInferChunk) + 1);
            grow(r.cand, static_cast<size_t>(std::max<int64_t>(nc, 1)));
            NVSM_HIP_CHECK(hipMemcpyAsync(r.cand_off.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, stream_));
            if (nc > 0) NVSM_HIP_CHECK(hipMemcpyAsync(r.cand.p, cand.data() + c0, static_cast<size_t>(nc) * sizeof(int), hipMemcpyHostToDevice, stream_));
            NVSM_HIP_CHECK(hipStreamSynchronize(stream_));      // (`off` goes out of scope)
            cand_off_dev = r.cand_off.p;
            RankProf scope(prof, "rank_scan", stream_);
            prof.note("rank_scan_candidates");
            launch_rank_scan_candidates(ents_.P.p, de, r.proj.p, r.qinv.p, r.cand.p, r.cand_off.p, static_cast<int>(qn), npad, r.keys.p, cosine, view, stream_);
        } else {
            const int64_t ld = (S + 3) / 4 * 4;                 // rows of the slab start 16-byte aligned (rank.hip rank_keys4)
            grow(r.scores, static_cast<size_t>(qn * ld));
            grow(r.sel_ws, rank_select_ws_bytes(static_cast<int>(qn), static_cast<int>(S)));
            int64_t key_off = 0;
            for (int64_t d0 = 0; d0 < D; d0 += S) {
                const int Ss = static_cast<int>(std::min(S, D - d0));
                {
                    RankProf scope(prof, "rank_scan", stream_);
                    prof.note(rank_scan_uses_mfma(de) ? "rank_scan_mfma" : "rank_scan_plain");
                    launch_rank_scan(ents_.P.p, de, d0, Ss, r.proj.p, static_cast<int>(qn), r.qinv.p, r.scores.p, ld, cosine, view, stream_);
                }
                {
                    RankProf scope(prof, "rank_select", stream_);
                    const bool radix = launch_rank_select(r.scores.p, ld, Ss, d0, static_cast<int>(qn), k, r.sel_ws.p, r.keys.p, npad, key_off, stream_);
                    prof.note(radix ? "rank_select_radix" : "rank_select_all");
                }
                key_off += std::min<int64_t>(k, Ss);
            }
            launch_rank_fill_keys(r.keys.p, npad, n_keys, npad, static_cast<int>(qn), stream_);
        }
        {
            RankProf scope(prof, "rank_sort", stream_);
            const bool global_steps = launch_rank_sort(r.keys.p, npad, static_cast<int>(qn), stream_);
            prof.note(global_steps ? "rank_sort_global" : "rank_sort_lds");
            launch_rank_write(r.keys.p, npad, static_cast<int>(qn), k, cand_off_dev, n_keys, r.out_ids.p, r.out_scores.p, r.out_counts.p, stream_);
        }
        NVSM_HIP_CHECK(hipMemcpyAsync(doc_ids + q0 * k, r.out_ids.p, static_cast<size_t>(qn) * k * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipMemcpyAsync(scores + q0 * k, r.out_scores.p, static_cast<size_t>(qn) * k * sizeof(float), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipMemcpyAsync(counts + q0, r.out_counts.p, static_cast<size_t>(qn) * sizeof(int64_t), hipMemcpyDeviceToHost, stream_));
        NVSM_HIP_CHECK(hipStreamSynchronize(stream_));
        q0 += qn;
    }
    // a query without words retrieves nothing (the reference returns None)
    for (int64_t i = 0; i < Q; ++i) {
        if (q.offsets[i + 1] > q.offsets[i]) continue;
        counts[i] = 0;
        for (int j = 0; j < k; ++j) { doc_ids[i * k + j] = -1; scores[i * k + j] = -INFINITY; }
    }
    raise_device_error();
}

}  // namespace cunvsm
