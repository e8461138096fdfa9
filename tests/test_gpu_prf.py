"""Weighted query likelihood and pseudo-relevance feedback on the GPU against the fp64 restatement of their contract
(tests/prf_reference.py). Each stage is checked on the GPU's own inputs, so that a near-tie of one stage cannot cascade into the next:
A  nvsm_relevance_model against the restatement fed with the GPU's first-pass list;
B  nvsm_lexical_rank_weighted against the restatement of the weighted score;
C  nvsm_lexical_rank_prf has the bits of nvsm_lexical_rank_weighted of the query the restatement expands from the GPU's relevance model;
D  nvsm_rank_ensemble_prf against the fusion restatement fed with nvsm_rank's list and nvsm_lexical_rank_prf's.
At most 1 % of the positions may be open in A and in B at top_k 10 and 100 (tests/test_prf_reference.py checks those shares on the
CPU); at top_k = number of documents the cap is waived — deep in the list the documents that match one weak expansion term crowd
together — and completeness is asserted instead."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import lexical_reference as lr
from tests import prf_reference as pr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_ensemble import REL, ensemble_model, queries_for
from tests.test_gpu_lexical import collection, hand_built, lexical_model
from tests.test_gpu_rank import ADAM_STATE, same_bits

pytestmark = pytest.mark.gpu

V = pr.NUM_WORDS


# ---- the stages' checks ---------------------------------------------------------------------------------------------------------------
def check_model(m, coll, queries, method, param, fb_docs, fb_terms, share=pr.SHARE):
    """stage A for one call; returns (the GPU's term lists, positions open, positions)"""
    d_ids, d_sc, d_n = m.lexical_rank(queries, method=method, param=param, top_k=fb_docs)
    ids, probs, counts = res = m.relevance_model(queries, fb_docs=fb_docs, fb_terms=fb_terms, method=method, param=param)
    assert ids.shape == probs.shape == (len(queries), fb_terms) and counts.shape == (len(queries),)
    assert ids.dtype == np.int64 and probs.dtype == np.float32
    left = total = 0
    for i in range(len(queries)):
        n_docs = int(d_n[i])
        order, pi, bound = pr.relevance_model(coll, d_ids[i, :n_docs], d_sc[i, :n_docs], fb_terms)
        n = order.size
        assert counts[i] == n, (i, counts[i], n)
        assert (ids[i, n:] == -1).all() and np.isneginf(probs[i, n:]).all()
        if n == 0:
            assert n_docs == 0
            continue
        got = ids[i, :n]
        assert got.min() >= 0 and got.max() < coll.num_words and np.unique(got).size == n
        assert (probs[i, :n] > 0).all()
        err = np.abs(probs[i, :n].astype(np.float64) - pi[got])
        assert (err <= bound[got]).all(), (i, float((err / bound[got]).max()))
        if n_docs == 1:                                                    # no exp involved: float32(tf / len) exactly
            np.testing.assert_array_equal(probs[i, :n], pi[got].astype(np.float32))
        tied = probs[i, :n - 1] == probs[i, 1:n]                           # the GPU's own ties: ascending word id
        assert (probs[i, :n - 1] >= probs[i, 1:n]).all() and (got[:-1][tied] < got[1:][tied]).all()
        cand = np.flatnonzero(pi.astype(np.float32) > 0)                   # every candidate, best first: runs may reach past fb_terms
        full = cand[np.lexsort((cand, -pi[cand]))]
        open_ = lr.excused(pi[full], bound[full])[:n]
        differ = got != order
        assert not (differ & ~open_).any(), (i, np.flatnonzero(differ & ~open_)[:5])
        left += int(open_.sum())
        total += n
    assert left <= share * total, (left, total)
    return res, left, total


def check_weighted(result, coll, queries, weights, method, param, top_k, cap=True):
    """stage B for one call: check_ranking's assertions with the weighted bound; cap False: no cap on the open positions, but what
    was left out is nowhere better than the last returned entry by more than the two margins"""
    ids, scores, counts = result
    assert ids.shape == scores.shape == (len(queries), top_k) and counts.shape == (len(queries),)
    left = total = 0
    for i, (q, w) in enumerate(zip(queries, weights)):
        order, ref, bound = pr.weighted_rank_query(coll, q, w, method, param)
        n = min(top_k, order.size)
        assert counts[i] == n, (i, counts[i], n)
        assert (ids[i, n:] == -1).all() and np.isneginf(scores[i, n:]).all()
        if n == 0:
            continue
        got = ids[i, :n]
        assert got.min() >= 0 and np.unique(got).size == n
        assert np.isin(got, order).all()                                   # only matching documents
        err = np.abs(scores[i, :n].astype(np.float64) - ref[got])
        assert (err <= bound[got]).all(), (i, float((err / bound[got]).max()))
        tied = scores[i, :n - 1] == scores[i, 1:n]
        assert (scores[i, :n - 1] >= scores[i, 1:n]).all() and (got[:-1][tied] < got[1:][tied]).all()
        open_ = lr.excused(ref[order], bound[order])[:n]
        differ = got != order[:n]
        assert not (differ & ~open_).any(), (i, np.flatnonzero(differ & ~open_)[:5])
        rest = np.setdiff1d(order, got)                                    # completeness
        if rest.size:
            last = got[-1]
            assert (ref[rest] - bound[rest] <= ref[last] + bound[last]).all(), i
        left += int(open_.sum())
        total += n
    if cap:
        assert left <= pr.SHARE * total, (left, total)
    return left, total


def expansions(coll, queries, model_result, orig_weight):
    """the restatement's RM3 queries from the GPU's relevance model"""
    ids, probs, counts = model_result
    out = [pr.expand(coll, q, ids[i, :counts[i]], probs[i, :counts[i]], orig_weight) for i, q in enumerate(queries)]
    return [e[0] for e in out], [e[1] for e in out]


# ---- seeded collections: one document, fewer than a wave, one slab, three slabs; relevance-model rounds of four queries ---------------
@pytest.mark.parametrize("fb", pr.FEEDBACK)
@pytest.mark.parametrize("documents,queries", pr.CASES)
def test_seeded_collections(documents, queries, fb, monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", "1")                          # V = 20000: five slabs over the vocabulary, four queries a round
    tokens, offsets, qs = lr.case_inputs(documents, queries)
    coll = collection(tokens, offsets, V)
    m = lexical_model(documents, corpus=(tokens, offsets))
    m.profile_enable(True)
    fb_docs, fb_terms = pr.fb_of(documents, fb)
    for method, param in pr.METHODS:
        model, left, total = check_model(m, coll, qs, method, param, fb_docs, fb_terms)
        print("prf A D=%d Q=%d fb=%s %s: %d of %d positions open" % (documents, queries, fb, method, left, total))
        same_bits(model, m.relevance_model(qs, fb_docs=fb_docs, fb_terms=fb_terms, method=method, param=param))
        xq, xw = expansions(coll, qs, model, pr.ORIG_WEIGHT)
        for k in sorted(set(min(k, documents) for k in pr.TOP_KS + (documents,))):
            if k == documents and documents > 1000 and fb != pr.FEEDBACK[-1]:
                continue                                                   # the deepest lists once per collection
            weighted = m.lexical_rank(xq, method=method, param=param, top_k=k, weights=xw)
            left, total = check_weighted(weighted, coll, xq, xw, method, param, k, cap=k < documents or documents < 1000)
            print("prf B D=%d Q=%d fb=%s %s k=%d: %d of %d positions open" % (documents, queries, fb, method, k, left, total))
            prf = m.lexical_rank_prf(qs, fb_docs=fb_docs, fb_terms=fb_terms, orig_weight=pr.ORIG_WEIGHT, method=method, param=param, top_k=k)
            same_bits(prf, weighted)                                       # stage C
            again = k
        same_bits(prf, m.lexical_rank_prf(qs, fb_docs=fb_docs, fb_terms=fb_terms, orig_weight=pr.ORIG_WEIGHT, method=method, param=param,
                                          top_k=again))
    names = set(m.profile())
    assert {"lex_rm", "lex_rm_narrow", "lex_score_weighted", "lex_score"} <= names
    if queries == 300:
        assert "rank_select_radix" in names


def test_unit_and_power_of_two_weights():
    tokens, offsets, qs = lr.case_inputs(1000, 300)
    m = lexical_model(1000, corpus=(tokens, offsets))
    for method, param in pr.METHODS:
        plain = m.lexical_rank(qs, method=method, param=param, top_k=100)
        same_bits(plain, m.lexical_rank(qs, method=method, param=param, top_k=100, weights=[[1.0] * len(q) for q in qs]))
        ids, scores, counts = m.lexical_rank(qs, method=method, param=param, top_k=100, weights=[[0.5] * len(q) for q in qs])
        np.testing.assert_array_equal(ids, plain[0])
        np.testing.assert_array_equal(counts, plain[2])
        np.testing.assert_array_equal(scores, plain[1] * np.float32(0.5))  # a power-of-two scale is exact
    # a weight 0 drops its term: the query without it, bit for bit; all weights 0 retrieve nothing
    long = [q for q in qs if len(q) >= 2][:20]
    dropped = m.lexical_rank(long, top_k=50, weights=[[0.0] + [1.0] * (len(q) - 1) for q in long])
    same_bits(dropped, m.lexical_rank([q[1:] for q in long], top_k=50))
    none = m.lexical_rank(long, top_k=50, weights=[[0.0] * len(q) for q in long])
    assert (none[2] == 0).all() and (none[0] == -1).all() and np.isneginf(none[1]).all()


# ---- the hand-built collection: empty documents, one token, 63 / 64 / 65 tokens, 5000 tokens, exact twins -------------------------------
HAND_QUERIES = [[7], [7, 7], [3, V - 1, 4], [V - 1, V - 2], [], [7, 3, 7, 39, 0], [11, 11, 11]]


@pytest.mark.parametrize("method,param", pr.METHODS)
def test_hand_built_collection(method, param):
    tokens, offsets = hand_built()
    D = offsets.size - 1
    coll = collection(tokens, offsets, V)
    m = lexical_model(D, corpus=(tokens, offsets))
    for fb_docs, fb_terms in ((1, 1), (3, 10), (8, 60)):                  # 40 distinct words in all: fewer than fb_terms = 60
        model, _, _ = check_model(m, coll, HAND_QUERIES, method, param, fb_docs, fb_terms, share=1.0)
        ids, probs, counts = model
        assert counts[3] == 0 and counts[4] == 0                          # only absent terms; no words: no feedback documents
        assert (counts[[0, 1, 2, 5, 6]] > 0).all() and (counts <= 40).all()
        xq, xw = expansions(coll, HAND_QUERIES, model, 0.5)
        assert xq[3] == [] and xq[4] == [] and xq[2][:2] == [3, 4]        # the absent word of query 2 is not part of its expansion
        for k in (1, 3, D):
            weighted = m.lexical_rank(xq, method=method, param=param, top_k=k, weights=xw)
            check_weighted(weighted, coll, xq, xw, method, param, k, cap=False)
            prf = m.lexical_rank_prf(HAND_QUERIES, fb_docs=fb_docs, fb_terms=fb_terms, method=method, param=param, top_k=k)
            same_bits(prf, weighted)
        assert prf[2][3] == 0 and prf[2][4] == 0
        assert not np.isin(prf[0], [0, 6]).any()                          # the empty documents are never retrieved
        # the twins (documents 5 and 7) tie exactly wherever both are returned: ascending id
        for i in range(len(HAND_QUERIES)):
            row = list(prf[0][i])
            if 5 in row and 7 in row:
                assert row.index(5) + 1 == row.index(7) and prf[1][i][row.index(5)] == prf[1][i][row.index(7)]
    # fb_docs 1: the relevance model of the one-token document 1 is word 7 with probability 1
    ids, probs, counts = m.relevance_model([[7]], fb_docs=1, fb_terms=5, method=method, param=param)
    first = m.lexical_rank([[7]], method=method, param=param, top_k=1)[0][0, 0]
    lo, hi = offsets[first], offsets[first + 1]
    tf = np.bincount(tokens[lo:hi], minlength=V)
    want = np.flatnonzero(tf)[np.lexsort((np.flatnonzero(tf), -tf[np.flatnonzero(tf)]))][:5]
    np.testing.assert_array_equal(ids[0, :counts[0]], want)
    np.testing.assert_array_equal(probs[0, :counts[0]], (tf[want] / float(hi - lo)).astype(np.float32))


def test_orig_weight_0_and_1_drop_the_other_group():
    tokens, offsets, qs = lr.case_inputs(1000, 300)
    qs = qs[:40]
    m = lexical_model(1000, corpus=(tokens, offsets))
    # orig_weight 1: the expansion terms weigh 0 and are dropped; the original terms weigh 1 / L each
    prf = m.lexical_rank_prf(qs, orig_weight=1.0, top_k=50)
    coll = collection(tokens, offsets, V)
    kept = [pr.remaining(coll, q) for q in qs]
    same_bits(prf, m.lexical_rank(kept, top_k=50, weights=[[np.float32(1.0 / max(len(q), 1))] * len(q) for q in kept]))
    np.testing.assert_array_equal(prf[2], m.lexical_rank(qs, top_k=50)[2])
    # orig_weight 0: the expansion terms alone
    ids, probs, counts = m.relevance_model(qs)
    xq, xw = expansions(coll, qs, (ids, probs, counts), 0.0)
    assert all((w[:len(k)] == 0).all() for w, k in zip(xw, kept))
    same_bits(m.lexical_rank_prf(qs, orig_weight=0.0, top_k=50),
              m.lexical_rank([q[len(k):] for q, k in zip(xq, kept)], top_k=50, weights=[w[len(k):] for w, k in zip(xw, kept)]))


# ---- stage D --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,normalizer", [(0.5, "standardize"), (0.3, "minmax"), (0.0, "none")])
def test_ensemble_with_feedback(alpha, normalizer):
    from tests import eval_reference as er
    from tests.test_gpu_ensemble import CUTOFFS, METRIC_BOUND
    from tests.test_gpu_eval import judged_list
    D = 300
    m, tokens, offsets = ensemble_model(D)
    rs = np.random.RandomState(3)
    fb = dict(fb_docs=5, fb_terms=8, orig_weight=0.6)
    for Q, k in ((7, 1), (40, 25), (300, 10)):
        qs = queries_for(tokens, Q, Q + k)
        judged = [judged_list(rs, D, (0, 1, 9, 65)[q % 4]) for q in range(Q)]
        a_ids, a_sc, a_n = m.rank(qs, top_k=k)
        b_ids, b_sc, b_n = m.lexical_rank_prf(qs, top_k=k, **fb)
        metrics, ids, scores, counts = m.rank_ensemble(qs, alpha=alpha, normalizer=normalizer, top_k=k, judgments=judged, cutoffs=CUTOFFS,
                                                       feedback=fb)
        left = total = 0
        for i in range(Q):
            r_ids, r_sc = lr.fuse_query(a_ids[i, :a_n[i]], a_sc[i, :a_n[i]], b_ids[i, :b_n[i]], b_sc[i, :b_n[i]], alpha, normalizer)
            n = r_ids.size
            assert counts[i] == n
            assert (ids[i, n:] == -1).all() and np.isneginf(scores[i, n:]).all()
            if n == 0:
                continue
            got = ids[i, :n]
            assert np.array_equal(np.sort(got), np.sort(r_ids))
            ref_of = dict(zip(r_ids.tolist(), r_sc.tolist()))
            narrowed = np.array([ref_of[int(d)] for d in got]).astype(np.float32).astype(np.float64)
            assert (np.abs(scores[i, :n].astype(np.float64) - narrowed) <= REL * np.abs(narrowed)).all(), i
            open_ = lr.excused(r_sc, REL * np.abs(r_sc))
            assert not ((got != r_ids) & ~open_).any(), i
            left += int(open_.sum())
            total += n
        assert left <= lr.SHARE * total, (left, total)
        ref = er.evaluate(ids, counts, judged, CUTOFFS, has_words=[len(q) > 0 for q in qs])
        for name in er.names(CUTOFFS):
            if name in er.INTEGER:
                np.testing.assert_array_equal(metrics[name], ref[name], err_msg=name)
            else:
                assert np.abs(metrics[name] - ref[name]).max() <= METRIC_BOUND, name
        same_bits((ids, scores, counts), m.rank_ensemble(qs, alpha=alpha, normalizer=normalizer, top_k=k, feedback=fb))
        if Q >= 4:
            assert counts[1] == 0 and b_n[2] == 0 and counts[2] == a_n[2] == k      # both lists empty; list B empty: list A alone
    # feedback changes list B, and with it the fusion
    assert not np.array_equal(b_ids, m.lexical_rank(qs, top_k=k)[0])


def test_a_prf_call_between_steps_never_disturbs_training():
    spec = dict(num_words=2000, num_entities=600, word_dim=24, entity_dim=36, window=4, num_random=3, nonlinearity="tanh",
                batch_norm=True, update_method="sparse_adam")
    spec["lambda"] = 0.01
    tokens, offsets = lr.zipf_corpus(3, 600, 2000)
    queries = lr.zipf_queries(4, 20, 2000, tokens)
    models = []
    for _ in range(2):
        m = gpu_model(spec, 64)
        load_params(m, random_params(spec, np.random.RandomState(9)), True)
        m.upload_corpus(ca.Corpus(tokens, offsets))
        models.append(m)
    a, b = models
    rs = np.random.RandomState(10)
    first = None
    for words, ww, labels, iw, ids in [random_batch(spec, rs, 64, zipf=True) for _ in range(4)]:
        for m in (a, b):
            m.step(ca.Batch(words, labels, ww, iw), 5e-3, entity_ids=ids)
        res = a.lexical_rank_prf(queries, top_k=50) + a.relevance_model(queries)      # straight behind nvsm_step
        a.rank_ensemble(queries, top_k=50, feedback=True)
        if first is None:
            first = res
        same_bits(first, res)                                             # a function of corpus and query, not of the parameters
    assert a.rng_state == b.rng_state
    for n in list(PARAMS) + ADAM_STATE:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_call(m, call, top_k=5, fb_docs=3, fb_terms=4, orig_weight=0.5, method=0, param=0.0, words=(1, 2, 3), word_offsets=(0, 2, 3),
             weights=(1.0, 0.5, 2.0), null=None):
    """one of the four calls through the bare ABI, every output pre-filled with -7"""
    L = ca.lib()
    w, off, wt = np.asarray(words, np.int64), np.asarray(word_offsets, np.int64), np.asarray(weights, np.float32)
    Q = off.size - 1
    q = ca.NvsmQueries(w.ctypes.data, None if null == "word_weights" else wt.ctypes.data, None if null == "offsets" else off.ctypes.data, Q)
    lo, fo, ro, eo = ca.NvsmLexicalOptions(), ca.NvsmFeedbackOptions(), ca.NvsmRankOptions(), ca.NvsmEnsembleOptions()
    L.nvsm_lexical_options_default(C.byref(lo))
    L.nvsm_feedback_options_default(C.byref(fo))
    L.nvsm_rank_options_default(C.byref(ro))
    L.nvsm_ensemble_options_default(C.byref(eo))
    lo.method, lo.param, lo.top_k, ro.top_k = method, param, top_k, top_k
    fo.fb_docs, fo.fb_terms, fo.orig_weight = fb_docs, fb_terms, orig_weight
    width = {"weighted": max(top_k, 1), "model": max(fb_terms, 1), "prf": max(top_k, 1), "ensemble": 2 * max(top_k, 1)}[call]
    ids, scores, counts = np.full((Q, width), -7, np.int64), np.full((Q, width), -7.0, np.float32), np.full(Q, -7, np.int64)
    ptr = lambda name, a: None if null == name else a.ctypes.data
    ref = lambda name, s: None if null == name else C.byref(s)
    outs = (ptr("doc_ids", ids), ptr("scores", scores), ptr("counts", counts))
    if call == "weighted":
        st = L.nvsm_lexical_rank_weighted(m._h, ref("queries", q), ref("lex", lo), *outs)
    elif call == "model":
        st = L.nvsm_relevance_model(m._h, ref("queries", q), ref("lex", lo), ref("fb", fo), *outs)
    elif call == "prf":
        st = L.nvsm_lexical_rank_prf(m._h, ref("queries", q), ref("lex", lo), ref("fb", fo), *outs)
    else:
        st = L.nvsm_rank_ensemble_prf(m._h, ref("queries", q), ref("rank_opt", ro), ref("lex", lo), ref("fb", fo), ref("ens", eo), None, None, *outs)
    return st, (ids, scores, counts)


def test_refusals_are_status_codes_and_the_handle_stays_usable():
    tokens, offsets = lr.zipf_corpus(31, 40, 300)
    m = lexical_model(40, num_words=300)
    L = ca.lib()
    for call in ("weighted", "model", "prf", "ensemble"):
        st, out = raw_call(m, call)
        assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error() and all((a == -7).all() for a in out)      # no corpus uploaded
    m.upload_corpus(ca.Corpus(tokens, offsets))
    lexical = [
        (dict(method=2), b"method"), (dict(param=1.0), b"lambda"), (dict(param=float("nan")), b"param"), (dict(method=1, param=-1.0), b"mu"),
        (dict(top_k=0), b"top_k"), (dict(top_k=41), b"top_k"),
        (dict(word_offsets=(0, 3, 2)), b"queries->offsets decrease"), (dict(word_offsets=(1, 2, 3)), b"offsets[0]"),
        (dict(null="queries"), b"null argument: queries"), (dict(null="lex"), b"null argument: lex"),
        (dict(null="doc_ids"), b"null argument: "), (dict(null="scores"), b"null argument: "), (dict(null="counts"), b"null argument: counts"),
        (dict(null="offsets"), b"null argument: queries->offsets"),
    ]
    feedback = [
        (dict(fb_docs=0), b"fb_docs"), (dict(fb_docs=41), b"fb_docs"), (dict(fb_docs=-3), b"fb_docs"),
        (dict(fb_terms=0), b"fb_terms"), (dict(fb_terms=301), b"fb_terms"),
        (dict(orig_weight=-0.1), b"orig_weight"), (dict(orig_weight=1.5), b"orig_weight"), (dict(orig_weight=float("nan")), b"orig_weight"),
        (dict(null="fb"), b"null argument: fb"),
    ]
    weights = [
        (dict(null="word_weights"), b"null argument: queries->word_weights"), (dict(weights=(1.0, -0.5, 1.0)), b"negative"),
        (dict(weights=(1.0, float("inf"), 1.0)), b"not finite"), (dict(weights=(float("nan"), 1.0, 1.0)), b"not finite"),
    ]
    for call, bad in (("weighted", lexical + weights), ("model", lexical + feedback), ("prf", lexical + feedback),
                      ("ensemble", lexical + feedback + [(dict(null="rank_opt"), b"null argument: rank_opt"), (dict(null="ens"), b"null argument: ens")])):
        for kwargs, word in bad:
            st, out = raw_call(m, call, **kwargs)
            assert st == 1 and word in L.nvsm_last_error(), (call, kwargs, L.nvsm_last_error())
            assert all((a == -7).all() for a in out), "nothing was written"
        st, out = raw_call(m, call)
        assert st == 0 and (out[2] >= 0).all(), (call, L.nvsm_last_error())
    # the limits themselves are served
    assert raw_call(m, "model", fb_docs=40, fb_terms=300)[0] == 0
    assert raw_call(m, "prf", orig_weight=0.0)[0] == 0 and raw_call(m, "prf", orig_weight=1.0)[0] == 0
    # a word id out of range: the PRF calls fail behind their first pass and write nothing
    for call in ("model", "prf", "ensemble"):
        st, out = raw_call(m, call, words=(1, 300, 3))
        assert st == 1 and b"num_words" in L.nvsm_last_error() and all((a == -7).all() for a in out)
    # the Python layer refuses what needs no device
    for kwargs in (dict(fb_docs=0), dict(fb_terms=0), dict(orig_weight=1.5)):
        with pytest.raises(ValueError):
            m.lexical_rank_prf([[1]], **kwargs)
    with pytest.raises(ValueError):
        m.lexical_rank([[1, 2]], weights=[[1.0, -1.0]])
    with pytest.raises(ValueError):
        m.lexical_rank([[1, 2]], weights=[[1.0]])
    fresh = lexical_model(40, num_words=300, corpus=(tokens, offsets))      # what the calls allocated is not in the text
    assert m.describe() == fresh.describe()


def test_an_expanded_query_of_more_than_1024_distinct_terms_is_unsupported():
    """document 0 holds the words 0 .. 1029 once each, so with one feedback document every word has probability 1 / 1030 and the three
    expansion terms are the words 0, 1, 2 (ties by ascending id): a query of the words 0 .. 1023 already holds them — 1024 distinct
    terms, served —, a query of the words 3 .. 1026 does not — 1027 distinct terms"""
    tokens = np.concatenate([np.arange(1030), [5000]]).astype(np.int32)
    offsets = np.array([0, 1030, 1031], np.int64)
    m = lexical_model(2, corpus=(tokens, offsets))
    fb = dict(fb_docs=1, fb_terms=3)
    ids, probs, counts = m.relevance_model([list(range(3, 1027))], **fb)
    assert counts[0] == 3 and list(ids[0]) == [0, 1, 2] and (probs[0] == np.float32(1.0 / 1030.0)).all()
    ok = m.lexical_rank_prf([list(range(1024))], top_k=2, **fb)
    assert ok[2][0] == 1 and ok[0][0, 0] == 0
    with pytest.raises(ca.NvsmError) as e:
        m.lexical_rank_prf([list(range(3, 1027))], top_k=2, **fb)
    assert e.value.status == 2 and "distinct terms" in str(e.value)
    with pytest.raises(ca.NvsmError) as e:
        m.rank_ensemble([list(range(3, 1027))], top_k=2, feedback=fb)
    assert e.value.status == 2 and "distinct terms" in str(e.value)
    same_bits(ok, m.lexical_rank_prf([list(range(1024))], top_k=2, **fb))     # the handle stays usable
