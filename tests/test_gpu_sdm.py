"""nvsm_sdm_pair_counts, nvsm_sdm_rank and nvsm_rank_ensemble_sdm on the GPU against the fp64 restatement of their contract
(tests/sdm_reference.py): the collection counts equal as integers; the ranking's counts equal, its scores within 2^-23 of the fp64 value,
its ids equal except where the restatement's own neighbouring scores are closer than twice the bound (at most 1 % of the positions:
tests/test_sdm_reference.py checks that share on the CPU), exact ties by ascending id; the same bits from a repeated call and from a
round the driver had to split; training undisturbed; the fused list that of the GPU's own two lists; and every refusal."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import eval_reference as er
from tests import lexical_reference as lr
from tests import sdm_reference as sr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_eval import judged_list
from tests.test_gpu_lexical import lexical_model
from tests.test_gpu_rank import ADAM_STATE, same_bits

pytestmark = pytest.mark.gpu

METHODS = ("jm", "dirichlet")
_positions = {}


def positions(tokens, offsets, num_words):
    """the restatement's view of a collection — with the pair counts and rankings it has worked out —, made once and shared"""
    key = (tokens.tobytes(), offsets.tobytes(), num_words)
    if key not in _positions:
        _positions.clear()
        pos = sr.Positions(lr.Collection(tokens, offsets, num_words))
        pos.rankings = {}
        _positions[key] = pos
    return _positions[key]


def reference(pos, query, method, param, weights, window):
    key = (tuple(int(t) for t in query), method, param, tuple(weights), window)
    if key not in pos.rankings:
        pos.rankings[key] = sr.rank_query(pos, query, method, param, weights, window)
    return pos.rankings[key]


def check_ranking(result, pos, queries, method, param, top_k, weights=sr.DEFAULT_WEIGHTS, window=8, share=lr.SHARE):
    """every assertion of the contract for one call; returns (positions excused, positions, worst score error / bound)"""
    assert hasattr(ca.lib(), "nvsm_sdm_rank")
    ids, scores, counts = result
    assert ids.shape == scores.shape == (len(queries), top_k) and counts.shape == (len(queries),)
    left = total = 0
    worst = 0.0
    for i, q in enumerate(queries):
        order, ref, bound = reference(pos, q, method, param, weights, window)
        n = min(top_k, order.size)
        assert counts[i] == n, (i, counts[i], n)
        assert (ids[i, n:] == -1).all() and np.isneginf(scores[i, n:]).all()
        if n == 0:
            continue
        got = ids[i, :n]
        assert got.min() >= 0 and np.unique(got).size == n
        err = np.abs(scores[i, :n].astype(np.float64) - ref[got])
        assert (err <= bound[got]).all(), (i, q, float((err / np.maximum(bound[got], 1e-300)).max()))
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound[got] > 0, err / bound[got], 0.0))))
        open_ = lr.excused(ref[order], bound[order])[:n]
        differ = got != order[:n]
        assert not (differ & ~open_).any(), (i, q, np.flatnonzero(differ & ~open_)[:5])
        tied = scores[i, :n - 1] == scores[i, 1:n]                        # the GPU's own ties: ascending id
        assert (got[:-1][tied] < got[1:][tied]).all()
        left += int(open_.sum())
        total += n
    assert left <= share * total, (left, total)
    return left, total, worst


# ---- pair counts and ranking on the hand-built collection: every document shape the kernel treats differently -------------------------
@pytest.mark.parametrize("window", sr.WINDOWS)
def test_pair_counts_of_the_hand_built_collection(window, monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", "1")                          # slabs of 4096 documents: documents 4095 and 4096 both match
    assert window <= ca.SDM_MAX_WINDOW and sr.WINDOWS[-1] == ca.SDM_MAX_WINDOW
    tokens, offsets, notes = sr.hand_built(window)
    pos = positions(tokens, offsets, sr.HAND_WORDS)
    m = lexical_model(offsets.size - 1, num_words=sr.HAND_WORDS, corpus=(tokens, offsets))
    queries = sr.HAND_QUERIES + [[int(t) for t in tokens[offsets[notes["long"]]:offsets[notes["long"]] + 300]]]
    want_o, want_u = sr.pair_counts(pos, queries, window)
    got_o, got_u = m.sdm_pair_counts(queries, window=window)
    assert got_o.dtype == got_u.dtype == np.uint64 and got_o.size == sum(max(len(q) - 1, 0) for q in queries)
    np.testing.assert_array_equal(got_o, want_o)
    np.testing.assert_array_equal(got_u, want_u)
    assert want_o[0] > 0 and want_u[0] > want_o[0] and want_u[1] == want_u[0]      # (1, 2) and (2, 1): the unordered count is symmetric
    same_bits((got_o, got_u), m.sdm_pair_counts(queries, window=window))
    # the counts do not depend on what shares the round: every query alone
    at = 0
    for q in queries[:6]:
        n = max(len(q) - 1, 0)
        one_o, one_u = m.sdm_pair_counts([q], window=window)
        np.testing.assert_array_equal(one_o, want_o[at:at + n])
        np.testing.assert_array_equal(one_u, want_u[at:at + n])
        at += n


@pytest.mark.parametrize("window", sr.WINDOWS)
@pytest.mark.parametrize("method", METHODS)
def test_ranking_of_the_hand_built_collection(method, window, monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", "1")
    tokens, offsets, notes = sr.hand_built(window)
    D = offsets.size - 1
    assert D > 4096 + 16
    pos = positions(tokens, offsets, sr.HAND_WORDS)
    m = lexical_model(D, num_words=sr.HAND_WORDS, corpus=(tokens, offsets))
    m.profile_enable(True)
    worst = 0.0
    for k in (1, 10, D):
        res = m.sdm_rank(sr.HAND_QUERIES, method=method, top_k=k, window=window)
        left, total, w = check_ranking(res, pos, sr.HAND_QUERIES, method, None, k, window=window)
        worst = max(worst, w)
        print("sdm hand-built W=%d %s k=%d: %d of %d positions open, worst error %.3g of the bound" % (window, method, k, left, total, w))
    ids, scores, counts = res
    assert counts[7] == 0 and counts[8] == 0                              # no words; only a word that does not occur
    assert not np.isin(ids, [notes["empty0"], notes["empty1"]]).any()
    for name in ("slab_last", "slab_first", "last", "len257", "long"):   # both sides of the slab boundary, the corpus's last document
        assert notes[name] in ids[0], name
    # a one-term query ranks as its T group alone: the order of nvsm_lexical_rank
    np.testing.assert_array_equal(ids[6], m.lexical_rank([[1]], method=method, top_k=D)[0][0])
    assert {"sdm_score", "sdm_collect"} <= set(m.profile())


# ---- seeded Zipf collections: one document, fewer than a wave, one slab, three slabs; one round and two -------------------------------
@pytest.mark.parametrize("documents,queries,top_ks", sr.CASES)
def test_seeded_collections(documents, queries, top_ks, monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", "1")                          # 9001 documents, 256 queries: three slabs of 4096
    tokens, offsets, qs = sr.case_inputs(documents, queries)
    pos = positions(tokens, offsets, sr.NUM_WORDS)
    m = lexical_model(documents, num_words=sr.NUM_WORDS, corpus=(tokens, offsets))
    want_o, want_u = sr.pair_counts(pos, qs, 8)
    got_o, got_u = m.sdm_pair_counts(qs)
    np.testing.assert_array_equal(got_o, want_o)
    np.testing.assert_array_equal(got_u, want_u)
    for k in top_ks:
        for method in METHODS:
            res = m.sdm_rank(qs, method=method, top_k=k)
            left, total, worst = check_ranking(res, pos, qs, method, None, k)
            print("sdm D=%d Q=%d k=%d %s: %d of %d positions open, worst error %.3g of the bound" % (documents, queries, k, method, left, total, worst))
        same_bits(res, m.sdm_rank(qs, method=method, top_k=k))            # a repeated call returns the same bits


def test_explicit_parameters_and_another_window():
    tokens, offsets, qs = sr.case_inputs(1000, 300)
    pos = positions(tokens, offsets, sr.NUM_WORDS)
    m = lexical_model(1000, num_words=sr.NUM_WORDS, corpus=(tokens, offsets))
    for method in METHODS:
        res = m.sdm_rank(qs[:60], method=method, param=lr.EXPLICIT[method], top_k=10, weights=(0.5, 0.3, 0.2), window=3)
        check_ranking(res, pos, qs[:60], method, lr.EXPLICIT[method], 10, weights=(0.5, 0.3, 0.2), window=3)


# ---- weights ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_weights_select_the_groups(method):
    tokens, offsets, qs = sr.case_inputs(1000, 300)
    pos = positions(tokens, offsets, sr.NUM_WORDS)
    m = lexical_model(1000, num_words=sr.NUM_WORDS, corpus=(tokens, offsets))
    k = 50
    # (1, 0, 0): the terms alone, the mean of nvsm_lexical_rank's sum: its order where nothing is nearly tied, its fp64 sum over L
    t_ids, t_sc, t_n = m.sdm_rank(qs, method=method, top_k=k, weights=(1, 0, 0))
    check_ranking((t_ids, t_sc, t_n), pos, qs, method, None, k, weights=(1, 0, 0))
    l_ids, l_sc, l_n = m.lexical_rank(qs, method=method, top_k=k)
    np.testing.assert_array_equal(t_n, l_n)
    compared = 0
    for i, q in enumerate(qs):
        order, ref, bound = lr.rank_query(pos.coll, q, method, None)
        n = min(k, order.size)
        if n == 0:
            continue
        L = sum(1 for t in q if 0 <= t < sr.NUM_WORDS and pos.coll.cf[t] > 0)
        mean = ref / L
        got = t_ids[i, :n]
        assert (np.abs(t_sc[i, :n].astype(np.float64) - mean[got]) <= sr.EPS * np.abs(mean[got])).all(), i
        if not lr.excused(ref[order], bound[order])[:n].any() and not lr.excused(mean[order], sr.EPS * np.abs(mean[order]))[:n].any():
            np.testing.assert_array_equal(got, l_ids[i, :n])
            compared += 1
    assert compared > 0
    # (0, 1, 0): by ordered pairs alone, over the same retrieved set
    o_res = m.sdm_rank(qs, method=method, top_k=1000, weights=(0, 1, 0))
    check_ranking(o_res, pos, qs, method, None, 1000, weights=(0, 1, 0))
    full = m.lexical_rank(qs, method=method, top_k=1000)
    np.testing.assert_array_equal(o_res[2], full[2])
    for i in range(len(qs)):
        np.testing.assert_array_equal(np.sort(o_res[0][i, :o_res[2][i]]), np.sort(full[0][i, :full[2][i]]))


# ---- rounds ----------------------------------------------------------------------------------------------------------------------------
def test_a_round_with_more_distinct_pairs_than_counters_is_split():
    """300 queries of ten words over a vocabulary of 40: the 256 queries of a plain round hold at most 40 distinct terms and more than
    the 1024 distinct pairs a round has counters for, so the rounds are cut by pairs; the result is that of the queries one by one"""
    V = 40
    tokens, offsets = lr.zipf_corpus(77, 1000, V, s=0.5)
    pos = positions(tokens, offsets, V)
    rs = np.random.RandomState(78)
    qs = [[int(t) for t in rs.randint(0, V, 10)] for _ in range(300)]
    assert len({p for q in qs[:256] for p in sr.query_pairs(q)}) > 1024
    m = lexical_model(1000, num_words=V, corpus=(tokens, offsets))
    res = m.sdm_rank(qs, top_k=20)
    check_ranking(res, pos, qs, "jm", None, 20, share=1.0)                # (every document matches every query: no cap on near-ties here)
    for i in (0, 100, 171, 255, 256, 299):
        same_bits([r[i:i + 1] for r in res], m.sdm_rank([qs[i]], top_k=20))
    o, u = m.sdm_pair_counts(qs)
    want_o, want_u = sr.pair_counts(pos, qs, 8)
    np.testing.assert_array_equal(o, want_o)
    np.testing.assert_array_equal(u, want_u)
    # one query alone may hold as many distinct pairs as there are counters, and no more
    walk = [int(t) for t in rs.randint(0, V, 3000)]
    pairs, n = set(), 0
    while len(pairs) < 1024:
        pairs.add((walk[n], walk[n + 1]))
        n += 1
    check_ranking(m.sdm_rank([walk[:n + 1]], top_k=5), pos, [walk[:n + 1]], "jm", None, 5, share=1.0)
    more = n
    while len(pairs) < 1025:
        pairs.add((walk[more], walk[more + 1]))
        more += 1
    with pytest.raises(ca.NvsmError) as e:
        m.sdm_rank([walk[:more + 1]], top_k=5)
    assert e.value.status == 2 and "distinct term pairs" in str(e.value)
    same_bits([r[:1] for r in res], m.sdm_rank([qs[0]], top_k=20))        # the handle stays usable


def test_an_sdm_call_between_steps_never_disturbs_training():
    spec = dict(num_words=300, num_entities=600, word_dim=24, entity_dim=36, window=4, num_random=3, nonlinearity="tanh",
                batch_norm=True, update_method="sparse_adam")
    spec["lambda"] = 0.01
    tokens, offsets = lr.zipf_corpus(3, 600, 300)
    queries = sr.seeded_queries(4, 20, tokens, offsets, 300)
    pos = positions(tokens, offsets, 300)
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
        res = a.sdm_rank(queries, top_k=50) + a.sdm_pair_counts(queries)  # straight behind nvsm_step
        if first is None:
            first = res
        same_bits(first, res)                                             # a function of corpus and query, not of the parameters
    check_ranking(res[:3], pos, queries, "jm", None, 50)
    assert a.rng_state == b.rng_state
    for n in list(PARAMS) + ADAM_STATE:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)


# ---- fusion ----------------------------------------------------------------------------------------------------------------------------
W_NAME, E_NAME, T_NAME, B_NAME = PARAMS
CUTOFFS = (1, 5, 10, 100, 1000)
REL = 2.0 ** -22
METRIC_BOUND = 1e-10          # tests/test_gpu_eval.py's


def fusion_model(D, num_words):
    spec = dict(num_words=num_words, num_entities=D, word_dim=24, entity_dim=36, window=2, num_random=1, nonlinearity="tanh", update_method="sgd")
    rs = np.random.RandomState(D)
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 2).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    m = gpu_model(spec, 8)
    load_params(m, params, True)
    tokens, offsets = lr.zipf_corpus(D, D, num_words)
    m.upload_corpus(ca.Corpus(tokens, offsets))
    return m, tokens, offsets


@pytest.mark.parametrize("alpha,normalizer", [(0.5, "standardize"), (0.3, "minmax"), (1.0, "none"), (0.0, "standardize")])
def test_fusion_with_the_sdm_list(alpha, normalizer):
    D, V = 300, 300
    m, tokens, offsets = fusion_model(D, V)
    m.profile_enable(True)
    rs = np.random.RandomState(int(alpha * 10) + len(normalizer))
    dependence = dict(weights=(0.8, 0.15, 0.05), window=4)
    for Q, k in ((7, 1), (40, 25), (5, D)):
        qs = sr.seeded_queries(Q + k, Q, tokens, offsets, V)
        judged = [judged_list(rs, D, (0, 1, 9, 65)[q % 4]) for q in range(Q)]
        a_ids, a_sc, a_n = m.rank(qs, top_k=k)
        b_ids, b_sc, b_n = m.sdm_rank(qs, top_k=k, **dependence)
        metrics, ids, scores, counts = m.rank_ensemble(qs, alpha=alpha, normalizer=normalizer, top_k=k, judgments=judged, cutoffs=CUTOFFS,
                                                       dependence=dependence)
        assert ids.shape == scores.shape == (Q, 2 * k)
        left = total = 0
        for i in range(Q):
            r_ids, r_sc = lr.fuse_query(a_ids[i, :a_n[i]], a_sc[i, :a_n[i]], b_ids[i, :b_n[i]], b_sc[i, :b_n[i]], alpha, normalizer)
            n = r_ids.size
            assert counts[i] == n == np.union1d(a_ids[i, :a_n[i]], b_ids[i, :b_n[i]]).size
            assert (ids[i, n:] == -1).all() and np.isneginf(scores[i, n:]).all()
            if n == 0:
                continue
            got = ids[i, :n]
            assert np.array_equal(np.sort(got), np.sort(r_ids))
            ref_of = dict(zip(r_ids.tolist(), r_sc.tolist()))
            narrowed = np.array([ref_of[int(d)] for d in got]).astype(np.float32).astype(np.float64)
            assert (np.abs(scores[i, :n].astype(np.float64) - narrowed) <= REL * np.abs(narrowed)).all(), i
            open_ = lr.excused(r_sc, REL * np.abs(r_sc))
            differ = got != r_ids
            assert not (differ & ~open_).any(), (i, np.flatnonzero(differ & ~open_)[:5])
            left += int(open_.sum())
            total += n
        assert left <= lr.SHARE * total, (left, total)
        ref = er.evaluate(ids, counts, judged, CUTOFFS, has_words=[len(q) > 0 for q in qs])
        assert list(metrics) == er.names(CUTOFFS)
        for name in er.names(CUTOFFS):
            if name in er.INTEGER:
                np.testing.assert_array_equal(metrics[name], ref[name], err_msg=name)
            else:
                assert np.abs(metrics[name] - ref[name]).max() <= METRIC_BOUND, name
        # without judgments: the same fused list, bit for bit; and list B really is the sdm list, not the unigram one
        same_bits((ids, scores, counts), m.rank_ensemble(qs, alpha=alpha, normalizer=normalizer, top_k=k, dependence=dependence))
    assert {"fuse_lists", "sdm_score", "rank_eval"} <= set(m.profile()) and "lex_score" not in set(m.profile())
    with pytest.raises(ValueError):
        m.rank_ensemble(qs, dependence=True, feedback=True)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def raw_sdm(m, call="rank", method=0, param=0.0, top_k=5, weights=(0.85, 0.10, 0.05), window=8, words=(1, 2, 3), word_offsets=(0, 2, 3)):
    w, off = np.asarray(words, np.int64), np.asarray(word_offsets, np.int64)
    Q = off.size - 1
    q = ca.NvsmQueries(w.ctypes.data, None, off.ctypes.data, Q)
    L = ca.lib()
    lo, so = ca.NvsmLexicalOptions(), ca.NvsmSdmOptions()
    L.nvsm_lexical_options_default(C.byref(lo))
    L.nvsm_sdm_options_default(C.byref(so))
    lo.method, lo.param, lo.top_k = method, param, top_k
    (so.w_term, so.w_ordered, so.w_unordered), so.window = weights, window
    if call == "pairs":
        o, u = np.full(8, 7, np.uint64), np.full(8, 7, np.uint64)
        return L.nvsm_sdm_pair_counts(m._h, C.byref(q), C.byref(so), o.ctypes.data, u.ctypes.data), (o, u)
    ids = np.full((Q, max(top_k, 1)), -7, np.int64)
    scores = np.full((Q, max(top_k, 1)), -7.0, np.float32)
    counts = np.full(Q, -7, np.int64)
    st = L.nvsm_sdm_rank(m._h, C.byref(q), C.byref(lo), C.byref(so), ids.ctypes.data, scores.ctypes.data, counts.ctypes.data)
    return st, (ids, scores, counts)


def test_refusals_are_status_codes_and_the_handle_stays_usable():
    tokens, offsets = lr.zipf_corpus(31, 40, 300)
    m = lexical_model(40, num_words=300)
    L = ca.lib()
    for call in ("rank", "pairs"):
        st, _ = raw_sdm(m, call)
        assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error()  # no corpus uploaded
    m.upload_corpus(ca.Corpus(tokens, offsets))
    nan, inf = float("nan"), float("inf")
    own = [
        (dict(weights=(-0.5, 1, 1)), b"negative or not finite"), (dict(weights=(1, nan, 0)), b"negative or not finite"),
        (dict(weights=(1, 0, inf)), b"negative or not finite"), (dict(weights=(0, 0, 0)), b"all zero"),
        (dict(window=1), b"window"), (dict(window=0), b"window"), (dict(window=ca.SDM_MAX_WINDOW + 1), b"window"), (dict(window=-8), b"window"),
        (dict(word_offsets=(0, 3, 2)), b"queries->offsets decrease"), (dict(word_offsets=(1, 2, 3)), b"offsets[0]"),
    ]
    lexical = [
        (dict(method=2), b"method"), (dict(param=1.0), b"lambda"), (dict(param=nan), b"param"), (dict(method=1, param=-1.0), b"mu"),
        (dict(top_k=0), b"top_k"), (dict(top_k=41), b"top_k"),
    ]
    for call, bad in (("rank", own + lexical), ("pairs", own)):
        for kwargs, word in bad:
            st, out = raw_sdm(m, call, **kwargs)
            assert st == 1 and word in L.nvsm_last_error(), (call, kwargs, L.nvsm_last_error())
            assert all((a == (7 if call == "pairs" else -7)).all() for a in out), "nothing was written"
            st, out = raw_sdm(m, call)
            assert st == 0
    assert raw_sdm(m, window=2)[0] == 0 and raw_sdm(m, window=ca.SDM_MAX_WINDOW)[0] == 0 and raw_sdm(m, weights=(0, 0, 1))[0] == 0
    # a word id out of range matches nothing, and the call says so
    st, out = raw_sdm(m, words=(1, 300, 3))
    assert st == 1 and b"num_words" in L.nvsm_last_error()
    same_bits(out, raw_sdm(m, words=(1, 3), word_offsets=(0, 1, 2))[1])
    st, (o, u) = raw_sdm(m, "pairs", words=(1, 300, 3))
    assert st == 1 and b"num_words" in L.nvsm_last_error() and o[0] == 0 and u[0] == 0
    for kwargs in (dict(weights=(0, 0, 0)), dict(window=1), dict(window=ca.SDM_MAX_WINDOW + 1), dict(method="bm25"), dict(top_k=0)):
        with pytest.raises(ValueError):
            m.sdm_rank([[1, 2]], **kwargs)
    fresh = lexical_model(40, num_words=300, corpus=(tokens, offsets))      # what the calls allocated is not in the text
    assert m.describe() == fresh.describe()
    m.upload_corpus(None)
    st, _ = raw_sdm(m)
    assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error()
