"""nvsm_lexical_rank on the GPU against the fp64 restatement of its contract (tests/lexical_reference.py): counts equal, scores within
the header's bound, ids equal except where the restatement's own neighbouring scores are closer than twice the bound (at most 1 %
of the positions: tests/test_lexical_reference.py checks that share on the CPU), exact ties by ascending id, the same bits from a
repeated call, training undisturbed, the cf table renewed by an upload, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import lexical_reference as lr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_rank import ADAM_STATE, same_bits

pytestmark = pytest.mark.gpu

V = lr.NUM_WORDS
METHODS = [(m, p) for m in ("jm", "dirichlet") for p in (None, lr.EXPLICIT[m])]


def lexical_model(num_documents, num_words=V, corpus=None):
    spec = dict(num_words=num_words, num_entities=max(num_documents, 2), word_dim=8, entity_dim=8, window=2, num_random=1,
                nonlinearity="tanh", update_method="sgd")
    m = gpu_model(spec, 8)
    load_params(m, random_params(spec, np.random.RandomState(num_documents)), True)
    if corpus is not None:
        m.upload_corpus(ca.Corpus(*corpus))
    return m


_collections, _references = {}, {}


def collection(tokens, offsets, num_words):
    """the restatement's view of a collection, made once per collection and shared by the tests' calls"""
    key = (tokens.tobytes(), offsets.tobytes(), num_words)
    if key not in _collections:
        _collections.clear()
        _references.clear()
        _collections[key] = lr.Collection(tokens, offsets, num_words)
    return _collections[key]


def reference(coll, query, method, param):
    """... and a query's restatement ranking: computed once, shared among the top_k values, never changed"""
    key = (tuple(int(t) for t in query), method, param)
    if key not in _references:
        _references[key] = lr.rank_query(coll, query, method, param)
    return _references[key]


def check_ranking(result, tokens, offsets, queries, method, param, top_k, num_words=V, share=lr.SHARE):
    """every assertion of the contract for one call; returns (positions excused, positions, worst score error / bound)"""
    ids, scores, counts = result
    assert ids.shape == scores.shape == (len(queries), top_k) and counts.shape == (len(queries),)
    coll = collection(tokens, offsets, num_words)
    left = total = 0
    worst = 0.0
    for i, q in enumerate(queries):
        order, ref, bound = reference(coll, q, method, param)
        n = min(top_k, order.size)
        assert counts[i] == n, (i, counts[i], n)
        assert (ids[i, n:] == -1).all() and np.isneginf(scores[i, n:]).all()
        if n == 0:
            continue
        got = ids[i, :n]
        assert got.min() >= 0 and np.unique(got).size == n
        err = np.abs(scores[i, :n].astype(np.float64) - ref[got])
        assert (err <= bound[got]).all(), (i, float((err / bound[got]).max()))
        worst = max(worst, float((err / bound[got]).max()))
        open_ = lr.excused(ref[order], bound[order])[:n]
        differ = got != order[:n]
        assert not (differ & ~open_).any(), (i, np.flatnonzero(differ & ~open_)[:5])
        tied = scores[i, :n - 1] == scores[i, 1:n]                        # the GPU's own ties: ascending id
        assert (got[:-1][tied] < got[1:][tied]).all()
        left += int(open_.sum())
        total += n
    assert left <= share * total, (left, total)
    return left, total, worst


# ---- the hand-built collection: every document shape the kernel treats differently ------------------------------------------------
def hand_built():
    rs = np.random.RandomState(5)
    draw = lambda n: list(rs.randint(0, 40, n))
    twin = draw(30)
    docs = [[], [7], draw(63), draw(64), draw(65), twin, [], list(twin), draw(5000), draw(17)]
    tokens = np.array([t for d in docs for t in d], np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    assert offsets[-1] == tokens.size and len(docs[-1]) > 0
    return tokens, offsets


HAND_QUERIES = [[7], [7, 7], [3, V - 1, 4], [V - 1, V - 2], [], [7, 3, 7, 39, 0], [11, 11, 11]]


@pytest.mark.parametrize("method,param", METHODS)
def test_hand_built_collection(method, param):
    tokens, offsets = hand_built()
    m = lexical_model(offsets.size - 1, corpus=(tokens, offsets))
    for k in (1, 3, offsets.size - 1):
        res = m.lexical_rank(HAND_QUERIES, method=method, param=param, top_k=k)
        check_ranking(res, tokens, offsets, HAND_QUERIES, method, param, k)
        ids, scores, counts = res
        assert counts[3] == 0 and counts[4] == 0                          # only absent terms; no words
        np.testing.assert_array_equal(scores[0], m.lexical_rank([[7]], method=method, param=param, top_k=k)[1][0])
    # the twins (documents 5 and 7, an empty one between them) tie exactly: ascending id; the empty documents are never retrieved
    assert list(ids[5]).index(5) + 1 == list(ids[5]).index(7) and scores[5][list(ids[5]).index(5)] == scores[5][list(ids[5]).index(7)]
    assert not np.isin(ids, [0, 6]).any()
    # a repeated term counts twice: a + a is exact in fp64, so the narrowed scores of [7, 7] are twice those of [7], bit for bit
    assert counts[1] == counts[0] > 0
    np.testing.assert_array_equal(scores[1][:counts[1]], 2 * scores[0][:counts[0]])


# ---- seeded Zipf collections over the shapes: one document, fewer than a wave, one slab, three slabs; one round and two -------------
@pytest.mark.parametrize("documents,queries,top_ks", lr.CASES)
def test_seeded_collections(documents, queries, top_ks, monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", "1")                          # 9001 documents, 256 queries: three slabs of 4096
    tokens, offsets, qs = lr.case_inputs(documents, queries)
    m = lexical_model(documents, corpus=(tokens, offsets))
    m.profile_enable(True)
    for j, k in enumerate(top_ks):
        for method, param in METHODS:
            res = m.lexical_rank(qs, method=method, param=param, top_k=k)
            left, total, worst = check_ranking(res, tokens, offsets, qs, method, param, k)
            print("lexical D=%d Q=%d k=%d %s %s: %d of %d positions open, worst error %.3g of the bound"
                  % (documents, queries, k, method, param, left, total, worst))
        same_bits(res, m.lexical_rank(qs, method=method, param=param, top_k=k))
    names = set(m.profile())
    assert "lex_score" in names and "lex_cf" in names
    if documents == 9001 and queries == 300:
        assert "rank_select_radix" in names and "rank_select_all" in names


def test_a_round_with_more_distinct_terms_than_slots():
    """300 queries of five words drawn evenly from the words that occur: the 256 queries of a plain round hold more than the 1024 distinct
    terms a round has counters for, so the rounds are cut by terms; the result is that of the queries ranked one by one"""
    tokens, offsets = lr.zipf_corpus(77, 1000, V)
    cf = lr.collection_frequencies(tokens, V)
    present = np.flatnonzero(cf > 0)
    rs = np.random.RandomState(78)
    qs = [list(present[rs.randint(0, present.size, 5)]) for _ in range(300)]
    assert np.unique(np.concatenate(qs[:256])).size > 1024
    m = lexical_model(1000, corpus=(tokens, offsets))
    res = m.lexical_rank(qs, top_k=20)
    check_ranking(res, tokens, offsets, qs, "jm", None, 20)
    for i in (0, 170, 171, 255, 256, 299):
        one = m.lexical_rank([qs[i]], top_k=20)
        same_bits([r[i:i + 1] for r in res], one)
    # one query alone may hold as many distinct terms as there are slots, and no more
    wide = list(present[:1024])
    # (L = 1027 makes the bound, and with it the margin, a thousand times a short query's: no cap on the open positions here)
    check_ranking(m.lexical_rank([wide + wide[:3]], top_k=5), tokens, offsets, [wide + wide[:3]], "jm", None, 5, share=1.0)
    with pytest.raises(ca.NvsmError) as e:
        m.lexical_rank([list(present[:1025])], top_k=5)
    assert e.value.status == 2 and "distinct terms" in str(e.value)


def test_a_lexical_call_between_steps_never_disturbs_training():
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
        res = a.lexical_rank(queries, top_k=50)                           # straight behind nvsm_step
        if first is None:
            first = res
        same_bits(first, res)                                             # a function of corpus and query, not of the parameters
    check_ranking(res, tokens, offsets, queries, "jm", None, 50, num_words=2000)
    state_a, state_b = a.rng_state, b.rng_state
    assert state_a == state_b
    for n in list(PARAMS) + ADAM_STATE:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)


def test_an_upload_renews_the_cf_table_and_freeing_the_corpus_refuses():
    tokens, offsets = lr.zipf_corpus(21, 50, 300)
    other = (tokens[::-1].copy() + 7) % 300
    m = lexical_model(50, num_words=300, corpus=(tokens, offsets))
    queries = lr.zipf_queries(22, 12, 300, tokens)
    check_ranking(m.lexical_rank(queries, top_k=50), tokens, offsets, queries, "jm", None, 50, num_words=300)
    m.upload_corpus(ca.Corpus(other.astype(np.int32), offsets))
    assert (lr.collection_frequencies(other, 300) != lr.collection_frequencies(tokens, 300)).any()
    check_ranking(m.lexical_rank(queries, top_k=50), other, offsets, queries, "jm", None, 50, num_words=300)
    m.upload_corpus(None)
    with pytest.raises(ca.NvsmError) as e:
        m.lexical_rank(queries, top_k=5)
    assert e.value.status == 1 and "corpus" in str(e.value)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_lexical(m, method=0, param=0.0, top_k=5, words=(1, 2, 3), word_offsets=(0, 2, 3), null=None):
    w, off = np.asarray(words, np.int64), np.asarray(word_offsets, np.int64)
    Q = off.size - 1
    q = ca.NvsmQueries(w.ctypes.data, None, None if null == "offsets" else off.ctypes.data, Q)
    o = ca.NvsmLexicalOptions()
    ca.lib().nvsm_lexical_options_default(C.byref(o))
    o.method, o.param, o.top_k = method, param, top_k
    ids = np.full((Q, max(top_k, 1)), -7, np.int64)
    scores = np.full((Q, max(top_k, 1)), -7.0, np.float32)
    counts = np.full(Q, -7, np.int64)
    ptr = lambda name, a: None if null == name else a.ctypes.data
    st = ca.lib().nvsm_lexical_rank(m._h, None if null == "queries" else C.byref(q), None if null == "lex" else C.byref(o),
                                    ptr("doc_ids", ids), ptr("scores", scores), ptr("counts", counts))
    return st, (ids, scores, counts)


def test_refusals_are_status_codes_and_the_handle_stays_usable():
    tokens, offsets = lr.zipf_corpus(31, 40, 300)
    m = lexical_model(40, num_words=300)
    L = ca.lib()
    st, _ = raw_lexical(m)
    assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error()      # no corpus uploaded
    m.upload_corpus(ca.Corpus(tokens, offsets))
    bad = [
        (dict(method=2), b"method"), (dict(method=-1), b"method"),
        (dict(param=1.0), b"lambda"), (dict(param=-0.1), b"lambda"), (dict(param=1.5), b"lambda"), (dict(param=float("nan")), b"param"),
        (dict(method=1, param=-1.0), b"mu"),
        (dict(top_k=0), b"top_k"), (dict(top_k=41), b"top_k"),
        (dict(word_offsets=(0, 3, 2)), b"queries->offsets decrease"), (dict(word_offsets=(1, 2, 3)), b"offsets[0]"),
        (dict(null="queries"), b"null argument: queries"), (dict(null="lex"), b"null argument: lex"),
        (dict(null="doc_ids"), b"null argument: doc_ids"), (dict(null="scores"), b"null argument: scores"),
        (dict(null="counts"), b"null argument: counts"), (dict(null="offsets"), b"null argument: queries->offsets"),
    ]
    for kwargs, word in bad:
        st, out = raw_lexical(m, **kwargs)
        assert st == 1 and word in L.nvsm_last_error(), (kwargs, L.nvsm_last_error())
        assert all((a == -7).all() for a in out), "nothing was written"
        st, out = raw_lexical(m)
        assert st == 0 and (out[2] >= 0).all()
    # a word id out of range matches nothing, and the call says so
    st, out = raw_lexical(m, words=(1, 300, 3))
    assert st == 1 and b"num_words" in L.nvsm_last_error()
    good = raw_lexical(m, words=(1, 3), word_offsets=(0, 1, 2))[1]
    same_bits(out, good)
    st, out = raw_lexical(m, words=(-1, 2, 3))
    assert st == 1 and b"num_words" in L.nvsm_last_error()
    # mu = 0 is auto, not a refusal; the Python layer refuses what needs no device
    assert raw_lexical(m, method=1, param=0.0)[0] == 0
    for kwargs in (dict(method="bm25"), dict(param=1.0), dict(method="dirichlet", param=-1.0), dict(top_k=0)):
        with pytest.raises(ValueError):
            m.lexical_rank([[1]], **kwargs)
    fresh = lexical_model(40, num_words=300, corpus=(tokens, offsets))      # what the lexical calls allocated is not in the text
    assert m.describe() == fresh.describe()
