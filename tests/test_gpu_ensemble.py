"""nvsm_rank_ensemble on the GPU against the fp64 restatement of the fusion contract (tests/lexical_reference.py) fed with the GPU's
own two lists — nvsm_rank's and nvsm_lexical_rank's —, and its metrics against nvsm_evaluate's formulas (tests/eval_reference.py)
applied to the fused ids."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import eval_reference as er
from tests import lexical_reference as lr
from tests.helpers import PARAMS, gpu_model, load_params, random_params
from tests.test_gpu_eval import judged_list
from tests.test_gpu_rank import same_bits

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME, B_NAME = PARAMS
NUM_WORDS = 2000
CUTOFFS = (1, 5, 10, 100, 1000)
REL = 2.0 ** -22
METRIC_BOUND = 1e-10          # tests/test_gpu_eval.py's


def ensemble_model(D, seed=0, constant_documents=False):
    spec = dict(num_words=NUM_WORDS, num_entities=D, word_dim=24, entity_dim=36, window=2, num_random=1, nonlinearity="tanh",
                update_method="sgd")
    rs = np.random.RandomState(seed + D)
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 2).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    if constant_documents:      # every document row alike: nvsm_rank's scores are one constant per query
        params[E_NAME] = np.tile(params[E_NAME][:36], D)
    m = gpu_model(spec, 8)
    load_params(m, params, True)
    tokens, offsets = lr.zipf_corpus(seed + D, D, NUM_WORDS)
    m.upload_corpus(ca.Corpus(tokens, offsets))
    return m, tokens, offsets


def queries_for(tokens, n, seed):
    qs = lr.zipf_queries(seed, n, NUM_WORDS, tokens)
    absent = np.flatnonzero(lr.collection_frequencies(tokens, NUM_WORDS) == 0)
    assert absent.size >= 2
    if n >= 4:
        qs[1] = []                                        # no words: both lists empty
        qs[2] = [int(absent[0]), int(absent[1])]          # only words that do not occur: the lexical list is empty
    return qs


def check_fusion(m, qs, k, alpha, normalizer, judged=None, **lex):
    """(positions open, positions) of one call checked against the restatement of the GPU's own two lists"""
    a_ids, a_sc, a_n = m.rank(qs, top_k=k)
    b_ids, b_sc, b_n = m.lexical_rank(qs, top_k=k, **lex)
    out = m.rank_ensemble(qs, alpha=alpha, normalizer=normalizer, top_k=k, judgments=judged, cutoffs=CUTOFFS, **lex)
    metrics = None
    if judged is not None:
        metrics, out = out[0], out[1:]
    ids, scores, counts = out
    assert ids.shape == scores.shape == (len(qs), 2 * k) and ids.dtype == np.int64 and scores.dtype == np.float32
    left = total = 0
    for i in range(len(qs)):
        r_ids, r_sc = lr.fuse_query(a_ids[i, :a_n[i]], a_sc[i, :a_n[i]], b_ids[i, :b_n[i]], b_sc[i, :b_n[i]], alpha, normalizer)
        n = r_ids.size
        assert counts[i] == n == np.union1d(a_ids[i, :a_n[i]], b_ids[i, :b_n[i]]).size
        assert (ids[i, n:] == -1).all() and np.isneginf(scores[i, n:]).all()
        if n == 0:
            continue
        got = ids[i, :n]
        assert np.array_equal(np.sort(got), np.sort(r_ids))
        ref_of = dict(zip(r_ids.tolist(), r_sc.tolist()))
        want = np.array([ref_of[int(d)] for d in got])
        narrowed = want.astype(np.float32).astype(np.float64)
        assert (np.abs(scores[i, :n].astype(np.float64) - narrowed) <= REL * np.abs(narrowed)).all(), i
        open_ = lr.excused(r_sc, REL * np.abs(r_sc))
        differ = got != r_ids
        assert not (differ & ~open_).any(), (i, np.flatnonzero(differ & ~open_)[:5])
        left += int(open_.sum())
        total += n
    assert left <= lr.SHARE * total, (left, total)
    if metrics is not None:
        ref = er.evaluate(ids, counts, judged, CUTOFFS, has_words=[len(q) > 0 for q in qs])
        assert list(metrics) == er.names(CUTOFFS)
        for name in er.names(CUTOFFS):
            if name in er.INTEGER:
                np.testing.assert_array_equal(metrics[name], ref[name], err_msg=name)
            else:
                assert np.abs(metrics[name] - ref[name]).max() <= METRIC_BOUND, name
    return (ids, scores, counts), (a_n, b_n), (left, total)


@pytest.mark.parametrize("normalizer", ["standardize", "minmax", "none"])
@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
def test_fusion_and_metrics(alpha, normalizer):
    D = 300
    m, tokens, offsets = ensemble_model(D)
    m.profile_enable(True)
    rs = np.random.RandomState(int(alpha * 10) + len(normalizer))
    for Q, k in ((7, 1), (40, 25), (300, 10), (5, D)):
        qs = queries_for(tokens, Q, Q + k)
        judged = [judged_list(rs, D, (0, 1, 9, 65)[q % 4]) for q in range(Q)]
        res, (a_n, b_n), (left, total) = check_fusion(m, qs, k, alpha, normalizer, judged)
        assert ((res[2] > b_n) & (b_n > 0)).any()                         # documents in one list only (list A's, beside a list B)
        if Q >= 4:
            assert res[2][1] == 0 and b_n[2] == 0 and res[2][2] == a_n[2] == k      # both lists empty; one empty: the other alone
        again = m.rank_ensemble(qs, alpha=alpha, normalizer=normalizer, top_k=k)
        same_bits(res, again)                                             # without judgments: the same fused list, bit for bit
        print("ensemble D=%d Q=%d k=%d alpha=%g %s: %d of %d positions open" % (D, Q, k, alpha, normalizer, left, total))
    assert {"fuse_lists", "lex_score", "rank_eval"} <= set(m.profile())


@pytest.mark.parametrize("normalizer", ["standardize", "minmax", "none"])
def test_a_constant_list_normalises_to_zero(normalizer):
    D = 200
    m, tokens, offsets = ensemble_model(D, seed=1, constant_documents=True)
    qs = queries_for(tokens, 12, 3)
    a_ids, a_sc, a_n = m.rank(qs, top_k=10)
    assert all(np.unique(a_sc[i, :a_n[i]]).size == 1 for i in range(12) if a_n[i])       # the premise: list A is one constant per query
    (ids, scores, counts), (a_n, b_n), _ = check_fusion(m, qs, 10, 0.5, normalizer)
    assert np.isfinite(scores[0, :counts[0]]).all()
    if normalizer != "none":                                              # what only list A holds scores alpha * 0 exactly
        only_a = ~np.isin(ids[0, :counts[0]], m.lexical_rank(qs, top_k=10)[0][0])
        assert only_a.any() and (scores[0, :counts[0]][only_a] == 0.0).all()


def test_top_k_1000_over_two_thousand_documents():
    D = 2000
    m, tokens, offsets = ensemble_model(D, seed=2)
    qs = queries_for(tokens, 6, 11) + [[int(t) for t in tokens[:40]]]    # the last one matches most documents: a long lexical list
    rs = np.random.RandomState(4)
    judged = [judged_list(rs, D, 65) for _ in qs]
    res, (a_n, b_n), (left, total) = check_fusion(m, qs, 1000, 0.5, "standardize", judged)
    assert a_n[-1] == 1000 and b_n[-1] == 1000 and 1000 < res[2][-1] <= 2000
    check_fusion(m, qs, 1000, 0.3, "minmax", method="dirichlet", param=300.0)
    print("ensemble D=%d k=1000: %d of %d positions open" % (D, left, total))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_ensemble(m, top_k=5, lex_top_k=None, alpha=0.5, normalizer=0, method=0, param=0.0, candidates=False, similarity=0):
    words, off = np.asarray([1, 2, 3], np.int64), np.asarray([0, 2, 3], np.int64)
    q = ca.NvsmQueries(words.ctypes.data, None, off.ctypes.data, 2)
    ro, lo, eo = ca.NvsmRankOptions(), ca.NvsmLexicalOptions(), ca.NvsmEnsembleOptions()
    L = ca.lib()
    L.nvsm_rank_options_default(C.byref(ro))
    L.nvsm_lexical_options_default(C.byref(lo))
    L.nvsm_ensemble_options_default(C.byref(eo))
    ro.top_k, ro.similarity = top_k, similarity
    lo.top_k, lo.method, lo.param = top_k if lex_top_k is None else lex_top_k, method, param
    eo.alpha, eo.normalizer = alpha, normalizer
    cand, coff = np.asarray([0, 1], np.int64), np.asarray([0, 1, 2], np.int64)
    if candidates:
        ro.candidates, ro.candidate_offsets = cand.ctypes.data, coff.ctypes.data
    width = 2 * max(top_k, 1)
    ids, scores, counts = np.full((2, width), -7, np.int64), np.full((2, width), -7.0, np.float32), np.full(2, -7, np.int64)
    st = L.nvsm_rank_ensemble(m._h, C.byref(q), C.byref(ro), C.byref(lo), C.byref(eo), None, None, ids.ctypes.data, scores.ctypes.data,
                              counts.ctypes.data)
    return st, (ids, scores, counts)


def test_refusals_are_status_codes_and_the_handle_stays_usable():
    D = 1100
    m, tokens, offsets = ensemble_model(D, seed=5)
    L = ca.lib()
    bad = [
        (dict(normalizer=3), 1, b"normalizer"), (dict(normalizer=-1), 1, b"normalizer"),
        (dict(alpha=1.5), 1, b"alpha"), (dict(alpha=-0.01), 1, b"alpha"), (dict(alpha=float("nan")), 1, b"alpha"),
        (dict(method=7), 1, b"method"), (dict(param=1.0), 1, b"lambda"), (dict(method=1, param=-2.0), 1, b"mu"),
        (dict(top_k=0), 1, b"top_k"), (dict(top_k=D + 1), 1, b"top_k"), (dict(lex_top_k=4), 1, b"equal"),
        (dict(candidates=True), 1, b"candidates"), (dict(similarity=9), 1, b"similarity"),
        (dict(top_k=1025), 2, b"NVSM_ENSEMBLE_MAX_TOP_K"),
    ]
    for kwargs, status, word in bad:
        st, out = raw_ensemble(m, **kwargs)
        assert st == status and word in L.nvsm_last_error(), (kwargs, st, L.nvsm_last_error())
        assert all((a == -7).all() for a in out), "nothing was written"
        st, out = raw_ensemble(m)
        assert st == 0 and (out[2] >= 5).all()
    assert raw_ensemble(m, top_k=1024)[0] == 0                            # the limit itself is served
    m.upload_corpus(None)
    st, out = raw_ensemble(m)
    assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error() and all((a == -7).all() for a in out)
    with pytest.raises(ValueError):
        m.rank_ensemble([[1]], alpha=2.0)
    with pytest.raises(ValueError):
        m.rank_ensemble([[1]], normalizer="zscore")
