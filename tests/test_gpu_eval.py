"""-m gpu: nvsm_evaluate (csrc/eval.hip) — the ranking of nvsm_rank plus per-query retrieval metrics computed on the device —
against Model.rank and the fp64 restatement of the metric contract in tests/eval_reference.py.

What is asserted for every case: the ids, scores and counts equal Model.rank's bit for bit; num_ret, num_rel and num_rel_ret
equal the reference's exactly; every real metric is within 1e-10 of the reference applied to those ids; a second call returns
the same bits.

The bound. A metric is a ratio of two sums of at most 5000 terms here (k <= |D| <= 5000, judged lists <= 4097), every term at
most 3 (grades <= 3, c_i / i <= 1) and within 8 ulp of its fp64 value (one log2, one division), summed in fp64 in another
order than numpy's: below 5000 · 3 · 9e-16 ≈ 1.4e-11 absolute per sum, and the ratios are at most 1, so 1e-10 holds both."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import eval_reference as er
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_rank import ADAM_STATE, same_bits, trained_like_model

pytestmark = pytest.mark.gpu

W_NAME, E_NAME, T_NAME, B_NAME = PARAMS
CUTOFFS = (1, 5, 64, 65, 1000, 10 ** 6)
JUDGED_LENGTHS = (0, 1, 2, 63, 64, 65, 4097)
BOUND = 1e-10
NUM_WORDS = 300


def random_model(D, de, seed):
    spec = dict(num_words=NUM_WORDS, num_entities=D, word_dim=24, entity_dim=de, window=2, num_random=1, nonlinearity="tanh",
                update_method="sgd")
    rs = np.random.RandomState(seed)
    params = random_params(spec, rs)
    params[W_NAME] = rs.uniform(-1, 1, params[W_NAME].size).astype(np.float32)
    params[T_NAME] = (params[T_NAME] * 2).astype(np.float32)
    params[E_NAME] = rs.standard_normal(params[E_NAME].size).astype(np.float32)
    m = gpu_model(spec, 8)
    load_params(m, params, True)
    return m


def judged_list(rs, D, length):
    """`length` judged (id, grade) pairs: distinct ids of [0, D) — 0 and D - 1 among them where there is room — and some -1
    entries (every entry that finds no distinct id left is one); grades in {-1, 0, 1, 2, 3}"""
    held = min(length - length // 8, D)
    if held >= 2:
        ids = np.concatenate([[0, D - 1], rs.choice(np.arange(1, D - 1), held - 2, replace=False)])
    else:
        ids = rs.choice(D, held, replace=False)
    ids = np.concatenate([ids, np.full(length - held, -1)]).astype(np.int64)
    grades = rs.randint(-1, 4, length)
    order = rs.permutation(length)
    return np.stack([ids[order], grades[order]], 1).astype(np.int64)


def inputs(rs, D, Q, wordless=True):
    queries = [rs.randint(0, NUM_WORDS, rs.randint(1, 9)) for _ in range(Q)]
    if wordless and Q >= 3:
        queries[1] = np.zeros(0, np.int64)
    judged = [judged_list(rs, D, JUDGED_LENGTHS[(q + Q) % len(JUDGED_LENGTHS)]) for q in range(Q)]
    return queries, judged


def check_against_reference(res, ranking, queries, judged, cutoffs=CUTOFFS):
    ids, scores, counts = ranking
    ref = er.evaluate(ids, counts, judged, cutoffs, has_words=[len(q) > 0 for q in queries])
    assert list(res) == er.names(cutoffs)
    worst = 0.0
    for name in er.names(cutoffs):
        assert res[name].dtype == np.float64 and res[name].shape == (len(queries),)
        if name in er.INTEGER:
            np.testing.assert_array_equal(res[name], ref[name], err_msg=name)
        else:
            err = float(np.abs(res[name] - ref[name]).max()) if len(queries) else 0.0
            worst = max(worst, err)
            assert err <= BOUND, (name, err)
    return worst


# ---- shapes: every k, Q and judged length at which the kernel takes another number of blocks, search steps or rounds ------------------
@pytest.mark.parametrize("D,de", [(1, 36), (1, 64), (65, 36), (65, 64), (5000, 36), (5000, 64)])
def test_metrics_and_ranking_over_shapes(D, de):
    m = random_model(D, de, D + de)
    m.profile_enable(True)
    rs = np.random.RandomState(D * 3 + de)
    ks = sorted({k for k in (1, 63, 64, 65, 129, 1000, D) if k <= D})
    cases = [(k, (1, 3, 257)[(i + (2 if de == 64 else 0)) % 3], ("cosine", "dot")[i % 2]) for i, k in enumerate(ks)]
    cases.append((ks[-1], 257, "cosine"))                            # two rounds at the largest k: the second round's query offset
    seen_more_relevant_than_k = False
    for k, Q, sim in cases:
        queries, judged = inputs(rs, D, Q)
        res, ids, scores, counts = m.evaluate(queries, judged, top_k=k, cutoffs=CUTOFFS, similarity=sim, return_ranking=True)
        same_bits((ids, scores, counts), m.rank(queries, top_k=k, similarity=sim))
        worst = check_against_reference(res, (ids, scores, counts), queries, judged)
        again = m.evaluate(queries, judged, top_k=k, cutoffs=CUTOFFS, similarity=sim)          # metrics alone: no ranking comes back
        for name in res:
            np.testing.assert_array_equal(again[name].view(np.uint64), res[name].view(np.uint64), err_msg=name)
        if Q >= 3:
            assert all(res[name][1] == 0.0 for name in res), "a query without words gets all zeros"
        seen_more_relevant_than_k |= bool((res["num_rel"] > k).any())
        print("eval-error D=%d de=%d Q=%d k=%d %s: max |metric - fp64 reference| %.3g" % (D, de, Q, k, sim, worst))
    assert seen_more_relevant_than_k
    names = set(m.profile())
    assert "rank_eval" in names and ("rank_scan_mfma" if de % 64 == 0 else "rank_scan_plain") in names


def test_rank_alone_never_launches_the_metrics_kernel():
    m = random_model(65, 36, 1)
    m.profile_enable(True)
    m.rank([[1, 2]], top_k=5)
    assert "rank_eval" not in m.profile()


def test_candidate_lists_shorter_than_k():
    D, k = 5000, 129
    m = random_model(D, 64, 9)
    rs = np.random.RandomState(4)
    lengths = [0, 1, 63, 64, 65, 128, 129, 500]
    queries, judged = inputs(rs, D, len(lengths), wordless=False)
    cands = [rs.randint(0, D, n) for n in lengths]
    for q, c in enumerate(cands):                                    # half of every list is judged, so that something is found
        if c.size >= 2:
            half = np.unique(c)[::2]
            judged[q] = np.stack([half, rs.randint(-1, 4, half.size)], 1)
    for sim in ("cosine", "dot"):
        res, ids, scores, counts = m.evaluate(queries, judged, top_k=k, cutoffs=CUTOFFS, candidates=cands, similarity=sim,
                                              return_ranking=True)
        same_bits((ids, scores, counts), m.rank(queries, top_k=k, candidates=cands, similarity=sim))
        assert list(counts) == [min(k, np.unique(c).size) for c in cands] and (counts < k).any()
        np.testing.assert_array_equal(res["num_ret"], counts.astype(np.float64))
        check_against_reference(res, (ids, scores, counts), queries, judged)
        assert res["num_rel_ret"].sum() > 0


def test_no_cutoffs_and_no_queries():
    m = random_model(65, 36, 2)
    rs = np.random.RandomState(6)
    queries, judged = inputs(rs, 65, 3)
    res, ids, scores, counts = m.evaluate(queries, judged, top_k=10, cutoffs=(), return_ranking=True)
    assert list(res) == list(er.FIXED)
    check_against_reference(res, (ids, scores, counts), queries, judged, cutoffs=())
    res = m.evaluate([], [], top_k=10)
    assert all(v.shape == (0,) for v in res.values()) and len(res) == 7 + 3 * 5


def test_evaluating_between_steps_never_disturbs_training():
    """as tests/test_gpu_rank.py checks for nvsm_rank: a call straight behind nvsm_step sees the finished updates, and parameters and
    optimiser state stay bit-identical to a twin that never evaluated"""
    rs = np.random.RandomState(17)
    spec, params, a = trained_like_model(rs)
    _, _, b = trained_like_model(np.random.RandomState(17))
    _, _, c = trained_like_model(np.random.RandomState(17))
    D = spec["num_entities"]
    queries = [rs.randint(0, 2000, rs.randint(1, 12)) for _ in range(20)]
    judged = [judged_list(rs, D, 65) for _ in queries]
    batches = [random_batch(spec, rs, 64, zipf=True) for _ in range(6)]
    for words, ww, labels, iw, ids in batches:
        for m in (a, b, c):
            m.step(ca.Batch(words, labels, ww, iw), 5e-3, entity_ids=ids)
        ra = a.evaluate(queries, judged, top_k=50, return_ranking=True)      # straight behind nvsm_step: its side-stream tails still run
        c.synchronize()
        same_bits(ra[1:], c.rank(queries, top_k=50))
    check_against_reference(ra[0], ra[1:], queries, judged, cutoffs=(5, 10, 20, 100, 1000))
    for n in list(PARAMS) + ADAM_STATE:                                      # b never ranked or evaluated
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    assert np.abs(a.get_param(E_NAME) - params[E_NAME]).max() > 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def raw_evaluate(m, judged_ids, grades, joff, cutoffs, top_k=5, metrics=True, num_cutoffs=None, word_offsets=(0, 2, 3)):
    words, woff = np.asarray([1, 2, 3], np.int64), np.asarray(word_offsets, np.int64)
    Q = woff.size - 1
    q = ca.NvsmQueries(words.ctypes.data, None, woff.ctypes.data, Q)
    o = ca.NvsmRankOptions()
    ca.lib().nvsm_rank_options_default(C.byref(o))
    o.top_k = top_k
    jd, jg, jo = np.asarray(judged_ids, np.int64), np.asarray(grades, np.int32), np.asarray(joff, np.int64)
    cut = np.asarray(cutoffs, np.int32)
    j = ca.NvsmJudgments(jd.ctypes.data, jg.ctypes.data, jo.ctypes.data, cut.ctypes.data, cut.size if num_cutoffs is None else num_cutoffs)
    out = np.full(Q * (7 + 3 * 8), -7.0)          # room for the widest rows; the call writes [Q][7 + 3 * num_cutoffs] at its start
    st = ca.lib().nvsm_evaluate(m._h, C.byref(q), C.byref(o), C.byref(j), out.ctypes.data if metrics else None, None, None, None)
    return st, out


def test_refusals_are_status_codes_and_the_handle_stays_usable():
    D = 65
    m = random_model(D, 36, 3)
    L = ca.lib()
    good = dict(judged_ids=[4, -1, 7], grades=[1, 2, 1], joff=[0, 2, 3], cutoffs=[1, 5])
    bad = [
        (dict(good, joff=[0, 3, 2]), b"offsets"),                         # decreasing offsets
        (dict(good, joff=[1, 2, 3]), b"offsets[0]"),
        (dict(good, judged_ids=[4, D, 7]), b"judged document id"),        # an id outside [-1, num_entities)
        (dict(good, judged_ids=[4, -2, 7]), b"judged document id"),
        (dict(good, judged_ids=[4, 4, 7]), b"twice"),                     # the same id >= 0 twice within one query
        (dict(good, cutoffs=[5, 5]), b"ascend"),
        (dict(good, cutoffs=[5, 1]), b"ascend"),
        (dict(good, cutoffs=[0, 5]), b"cutoff"),
        (dict(good, cutoffs=list(range(1, 10))), b"num_cutoffs"),         # more than 8
        (dict(good, num_cutoffs=-1), b"num_cutoffs"),
        (dict(good, metrics=False), b"metrics"),
        (dict(good, top_k=0), b"top_k"),                                  # ... and what nvsm_rank refuses, in its words
        (dict(good, top_k=D + 1), b"top_k"),
        (dict(good, word_offsets=(0, 3, 2)), b"queries->offsets decrease"),
    ]
    for kwargs, word in bad:
        st, out = raw_evaluate(m, **kwargs)
        assert st == 1 and word in L.nvsm_last_error(), (kwargs, L.nvsm_last_error())
        assert (out == -7.0).all(), "nothing was written"
        st, out = raw_evaluate(m, **good)                                 # the handle is usable after every refusal
        assert st == 0 and (out[:2 * 13] != -7.0).all() and (out[2 * 13:] == -7.0).all()
    rows = out[:2 * 13].reshape(2, 13)
    assert list(rows[:, 1]) == [2.0, 1.0]                                 # num_rel: the -1 entry counts
    # the same id twice in DIFFERENT queries, and -1 twice in one, are fine
    assert raw_evaluate(m, [4, 4, -1, -1], [1, 1, 1, 1], [0, 1, 4], [1])[0] == 0
    queries, judged = [[1, 2], [3]], [[(4, 1), (-1, 2)], [(7, 1)]]
    res, ids, scores, counts = m.evaluate(queries, judged, top_k=5, cutoffs=(1, 5), return_ranking=True)
    check_against_reference(res, (ids, scores, counts), queries, judged, cutoffs=(1, 5))
    np.testing.assert_array_equal(np.stack([res[n] for n in res], 1), rows)
