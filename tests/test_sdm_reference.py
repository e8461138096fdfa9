"""tests/sdm_reference.py held to counts and scores worked out by hand on a three-document collection, and — on the inputs the GPU test
ranks — to the condition that test relies on: the restatement alone leaves the order of at most lexical_reference.SHARE of the top-k
positions open."""
import math

import numpy as np
import pytest

from tests import lexical_reference as lr
from tests import sdm_reference as sr

#          d0: 1 2 1 3 2        d1: 2 1      d2: 1 1 2 4
TOY = (np.array([1, 2, 1, 3, 2, 2, 1, 1, 1, 2, 4], np.int32), np.array([0, 5, 7, 11], np.int64))
W = 3      # a position looks at the two positions behind it


def toy():
    return sr.Positions(lr.Collection(TOY[0], TOY[1], 6))


def test_counts_by_hand():
    pos = toy()
    # (1, 2) ordered: d0 position 0, d2 position 1. d1's "2 1" is the other order; its last 1 does not pair with d2's first token
    od, uw = pos.pair_counts(1, 2, W)
    assert od.tolist() == [1, 0, 1]
    # unordered: d0 positions 0 (2 follows), 1 (1 follows), 2 (2 two behind), not 4 (the document ends); d1 position 0; d2 positions 0, 1
    assert uw.tolist() == [3, 1, 2]
    od, uw = pos.pair_counts(2, 1, W)
    assert od.tolist() == [1, 1, 0] and uw.tolist() == [3, 1, 2]      # the unordered count is symmetric
    # a = a: d2 "1 1" once; d1's last token and d2's first are both 1 and do not pair. Unordered: d0 position 0 (1 two behind), d2 position 0
    od, uw = pos.pair_counts(1, 1, W)
    assert od.tolist() == [0, 0, 1] and uw.tolist() == [1, 0, 1]
    # an existence test: with W = 4 d0's position 0 sees two 1s... and still counts once
    assert pos.pair_counts(2, 1, 4)[1].tolist() == [3, 1, 2] and pos.pair_counts(1, 2, 2)[1].tolist() == [2, 1, 1]
    # a word nobody holds, and one outside the vocabulary
    assert pos.pair_counts(1, 5, W)[1].sum() == 0 and pos.pair_counts(1, 6, W)[0].sum() == 0 and pos.pair_counts(-1, 1, W)[1].sum() == 0
    o, u = sr.pair_counts(pos, [[1, 2, 1], [], [1], [1, 1], [1, 5, 2]], W)
    assert o.dtype == np.uint64 and o.tolist() == [2, 2, 1, 0, 0] and u.tolist() == [6, 6, 2, 0, 0]


def test_scores_by_hand():
    pos = toy()
    N, mu = 11.0, 2.0
    weights = (0.5, 0.25, 0.25)
    scores, matched, bound = sr.score_query(pos, [1, 2], "dirichlet", mu, weights, W)
    assert matched.tolist() == [True, True, True]
    # d0: len 5, tf(1) = 2, tf(2) = 2, od = 1 of cf_o = 2, uw = 3 of cf_u = 6; cf(1) = 5, cf(2) = 4
    g_t = (math.log((2 + mu * 5 / N) / (5 + mu)) + math.log((2 + mu * 4 / N) / (5 + mu))) / 2
    g_o = math.log((1 + mu * 2 / N) / (5 + mu))
    g_u = math.log((3 + mu * 6 / N) / (5 + mu))
    assert scores[0] == pytest.approx(0.5 * g_t + 0.25 * g_o + 0.25 * g_u, rel=1e-14)
    # d1: len 2, tf 1 and 1, od = 0, uw = 1
    g_t = (math.log((1 + mu * 5 / N) / (2 + mu)) + math.log((1 + mu * 4 / N) / (2 + mu))) / 2
    assert scores[1] == pytest.approx(0.5 * g_t + 0.25 * math.log((mu * 2 / N) / (2 + mu)) + 0.25 * math.log((1 + mu * 6 / N) / (2 + mu)), rel=1e-14)
    assert (bound == sr.EPS * np.abs(scores)).all()
    # Jelinek-Mercer, the same document: (1 - lam) c / len + lam cf_x / N
    lam = 0.5
    jm = sr.score_query(pos, [1, 2], "jm", None, weights, W)[0]
    g_t = (math.log(lam * 2 / 5 + lam * 5 / N) + math.log(lam * 2 / 5 + lam * 4 / N)) / 2
    assert jm[0] == pytest.approx(0.5 * g_t + 0.25 * math.log(lam * 1 / 5 + lam * 2 / N) + 0.25 * math.log(lam * 3 / 5 + lam * 6 / N), rel=1e-14)


def test_dropped_members_and_absent_groups():
    pos = toy()
    mu, N = 2.0, 11.0
    # [1, 4, 2]: (1, 4) and (4, 2) never occur as phrases (cf_o = 0: O has no member) but each co-occurs once in d2 within W = 3
    o, u = sr.pair_counts(pos, [[1, 4, 2]], W)
    assert o.tolist() == [0, 0] and u.tolist() == [1, 1]
    scores = sr.score_query(pos, [1, 4, 2], "dirichlet", mu, (0.5, 0.25, 0.25), W)[0]
    # d2: len 4, tf(1) = 2, tf(4) = 1, tf(2) = 1; both unordered counts 1 of cf_u = 1; the weights are normalised over T and U
    g_t = (math.log((2 + mu * 5 / N) / 6) + math.log((1 + mu * 1 / N) / 6) + math.log((1 + mu * 4 / N) / 6)) / 3
    g_u = (math.log((1 + mu * 1 / N) / 6) + math.log((1 + mu * 1 / N) / 6)) / 2
    assert scores[2] == pytest.approx((0.5 / 0.75) * g_t + (0.25 / 0.75) * g_u, rel=1e-14)
    # an absent word in the middle: both pairs around it drop, the score is that of the terms alone — the mean of lexical_reference's sum
    s, matched, _ = sr.score_query(pos, [1, 5, 2], "dirichlet", mu, sr.DEFAULT_WEIGHTS, W)
    plain = lr.score_query(pos.coll, [1, 2], "dirichlet", mu)[0]
    np.testing.assert_allclose(s, plain / 2, rtol=1e-14)
    # one term: no pairs; no term: nothing retrieved; weights (0, 1, 0) on a query without pairs: retrieved, score 0
    one = sr.rank_query(pos, [3], "jm", None)
    assert one[0].tolist() == [0]
    assert sr.rank_query(pos, [], "jm", None)[0].size == 0 and sr.rank_query(pos, [5], "jm", None)[0].size == 0
    order, s, _ = sr.rank_query(pos, [3], "jm", None, (0.0, 1.0, 0.0))
    assert order.tolist() == [0] and s[0] == 0.0
    # (0, 1, 0): by ordered pairs alone over the retrieved set of the terms; d1 holds both words and no phrase "1 2"
    order, s, _ = sr.rank_query(pos, [1, 2], "dirichlet", mu, (0.0, 1.0, 0.0), W)
    assert sorted(order.tolist()) == [0, 1, 2] and order[-1] == 1
    assert s[1] == pytest.approx(math.log((mu * 2 / N) / 4), rel=1e-14)


def test_the_hand_built_collection_holds_what_it_says():
    for window in sr.WINDOWS:
        tokens, offsets, notes = sr.hand_built(window)
        assert tokens.max() < sr.HAND_WORDS and offsets[-1] == tokens.size
        assert notes["slab_last"] == 4095 and notes["slab_first"] == 4096 and notes["last"] == offsets.size - 2
        lens = offsets[1:] - offsets[:-1]
        assert lens[notes["empty0"]] == lens[notes["empty1"]] == 0 and notes["empty1"] == notes["empty0"] + 1
        assert [int(lens[notes[n]]) for n in ("one", "len255", "len256", "len257", "len256w", "long")] == [1, 255, 256, 257, 256 + window - 1, 5000]
        pos = sr.Positions(lr.Collection(tokens, offsets, sr.HAND_WORDS))
        od, uw = pos.pair_counts(1, 2, window)
        assert od[notes["len257"]] == 1 and uw[notes["len257"]] == 1                 # across the tile boundary, distance 1; b is the last token
        assert od[notes["len256w"]] == 0 and uw[notes["len256w"]] == 1               # b first, distance W - 1: b's position counts, a's has no look-ahead
        assert od[notes["exact_w"]] == 0 and uw[notes["exact_w"]] == 0               # a distance of exactly W
        assert od[notes["last_a"]] == 0 and uw[notes["last_a"]] == 0 and uw[notes["first_b"]] == 0
        assert od[notes["last"]] == 1 and od[notes["slab_last"]] == 1 and od[notes["slab_first"]] == 1
        # the long document: "1 2" across position 2048, and across 512 where W - 1 = 1; "2 1" across 256 and at the very end
        assert od[notes["long"]] == 1 + (window == 2) and pos.pair_counts(2, 1, window)[0][notes["long"]] == 2
        assert uw[notes["long"]] == 4                                            # the pair at distance W is the one that does not count
        od33, uw33 = pos.pair_counts(3, 3, window)
        assert od33[notes["runs"]] == 3 and uw33[notes["runs"]] == (3 if window == 2 else 5)


@pytest.mark.parametrize("documents,queries,top_ks", sr.CASES)
def test_open_share_of_the_seeded_cases(documents, queries, top_ks):
    tokens, offsets, qs = sr.case_inputs(documents, queries)
    pos = sr.Positions(lr.Collection(tokens, offsets, sr.NUM_WORDS))
    for method in ("jm", "dirichlet"):
        for k in top_ks:
            left, total = sr.open_share(pos, qs, method, None, k)
            assert left <= lr.SHARE * total, (method, k, left, total)


def test_open_share_of_the_other_calls_the_gpu_test_caps():
    tokens, offsets, qs = sr.case_inputs(1000, 300)
    pos = sr.Positions(lr.Collection(tokens, offsets, sr.NUM_WORDS))
    for method in ("jm", "dirichlet"):
        for queries, param, k, weights, window in ((qs[:60], lr.EXPLICIT[method], 10, (0.5, 0.3, 0.2), 3), (qs, None, 50, (1, 0, 0), 8),
                                                   (qs, None, 1000, (0, 1, 0), 8)):
            left, total = sr.open_share(pos, queries, method, param, k, weights, window)
            assert left <= lr.SHARE * total, (method, weights, left, total)
    tokens, offsets = lr.zipf_corpus(3, 600, 300)                        # the collection of the training test
    pos = sr.Positions(lr.Collection(tokens, offsets, 300))
    left, total = sr.open_share(pos, sr.seeded_queries(4, 20, tokens, offsets, 300), "jm", None, 50)
    assert left <= lr.SHARE * total, (left, total)


@pytest.mark.parametrize("window", sr.WINDOWS)
def test_open_share_of_the_hand_built_collection(window):
    tokens, offsets, _ = sr.hand_built(window)
    pos = sr.Positions(lr.Collection(tokens, offsets, sr.HAND_WORDS))
    for method in ("jm", "dirichlet"):
        for k in (1, 10, offsets.size - 1):
            left, total = sr.open_share(pos, sr.HAND_QUERIES, method, None, k, window=window)
            assert left <= lr.SHARE * total, (method, k, left, total)
