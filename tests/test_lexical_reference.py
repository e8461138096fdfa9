"""The fp64 restatement of the lexical and fusion contract (tests/lexical_reference.py) against examples worked by hand, its
invariances, and the near-tie share of the seeded collections the GPU tests rank. No GPU."""
import math

import numpy as np
import pytest

from tests import lexical_reference as lr

# three documents over four words: d0 = [0 1 1], d1 = [2], d2 = [0 0 2 3]; N = 8, cf = 3 2 2 1
TOKENS = np.array([0, 1, 1, 2, 0, 0, 2, 3], np.int32)
OFFSETS = np.array([0, 3, 4, 8], np.int64)
CF = np.array([3, 2, 2, 1, 0], np.int64)              # word 4 does not occur
COLL = lr.Collection(TOKENS, OFFSETS, 5)


def test_collection_frequencies():
    np.testing.assert_array_equal(lr.collection_frequencies(TOKENS, 5), CF)


def test_jelinek_mercer_by_hand():
    order, scores, _ = lr.rank_query(COLL, [1, 0], "jm", None)             # lambda = 0.5
    d0 = math.log(0.5 * 2 / 3 + 0.5 * 2 / 8) + math.log(0.5 * 1 / 3 + 0.5 * 3 / 8)
    d2 = math.log(0.5 * 2 / 8) + math.log(0.5 * 2 / 4 + 0.5 * 3 / 8)
    assert list(order) == [0, 2]                                                          # d1 holds neither word: not retrieved
    assert scores[0] == pytest.approx(d0, abs=1e-15) and scores[2] == pytest.approx(d2, abs=1e-15)
    order, scores, _ = lr.rank_query(COLL, [2], "jm", 0.25)
    assert list(order) == [1, 2]
    assert scores[1] == pytest.approx(math.log(0.75 * 1 / 1 + 0.25 * 2 / 8), abs=1e-15)
    assert scores[2] == pytest.approx(math.log(0.75 * 1 / 4 + 0.25 * 2 / 8), abs=1e-15)


def test_dirichlet_by_hand():
    mu = 8 / 3                                                                            # auto: N / D_c
    order, scores, _ = lr.rank_query(COLL, [0, 3], "dirichlet", None)
    d0 = math.log((1 + mu * 3 / 8) / (3 + mu)) + math.log((0 + mu * 1 / 8) / (3 + mu))
    d2 = math.log((2 + mu * 3 / 8) / (4 + mu)) + math.log((1 + mu * 1 / 8) / (4 + mu))
    assert list(order) == [2, 0]
    assert scores[0] == pytest.approx(d0, abs=1e-15) and scores[2] == pytest.approx(d2, abs=1e-15)
    _, scores, _ = lr.rank_query(COLL, [0], "dirichlet", 2.0)
    assert scores[2] == pytest.approx(math.log((2 + 2.0 * 3 / 8) / (4 + 2.0)), abs=1e-15)


def test_duplicates_count_and_absent_terms_drop():
    _, once, _ = lr.rank_query(COLL, [1], "jm", None)
    order, twice, bound = lr.rank_query(COLL, [1, 1], "jm", None)
    assert twice[0] == pytest.approx(2 * once[0], abs=1e-15)
    _, with_absent, bound3 = lr.rank_query(COLL, [1, 4, 1, 99, -1], "jm", None)   # absent, and out of the vocabulary
    np.testing.assert_array_equal(with_absent, twice)
    np.testing.assert_array_equal(bound3, bound)                                          # L counts the remaining terms
    for nothing in ([4], [], [4, 4]):
        order, _, _ = lr.rank_query(COLL, nothing, "dirichlet", None)
        assert order.size == 0


def test_empty_documents_are_never_retrieved_and_ties_go_by_id():
    tokens = np.array([5, 6, 5, 6, 5], np.int32)
    offsets = np.array([0, 0, 2, 2, 4, 5], np.int64)                                      # d0 and d2 are empty, d1 = d3 = [5 6]
    order, scores, _ = lr.rank_query(lr.Collection(tokens, offsets, 8), [5], "jm", None)
    assert list(order) == [4, 1, 3] and scores[1] == scores[3]


def test_the_bound_is_the_headers():
    _, scores, bound = lr.rank_query(COLL, [1, 0], "jm", None)
    a = [math.log(0.5 * 2 / 3 + 0.5 * 2 / 8), math.log(0.5 * 1 / 3 + 0.5 * 3 / 8)]
    assert bound[0] == pytest.approx(2.0 ** -23 * sum(8 + 4 * abs(x) for x in a), rel=1e-12)


def test_permuting_a_query_leaves_the_scores():
    tokens, offsets, queries = lr.case_inputs(1000, 40)
    coll = lr.Collection(tokens, offsets, lr.NUM_WORDS)
    rs = np.random.RandomState(0)
    for q in queries:
        for method in ("jm", "dirichlet"):
            a, _, _ = lr.score_query(coll, q, method, None)
            b, _, _ = lr.score_query(coll, list(rs.permutation(q)), method, None)
            assert np.abs(a - b).max() <= 1e-12


# ---- fusion ------------------------------------------------------------------------------------------------------------------
A_IDS, A_SC = [5, 2, 9], [3.0, 2.0, 1.0]
B_IDS, B_SC = [2, 7], [-1.0, -3.0]


def test_fusion_by_hand():
    ids, sc = lr.fuse_query(A_IDS, A_SC, B_IDS, B_SC, 0.5, "standardize")
    z = 1 / math.sqrt(2 / 3)                                                              # list A: mean 2, population std sqrt(2/3)
    # document 2 is in both lists: the mean of 0.5 * 0 and 0.5 * 1; the others keep w * n undivided
    assert list(ids) == [5, 2, 7, 9]
    np.testing.assert_allclose(sc, [0.5 * z, 0.25, -0.5, -0.5 * z], rtol=1e-15)
    ids, sc = lr.fuse_query(A_IDS, A_SC, B_IDS, B_SC, 0.25, "minmax")
    assert list(ids) == [2, 5, 7, 9]                                                      # 7 and 9 tie at 0: by id
    np.testing.assert_allclose(sc, [(0.25 * 0.5 + 0.75 * 1.0) / 2, 0.25, 0.0, 0.0], rtol=1e-15)
    ids, sc = lr.fuse_query(A_IDS, A_SC, B_IDS, B_SC, 0.5, "none")
    assert list(ids) == [5, 9, 2, 7]
    np.testing.assert_allclose(sc, [1.5, 0.5, (0.5 * 2.0 + 0.5 * -1.0) / 2, -1.5], rtol=1e-15)


def test_the_two_deviations():
    for normalizer in ("standardize", "minmax"):                                          # a constant list normalises to 0
        ids, sc = lr.fuse_query([4, 1], [2.5, 2.5], B_IDS, B_SC, 0.5, normalizer)
        assert sc[list(ids).index(4)] == 0.0 and sc[list(ids).index(1)] == 0.0 and not np.isnan(sc).any()
    ids, sc = lr.fuse_query([], [], B_IDS, B_SC, 0.5, "standardize")                      # an empty list: the other alone
    assert list(ids) == [2, 7]
    np.testing.assert_allclose(sc, [0.5, -0.5], rtol=1e-15)
    ids, sc = lr.fuse_query(A_IDS, A_SC, [], [], 0.5, "minmax")
    assert list(ids) == [5, 2, 9]
    ids, sc = lr.fuse_query([], [], [], [], 0.5, "none")
    assert ids.size == 0


def test_alpha_one_without_normaliser_keeps_list_a_in_order():
    rs = np.random.RandomState(1)
    a_ids = rs.permutation(50)[:20]
    a_sc = np.sort(rs.uniform(0.1, 1.0, 20))[::-1]                                        # positive: a document only in B scores 0, below
    b_ids = rs.permutation(50)[:20]
    ids, sc = lr.fuse_query(a_ids, a_sc, b_ids, rs.standard_normal(20), 1.0, "none")
    both = np.isin(a_ids, b_ids)
    # (a document in both lists is halved — the mean over the lists that hold it — so the order is list A's within each group)
    np.testing.assert_array_equal([d for d in ids if d in set(a_ids[~both])], a_ids[~both])
    np.testing.assert_array_equal([d for d in ids if d in set(a_ids[both])], a_ids[both])
    ids, sc = lr.fuse_query(a_ids, a_sc, [], [], 1.0, "none")                             # ... and exactly list A without a list B
    np.testing.assert_array_equal(ids, a_ids)
    np.testing.assert_array_equal(sc, a_sc)


# ---- what the GPU tests rely on: the restatement alone leaves at most 1 % of the positions open ----------------------------------
@pytest.mark.parametrize("documents,queries,top_ks", lr.CASES)
def test_near_ties_are_rare_in_the_seeded_collections(documents, queries, top_ks):
    tokens, offsets, qs = lr.case_inputs(documents, queries)
    coll = lr.Collection(tokens, offsets, lr.NUM_WORDS)
    for method in ("jm", "dirichlet"):
        for param in (None, lr.EXPLICIT[method]):
            for k in top_ks:
                left, total = lr.open_share(coll, qs, method, param, k)
                assert left <= lr.SHARE * total, (method, param, k, left, total)


def test_excused_marks_both_neighbours_and_never_an_exact_tie():
    got = lr.excused([3.0, 2.0, 2.0 - 1e-9, 1.0, 1.0], 1e-6)
    assert list(got) == [False, True, True, False, False]
