"""The fp64 restatement of nvsm_evaluate's metric contract (tests/eval_reference.py) against cases worked by hand here."""
import math

import numpy as np
import pytest

from tests import eval_reference as er

A, B, C_, X = 10, 11, 12, 99          # three retrieved documents and one that is never retrieved


def close(got, want):
    assert got == pytest.approx(want, rel=0, abs=1e-15), (got, want)


@pytest.mark.parametrize("g3,missing_id", [(1, X), (3, -1)])
def test_two_of_three_relevant_documents_retrieved(g3, missing_id):
    """ranking [a, b, c], a and c relevant with grades 2 and 1, a third relevant document (grade g3) never retrieved — held by the
    model or not (id -1), it counts towards R = 3 either way"""
    m = er.evaluate_query([A, B, C_], [(A, 2), (C_, 1), (missing_id, g3), (B, 0)], cutoffs=(1, 2, 5))
    assert (m["num_ret"], m["num_rel"], m["num_rel_ret"]) == (3.0, 3.0, 2.0)
    close(m["map"], (1 / 1 + 2 / 3) / 3)
    close(m["Rprec"], 2 / 3)
    close(m["recip_rank"], 1.0)
    close(m["P_5"], 2 / 5)
    close(m["P_1"], 1.0)
    close(m["P_2"], 1 / 2)
    close(m["recall_2"], 1 / 3)
    close(m["recall_5"], 2 / 3)
    dcg = 2 / math.log2(2) + 1 / math.log2(4)
    assert dcg == 2.5
    ideal = sorted([2, 1, g3], reverse=True)
    idcg = sum(g / math.log2(i + 2) for i, g in enumerate(ideal))
    close(m["ndcg"], dcg / idcg)
    close(m["ndcg_cut_5"], dcg / idcg)
    close(m["ndcg_cut_1"], 2.0 / ideal[0])
    close(m["ndcg_cut_2"], 2.0 / (ideal[0] + ideal[1] / math.log2(3)))


def test_no_relevant_judgment_makes_every_ratio_zero():
    m = er.evaluate_query([A, B, C_], [(A, 0), (B, -1)], cutoffs=(2,))
    assert (m["num_ret"], m["num_rel"], m["num_rel_ret"]) == (3.0, 0.0, 0.0)
    assert all(m[k] == 0.0 for k in ("map", "Rprec", "recip_rank", "ndcg", "P_2", "recall_2", "ndcg_cut_2"))
    m = er.evaluate_query([A, B], [], cutoffs=(2,))
    assert m["num_ret"] == 2.0 and sum(m.values()) == 2.0


def test_nothing_retrieved():
    m = er.evaluate_query([], [(A, 1), (B, 2)], cutoffs=(1, 10))
    assert (m["num_ret"], m["num_rel"], m["num_rel_ret"]) == (0.0, 2.0, 0.0)
    assert all(v == 0.0 for k, v in m.items() if k != "num_rel")


def test_everything_relevant():
    m = er.evaluate_query([A, B, C_], [(A, 1), (B, 1), (C_, 1)], cutoffs=(2, 5))
    assert (m["num_ret"], m["num_rel"], m["num_rel_ret"]) == (3.0, 3.0, 3.0)
    for k in ("map", "Rprec", "recip_rank", "ndcg", "P_2", "recall_5", "ndcg_cut_2", "ndcg_cut_5"):
        close(m[k], 1.0)
    close(m["P_5"], 3 / 5)                  # always divided by the cutoff
    close(m["recall_2"], 2 / 3)


def test_first_hit_at_the_last_rank():
    m = er.evaluate_query([A, B, C_], [(C_, 2)], cutoffs=(2, 3))
    close(m["recip_rank"], 1 / 3)
    close(m["map"], 1 / 3)
    close(m["Rprec"], 0.0)                  # R = 1: only rank 1 counts
    assert m["P_2"] == 0.0 and m["ndcg_cut_2"] == 0.0
    close(m["P_3"], 1 / 3)
    close(m["ndcg"], (2 / math.log2(4)) / 2.0)


def test_more_relevant_than_retrieved_and_a_negative_grade():
    judged = [(A, 1), (B, -1), (X, 1), (X + 1, 1), (-1, 1), (-1, 1)]
    m = er.evaluate_query([B, A], judged, cutoffs=(1,))
    assert (m["num_rel"], m["num_rel_ret"]) == (5.0, 1.0)
    close(m["Rprec"], 1 / 5)                # c_min(R, n) = c_2
    close(m["map"], (1 / 2) / 5)
    assert m["P_1"] == 0.0


def test_a_query_without_words_is_all_zeros_and_the_batched_form_stacks_rows():
    ids = np.array([[A, B, C_], [C_, -1, -1]])
    res = er.evaluate(ids, [3, 1], [[(A, 1)], [(C_, 1), (X, 1)]], cutoffs=(1,), has_words=[True, True])
    assert er.names((1,)) == list(res) and list(res["num_ret"]) == [3.0, 1.0] and list(res["recall_1"]) == [1.0, 0.5]
    res = er.evaluate(ids, [3, 1], [[(A, 1)], [(C_, 1), (X, 1)]], cutoffs=(1,), has_words=[True, False])
    assert all(v[1] == 0.0 for v in res.values()) and res["num_rel"][0] == 1.0
