"""The restatement of supervised run fusion (tests/fusion_cv_reference.py) and alpha_grid on cases small enough to do by hand."""
import numpy as np
import pytest

import cunvsm_amd as ca
from tests import fusion_cv_reference as fr

# list A holds documents 0 and 1, list B documents 1 and 2; no normalisation, so the fused scores can be read off:
#   alpha 0.25: doc 0 = 0.25·4 = 1, doc 1 = (0.25·2 + 0.75·8) / 2 = 3.25, doc 2 = 0.75·4 = 3      -> 1, 2, 0
#   alpha 0.75: doc 0 = 0.75·4 = 3, doc 1 = (0.75·2 + 0.25·8) / 2 = 1.75, doc 2 = 0.25·4 = 1      -> 0, 1, 2
A = (np.array([0, 1]), np.array([4.0, 2.0], np.float32))
B = (np.array([1, 2]), np.array([8.0, 4.0], np.float32))
JUDGED = [(0, 1), (2, 0)]                   # document 0 is the relevant one


def sweep(depth, alphas=(0.25, 0.75)):
    return fr.sweep_query(A[0], A[1], B[0], B[1], alphas, "none", JUDGED, cutoffs=(1, 2), depth=depth)


def test_the_order_flips_between_a_quarter_and_three_quarters():
    low, high = sweep(0)
    assert (low["map"], low["recip_rank"], low["P_1"], low["P_2"], low["num_ret"]) == (1.0 / 3.0, 1.0 / 3.0, 0.0, 0.0, 3.0)
    assert (high["map"], high["recip_rank"], high["P_1"], high["P_2"], high["num_ret"]) == (1.0, 1.0, 1.0, 0.5, 3.0)
    assert low["ndcg"] == pytest.approx(1.0 / np.log2(4.0)) and high["ndcg"] == 1.0


def test_depth_one_the_list_length_and_beyond():
    low, high = sweep(1)
    assert (low["num_ret"], low["map"], low["num_rel"], low["num_rel_ret"]) == (1.0, 0.0, 1.0, 0.0)      # the cut list is [1]
    assert (high["num_ret"], high["map"], high["num_rel_ret"]) == (1.0, 1.0, 1.0)                       # ... is [0]
    assert sweep(3) == sweep(0) == sweep(4)
    two = sweep(2)
    assert two[0]["num_ret"] == 2.0 and two[0]["map"] == 0.0 and two[1]["map"] == 1.0


def test_seven_queries_in_three_folds():
    fold_of = fr.kfold(7, 3)
    assert fold_of.tolist() == [0, 0, 0, 1, 1, 2, 2]
    assert np.bincount(fr.kfold(23, 5)).tolist() == [5, 5, 5, 4, 4]
    assert fr.kfold(4, 4).tolist() == [0, 1, 2, 3]
    for bad in ((3, 1), (3, 4)):
        with pytest.raises(ValueError):
            fr.kfold(*bad)


def test_the_mean_is_sequential():
    values = [1e16, 1.0, -1e16, 1.0]
    assert fr.sequential_mean(values) == 0.25                            # ((1e16 + 1) − 1e16) + 1 = 1: the first 1 is absorbed
    assert fr.sequential_mean([0.1, 0.2, 0.3]) == ((0.1 + 0.2) + 0.3) / 3


def test_the_best_training_measure_wins_and_a_tie_selects_the_largest_alpha():
    alphas = ca.alpha_grid(0.05)
    fold_of = fr.kfold(7, 3)
    tie = np.full((alphas.size, 7), 0.375)
    fold_alpha, fold_train = fr.select(tie, alphas, fold_of, 3)
    assert (fold_alpha == np.float32(0.95)).all() and (fold_train == 0.375).all()
    tie = np.full((3, 7), 0.5)                                              # ... whatever the order of the grid
    assert (fr.select(tie, np.array([0.5, 0.75, 0.25], np.float32), fold_of, 3)[0] == np.float32(0.75)).all()
    # queries 0-2 like alpha[1], queries 3-6 alpha[0]: fold 0 (trained on 3-6) picks alpha[0], the others see 3 against 2 or 2 against 2
    table = np.zeros((2, 7))
    table[1, :3] = 1.0
    table[0, 3:] = 1.0
    fold_alpha, fold_train = fr.select(table, np.array([0.2, 0.6], np.float32), fold_of, 3)
    assert fold_alpha.tolist() == [np.float32(0.2), np.float32(0.6), np.float32(0.6)]
    assert fold_train.tolist() == [1.0, 3.0 / 5.0, 3.0 / 5.0]
    # an empty fold
    fold_alpha, fold_train = fr.select(table, np.array([0.2, 0.6], np.float32), [0, 0, 0, 2, 2, 2, 2], 3)
    assert np.isnan(fold_alpha[1]) and fold_train[1] == 0.0 and fold_alpha[0] == np.float32(0.2) and fold_alpha[2] == np.float32(0.6)


def test_alpha_grid():
    g = ca.alpha_grid(0.01)
    assert g.dtype == np.float32 and g.size == 100 and g[0] == 0.0 and g[-1] == np.float32(0.99)
    np.testing.assert_array_equal(g, np.arange(0.0, 1.0, 0.01).astype(np.float32))
    assert ca.alpha_grid(0.05).size == 20 and ca.alpha_grid(0.05)[-1] == np.float32(0.95)
    assert ca.alpha_grid(0.3).tolist() == [0.0, np.float32(0.3), np.float32(0.6), np.float32(0.9)]
    assert ca.alpha_grid(1.0).tolist() == [0.0]
    for bad in (0.0005, 0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ca.alpha_grid(bad)
