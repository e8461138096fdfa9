"""nvsm_rank_ensemble_cv on the GPU: the choice of every fold against the restatement (tests/fusion_cv_reference.py) applied to the
sweep table the GPU returned — exactly, the selection is a host function of that table's bits —, every query's list against
nvsm_rank_ensemble at its fold's alpha bit for bit, and the returned metrics against nvsm_ensemble_sweep's rows."""
import numpy as np
import pytest

import cunvsm_amd as ca
from tests import fusion_cv_reference as fr
from tests.test_gpu_ensemble import CUTOFFS, queries_for
from tests.test_gpu_fusion_sweep import NAMES, judgments_for, model, same_rows
from tests.test_gpu_rank import bits

pytestmark = pytest.mark.gpu

D, Q, K = 300, 23, 20
GRID = ca.alpha_grid(0.05)


def setup():
    m, tokens, offsets = model(D)
    return m, queries_for(tokens, Q, 31), judgments_for(Q, D, 41)


def check_lists(m, qs, fold_of, fold_alpha, ids, scores, counts, **kw):
    """every query's list is rank_ensemble's at its fold's alpha"""
    for alpha in np.unique(fold_alpha[~np.isnan(fold_alpha)]):
        r_ids, r_sc, r_n = m.rank_ensemble(qs, alpha=float(alpha), top_k=K, **kw)
        at = np.flatnonzero(fold_alpha[fold_of] == alpha)
        assert at.size
        np.testing.assert_array_equal(ids[at], r_ids[at])
        np.testing.assert_array_equal(bits(scores[at]), bits(r_sc[at]))
        np.testing.assert_array_equal(counts[at], r_n[at])


@pytest.mark.parametrize("measure", ["map", "ndcg", "P_5"])
@pytest.mark.parametrize("num_folds", [2, 5, 23])
def test_folds_choice_lists_and_metrics(num_folds, measure):
    m, qs, judged = setup()
    depth = 30
    fold_alpha, fold_train, metrics, ids, scores, counts, table = m.rank_ensemble_cv(
        qs, judged, stepsize=0.05, num_folds=num_folds, measure=measure, depth=depth, top_k=K, cutoffs=CUTOFFS, return_sweep=True)
    assert fold_alpha.shape == fold_train.shape == (num_folds,) and fold_alpha.dtype == np.float32 and fold_train.dtype == np.float64
    assert ids.shape == scores.shape == (Q, 2 * K) and list(metrics) == list(table) == NAMES
    same_rows(table, m.ensemble_sweep(qs, judged, GRID, depth=depth, top_k=K, cutoffs=CUTOFFS), "the sweep table")
    fold_of = fr.kfold(Q, num_folds)
    want_alpha, want_train = fr.select(table[measure], GRID, fold_of, num_folds)
    np.testing.assert_array_equal(bits(fold_alpha), bits(want_alpha))
    np.testing.assert_array_equal(bits(fold_train), bits(want_train))
    check_lists(m, qs, fold_of, fold_alpha, ids, scores, counts)
    index = np.array([int(np.flatnonzero(GRID == a)[0]) for a in fold_alpha])[fold_of]
    same_rows(metrics, {n: v[index, np.arange(Q)] for n, v in table.items()}, "the returned metrics")
    print("cv F=%d %s: alphas %s" % (num_folds, measure, sorted(set(fold_alpha.tolist()))))


def test_explicit_folds_one_of_them_empty_and_feedback():
    m, qs, judged = setup()
    fold_of = (np.arange(Q) * 7 % 3) * 2                                  # folds 0, 2 and 4 of five: 1 and 3 are empty
    fold_alpha, fold_train, metrics, ids, scores, counts, table = m.rank_ensemble_cv(
        qs, judged, alphas=GRID[::-1], num_folds=5, measure="ndcg_cut_10", depth=0, fold_of=fold_of, top_k=K, cutoffs=CUTOFFS,
        feedback=True, normalizer="minmax", return_sweep=True)
    assert np.isnan(fold_alpha[[1, 3]]).all() and (fold_train[[1, 3]] == 0.0).all() and not np.isnan(fold_alpha[[0, 2, 4]]).any()
    want_alpha, want_train = fr.select(table["ndcg_cut_10"], GRID[::-1], fold_of, 5)
    np.testing.assert_array_equal(bits(fold_alpha), bits(want_alpha))
    np.testing.assert_array_equal(bits(fold_train), bits(want_train))
    check_lists(m, qs, fold_of, fold_alpha, ids, scores, counts, feedback=True, normalizer="minmax")
    ens = {a: m.rank_ensemble(qs, alpha=float(a), top_k=K, judgments=judged, cutoffs=CUTOFFS, feedback=True, normalizer="minmax")[0]
           for a in np.unique(fold_alpha[[0, 2, 4]])}
    for i in range(Q):                      # depth 0: the metrics are rank_ensemble's own
        for n in NAMES:
            assert bits(metrics[n][i:i + 1]) == bits(ens[fold_alpha[fold_of[i]]][n][i:i + 1]), (n, i)


def test_judgments_under_which_every_alpha_scores_the_same_select_the_largest():
    m, qs, _ = setup()
    judged = [[(-1, 1)] for _ in range(Q)]                                # one relevant document the model does not hold: every measure is 0
    fold_alpha, fold_train, metrics, ids, scores, counts = m.rank_ensemble_cv(qs, judged, stepsize=0.05, num_folds=5, top_k=K, cutoffs=CUTOFFS)
    assert (fold_alpha == np.float32(0.95)).all() and (fold_train == 0.0).all()
    check_lists(m, qs, fr.kfold(Q, 5), fold_alpha, ids, scores, counts)
