"""numpy restatement of supervised run fusion (include/cunvsm_amd.h nvsm_ensemble_sweep / nvsm_rank_ensemble_cv), built from the
restatements of the fusion (tests/lexical_reference.py fuse_query) and of the metrics (tests/eval_reference.py evaluate_query):
  sweep      per alpha: fuse the two lists, cut the fused list at depth (0: no cut), evaluate
  folds      sklearn's un-shuffled KFold: contiguous, fold f holds n // F + 1 queries when f < n % F, else n // F
  mean       the training queries' values added in ascending query index one by one, then one division (not numpy's pairwise sum)
  choice     the largest mean; on an exact tie the largest alpha (Python's max() over (value, alpha) tuples)"""
import numpy as np

from tests import eval_reference as er
from tests import lexical_reference as lr


def cut(ids, depth):
    return ids if depth == 0 else ids[:depth]


def sweep_query(ids_a, scores_a, ids_b, scores_b, alphas, normalizer, judged, cutoffs=(), depth=0, has_words=True):
    """One metric dict per alpha for one query's two lists (each: the returned entries only)."""
    rows = []
    for alpha in alphas:
        ids, _ = lr.fuse_query(ids_a, scores_a, ids_b, scores_b, alpha, normalizer)
        rows.append(er.evaluate_query(cut(ids, depth), judged, cutoffs, has_words))
    return rows


def kfold(n, num_folds):
    """fold_of [n] of the un-shuffled KFold"""
    if not 2 <= num_folds <= n:
        raise ValueError("num_folds = %d outside [2, %d]" % (num_folds, n))
    sizes = [n // num_folds + (1 if f < n % num_folds else 0) for f in range(num_folds)]
    return np.repeat(np.arange(num_folds), sizes).astype(np.int32)


def shuffled_folds(n, num_folds, seed):
    """cuNVSMQuery --ensemble_seed (its --help has the rule): the topics permuted by a Fisher-Yates pass driven by
    std::minstd_rand0(seed) — x' = 16807 x mod (2^31 - 1); for i = n - 1 down to 1: j = x' % (i + 1), swap — then cut into the
    contiguous folds of kfold; seed 0: topic-file order. fold_of [n] in topic-file order."""
    order = list(range(n))
    if seed > 0:
        x = seed % 2147483647 or 1
        for i in range(n - 1, 0, -1):
            x = x * 16807 % 2147483647
            j = x % (i + 1)
            order[i], order[j] = order[j], order[i]
    fold_of = np.zeros(n, np.int32)
    fold_of[order] = kfold(n, num_folds)
    return fold_of


def sequential_mean(values):
    total = 0.0
    for v in values:
        total += float(v)
    return total / len(values)


def select(table, alphas, fold_of, num_folds):
    """table [A][Q] of the training measure -> (fold_alpha [F] float32, fold_train_measure [F] float64); an empty fold: (NaN, 0)"""
    table = np.asarray(table, np.float64)
    alphas = np.asarray(alphas, np.float32)
    fold_of = np.asarray(fold_of)
    fold_alpha = np.full(num_folds, np.nan, np.float32)
    fold_train = np.zeros(num_folds, np.float64)
    for f in range(num_folds):
        train = np.flatnonzero(fold_of != f)
        if train.size == fold_of.size:
            continue
        if train.size == 0:
            raise ValueError("fold %d holds every query" % f)
        best = max((sequential_mean(table[a, train]), float(alphas[a])) for a in range(alphas.size))
        fold_train[f], fold_alpha[f] = best[0], np.float32(best[1])
    return fold_alpha, fold_train
