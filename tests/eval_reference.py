"""fp64 numpy restatement of the metric contract of nvsm_evaluate (include/cunvsm_amd.h), for one query at a time.

For a ranking r_1 .. r_n and judged (id, grade) pairs: g(d) the judged grade (0 if unjudged), rel(d) = g(d) >= 1, R the number of
judged entries with grade >= 1 (id -1, a judged document the model does not hold, included), c_i = sum_{j <= i} rel(r_j):
  num_ret = n, num_rel = R, num_rel_ret = c_n
  map = (1 / R) sum_{i: rel(r_i)} c_i / i;  Rprec = c_min(R, n) / R;  recip_rank = 1 / min{i: rel(r_i)} (0 if none)
  P_c = c_min(c, n) / c;  recall_c = c_min(c, n) / R
  dcg@c = sum_{i <= min(c, n), g(r_i) > 0} g(r_i) / log2(i + 1);  idcg@c the same over the judged grades > 0, descending, first c
  ndcg_cut_c = dcg@c / idcg@c;  ndcg = the same without a cutoff
Every ratio with a zero denominator is 0; a query without words gets all zeros."""
import numpy as np

FIXED = ("num_ret", "num_rel", "num_rel_ret", "map", "Rprec", "recip_rank", "ndcg")
INTEGER = ("num_ret", "num_rel", "num_rel_ret")


def names(cutoffs):
    out = list(FIXED)
    for c in cutoffs:
        out += ["P_%d" % c, "recall_%d" % c, "ndcg_cut_%d" % c]
    return out


def _ratio(a, b):
    return float(a) / float(b) if b > 0 else 0.0


def evaluate_query(ranking, judged, cutoffs=(), has_words=True):
    """ranking: the retrieved document ids in rank order (only the first counts[q] slots); judged: (id, grade) pairs."""
    keys = names(cutoffs)
    if not has_words:
        return dict.fromkeys(keys, 0.0)
    ranking = np.asarray(ranking, np.int64).ravel()
    judged = np.asarray(list(judged), np.int64).reshape(-1, 2)
    n = ranking.size
    held = judged[judged[:, 0] >= 0]
    held = held[np.argsort(held[:, 0], kind="stable")]
    g = np.zeros(n, np.int64)                      # g(r_i): the judged grade, 0 if unjudged
    if held.shape[0] and n:
        at = np.minimum(np.searchsorted(held[:, 0], ranking), held.shape[0] - 1)
        g = np.where(held[at, 0] == ranking, held[at, 1], 0)
    rel = g >= 1
    R = int((judged[:, 1] >= 1).sum())
    c = np.cumsum(rel)
    i = np.arange(1, n + 1, dtype=np.float64)
    gains = np.where(g > 0, g, 0).astype(np.float64) / np.log2(i + 1.0)
    ideal = np.sort(judged[judged[:, 1] > 0, 1])[::-1].astype(np.float64)
    ideal = ideal / np.log2(np.arange(1, ideal.size + 1, dtype=np.float64) + 1.0)

    def c_at(m):
        m = min(int(m), n)
        return int(c[m - 1]) if m > 0 else 0

    out = {"num_ret": float(n), "num_rel": float(R), "num_rel_ret": float(c_at(n)),
           "map": _ratio((c[rel] / i[rel]).sum(dtype=np.float64), R), "Rprec": _ratio(c_at(R), R),
           "recip_rank": 1.0 / (int(np.flatnonzero(rel)[0]) + 1) if rel.any() else 0.0,
           "ndcg": _ratio(gains.sum(dtype=np.float64), ideal.sum(dtype=np.float64))}
    for cut in cutoffs:
        out["P_%d" % cut] = c_at(cut) / float(cut)
        out["recall_%d" % cut] = _ratio(c_at(cut), R)
        out["ndcg_cut_%d" % cut] = _ratio(gains[:cut].sum(dtype=np.float64), ideal[:cut].sum(dtype=np.float64))
    return out


def evaluate(ids, counts, judgments, cutoffs=(), has_words=None):
    """A dict of float64 arrays [Q] from rank()'s ids [Q][k] and counts [Q] and per-query judged (id, grade) lists."""
    Q = len(judgments)
    rows = [evaluate_query(ids[q][:int(counts[q])], judgments[q], cutoffs, True if has_words is None else bool(has_words[q]))
            for q in range(Q)]
    return {k: np.array([r[k] for r in rows], np.float64) for k in names(cutoffs)}
