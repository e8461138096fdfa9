"""fp64 numpy restatement of the weighted query likelihood, the relevance model and the RM3 expansion of include/cunvsm_amd.h
(nvsm_lexical_rank_weighted, nvsm_relevance_model, nvsm_lexical_rank_prf). The collection, cf, p(t), len(d), tf, the smoothing
methods and "auto" are those of tests/lexical_reference.py.

Weighted query likelihood: the terms t_j carry float32 weights w_j >= 0; a term with cf = 0 (or outside the vocabulary) or w_j = 0 is
dropped; s(q, d) = sum_j w_j a_j(d), a_j the Jelinek-Mercer or Dirichlet log term, summed in query order; a document is retrieved if
it holds at least one remaining term. bound: |float32 score - s| <= 2^-23 |s| (every a_j <= 0, every w_j >= 0: nothing cancels).

Relevance model of a first-pass list d_0 .. d_{n-1} with float32 scores s_0 >= ...: w_i = exp(s_i - s_0) (w_0 = 1),
pi(t) = (sum_i w_i tf(t, d_i) / len(d_i)) / sum_i w_i, both sums in rank order; pi is narrowed to float32; the expansion terms are
the fb_terms terms of largest float32 pi > 0, ties by ascending word id. bound: |float32 pi - pi| <= 2^-23 pi + 2^-149.

Expansion: o = float32 orig_weight as a double, L the number of remaining original terms; these first, in query order, each with
weight float32(o / L); then the expansion terms in rank order with weights float32(((1 - o) pi_i) / S), S = sum_i pi_i in rank order.
A query without remaining terms stays empty."""
import numpy as np

from tests import lexical_reference as lr

EPS = lr.EPS
TINY = 2.0 ** -149


def remaining(coll, query):
    return [int(t) for t in query if 0 <= int(t) < coll.num_words and coll.cf[int(t)] > 0]


def weighted_score_query(coll, query, weights, method, param):
    """(scores [D_c] float64, matched [D_c] bool, bound [D_c] float64) of one weighted query over every document."""
    value = lr.parameter(method, param, coll.num_tokens, coll.num_documents)
    D = coll.num_documents
    scores = np.zeros(D, np.float64)
    matched = np.zeros(D, bool)
    safe = np.where(coll.lens > 0, coll.lens, 1.0)
    for t, w in zip(query, weights):                 # in query order
        t, w = int(t), float(np.float32(w))
        if not (0 <= t < coll.num_words and coll.cf[t] > 0) or w == 0.0:
            continue
        tf = coll.tf(t)
        p = float(coll.cf[t]) / float(coll.num_tokens)
        if method == "jm":
            a = np.log((1.0 - value) * tf / safe + value * p)
        else:
            a = np.log((tf + value * p) / (coll.lens + value))
        scores += w * a
        matched |= tf > 0
    return scores, matched, EPS * np.abs(scores)


def weighted_rank_query(coll, query, weights, method, param):
    """(order, scores, bound) as lexical_reference.rank_query: order = every matching document, best first"""
    scores, matched, bound = weighted_score_query(coll, query, weights, method, param)
    ids = np.flatnonzero(matched)
    return ids[np.lexsort((ids, -scores[ids]))], scores, bound


def relevance_model(coll, doc_ids, doc_scores, fb_terms):
    """(term ids [<= fb_terms] best first, pi [num_words] float64, bound [num_words]) of one query's first-pass list (the returned
    entries only, scores as float32)"""
    V = coll.num_words
    acc = np.zeros(V, np.float64)
    n = len(doc_ids)
    if n == 0:
        return np.zeros(0, np.int64), acc, np.full(V, TINY)
    s = np.asarray(doc_scores, np.float32).astype(np.float64)
    total = 0.0
    for i, d in enumerate(doc_ids):                  # in rank order
        w = 1.0 if i == 0 else float(np.exp(s[i] - s[0]))
        lo, hi = int(coll.offsets[d]), int(coll.offsets[d + 1])
        tf = np.bincount(coll.tokens[lo:hi], minlength=V).astype(np.float64)
        acc += w * (tf / float(hi - lo))
        total += w
    pi = acc / total
    narrowed = pi.astype(np.float32)
    cand = np.flatnonzero(narrowed > 0)
    order = cand[np.lexsort((cand, -narrowed[cand].astype(np.float64)))][:fb_terms]
    return order, pi, EPS * pi + TINY


def expand(coll, query, term_ids, term_probs, orig_weight):
    """(word ids, float32 weights) of the RM3 query; term_probs: the float32 probabilities of term_ids, in rank order"""
    orig = remaining(coll, query)
    if not orig:
        return [], np.zeros(0, np.float32)
    o = float(np.float32(orig_weight))
    weights = [np.float32(o / float(len(orig)))] * len(orig)
    S = 0.0
    for p in term_probs:
        S += float(np.float32(p))
    for p in term_probs:
        weights.append(np.float32(((1.0 - o) * float(np.float32(p))) / S))
    return orig + [int(t) for t in term_ids], np.array(weights, np.float32)


def first_pass(coll, query, method, param, fb_docs):
    """the restatement's own first pass: (ids, float32 scores) of the fb_docs best documents — what the CPU tests feed the relevance
    model with; the GPU tests feed it the GPU's list"""
    order, scores, _ = lr.rank_query(coll, query, method, param)
    top = order[:fb_docs]
    return top, scores[top].astype(np.float32)


# ---- the cases of tests/test_gpu_prf.py, named here so that tests/test_prf_reference.py can check on the CPU what the GPU tests rely
# on: that the restatement alone leaves at most 1 % of the positions open
NUM_WORDS = lr.NUM_WORDS
METHODS = (("jm", None), ("dirichlet", None))
FEEDBACK = ((1, 1), (3, 10), (10, 10))               # (fb_docs, fb_terms)
CASES = ((1, 1), (7, 5), (1000, 300), (9001, 300))   # (documents, queries) of lexical_reference.case_inputs
TOP_KS = (10, 100)
ORIG_WEIGHT = 0.5
SHARE = lr.SHARE


def fb_of(documents, fb):
    """the feedback sizes a collection admits: fb_docs <= num_documents"""
    return min(fb[0], documents), fb[1]


def open_shares(coll, queries, method, param, fb_docs, fb_terms, orig_weight, top_ks):
    """((open positions, positions) of the relevance model's term lists, {top_k: (open positions, positions) among the first top_k of
    the expanded queries' rankings}), every stage fed by the restatement's own previous stage"""
    a_left = a_total = 0
    b = {k: [0, 0] for k in top_ks}
    for q in queries:
        ids, sc = first_pass(coll, q, method, param, fb_docs)
        terms, pi, bound = relevance_model(coll, ids, sc, fb_terms)
        cand = np.flatnonzero(pi.astype(np.float32) > 0)
        full = cand[np.lexsort((cand, -pi[cand]))]
        a_left += int(lr.excused(pi[full], bound[full])[:terms.size].sum())
        a_total += int(terms.size)
        words, weights = expand(coll, q, terms, pi[terms].astype(np.float32), orig_weight)
        order, scores, bound = weighted_rank_query(coll, words, weights, method, param)
        open_ = lr.excused(scores[order], bound[order])
        for k in top_ks:
            n = min(k, order.size)
            b[k][0] += int(open_[:n].sum())
            b[k][1] += n
    return (a_left, a_total), {k: tuple(v) for k, v in b.items()}
