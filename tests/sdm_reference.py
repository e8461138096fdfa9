"""fp64 numpy restatement of the sequential-dependence contract of include/cunvsm_amd.h (nvsm_sdm_rank, nvsm_sdm_pair_counts), written
from the contract's sentences. The collection, cf, p, len, the smoothing parameter and "auto" are lexical_reference's.

A query t_1 .. t_L as given has the pairs (t_j, t_{j+1}). For a pair (a, b) and a window W:
  od(a, b; d)  positions i with tok_i = a and tok_{i+1} = b, both inside d
  uw(a, b; d)  positions i with tok_i in {a, b} such that some j, i < j < i + W, inside d, holds the other term (a itself when a = b):
               a position counts once however many such j there are
cf_o, cf_u are their sums over the collection. Groups T (terms with cf > 0), O (pairs with cf_o > 0), U (pairs with cf_u > 0), each in
query order; a member's value is lexical_reference's log term with its count in place of tf and cf_x / N in place of p;
g_G = (sum of the members in order) / n_G and s = sum over the present groups (n_G > 0 and w_G > 0), in the order T, O, U, of
(w_G / sum of the present weights) * g_G, the weights float32 widened. A document is retrieved if it holds a remaining term.
bound: |float32 score - fp64 score| <= 2^-23 |fp64 score|."""
import numpy as np

from tests import lexical_reference as lr

EPS = lr.EPS
DEFAULT_WEIGHTS = (0.85, 0.10, 0.05)


class Positions:
    """a lexical_reference.Collection with the order of its tokens: per position its document's end, per word its positions"""

    def __init__(self, coll):
        self.coll = coll
        lens = coll.offsets[1:] - coll.offsets[:-1]
        self.doc_of = np.repeat(np.arange(coll.num_documents), lens)
        self.end_of = np.repeat(coll.offsets[1:], lens)              # the first position behind the position's document
        order = np.argsort(coll.tokens, kind="stable")
        self._pos = order                                            # positions grouped by word, ascending inside a word
        self._first = np.concatenate([[0], np.cumsum(coll.cf)])
        self._pairs = {}

    def positions(self, t):
        return self._pos[self._first[t]:self._first[t + 1]]

    def _next_within(self, at, other, window):
        """for every position in `at`: does a position of `other` lie in (i, i + window) before the end of i's document"""
        if at.size == 0 or other.size == 0:
            return np.zeros(at.size, bool)
        nxt = np.searchsorted(other, at, side="right")               # the first position of `other` strictly behind i
        ok = nxt < other.size
        j = other[np.minimum(nxt, other.size - 1)]
        return ok & (j < at + window) & (j < self.end_of[at])

    def pair_counts(self, a, b, window):
        """(od [D] int64, uw [D] int64) of the pair (a, b) per document; zeros where a term is not a word of the collection"""
        key = (int(a), int(b), int(window))
        if key not in self._pairs:
            D, V = self.coll.num_documents, self.coll.num_words
            od, uw = np.zeros(D, np.int64), np.zeros(D, np.int64)
            if 0 <= a < V and 0 <= b < V:
                pa, pb = self.positions(a), self.positions(b)
                hit = self._next_within(pa, pb, 2)                   # the very next position, inside the document
                od = np.bincount(self.doc_of[pa[hit]], minlength=D).astype(np.int64)
                hit_a = self._next_within(pa, pb, window)
                uw = np.bincount(self.doc_of[pa[hit_a]], minlength=D).astype(np.int64)
                if a != b:
                    hit_b = self._next_within(pb, pa, window)
                    uw = uw + np.bincount(self.doc_of[pb[hit_b]], minlength=D).astype(np.int64)
            self._pairs[key] = (od, uw)
        return self._pairs[key]


def query_pairs(query):
    return [(int(query[j]), int(query[j + 1])) for j in range(len(query) - 1)]


def pair_counts(pos, queries, window):
    """(cf_o, cf_u) uint64 of every pair of every query, in query order: nvsm_sdm_pair_counts"""
    o, u = [], []
    for q in queries:
        for a, b in query_pairs(q):
            od, uw = pos.pair_counts(a, b, window)
            o.append(int(od.sum()))
            u.append(int(uw.sum()))
    return np.array(o, np.uint64), np.array(u, np.uint64)


def _feature(count, held, value, method, coll):
    p = float(held) / float(coll.num_tokens)
    if method == "jm":
        safe = np.where(coll.lens > 0, coll.lens, 1.0)
        return np.log((1.0 - value) * count / safe + value * p)
    return np.log((count + value * p) / (coll.lens + value))


def score_query(pos, query, method, param, weights=DEFAULT_WEIGHTS, window=8):
    """(scores [D] float64, matched [D] bool, bound [D]) of one query over every document"""
    coll = pos.coll
    value = lr.parameter(method, param, coll.num_tokens, coll.num_documents)
    D = coll.num_documents
    groups = [[], [], []]
    matched = np.zeros(D, bool)
    with np.errstate(divide="ignore"):
        for t in query:                                              # T, in query order
            t = int(t)
            if 0 <= t < coll.num_words and coll.cf[t] > 0:
                tf = coll.tf(t)
                matched |= tf > 0
                groups[0].append(_feature(tf, coll.cf[t], value, method, coll))
        for a, b in query_pairs(query):                              # O and U, in query order
            od, uw = pos.pair_counts(a, b, window)
            if od.sum() > 0:
                groups[1].append(_feature(od.astype(np.float64), od.sum(), value, method, coll))
            if uw.sum() > 0:
                groups[2].append(_feature(uw.astype(np.float64), uw.sum(), value, method, coll))
    w = [float(np.float32(x)) for x in weights]
    present = [g for g in range(3) if groups[g] and w[g] > 0.0]
    total = 0.0
    for g in present:
        total += w[g]
    scores = np.zeros(D, np.float64)
    for g in present:
        s = np.zeros(D, np.float64)
        for a in groups[g]:
            s = s + a
        scores = scores + (w[g] / total) * (s / float(len(groups[g])))
    scores = np.where(matched, scores, 0.0)                          # (an empty document's terms are not numbers; it is never retrieved)
    return scores, matched, EPS * np.abs(scores)


def rank_query(pos, query, method, param, weights=DEFAULT_WEIGHTS, window=8):
    """(order, scores [D] float64, bound [D]): order = every retrieved document, score descending then id ascending"""
    scores, matched, bound = score_query(pos, query, method, param, weights, window)
    ids = np.flatnonzero(matched)
    return ids[np.lexsort((ids, -scores[ids]))], scores, bound


def open_share(pos, queries, method, param, top_k, weights=DEFAULT_WEIGHTS, window=8):
    """(positions whose order the restatement leaves open, positions) among the first top_k of every query"""
    left = total = 0
    for q in queries:
        order, scores, bound = rank_query(pos, q, method, param, weights, window)
        n = min(top_k, order.size)
        left += int(lr.excused(scores[order], bound[order])[:n].sum())
        total += n
    return left, total


# ---- the inputs the GPU tests rank (tests/test_gpu_sdm.py), named here so that tests/test_sdm_reference.py can check on the CPU what
# they rely on: that the restatement alone leaves the order of at most lexical_reference.SHARE of the positions open
NUM_WORDS = 300          # small enough that pairs of query words recur in the collection
CASES = ((1, 1, (1,)), (7, 5, (1, 7)), (1000, 300, (10, 1000)), (9001, 5, (10,)), (9001, 300, (1, 9001)))
WINDOWS = (2, 8, 64)     # 64: NVSM_SDM_MAX_WINDOW


def seeded_queries(seed, num_queries, tokens, offsets, num_words):
    """queries of 1 .. 4 words: three in four are a run of adjacent tokens of one document (their pairs occur), the others words that
    occur, drawn alike; every seventh query repeats its first pair, every fifth holds a word that does not occur in its middle, every
    eleventh is one word, every thirteenth is empty"""
    rs = np.random.RandomState(seed)
    cf = lr.collection_frequencies(tokens, num_words)
    present, absent = np.flatnonzero(cf > 0), np.flatnonzero(cf == 0)
    lens = offsets[1:] - offsets[:-1]
    out = []
    for i in range(num_queries):
        n = rs.randint(1, 5)
        d = rs.randint(0, lens.size)
        if i % 4 != 3 and lens[d] >= n:
            s = offsets[d] + rs.randint(0, lens[d] - n + 1)
            q = [int(t) for t in tokens[s:s + n]]
        else:
            q = [int(t) for t in present[rs.randint(0, present.size, n)]]
        if i % 7 == 3 and len(q) >= 2:
            q = q + q[:2]
        if i % 5 == 2 and absent.size and len(q) >= 2:
            q.insert(rs.randint(1, len(q)), int(absent[rs.randint(absent.size)]))
        if i % 11 == 6:
            q = q[:1]
        if i % 13 == 9 and num_queries > 1:
            q = []
        out.append(q)
    return out


def case_inputs(num_documents, num_queries):
    tokens, offsets = lr.zipf_corpus(1000 + num_documents, num_documents, NUM_WORDS)
    queries = seeded_queries(2000 + num_documents + num_queries, num_queries, tokens, offsets, NUM_WORDS)
    return tokens, offsets, queries


def hand_built(window):
    """(tokens, offsets, notes) of the hand-built collection for one window W: every document shape the kernel treats differently.
    Words 1 and 2 are the pair under test (a, b), word 3 makes the a = a runs, word 0 and words >= 10 are filler; notes names the
    documents the tests look at."""
    W = int(window)
    rs = np.random.RandomState(17)
    fill = lambda n: [int(t) for t in rs.randint(10, 40, n)]
    def doc(n, marks):                                               # a filler document of n tokens with marked positions
        d = fill(n)
        for i, t in marks.items():
            d[i] = t
        return d
    docs, notes = [], {}
    def add(name, d):
        notes[name] = len(docs)
        docs.append(d)
    add("empty0", [])
    add("empty1", [])                                                # two empty documents in a row
    add("one", [1])                                                  # length 1
    add("len255", doc(255, {253: 1, 254: 2}))                        # the pair at the document's end
    add("len256", doc(256, {254: 1, 255: 2}))
    add("len257", doc(257, {255: 1, 256: 2}))                        # straddles the tile boundary, a first, distance 1
    add("len256w", doc(256 + W - 1, {255: 2, 255 + W - 1: 1}))       # straddles, b first, distance W - 1, b's look-ahead ends at the document's end
    add("long", doc(5000, {255: 2, 256: 1, 511: 1, 511 + W - 1: 2, 1000: 1, 1000 + W: 2, 2047: 1, 2048: 2, 4998: 2, 4999: 1}))
    add("exact_w", doc(3 * W + 3, {1: 1, 1 + W: 2}))                 # a distance of exactly W: must not count
    add("last_a", doc(40, {39: 1}))                                  # a as the last token ...
    add("first_b", doc(40, {0: 2}))                                  # ... b as the next document's first: must not count
    add("runs", [3, 3, 3, 11, 3, 12, 12, 3, 3])                      # a = a pairs, runs
    add("both", [1, 2, 1, 2, 2, 1])
    while len(docs) < 4095:                                          # short filler documents up to the slab boundary (slabs of 4096)
        docs.append(fill(rs.randint(1, 6)))
    add("slab_last", doc(30, {3: 1, 4: 2, 20: 3, 21: 3}))            # the last document of the first slab and
    add("slab_first", doc(30, {3: 2, 4: 1, 9: 1, 10: 2}))            # the first of the second both match
    for _ in range(20):
        docs.append(fill(rs.randint(1, 6)))
    add("last", doc(12, {10: 1, 11: 2}))                             # the last document of the corpus, the pair at its very end
    tokens = np.array([t for d in docs for t in d], np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    return tokens, offsets, notes


HAND_WORDS = 50
# a repeated word, a repeated pair, an absent word in the middle (both pairs around it drop), one term, no term, an a = a pair,
# pairs in both orders, filler pairs
HAND_QUERIES = [[1, 2], [2, 1], [3, 3], [1, 2, 1, 2], [1, 1, 2], [1, 49, 2], [1], [], [49], [3, 3, 3], [12, 12, 3], [1, 2, 3, 3],
                [10, 11, 12, 13], [2, 48, 47, 1], [1, 2, 2, 1, 3]]
