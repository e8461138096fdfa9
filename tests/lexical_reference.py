"""fp64 numpy restatement of the lexical-ranking and fusion contract of include/cunvsm_amd.h (nvsm_lexical_rank, nvsm_rank_ensemble).

Corpus: a token arena of model word ids with document offsets. D_c documents, N tokens, len(d) = offsets[d + 1] - offsets[d],
tf(t, d), cf(t) and p(t) = cf(t) / N as in the header. A query is a list of word ids; a repeated word counts once per occurrence,
a word with cf = 0 (or outside [0, num_words)) is dropped, a query with nothing left retrieves nothing.
  jm         s(q, d) = sum_j log((1 - lam) tf(t_j, d) / len(d) + lam p(t_j)),        lam in (0, 1), auto 0.5
  dirichlet  s(q, d) = sum_j log((tf(t_j, d) + mu p(t_j)) / (len(d) + mu)),          mu > 0, auto N / D_c
A document is retrieved if it holds at least one remaining query term (an empty document never is); the order is score descending,
ties by ascending document id. Explicit parameters are taken at their float32 value, as the ABI carries them.
bound: |float32 score - fp64 score| <= 2^-23 sum_j (8 + (L + 2) |a_j|), a_j the fp64 terms, L the number of remaining terms.

Fusion: lists A and B of one query, weights w_A = alpha (float32), w_B = 1 - w_A. A list's scores are normalised over its returned
entries — standardize: (x - mean) / population std; minmax: (x - min) / (max - min); none: x — and a list whose scores are all equal
normalises to 0. The fused score of a document is the mean over the lists that contain it of w * normalised score. Sums run in
index order. The union is ordered by fused score descending, ties by ascending id."""
import numpy as np

EPS = 2.0 ** -23


def collection_frequencies(tokens, num_words):
    return np.bincount(np.asarray(tokens, np.int64), minlength=num_words).astype(np.int64)


def zipf_corpus(seed, num_documents, num_words, max_len=60, s=1.0):
    """(tokens int32, offsets int64) of a seeded collection: document lengths uniform in [1, max_len], word ids Zipf-distributed
    (the rarest words of a large vocabulary do not occur at all: cf = 0). What the GPU tests rank and what the CPU test checks the
    near-tie share of."""
    rs = np.random.RandomState(seed)
    lens = rs.randint(1, max_len + 1, num_documents)
    p = 1.0 / np.arange(1, num_words + 1) ** s
    p /= p.sum()
    tokens = rs.choice(num_words, size=int(lens.sum()), p=p).astype(np.int32)
    return tokens, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def zipf_queries(seed, num_queries, num_words, tokens, max_terms=3):
    """queries of 1 .. max_terms words drawn from the words that occur in the collection, every word alike (so that most terms are
    rare and a query matches a modest share of the documents; every seventeenth query is drawn from the tokens instead: frequent
    words, most documents match); every seventh query repeats a word and every fifth holds a word that does not occur, where the
    vocabulary has one"""
    rs = np.random.RandomState(seed)
    cf = collection_frequencies(tokens, num_words)
    present, absent = np.flatnonzero(cf > 0), np.flatnonzero(cf == 0)
    out = []
    for i in range(num_queries):
        n = rs.randint(1, max_terms + 1)
        q = [int(t) for t in (tokens[rs.randint(0, len(tokens), n)] if i % 17 == 5 else present[rs.randint(0, present.size, n)])]
        if i % 7 == 3:
            q.append(q[0])
        if i % 5 == 2 and absent.size:
            q.insert(rs.randint(0, len(q) + 1), int(absent[rs.randint(absent.size)]))
        out.append(q)
    return out


def parameter(method, param, num_tokens, num_documents):
    if param is None or param == 0:
        return 0.5 if method == "jm" else float(num_tokens) / float(num_documents)
    return float(np.float32(param))


class Collection:
    """a token arena with what the scorer needs of it: cf, the document lengths, and per word the documents of its occurrences"""

    def __init__(self, tokens, offsets, num_words):
        self.tokens, self.offsets = np.asarray(tokens, np.int64), np.asarray(offsets, np.int64)
        self.num_words, self.num_documents, self.num_tokens = int(num_words), self.offsets.size - 1, int(self.offsets[-1])
        self.cf = collection_frequencies(self.tokens, num_words)
        self.lens = (self.offsets[1:] - self.offsets[:-1]).astype(np.float64)
        doc_of = np.repeat(np.arange(self.num_documents), self.offsets[1:] - self.offsets[:-1])
        by_word = np.argsort(self.tokens, kind="stable")
        self._docs = doc_of[by_word]
        self._first = np.concatenate([[0], np.cumsum(self.cf)])

    def tf(self, t):
        """tf(t, d) for every document, float64"""
        return np.bincount(self._docs[self._first[t]:self._first[t + 1]], minlength=self.num_documents).astype(np.float64)


def score_query(coll, query, method, param):
    """(scores [D_c] float64, matched [D_c] bool, bound [D_c] float64) of one query over every document."""
    value = parameter(method, param, coll.num_tokens, coll.num_documents)
    terms = [int(t) for t in query if 0 <= int(t) < coll.num_words and coll.cf[int(t)] > 0]
    L = len(terms)
    D = coll.num_documents
    scores = np.zeros(D, np.float64)
    mass = np.zeros(D, np.float64)
    matched = np.zeros(D, bool)
    safe = np.where(coll.lens > 0, coll.lens, 1.0)
    for t in terms:                                  # in query order
        tf = coll.tf(t)
        p = float(coll.cf[t]) / float(coll.num_tokens)
        if method == "jm":
            a = np.log((1.0 - value) * tf / safe + value * p)
        else:
            a = np.log((tf + value * p) / (coll.lens + value))
        scores += a
        mass += 8.0 + (L + 2) * np.abs(a)
        matched |= tf > 0
    return scores, matched, EPS * mass


def rank_query(coll, query, method, param):
    """(order, scores [D_c] float64, bound [D_c]): order = EVERY matching document, score descending then id ascending; the
    ranking at top_k is order[:top_k]."""
    scores, matched, bound = score_query(coll, query, method, param)
    ids = np.flatnonzero(matched)
    return ids[np.lexsort((ids, -scores[ids]))], scores, bound


def normalise(x, normalizer):
    x = np.asarray(x, np.float64)
    n = x.size
    if n == 0 or normalizer == "none":
        return x.copy()
    if normalizer == "standardize":
        total = 0.0
        for v in x:
            total += float(v)
        mean = total / n
        sq = 0.0
        for v in x:
            sq += (float(v) - mean) * (float(v) - mean)
        std = np.sqrt(sq / n)
        return (x - mean) / std if std > 0 else np.zeros(n)
    if normalizer == "minmax":
        lo, hi = x.min(), x.max()
        return (x - lo) / (hi - lo) if hi > lo else np.zeros(n)
    raise ValueError(normalizer)


def fuse_query(ids_a, scores_a, ids_b, scores_b, alpha, normalizer):
    """ids [n], fused scores [n] float64 of the union of two lists (each: the returned entries only)."""
    w_a = float(np.float32(alpha))
    w_b = 1.0 - w_a
    na, nb = normalise(scores_a, normalizer), normalise(scores_b, normalizer)
    in_b = {int(d): i for i, d in enumerate(ids_b)}
    fused = {}
    for i, d in enumerate(ids_a):
        d = int(d)
        f = w_a * na[i]
        if d in in_b:
            f = (f + w_b * nb[in_b[d]]) / 2.0
        fused[d] = f
    for i, d in enumerate(ids_b):
        if int(d) not in fused:
            fused[int(d)] = w_b * nb[i]
    ids = np.array(sorted(fused), np.int64)
    sc = np.array([fused[int(d)] for d in ids], np.float64)
    order = np.lexsort((ids, -sc))
    return ids[order], sc[order]


def excused(scores, margin):
    """positions of a descending score list whose order the contract leaves open. Neighbours whose scores are closer than their two
    margins together (twice the bound) belong to one run; a run that holds two different scores is open as a whole — narrowed to
    float32 all of it may tie and come out by id —, a run of one exact score is decided by the id and never open."""
    scores = np.asarray(scores, np.float64)
    margin = np.broadcast_to(np.asarray(margin, np.float64), scores.shape)
    out = np.zeros(scores.size, bool)
    if scores.size > 1:
        close = np.abs(scores[:-1] - scores[1:]) < margin[:-1] + margin[1:]
        run = np.concatenate([[0], np.cumsum(~close)])                 # the run every position belongs to
        first = np.flatnonzero(np.concatenate([[True], ~close]))
        last = np.concatenate([first[1:], [scores.size]]) - 1
        out = (scores[first] != scores[last])[run]                     # descending: a run's first and last score are its extremes
    return out


# ---- the seeded collections the GPU tests rank (tests/test_gpu_lexical.py), named here so that tests/test_lexical_reference.py can
# check on the CPU what the GPU tests rely on: that the restatement alone leaves the order of at most 1 % of the positions open
NUM_WORDS = 20000
EXPLICIT = {"jm": 0.2, "dirichlet": 30.0}
# (documents, queries, top_k values)
CASES = ((1, 1, (1,)), (7, 5, (1, 7)), (1000, 300, (10, 1000)), (9001, 5, (10,)), (9001, 300, (1, 9001)))
SHARE = 0.01


def case_inputs(num_documents, num_queries):
    tokens, offsets = zipf_corpus(num_documents, num_documents, NUM_WORDS)
    queries = zipf_queries(num_documents + num_queries, num_queries, NUM_WORDS, tokens)
    return tokens, offsets, queries


def open_share(coll, queries, method, param, top_k):
    """(positions whose order the restatement leaves open, positions) among the first top_k of every query"""
    left = total = 0
    for q in queries:
        order, scores, bound = rank_query(coll, q, method, param)
        n = min(top_k, order.size)
        left += int(excused(scores[order], bound[order])[:n].sum())
        total += n
    return left, total
