"""fp64 numpy restatement of the TF-IDF contract of include/cunvsm_amd.h (nvsm_tfidf_rank), written from the header.

Corpus, D_c, N, len(d) and tf(t, d) as in tests/lexical_reference.py. df(t) = documents with tf(t, d) >= 1; avgdl = N / D_c with empty
documents counted. A query is a list of word ids with optional float32 weights w_j >= 0 (None: every w_j = 1).
  term value   a_j(d) = idf(t_j) tf (k1 + 1) / (tf + k1 (1 - b + b len(d) / avgdl)),   k1 auto 1.2, b auto 0.75
  robertson    idf = ln((D_c + 1) / (df + 0.5))
  okapi        idf = ln((D_c - df + 0.5) / (df + 0.5))          (negative for df > D_c / 2, as it is)
  score        s(q, d) = sum_j w_j a_j(d) in query order, a repeated word once per occurrence; a word with df = 0, outside
               [0, num_words) or of weight 0 is dropped; a query with nothing left retrieves nothing
A document is retrieved if it holds at least one remaining term; the order is score descending, ties by ascending document id.
Explicit parameters and weights are taken at their float32 value, as the ABI carries them.
bound: |float32 score - exact score| <= 2^-23 sum_j |w_j a_j|."""
import numpy as np

from tests import lexical_reference as lr

EPS = 2.0 ** -23


def document_frequencies(tokens, offsets, num_words):
    tokens, offsets = np.asarray(tokens, np.int64), np.asarray(offsets, np.int64)
    doc_of = np.repeat(np.arange(offsets.size - 1), offsets[1:] - offsets[:-1])
    pairs = np.unique(doc_of * int(num_words) + tokens)                 # one entry per (document, word) that occurs
    return np.bincount(pairs % int(num_words), minlength=num_words).astype(np.int64)


def idf_values(df, num_documents, idf):
    df, D = np.asarray(df, np.float64), float(num_documents)
    if idf == "robertson":
        return np.log((D + 1.0) / (df + 0.5))
    if idf == "okapi":
        return np.log((D - df + 0.5) / (df + 0.5))
    raise ValueError(idf)


def parameters(k1, b):
    return (1.2 if k1 is None or k1 == 0 else float(np.float32(k1))), (0.75 if b is None or b == 0 else float(np.float32(b)))


class Collection(lr.Collection):
    """lexical_reference's view of a token arena plus the df table"""

    def __init__(self, tokens, offsets, num_words):
        super().__init__(tokens, offsets, num_words)
        self.df = document_frequencies(tokens, offsets, num_words)


def score_query(coll, query, weights=None, k1=None, b=None, idf="robertson"):
    """(scores [D_c] float64, matched [D_c] bool, bound [D_c] float64) of one query over every document."""
    k1, b = parameters(k1, b)
    D = coll.num_documents
    avgdl = float(coll.num_tokens) / float(D)
    scores, mass, matched = np.zeros(D, np.float64), np.zeros(D, np.float64), np.zeros(D, bool)
    norm = k1 * (1.0 - b + b * coll.lens / avgdl) if coll.num_tokens > 0 else np.zeros(D)
    for j, t in enumerate(query):                                    # in query order
        t = int(t)
        w = 1.0 if weights is None else float(np.float32(weights[j]))
        if not 0 <= t < coll.num_words or coll.df[t] == 0 or w == 0.0:
            continue
        tf = coll.tf(t)
        held = tf > 0
        a = np.zeros(D, np.float64)
        a[held] = float(idf_values(coll.df[t], D, idf)) * tf[held] * (k1 + 1.0) / (tf[held] + norm[held])
        scores += w * a
        mass += np.abs(w * a)
        matched |= held
    return scores, matched, EPS * mass


def rank_query(coll, query, weights=None, k1=None, b=None, idf="robertson"):
    """(order, scores [D_c] float64, bound [D_c]): order = EVERY matching document, score descending then id ascending; the ranking
    at top_k is order[:top_k]."""
    scores, matched, bound = score_query(coll, query, weights, k1, b, idf)
    ids = np.flatnonzero(matched)
    return ids[np.lexsort((ids, -scores[ids]))], scores, bound


# ---- the collection the GPU tests rank (tests/test_gpu_tfidf.py), named here so that tests/test_tfidf_reference.py can check on the
# CPU what they rely on: that the restatement alone leaves the order of at most 1 % of the (query, rank) slots open.
# SEED was settled on the CPU by that test's own measure (open_share below): with it no slot at all is open, for either idf, weighted
# or not, at the automatic and at the explicit parameters.
NUM_WORDS = 300
ZIPF_WORDS = 296                          # the seeded part draws from these; the four words behind them are placed by hand
W_ALL, W_HALF, W_EDGE, W_ABSENT = 296, 297, 298, 299
SEED = 1
SHARE = 0.01
IDFS = ("robertson", "okapi")
EXPLICIT = dict(k1=0.9, b=0.4)


def gpu_corpus():
    """(tokens int32, offsets int64): about 70 seeded Zipf documents over 296 words, every one of them extended with W_ALL and two of
    three with W_HALF; then an empty document, a one-token document, and a document of more than 2 x 256 tokens whose first and last
    token are W_EDGE, which occurs nowhere else in it. W_ABSENT occurs nowhere."""
    tokens, offsets = lr.zipf_corpus(SEED, 70, ZIPF_WORDS)
    docs = [list(tokens[offsets[d]:offsets[d + 1]]) for d in range(offsets.size - 1)]
    for d, doc in enumerate(docs):
        doc.insert(len(doc) // 2, W_ALL)
        if d % 3 != 2:
            doc.append(W_HALF)
    rs = np.random.RandomState(SEED + 1000)
    long_doc = [W_EDGE] + [int(t) for t in rs.randint(0, ZIPF_WORDS, 600)] + [W_ALL, W_EDGE]
    docs += [[], [W_ALL], long_doc, [W_EDGE, 3, W_ALL]]
    flat = np.array([t for doc in docs for t in doc], np.int32)
    return flat, np.concatenate([[0], np.cumsum([len(doc) for doc in docs])]).astype(np.int64)


def gpu_queries(tokens):
    """seeded queries (repeated words and absent words among them: lexical_reference.zipf_queries) and the hand-made ones: the word of
    every document, the word of most, the long document's edge word once and twice, only an absent word, no words, a mixture"""
    seeded = lr.zipf_queries(SEED + 2000, 40, NUM_WORDS, tokens)
    return seeded + [[W_ALL], [W_HALF, 3], [W_EDGE], [W_EDGE, W_EDGE], [W_ABSENT], [], [W_ALL, W_HALF, W_EDGE, 5, 5], [W_ABSENT, 7]]


def gpu_weights(queries, seed=SEED + 3000):
    """float32 weights >= 0 for every word of every query, a zero among them now and then"""
    rs = np.random.RandomState(seed)
    return [np.where(rs.rand(len(q)) < 0.1, 0.0, rs.rand(len(q)) * 2.0).astype(np.float32) for q in queries]


def open_share(coll, queries, weights, top_k, **params):
    """(slots whose order the restatement leaves open, slots) among the first top_k of every query"""
    left = total = 0
    for i, q in enumerate(queries):
        order, scores, bound = rank_query(coll, q, None if weights is None else weights[i], **params)
        n = min(top_k, order.size)
        left += int(lr.excused(scores[order], bound[order])[:n].sum())
        total += n
    return left, total
