"""numpy restatement of the positional layer of the inverted index (include/cunvsm_amd.h nvsm_corpus_index_positions):
beside the postings of tests/index_reference.py, post_first [P + 1] — a posting's first entry of pos, post_first[P] = N — and pos [N],
every posting's in-document offsets, ascending. A stable argsort by term keeps a term's arena positions ascending; the run heads —
where (term, document) changes — are post_first; a position's document comes from searchsorted into the offsets. Nothing here is
shared with the device build."""
import numpy as np


def build(tokens, offsets, num_words):
    """(post_off [V + 1], post_doc [P], post_tf [P], post_first [P + 1], pos [N]) of the collection"""
    tokens = np.asarray(tokens, np.int64)
    offsets = np.asarray(offsets, np.int64)
    N = tokens.size
    order = np.argsort(tokens, kind="stable")                        # arena positions grouped by term, ascending inside a term
    term = tokens[order]
    doc = np.searchsorted(offsets, order, side="right") - 1          # the last document whose first token is <= the position
    pos = (order - offsets[doc]).astype(np.int32) if N else np.zeros(0, np.int32)
    head = np.ones(N, bool)
    if N:
        head[1:] = (term[1:] != term[:-1]) | (doc[1:] != doc[:-1])
    first = np.flatnonzero(head)
    post_first = np.concatenate([first, [N]]).astype(np.int32)
    post_doc = doc[first].astype(np.int32)
    post_tf = np.diff(post_first).astype(np.int32)
    post_off = np.concatenate([[0], np.cumsum(np.bincount(term[first], minlength=num_words))]).astype(np.int64)
    return post_off, post_doc, post_tf, post_first, pos


def positions(layer, word, document):
    """the in-document offsets of `word` in `document`, ascending; empty when the document does not hold it"""
    post_off, post_doc, _, post_first, pos = layer
    lo, hi = post_off[word], post_off[word + 1]
    p = lo + np.searchsorted(post_doc[lo:hi], document)
    if p == hi or post_doc[p] != document:
        return np.zeros(0, np.int64)
    return pos[post_first[p]:post_first[p + 1]].astype(np.int64)


def postings(layer):
    """every (word, document, run) of the layer, in posting order"""
    post_off, post_doc, _, post_first, pos = layer
    word_of = np.repeat(np.arange(post_off.size - 1), np.diff(post_off))
    for p in range(post_doc.size):
        yield int(word_of[p]), int(post_doc[p]), pos[post_first[p]:post_first[p + 1]].astype(np.int64)


def _follows(a, b, window):
    """how many positions i of the ascending run a have a position j of b with i < j < i + window"""
    if a.size == 0 or b.size == 0:
        return 0
    nxt = np.searchsorted(b, a, side="right")
    ok = nxt < b.size
    j = b[np.minimum(nxt, b.size - 1)]
    return int((ok & (j < a + window)).sum())


def pair_counts(layer, a, b, window):
    """(cf_o, cf_u) of the pair (a, b) from the layer alone: both runs of a document merged, no document boundary to test"""
    post_off, post_doc, _, _, _ = layer
    V = post_off.size - 1
    if not (0 <= a < V and 0 <= b < V):
        return 0, 0
    docs = np.intersect1d(post_doc[post_off[a]:post_off[a + 1]], post_doc[post_off[b]:post_off[b + 1]])
    o = u = 0
    for d in docs:
        pa, pb = positions(layer, a, int(d)), positions(layer, b, int(d))
        o += _follows(pa, pb, 2)
        u += _follows(pa, pb, window) + (_follows(pb, pa, window) if a != b else 0)
    return o, u
