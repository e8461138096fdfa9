"""numpy restatement of the inverted index's layout (include/cunvsm_amd.h nvsm_corpus_index): a CSR of postings over
the corpus as uploaded — post_off [V + 1] int64, post_doc [P] / post_tf [P] int32, within a term the documents ascending and each
once. np.unique over (term, document) pairs with counts; nothing here is shared with the device build (a stable sort, head flags,
a scan)."""
import numpy as np


def build(tokens, offsets, num_words):
    """(post_off, post_doc, post_tf) of the collection"""
    tokens = np.asarray(tokens, np.int64)
    offsets = np.asarray(offsets, np.int64)
    num_documents = offsets.size - 1
    doc_of = np.repeat(np.arange(num_documents, dtype=np.int64), np.diff(offsets))
    assert doc_of.size == tokens.size
    pairs, tf = np.unique(tokens * max(num_documents, 1) + doc_of, return_counts=True)      # ascending by (term, document)
    term, doc = pairs // max(num_documents, 1), pairs % max(num_documents, 1)
    post_off = np.concatenate([[0], np.cumsum(np.bincount(term, minlength=num_words))]).astype(np.int64)
    return post_off, doc.astype(np.int32), tf.astype(np.int32)


def postings(index, word):
    post_off, post_doc, post_tf = index
    return post_doc[post_off[word]:post_off[word + 1]], post_tf[post_off[word]:post_off[word + 1]]


def frequencies(index):
    """(cf [V], df [V]) as the index holds them"""
    post_off, _, post_tf = index
    df = np.diff(post_off)
    term_of = np.repeat(np.arange(df.size), df)
    cf = np.zeros(df.size, np.int64)
    np.add.at(cf, term_of, post_tf.astype(np.int64))
    return cf, df


def info(index):
    post_off, post_doc, post_tf = index
    return {"num_postings": int(post_doc.size), "max_df": int(np.diff(post_off).max()) if post_off.size > 1 else 0}


# ---- the collections the GPU layout tests build (tests/test_gpu_index.py): small, and where the build can go wrong ------------------
def flat_corpus(seed, num_tokens, num_words, num_documents):
    """num_tokens uniform tokens cut into num_documents documents at seeded places (documents may be empty)"""
    rs = np.random.RandomState(seed)
    tokens = rs.randint(0, num_words, num_tokens).astype(np.int32)
    cuts = np.sort(rs.randint(0, num_tokens + 1, max(num_documents - 1, 0)))
    return tokens, np.concatenate([[0], cuts, [num_tokens]]).astype(np.int64)


def shaped_corpus():
    """empty documents first, last and in between; a document of 700 tokens (longer than a workgroup); a document that is one word
    repeated; word 3 in every non-empty document; word 39 in none. V = 40."""
    rs = np.random.RandomState(11)
    draw = lambda n: [3] + list(rs.randint(0, 39, n - 1))
    docs = [[], draw(5), [], [], draw(700), [3] * 90, draw(64), [], draw(1), draw(65), []]
    tokens = np.array([t for d in docs for t in d], np.int32)
    return tokens, np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64), 40
