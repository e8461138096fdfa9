"""The numpy restatement of the inverted index's layout (tests/index_reference.py), held to a hand-written example and to counts
made another way: np.bincount for cf, the distinct (term, document) pairs for df. CPU only."""
import numpy as np

from tests import index_reference as ir
from tests import lexical_reference as lr


def test_three_documents_by_hand():
    #            d0: 2 0 2      d1: (empty)   d2: 1      d3: 0 0 2 4
    tokens = np.array([2, 0, 2, 1, 0, 0, 2, 4], np.int32)
    offsets = np.array([0, 3, 3, 4, 8], np.int64)
    post_off, post_doc, post_tf = ir.build(tokens, offsets, 6)
    assert post_off.dtype == np.int64 and post_doc.dtype == np.int32 and post_tf.dtype == np.int32
    assert list(post_off) == [0, 2, 3, 5, 5, 6, 6]          # word 3 and word 5 occur nowhere
    assert list(post_doc) == [0, 3, 2, 0, 3, 3]
    assert list(post_tf) == [1, 2, 1, 2, 1, 1]
    ids, tfs = ir.postings((post_off, post_doc, post_tf), 2)
    assert list(ids) == [0, 3] and list(tfs) == [2, 1]
    assert ir.postings((post_off, post_doc, post_tf), 3)[0].size == 0
    assert ir.info((post_off, post_doc, post_tf)) == {"num_postings": 6, "max_df": 2}


def check_contract(tokens, offsets, num_words):
    index = ir.build(tokens, offsets, num_words)
    post_off, post_doc, post_tf = index
    assert post_off[0] == 0 and post_off.size == num_words + 1 and post_off[-1] == post_doc.size == post_tf.size
    assert (post_tf >= 1).all() and post_tf.sum() == tokens.size
    cf, df = ir.frequencies(index)
    np.testing.assert_array_equal(cf, np.bincount(tokens, minlength=num_words))
    doc_of = np.repeat(np.arange(offsets.size - 1), np.diff(offsets))
    pairs = set(zip(tokens.tolist(), doc_of.tolist()))
    np.testing.assert_array_equal(df, np.bincount([t for t, _ in pairs], minlength=num_words))
    for t in range(num_words):
        ids, _ = ir.postings(index, t)
        assert (np.diff(ids) > 0).all()                     # ascending, each document once
    return index


def test_counts_made_another_way():
    check_contract(*lr.zipf_corpus(3, 200, 500), 500)
    check_contract(*ir.flat_corpus(4, 1025, 7, 9), 7)
    check_contract(*ir.flat_corpus(5, 1, 3, 1), 3)
    tokens, offsets, V = ir.shaped_corpus()
    index = check_contract(tokens, offsets, V)
    lens = np.diff(offsets)
    ids, tfs = ir.postings(index, 3)
    np.testing.assert_array_equal(ids, np.flatnonzero(lens > 0))            # in every document that holds anything
    assert tfs[list(ids).index(5)] == 90                                   # the document that is one word repeated
    assert ir.postings(index, 39)[0].size == 0
