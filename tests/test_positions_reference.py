"""The restatement of the positional layer (tests/positions_reference.py) held to lists written by hand on five documents, one of
them empty, and to the sequential-dependence restatement (tests/sdm_reference.py) on its hand-built collections: the pair counts
worked out from the layer's runs alone are those counted over the arena."""
import numpy as np
import pytest

from tests import index_reference as ir
from tests import lexical_reference as lr
from tests import positions_reference as pr
from tests import sdm_reference as sr

#        document 0      1 (empty)  2            3      4
DOCS = [[2, 0, 2, 1],    [],        [1, 1, 1],   [0],   [2, 1, 0, 0, 2]]
TOKENS = np.array([t for d in DOCS for t in d], np.int32)
OFFSETS = np.concatenate([[0], np.cumsum([len(d) for d in DOCS])]).astype(np.int64)
V = 4                                                               # word 3 occurs nowhere


def test_the_layer_of_five_documents_by_hand():
    post_off, post_doc, post_tf, post_first, pos = pr.build(TOKENS, OFFSETS, V)
    assert list(post_off) == [0, 3, 6, 8, 8]
    assert list(post_doc) == [0, 3, 4, 0, 2, 4, 0, 4]
    assert list(post_tf) == [1, 1, 2, 1, 3, 1, 2, 2]
    assert list(post_first) == [0, 1, 2, 4, 5, 8, 9, 11, 13]
    assert list(pos) == [1, 0, 2, 3, 3, 0, 1, 2, 1, 0, 2, 0, 4]
    assert post_first.dtype == pos.dtype == np.int32 and post_first[-1] == TOKENS.size
    np.testing.assert_array_equal(np.diff(post_first), post_tf)
    for got, want in zip((post_off, post_doc, post_tf), ir.build(TOKENS, OFFSETS, V)):
        np.testing.assert_array_equal(got, want)
    layer = (post_off, post_doc, post_tf, post_first, pos)
    assert list(pr.positions(layer, 2, 0)) == [0, 2] and list(pr.positions(layer, 0, 4)) == [2, 3]
    assert pr.positions(layer, 2, 1).size == 0 and pr.positions(layer, 3, 0).size == 0 and pr.positions(layer, 0, 2).size == 0
    assert pr.positions(layer, 1, 2).dtype == np.int64
    assert [(w, d) for w, d, _ in pr.postings(layer)] == [(0, 0), (0, 3), (0, 4), (1, 0), (1, 2), (1, 4), (2, 0), (2, 4)]
    # every token is found again where the layer says it is
    for w, d, run in pr.postings(layer):
        assert (TOKENS[OFFSETS[d] + run] == w).all() and (np.diff(run) > 0).all()


def test_an_empty_corpus_and_a_single_token():
    post_off, post_doc, post_tf, post_first, pos = pr.build(np.zeros(0, np.int32), np.array([0, 0, 0], np.int64), 3)
    assert list(post_off) == [0, 0, 0, 0] and post_doc.size == post_tf.size == pos.size == 0 and list(post_first) == [0]
    layer = pr.build(np.array([2], np.int32), np.array([0, 0, 1], np.int64), 3)
    assert list(layer[3]) == [0, 1] and list(layer[4]) == [0] and list(pr.positions(layer, 2, 1)) == [0]


def test_pair_counts_by_hand():
    layer = pr.build(TOKENS, OFFSETS, V)
    assert pr.pair_counts(layer, 2, 0, 8) == (1, 5)                 # document 0: "2 0" and "0 2"; document 4: one 2 before two 0, both before a 2
    assert pr.pair_counts(layer, 0, 2, 8) == (2, 5) and pr.pair_counts(layer, 2, 0, 2) == (1, 3)
    assert pr.pair_counts(layer, 1, 1, 2) == (2, 2) and pr.pair_counts(layer, 1, 1, 8) == (2, 2)
    assert pr.pair_counts(layer, 0, 0, 2) == (1, 1) and pr.pair_counts(layer, 3, 0, 8) == (0, 0) and pr.pair_counts(layer, 0, 9, 8) == (0, 0)


@pytest.mark.parametrize("window", sr.WINDOWS)
def test_the_layer_reproduces_the_arena_pair_counts_on_the_hand_built_collection(window):
    tokens, offsets, notes = sr.hand_built(window)
    layer = pr.build(tokens, offsets, sr.HAND_WORDS)
    pos = sr.Positions(lr.Collection(tokens, offsets, sr.HAND_WORDS))
    want_o, want_u = sr.pair_counts(pos, sr.HAND_QUERIES, window)
    got = [pr.pair_counts(layer, a, b, window) for q in sr.HAND_QUERIES for a, b in sr.query_pairs(q)]
    np.testing.assert_array_equal(np.array([o for o, _ in got], np.uint64), want_o)
    np.testing.assert_array_equal(np.array([u for _, u in got], np.uint64), want_u)
    assert want_o[0] > 0 and want_u[0] > want_o[0]
    # the long document's runs are what the arena holds
    d = notes["long"]
    for w in (1, 2):
        np.testing.assert_array_equal(pr.positions(layer, w, d), np.flatnonzero(tokens[offsets[d]:offsets[d + 1]] == w))
