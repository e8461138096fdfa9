"""The core check of SDM over positional postings: through nvsm_sdm_rank, nvsm_sdm_pair_counts and list B of
nvsm_rank_ensemble_sdm, ids, scores (compared as uint32), counts and pair counts with both phases served from the postings
(use = "always", the layer built) equal those of the arena scan (use = "never") bit for bit, with no tolerance; the profiler shows
which form ran; "auto" and a repeated call return the same bits; and the collection counts of the hand-built collections equal the
restatement's (tests/sdm_reference.py) directly through the postings."""
import numpy as np
import pytest

from tests import lexical_reference as lr
from tests import sdm_reference as sr
from tests.test_gpu_lexical import lexical_model
from tests.test_gpu_rank import bits
from tests.test_gpu_sdm import fusion_model

pytestmark = pytest.mark.gpu

SCAN = {"sdm_collect", "sdm_score"}
POSTINGS = {"sdm_postings_collect", "sdm_postings_score"}
METHODS = ("jm", "dirichlet")


def flat(result):
    out = []
    for r in result:
        out += [r[k] for k in sorted(r)] if isinstance(r, dict) else [r]
    return out


def assert_same_bits(a, b, what):
    a, b = flat(a), flat(b)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(bits(x), bits(y), err_msg=what)


def under(m, use, call):
    """the call's result with the index used as `use`, and the SDM groups the profiler saw meanwhile"""
    m.index_corpus(use)
    m.profile_reset()
    result = call(m)
    return result, {n for n, (_, launches) in m.profile().items() if n in SCAN | POSTINGS and launches > 0}


def layered_model(tokens, offsets, num_words):
    m = lexical_model(offsets.size - 1, num_words=num_words, corpus=(tokens, offsets))
    m.index_corpus("never", positions=True)
    m.profile_enable(True)
    return m


def check_calls(m, calls, groups=POSTINGS):
    """every call: the scan under "never", the postings under "always", the same bits; "auto" and a repeated call likewise"""
    for what, call in calls:
        scan, seen = under(m, "never", call)
        assert seen <= SCAN, (what, seen)
        post, seen = under(m, "always", call)
        assert seen == groups, (what, seen)
        assert_same_bits(scan, post, what)
        assert_same_bits(post, call(m), what + " (repeated)")
        assert_same_bits(scan, under(m, "auto", call)[0], what + " (auto)")


def rank_and_pairs(queries, **kwargs):
    pair_kwargs = {k: v for k, v in kwargs.items() if k == "window"}
    return lambda m: tuple(m.sdm_rank(queries, **kwargs)) + tuple(m.sdm_pair_counts(queries, **pair_kwargs))


# ---- the hand-built collection: every document shape the scan treats differently, a 5 000-token document of two words' pairs --------
@pytest.mark.parametrize("window", sr.WINDOWS)
def test_the_hand_built_collection(window, monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", "1")                   # slabs of 4096 documents: documents 4095 and 4096 both match
    tokens, offsets, notes = sr.hand_built(window)
    D = offsets.size - 1
    m = layered_model(tokens, offsets, sr.HAND_WORDS)
    long_query = [int(t) for t in tokens[offsets[notes["long"]]:offsets[notes["long"]] + 300]]
    queries = sr.HAND_QUERIES + [long_query]
    check_calls(m, [("%s k=%d" % (method, k), rank_and_pairs(queries, method=method, top_k=k, window=window))
                    for method in METHODS for k in (10, D)])
    # the collection counts from the postings against the restatement itself
    pos = sr.Positions(lr.Collection(tokens, offsets, sr.HAND_WORDS))
    want_o, want_u = sr.pair_counts(pos, queries, window)
    (got_o, got_u), seen = under(m, "always", lambda m: m.sdm_pair_counts(queries, window=window))
    assert seen == {"sdm_postings_collect"}
    np.testing.assert_array_equal(got_o, want_o)
    np.testing.assert_array_equal(got_u, want_u)
    assert want_o[0] > 0 and want_u[0] > want_o[0] and want_u[1] == want_u[0]
    ids = under(m, "always", lambda m: m.sdm_rank(sr.HAND_QUERIES, top_k=D, window=window))[0][0]
    for name in ("slab_last", "slab_first", "last", "len257", "long"):
        assert notes[name] in ids[0], name
    assert not np.isin(ids, [notes["empty0"], notes["empty1"]]).any()


def test_which_form_runs():
    """the postings only with the layer AND a use other than "never"; without the layer "always" is the scan"""
    tokens, offsets, _ = sr.hand_built(8)
    m = lexical_model(offsets.size - 1, num_words=sr.HAND_WORDS, corpus=(tokens, offsets))
    m.profile_enable(True)
    call = rank_and_pairs(sr.HAND_QUERIES, top_k=10)
    plain, seen = under(m, "always", call)                          # an index without the layer
    assert seen == SCAN
    m.index_positions()
    assert under(m, "never", call)[1] == SCAN
    post, seen = under(m, "always", call)
    assert seen == POSTINGS
    assert_same_bits(plain, post, "layer or none")
    assert under(m, "auto", call)[1] == POSTINGS                    # a round of short queries: far below the rule's bound
    m.drop_positions()
    assert under(m, "auto", call)[1] == SCAN
    assert under(m, "always", call)[1] == SCAN
    # a = a pairs, a pair holding a word of cf = 0, one word, no word, only an absent word: each query alone, a round of its own
    m.index_positions()
    for q in ([3, 3], [3, 3, 3], [1, 49, 2], [1], [], [49], [12, 12, 3]):
        for method in METHODS:
            scan = under(m, "never", rank_and_pairs([q], method=method, top_k=50))[0]
            post, seen = under(m, "always", rank_and_pairs([q], method=method, top_k=50))
            assert seen <= POSTINGS
            assert_same_bits(scan, post, str(q))
            assert (post[2][0] == 0) == (q in ([], [49]))            # no word, or only one nobody holds: nothing is retrieved


# ---- a seeded Zipf collection, two rounds of queries ----------------------------------------------------------------------------------
@pytest.mark.parametrize("top_k", [10, 1000])
def test_a_seeded_collection(top_k):
    tokens, offsets, qs = sr.case_inputs(1000, 300)
    m = layered_model(tokens, offsets, sr.NUM_WORDS)
    check_calls(m, [(method, rank_and_pairs(qs, method=method, top_k=top_k)) for method in METHODS])


@pytest.mark.parametrize("weights", [(1, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_weights_select_the_groups(weights):
    tokens, offsets, qs = sr.case_inputs(1000, 300)
    m = layered_model(tokens, offsets, sr.NUM_WORDS)
    check_calls(m, [(method, lambda m, method=method: m.sdm_rank(qs, method=method, top_k=50, weights=weights, window=5)) for method in METHODS])


# ---- 9 001 documents, three slabs of 4 096: a matching pair in every slab's first and last column -------------------------------------
def test_three_slabs(monkeypatch):
    monkeypatch.setenv("NVSM_RANK_SLAB_MB", "1")
    tokens, offsets = lr.zipf_corpus(9001, 9001, sr.NUM_WORDS)
    queries = sr.seeded_queries(9257, 60, tokens, offsets, sr.NUM_WORDS)
    edges = [0, 4095, 4096, 8191, 8192, 9000]                       # every slab's first and last column
    for i, d in enumerate(edges):
        assert offsets[d + 1] - offsets[d] >= 2
        queries[10 + i] = [int(t) for t in tokens[offsets[d]:offsets[d] + 2]] + queries[10 + i][:1]
    queries[20] = [int(t) for d in edges for t in tokens[offsets[d]:offsets[d] + 2]]      # one query whose pairs cross every edge
    m = layered_model(tokens, offsets, sr.NUM_WORDS)
    check_calls(m, [(method, rank_and_pairs(queries, method=method, top_k=k)) for method, k in (("jm", 9001), ("dirichlet", 10))])
    (ids, scores, counts), _ = under(m, "always", lambda m: m.sdm_rank(queries, top_k=9001))
    for d in edges:
        assert d in ids[20, :counts[20]]
    groups = m.profile()["sdm_postings_score"][1]
    assert groups >= 3 and groups % 3 == 0                          # one group per slab and round


# ---- rounds ---------------------------------------------------------------------------------------------------------------------------
def test_a_round_cut_by_its_distinct_pairs():
    """tests/test_gpu_sdm.py's inputs: 300 queries of ten words over a vocabulary of 40 hold more than the 1024 distinct pairs a round
    has counters for, so the rounds are cut by pairs — the same cut under both forms"""
    V = 40
    tokens, offsets = lr.zipf_corpus(77, 1000, V, s=0.5)
    rs = np.random.RandomState(78)
    qs = [[int(t) for t in rs.randint(0, V, 10)] for _ in range(300)]
    assert len({p for q in qs[:256] for p in sr.query_pairs(q)}) > 1024
    m = layered_model(tokens, offsets, V)
    check_calls(m, [("cut", rank_and_pairs(qs, top_k=20))])
    for use, group in (("never", "sdm_collect"), ("always", "sdm_postings_collect")):
        under(m, use, lambda m: m.sdm_pair_counts(qs))
        assert m.profile()[group][1] >= 2, use                      # more than one round, under either form


# ---- fusion ---------------------------------------------------------------------------------------------------------------------------
def test_list_b_of_the_fused_call():
    D, V = 300, 300
    m, tokens, offsets = fusion_model(D, V)
    m.index_corpus("never", positions=True)
    m.profile_enable(True)
    dependence = dict(weights=(0.8, 0.15, 0.05), window=4)
    qs = sr.seeded_queries(65, 40, tokens, offsets, V)
    check_calls(m, [("fused", lambda m: m.rank_ensemble(qs, alpha=0.4, top_k=25, dependence=dependence)),
                    ("fused, dirichlet", lambda m: m.rank_ensemble(qs, alpha=0.4, top_k=D, method="dirichlet", dependence=dependence))])
