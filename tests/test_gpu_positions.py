"""nvsm_corpus_index_positions on the GPU: every (word, document) run read through Model.positions equals the numpy restatement
(tests/positions_reference.py) on small corpora placed where the build can go wrong; a second build gives the same bytes; the
index's own dictionary does not change; and the layer's life — dropped alone, with the index, by an upload; refusals as status
codes; training undisturbed."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import index_reference as ir
from tests import lexical_reference as lr
from tests import positions_reference as pr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_lexical import lexical_model
from tests.test_gpu_rank import ADAM_STATE

pytestmark = pytest.mark.gpu

TILE = 2048                                                       # index.hip kIndexTile


def all_runs(m, layer):
    """every posting's run read back through Model.positions, concatenated in posting order: the layer's pos array"""
    runs = []
    for w, d, _ in pr.postings(layer):
        run = m.positions(w, d)
        assert run.dtype == np.int64
        runs.append(run)
    return np.concatenate(runs) if runs else np.zeros(0, np.int64)


def check_layer(tokens, offsets, num_words, absent=()):
    """the layer of the collection against the restatement: info, every posting's run, and empty runs where nothing is held"""
    m = lexical_model(offsets.size - 1, num_words=num_words, corpus=(tokens, offsets))
    before = m.index_corpus("always")
    info = m.index_positions()
    layer = pr.build(tokens, offsets, num_words)
    P, N = layer[1].size, tokens.size
    assert info == {"num_positions": N, "bytes": 4 * (P + 1) + 4 * max(N, 1)}
    assert m.index_corpus("always") == before and before["bytes"] == 8 * (num_words + 1) + 8 * max(P, 1)
    for w, d, want in pr.postings(layer):
        np.testing.assert_array_equal(m.positions(w, d), want, err_msg="word %d document %d" % (w, d))
    for w, d in absent:
        assert pr.positions(layer, w, d).size == 0 and m.positions(w, d).size == 0
    return m, layer


def test_an_empty_corpus_and_a_single_token():
    m, _ = check_layer(np.zeros(0, np.int32), np.array([0, 0, 0], np.int64), 5, absent=[(0, 0), (4, 1)])
    assert m.index_positions()["num_positions"] == 0
    check_layer(np.array([3], np.int32), np.array([0, 0, 1, 1], np.int64), 5, absent=[(3, 0), (3, 2), (2, 1)])


def test_the_shaped_corpus():
    """empty documents first, in the middle and last; a document of one word repeated; a word everywhere; a word nowhere"""
    tokens, offsets, V = ir.shaped_corpus()
    assert offsets[1] == 0 and offsets[-1] == offsets[-2] and (np.diff(offsets)[2:4] == 0).all()
    m, layer = check_layer(tokens, offsets, V, absent=[(39, 1), (39, 5), (3, 0), (3, 10), (3, 2), (0, 5)])
    np.testing.assert_array_equal(m.positions(3, 5), np.arange(90))                 # one word repeated: every offset
    assert m.positions(3, 4)[0] == 0 and m.positions(3, 4).size == pr.positions(layer, 3, 4).size


# N around the scan's tile of 2048 entries; nine documents, some of them empty
@pytest.mark.parametrize("num_tokens", [TILE - 1, TILE, TILE + 1])
def test_the_layer_at_the_tile_edges(num_tokens):
    tokens, offsets = ir.flat_corpus(num_tokens, num_tokens, 30, 9)
    m, layer = check_layer(tokens, offsets, 30)
    last = layer[1].size - 1                                                        # the corpus's last posting closes the arrays
    w, d, run = list(pr.postings(layer))[last]
    np.testing.assert_array_equal(m.positions(w, d), run)
    assert layer[3][last + 1] == num_tokens


def test_a_posting_whose_run_straddles_a_tile():
    """word 1 fills the sorted entries 1 900 .. 2 299 with ONE posting (a document that holds it 400 times): its run lies on both
    sides of entry 2 048, its head in the first tile; the postings behind it have their heads counted in the second"""
    rs = np.random.RandomState(5)
    docs = [[0] * 1000, [0] * 900 + [2, 2, 2], [], list(rs.permutation([1] * 400 + [2] * 50 + [3] * 30)), [3, 2, 3], [4]]
    tokens = np.array([t for d in docs for t in d], np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    layer = pr.build(tokens, offsets, 6)
    p = int(np.flatnonzero((np.repeat(np.arange(6), np.diff(layer[0])) == 1) & (layer[1] == 3))[0])
    assert layer[3][p] < TILE < layer[3][p + 1] and tokens.size > TILE
    m, _ = check_layer(tokens, offsets, 6, absent=[(1, 0), (1, 2), (5, 3), (4, 4)])
    assert m.positions(1, 3).size == 400 and m.positions(4, 5).tolist() == [0]


def test_a_second_build_gives_the_same_bytes():
    V = 600
    tokens, offsets = lr.zipf_corpus(47, 300, V)
    layer = pr.build(tokens, offsets, V)
    m = lexical_model(offsets.size - 1, num_words=V, corpus=(tokens, offsets))
    plain = m.index_corpus("auto")
    both = m.index_corpus("auto", positions=True)
    assert both == dict(plain, positions=m.index_positions()) and m.index_corpus("auto") == plain
    first = all_runs(m, layer)
    np.testing.assert_array_equal(first, layer[4])
    m.drop_positions()
    m.drop_positions()                                                              # no layer: success
    assert m.index_corpus("auto") == plain                                          # ... and the index stays
    np.testing.assert_array_equal(m.postings(7)[0], ir.postings(layer[:3], 7)[0])
    with pytest.raises(ca.NvsmError) as e:
        m.positions(7, 0)
    assert e.value.status == 1 and "nvsm_corpus_index_positions" in str(e.value)
    assert m.index_positions() == both["positions"]
    assert all_runs(m, layer).tobytes() == first.tobytes()
    twin = lexical_model(offsets.size - 1, num_words=V, corpus=(tokens, offsets))
    assert twin.index_corpus("never", positions=True)["positions"] == both["positions"]
    assert all_runs(twin, layer).tobytes() == first.tobytes()
    # drop_index drops both: a new index comes without the layer
    m.drop_index()
    m.index_corpus("auto")
    with pytest.raises(ca.NvsmError) as e:
        m.positions(7, 0)
    assert e.value.status == 1 and "nvsm_corpus_index_positions" in str(e.value)


def raw_positions(m, word, document, capacity, null=None):
    out, n = np.full(max(capacity, 1), -7, np.int64), C.c_int64(-7)
    st = ca.lib().nvsm_corpus_positions(m._h, word, document, capacity, None if null == "positions" else out.ctypes.data,
                                        None if null == "count" else C.byref(n))
    return st, out, n.value


def test_refusals_are_status_codes_and_an_upload_drops_the_layer():
    V, D = 300, 40
    tokens, offsets = lr.zipf_corpus(31, D, V)
    m = lexical_model(D, num_words=V)
    L = ca.lib()
    info = ca.NvsmPositionsInfo()
    assert L.nvsm_corpus_index_positions(m._h, C.byref(info)) == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error()      # no corpus
    st, _, n = raw_positions(m, 1, 0, 4)
    assert st == 1 and n == 0 and b"nvsm_corpus_upload" in L.nvsm_last_error()
    assert L.nvsm_corpus_index_positions_free(m._h) == 0
    m.upload_corpus(ca.Corpus(tokens, offsets))
    assert L.nvsm_corpus_index_positions(m._h, C.byref(info)) == 1 and b"nvsm_corpus_index first" in L.nvsm_last_error()  # no index
    st, _, n = raw_positions(m, 1, 0, 4)
    assert st == 1 and n == 0 and b"nvsm_corpus_index first" in L.nvsm_last_error()
    m.index_corpus("auto")
    st, _, n = raw_positions(m, 1, 0, 4)
    assert st == 1 and n == 0 and b"nvsm_corpus_index_positions first" in L.nvsm_last_error()                             # no layer
    assert L.nvsm_corpus_index_positions(m._h, None) == 0                                                                 # info may be NULL
    layer = pr.build(tokens, offsets, V)
    p = int(np.argmax(layer[2]))                                                    # the posting with the longest run
    word = int(np.repeat(np.arange(V), np.diff(layer[0]))[p])
    doc, tf = int(layer[1][p]), int(layer[2][p])
    assert tf > 1
    st, out, n = raw_positions(m, word, doc, tf - 1)
    assert st == 1 and n == tf and b"capacity" in L.nvsm_last_error() and (out == -7).all()
    st, out, n = raw_positions(m, word, doc, tf + 2)
    assert st == 0 and n == tf and (out[tf:] == -7).all()
    np.testing.assert_array_equal(out[:tf], pr.positions(layer, word, doc))
    for bad in (-1, V):
        st, _, n = raw_positions(m, bad, 0, 4)
        assert st == 1 and n == 0 and b"word_id" in L.nvsm_last_error()
    for bad in (-1, D):
        st, _, n = raw_positions(m, word, bad, 4)
        assert st == 1 and n == 0 and b"doc_id" in L.nvsm_last_error()
    assert raw_positions(m, word, doc, tf, null="positions")[0] == 1 and b"null argument: positions" in L.nvsm_last_error()
    assert raw_positions(m, word, doc, tf, null="count")[0] == 1 and b"null argument: count" in L.nvsm_last_error()
    np.testing.assert_array_equal(m.positions(word, doc), pr.positions(layer, word, doc))       # the handle is still usable
    # what the layer allocated is not in the text; a new upload — or none — drops it with the index
    assert m.describe() == lexical_model(D, num_words=V, corpus=(tokens, offsets)).describe()
    m.upload_corpus(ca.Corpus(tokens, offsets))
    with pytest.raises(ca.NvsmError) as e:
        m.positions(word, doc)
    assert e.value.status == 1 and "nvsm_corpus_index first" in str(e.value)
    with pytest.raises(ca.NvsmError):
        m.index_positions()
    m.index_corpus("auto", positions=True)
    m.upload_corpus(None)
    with pytest.raises(ca.NvsmError):
        m.positions(word, doc)


def test_a_build_and_reads_between_steps_never_disturb_training():
    spec = dict(num_words=2000, num_entities=600, word_dim=24, entity_dim=36, window=4, num_random=3, nonlinearity="tanh",
                batch_norm=True, update_method="sparse_adam")
    spec["lambda"] = 0.01
    tokens, offsets = lr.zipf_corpus(3, 600, 2000)
    layer = pr.build(tokens, offsets, 2000)
    some = list(pr.postings(layer))[::997]
    models = []
    for _ in range(2):
        m = gpu_model(spec, 64)
        load_params(m, random_params(spec, np.random.RandomState(9)), True)
        m.upload_corpus(ca.Corpus(tokens, offsets))
        models.append(m)
    a, b = models
    rs = np.random.RandomState(10)
    for i, (words, ww, labels, iw, ids) in enumerate([random_batch(spec, rs, 64, zipf=True) for _ in range(4)]):
        for m in (a, b):
            m.step(ca.Batch(words, labels, ww, iw), 5e-3, entity_ids=ids)
        if i == 1:
            a.index_corpus("always", positions=True)                          # straight behind nvsm_step
        if i == 2:
            a.drop_positions()
            a.index_positions()
        if i >= 1:
            for w, d, run in some:
                np.testing.assert_array_equal(a.positions(w, d), run)
    assert a.rng_state == b.rng_state
    for n in list(PARAMS) + ADAM_STATE:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
