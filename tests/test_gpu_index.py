"""nvsm_corpus_index on the GPU: the layout equals the numpy restatement (tests/index_reference.py) exactly, term by term through
Model.postings, on small corpora placed where the build can go wrong; a second build gives the same bytes; cf and df are those of
np.bincount and of lex_df_kernel; and the index's life — dropped by an upload, refusals as status codes, training undisturbed."""
import ctypes as C

import numpy as np
import pytest

import cunvsm_amd as ca
from tests import index_reference as ir
from tests import lexical_reference as lr
from tests.helpers import PARAMS, gpu_model, load_params, random_batch, random_params
from tests.test_gpu_lexical import lexical_model
from tests.test_gpu_rank import ADAM_STATE, same_bits

pytestmark = pytest.mark.gpu


def all_postings(m, num_words):
    """(post_off, post_doc, post_tf) read back term by term"""
    lists = [m.postings(t) for t in range(num_words)]
    for ids, tfs in lists:
        assert ids.dtype == np.int64 and tfs.dtype == np.int32 and ids.shape == tfs.shape
    off = np.concatenate([[0], np.cumsum([ids.size for ids, _ in lists])]).astype(np.int64)
    cat = lambda i, dt: np.concatenate([l[i] for l in lists]).astype(dt) if lists else np.zeros(0, dt)
    return off, cat(0, np.int32), cat(1, np.int32)


def check_layout(tokens, offsets, num_words, words=None):
    """the index of the collection against the restatement: info, then every list (`words`: only these, for a large vocabulary)"""
    m = lexical_model(offsets.size - 1, num_words=num_words, corpus=(tokens, offsets))
    info = m.index_corpus("always")
    want = ir.build(tokens, offsets, num_words)
    assert info["num_postings"] == want[1].size and info["max_df"] == ir.info(want)["max_df"] and info["use"] == "always"
    assert info["bytes"] == 8 * (num_words + 1) + 8 * max(want[1].size, 1)
    if words is None:
        got = all_postings(m, num_words)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        assert got[2].sum() == tokens.size
    else:
        for t in words:
            ids, tfs = m.postings(int(t))
            w_ids, w_tfs = ir.postings(want, int(t))
            np.testing.assert_array_equal(ids, w_ids)
            np.testing.assert_array_equal(tfs, w_tfs)
    return m, want


# N at the wave's and the sort tile's edges; seven documents, some of them empty
@pytest.mark.parametrize("num_tokens", [1, 63, 64, 65, 1023, 1024, 1025])
def test_layout_at_the_wave_and_tile_edges(num_tokens):
    tokens, offsets = ir.flat_corpus(num_tokens, num_tokens, 50, 7)
    check_layout(tokens, offsets, 50)


def test_layout_of_the_shaped_corpus():
    """empty documents first, last and in between, a document longer than a workgroup, one word repeated, a word everywhere, a word nowhere"""
    tokens, offsets, V = ir.shaped_corpus()
    m, want = check_layout(tokens, offsets, V)
    ids, tfs = m.postings(3)
    np.testing.assert_array_equal(ids, np.flatnonzero(np.diff(offsets) > 0))
    assert m.postings(39)[0].size == 0 and m.postings(39)[1].size == 0


def test_layout_of_a_single_document():
    tokens = np.array([4, 4, 1, 0, 4], np.int32)
    m, _ = check_layout(tokens, np.array([0, 5], np.int64), 6)
    ids, tfs = m.postings(4)
    assert list(ids) == [0] and list(tfs) == [3]


def test_layout_over_several_sort_workgroups_and_two_digit_passes():
    tokens, offsets = lr.zipf_corpus(41, 1300, 600)            # about 40 000 tokens, V = 600: 10 key bits
    assert 35000 < tokens.size < 45000
    check_layout(tokens, offsets, 600)


def test_layout_of_a_sparsely_used_large_vocabulary():
    V = 300000                                                  # 19 key bits: three digit passes
    rs = np.random.RandomState(43)
    used = np.unique(np.concatenate([[0, V - 1], rs.randint(0, V, 400)]))
    tokens = used[rs.randint(0, used.size, 5000)].astype(np.int32)
    offsets = np.concatenate([[0], np.sort(rs.randint(0, 5001, 299)), [5000]]).astype(np.int64)
    unused = np.setdiff1d(rs.randint(0, V, 50), used)
    m, want = check_layout(tokens, offsets, V, words=np.concatenate([used, unused, [1, V - 2]]))
    assert m.postings(int(unused[0]))[0].size == 0


def test_a_second_build_gives_the_same_bytes_and_cf_df_are_the_scan_kernels():
    V = 600
    tokens, offsets = lr.zipf_corpus(47, 300, V)
    m = lexical_model(offsets.size - 1, num_words=V, corpus=(tokens, offsets))
    first_info = m.index_corpus("auto")
    first = all_postings(m, V)
    assert m.index_corpus("never") == dict(first_info, use="never")          # a second call only changes `use`
    m.drop_index()
    m.drop_index()                                                            # no index: success
    assert m.index_corpus("auto") == first_info
    for a, b in zip(first, all_postings(m, V)):
        assert a.tobytes() == b.tobytes()
    other = lexical_model(offsets.size - 1, num_words=V, corpus=(tokens, offsets))
    other.index_corpus()
    for a, b in zip(first, all_postings(other, V)):
        assert a.tobytes() == b.tobytes()
    # cf and df of the index: np.bincount, and what lex_df_kernel counts
    cf, df = ir.frequencies(first)
    np.testing.assert_array_equal(cf, np.bincount(tokens, minlength=V))
    hook_df = np.zeros(V, np.int64)
    assert ca.lib().nvsm_debug_lex_df(tokens.ctypes.data, tokens.size, offsets.ctypes.data, offsets.size - 1, V, 64, hook_df.ctypes.data) == 0
    np.testing.assert_array_equal(df, hook_df)
    # ... and the tables the rankers take from the index are the ones they make themselves: the same bits from a handle that
    # indexed before its first lexical call and from one that never indexed
    plain = lexical_model(offsets.size - 1, num_words=V, corpus=(tokens, offsets))
    queries = lr.zipf_queries(48, 20, V, tokens)
    other.index_corpus("never")
    same_bits(plain.lexical_rank(queries, top_k=30), other.lexical_rank(queries, top_k=30))
    same_bits(plain.tfidf_rank(queries, top_k=30), other.tfidf_rank(queries, top_k=30))


# ---- lifecycle ---------------------------------------------------------------------------------------------------------------------------
def raw_postings(m, word, capacity, null=None):
    ids, tfs, n = np.full(max(capacity, 1), -7, np.int64), np.full(max(capacity, 1), -7, np.int32), C.c_int64(-7)
    st = ca.lib().nvsm_corpus_postings(m._h, word, capacity, None if null == "doc_ids" else ids.ctypes.data,
                                       None if null == "tfs" else tfs.ctypes.data, None if null == "count" else C.byref(n))
    return st, ids, tfs, n.value


def raw_index(m, use=0, null=None, with_info=True):
    opt, info = ca.NvsmIndexOptions(), ca.NvsmIndexInfo()
    ca.lib().nvsm_index_options_default(C.byref(opt))
    opt.use = use
    return ca.lib().nvsm_corpus_index(m._h, None if null == "opt" else C.byref(opt), C.byref(info) if with_info else None), info


def test_an_upload_drops_the_index_and_refusals_are_status_codes():
    V = 300
    tokens, offsets = lr.zipf_corpus(31, 40, V)
    m = lexical_model(40, num_words=V)
    L = ca.lib()
    st, _ = raw_index(m)
    assert st == 1 and b"nvsm_corpus_upload" in L.nvsm_last_error()                    # no corpus
    st, _, _, n = raw_postings(m, 1, 4)
    assert st == 1 and n == 0 and b"nvsm_corpus_upload" in L.nvsm_last_error()
    assert L.nvsm_corpus_index_free(m._h) == 0
    m.upload_corpus(ca.Corpus(tokens, offsets))
    st, _, _, n = raw_postings(m, 1, 4)
    assert st == 1 and n == 0 and b"nvsm_corpus_index" in L.nvsm_last_error()          # no index
    for kwargs, word in ((dict(use=3), b"unknown index use"), (dict(use=-1), b"unknown index use"), (dict(null="opt"), b"null argument: opt")):
        st, _ = raw_index(m, **kwargs)
        assert st == 1 and word in L.nvsm_last_error(), kwargs
        assert raw_postings(m, 1, 4)[0] == 1                                            # ... and nothing was built
    assert raw_index(m, use=1, with_info=False)[0] == 0                                 # info may be NULL
    want = ir.build(tokens, offsets, V)
    word = int(np.argmax(np.diff(want[0])))
    df = int(np.diff(want[0])[word])
    assert df > 1
    st, ids, tfs, n = raw_postings(m, word, df - 1)
    assert st == 1 and n == df and b"capacity" in L.nvsm_last_error() and (ids == -7).all() and (tfs == -7).all()
    st, ids, tfs, n = raw_postings(m, word, df + 2)
    assert st == 0 and n == df and (ids[df:] == -7).all()
    np.testing.assert_array_equal(ids[:df], ir.postings(want, word)[0])
    for bad in (-1, V):
        st, _, _, n = raw_postings(m, bad, 4)
        assert st == 1 and n == 0 and b"num_words" in L.nvsm_last_error()
    for null, name in (("doc_ids", b"null argument: doc_ids"), ("tfs", b"null argument: tfs"), ("count", b"null argument: count")):
        assert raw_postings(m, word, df, null=null)[0] == 1 and name in L.nvsm_last_error()
    with pytest.raises(ValueError):
        m.index_corpus("sometimes")
    # the handle is still usable, and a new upload — or none — drops the index with the corpus
    queries = lr.zipf_queries(32, 8, V, tokens)
    indexed = m.lexical_rank(queries, top_k=10)
    m.upload_corpus(ca.Corpus(tokens, offsets))
    with pytest.raises(ca.NvsmError) as e:
        m.postings(word)
    assert e.value.status == 1 and "nvsm_corpus_index" in str(e.value)
    same_bits(indexed, m.lexical_rank(queries, top_k=10))
    m.index_corpus()
    # what the index allocated is not in the text
    assert m.describe() == lexical_model(40, num_words=V, corpus=(tokens, offsets)).describe()
    m.upload_corpus(None)
    with pytest.raises(ca.NvsmError):
        m.postings(word)


def test_an_index_build_and_an_indexed_call_between_steps_never_disturb_training():
    spec = dict(num_words=2000, num_entities=600, word_dim=24, entity_dim=36, window=4, num_random=3, nonlinearity="tanh",
                batch_norm=True, update_method="sparse_adam")
    spec["lambda"] = 0.01
    tokens, offsets = lr.zipf_corpus(3, 600, 2000)
    queries = lr.zipf_queries(4, 20, 2000, tokens)
    models = []
    for _ in range(2):
        m = gpu_model(spec, 64)
        load_params(m, random_params(spec, np.random.RandomState(9)), True)
        m.upload_corpus(ca.Corpus(tokens, offsets))
        models.append(m)
    a, b = models
    rs = np.random.RandomState(10)
    first = None
    for i, (words, ww, labels, iw, ids) in enumerate([random_batch(spec, rs, 64, zipf=True) for _ in range(4)]):
        for m in (a, b):
            m.step(ca.Batch(words, labels, ww, iw), 5e-3, entity_ids=ids)
        if i == 1:
            a.index_corpus("always")                                          # straight behind nvsm_step
        if i == 2:
            a.drop_index()
            a.index_corpus("always")
        res = a.lexical_rank(queries, top_k=50)
        if first is None:
            first = res
        same_bits(first, res)                                                 # scan in step 0, postings from step 1 on
    assert a.rng_state == b.rng_state
    for n in list(PARAMS) + ADAM_STATE:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
