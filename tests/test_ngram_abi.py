"""CPU-side checks of the n-gram boundary (nvsm_ngram_search / nvsm_ngram_rows / nvsm_ngram_options_default): the symbols are
declared and exported, the hook lives in the hooks library only, bad pointers are status codes, the defaults are the header's, the
ctypes struct has the C size, no earlier struct moved, the C++ wrapper compiles as C++11, and the Python layer's checks need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT
from tests.test_neighbors_abi import StubModel

NEW = ("nvsm_ngram_search", "nvsm_ngram_rows", "nvsm_ngram_options_default")


def test_the_header_declares_and_the_library_exports_the_ngram_calls():
    ca.build_library()
    names = ca.abi_symbols()
    for n in NEW:
        assert n in names
        assert hasattr(ca.lib(), n)
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert " T " + n in exported, n
    assert "nvsm_debug_ngram_rows" in ca._lib.hook_symbols()
    assert "nvsm_debug_ngram_rows" not in exported                       # the hook lives in the test-hooks library only
    assert hasattr(ca.lib(), "nvsm_debug_ngram_rows")
    hooks = subprocess.run(["nm", "-D", "--defined-only", ca._lib._HOOKS_SO], capture_output=True, text=True, check=True).stdout
    assert " T nvsm_debug_ngram_rows" in hooks
    assert "ngram_rows_kernel" not in hooks, "the hooks library carries no kernels of its own"
    assert "launch_ngram_rows" in exported and "launch_ngram_rows" not in hooks      # the launcher it calls is the product's


def test_null_arguments_are_status_1_with_their_names():
    L = ca.lib()
    q, o = ca.NvsmNeighborQueries(), ca.NvsmNgramOptions()
    rows, terms, sc, cnt = np.zeros(4, np.int64), np.zeros(8, np.int64), np.zeros(4, np.float32), np.zeros(1, np.int64)
    args = [C.byref(q), C.byref(o), rows.ctypes.data, terms.ctypes.data, sc.ctypes.data, cnt.ctypes.data]
    assert L.nvsm_ngram_search(None, *args) == 1
    assert b"null argument: m" in L.nvsm_last_error()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    for i, name in enumerate((b"queries", b"opt", b"phrase_rows", b"terms", b"scores", b"counts")):
        a = list(args)
        a[i] = None
        assert L.nvsm_ngram_search(fake, *a) == 1 and b"null argument: " + name in L.nvsm_last_error(), name
    G = np.zeros(4, np.float32)
    assert L.nvsm_debug_ngram_rows(None, 1, 4, G.ctypes.data, 1.0, 0, 0, 1, G.ctypes.data, 1, 0) == 1 and b"null argument: G" in L.nvsm_last_error()
    assert L.nvsm_debug_ngram_rows(G.ctypes.data, 1, 4, None, 1.0, 0, 0, 1, G.ctypes.data, 1, 0) == 1 and b"bias" in L.nvsm_last_error()
    assert L.nvsm_debug_ngram_rows(G.ctypes.data, 1, 4, G.ctypes.data, 1.0, 0, 0, 1, None, 1, 0) == 1 and b"out" in L.nvsm_last_error()
    L.nvsm_ngram_options_default(None)      # a no-op, not a crash


def test_ngram_options_default():
    o = ca.NvsmNgramOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    ca.lib().nvsm_ngram_options_default(C.byref(o))
    assert (o.max_cardinality, o.similarity, o.top_k, o.activation) == (1, ca.SIM_COSINE, 20, ca.ACT_MODEL)
    assert o.bias_coefficient == 1.0 and o.vocabulary is None and o.vocabulary_size == 0
    assert o.reserved0 == 0 and list(o.reserved) == [0] * 4


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(nvsm_ngram_options),\n'
                   '  offsetof(nvsm_ngram_options, vocabulary), offsetof(nvsm_ngram_options, vocabulary_size),\n'
                   '  offsetof(nvsm_ngram_options, reserved), sizeof(nvsm_queries), sizeof(nvsm_rank_options),\n'
                   '  sizeof(nvsm_neighbor_options), sizeof(nvsm_config), sizeof(nvsm_neighbor_queries)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    N = ca.NvsmNgramOptions
    assert sizes[:4] == [C.sizeof(N), N.vocabulary.offset, N.vocabulary_size.offset, N.reserved.offset] == [56, 24, 32, 40]
    assert sizes[4:] == [C.sizeof(ca.NvsmQueries), C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmNeighborOptions), C.sizeof(ca.NvsmConfig),
                         C.sizeof(ca.NvsmNeighborQueries)]
    assert sizes[4:] == [32, 48, 48, 112, 32]      # no earlier struct changed size


def test_the_cpp_wrapper_compiles_as_cpp11_with_the_ngram_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m) { nvsm_ngram_options o; nvsm_ngram_options_default(&o); o.max_cardinality = 2;\n'
                   '  std::vector<int64_t> ids{1, 2, 3}, voc{4, 9}; std::vector<float> v(512, 0.5f); o.vocabulary = voc.data(); o.vocabulary_size = 2;\n'
                   '  cunvsm_amd::Model::Ngrams r = m.ngram_search(ids, NVSM_SPACE_ENTITIES, o), s = m.ngram_search_of_vectors(v, o);\n'
                   '  (void)r.terms; (void)s.phrase_rows; (void)nvsm_ngram_rows(5, 2); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_python_checks_need_no_device():
    m = StubModel()                             # 50 words, 100 entities, d_w = 12, d_e = 8
    ok = dict(entity_ids=[1, 2], vocabulary=[3, 5, 9, 40])      # R = 4 + 6
    for kw, word in ((dict(max_cardinality=0), "max_cardinality"), (dict(max_cardinality=3), "max_cardinality"),
                     (dict(vocabulary=[3, 3, 9]), "ascending"), (dict(vocabulary=[9, 3]), "ascending"),
                     (dict(vocabulary=[3, 50]), "outside"), (dict(vocabulary=[-1, 5]), "outside"), (dict(vocabulary=[]), "vocabulary_size"),
                     (dict(vocabulary=[[1, 2]]), "flat"),
                     (dict(top_k=0), "top_k"), (dict(top_k=11), "top_k"), (dict(top_k=5, max_cardinality=1), "top_k"),
                     (dict(similarity="l2"), "similarity"), (dict(similarity=7), "similarity"),
                     (dict(activation="relu"), "activation"), (dict(activation=9), "activation"),
                     (dict(bias_coefficient=float("nan")), "finite"), (dict(bias_coefficient=float("inf")), "finite"),
                     (dict(entity_ids=None), "exactly one"), (dict(word_ids=[1]), "exactly one"),
                     (dict(vectors=np.zeros((1, 8), np.float32)), "exactly one"),
                     (dict(entity_ids=None, vectors=np.zeros((2, 12), np.float32)), "dimension"),
                     (dict(entity_ids=[100]), "outside"), (dict(entity_ids=[-1]), "outside"),
                     (dict(entity_ids=None, word_ids=[50]), "outside"), (dict(entity_ids=[[1, 2]]), "flat")):
        with pytest.raises(ValueError, match=word):
            m.nearest_ngrams(**dict(ok, **kw))
    with pytest.raises(ValueError, match="limit"):
        StubModel(num_words=65536).nearest_ngrams(entity_ids=[1])
    with pytest.raises(ValueError, match="top_k"):
        m.nearest_ngrams(entity_ids=[1], max_cardinality=1, top_k=51)


def test_ngram_arguments_fill_the_structs():
    cfg = StubModel().cfg
    q, o, voc, keep = cm.ngram_arguments(cfg, entity_ids=[3, 4], vocabulary=[2, 7, 30], top_k=6, similarity="dot", bias_coefficient=0,
                                         activation="identity")
    assert (q.num_queries, q.source_space, q.dim, q.vectors) == (2, ca.SPACE_ENTITIES, 8, None) and q.ids == keep.ctypes.data
    assert (o.max_cardinality, o.similarity, o.top_k, o.bias_coefficient, o.activation) == (2, ca.SIM_DOT, 6, 0.0, ca.ACT_IDENTITY)
    assert o.vocabulary == voc.ctypes.data and o.vocabulary_size == 3 and voc.dtype == np.int64 and list(voc) == [2, 7, 30]
    q, o, voc, keep = cm.ngram_arguments(cfg, word_ids=[9], max_cardinality=1)
    assert (q.source_space, q.num_queries, o.max_cardinality, o.top_k, o.similarity, o.activation) == \
        (ca.SPACE_PROJECTED_WORDS, 1, 1, 20, ca.SIM_COSINE, ca.ACT_MODEL)
    assert voc is None and o.vocabulary is None and o.vocabulary_size == 0
    q, o, voc, keep = cm.ngram_arguments(cfg, vectors=np.ones(8), vocabulary=np.arange(50))       # one vector: one query
    assert (q.num_queries, q.dim, q.ids) == (1, 8, None) and q.vectors == keep.ctypes.data and keep.dtype == np.float32
    assert o.top_k == 20 and o.vocabulary_size == 50


def test_the_benchmark_tool_fails_without_a_gpu():
    from tests.conftest import gpu_available
    if gpu_available():
        return                                # (with a GPU the tool runs: tools/bench_ngrams.py's own output is the check there)
    p = subprocess.run(["python", os.path.join(ROOT, "tools", "bench_ngrams.py"), "--words", "100", "--seconds", "0.01"],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)
