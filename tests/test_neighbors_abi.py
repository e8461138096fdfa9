"""CPU-side checks of the nearest-neighbour boundary (nvsm_neighbors / nvsm_similarity / nvsm_neighbor_options_default): the
symbols are declared and exported, bad pointers are status codes, the defaults are the header's, the ctypes structs have the
C sizes, the ranking and training structs did not move, and the Python layer's checks need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_neighbors", "nvsm_similarity", "nvsm_neighbor_options_default")


def test_the_header_declares_and_the_library_exports_the_neighbour_calls():
    ca.build_library()
    names = ca.abi_symbols()
    for n in NEW:
        assert n in names
        assert hasattr(ca.lib(), n)
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert " T " + n in exported, n
    assert "nvsm_debug_neighbors_force_plain" in ca._lib.hook_symbols()
    assert "nvsm_debug_neighbors_force_plain" not in exported          # the hook lives in the test-hooks library only
    assert hasattr(ca.lib(), "nvsm_debug_neighbors_force_plain")


def test_null_arguments_are_status_1_with_a_message():
    L = ca.lib()
    q, o = ca.NvsmNeighborQueries(), ca.NvsmNeighborOptions()
    sc = np.zeros(4, np.float32)
    ids, cnt = np.zeros(4, np.int64), np.zeros(1, np.int64)
    args = [C.byref(q), C.byref(o), ids.ctypes.data, sc.ctypes.data, cnt.ctypes.data]
    assert L.nvsm_neighbors(None, *args) == 1
    assert b"null argument: m" in L.nvsm_last_error()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    for i, name in enumerate((b"queries", b"opt", b"ids", b"scores", b"counts")):
        a = list(args)
        a[i] = None
        assert L.nvsm_neighbors(fake, *a) == 1 and b"null argument" in L.nvsm_last_error() and name in L.nvsm_last_error(), name
    a, b, out = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(2, np.float32)
    assert L.nvsm_similarity(None, 0, a.ctypes.data, b.ctypes.data, 2, 0, out.ctypes.data) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_similarity(fake, 0, None, b.ctypes.data, 2, 0, out.ctypes.data) == 1 and b"null argument: a" in L.nvsm_last_error()
    assert L.nvsm_similarity(fake, 0, a.ctypes.data, None, 2, 0, out.ctypes.data) == 1 and b"null argument: b" in L.nvsm_last_error()
    assert L.nvsm_similarity(fake, 0, a.ctypes.data, b.ctypes.data, 2, 0, None) == 1 and b"out" in L.nvsm_last_error()
    L.nvsm_neighbor_options_default(None)   # a no-op, not a crash


def test_neighbor_options_default():
    o = ca.NvsmNeighborOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    ca.lib().nvsm_neighbor_options_default(C.byref(o))
    assert (o.space, o.similarity, o.top_k, o.exclude_self) == (ca.SPACE_WORDS, ca.SIM_COSINE, 30, 0)
    assert o.bias_coefficient == 1.0 and o.activation == ca.ACT_MODEL and list(o.reserved) == [0] * 6
    assert (ca.SPACE_WORDS, ca.SPACE_PROJECTED_WORDS, ca.SPACE_ENTITIES) == (0, 1, 2)


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %d %d\\n", sizeof(nvsm_neighbor_queries), sizeof(nvsm_neighbor_options),\n'
                   '  sizeof(nvsm_queries), sizeof(nvsm_rank_options), sizeof(nvsm_config),\n'
                   '  NVSM_SPACE_WORDS, NVSM_SPACE_PROJECTED_WORDS, NVSM_SPACE_ENTITIES); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes[:5] == [C.sizeof(ca.NvsmNeighborQueries), C.sizeof(ca.NvsmNeighborOptions), C.sizeof(ca.NvsmQueries),
                         C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmConfig)]
    assert sizes[:2] == [32, 48]
    assert sizes[2:5] == [32, 48, 112]       # the ranking and the training ABI did not move
    assert sizes[5:] == [ca.SPACE_WORDS, ca.SPACE_PROJECTED_WORDS, ca.SPACE_ENTITIES]


def test_the_cpp_wrapper_compiles_with_the_neighbour_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m) { nvsm_neighbor_options o; nvsm_neighbor_options_default(&o); o.top_k = 3;\n'
                   '  std::vector<int64_t> ids{1, 2, 3}; std::vector<float> v(600, 0.5f);\n'
                   '  auto r = m.neighbors(ids, NVSM_SPACE_WORDS, o); auto s = m.neighbors_of_vectors(v, 300, o);\n'
                   '  auto t = m.similarity(NVSM_SPACE_ENTITIES, ids, ids, NVSM_SIM_DOT); (void)r.counts; (void)s.ids; (void)t; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


class StubModel(ca.Model):
    """a Model without a handle: everything the Python layer checks happens before the library is called"""

    def __init__(self, num_words=50, num_entities=100, word_repr_size=12, entity_repr_size=8):
        self.cfg = ca.NvsmConfig()
        self.cfg.num_words, self.cfg.num_entities = num_words, num_entities
        self.cfg.word_repr_size, self.cfg.entity_repr_size = word_repr_size, entity_repr_size
        self._h = C.c_void_p()
        self._cb = None


def test_python_checks_need_no_device():
    m = StubModel()
    # the source space's dimension must be the searched space's
    with pytest.raises(ValueError, match="dimension"):
        m.neighbors("words", ids=[1], source="entities")
    with pytest.raises(ValueError, match="dimension"):
        m.neighbors("entities", ids=[1], source="words")
    with pytest.raises(ValueError, match="dimension"):
        m.neighbors("projected_words", ids=[1], source="words")
    with pytest.raises(ValueError, match="dimension"):
        m.neighbors("words", vectors=np.zeros((2, 8), np.float32))
    with pytest.raises(ValueError, match="dimension"):
        m.nearest_terms(vectors=np.zeros((2, 12), np.float32))
    # exclude_self only with row ids of the searched space itself
    with pytest.raises(ValueError, match="exclude_self"):
        m.neighbors("entities", ids=[1], source="projected_words", exclude_self=True)
    with pytest.raises(ValueError, match="exclude_self"):
        m.neighbors("projected_words", ids=[1], source="entities", exclude_self=True)
    with pytest.raises(ValueError, match="exclude_self"):
        m.neighbors("words", vectors=np.zeros((1, 12), np.float32), exclude_self=True)
    # top_k in [1, rows of the searched space]
    for space, rows in (("words", 50), ("projected_words", 50), ("entities", 100)):
        for bad in (0, -1, rows + 1):
            with pytest.raises(ValueError, match="top_k"):
                m.neighbors(space, ids=[1], top_k=bad)
    with pytest.raises(ValueError, match="top_k"):
        m.related_terms([1], top_k=51)
    with pytest.raises(ValueError, match="top_k"):
        m.related_documents([1], top_k=101)
    with pytest.raises(ValueError, match="top_k"):
        m.nearest_terms(entity_ids=[1], top_k=51)
    # both or neither of ids / vectors
    with pytest.raises(ValueError, match="exactly one"):
        m.neighbors("words")
    with pytest.raises(ValueError, match="exactly one"):
        m.neighbors("words", ids=[1], vectors=np.zeros((1, 12), np.float32))
    with pytest.raises(ValueError, match="exactly one"):
        m.nearest_terms()
    # ids in range of the source, enums known
    with pytest.raises(ValueError, match="outside"):
        m.neighbors("words", ids=[50])
    with pytest.raises(ValueError, match="outside"):
        m.neighbors("projected_words", ids=[100], source="entities")
    with pytest.raises(ValueError, match="outside"):
        m.related_documents([-1], top_k=3)
    with pytest.raises(ValueError, match="space"):
        m.neighbors("documents", ids=[1])
    with pytest.raises(ValueError, match="space"):
        m.neighbors("words", ids=[1], source="terms")
    with pytest.raises(ValueError, match="similarity"):
        m.neighbors("words", ids=[1], similarity="l2")
    with pytest.raises(ValueError, match="activation"):
        m.nearest_terms(entity_ids=[1], activation="relu")
    with pytest.raises(ValueError, match="flat"):
        m.neighbors("words", ids=[[1, 2], [3, 4]])
    with pytest.raises(ValueError, match="outside"):
        m.term_similarity([1, 2], [3, 50])
    with pytest.raises(ValueError, match="holds"):
        m.similarity("entities", [1, 2], [3])
    with pytest.raises(ValueError, match="similarity"):
        m.similarity("entities", [1], [3], similarity="l2")


def test_neighbor_arguments_fill_the_structs():
    cfg = StubModel().cfg
    q, o, keep = cm.neighbor_arguments(cfg, "projected_words", ids=[3, 4], source="entities", top_k=7, similarity="dot",
                                       bias_coefficient=0, activation="identity")
    assert (q.num_queries, q.source_space, q.dim, q.vectors) == (2, ca.SPACE_ENTITIES, 8, None) and q.ids == keep.ctypes.data
    assert keep.dtype == np.int64 and list(keep) == [3, 4]
    assert (o.space, o.similarity, o.top_k, o.exclude_self, o.bias_coefficient, o.activation) == \
        (ca.SPACE_PROJECTED_WORDS, ca.SIM_DOT, 7, 0, 0.0, ca.ACT_IDENTITY)
    q, o, keep = cm.neighbor_arguments(cfg, "words", ids=[9], exclude_self=True, top_k=50)
    assert (q.source_space, o.space, o.exclude_self, o.top_k, o.similarity, o.activation) == \
        (ca.SPACE_WORDS, ca.SPACE_WORDS, 1, 50, ca.SIM_COSINE, ca.ACT_MODEL)
    q, o, keep = cm.neighbor_arguments(cfg, "entities", vectors=np.ones(8))            # one vector: one query
    assert (q.num_queries, q.dim, q.ids) == (1, 8, None) and q.vectors == keep.ctypes.data and keep.dtype == np.float32


def test_the_benchmark_tool_fails_without_a_gpu():
    from tests.conftest import gpu_available
    if gpu_available():
        return                                # (with a GPU the tool runs: tools/bench_neighbors.py's own output is the check there)
    p = subprocess.run(["python", os.path.join(ROOT, "tools", "bench_neighbors.py"), "--words", "1000", "--seconds", "0.01"],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)
