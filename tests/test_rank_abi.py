"""CPU-side checks of the ranking boundary (nvsm_infer / nvsm_rank / nvsm_rank_options_default): the symbols are declared
and exported, bad pointers are status codes, the defaults are the header's, the ctypes structs have the C sizes, and the
Python layer's shape checks need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_infer", "nvsm_rank", "nvsm_rank_options_default")


def test_the_header_declares_and_the_library_exports_the_ranking_calls():
    ca.build_library()
    names = ca.abi_symbols()
    for n in NEW:
        assert n in names
        assert hasattr(ca.lib(), n)
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert " T " + n in exported, n


def test_null_arguments_are_status_1_with_a_message():
    L = ca.lib()
    q, o = ca.NvsmQueries(), ca.NvsmRankOptions()
    out = np.zeros(4, np.float32)
    ids, cnt = np.zeros(4, np.int64), np.zeros(1, np.int64)
    assert L.nvsm_infer(None, C.byref(q), C.byref(o), out.ctypes.data) == 1
    assert b"null argument" in L.nvsm_last_error()
    assert L.nvsm_rank(None, C.byref(q), C.byref(o), ids.ctypes.data, out.ctypes.data, cnt.ctypes.data) == 1
    assert b"null argument: m" in L.nvsm_last_error()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    assert L.nvsm_infer(fake, None, C.byref(o), out.ctypes.data) == 1 and b"queries" in L.nvsm_last_error()
    assert L.nvsm_infer(fake, C.byref(q), None, out.ctypes.data) == 1 and b"opt" in L.nvsm_last_error()
    assert L.nvsm_infer(fake, C.byref(q), C.byref(o), None) == 1 and b"out" in L.nvsm_last_error()
    assert L.nvsm_rank(fake, None, C.byref(o), ids.ctypes.data, out.ctypes.data, cnt.ctypes.data) == 1
    assert L.nvsm_rank(fake, C.byref(q), None, ids.ctypes.data, out.ctypes.data, cnt.ctypes.data) == 1
    assert L.nvsm_rank(fake, C.byref(q), C.byref(o), None, out.ctypes.data, cnt.ctypes.data) == 1 and b"doc_ids" in L.nvsm_last_error()
    assert L.nvsm_rank(fake, C.byref(q), C.byref(o), ids.ctypes.data, None, cnt.ctypes.data) == 1 and b"scores" in L.nvsm_last_error()
    assert L.nvsm_rank(fake, C.byref(q), C.byref(o), ids.ctypes.data, out.ctypes.data, None) == 1 and b"counts" in L.nvsm_last_error()
    L.nvsm_rank_options_default(None)       # a no-op, not a crash


def test_rank_options_default():
    o = ca.NvsmRankOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    ca.lib().nvsm_rank_options_default(C.byref(o))
    assert o.bias_coefficient == 1.0 and o.activation == ca.ACT_MODEL == -1 and o.similarity == ca.SIM_COSINE == 0 and o.top_k == 1000
    assert not o.candidates and not o.candidate_offsets and list(o.reserved) == [0, 0, 0, 0]
    assert (ca.SIM_DOT, ca.ACT_IDENTITY) == (1, -2)


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu\\n", sizeof(nvsm_queries), sizeof(nvsm_rank_options), sizeof(nvsm_config)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(ca.NvsmQueries), C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmConfig)]
    assert sizes[2] == 112                   # the training ABI did not move


def test_the_cpp_wrapper_compiles_with_the_ranking_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m) { nvsm_rank_options o; nvsm_rank_options_default(&o); o.top_k = 3;\n'
                   '  std::vector<int64_t> ids{1, 2, 3}, off{0, 2, 3}; std::vector<float> w{1.f, 2.f, 1.f};\n'
                   '  auto p = m.infer(ids, off, &w); auto r = m.rank(ids, off, o, &w); (void)p; (void)r.counts; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


class StubModel(ca.Model):
    """a Model without a handle: everything the Python layer checks happens before the library is called"""

    def __init__(self, num_entities=100, entity_repr_size=8):
        self.cfg = ca.NvsmConfig()
        self.cfg.num_entities, self.cfg.entity_repr_size = num_entities, entity_repr_size
        self._h = C.c_void_p()
        self._cb = None


def test_python_shape_checks_need_no_device():
    m = StubModel()
    for bad in (dict(top_k=0), dict(top_k=101), dict(top_k=-3)):
        with pytest.raises(ValueError, match="top_k"):
            m.rank([[1, 2]], **bad)
    with pytest.raises(ValueError, match="weights"):
        m.rank([[1, 2], [3]], top_k=5, weights=[[1.0, 2.0]])
    with pytest.raises(ValueError, match="weights"):
        m.rank([[1, 2], [3]], top_k=5, weights=[[1.0], [1.0]])
    with pytest.raises(ValueError, match="sum to zero"):
        m.infer([[1, 2]], weights=[[1.0, -1.0]])
    with pytest.raises(ValueError, match="candidates"):
        m.rank([[1, 2], [3]], top_k=5, candidates=[[1, 2, 3]])
    with pytest.raises(ValueError, match="candidate"):
        m.rank([[1, 2]], top_k=5, candidates=[[100]])
    with pytest.raises(ValueError, match="activation"):
        m.infer([[1]], activation="relu")
    with pytest.raises(ValueError, match="similarity"):
        m.rank([[1]], top_k=5, similarity="l2")
    with pytest.raises(ValueError, match="flat"):
        m.infer([[[1, 2], [3, 4]]])


def test_queries_flatten_ragged_lists():
    q = cm.Queries([[5, 6, 7], [], [9]], weights=[[1, 2, 3], [], [4]])
    assert q.num_queries == 3 and list(q.offsets) == [0, 3, 3, 4] and list(q.word_ids) == [5, 6, 7, 9]
    assert q.word_ids.dtype == np.int64 and q.offsets.dtype == np.int64 and q.word_weights.dtype == np.float32
    st = q.as_struct()
    assert st.num_queries == 3 and st.word_ids == q.word_ids.ctypes.data and st.word_weights == q.word_weights.ctypes.data
    assert cm.Queries([[1]]).as_struct().word_weights is None
    o = cm.rank_options(50, 7, bias_coefficient=0, activation="identity", similarity="dot")
    assert (o.bias_coefficient, o.activation, o.similarity, o.top_k) == (0.0, ca.ACT_IDENTITY, ca.SIM_DOT, 7)
    assert cm.rank_options(50, 7, activation="hard_tanh").activation == ca.HARD_TANH


def test_self_information_weights():
    tf = np.array([1, 10, 250, 99999], np.int64)
    got = ca.self_information_weights(tf, 100000)
    assert got.dtype == np.float32
    np.testing.assert_allclose(got, -np.log(tf / 100000.0), rtol=1e-6)
    assert got[0] > got[1] > got[2] > got[3] > 0
    for bad in ((np.array([0, 3]), 10), (np.array([1, 3]), 0)):
        with pytest.raises(ValueError):
            ca.self_information_weights(*bad)


def test_the_benchmark_tool_fails_without_a_gpu():
    from tests.conftest import gpu_available
    if gpu_available():
        return                                # (with a GPU the tool runs: tools/bench_rank.py's own output is the check there)
    p = subprocess.run(["python", os.path.join(ROOT, "tools", "bench_rank.py"), "--docs", "1000", "--seconds", "0.01"],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)
