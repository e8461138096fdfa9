"""CPU-side checks of the evaluation boundary (nvsm_evaluate): the symbol is declared and exported, null arguments are status
codes that name the argument, the ctypes struct has the C layout (and the ranking structs did not move), the C++ wrapper
compiles, and the Python layer's checks need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import _lib
from cunvsm_amd import model as cm
from tests.conftest import ROOT


def test_the_header_declares_and_the_library_exports_nvsm_evaluate():
    ca.build_library()
    assert "nvsm_evaluate" in ca.abi_symbols() and hasattr(ca.lib(), "nvsm_evaluate")
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    assert " T nvsm_evaluate" in exported
    symbols = subprocess.run(["nm", "-C", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    assert "eval_metrics_kernel" in symbols, "the metrics kernel of eval.hip is part of the library"


def test_null_arguments_are_status_1_with_the_arguments_name():
    L = ca.lib()
    q, o, j = ca.NvsmQueries(), ca.NvsmRankOptions(), ca.NvsmJudgments()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    out = np.zeros(8)
    assert L.nvsm_evaluate(None, C.byref(q), C.byref(o), C.byref(j), out.ctypes.data, None, None, None) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_evaluate(fake, None, C.byref(o), C.byref(j), out.ctypes.data, None, None, None) == 1 and b"null argument: queries" in L.nvsm_last_error()
    assert L.nvsm_evaluate(fake, C.byref(q), None, C.byref(j), out.ctypes.data, None, None, None) == 1 and b"null argument: opt" in L.nvsm_last_error()
    assert L.nvsm_evaluate(fake, C.byref(q), C.byref(o), None, out.ctypes.data, None, None, None) == 1 and b"null argument: judgments" in L.nvsm_last_error()


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(nvsm_judgments), offsetof(nvsm_judgments, doc_ids),\n'
                   '  offsetof(nvsm_judgments, grades), offsetof(nvsm_judgments, offsets), offsetof(nvsm_judgments, cutoffs),\n'
                   '  offsetof(nvsm_judgments, num_cutoffs), offsetof(nvsm_judgments, reserved), sizeof(nvsm_rank_options), sizeof(nvsm_queries),\n'
                   '  NVSM_EVAL_MAX_CUTOFFS, NVSM_EVAL_FIXED);\n'
                   '  printf("%d %d %d %d %d %d %d\\n", NVSM_EVAL_NUM_RET, NVSM_EVAL_NUM_REL, NVSM_EVAL_NUM_REL_RET, NVSM_EVAL_AP, NVSM_EVAL_RPREC,\n'
                   '  NVSM_EVAL_RECIP_RANK, NVSM_EVAL_NDCG); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    J = ca.NvsmJudgments
    assert [int(x) for x in lines[0].split()] == [
        C.sizeof(J), J.doc_ids.offset, J.grades.offset, J.offsets.offset, J.cutoffs.offset, J.num_cutoffs.offset, J.reserved.offset,
        C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmQueries), ca.EVAL_MAX_CUTOFFS, _lib.EVAL_FIXED]
    assert (C.sizeof(J), J.num_cutoffs.offset, C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmQueries)) == (48, 32, 48, 32)
    assert [int(x) for x in lines[1].split()] == [_lib.EVAL_NUM_RET, _lib.EVAL_NUM_REL, _lib.EVAL_NUM_REL_RET, _lib.EVAL_AP, _lib.EVAL_RPREC,
                                                  _lib.EVAL_RECIP_RANK, _lib.EVAL_NDCG] == list(range(7))
    assert len(cm.EVAL_FIXED_NAMES) == _lib.EVAL_FIXED
    assert list(J().reserved) == [0, 0, 0]


def test_the_cpp_wrapper_compiles_with_evaluate(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'double f(cunvsm_amd::Model& m) {\n'
                   '  std::vector<int64_t> words{1, 2, 3}, off{0, 2, 3}, docs{4, -1, 7}, joff{0, 2, 3};\n'
                   '  std::vector<int32_t> grades{1, 2, 0}, cut{5, 10};\n'
                   '  nvsm_rank_options o; nvsm_rank_options_default(&o); o.top_k = 10;\n'
                   '  nvsm_judgments j = {docs.data(), grades.data(), joff.data(), cut.data(), 2, {0, 0, 0}};\n'
                   '  cunvsm_amd::Model::Evaluation e = m.evaluate(words, off, o, j);\n'
                   '  cunvsm_amd::Model::Evaluation e2 = m.evaluate(words, off, o, j, nullptr, false);\n'
                   '  return e.metrics[NVSM_EVAL_AP] + e.metrics[e.width + NVSM_EVAL_FIXED + 3 * 1 + 2] + e2.metrics[0] + e.ranking.counts[0]; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


class StubModel(ca.Model):
    """a Model without a handle: everything the Python layer checks happens before the library is called"""

    def __init__(self, num_entities=100):
        self.cfg = ca.NvsmConfig()
        self.cfg.num_entities = num_entities
        self._h = C.c_void_p()
        self._cb = None


def test_judgments_layout():
    j = ca.Judgments([[(5, 1), (-1, 2), (3, 0)], [], [(7, -1)]])
    assert j.num_queries == 3 and list(j.offsets) == [0, 3, 3, 4]
    assert list(j.doc_ids) == [5, -1, 3, 7] and list(j.grades) == [1, 2, 0, -1]
    assert j.doc_ids.dtype == np.int64 and j.grades.dtype == np.int32 and j.offsets.dtype == np.int64
    cut = cm.eval_cutoffs((5, 10))
    st = j.as_struct(cut)
    assert (st.doc_ids, st.grades, st.offsets, st.cutoffs, st.num_cutoffs) == (
        j.doc_ids.ctypes.data, j.grades.ctypes.data, j.offsets.ctypes.data, cut.ctypes.data, 2)
    empty = ca.Judgments([[], []]).as_struct(cm.eval_cutoffs(()))
    assert empty.doc_ids is None and empty.cutoffs is None and empty.num_cutoffs == 0
    assert ca.Judgments([[(-1, 1), (-1, 1)]]).doc_ids.size == 2      # documents the model does not hold may repeat
    assert cm.eval_metric_names((5, 10)) == ["num_ret", "num_rel", "num_rel_ret", "map", "Rprec", "recip_rank", "ndcg",
                                             "P_5", "recall_5", "ndcg_cut_5", "P_10", "recall_10", "ndcg_cut_10"]


def test_python_checks_need_no_device():
    with pytest.raises(ValueError, match="pairs"):
        ca.Judgments([[1, 2, 3]])
    with pytest.raises(ValueError, match="pairs"):
        ca.Judgments([[(1, 2, 3)]])
    with pytest.raises(ValueError, match="twice"):
        ca.Judgments([[(4, 1), (5, 1), (4, 0)]])
    m = StubModel(100)
    one = [[(4, 1)]]
    with pytest.raises(ValueError, match="one per query"):
        m.evaluate([[1], [2]], one, top_k=10)
    for bad in (100, -2):
        with pytest.raises(ValueError, match="judged document id"):
            m.evaluate([[1]], [[(bad, 1)]], top_k=10)
    with pytest.raises(ValueError, match="at most 8"):
        m.evaluate([[1]], one, top_k=10, cutoffs=range(1, 10))
    with pytest.raises(ValueError, match="ascend"):
        m.evaluate([[1]], one, top_k=10, cutoffs=(5, 5))
    with pytest.raises(ValueError, match="ascend"):
        m.evaluate([[1]], one, top_k=10, cutoffs=(10, 5))
    with pytest.raises(ValueError, match="cutoff"):
        m.evaluate([[1]], one, top_k=10, cutoffs=(0, 5))
    with pytest.raises(ValueError, match="top_k"):
        m.evaluate([[1]], one, top_k=101)
    with pytest.raises(ValueError, match="top_k"):
        m.evaluate([[1]], one, top_k=0)
    with pytest.raises(ValueError, match="candidate"):
        m.evaluate([[1]], one, top_k=10, candidates=[[100]])
    with pytest.raises(ValueError, match="one per query"):
        m.evaluate([[1]], one, top_k=10, candidates=[[1], [2]])
    with pytest.raises(ValueError, match="similarity"):
        m.evaluate([[1]], one, top_k=10, similarity="euclid")
    with pytest.raises(ValueError, match="weights"):
        m.evaluate([[1, 2]], one, top_k=10, weights=[[1.0]])
