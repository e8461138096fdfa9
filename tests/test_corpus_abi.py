"""CPU-side checks of the window-reference boundary (nvsm_corpus_upload / nvsm_compute_cost_windows / nvsm_step_windows /
nvsm_step_windows_deferred): the symbols are declared and exported, null arguments are status codes that name the argument, the
ctypes structs have the C sizes and the training structs did not move, the C++ wrapper compiles, and expand_windows — the
reference of the GPU tests — and the Python layer's shape and dtype checks need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_corpus_upload", "nvsm_compute_cost_windows", "nvsm_step_windows", "nvsm_step_windows_deferred")


def test_the_header_declares_and_the_library_exports_the_window_calls():
    ca.build_library()
    names = ca.abi_symbols()
    for n in NEW:
        assert n in names
        assert hasattr(ca.lib(), n)
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert " T " + n in exported, n


def test_null_arguments_are_status_1_with_the_arguments_name():
    L = ca.lib()
    wb, corpus = ca.NvsmWindowBatch(), ca.NvsmCorpus()
    cost, ticket = C.c_float(), C.c_int64()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    assert L.nvsm_corpus_upload(None, C.byref(corpus)) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_compute_cost_windows(None, C.byref(wb), None) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_compute_cost_windows(fake, None, None) == 1 and b"null argument: windows" in L.nvsm_last_error()
    assert L.nvsm_step_windows(None, C.byref(wb), None, 0.1, C.byref(cost)) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_step_windows(fake, None, None, 0.1, C.byref(cost)) == 1 and b"null argument: windows" in L.nvsm_last_error()
    assert L.nvsm_step_windows_deferred(None, C.byref(wb), None, 0.1, C.byref(ticket)) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_step_windows_deferred(fake, None, None, 0.1, C.byref(ticket)) == 1 and b"null argument: windows" in L.nvsm_last_error()
    assert L.nvsm_step_windows_deferred(fake, C.byref(wb), None, 0.1, None) == 1 and b"null argument: ticket" in L.nvsm_last_error()


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(nvsm_corpus), sizeof(nvsm_window_batch),\n'
                   '  sizeof(nvsm_config), sizeof(nvsm_batch), offsetof(nvsm_corpus, num_tokens), offsetof(nvsm_window_batch, on_device),\n'
                   '  offsetof(nvsm_batch, num_instances), offsetof(nvsm_batch, on_device)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes[:4] == [C.sizeof(ca.NvsmCorpus), C.sizeof(ca.NvsmWindowBatch), C.sizeof(ca.NvsmConfig), C.sizeof(ca.NvsmBatch)]
    assert sizes[:2] == [64, 32]
    assert sizes[2:4] == [112, 48]          # nvsm_config and nvsm_batch did not move
    assert sizes[4:] == [ca.NvsmCorpus.num_tokens.offset, ca.NvsmWindowBatch.on_device.offset,
                         ca.NvsmBatch.num_instances.offset, ca.NvsmBatch.on_device.offset]
    assert sizes[6:] == [32, 40]


def test_the_cpp_wrapper_compiles_with_the_window_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m, const nvsm_corpus& c, const uint32_t* refs) {\n'
                   '  m.upload_corpus(&c); nvsm_window_batch wb = cunvsm_amd::Model::windows_of(refs, 4);\n'
                   '  m.compute_cost_windows(wb); float cost = m.step_windows(wb, 0.1f); int64_t t = m.step_windows_deferred(wb, 0.1f);\n'
                   '  m.wait_inputs(); cost += m.deferred_cost(t); (void)cost; m.upload_corpus(nullptr); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def small_corpus():
    tokens = np.array([5, 6, 7, 1, 2, 3, 4, 9, 8, 7, 6], np.int32)
    offsets = np.array([0, 3, 3, 7, 11], np.int64)      # lengths 3, 0, 4, 4
    return ca.Corpus(tokens, offsets, doc_weights=[1.0, 2.0, 3.0, 4.0], term_weights=np.arange(10) * 0.5)


def test_expand_windows_is_the_headers_definition():
    c = small_corpus()
    refs = np.array([[0, 0], [2, 1], [3, 0], [3, 1], [2, 1]], np.uint32)
    b = ca.expand_windows(c, refs, 3)
    assert b.features.dtype == np.int64 and b.labels.dtype == np.int64
    assert b.features.reshape(5, 3).tolist() == [[5, 6, 7], [2, 3, 4], [9, 8, 7], [8, 7, 6], [2, 3, 4]]
    assert b.labels.tolist() == [0, 2, 3, 3, 2]
    assert b.feature_weights.dtype == np.float32 and np.array_equal(b.feature_weights, (b.features * 0.5).astype(np.float32))
    assert b.weights.dtype == np.float32 and b.weights.tolist() == [1.0, 3.0, 4.0, 4.0, 3.0]
    assert b.num_instances == 5 and not b.on_device
    b.check_shapes(3)
    # without the weight tables the batch has no weight arrays: the twin of NULL is NULL
    plain = ca.Corpus(c.tokens, c.doc_offsets)
    b = ca.expand_windows(plain, refs, 1)
    assert b.feature_weights is None and b.weights is None and b.features.tolist() == [5, 2, 9, 8, 2]
    # the last document ends at num_tokens; a window of the whole document
    assert ca.expand_windows(plain, np.array([[3, 0]], np.uint32), 4).features.tolist() == [9, 8, 7, 6]
    # what the device would flag
    with pytest.raises(ValueError, match="document"):
        ca.expand_windows(c, np.array([[4, 0]], np.uint32), 1)
    with pytest.raises(ValueError, match="beyond"):
        ca.expand_windows(c, np.array([[0, 1]], np.uint32), 3)
    with pytest.raises(ValueError, match="beyond"):
        ca.expand_windows(c, np.array([[1, 0]], np.uint32), 1)       # the empty document holds no window
    with pytest.raises(ValueError, match="shape"):
        ca.expand_windows(c, np.zeros(4, np.uint32), 1)


def test_corpus_checks_need_no_device():
    tokens, off = np.arange(6, dtype=np.int32), np.array([0, 2, 6], np.int64)
    c = ca.Corpus(tokens, off)
    assert (c.num_tokens, c.num_documents) == (6, 2) and c.tokens.dtype == np.int32 and c.doc_offsets.dtype == np.int64
    st = c.as_struct()
    assert (st.num_tokens, st.num_documents, st.doc_weights, st.term_weights) == (6, 2, None, None)
    assert st.tokens == c.tokens.ctypes.data and st.doc_offsets == c.doc_offsets.ctypes.data and list(st.reserved) == [0] * 4
    assert ca.Corpus(np.arange(6, dtype=np.int64), [0, 2, 6]).tokens.dtype == np.int32      # narrowed, values kept
    with pytest.raises(ValueError, match="start at 0"):
        ca.Corpus(tokens, [1, 2, 6])
    with pytest.raises(ValueError, match="decrease"):
        ca.Corpus(tokens, [0, 4, 2, 6])
    with pytest.raises(ValueError, match="num_tokens"):
        ca.Corpus(tokens, [0, 2, 5])
    with pytest.raises(ValueError, match="doc_weights"):
        ca.Corpus(tokens, off, doc_weights=[1.0])
    with pytest.raises(ValueError, match="integers"):
        ca.Corpus(tokens.astype(np.float32), off)
    with pytest.raises(ValueError, match="flat"):
        ca.Corpus(tokens.reshape(2, 3), off)
    with pytest.raises(ValueError, match="int32"):
        ca.Corpus(np.array([2 ** 31], np.int64), [0, 1])


class StubModel(ca.Model):
    """a Model without a handle: everything the Python layer checks happens before the library is called"""

    def __init__(self, num_words=10, num_random=2):
        self.cfg = ca.NvsmConfig()
        self.cfg.num_words, self.cfg.num_entities, self.cfg.window_size, self.cfg.num_random_entities = num_words, 8, 3, num_random
        self._h = C.c_void_p()
        self._cb = None


def test_window_batch_checks_need_no_device():
    refs = np.array([[0, 0], [2, 1], [3, 1]], np.uint32)
    wb = ca.WindowBatch(refs)
    st = wb.as_struct()
    assert (st.num_instances, st.on_device, st.refs) == (3, 0, refs.ctypes.data) and list(st.reserved) == [0] * 3
    tail = ca.WindowBatch(refs[1:])                       # a row slice is passed where it lies (a slice of a pinned plan)
    assert tail.as_struct().refs == refs.ctypes.data + 8 and tail.num_instances == 2
    dev = ca.WindowBatch(0x1000, num_instances=7)         # a device pointer
    assert (dev.as_struct().refs, dev.as_struct().num_instances, dev.as_struct().on_device) == (0x1000, 7, 1)
    with pytest.raises(ValueError, match="uint32"):
        ca.WindowBatch(refs.astype(np.int64))
    with pytest.raises(ValueError, match="uint32"):
        ca.WindowBatch(refs.astype(np.int32))
    with pytest.raises(ValueError, match="shape"):
        ca.WindowBatch(refs.ravel())
    with pytest.raises(ValueError, match="shape"):
        ca.WindowBatch(np.zeros((2, 3), np.uint32))
    with pytest.raises(ValueError, match="empty"):
        ca.WindowBatch(np.zeros((0, 2), np.uint32))
    with pytest.raises(ValueError, match="num_instances"):
        ca.WindowBatch(refs, num_instances=2)
    with pytest.raises(ValueError, match="num_instances"):
        ca.WindowBatch(0x1000)
    with pytest.raises(ValueError, match="null"):
        ca.WindowBatch(0, num_instances=2)
    m = StubModel()
    with pytest.raises(ValueError, match="entity_ids"):
        m.step_windows(wb, 0.1, entity_ids=np.zeros(5, np.int64))
    with pytest.raises(ValueError, match="entity_ids"):
        m.compute_cost_windows(refs, entity_ids=np.zeros(10, np.int64))
    with pytest.raises(ValueError, match="term_weights"):
        m.upload_corpus(ca.Corpus(np.arange(6, dtype=np.int32), [0, 6], term_weights=np.ones(9)))
    assert cm.WindowBatch is ca.WindowBatch and cm.expand_windows is ca.expand_windows
