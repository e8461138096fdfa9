"""CPU-side checks of the term-pair boundary (nvsm_compute_cost_term_mixed / nvsm_step_term_mixed): the symbols are declared and
exported, null arguments are status codes that name the argument, the pair structs did not move, the C++ wrapper compiles, the
Python methods exist and check shapes without a device, and on a machine without a GPU the handle these calls need is refused with
the no-device status (there is no CPU path behind them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from tests.conftest import ROOT, gpu_available

NEW = ("nvsm_compute_cost_term_mixed", "nvsm_step_term_mixed")


def test_the_header_declares_and_the_library_exports_the_term_calls():
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
    b, p, x = ca.NvsmBatch(), ca.NvsmPairBatch(), ca.NvsmMixture(0.5, 0.5)
    cost = C.c_float()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    assert L.nvsm_compute_cost_term_mixed(None, C.byref(b), None, C.byref(p), C.byref(x)) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_compute_cost_term_mixed(fake, C.byref(b), None, None, C.byref(x)) == 1 and b"null argument: pairs" in L.nvsm_last_error()
    assert L.nvsm_compute_cost_term_mixed(fake, C.byref(b), None, C.byref(p), None) == 1 and b"null argument: mix" in L.nvsm_last_error()
    assert L.nvsm_step_term_mixed(None, C.byref(b), None, C.byref(p), C.byref(x), 0.1, C.byref(cost)) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_step_term_mixed(fake, C.byref(b), None, None, C.byref(x), 0.1, None) == 1 and b"null argument: pairs" in L.nvsm_last_error()
    assert L.nvsm_step_term_mixed(fake, C.byref(b), None, C.byref(p), None, 0.1, None) == 1 and b"null argument: mix" in L.nvsm_last_error()
    assert L.nvsm_step_term_mixed(fake, None, None, None, None, 0.1, None) == 1 and b"null argument: pairs" in L.nvsm_last_error()


def test_the_calls_take_the_existing_structs_unchanged():
    L = ca.lib()
    for n, entity_twin in zip(NEW, ("nvsm_compute_cost_mixed", "nvsm_step_mixed")):
        assert getattr(L, n).argtypes == getattr(L, entity_twin).argtypes and getattr(L, n).restype == getattr(L, entity_twin).restype
    assert C.sizeof(ca.NvsmPairBatch) == 40 and C.sizeof(ca.NvsmMixture) == 16
    assert list(ca.NvsmPairBatch().reserved) == [0, 0, 0]


def test_the_cpp_wrapper_compiles_with_the_term_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'float f(cunvsm_amd::Model& m, const cunvsm_amd::Batch& b) {\n'
                   '  std::vector<int64_t> ids{0, 1, 1, 2}; std::vector<float> w{1.f, 0.5f};\n'
                   '  cunvsm_amd::PairBatch p(ids.data(), w.data(), 2);\n'
                   '  m.compute_cost_term_mixed(&b, p, 0.7f, 0.3f); m.compute_gradients(); m.update(0.1f, m.scaled_regularization_lambda());\n'
                   '  m.compute_cost_term_mixed(nullptr, p);\n'
                   '  return m.step_term_mixed(&b, p, 0.1f, 0.7f, 0.3f) + m.step_term_mixed(nullptr, p, 0.1f); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


class StubModel(ca.Model):
    """a Model without a handle: everything the Python layer checks happens before the library is called"""

    def __init__(self, max_batch_size=8, window_size=2, num_random_entities=1):
        self.cfg = ca.NvsmConfig()
        self.cfg.max_batch_size, self.cfg.window_size, self.cfg.num_random_entities = max_batch_size, window_size, num_random_entities
        self._h = C.c_void_p()
        self._cb = None


def test_python_methods_exist_and_check_shapes_without_a_device():
    assert callable(ca.Model.compute_cost_term_mixed) and callable(ca.Model.step_term_mixed)
    m = StubModel()
    nine = ca.PairBatch(np.arange(18).reshape(9, 2))
    with pytest.raises(ValueError, match="max_batch_size"):
        m.compute_cost_term_mixed(None, nine)
    with pytest.raises(ValueError, match="max_batch_size"):
        m.step_term_mixed(None, nine, 0.1)
    ok = ca.PairBatch([[0, 1]])
    batch = ca.Batch(np.zeros(3, np.int64), np.zeros(2, np.int64))            # 3 ids for 2 windows of 2 words
    with pytest.raises(ValueError, match="features"):
        m.compute_cost_term_mixed(batch, ok)
    good = ca.Batch(np.zeros(4, np.int64), np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="> 0"):
        m.step_term_mixed(good, ok, 0.1, (1.0, 0.0))
    # the null handle of the stub reaches the library: status 1, the handle named
    with pytest.raises(ca.NvsmError) as e:
        m.compute_cost_term_mixed(None, ok)
    assert e.value.status == 1 and "null argument: m" in str(e.value)


def test_without_a_gpu_the_handle_of_these_calls_is_the_no_device_status():
    if gpu_available():
        return                                # (with a GPU the calls run: tests/test_gpu_term_pairs.py)
    from tests.helpers import gpu_model
    spec = dict(num_words=20, num_entities=10, word_dim=8, entity_dim=8, window=2, num_random=1)
    with pytest.raises(ca.NvsmError) as e:
        gpu_model(spec, 8).step_term_mixed(None, ca.PairBatch([[0, 1]]), 0.1)
    assert e.value.status == 5


def test_the_benchmark_tool_fails_without_a_gpu():
    if gpu_available():
        return                                # (with a GPU the tool runs: its own output is the check there)
    p = subprocess.run(["python", os.path.join(ROOT, "tools", "bench_term_pairs.py"), "--seconds", "0.01"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)
