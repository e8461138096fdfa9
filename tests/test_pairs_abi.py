"""CPU-side checks of the pair-objective boundary (nvsm_compute_cost_mixed / nvsm_step_mixed): the symbols are declared and
exported, null arguments are status codes that name the argument, the ctypes structs have the C sizes (and nvsm_config did not
move), the C++ wrapper compiles, and the Python layer's shape checks need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_compute_cost_mixed", "nvsm_step_mixed")


def test_the_header_declares_and_the_library_exports_the_mixed_calls():
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
    assert L.nvsm_compute_cost_mixed(None, C.byref(b), None, C.byref(p), C.byref(x)) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_compute_cost_mixed(fake, C.byref(b), None, None, C.byref(x)) == 1 and b"null argument: pairs" in L.nvsm_last_error()
    assert L.nvsm_compute_cost_mixed(fake, C.byref(b), None, C.byref(p), None) == 1 and b"null argument: mix" in L.nvsm_last_error()
    assert L.nvsm_step_mixed(None, C.byref(b), None, C.byref(p), C.byref(x), 0.1, C.byref(cost)) == 1 and b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_step_mixed(fake, C.byref(b), None, None, C.byref(x), 0.1, None) == 1 and b"null argument: pairs" in L.nvsm_last_error()
    assert L.nvsm_step_mixed(fake, C.byref(b), None, C.byref(p), None, 0.1, None) == 1 and b"null argument: mix" in L.nvsm_last_error()
    assert L.nvsm_step_mixed(fake, None, None, None, None, 0.1, None) == 1 and b"null argument: pairs" in L.nvsm_last_error()


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(nvsm_pair_batch), sizeof(nvsm_mixture), sizeof(nvsm_config), sizeof(nvsm_batch)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [C.sizeof(ca.NvsmPairBatch), C.sizeof(ca.NvsmMixture), C.sizeof(ca.NvsmConfig), C.sizeof(ca.NvsmBatch)]
    assert sizes[:3] == [40, 16, 112]        # the training ABI did not move
    p = ca.NvsmPairBatch()
    assert list(p.reserved) == [0, 0, 0] and ca.NvsmPairBatch.on_device.offset == 24 and ca.NvsmMixture.pair_weight.offset == 4


def test_the_cpp_wrapper_compiles_with_the_mixed_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'float f(cunvsm_amd::Model& m, const cunvsm_amd::Batch& b) {\n'
                   '  std::vector<int64_t> ids{0, 1, 1, 2}; std::vector<float> w{1.f, 0.5f};\n'
                   '  cunvsm_amd::PairBatch p(ids.data(), w.data(), 2);\n'
                   '  m.compute_cost_mixed(&b, p, 0.7f, 0.3f); m.compute_gradients(); m.update(0.1f, m.scaled_regularization_lambda());\n'
                   '  m.compute_cost_mixed(nullptr, p);\n'
                   '  return m.step_mixed(&b, p, 0.1f, 0.7f, 0.3f) + m.step_mixed(nullptr, p, 0.1f) + static_cast<float>(p.num_pairs()); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


class StubModel(ca.Model):
    """a Model without a handle: everything the Python layer checks happens before the library is called"""

    def __init__(self, max_batch_size=8, window_size=2, num_random_entities=1):
        self.cfg = ca.NvsmConfig()
        self.cfg.max_batch_size, self.cfg.window_size, self.cfg.num_random_entities = max_batch_size, window_size, num_random_entities
        self._h = C.c_void_p()
        self._cb = None


def test_pair_batch_layout():
    p = ca.PairBatch([[3, 4], [5, 6], [3, 3]], [1.0, 0.5, 2.0])
    assert p.num_pairs == 3 and list(p.pairs) == [3, 4, 5, 6, 3, 3] and p.pairs.dtype == np.int64 and p.weights.dtype == np.float32
    st = p.as_struct()
    assert st.num_pairs == 3 and st.on_device == 0 and st.pairs == p.pairs.ctypes.data and st.weights == p.weights.ctypes.data
    flat = ca.PairBatch(np.array([3, 4, 5, 6]))
    assert flat.num_pairs == 2 and flat.as_struct().weights is None
    x = cm.mixture(0.25, 0.75)
    assert (x.text_weight, x.pair_weight, list(x.reserved)) == (0.25, 0.75, [0, 0])


def test_python_shape_checks_need_no_device():
    for bad in ([[1, 2, 3]], [1, 2, 3], [], np.zeros((2, 2, 2), np.int64)):
        with pytest.raises(ValueError, match="pairs"):
            ca.PairBatch(bad)
    with pytest.raises(ValueError, match="integer"):
        ca.PairBatch([[0.5, 1.0]])
    with pytest.raises(ValueError, match="weights"):
        ca.PairBatch([[1, 2], [3, 4]], [1.0])
    for wt, wp in ((0.0, 1.0), (1.0, 0.0), (-1.0, 2.0)):
        with pytest.raises(ValueError, match="> 0"):
            cm.mixture(wt, wp)
    m = StubModel()
    nine = ca.PairBatch(np.arange(18).reshape(9, 2))
    with pytest.raises(ValueError, match="max_batch_size"):
        m.compute_cost_mixed(None, nine)
    with pytest.raises(ValueError, match="max_batch_size"):
        m.step_mixed(None, nine, 0.1)
    ok = ca.PairBatch([[0, 1]])
    batch = ca.Batch(np.zeros(3, np.int64), np.zeros(2, np.int64))            # 3 ids for 2 windows of 2 words
    with pytest.raises(ValueError, match="features"):
        m.compute_cost_mixed(batch, ok)
    good = ca.Batch(np.zeros(4, np.int64), np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="entity_ids"):
        m.step_mixed(good, ok, 0.1, entity_ids=np.zeros(3, np.int64))
    with pytest.raises(ValueError, match="> 0"):
        m.compute_cost_mixed(good, ok, (1.0, 0.0))


def test_the_benchmark_tool_fails_without_a_gpu():
    from tests.conftest import gpu_available
    if gpu_available():
        return                                # (with a GPU the tool runs: tools/bench_pairs.py's own output is the check there)
    p = subprocess.run(["python", os.path.join(ROOT, "tools", "bench_pairs.py"), "--seconds", "0.01"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)
