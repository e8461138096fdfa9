"""CPU-side checks of the sparse t-SNE boundary (nvsm_tsne_sparse / nvsm_tsne_sparse_options_default): the symbols are declared and
exported, the hooks live in the hooks library only, null arguments are status 1 with their names, the defaults are the header's, the
ctypes struct has the C size while nvsm_tsne_options keeps its own, the C++ wrapper compiles as C++11, and every refusal of
tsne_arguments(method="sparse") that needs no device is raised."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT
from tests.test_neighbors_abi import StubModel

NEW = ("nvsm_tsne_sparse", "nvsm_tsne_sparse_options_default")
HOOKS = ("nvsm_debug_tsne_knn", "nvsm_debug_tsne_sparse_affinities", "nvsm_debug_tsne_sparse_gradient", "nvsm_debug_tsne_sparse_descent")
LAUNCHERS = ("launch_tsne_nn_scores", "launch_tsne_nn_conditionals", "launch_tsne_sparse_forces", "launch_tsne_sparse_update",
             "launch_tsne_sparse_kl_rows", "tsne_sparse_knn", "tsne_sparse_affinities", "tsne_sparse_descent")


def test_the_header_declares_and_the_library_exports_the_sparse_tsne_calls():
    ca.build_library()
    names = ca.abi_symbols()
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert n in names and hasattr(ca.lib(), n)
        assert " T " + n in exported, n
    hooks = subprocess.run(["nm", "-D", "--defined-only", ca._lib._HOOKS_SO], capture_output=True, text=True, check=True).stdout
    for n in HOOKS:
        assert n in ca._lib.hook_symbols() and n not in exported and hasattr(ca.lib(), n)      # the hooks live in the test-hooks library only
        assert " T " + n in hooks
    assert "tsne_sp_repulsion_kernel" not in hooks, "the hooks library carries no kernels of its own"
    for fn in LAUNCHERS:
        mangled = "_ZN6cunvsm%d%s" % (len(fn), fn)
        assert mangled in exported and mangled not in hooks      # what the hooks call is the product's


def test_null_arguments_are_status_1_with_their_names():
    L = ca.lib()
    o, sp = ca.NvsmTsneOptions(), ca.NvsmTsneSparseOptions()
    out, kl, it = np.zeros(8, np.float32), C.c_double(), C.c_int32()
    args = [C.byref(o), C.byref(sp), out.ctypes.data, C.byref(kl), C.byref(it)]
    assert L.nvsm_tsne_sparse(None, *args) == 1 and b"null argument: m" in L.nvsm_last_error()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    for i, name in ((0, b"opt"), (2, b"embedding"), (3, b"kl_divergence"), (4, b"n_iter")):      # (sparse may be NULL: the defaults)
        a = list(args)
        a[i] = None
        assert L.nvsm_tsne_sparse(fake, *a) == 1 and b"null argument: " + name in L.nvsm_last_error(), name
    p = np.zeros(8, np.float32).ctypes.data
    for i, name in ((0, b"X"), (5, b"ids_out"), (6, b"d2_out")):
        a = [p, 2, 1, 1, 0, p, p]
        a[i] = None
        assert L.nvsm_debug_tsne_knn(*a) == 1 and b"null argument: " + name in L.nvsm_last_error(), name
    for i, name in ((0, b"X"), (5, b"indptr_out"), (6, b"indices_out"), (7, b"data_out")):      # (cond_out may be NULL)
        a = [p, 2, 1, 1.5, 1, p, p, p, None]
        a[i] = None
        assert L.nvsm_debug_tsne_sparse_affinities(*a) == 1 and b"null argument: " + name in L.nvsm_last_error(), name
    for i, name in ((0, b"indptr"), (1, b"indices"), (2, b"data"), (3, b"Y"), (7, b"grad_out"), (8, b"kl_out")):
        a = [p, p, p, p, 2, 1.0, 0, p, C.byref(kl)]
        a[i] = None
        assert L.nvsm_debug_tsne_sparse_gradient(*a) == 1 and b"null argument: " + name in L.nvsm_last_error(), name
    for i, name in ((0, b"indptr"), (1, b"indices"), (2, b"data"), (3, b"Y"), (5, b"opt"), (7, b"kl_out"), (8, b"n_iter_out")):
        a = [p, p, p, p, 2, C.byref(o), 1, C.byref(kl), C.byref(it)]
        a[i] = None
        assert L.nvsm_debug_tsne_sparse_descent(*a) == 1 and b"null argument: " + name in L.nvsm_last_error(), name
    L.nvsm_tsne_sparse_options_default(None)       # a no-op, not a crash


def test_sparse_options_default():
    o = ca.NvsmTsneSparseOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    ca.lib().nvsm_tsne_sparse_options_default(C.byref(o))
    assert o.n_neighbors == 0 and list(o.reserved) == [0] * 7


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(nvsm_tsne_sparse_options),\n'
                   '  offsetof(nvsm_tsne_sparse_options, n_neighbors), offsetof(nvsm_tsne_sparse_options, reserved), sizeof(nvsm_tsne_options),\n'
                   '  NVSM_TSNE_SPARSE_MAX_ROWS, NVSM_TSNE_SPARSE_MAX_NEIGHBORS, NVSM_TSNE_MAX_ROWS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = ca.NvsmTsneSparseOptions
    assert sizes[:3] == [C.sizeof(S), S.n_neighbors.offset, S.reserved.offset] == [32, 0, 4]
    assert sizes[3] == C.sizeof(ca.NvsmTsneOptions) == 88      # the exact call's struct did not move
    assert sizes[4:] == [ca.TSNE_SPARSE_MAX_ROWS, ca.TSNE_SPARSE_MAX_NEIGHBORS, ca.TSNE_MAX_ROWS] == [1048576, 1024, 32768]


def test_the_cpp_wrapper_compiles_as_cpp11_with_the_sparse_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m) { nvsm_tsne_options o; nvsm_tsne_options_default(&o); o.max_iter = 500;\n'
                   '  std::vector<int64_t> ids{4, 1, 3};\n'
                   '  cunvsm_amd::Model::Tsne r = m.tsne_sparse(o), s = m.tsne_sparse(ids, o, 2), t = m.tsne_sparse(o, 90);\n'
                   '  (void)r.embedding; (void)s.kl_divergence; (void)t.n_iter; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_python_checks_need_no_device():
    m = StubModel()                             # 50 words, 100 entities
    with pytest.raises(ValueError, match="method"):
        m.tsne(method="spectral")
    with pytest.raises(ValueError, match="n_neighbors"):
        m.tsne(n_neighbors=5)                   # belongs to the sparse method
    for k in (0, 100, -1, ca.TSNE_SPARSE_MAX_NEIGHBORS + 1):
        with pytest.raises(ValueError, match="n_neighbors"):
            m.tsne(method="sparse", n_neighbors=k)
    with pytest.raises(ValueError, match="n_neighbors"):
        StubModel(num_entities=5000).tsne(method="sparse", n_neighbors=ca.TSNE_SPARSE_MAX_NEIGHBORS + 1)
    with pytest.raises(ValueError, match="neighbours"):      # the default k of this perplexity is above the cap
        StubModel(num_entities=5000).tsne(method="sparse", perplexity=400.0)
    # what the exact call refuses is refused alike, in its order: the row checks come before n_neighbors
    for kw, word in ((dict(space="projected_words"), "space"), (dict(limit=1), "at least 2"), (dict(limit=101), "exceeds"),
                     (dict(ids=[1, 100]), "outside"), (dict(perplexity=100.0), "perplexity"), (dict(init="spectral"), "init"),
                     (dict(max_iter=0), "max_iter")):
        with pytest.raises(ValueError, match=word):
            m.tsne(method="sparse", n_neighbors=1000, **kw)
    big = StubModel(num_entities=40000).cfg
    o, n, keep = cm.tsne_arguments(big, method="sparse")
    assert n == 40000 and o.num_rows == 40000 and keep[2].n_neighbors == 0
    with pytest.raises(ValueError, match="limit of 32768"):
        cm.tsne_arguments(big)
    with pytest.raises(ValueError, match="limit of 32768"):
        cm.tsne_arguments(big, method="exact")
    with pytest.raises(ValueError, match="limit of 1048576"):
        cm.tsne_arguments(StubModel(num_entities=ca.TSNE_SPARSE_MAX_ROWS + 1).cfg, method="sparse")
    cm.tsne_arguments(StubModel(num_entities=ca.TSNE_SPARSE_MAX_ROWS).cfg, method="sparse")      # the cap itself, 91 neighbours: 2nk < 2^31
    with pytest.raises(ValueError, match="directed entries"):
        cm.tsne_arguments(StubModel(num_entities=ca.TSNE_SPARSE_MAX_ROWS).cfg, method="sparse", n_neighbors=1024)


def test_tsne_arguments_fill_the_sparse_struct():
    cfg = StubModel().cfg
    o, n, keep = cm.tsne_arguments(cfg, "words", ids=[9, 3, 4], perplexity=2, method="sparse", n_neighbors=2)
    ids, given, sp = keep
    assert n == 3 and o.space == ca.SPACE_WORDS and list(ids) == [9, 3, 4] and given is None and sp.n_neighbors == 2 and list(sp.reserved) == [0] * 7
    exact = cm.tsne_arguments(cfg, "words", ids=[9, 3, 4], perplexity=2)
    assert bytes(o)[:8] == bytes(exact[0])[:8] and bytes(o)[16:] == bytes(exact[0])[16:] and len(exact[2]) == 2      # the same options either way


def test_the_benchmark_tool_fails_without_a_gpu():
    from tests.conftest import gpu_available
    if gpu_available():
        return                                # (with a GPU the tool runs: tools/bench_tsne_sparse.py's own output is the check there)
    p = subprocess.run(["python", os.path.join(ROOT, "tools", "bench_tsne_sparse.py"), "--rows", "100", "--big-rows", "", "--iterations", "10"],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)
