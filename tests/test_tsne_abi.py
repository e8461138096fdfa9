"""CPU-side checks of the t-SNE boundary (nvsm_tsne / nvsm_tsne_options_default): the symbols are declared and exported, the hooks
live in the hooks library only and that library carries no kernel, null arguments are status 1 with their names, the defaults are
the header's, the ctypes struct has the C size, no earlier struct moved, the C++ wrapper compiles as C++11, and every refusal of
tsne_arguments that needs no device is raised."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT
from tests.test_neighbors_abi import StubModel

NEW = ("nvsm_tsne", "nvsm_tsne_options_default")
HOOKS = ("nvsm_debug_tsne_affinities", "nvsm_debug_tsne_gradient", "nvsm_debug_tsne_pca", "nvsm_debug_tsne_descent")
KERNELS = ("tsne_dist_kernel", "tsne_perplexity_kernel", "tsne_joint_kernel", "tsne_forces_kernel", "tsne_update_kernel", "tsne_kl_rows_kernel")
LAUNCHERS = ("launch_tsne_conditionals", "launch_tsne_joint", "launch_tsne_forces", "launch_tsne_update", "launch_tsne_kl_rows", "tsne_pca_start", "tsne_descent")


def test_the_header_declares_and_the_library_exports_the_tsne_calls():
    ca.build_library()
    names = ca.abi_symbols()
    for n in NEW:
        assert n in names
        assert hasattr(ca.lib(), n)
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert " T " + n in exported, n
    hooks = subprocess.run(["nm", "-D", "--defined-only", ca._lib._HOOKS_SO], capture_output=True, text=True, check=True).stdout
    for n in HOOKS:
        assert n in ca._lib.hook_symbols() and n not in exported and hasattr(ca.lib(), n)      # the hooks live in the test-hooks library only
        assert " T " + n in hooks
    for k in KERNELS:
        assert k not in hooks, "the hooks library carries no kernels of its own"
    for fn in LAUNCHERS:
        mangled = "_ZN6cunvsm%d%s" % (len(fn), fn)
        assert mangled in exported and mangled not in hooks      # what the hooks call is the product's


def test_null_arguments_are_status_1_with_their_names():
    L = ca.lib()
    o = ca.NvsmTsneOptions()
    out, kl, it = np.zeros(8, np.float32), C.c_double(), C.c_int32()
    args = [C.byref(o), out.ctypes.data, C.byref(kl), C.byref(it)]
    assert L.nvsm_tsne(None, *args) == 1 and b"null argument: m" in L.nvsm_last_error()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    for i, name in enumerate((b"opt", b"embedding", b"kl_divergence", b"n_iter")):
        a = list(args)
        a[i] = None
        assert L.nvsm_tsne(fake, *a) == 1 and b"null argument: " + name in L.nvsm_last_error(), name
    x = np.zeros(8, np.float32)
    p = x.ctypes.data
    assert L.nvsm_debug_tsne_affinities(None, 2, 1, 1.5, p, None) == 1 and b"null argument: X" in L.nvsm_last_error()
    assert L.nvsm_debug_tsne_affinities(p, 2, 1, 1.5, None, None) == 1 and b"null argument: P_out" in L.nvsm_last_error()
    assert L.nvsm_debug_tsne_gradient(None, p, 2, 1.0, p, C.byref(kl)) == 1 and b"null argument: P" in L.nvsm_last_error()
    assert L.nvsm_debug_tsne_gradient(p, p, 2, 1.0, p, None) == 1 and b"null argument: kl_out" in L.nvsm_last_error()
    assert L.nvsm_debug_tsne_pca(p, 2, 1, None) == 1 and b"null argument: Y0_out" in L.nvsm_last_error()
    assert L.nvsm_debug_tsne_descent(p, p, 2, None, 1, C.byref(kl), C.byref(it)) == 1 and b"null argument: opt" in L.nvsm_last_error()
    L.nvsm_tsne_options_default(None)       # a no-op, not a crash


def test_tsne_options_default():
    o = ca.NvsmTsneOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    ca.lib().nvsm_tsne_options_default(C.byref(o))
    assert (o.space, o.l2_normalize, o.ids, o.num_rows) == (ca.SPACE_ENTITIES, 0, None, 0)
    assert (o.perplexity, o.early_exaggeration, o.learning_rate, o.min_grad_norm) == (30.0, 12.0, 0.0, float(np.float32(1e-7)))
    assert (o.max_iter, o.n_iter_without_progress, o.init, o.init_embedding) == (1000, 300, ca.TSNE_INIT_PCA, None)
    assert o.reserved0 == 0 and list(o.reserved) == [0] * 6


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(nvsm_tsne_options),\n'
                   '  offsetof(nvsm_tsne_options, ids), offsetof(nvsm_tsne_options, perplexity), offsetof(nvsm_tsne_options, init_embedding),\n'
                   '  offsetof(nvsm_tsne_options, reserved), sizeof(nvsm_queries), sizeof(nvsm_rank_options),\n'
                   '  sizeof(nvsm_neighbor_options), sizeof(nvsm_config), sizeof(nvsm_neighbor_queries), sizeof(nvsm_ngram_options),\n'
                   '  NVSM_TSNE_MAX_ROWS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    N = ca.NvsmTsneOptions
    assert sizes[:5] == [C.sizeof(N), N.ids.offset, N.perplexity.offset, N.init_embedding.offset, N.reserved.offset] == [88, 8, 24, 56, 64]
    assert sizes[5:11] == [C.sizeof(ca.NvsmQueries), C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmNeighborOptions), C.sizeof(ca.NvsmConfig),
                           C.sizeof(ca.NvsmNeighborQueries), C.sizeof(ca.NvsmNgramOptions)]
    assert sizes[5:11] == [32, 48, 48, 112, 32, 56]      # no earlier struct changed size
    assert sizes[11] == ca.TSNE_MAX_ROWS == 32768


def test_the_cpp_wrapper_compiles_as_cpp11_with_the_tsne_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m) { nvsm_tsne_options o; nvsm_tsne_options_default(&o); o.l2_normalize = 1; o.max_iter = 500;\n'
                   '  std::vector<int64_t> ids{4, 1, 3};\n'
                   '  cunvsm_amd::Model::Tsne r = m.tsne(o), s = m.tsne(ids, o);\n'
                   '  (void)r.embedding; (void)s.kl_divergence; (void)s.n_iter; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_python_checks_need_no_device():
    m = StubModel()                             # 50 words, 100 entities, d_w = 12, d_e = 8
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(space="projected_words"), "space"), (dict(space="documents"), "space"), (dict(space=7), "space"),
                     (dict(ids=[1, 2], limit=5), "at most one"), (dict(ids=[[1, 2]]), "flat"),
                     (dict(ids=[3]), "at least 2"), (dict(limit=1), "at least 2"), (dict(limit=0), "at least 2"), (dict(limit=101), "exceeds"),
                     (dict(space="words", limit=51), "exceeds"),
                     (dict(ids=[1, 100]), "outside"), (dict(ids=[-1, 5]), "outside"), (dict(space="words", ids=[1, 50]), "outside"),
                     (dict(perplexity=nan), "perplexity"), (dict(perplexity=0), "perplexity"), (dict(perplexity=-3.0), "perplexity"),
                     (dict(perplexity=100.0), "perplexity"), (dict(ids=[1, 2, 3], perplexity=3.0), "perplexity"), (dict(perplexity=inf), "perplexity"),
                     (dict(early_exaggeration=0), "early_exaggeration"), (dict(early_exaggeration=nan), "early_exaggeration"),
                     (dict(learning_rate="fast"), "learning_rate"), (dict(learning_rate=0.0), "learning_rate"), (dict(learning_rate=inf), "learning_rate"),
                     (dict(min_grad_norm=nan), "min_grad_norm"),
                     (dict(init="spectral"), "init"), (dict(init=np.zeros((99, 2))), "shape"), (dict(init=np.zeros((100, 3))), "shape"),
                     (dict(init=np.full((100, 2), nan)), "finite"),
                     (dict(max_iter=0), "max_iter"), (dict(n_iter_without_progress=-1), "n_iter_without_progress")):
        with pytest.raises(ValueError, match=word):
            m.tsne(**kw)
    with pytest.raises(ValueError, match="limit of 32768"):
        StubModel(num_entities=40000).tsne()


def test_tsne_arguments_fill_the_struct():
    cfg = StubModel().cfg
    o, n, keep = cm.tsne_arguments(cfg)
    assert n == 100 and (o.space, o.l2_normalize, o.ids, o.num_rows, o.init, o.init_embedding) == (ca.SPACE_ENTITIES, 0, None, 100, ca.TSNE_INIT_PCA, None)
    assert (o.perplexity, o.early_exaggeration, o.learning_rate, o.max_iter, o.n_iter_without_progress) == (30.0, 12.0, 0.0, 1000, 300)
    assert o.min_grad_norm == float(np.float32(1e-7))
    o, n, keep = cm.tsne_arguments(cfg, "words", ids=[9, 3, 4], l2_normalize=True, perplexity=2, learning_rate=200, max_iter=7, init="random")
    ids, given = keep
    assert n == 3 and (o.space, o.l2_normalize, o.num_rows, o.learning_rate, o.max_iter) == (ca.SPACE_WORDS, 1, 3, 200.0, 7)
    assert o.ids == ids.ctypes.data and list(ids) == [9, 3, 4] and ids.dtype == np.int64      # any order, kept as given
    assert o.init == ca.TSNE_INIT_GIVEN and o.init_embedding == given.ctypes.data and given.dtype == np.float32
    want = (1e-4 * np.random.RandomState(0).standard_normal(size=(3, 2))).astype(np.float32)      # sklearn's own expression
    assert np.array_equal(given, want)
    o, n, keep = cm.tsne_arguments(cfg, limit=40, init=np.ones((40, 2)), random_state=5)
    assert n == 40 and o.ids is None and o.num_rows == 40 and o.init == ca.TSNE_INIT_GIVEN and (keep[1] == 1).all()


def test_the_benchmark_tool_fails_without_a_gpu():
    from tests.conftest import gpu_available
    if gpu_available():
        return                                # (with a GPU the tool runs: tools/bench_tsne.py's own output is the check there)
    p = subprocess.run(["python", os.path.join(ROOT, "tools", "bench_tsne.py"), "--rows", "100", "--iterations", "10"],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)
