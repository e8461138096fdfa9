"""CPU-side checks of the k-means boundary (nvsm_kmeans / nvsm_kmeans_options_default): the symbols are declared and exported, the
hooks live in the hooks library only and that library carries no kernel, null arguments are status 1 with their names, the defaults
are the header's, the ctypes struct has the C layout, no earlier struct moved, the C++ wrapper compiles as C++11, and every refusal
of kmeans_arguments that needs no device is raised, in the ABI's order."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import model as cm
from tests.conftest import ROOT
from tests.test_neighbors_abi import StubModel

NEW = ("nvsm_kmeans", "nvsm_kmeans_options_default")
HOOKS = ("nvsm_debug_kmeans_assign", "nvsm_debug_kmeans_update", "nvsm_debug_kmeans_plusplus")
KERNELS = ("kmeans_assign_kernel", "kmeans_segsum_kernel", "kmeans_finish_kernel", "kmeans_rowdist_kernel", "kmeans_kpp_pick_kernel")
LAUNCHERS = ("launch_kmeans_assign", "launch_kmeans_update", "launch_kmeans_kpp_pick", "kmeans_assign_pass", "kmeans_update_pass", "kmeans_plusplus",
             "kmeans_assign_uses_mfma")


def test_the_header_declares_and_the_library_exports_the_kmeans_calls():
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
    o = ca.NvsmKmeansOptions()
    out, inertia, it = np.zeros(8, np.int64), C.c_double(), C.c_int32()
    p = out.ctypes.data
    args = [C.byref(o), p, p, p, None, C.byref(inertia), C.byref(it)]      # distances may be NULL
    assert L.nvsm_kmeans(None, *args) == 1 and b"null argument: m" in L.nvsm_last_error()
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    for i, name in ((0, b"opt"), (1, b"labels"), (2, b"centers"), (3, b"counts"), (5, b"inertia"), (6, b"n_iter")):
        a = list(args)
        a[i] = None
        assert L.nvsm_kmeans(fake, *a) == 1 and b"null argument: " + name in L.nvsm_last_error(), name
    sh = C.c_double()
    assert L.nvsm_debug_kmeans_assign(None, 2, 1, p, 1, p, None) == 1 and b"null argument: X" in L.nvsm_last_error()
    assert L.nvsm_debug_kmeans_assign(p, 2, 1, None, 1, p, None) == 1 and b"null argument: C" in L.nvsm_last_error()
    assert L.nvsm_debug_kmeans_assign(p, 2, 1, p, 1, None, None) == 1 and b"null argument: labels_out" in L.nvsm_last_error()
    assert L.nvsm_debug_kmeans_update(p, 2, 1, None, p, 1, p, p, C.byref(sh)) == 1 and b"null argument: labels" in L.nvsm_last_error()
    assert L.nvsm_debug_kmeans_update(p, 2, 1, p, p, 1, p, p, None) == 1 and b"null argument: shift_out" in L.nvsm_last_error()
    assert L.nvsm_debug_kmeans_plusplus(p, 2, 1, 1, 1, None, None) == 1 and b"null argument: rows_out" in L.nvsm_last_error()
    L.nvsm_kmeans_options_default(None)     # a no-op, not a crash


def test_kmeans_options_default():
    o = ca.NvsmKmeansOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    ca.lib().nvsm_kmeans_options_default(C.byref(o))
    assert (o.space, o.l2_normalize, o.ids, o.num_rows) == (ca.SPACE_ENTITIES, 0, None, 0)
    assert (o.num_clusters, o.max_iter, o.tol, o.init, o.init_centers, o.seed) == (8, 300, 1e-4, ca.KMEANS_INIT_PLUSPLUS, None, 1)
    assert o.reserved0 == 0 and list(o.reserved) == [0] * 6
    assert (ca.KMEANS_INIT_PLUSPLUS, ca.KMEANS_INIT_GIVEN) == (0, 1)


def test_struct_layout_matches_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    fields = ("space", "l2_normalize", "ids", "num_rows", "num_clusters", "max_iter", "tol", "init", "reserved0", "init_centers", "seed", "reserved")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu", sizeof(nvsm_kmeans_options));\n' +
                   "".join('  printf(" %%zu", offsetof(nvsm_kmeans_options, %s));\n' % f for f in fields) +
                   '  printf(" %zu %zu %zu %zu %d %d %d\\n", sizeof(nvsm_tsne_options), sizeof(nvsm_rank_options), sizeof(nvsm_neighbor_options),\n'
                   '    sizeof(nvsm_config), NVSM_KMEANS_MAX_CLUSTERS, NVSM_KMEANS_INIT_PLUSPLUS, NVSM_KMEANS_INIT_GIVEN); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    N = ca.NvsmKmeansOptions
    assert sizes[0] == C.sizeof(N) == 88
    assert sizes[1:13] == [getattr(N, f).offset for f in fields] == [0, 4, 8, 16, 24, 28, 32, 40, 44, 48, 56, 64]
    assert sizes[13:17] == [C.sizeof(ca.NvsmTsneOptions), C.sizeof(ca.NvsmRankOptions), C.sizeof(ca.NvsmNeighborOptions), C.sizeof(ca.NvsmConfig)]
    assert sizes[13:17] == [88, 48, 48, 112]      # no earlier struct changed size
    assert sizes[17:] == [ca.KMEANS_MAX_CLUSTERS, 0, 1] and ca.KMEANS_MAX_CLUSTERS == 4096


def test_the_cpp_wrapper_compiles_as_cpp11_with_the_kmeans_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m) { nvsm_kmeans_options o; nvsm_kmeans_options_default(&o); o.num_clusters = 12; o.seed = 4;\n'
                   '  std::vector<int64_t> ids{4, 1, 3, 1};\n'
                   '  cunvsm_amd::Model::Kmeans r = m.kmeans(o), s = m.kmeans(ids, o);\n'
                   '  (void)r.labels; (void)r.centers; (void)s.counts; (void)s.distances; (void)s.inertia; (void)s.n_iter; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_python_checks_need_no_device_and_come_in_the_abis_order():
    m = StubModel()                             # 50 words, 100 entities, d_w = 12, d_e = 8
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(space="projected_words", limit=0), "space"), (dict(space="documents"), "space"), (dict(space=7), "space"),
                     (dict(ids=[1, 2], limit=5), "at most one"), (dict(ids=[[1, 2]]), "flat"),
                     (dict(limit=0, num_clusters=0), "at least 1"), (dict(limit=101, num_clusters=0), "exceeds"), (dict(space="words", limit=51), "exceeds"),
                     (dict(ids=[1, 100], num_clusters=0), "outside"), (dict(ids=[-1, 5]), "outside"), (dict(space="words", ids=[1, 50]), "outside"),
                     (dict(num_clusters=0, max_iter=0), "num_clusters"), (dict(num_clusters=101, max_iter=0), "num_clusters"),
                     (dict(ids=[3, 3, 4], num_clusters=4), "num_clusters"),
                     (dict(max_iter=0, tol=nan), "max_iter"), (dict(tol=nan, init="random"), "tol"), (dict(tol=-1.0), "tol"), (dict(tol=inf), "tol"),
                     (dict(init="random", seed=0), "unknown init"), (dict(init=np.zeros((8, 7))), "shape"), (dict(init=np.zeros((7, 8))), "shape"),
                     (dict(init=np.full((8, 8), nan)), "finite"), (dict(seed=0), "seed"), (dict(seed=-2), "seed")):
        with pytest.raises(ValueError, match=word):
            m.kmeans(**kw)
    with pytest.raises(ValueError, match="limit of 4096"):
        StubModel(num_entities=5000).kmeans(num_clusters=4097, max_iter=0)


def test_kmeans_arguments_fill_the_struct():
    cfg = StubModel().cfg
    o, n, dim, keep = cm.kmeans_arguments(cfg)
    assert (n, dim) == (100, 8)
    assert (o.space, o.l2_normalize, o.ids, o.num_rows, o.init, o.init_centers) == (ca.SPACE_ENTITIES, 0, None, 100, ca.KMEANS_INIT_PLUSPLUS, None)
    assert (o.num_clusters, o.max_iter, o.tol, o.seed) == (8, 300, 1e-4, 1)
    o, n, dim, keep = cm.kmeans_arguments(cfg, "words", num_clusters=2, ids=[9, 3, 9], l2_normalize=True, max_iter=7, tol=0.0, seed=11)
    ids, given = keep
    assert (n, dim) == (3, 12) and (o.space, o.l2_normalize, o.num_rows, o.num_clusters, o.max_iter, o.tol, o.seed) == (ca.SPACE_WORDS, 1, 3, 2, 7, 0.0, 11)
    assert o.ids == ids.ctypes.data and list(ids) == [9, 3, 9] and ids.dtype == np.int64      # any order, duplicates kept
    assert given is None
    start = np.arange(24, dtype=np.float64).reshape(3, 8)
    o, n, dim, keep = cm.kmeans_arguments(cfg, num_clusters=3, limit=40, init=start, seed=-9)      # no seed is looked at with a given start
    assert n == 40 and o.ids is None and o.num_rows == 40 and o.init == ca.KMEANS_INIT_GIVEN
    assert o.init_centers == keep[1].ctypes.data and keep[1].dtype == np.float32 and np.array_equal(keep[1], start)


def test_the_benchmark_tool_fails_without_a_gpu():
    from tests.conftest import gpu_available
    if gpu_available():
        return                                # (with a GPU the tool runs: tools/bench_kmeans.py's own output is the check there)
    p = subprocess.run(["python", os.path.join(ROOT, "tools", "bench_kmeans.py"), "--shapes", "1000,36,8", "--iterations", "2"],
                       capture_output=True, text=True, cwd=ROOT)
    assert p.returncode != 0 and "GPU" in (p.stderr + p.stdout)
