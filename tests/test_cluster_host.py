"""cuNVSMCluster (cunvsm_amd/host/cluster_main.cpp, cluster_lib.hpp) without a device: the agreement functions of cluster_lib.hpp
against cunvsm_amd.cluster_agreement (itself held to sklearn.metrics in tests/test_kmeans_reference.py), the output writer, the
nearest-member choice, and the tool's argument handling. The clustering itself needs the GPU: tests/test_cluster_cli_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from tests.conftest import ROOT
from tests.test_query_host import HOST_DIR
from tests.test_visualize_host import Checkpoint

TOOL = os.path.join(ROOT, "cunvsm_amd", "bin", "cuNVSMCluster")


def run_tool(args, timeout=300):
    if not os.path.exists(TOOL):
        pytest.fail("%s is missing: __graft_entry__.build() builds it" % TOOL)
    return subprocess.run([TOOL] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def agreement_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_lib")
    src = d / "lib.cpp"
    src.write_text('#include <cstdio>\n#include <iostream>\n#include "cluster_lib.hpp"\nusing namespace nvsm_host;\n'
                   '// stdin: n, then n pairs "<label> <class>"; stdout: purity nmi ari (%.17g), the clusters file, the nearest members\n'
                   'int main() { size_t n; std::cin >> n; std::vector<int32_t> l(n); std::vector<std::string> c(n); std::vector<VisualRow> rows;\n'
                   '  std::vector<float> dist;\n'
                   '  for (size_t i = 0; i < n; ++i) { std::cin >> l[i] >> c[i]; rows.push_back(VisualRow{int64_t(i), "D-" + std::to_string(i), c[i]});\n'
                   '    dist.push_back(float((i * 7) % 5)); }\n'
                   '  const Contingency t = contingency(l, c);\n'
                   '  std::printf("%.17g %.17g %.17g\\n", cluster_purity(t), cluster_nmi(t), cluster_ari(t));\n'
                   '  write_clusters(std::cout, rows, l);\n'
                   '  int32_t k = 0; for (int32_t v : l) k = std::max(k, v + 1);\n'
                   '  for (int64_t b : nearest_members(l, dist, k)) std::cout << b << " ";\n  std::cout << "\\n"; return 0; }\n')
    exe = d / "lib"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", HOST_DIR, str(src), os.path.join(HOST_DIR, "base.cpp"), "-o", str(exe)])
    return str(exe)


@pytest.mark.parametrize("n,k,c,seed", [(500, 7, 5, 0), (50, 3, 3, 1), (40, 1, 4, 2), (40, 4, 1, 3), (30, 30, 2, 4), (12, 1, 1, 5)])
def test_the_agreement_functions_equal_the_python_ones(agreement_exe, n, k, c, seed):
    rs = np.random.RandomState(seed)
    labels = rs.randint(0, k, n)
    classes = ["cls%d" % v for v in rs.randint(0, c, n)]
    text = "%d\n" % n + "".join("%d %s\n" % (l, s) for l, s in zip(labels, classes))
    lines = subprocess.run([agreement_exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [float(v) for v in lines[0].split()]
    want = ca.cluster_agreement(labels, classes)
    assert np.abs(np.array(got) - np.array(want)).max() <= 1e-12, (got, want)
    assert lines[1:n + 1] == ["D-%d %d" % (i, l) for i, l in enumerate(labels)]      # the format cuNVSMVisualize's reader takes
    dist = np.array([(i * 7) % 5 for i in range(n)], dtype=np.float32)
    nearest = []
    for j in range(labels.max() + 1):
        members = np.flatnonzero(labels == j)
        nearest.append(-1 if members.size == 0 else int(members[np.argmin(dist[members])]))      # argmin: the first of equals
    assert [int(v) for v in lines[n + 1].split()] == nearest


def test_refusals_need_no_device(tmp_path):
    ck = Checkpoint(tmp_path)
    out = str(tmp_path / "clusters.txt")
    base = ["--stopwords", ck.stop, "--clusters_out", out]
    tail = [ck.checkpoint, ck.collection]
    cases = [(base + tail, "required"), (["--num_clusters", 3] + tail, "required"), (base + ["--num_clusters", 3, ck.checkpoint], "required"),
             (base + ["--num_clusters", -2] + tail, "--num_clusters"), (base + ["--num_clusters", 5000] + tail, "--num_clusters"),
             (base + ["--num_clusters", 3, "--limit", -1] + tail, "--limit"), (base + ["--num_clusters", 3, "--max_iter", 0] + tail, "--max_iter"),
             (base + ["--num_clusters", 3, "--tol", -1.0] + tail, "--tol"), (base + ["--num_clusters", 3, "--seed", 0] + tail, "--seed"),
             (base + ["--num_clusters", 3, "--object_classification", str(tmp_path / "none")] + tail, "cannot read the classification file"),
             (base + ["--num_clusters", 3, ck.base + "_9.hdf5", ck.collection], "cannot read the model"),
             (base + ["--num_clusters", 3, ck.checkpoint, str(tmp_path / "nowhere")], "cannot read collection"),
             (base + ["--num_clusters", 64] + tail, "fewer documents (63) than clusters (64)"),
             (base + ["--num_clusters", 21, "--object_classification", ck.other_path] + tail, "fewer documents (20) than clusters (21)")]
    for args, word in cases:
        p = run_tool(args)
        assert p.returncode != 0 and word in p.stderr, (args, p.stderr[-400:])
    assert not os.path.exists(out)
    p = run_tool(["--help"])
    assert p.returncode == 0 and "--num_clusters" in p.stdout and "--clusters_out" in p.stdout
