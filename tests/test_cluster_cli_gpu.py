"""-m gpu: cuNVSMCluster end to end — from a checkpoint in the trainer's formats to "<docno> <cluster>" lines — against Model.kmeans on
a handle loaded with the checkpoint's raw arrays: the same rows, the same seed, the same labels; and cuNVSMVisualize takes the file
as its classification unchanged."""
import os

import numpy as np
import pytest

import cunvsm_amd as ca
from tests.helpers import PARAMS, gpu_model
from tests.test_cluster_host import run_tool
from tests.test_visualize_host import Checkpoint
from tests.test_visualize_host import run_tool as run_visualize

pytestmark = pytest.mark.gpu


def test_the_tool_writes_what_model_kmeans_returns_and_the_picture_takes_it(tmp_path):
    ck = Checkpoint(tmp_path)
    out = str(tmp_path / "clusters.txt")
    K = 5
    p = run_tool(["--num_clusters", K, "--seed", 3, "--stopwords", ck.stop, "--clusters_out", out, ck.checkpoint, ck.collection])
    assert p.returncode == 0, p.stderr
    D, de = ck.E.shape
    V = np.fromfile(ck.base + ".W.f32", np.float32).size // 12
    spec = dict(num_words=V, num_entities=D, word_dim=12, entity_dim=de, window=1, num_random=1, nonlinearity="tanh", update_method="sgd")
    m = gpu_model(spec, 8)
    for name, ext in zip(PARAMS, ("W", "E", "T", "b")):
        m.set_param(name, np.fromfile("%s.%s.f32" % (ck.base, ext), np.float32))
    rows = sorted((mid, docno) for docno, mid in ck.model_doc.items())      # every document of the model, in model order
    labels, centers, counts, inertia, n_iter, dist = m.kmeans(ids=[r[0] for r in rows], num_clusters=K, seed=3, return_distances=True)
    lines = [line.split() for line in open(out)]
    assert [l[0] for l in lines] == [r[1] for r in rows] and len(lines) == 63
    assert [int(l[1]) for l in lines] == labels.tolist() and len({l[1] for l in lines}) == K
    said = p.stdout.strip().split("\n")
    for j in range(K):
        members = np.flatnonzero(labels == j)
        nearest = rows[int(members[np.argmin(dist[members])])][1]
        assert said[j] == "cluster %d: %d documents, nearest %s" % (j, counts[j], nearest)
    assert said[K] == "inertia %.17g after %d iterations" % (inertia, n_iter) and len(said) == K + 1
    # the classified documents only, normalised, with the agreement figures
    out2 = str(tmp_path / "classified.txt")
    p = run_tool(["--num_clusters", 3, "--l2_normalize", "--limit", 30, "--object_classification", ck.class_path, "--stopwords", ck.stop,
                  "--clusters_out", out2, ck.checkpoint, ck.collection])
    assert p.returncode == 0, p.stderr
    chosen = ck.rows(30)
    got = m.kmeans(ids=[r[0] for r in chosen], num_clusters=3, l2_normalize=True)
    m.close()
    lines = [line.split() for line in open(out2)]
    assert [l[0] for l in lines] == [r[1] for r in chosen] and [int(l[1]) for l in lines] == got[0].tolist()
    figures = p.stdout.strip().split("\n")[-1].split()
    assert figures[0::2] == ["purity", "nmi", "ari"]
    want = ca.cluster_agreement(got[0], [r[2] for r in chosen])
    assert np.abs(np.array([float(v) for v in figures[1::2]]) - np.array(want)).max() <= 1e-12
    # cuNVSMVisualize accepts the clusters file as a classification, unchanged
    (tmp_path / "plots").mkdir()
    plot = str(tmp_path / "plots" / "picture.pdf")
    p = run_visualize(["--object_classification", out, "--filter_unclassified", "--stopwords", ck.stop, "--perplexity", 5, "--max_iter", 20,
                       "--plot_out", plot, ck.checkpoint, ck.collection])
    assert p.returncode == 0, p.stderr
    tsv = [line.rstrip("\n").split("\t") for line in open(str(tmp_path / "plots" / "picture-clusters.txt.tsv"))]
    assert [(t[0], int(t[1])) for t in tsv] == [(r[1], int(l)) for r, l in zip(rows, labels)]
    assert os.path.getsize(out) > 0
