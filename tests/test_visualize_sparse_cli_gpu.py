"""cuNVSMVisualize --tsne_method sparse end to end against Model.tsne(method="sparse") on a handle loaded with the checkpoint's raw
arrays: the same rows in the same order give the same bits; without the flag the tool writes what it writes today (Model.tsne's exact
picture). The refusals of the two new flags need no device."""
import numpy as np
import pytest

from tests.helpers import PARAMS, gpu_model
from tests.test_visualize_host import Checkpoint, run_tool


def picture(path):
    lines = [line.rstrip("\n").split("\t") for line in open(path)]
    return [l[:2] for l in lines], np.array([[float(l[2]), float(l[3])] for l in lines], dtype=np.float32)


@pytest.mark.gpu
def test_the_sparse_method_writes_what_model_tsne_returns_and_the_default_stays_exact(tmp_path):
    ck = Checkpoint(tmp_path)
    (tmp_path / "sparse").mkdir()
    (tmp_path / "exact").mkdir()
    common = ("--filter_unclassified", "--l2_normalize", "--perplexity", 5, "--max_iter", 60)
    p = run_tool(ck.args(*common, "--tsne_method", "sparse", plot_out=str(tmp_path / "sparse" / "reuters.pdf")))
    assert p.returncode == 0, p.stderr
    p = run_tool(ck.args(*common, "--tsne_method", "sparse", "--tsne_neighbors", 7, plot_out=str(tmp_path / "sparse" / "seven.pdf")))
    assert p.returncode == 0, p.stderr
    p = run_tool(ck.args(*common, plot_out=str(tmp_path / "exact" / "reuters.pdf")))
    assert p.returncode == 0, p.stderr
    D, de = ck.E.shape
    V = np.fromfile(ck.base + ".W.f32", np.float32).size // 12
    spec = dict(num_words=V, num_entities=D, word_dim=12, entity_dim=de, window=1, num_random=1, nonlinearity="tanh", update_method="sgd")
    m = gpu_model(spec, 8)
    for name, ext in zip(PARAMS, ("W", "E", "T", "b")):
        m.set_param(name, np.fromfile("%s.%s.f32" % (ck.base, ext), np.float32))
    rows = ck.rows()
    kw = dict(ids=[r[0] for r in rows], l2_normalize=True, perplexity=5.0, max_iter=60)
    want = {"sparse/reuters": m.tsne(method="sparse", **kw), "sparse/seven": m.tsne(method="sparse", n_neighbors=7, **kw), "exact/reuters": m.tsne(**kw)}
    m.close()
    for name, (Y, kl, n_iter) in want.items():
        head, got = picture(str(tmp_path / ("%s-classes.txt.tsv" % name)))
        assert head == [[r[1], r[2]] for r in rows]
        assert np.array_equal(got.view(np.uint32), Y.view(np.uint32)) and n_iter == 59 and np.isfinite(kl), name
    assert not np.array_equal(want["sparse/seven"][0], want["sparse/reuters"][0]), "seven neighbours a row are another matrix than sixteen"


def test_the_flags_refusals_need_no_device(tmp_path):
    ck = Checkpoint(tmp_path)
    out = str(tmp_path / "x.pdf")
    p = run_tool(ck.args("--filter_unclassified", "--tsne_method", "spectral", plot_out=out))
    assert p.returncode != 0 and "neither exact nor sparse" in p.stderr
    p = run_tool(ck.args("--filter_unclassified", "--tsne_neighbors", 5, plot_out=out))
    assert p.returncode != 0 and "belongs to --tsne_method sparse" in p.stderr
    p = run_tool(ck.args("--filter_unclassified", "--tsne_method", "sparse", "--tsne_neighbors", 5000, plot_out=out))
    assert p.returncode != 0 and "--tsne_neighbors must be in" in p.stderr
