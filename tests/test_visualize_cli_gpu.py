"""-m gpu: cuNVSMVisualize --mode tsne end to end — from a checkpoint in the trainer's formats and classification files to
"<root>-<classification file>.tsv" — against Model.tsne on a handle loaded with the checkpoint's raw arrays: the same rows in the
same order give the same bits, and the file's %.9g round-trips a float32."""
import numpy as np
import pytest

from tests.helpers import PARAMS, gpu_model
from tests.test_visualize_host import Checkpoint, run_tool

pytestmark = pytest.mark.gpu


def test_tsne_mode_writes_what_model_tsne_returns(tmp_path):
    ck = Checkpoint(tmp_path)
    out = str(tmp_path / "plots" / "reuters.pdf")
    (tmp_path / "plots").mkdir()
    p = run_tool(ck.args("--filter_unclassified", "--l2_normalize", "--perplexity", 5, "--max_iter", 60, ck.other_path, plot_out=out))
    assert p.returncode == 0, p.stderr
    D, de = ck.E.shape
    V = np.fromfile(ck.base + ".W.f32", np.float32).size // 12
    spec = dict(num_words=V, num_entities=D, word_dim=12, entity_dim=de, window=1, num_random=1, nonlinearity="tanh", update_method="sgd")
    m = gpu_model(spec, 8)
    for name, ext in zip(PARAMS, ("W", "E", "T", "b")):
        m.set_param(name, np.fromfile("%s.%s.f32" % (ck.base, ext), np.float32))
    other = sorted((ck.model_doc[line.split()[0]], line.split()[0], "x") for line in open(ck.other_path))
    for name, rows in (("classes.txt", ck.rows()), ("other.cls", other)):
        Y, kl, n_iter = m.tsne(ids=[r[0] for r in rows], l2_normalize=True, perplexity=5.0, max_iter=60)
        lines = [line.rstrip("\n").split("\t") for line in open(str(tmp_path / "plots" / ("reuters-%s.tsv" % name)))]
        assert [l[:2] for l in lines] == [[r[1], r[2]] for r in rows]
        got = np.array([[float(l[2]), float(l[3])] for l in lines], dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), Y.view(np.uint32)) and n_iter == 59 and np.isfinite(kl)
    m.close()
    # fewer than two documents of the model: refused before the device is touched
    one = str(tmp_path / "one.cls")
    with open(one, "w") as f:
        f.write("%s a\nNOBODY b\n" % other[0][1])
    p = run_tool(ck.args("--filter_unclassified", classes=one, plot_out=out))
    assert p.returncode != 0 and "fewer than two documents" in p.stderr
