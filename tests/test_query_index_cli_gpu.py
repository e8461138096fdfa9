"""-m gpu: cuNVSMQuery --lexical_index (cunvsm_amd/host/query_main.cpp) on the Cranfield fixture: with --qlm and with --rerank, every
run file written with `--lexical_index always` holds the bytes of the one written without the flag; the flag alone is refused."""
import os

import pytest

from tests.test_query_cli_gpu import run_query
from tests.test_trainer_gpu import CRANFIELD, run_trainer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.dirname(CRANFIELD)


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("query_index_cli") / "lse")
    r = run_trainer(["--word_repr_size", "16", "--entity_repr_size", "16", "--window_size", "10", "--num_random_entities", "2", "--seed", "1",
                     "--update_method", "full_adam", "--nonlinearity", "tanh", "--batch_size", "1024", "--num_epochs", "1", "--output", out, CRANFIELD])
    assert r.returncode == 0, r.stderr[-3000:]
    return out + "_1.hdf5"


def run_files(tmp_path, checkpoint, label, extra, outputs):
    """the bytes of the run files of one cuNVSMQuery call: `outputs` names the flags that take a prefix"""
    common = ["--index", CRANFIELD, "--topics", os.path.join(GOLDEN, "cranfield.topics")]
    prefixes = {flag: str(tmp_path / ("%s_%s" % (flag, label))) for flag in outputs}
    flags = [x for flag, p in prefixes.items() for x in ("--" + flag, p)]
    run = str(tmp_path / ("run_" + label))
    r = run_query(common + extra + flags + [checkpoint, run])
    assert r.returncode == 0, r.stderr[-3000:]
    files = {}
    for name, prefix in list(prefixes.items()) + [("run", run)]:
        with open(prefix + "-cranfield.topics", "rb") as f:
            files[name] = f.read()
        assert len(files[name]) > 10000, name
    return files, r.stderr


@pytest.mark.parametrize("extra,outputs", [(["--qlm", "jm"], ["qlm_run_out"]), (["--rerank", "tfidf", "--rerank_depth", "100"], ["tfidf_run_out"])])
def test_the_run_files_are_those_written_without_the_flag(tmp_path, checkpoint, extra, outputs):
    plain, _ = run_files(tmp_path, checkpoint, "plain", extra, outputs)
    indexed, log = run_files(tmp_path, checkpoint, "indexed", extra + ["--lexical_index", "always"], outputs)
    assert "inverted index of" in log
    assert plain.keys() == indexed.keys()
    for name in plain:
        assert plain[name] == indexed[name], name


def test_the_flag_needs_a_lexical_ranking_and_a_known_value(tmp_path, checkpoint):
    common = ["--index", CRANFIELD, "--topics", os.path.join(GOLDEN, "cranfield.topics")]
    run = str(tmp_path / "run")
    for extra, word in ((["--lexical_index", "always"], "--lexical_index needs --qlm or --rerank"),
                        (["--lexical_index", "auto", "--tfidf_run_out", run + "_t"], "--lexical_index needs --qlm or --rerank"),
                        (["--qlm", "jm", "--qlm_run_out", run + "_q", "--lexical_index", "sometimes"], "none of auto, always, never")):
        r = run_query(common + extra + [checkpoint, run])
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr[-500:])
        assert not os.path.exists(run + "-cranfield.topics")
    assert "-lexical_index (" in run_query(["--help"]).stdout
