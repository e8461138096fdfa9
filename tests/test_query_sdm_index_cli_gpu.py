"""-m gpu: cuNVSMQuery --lexical_positions (cunvsm_amd/host/query_main.cpp) on the Cranfield fixture: the run files of
`--qlm dirichlet --qlm_sdm --lexical_index always --lexical_positions` hold the bytes of those written without the last two flags."""
import pytest

from tests.test_query_index_cli_gpu import checkpoint, run_files      # noqa: F401  (checkpoint: the module's fixture)

pytestmark = pytest.mark.gpu


def test_the_sdm_run_files_are_those_written_without_the_flags(tmp_path, checkpoint):      # noqa: F811
    extra, outputs = ["--qlm", "dirichlet", "--qlm_sdm"], ["qlm_run_out"]
    plain, _ = run_files(tmp_path, checkpoint, "plain", extra, outputs)
    layered, log = run_files(tmp_path, checkpoint, "layered", extra + ["--lexical_index", "always", "--lexical_positions"], outputs)
    assert "inverted index of" in log and "positional layer of" in log
    assert plain.keys() == layered.keys()
    for name in plain:
        assert plain[name] == layered[name], name
