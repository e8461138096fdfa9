"""-m gpu: cuNVSMQuery --qlm dirichlet --qlm_sdm (cunvsm_amd/host/query_main.cpp) end to end, on the 70-document collection and the
checkpoint of tests/test_query_lexical_cli_gpu.py: the lexical run file equals Model.sdm_rank on the same topics, the fused run file
equals Model.rank_ensemble(dependence=...), and <run_out> without fusion is the NVSM run it always was."""
import numpy as np
import pytest

import cunvsm_amd as ca
from tests.test_query_cli_gpu import assert_same_run, base_args, expected_rows, read_run, run_query
from tests.test_query_lexical_cli_gpu import corpus, kept_queries      # noqa: F401  (corpus: the module's fixture)

pytestmark = pytest.mark.gpu


def test_the_sdm_run_is_sdm_ranks_and_the_fusion_uses_it(corpus, tmp_path):      # noqa: F811
    assert hasattr(ca.lib(), "nvsm_sdm_rank")
    out, qlm = str(tmp_path / "run"), str(tmp_path / "qlm")
    flags, positional = base_args(corpus, out, "topics_a", "topics_b")
    r = run_query(flags + ["--qlm", "dirichlet", "--qlm_sdm", "--qlm_run_out", qlm] + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    differs = False
    for name in ("topics_a", "topics_b"):
        kept, queries = kept_queries(corpus, name)
        ids, scores, counts = corpus.model.sdm_rank(queries, method="dirichlet", top_k=corpus.D)
        assert (counts > 0).all()
        assert_same_run(read_run("%s-%s" % (qlm, name)), expected_rows(corpus, kept, ids, scores, counts))
        differs = differs or not np.array_equal(scores, corpus.model.lexical_rank(queries, method="dirichlet", top_k=corpus.D)[1])
        assert_same_run(read_run("%s-%s" % (out, name)), expected_rows(corpus, *corpus.expected(name)))
    assert differs and r.stdout == ""
    # other weights and window, and the fusion
    out2 = str(tmp_path / "fused")
    flags, positional = base_args(corpus, out2, "topics_b")
    r = run_query(flags + ["--qlm", "jm", "--qlm_sdm", "--sdm_weights", "0.7,0.2,0.1", "--sdm_window", "4", "--ensemble_alpha", "0.4", "--top_k", "20"]
                  + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    kept, queries = kept_queries(corpus, "topics_b")
    ids, scores, counts = corpus.model.rank_ensemble(queries, alpha=0.4, top_k=20, bias_coefficient=0.0, activation="tanh",
                                                     dependence=dict(weights=(0.7, 0.2, 0.1), window=4))
    assert_same_run(read_run("%s-topics_b" % out2), expected_rows(corpus, kept, ids, scores, counts))
