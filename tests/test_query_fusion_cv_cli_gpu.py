"""-m gpu: cuNVSMQuery --ensemble_qrel (cunvsm_amd/host/query_main.cpp) end to end. On the 70-document collection and the checkpoint of
tests/test_query_cli_gpu.py the fused run file and the printed means equal Model.rank_ensemble_cv's under the same permutation of the
topics. On Cranfield, with the two-epoch LSE model of tests/test_query_lexical_cli_gpu.py: twenty folds, every topic's lines are those
of the tool's own --ensemble_alpha run at its fold's alpha under the restated permutation (tests/fusion_cv_reference.py
shuffled_folds, held against the tool's own ensemble_folds by tests/test_fusion_folds_host.py), under the issue's settings and under a
training measure for which the folds choose different alphas; --ensemble_seed changes the run exactly on the topics whose fold's alpha
changes. The MAP is printed for DESIGN.md §17 and not asserted."""
import os
import re

import numpy as np
import pytest

from tests import fusion_cv_reference as fr
from tests.test_query_cli_gpu import CUTOFFS, assert_same_run, base_args, expected_rows, printed_metrics, read_run, run_query
from tests.test_query_lexical_cli_gpu import GOLDEN, corpus, kept_queries      # noqa: F401 (corpus: the fixture)
from tests.test_trainer_gpu import CRANFIELD, run_trainer

pytestmark = pytest.mark.gpu

FOLD_LINE = re.compile(r"Fold (\d+): best_alpha=(\d\.\d\d) train (\S+)=(\d\.\d{4})")


@pytest.mark.parametrize("seed,measure,num_folds,prf", [(1, "map", 5, False), (0, "ndcg", 2, False), (7, "map_cut_3", 3, True)])
def test_the_fused_run_and_the_printed_means_are_rank_ensemble_cvs(corpus, tmp_path, seed, measure, num_folds, prf):      # noqa: F811
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_a")
    extra = ["--qlm", "jm", "--ensemble_qrel", corpus.qrel_path, "--num_folds", str(num_folds), "--alpha_stepsize", "0.25",
             "--ensemble_measure", measure, "--ensemble_seed", str(seed), "--top_k", "10"] + (["--qlm_prf"] if prf else [])
    r = run_query(flags + extra + positional)
    assert r.returncode == 0, r.stderr[-3000:]
    kept, queries = kept_queries(corpus, "topics_a")
    judged = [corpus.judged_ids(t) for t, _ in kept]
    fold_of = fr.shuffled_folds(len(kept), num_folds, seed)
    depth = 3 if measure == "map_cut_3" else 0
    fold_alpha, fold_train, metrics, ids, scores, counts = corpus.model.rank_ensemble_cv(
        queries, judged, stepsize=0.25, num_folds=num_folds, measure="map" if depth else measure, depth=depth, fold_of=fold_of, top_k=10,
        cutoffs=CUTOFFS, feedback=True if prf else None, bias_coefficient=0.0, activation="tanh")
    assert_same_run(read_run(out + "-topics_a"), expected_rows(corpus, kept, ids, scores, counts))
    lines = FOLD_LINE.findall(r.stderr)
    assert [int(f) for f, _, _, _ in lines] == list(range(num_folds))
    for f, alpha, name, value in lines:
        assert name == measure and alpha == "%.2f" % fold_alpha[int(f)] and value == "%.4f" % fold_train[int(f)]
    block = printed_metrics(r.stdout)[0]
    evaluated = (metrics["num_rel"] > 0) & (counts > 0)
    assert block["num_q"] == str(int(evaluated.sum()))
    assert abs(float(block["map"]) - metrics["map"][evaluated].mean()) <= 0.5e-4 + 1e-9
    assert block["num_ret"] == str(int(metrics["num_ret"][evaluated].sum()))


def test_refusals_and_the_help_text(corpus, tmp_path):      # noqa: F811
    out = str(tmp_path / "run")
    flags, positional = base_args(corpus, out, "topics_a")
    cv = ["--qlm", "jm", "--ensemble_qrel", corpus.qrel_path]
    for extra, word in ((cv + ["--ensemble_alpha", "0.5"], "mutually exclusive"), (["--ensemble_qrel", corpus.qrel_path], "need --qlm"),
                        (["--qlm", "jm", "--qlm_run_out", out, "--num_folds", "3"], "need --ensemble_qrel"),
                        (cv + ["--num_folds", "1"], "--num_folds"), (cv + ["--num_folds", "6"], "num_folds"),
                        (cv + ["--alpha_stepsize", "0.0005"], "--alpha_stepsize"), (cv + ["--alpha_stepsize", "0"], "--alpha_stepsize"),
                        (cv + ["--ensemble_measure", "num_ret"], "--ensemble_measure"), (cv + ["--ensemble_measure", "map_cut_"], "--ensemble_measure"),
                        (cv + ["--ensemble_seed", "2147483647"], "--ensemble_seed"), (cv + ["--qrels", corpus.qrel_path], "--qrels")):
        r = run_query(flags + extra + positional)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr[-500:])
        assert not os.path.exists(out + "-topics_a")
    r = run_query(["--help"])
    assert r.returncode == 0 and "minstd_rand0" in r.stdout and "j = rng() % (i + 1)" in r.stdout
    for flag in ("ensemble_qrel", "num_folds", "alpha_stepsize", "ensemble_measure", "ensemble_seed"):
        assert "-%s (" % flag in r.stdout


def by_topic(rows):
    out = {}
    for topic, docno, rank, score in rows:
        out.setdefault(topic, []).append((docno, rank, np.float32(score).view(np.uint32)))
    return out


# (measure, whether the folds must disagree). Under the issue's own settings — map_cut_1000 on the 0.05 grid — every fold of the two-epoch
# model chooses 0.50, so that case alone would hold for any fold membership; under P_5 the folds choose 0.45 or 0.55, differently for
# the two seeds, and the run file then depends on the permutation, the fold of every topic and the choice.
CRANFIELD_CASES = (("map_cut_1000", False), ("P_5", True))


def test_cranfield_twenty_folds(tmp_path):
    out = str(tmp_path / "lse")
    r = run_trainer(["--word_repr_size", "64", "--entity_repr_size", "64", "--window_size", "10", "--num_random_entities", "4", "--seed", "1",
                     "--update_method", "full_adam", "--nonlinearity", "tanh", "--batch_size", "1024", "--num_epochs", "2", "--output", out, CRANFIELD])
    assert r.returncode == 0, r.stderr[-3000:]
    topics, qrels = os.path.join(GOLDEN, "cranfield.topics"), os.path.join(GOLDEN, "cranfield.qrel")
    common = ["--index", CRANFIELD, "--topics", topics, "--qlm", "jm"]
    cv = ["--ensemble_qrel", qrels, "--num_folds", "20", "--alpha_stepsize", "0.05"]
    fixed = {}                              # alpha -> the tool's own --ensemble_alpha run, by topic

    def fixed_run(alpha):
        if alpha not in fixed:
            run = str(tmp_path / ("fixed_" + alpha))
            q = run_query(common + ["--ensemble_alpha", alpha, out + "_2.hdf5", run])
            assert q.returncode == 0, q.stderr[-3000:]
            fixed[alpha] = by_topic(read_run(run + "-cranfield.topics"))
        return fixed[alpha]

    for measure, folds_disagree in CRANFIELD_CASES:
        runs, alphas = {}, {}
        for seed in (1, 0):
            run = str(tmp_path / ("cv_%s_%d" % (measure, seed)))
            q = run_query(common + cv + ["--ensemble_measure", measure, "--ensemble_seed", str(seed), out + "_2.hdf5", run])
            assert q.returncode == 0, q.stderr[-3000:]
            lines = FOLD_LINE.findall(q.stderr)
            assert [int(f) for f, _, _, _ in lines] == list(range(20)) and all(name == measure for _, _, name, _ in lines)
            runs[seed], alphas[seed] = by_topic(read_run(run + "-cranfield.topics")), [a for _, a, _, _ in lines]
            block = printed_metrics(q.stdout)[0]
            assert int(block["num_q"]) > 200
            print("cranfield-map (LSE, 2 epochs, d = 64): NVSM + QLM, 20 folds, step 0.05, train %s, seed %d: %s; fold alphas %s"
                  % (measure, seed, block["map"], sorted(set(alphas[seed]))))
        ranked = list(runs[1])                                             # (dicts keep the run file's order: the ranked topics')
        assert ranked == list(runs[0]) == list(fixed_run(alphas[1][0])) and len(ranked) > 200
        # every topic's lines are the --ensemble_alpha run's at its fold's alpha, under the permutation of --help
        alpha_of = {}
        for seed in (1, 0):
            fold_of = fr.shuffled_folds(len(ranked), 20, seed)
            alpha_of[seed] = [alphas[seed][fold_of[i]] for i in range(len(ranked))]
            for i, topic in enumerate(ranked):
                assert runs[seed][topic] == fixed_run(alpha_of[seed][i])[topic], (measure, seed, topic)
        # ... so --ensemble_seed changes the run only through the fold membership: exactly the topics whose fold's alpha differs
        moved = [t for i, t in enumerate(ranked) if alpha_of[1][i] != alpha_of[0][i]]
        assert [t for t in ranked if runs[1][t] != runs[0][t]] == moved
        if folds_disagree:
            assert len(set(alphas[1])) >= 2 and len(set(alphas[0])) >= 2 and 0 < len(moved) < len(ranked)
            # a fold membership other than the tool's would not pass the check above: the identity permutation under seed 1 does not
            wrong = fr.shuffled_folds(len(ranked), 20, 0)
            assert any(runs[1][t] != fixed_run(alphas[1][wrong[i]])[t] for i, t in enumerate(ranked))
    assert not np.array_equal(fr.shuffled_folds(len(ranked), 20, 1), fr.shuffled_folds(len(ranked), 20, 0))
    # the two flags together
    q = run_query(common + cv + ["--ensemble_alpha", "0.5", out + "_2.hdf5", str(tmp_path / "both")])
    assert q.returncode == 1 and "mutually exclusive" in q.stderr and not os.path.exists(str(tmp_path / "both") + "-cranfield.topics")
