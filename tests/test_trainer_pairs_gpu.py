"""GPU tests of cuNVSMTrainModel with document similarities: the mixed objective (text-entity + entity-entity, cpp/main.cu:733-741)
on the Cranfield collection with a similarity file written for the test, some of whose lines name unknown docnos."""
import re

import numpy as np
import pytest

from tests.test_trainer_gpu import CRANFIELD, epoch_costs, run_trainer

pytestmark = pytest.mark.gpu

ARGS = ["--word_repr_size", "64", "--entity_repr_size", "32", "--window_size", "10", "--num_random_entities", "4", "--seed", "1",
        "--batch_size", "2048", "--nonlinearity", "tanh", "--weighting", "uniform", "--regularization_lambda", "1e-2"]


def similarity_file(tmp_path, num_pairs=4096, unknown=("no-such-doc", "9999999")):
    """Neighbouring Cranfield documents (docnos 1 .. 1400) as substitutes of each other, plus a few lines that name documents the
    collection does not hold (on either side)."""
    rs = np.random.RandomState(0)
    lines = []
    for _ in range(num_pairs):
        a = int(rs.randint(1, 1400))
        lines.append("%d %d %.2f" % (a, a + 1, rs.choice([0.5, 1.0])))
    lines.insert(10, "%s 5 1.0" % unknown[0])
    lines.insert(200, "7 %s 1.0" % unknown[1])
    path = tmp_path / "similarities.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_mixed_objective_on_cranfield(tmp_path):
    sims = similarity_file(tmp_path)
    args = ARGS + ["--update_method", "dense_adam", "--learning_rate", "1e-3", "--entity_similarity_weight", "0.3", "--num_epochs", "3",
                   "--allow_ragged_batches"]       # (a few Cranfield documents are not in the model: a pass over the pairs ends short)
    a = run_trainer(args + ["--output", str(tmp_path / "mixed"), CRANFIELD, sims])
    assert a.returncode == 0, a.stderr[-3000:]
    for name in ("no-such-doc", "9999999"):
        assert "Entity '%s' not found; skipping pair." % name in a.stderr
    assert "Entity-entity objective:" in a.stderr and "text_entity_weight: 0.7" in a.stderr
    costs = epoch_costs(a.stderr)
    assert len(costs) == 3 and costs[2] < costs[1] < costs[0]
    assert (tmp_path / "mixed_3.hdf5").exists()
    b = run_trainer(args + ["--output", str(tmp_path / "again"), CRANFIELD, sims])
    assert b.returncode == 0, b.stderr[-3000:]
    assert epoch_costs(b.stderr) == costs                       # bit-identical runs: the same float costs, epoch by epoch


def test_short_pair_batches_are_skipped_unless_ragged_batches_are_allowed(tmp_path):
    """The step's instance count is the smaller of the two batches': some 300 pairs against 2048 windows is never a multiple of 1024."""
    sims = similarity_file(tmp_path, num_pairs=300)
    base = ARGS + ["--update_method", "sgd", "--entity_similarity_weight", "0.5", "--num_epochs", "1"]
    r = run_trainer(base + [CRANFIELD, sims])
    assert r.returncode == 0, r.stderr[-3000:]
    known = int(re.search(r"pair_source\.cpp:\d+\] Shuffling (\d+) instance pointers", r.stderr).group(1))
    assert 290 <= known <= 300                                  # (pairs naming a document the model does not hold are skipped)
    assert "Skipping Batch #0" in r.stderr and "(%d instances)" % known in r.stderr
    r = run_trainer(base + ["--allow_ragged_batches", "--num_epochs", "2", CRANFIELD, sims])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "Skipping Batch" not in r.stderr
    costs = epoch_costs(r.stderr)
    assert len(costs) == 2 and costs[1] < costs[0]
    assert "Shuffling %d instance pointers." % known in r.stderr


def test_refused_pair_configurations(tmp_path):
    sims = similarity_file(tmp_path, num_pairs=50)
    base = ARGS + ["--num_epochs", "1"]
    r = run_trainer(base + ["--update_method", "adagrad", "--entity_similarity_weight", "0.3", CRANFIELD, sims])
    assert r.returncode == 1 and "Adagrad currently does not implement multiple gradients." in r.stderr
    r = run_trainer(base + ["--update_method", "sparse_adam", "--entity_similarity_weight", "0.3", CRANFIELD, sims])
    assert r.returncode == 1 and "Sparse Adam currently does not implement multiple gradients." in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--entity_similarity_weight", "1", CRANFIELD, sims])
    assert r.returncode == 1 and "text_entity_weight" in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--entity_similarity_weight", "0.3", CRANFIELD])
    assert r.returncode == 1 and "only the text-entity objective" in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--term_similarity_weight", "0.3", CRANFIELD, sims])
    assert r.returncode == 1 and "--term_similarity_weight must be 0" in r.stderr
