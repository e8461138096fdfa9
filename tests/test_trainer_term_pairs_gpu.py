"""GPU tests of cuNVSMTrainModel with term similarities: the mixed objective (text-entity + term-term, TextEntityTermTerm,
cpp/main.cu:742-750) on the Cranfield collection with a term file written for the test from the collection's own frequent terms,
two of whose lines name terms the vocabulary does not hold. The pairs are named by --term_similarities (the reference reuses the
second positional argument, which names document similarities here: cunvsm_amd/host/train_main.cpp)."""
import collections
import re

import numpy as np
import pytest

from tests.test_trainer_gpu import CRANFIELD, epoch_costs, run_trainer
from tests.test_trainer_pairs_gpu import similarity_file

pytestmark = pytest.mark.gpu

ARGS = ["--word_repr_size", "64", "--entity_repr_size", "32", "--window_size", "10", "--num_random_entities", "4", "--seed", "1",
        "--batch_size", "2048", "--nonlinearity", "tanh", "--weighting", "uniform", "--regularization_lambda", "1e-2"]
UNKNOWN = ("zzznosuchterm", "qqqneitherthis")


def frequent_terms(count=300, skip=40):
    """Alphabetic tokens of the collection's text by frequency, without the `skip` most frequent (most of which the vocabulary's
    document-frequency ceiling removes). Whatever the indexer does not hold of them is skipped with a warning, like any unknown term."""
    text = re.sub(r"<[^>]+>", " ", open(CRANFIELD, errors="replace").read().lower())
    freq = collections.Counter(t for t in re.findall(r"[a-z]+", text) if len(t) >= 4)
    return [t for t, _ in freq.most_common(skip + count)][skip:]


def term_file(tmp_path, num_pairs=4096, unknown=UNKNOWN):
    rs = np.random.RandomState(0)
    terms = frequent_terms()
    lines = []
    for _ in range(num_pairs):
        i = int(rs.randint(0, len(terms) - 1))
        lines.append("%s %s %.2f" % (terms[i], terms[i + 1], rs.choice([0.5, 1.0])))
    lines.insert(10, "%s %s 1.0" % (unknown[0], terms[5]))
    lines.insert(200, "%s %s 1.0" % (terms[7], unknown[1]))
    path = tmp_path / "term_similarities.txt"
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def test_term_mixed_objective_on_cranfield(tmp_path):
    terms = term_file(tmp_path)
    args = ARGS + ["--update_method", "dense_adam", "--learning_rate", "1e-3", "--term_similarity_weight", "0.3", "--term_similarities", terms,
                   "--num_epochs", "3", "--allow_ragged_batches"]       # (a pass over the pairs ends short)
    a = run_trainer(args + ["--output", str(tmp_path / "mixed"), CRANFIELD])
    assert a.returncode == 0, a.stderr[-3000:]
    for name in UNKNOWN:
        assert "Entity '%s' not found; skipping pair." % name in a.stderr
    m = re.search(r"Term-term objective: (\d+) pairs", a.stderr)
    assert m and int(m.group(1)) > 2048                          # most of the 4 096 lines name two terms of the model
    assert "text_entity_weight: 0.7" in a.stderr and "term_term_weight: 0.3" in a.stderr and "entity_entity_weight: 0 " in a.stderr
    costs = epoch_costs(a.stderr)
    assert len(costs) == 3 and costs[2] < costs[1] < costs[0]
    assert (tmp_path / "mixed_3.hdf5").exists()
    b = run_trainer(args + ["--output", str(tmp_path / "again"), CRANFIELD])
    assert b.returncode == 0, b.stderr[-3000:]
    assert epoch_costs(b.stderr) == costs                       # bit-identical runs: the same float costs, epoch by epoch


def test_refused_term_pair_configurations(tmp_path):
    terms = term_file(tmp_path, num_pairs=50)
    sims = similarity_file(tmp_path, num_pairs=50)
    base = ARGS + ["--num_epochs", "1"]
    with_terms = ["--term_similarity_weight", "0.3", "--term_similarities", terms]
    # without the flag the weight stays refused, whatever the second positional argument holds, and the message names the flag
    r = run_trainer(base + ["--update_method", "sgd", "--term_similarity_weight", "0.3", CRANFIELD, sims])
    assert r.returncode == 1 and "--term_similarity_weight must be 0" in r.stderr and "--term_similarities" in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--term_similarity_weight", "0.3", CRANFIELD])
    assert r.returncode == 1 and "--term_similarity_weight must be 0" in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--entity_similarity_weight", "0.3"] + with_terms + [CRANFIELD, sims])
    assert r.returncode == 1 and "cannot both be non-zero" in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--term_similarity_weight", "1", "--term_similarities", terms, CRANFIELD])
    assert r.returncode == 1 and "text_entity_weight" in r.stderr
    r = run_trainer(base + ["--update_method", "adagrad"] + with_terms + [CRANFIELD])
    assert r.returncode == 1 and "Adagrad currently does not implement multiple gradients." in r.stderr
    r = run_trainer(base + ["--update_method", "sparse_adam"] + with_terms + [CRANFIELD])
    assert r.returncode == 1 and "Sparse Adam currently does not implement multiple gradients." in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--world_size", "2", "--rank", "0"] + with_terms + [CRANFIELD])
    assert r.returncode == 1 and "not implemented under data parallelism" in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--device_corpus"] + with_terms + [CRANFIELD])
    assert r.returncode == 1 and "--device_corpus cannot be combined with --term_similarities" in r.stderr
    r = run_trainer(base + ["--update_method", "sgd", "--check_gradients"] + with_terms + [CRANFIELD])
    assert r.returncode == 1 and "--check_gradients covers the text-entity objective only" in r.stderr
    nothing = tmp_path / "no_terms.txt"
    nothing.write_text("%s %s 1.0\n%s %s 0.5\n" % (UNKNOWN[0], UNKNOWN[1], UNKNOWN[1], UNKNOWN[0]))
    r = run_trainer(base + ["--update_method", "sgd", "--term_similarity_weight", "0.3", "--term_similarities", str(nothing), CRANFIELD])
    assert r.returncode == 1 and "names two terms of the model" in r.stderr
