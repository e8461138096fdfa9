"""-m gpu: cuNVSMTrainModel --device_corpus — the collection in HBM, every batch handed over as window references — against the
run without the flag: the same epoch costs digit for digit and the same checkpoint bit for bit, whatever the order of the
epochs, the feature weighting, the sampler and the recipe; and the three combinations the flag refuses."""
import re

import numpy as np
import pytest

from tests.test_host_layer import h5_header
from tests.test_trainer_gpu import CRANFIELD, LSE_ARGS, _read_dataset, run_trainer

pytestmark = pytest.mark.gpu

COMMON = ["--document_cutoff", "300", "--num_epochs", "2"]
NVSM_FLAGS = ["--nonlinearity", "hard_tanh", "--batch_normalization", "--nobias_negative_samples", "--update_method", "sparse_adam",
              "--allow_ragged_batches"]
DATASETS = ("entity_representations-representations", "word_entity_mapping-bias", "word_entity_mapping-transform",
            "word_representations-representations")


def cost_list(stderr):
    """the cost=[...] of the last epoch line, as the trainer printed it"""
    last = [l for l in stderr.splitlines() if re.search(r"Epoch #\d+.*cost=\[", l)][-1]
    return re.search(r"cost=\[(.*)\]", last).group(1)


@pytest.mark.parametrize("extra", [[], ["--no_shuffle"], ["--feature_weighting", "self_information", "--sampler", "device"], NVSM_FLAGS],
                         ids=["default", "no_shuffle", "self_information-device_sampler", "nvsm-ragged"])
def test_device_corpus_trains_the_same_model(extra, tmp_path):
    runs = {}
    for name, flag in (("host", []), ("device", ["--device_corpus"])):
        out = str(tmp_path / name)
        r = run_trainer(LSE_ARGS + COMMON + extra + flag + ["--output", out, CRANFIELD])
        assert r.returncode == 0, r.stderr[-3000:]
        assert ("Device corpus:" in r.stderr) == bool(flag)
        runs[name] = (r.stderr, out + "_2.hdf5")
    costs = cost_list(runs["host"][0])
    assert costs == cost_list(runs["device"][0]) and len([c for c in costs.split(",") if c.strip()]) == 2
    skipped = [re.findall(r"Skipping Batch #\d+ .*", runs[n][0]) for n in ("host", "device")]
    assert skipped[0] == skipped[1] and bool(skipped[0]) == ("--allow_ragged_batches" not in extra)      # the skip rule is the same
    shapes = h5_header(runs["host"][1])
    assert shapes == h5_header(runs["device"][1]) and set(shapes) == set(DATASETS)
    for name in DATASETS:
        a, b = (_read_dataset(runs[n][1], name, shapes[name][1]) for n in ("host", "device"))
        assert a.size > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def test_initial_cost_from_window_references(tmp_path):
    """--compute_initial_cost goes through nvsm_compute_cost_windows: one more epoch of the plan, the same numbers"""
    args = LSE_ARGS + ["--document_cutoff", "300", "--num_epochs", "1", "--compute_initial_cost"]
    a, b = run_trainer(args + [CRANFIELD]), run_trainer(args + ["--device_corpus", CRANFIELD])
    assert a.returncode == 0 and b.returncode == 0, a.stderr[-2000:] + b.stderr[-2000:]
    assert cost_list(a.stderr) == cost_list(b.stderr) and len(cost_list(a.stderr).split(",")) >= 2


def test_device_corpus_refusals(tmp_path):
    sims = tmp_path / "sims.txt"
    sims.write_text("1 2 1.0\n")
    base = LSE_ARGS + COMMON + ["--device_corpus"]
    r = run_trainer(base + [CRANFIELD, str(sims)])
    assert r.returncode == 1 and "--device_corpus cannot be combined with a similarity file" in r.stderr
    r = run_trainer(base + ["--check_gradients", CRANFIELD])
    assert r.returncode == 1 and "--device_corpus cannot be combined with --check_gradients" in r.stderr
    for dp in (["--gpus", "2"], ["--world_size", "2", "--rank", "0"]):
        r = run_trainer(base + dp + [CRANFIELD])
        assert r.returncode == 1 and "--device_corpus is not implemented under data parallelism" in r.stderr
