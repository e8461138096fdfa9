"""One sequence of training calls that mixes every call form on ONE handle — text batches, window references from the host and
from the device, the mixed objective, the pair objective alone, deferred costs, and two refused calls — in its fused form
(nvsm_step*) and as compute_cost*; compute_gradients; update. tests/test_gpu_step_requests.py holds the two forms against each
other bit for bit; tools/step_trace.py runs them under a tracer to compare the engine's HIP calls between two builds."""
import numpy as np

import cunvsm_amd as ca
from tests.helpers import gpu_model

# (a) tables larger than the batch: the hoisted decay of the words rows without entries, the loss kernel carrying the event the
#     documents update waits for, the dT product on side stream 2 with its slab sum in the projection update
# (b) a large batch: the documents update held behind the dx product with no loss event, the dT product on the main stream
SHAPES = {
    "a": (dict(num_words=20000, num_entities=30000, word_dim=64, entity_dim=96, window=5, num_random=4, nonlinearity="tanh",
               batch_norm=False, bias_negative_samples=True, update_method="sgd", **{"lambda": 0.01}), 512, 100, 0.1),
    "b": (dict(num_words=3000, num_entities=5000, word_dim=300, entity_dim=256, window=4, num_random=3, nonlinearity="hard_tanh",
               batch_norm=True, bias_negative_samples=False, update_method="dense_adam", **{"lambda": 0.01}), 16384, 1000, 0.001),
}
CORPUS_DOCUMENTS, CORPUS_TOKENS = 300, 40

# every call form at least twice, each followed at least once by another one; "no_corpus" (a window call before any upload) and
# "bad_lr" (a step with lr = -1: refused behind its forward pass) are refused and must leave nothing behind
SEQUENCE = ("no_corpus", "step", "windows_host", "windows_device", "mixed", "deferred", "bad_lr", "pairs", "step", "mixed", "pairs",
            "deferred", "windows_host", "windows_device", "step")
FUSED_TEXT_STEPS = sum(k in ("step", "windows_host", "windows_device", "mixed", "deferred") for k in SEQUENCE)


def status_of(call):
    try:
        call()
    except ca.NvsmError as e:
        return e.status
    return 0


class Inputs:
    """The corpus and one input per call of SEQUENCE, drawn once: both handles of a comparison get the same arrays."""

    def __init__(self, shape, seed=3):
        self.spec, self.B, self.M, self.lr = SHAPES[shape]
        spec, B, w = self.spec, self.B, self.spec["window"]
        rs = np.random.RandomState(seed)
        tokens = rs.randint(0, spec["num_words"], CORPUS_DOCUMENTS * CORPUS_TOKENS).astype(np.int32)
        offsets = np.arange(CORPUS_DOCUMENTS + 1, dtype=np.int64) * CORPUS_TOKENS
        self.corpus = ca.Corpus(tokens, offsets, rs.uniform(0.25, 2.0, CORPUS_DOCUMENTS).astype(np.float32),
                                rs.uniform(0.25, 2.0, spec["num_words"]).astype(np.float32))
        self.calls = []
        for kind in SEQUENCE:
            refs = np.stack([rs.randint(0, CORPUS_DOCUMENTS, B), rs.randint(0, CORPUS_TOKENS - w + 1, B)], axis=1).astype(np.uint32)
            words = (rs.zipf(1.3, B * w) % spec["num_words"]).astype(np.int64)
            batch = ca.Batch(words, rs.randint(0, spec["num_entities"], B).astype(np.int64),
                             rs.uniform(0.5, 1.5, B * w).astype(np.float32), rs.uniform(0.5, 1.5, B).astype(np.float32))
            pairs = ca.PairBatch(rs.randint(0, spec["num_entities"], (self.M, 2)).astype(np.int64),
                                 rs.uniform(0.5, 1.5, self.M).astype(np.float32))
            self.calls.append((kind, dict(refs=refs, batch=batch, pairs=pairs)))

    def model(self, seed=7):
        m = gpu_model(self.spec, self.B, sampler=ca.SAMPLER_DEVICE)
        m.initialize(seed)
        return m


def call(m, kind, x, lr, fused):
    """One call of SEQUENCE on handle m; returns its cost, or the status of a refused call."""
    if kind == "no_corpus":
        return status_of((lambda: m.step_windows(x["refs"], lr)) if fused else (lambda: m.compute_cost_windows(x["refs"])))
    if kind == "bad_lr":
        if fused:
            return status_of(lambda: m.step(x["batch"], -1.0))
        m.compute_cost(x["batch"])
        m.compute_gradients()
        return status_of(lambda: m.update(-1.0))
    refs = x["refs"]
    if kind == "windows_device":
        import torch
        refs = x["device_refs"] = torch.from_numpy(x["refs"].view(np.int32)).cuda()
    if fused:
        if kind == "step":
            return m.step(x["batch"], lr, want_cost=True)
        if kind == "deferred":
            return m.deferred_cost(m.step_deferred(x["batch"], lr))
        if kind in ("windows_host", "windows_device"):
            return m.step_windows(refs, lr, want_cost=True)
        return m.step_mixed(x["batch"] if kind == "mixed" else None, x["pairs"], lr, want_cost=True)
    if kind in ("step", "deferred"):
        m.compute_cost(x["batch"])
    elif kind in ("windows_host", "windows_device"):
        m.compute_cost_windows(refs)
    else:
        m.compute_cost_mixed(x["batch"] if kind == "mixed" else None, x["pairs"])
    m.compute_gradients()
    m.update(lr)
    return m.get_cost()
