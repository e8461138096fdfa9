"""-m gpu: the kernel dispatch table (Model::describe) against the fp64 oracle, at every regime and its boundaries.

A step picks its projection products, its ∂T product and its loss kernel by batch size, shape, batch-norm, the L2 normalisers and
the optimiser (the row-sums-of-squares epilogue of Adagrad / sparse Adam). The kernel-level tests hold each product alone; here a
whole step of a model goes through whichever kernels its (shape, batch) selects, with the epilogues the model fuses in, and every
case first asserts which kernels those are — a moved threshold fails loudly instead of quietly testing another path.

1. The dispatch matrix: six shape families x twelve batch sizes (63/64, 511/512, 1 023/1 024, 8 192/8 193, 16 383/16 384,
   40 959/40 960), one compute_cost / compute_gradients / update against the oracle at test_gpu_parity.py's tolerances, the
   optimiser rotated so that every batch size has an SGD case and a case with the rowsq epilogue. Plus one lazily decayed case
   at 40 960 (∂T on side stream 2) and a describe()-only test that the matrix reaches every kernel describe() can name.
2. The exact-fp32 twins (NVSM_GEMM_SPLIT=0) of two families.
3. One handle whose batch size crosses every regime from step to step, fused and queued without a host wait, against separate
   calls bit for bit and against the oracle over the whole sequence.
"""
import numpy as np
import pytest

import cunvsm_amd as ca
from oracle import nvsm_oracle as orc
from tests.helpers import PARAMS, gpu_model, load_params, oracle_model, random_batch, random_params, rel_err

FWD_TOL, GRAD_TOL, UPD_TOL = 2e-5, 2e-4, 2e-4          # = tests/test_gpu_parity.py


def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not _gpu_present(), reason="needs an MI355X")]


def _spec(**kw):
    lam = kw.pop("lam", 0.01)
    s = dict(kw)
    s["lambda"] = lam
    return s


FAMILIES = {
    # the NVSM recipe's shape (= test_gpu_parity.SPECS["nvsm"]): gemm_rsplit, gemm_split, gemm_dt on the main stream, gemm_dtw
    "nvsm": _spec(num_words=500, num_entities=300, word_dim=300, entity_dim=256, window=10, num_random=16,
                  nonlinearity="hard_tanh", batch_norm=True),
    # the LSE recipe's shape: gemm_split forward with the bias epilogue; the backward (8 column blocks) on gemm_rows / tstat / tiled
    "lse": _spec(num_words=500, num_entities=200, word_dim=128, entity_dim=256, window=10, num_random=16,
                 nonlinearity="tanh", batch_norm=False, bias_negative_samples=True),
    # d_e = 128 with batch-norm: forward on gemm_rows / tstat with the batch-norm column sums, backward on gemm_rsplit / gemm_split
    "de128": _spec(num_words=500, num_entities=300, word_dim=300, entity_dim=128, window=10, num_random=16,
                   nonlinearity="hard_tanh", batch_norm=True),
    # d_e = 512: gemm_rsplit refuses K = 512, gemm_rows takes the backward with the fused batch-norm backward
    "wide": _spec(num_words=64, num_entities=64, word_dim=64, entity_dim=512, window=4, num_random=2,
                  nonlinearity="tanh", batch_norm=True, lam=0.0),
    # both L2 normalisers: the backward unfused at every batch size, the generic loss kernel
    "l2": _spec(num_words=300, num_entities=500, word_dim=300, entity_dim=256, window=10, num_random=16,
                nonlinearity="hard_tanh", batch_norm=True, l2_phrase=True, l2_entity=True),
    # d_e % 4 != 0: the generic loss kernel, the tiled exact-fp32 products and ∂T
    "odd": _spec(num_words=500, num_entities=300, word_dim=37, entity_dim=50, window=5, num_random=6,
                 nonlinearity="hard_tanh", batch_norm=False),
}
# Lazily decayed tables (Model::table_decays_lazily): NVSM_LAZY_MIN_MB=0, a decaying optimiser AND rows x split ratio (2) >= the
# handle's entries (40 960 x 3 words, 40 960 x 3 documents) — short windows and few negatives keep the fp64 oracle in reach
LAZY = _spec(num_words=61440, num_entities=61440, word_dim=300, entity_dim=256, window=3, num_random=2,
             nonlinearity="hard_tanh", batch_norm=True)
LAZY_MAX_B = 40960

# Dimensions users pick that are no recipe's: whole steps at the shapes tests/test_gpu_gemm_epilogues.py holds kernel by kernel — the same tail
# tiles, padded k steps and planner choices as there, with the model's own workspaces and stream order. (d_w, d_e):
#   (100, 36)   gemm_rsplit with four waves, a 4-column last tile both ways, an odd number of k steps; beyond 8 192 rows the tiled kernel
#   (200, 100)  gemm_rsplit staging eight float4s per thread forward, eight waves with the fused batch-norm backward on the way back
#   (316, 320)  ten waves; beyond 8 192 rows gemm_split's backward product at its largest K with the batch-norm backward, 20 column blocks
#   (256, 512)  no row-panel forward (N = 512); the backward refused by gemm_rsplit (K = 512 with batch-norm) and taken by gemm_rows
UNUSUAL = {"d%dx%d" % (dw, de): _spec(num_words=500, num_entities=300, word_dim=dw, entity_dim=de, window=10, num_random=16,
                                      nonlinearity="hard_tanh", batch_norm=True)
           for dw, de in ((100, 36), (200, 100), (316, 320), (256, 512))}
UNUSUAL_CASES = [(fam, B, method) for fam in UNUSUAL for B in (1024, 8193) for method in ("sgd", "adagrad")]

BATCHES = [63, 64, 511, 512, 1023, 1024, 8192, 8193, 16383, 16384, 40959, 40960]
SMALL_ONLY = {"wide": 16384, "l2": 16384}       # (runtime: these two families stop at 16 384 windows)
# rotated over the cases so that every batch size has an SGD case and a case with the rowsq epilogue (need_msq)
METHODS_CYCLE = ["sgd", "adagrad", "sparse_adam", "full_adam"]
LR = {"sgd": 0.1, "adagrad": 0.01}               # Adam modes 1e-3 (tests_base_cuda.h:117-130, as test_update_parity)
NEED_MSQ = {"adagrad", "sparse_adam", "dense_adam"}

MATRIX = [(fam, B, METHODS_CYCLE[(fi + bi) % len(METHODS_CYCLE)])
          for fi, fam in enumerate(FAMILIES) for bi, B in enumerate(BATCHES) if B <= SMALL_ONLY.get(fam, BATCHES[-1])]
TWINS = [(fam, B, METHODS_CYCLE[i % 2]) for fam in ("nvsm", "lse") for i, B in enumerate([1024, 8192, 8193, 16384, 40960])]

# the strings Model::describe can print for a product, a ∂T form, a loss kernel
FWD = {k: "forward " + v for k, v in dict(rsplit="gemm_rsplit", rows="gemm_rows", split="gemm_split",
                                          tstat="gemm_tstat (exact fp32 MFMA, projection stationary in LDS) or tiled",
                                          f32="gemm_f32_mfma").items()}
BWD = {k: "backward " + v[len("forward "):] for k, v in FWD.items()}
FUSED = "with the batch-norm backward / bias gradient inside"
DT = {"dt": "dT gemm_dt (", "dtw": "dT gemm_dtw", "f32": "dT gemm_f32_mfma / gemm_panel split-K (exact fp32 MFMA)"}
MAIN, SIDE2 = "on the main stream", "on side stream 2"
LOSS = {"rows": "loss loss_rows", "generic": "loss loss_kernel (generic)"}


def expected(fam, B, split=True, lazy=False):
    """DESIGN.md §4 written out per family: which forward / backward product, ∂T form and loss kernel a step of B windows takes.
    Thresholds: gemm_rsplit / gemm_rows from 512 to NVSM_GEMM_ROWS_MAX = 8 192, gemm_split above; gemm_tstat from 1 024; gemm_dtw
    from 64 to 16 383; gemm_dt on the main stream from kDtMainMinBatch = 16 384 (eager tables), from dt_min_batch = 40 960 on side
    stream 2 (lazy tables)."""
    if fam in UNUSUAL:
        return expected_unusual(fam, B)
    small, rows = B < 512, 512 <= B <= 8192
    if fam in ("nvsm", "l2"):
        fwd = bwd = "f32" if small else ("rsplit" if rows else "split")
        if not split and not small:
            fwd = bwd = "rows" if rows else "tstat"
    elif fam == "lse":
        fwd = "f32" if small else ("rsplit" if rows else "split")
        bwd = "f32" if small else ("rows" if rows else "tstat")
        if not split and not small:
            fwd = "rows" if rows else "tstat"
    elif fam == "de128":
        fwd = "f32" if small else ("rows" if rows else "tstat")
        bwd = "f32" if small else ("rsplit" if rows else "split")
    elif fam == "wide":
        fwd = "tstat" if B >= 1024 else "f32"
        bwd = "f32" if small else ("rows" if rows else "tstat")
    else:                                             # odd
        fwd = bwd = "f32"
    fused = B >= 512 and fam != "l2"
    if fam == "odd" or not split:
        dt = "f32"
    elif fam == "wide":                               # (d_e = 512 is beyond gemm_dt's 256 columns)
        dt = "dtw" if 64 <= B <= 16383 else "f32"
    elif B >= 40960 or (B >= 16384 and not lazy):
        dt = "dt"
    else:                                             # (lazy tables, 16 384 to 40 959: neither kernel, the tiled fp32 one)
        dt = "dtw" if 64 <= B <= 16383 else "f32"
    on_main = dt == "dt" and not lazy
    # the row-gathering loss kernel covers d_e % 4 == 0, d_e <= 256, no entity normaliser (loss_reads_lazily)
    loss = "generic" if fam in ("odd", "l2", "wide") else "rows"
    return dict(forward=FWD[fwd], backward=BWD[bwd], fused=fused, dT=DT[dt], main=on_main, loss=LOSS[loss])


def expected_unusual(fam, B):
    """The UNUSUAL families at 512 <= B <= 16 383 (batch-norm on, eager tables): the row-panel kernels to 8 192 rows; above, gemm_split
    only where d_w makes 17 to 24 column blocks of the backward product, else gemm_tstat or the tiled kernel."""
    assert 512 <= B <= 16383
    rows = B <= 8192
    if fam == "d256x512":
        fwd, bwd = "tstat" if B >= 1024 else "f32", "rows" if rows else "tstat"
    elif fam == "d316x320":
        fwd, bwd = ("rsplit", "rsplit") if rows else ("tstat", "split")
    else:
        fwd = bwd = "rsplit" if rows else "tstat"
    loss = "rows" if UNUSUAL[fam]["entity_dim"] <= 256 else "generic"
    return dict(forward=FWD[fwd], backward=BWD[bwd], fused=True, dT=DT["dtw"], main=False, loss=LOSS[loss])


def fields(desc):
    """describe()'s ' | '-separated fields by their first word (forward / backward / dT / loss / tables / ...)."""
    out = {}
    for f in desc.split(" | "):
        f = f.split(": ", 1)[1] if f.startswith("batch ") else f
        out[f.split(" ", 1)[0]] = f
    return out


def assert_dispatch(desc, want):
    f = fields(desc)
    assert f["forward"].startswith(want["forward"]), (want["forward"], desc)
    assert f["backward"].startswith(want["backward"]), (want["backward"], desc)
    assert (FUSED in f["backward"]) == want["fused"], (want["fused"], desc)
    assert f["dT"].startswith(want["dT"]), (want["dT"], desc)
    assert f["dT"].endswith(MAIN if want["main"] else SIDE2), (want["main"], desc)
    assert f["loss"].startswith(want["loss"]), (want["loss"], desc)


def fam_spec(fam, method):
    return dict(LAZY if fam == "lazy" else UNUSUAL[fam] if fam in UNUSUAL else FAMILIES[fam], update_method=method)


def fp32_yardstick(err_hip, err_f32, bound):
    """err_hip <= bound, or — a genuine fp32 effect — no further from fp64 than the fp32 oracle is (x 1.25 for the order of its
    sums; test_gpu_configs.py's yardstick). hard_tanh after batch-norm puts a third of the units on the bound: at these batch
    sizes one unit or a few land within fp32 roundoff of it, and any fp32 path sends such a unit's derivative the other way
    than fp64 does. One such unit moves ∂T, the bias gradient and one row of ∂phrase by ~1 / sqrt(B · d_e) of their norms,
    2e-4 … 6e-3 here — measured: the fp32 oracle flips the same units and sits at the same distance or further (1e-3 at
    nvsm B 16 383, 5.8e-3 at l2 B 1 023); Adagrad's first step divides by the gradient's own size (test_gpu_configs.py)."""
    return err_hip <= bound or err_hip <= 1.25 * err_f32


def one_step_against_oracle(spec, B, seed):
    """One compute_cost / compute_gradients / update on a Zipf batch, HIP handle (max_batch_size = B) against the fp64 oracle,
    at test_forward_backward_parity's and test_update_parity's tolerances. Returns the handle's describe(B)."""
    rs = np.random.RandomState(seed)
    params = random_params(spec, rs)
    o, o32, g = oracle_model(spec), oracle_model(spec, orc.F32), gpu_model(spec, B)
    load_params(o, params, False)
    load_params(o32, params, False)
    load_params(g, params, True)
    desc = g.describe(B)
    words, ww, labels, iw, ids = random_batch(spec, rs, B, zipf=True)
    for m in (o, o32):
        m.forward(words, ww, ids, iw)
    g.compute_cost(ca.Batch(words, labels, ww, iw), ids)
    co, cg = o.get_cost(), g.get_cost()
    assert abs(cg - co) <= FWD_TOL * abs(co), (cg, co)
    for t in ("phrase", "pre", "proj", "probs"):
        assert rel_err(g.get_tensor(t), o.get(t)) < FWD_TOL, (t, rel_err(g.get_tensor(t), o.get(t)))
    if spec.get("batch_norm"):
        assert rel_err(g.get_tensor("bn_inv_std"), o.get("bn_inv_std")) < FWD_TOL
    for m in (o, o32):
        m.backward()
    g.compute_gradients()
    for t in ("grad_transform", "grad_bias", "grad_phrase", "grad_entity", "grad_proj"):
        a, b, c = g.get_tensor(t), o.get(t), o32.get(t)
        assert fp32_yardstick(rel_err(a, b), rel_err(c, b), GRAD_TOL), (t, rel_err(a, b), rel_err(c, b))
        nb = np.linalg.norm(b)
        d_hip, d_f32 = abs(np.linalg.norm(a.astype(np.float64)) - nb), abs(np.linalg.norm(c) - nb)
        assert fp32_yardstick(d_hip, d_f32, 1e-4 * nb), (t, d_hip / nb, d_f32 / nb)
    R = spec["num_random"] + 1
    sign = np.where(np.arange(B * R) % R == 0, 1.0, -1.0)
    assert rel_err(g.get_tensor("multipliers"), o.get("multipliers") * sign) < GRAD_TOL
    lr = LR.get(spec["update_method"], 1e-3)
    for m in (o, o32):
        m.update(lr)
    g.update(lr)
    for p in PARAMS:
        new_o = o.get(p)
        delta = np.linalg.norm(new_o - params[p].astype(np.float64))
        err = np.linalg.norm(g.get_param(p).astype(np.float64) - new_o)
        err32 = np.linalg.norm(np.asarray(o32.get(p), np.float64) - new_o)
        # + the fp32 storage floor: one rounding of every parameter
        floor = 1e-7 * np.linalg.norm(new_o)
        assert fp32_yardstick(err, err32 + floor, UPD_TOL * max(delta, 1e-12) + floor), (p, err / delta, err32 / delta)
    return desc


# ---------------------------------------------------------------------------------------------
# 1. the dispatch matrix
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,B,method", MATRIX, ids=["%s-B%d-%s" % c for c in MATRIX])
def test_dispatch_matrix_matches_fp64_oracle(fam, B, method):
    spec = fam_spec(fam, method)
    desc = one_step_against_oracle(spec, B, seed=B + 7 * len(fam))
    assert_dispatch(desc, expected(fam, B))
    assert "words eager decay, documents eager decay" in desc, desc


def test_dispatch_matrix_lazy_tables_dt_on_side_stream_2(monkeypatch):
    """Lazily decayed tables keep ∂T off the main stream: gemm_dt on side stream 2 from dt_min_batch = 40 960 on."""
    monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    desc = one_step_against_oracle(fam_spec("lazy", "sparse_adam"), LAZY_MAX_B, seed=4096)
    assert "words lazy decay, documents lazy decay" in desc, desc
    assert_dispatch(desc, expected("nvsm", LAZY_MAX_B, lazy=True))


def test_dispatch_matrix_reaches_every_kernel_describe_names(monkeypatch):
    """describe() only (no step): the matrix's handles together name every product kernel, every ∂T form, both loss kernels and
    both backward forms Model::describe can print — nothing of the table is silently left out of the oracle cases above."""
    for B in BATCHES:                                 # (the rotation: an SGD case and a rowsq case at every batch size)
        methods = {m for _, b, m in MATRIX if b == B}
        assert "sgd" in methods and methods & NEED_MSQ, (B, methods)
    seen, main_dt, side_dt = set(), False, False
    for fam, B, method in MATRIX + [("lazy", LAZY_MAX_B, "sparse_adam")]:
        if fam == "lazy":
            monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
        desc = gpu_model(fam_spec(fam, method), B).describe(B)
        monkeypatch.delenv("NVSM_LAZY_MIN_MB", raising=False)
        assert_dispatch(desc, expected("nvsm" if fam == "lazy" else fam, B, lazy=fam == "lazy"))
        f = fields(desc)
        seen |= {s for s in list(FWD.values()) + list(BWD.values()) + list(DT.values()) + list(LOSS.values())
                 if f[s.split(" ", 1)[0]].startswith(s)}
        seen.add("fused" if FUSED in f["backward"] else "unfused")
        main_dt |= f["dT"].startswith(DT["dt"]) and f["dT"].endswith(MAIN)
        side_dt |= f["dT"].startswith(DT["dt"]) and f["dT"].endswith(SIDE2)
    want = set(FWD.values()) | set(BWD.values()) | set(DT.values()) | set(LOSS.values()) | {"fused", "unfused"}
    assert want <= seen, sorted(want - seen)
    assert main_dt and side_dt


@pytest.mark.parametrize("fam,B,method", UNUSUAL_CASES, ids=["%s-B%d-%s" % c for c in UNUSUAL_CASES])
def test_unusual_dimensions_match_fp64_oracle(fam, B, method):
    """One step at dimensions no recipe uses (UNUSUAL), with SGD and with an optimiser that takes the row sums of squares."""
    assert method == "sgd" or method in NEED_MSQ
    desc = one_step_against_oracle(fam_spec(fam, method), B, seed=B + 11 * len(fam) + UNUSUAL[fam]["word_dim"])
    assert_dispatch(desc, expected(fam, B))
    assert "words eager decay, documents eager decay" in desc, desc


# ---------------------------------------------------------------------------------------------
# 2. the exact-fp32 twins
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,B,method", TWINS, ids=["%s-B%d-%s" % c for c in TWINS])
def test_exact_fp32_twin_matches_fp64_oracle(fam, B, method, monkeypatch):
    """NVSM_GEMM_SPLIT=0 (read when the handle is made): gemm_rows, gemm_tstat and the tiled split-K ∂T with
    their epilogues, at model level."""
    monkeypatch.setenv("NVSM_GEMM_SPLIT", "0")
    desc = one_step_against_oracle(fam_spec(fam, method), B, seed=B + 3)
    assert_dispatch(desc, expected(fam, B, split=False))


# ---------------------------------------------------------------------------------------------
# 3. one handle across regimes
# ---------------------------------------------------------------------------------------------
SEQUENCE = [40960, 63, 6400, 16384, 8193, 512, 40959, 17, 16383, 9000, 64, 40960]
STATE = {"adagrad": ["word_representations/a", "entity_representations/a", "word_entity_mapping/s0_transform"],
         "sparse_adam": ["word_representations/m", "word_representations/v", "entity_representations/m", "entity_representations/v",
                         "word_entity_mapping/s0_transform", "word_entity_mapping/s1_transform", "word_entity_mapping/s0_bias",
                         "word_entity_mapping/s1_bias"]}


@pytest.mark.parametrize("tables,method", [("eager_large", "sparse_adam"), ("eager", "adagrad"), ("lazy", "sparse_adam")])
def test_one_handle_across_regimes(tables, method, monkeypatch):
    """Batch sizes that change regime from step to step on one handle (max_batch_size 40 960) — the last short batch of an epoch,
    uneven data-parallel shards. The projection update cuts T's bf16 planes only in its own step's layout; ∂T moves between the
    main stream and side stream 2 at 16 384 with eager tables (and the CSR build layout with it); the slab count changes per step
    within a workspace sized once. Every step's loss must be a fresh handle's (max_batch_size = that step's batch, same
    parameters) bit for bit; fused steps queued without a host wait must equal separate calls bit for bit; and both must follow
    the fp64 oracle over the whole sequence.
    (tanh rather than the recipe's hard_tanh: over twelve steps the units that land within fp32 roundoff of hard_tanh's bound —
    see fp32_yardstick — compound through Adam's normalisation until every fp32 path, the fp32 oracle included, is 0.1 … 0.6 of
    the change away from fp64; a smooth nonlinearity keeps the comparison meaningful. Batch-norm stays on: the fused batch-norm
    backward changes kernel along with the product.
    Sparse Adam on eager tables runs on the lazy case's larger tables with the lazy decay switched off (NVSM_LAZY_DECAY=0): on
    SPECS["nvsm"]'s 500 words every row takes thousands of entries a step, and twelve steps of the reference's sparse-Adam rule
    leave every fp32 path far from fp64 — measured 2.4e-2 (HIP) and 1.7e-2 (fp32 oracle) of the change.)"""
    if tables == "lazy":
        monkeypatch.setenv("NVSM_LAZY_MIN_MB", "0")
    elif tables == "eager_large":
        monkeypatch.setenv("NVSM_LAZY_DECAY", "0")
    spec = dict(fam_spec("nvsm" if tables == "eager" else "lazy", method), nonlinearity="tanh")
    tables = "lazy" if tables == "lazy" else "eager"
    Bmax = max(SEQUENCE)
    rs = np.random.RandomState(1 + len(tables) + len(method))
    params = random_params(spec, rs)
    o, o32, a, b = oracle_model(spec), oracle_model(spec, orc.F32), gpu_model(spec, Bmax), gpu_model(spec, Bmax)
    for m in (o, o32):
        load_params(m, params, False)
    for m in (a, b):
        load_params(m, params, True)
    for B in set(SEQUENCE):
        d = a.describe(B)
        assert_dispatch(d, expected("nvsm", B, lazy=tables == "lazy"))
        assert ("lazy decay" in d) == (tables == "lazy"), d
    batches = [random_batch(spec, rs, B, zipf=True) for B in SEQUENCE]
    lr = LR.get(method, 1e-3)
    tickets = [b.step_deferred(ca.Batch(w, l, ww, iw), lr, entity_ids=ids) for (w, ww, l, iw, ids) in batches]
    costs_b = [b.deferred_cost(t) for t in tickets[-8:]]
    costs_a = []
    for s, (w, ww, l, iw, ids) in enumerate(batches):
        B = SEQUENCE[s]
        if tables == "eager":       # (reading a lazily decayed table brings its rows up to date, which would change a's own arithmetic)
            fresh = gpu_model(spec, B)
            load_params(fresh, {p: a.get_param(p) for p in PARAMS}, True)
            fresh.compute_cost(ca.Batch(w, l, ww, iw), ids)
        a.compute_cost(ca.Batch(w, l, ww, iw), ids)
        a.compute_gradients()
        costs_a.append(a.get_cost())
        if tables == "eager":
            assert costs_a[-1] == fresh.get_cost(), (s, B, costs_a[-1], fresh.get_cost())
            del fresh
        a.update(lr)
        for m in (o, o32):
            m.forward(w, ww, ids, iw)
            m.backward()
            m.update(lr)
        if s == 0:                  # (later steps: the parameters' distance, below, is what the oracle bounds)
            co = o.get_cost()
            assert abs(costs_a[-1] - co) <= FWD_TOL * abs(co), (costs_a[-1], co)
    assert costs_b == costs_a[-8:]
    for n in list(PARAMS) + STATE[method]:
        np.testing.assert_array_equal(a.get_param(n), b.get_param(n), err_msg=n)
    # (= test_per_rank_batch_fused_steps_match_fp64_oracle: 5e-4 of the change for SGD / Adagrad, 5e-3 for the Adam modes)
    tol = 5e-3 if method.endswith("adam") else 5e-4
    for n in PARAMS:
        new_o, old = o.get(n), params[n].astype(np.float64)
        change = np.linalg.norm(new_o - old)
        err = np.linalg.norm(a.get_param(n).astype(np.float64) - new_o)
        err32 = np.linalg.norm(np.asarray(o32.get(n), np.float64) - new_o)
        floor = 1e-7 * np.linalg.norm(old)
        assert fp32_yardstick(err, err32 + floor, tol * change + floor), (n, err / change, err32 / change)
