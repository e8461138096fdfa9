"""CPU-side checks of the supervised-fusion boundary (nvsm_ensemble_sweep / nvsm_rank_ensemble_cv and their option structs): the
symbols are declared and exported, the ctypes structs have the C sizes and the older structs did not move, the defaults are the
header's, null arguments are status codes that name the argument, the C++ wrapper compiles, and the Python layer refuses without a
device what needs none."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cunvsm_amd as ca
from cunvsm_amd import _lib
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_sweep_options_default", "nvsm_cv_options_default", "nvsm_ensemble_sweep", "nvsm_rank_ensemble_cv")


def test_the_header_declares_and_the_library_exports_the_calls():
    ca.build_library()
    names = ca.abi_symbols()
    for n in NEW:
        assert n in names
        assert hasattr(ca.lib(), n)
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert " T " + n in exported, n


def test_struct_sizes_match_the_header_and_the_older_structs_did_not_move(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\\n",\n'
                   '  sizeof(nvsm_sweep_options), sizeof(nvsm_cv_options), sizeof(nvsm_config), sizeof(nvsm_batch),\n'
                   '  sizeof(nvsm_ensemble_options), sizeof(nvsm_judgments), sizeof(nvsm_feedback_options),\n'
                   '  offsetof(nvsm_sweep_options, num_alphas), offsetof(nvsm_sweep_options, normalizer), offsetof(nvsm_sweep_options, depth),\n'
                   '  offsetof(nvsm_cv_options, num_folds), offsetof(nvsm_cv_options, fold_of), NVSM_SWEEP_MAX_ALPHAS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got[:2] == [C.sizeof(ca.NvsmSweepOptions), C.sizeof(ca.NvsmCvOptions)] == [40, 32]
    assert got[2:4] == [112, 48]                                          # nvsm_config and nvsm_batch did not move
    assert got[4:7] == [C.sizeof(ca.NvsmEnsembleOptions), C.sizeof(ca.NvsmJudgments), C.sizeof(ca.NvsmFeedbackOptions)] == [32, 48, 32]
    assert got[7:10] == [ca.NvsmSweepOptions.num_alphas.offset, ca.NvsmSweepOptions.normalizer.offset, ca.NvsmSweepOptions.depth.offset]
    assert got[10:12] == [ca.NvsmCvOptions.num_folds.offset, ca.NvsmCvOptions.fold_of.offset] == [4, 8]
    assert got[12] == _lib.SWEEP_MAX_ALPHAS == ca.SWEEP_MAX_ALPHAS == 1024


def test_defaults():
    L = ca.lib()
    sw, cv = ca.NvsmSweepOptions(), ca.NvsmCvOptions()
    C.memset(C.byref(sw), 0xFF, C.sizeof(sw))
    C.memset(C.byref(cv), 0xFF, C.sizeof(cv))
    L.nvsm_sweep_options_default(C.byref(sw))
    L.nvsm_cv_options_default(C.byref(cv))
    assert (sw.alphas, sw.num_alphas, sw.normalizer, sw.depth, list(sw.reserved)) == (None, 0, ca.NORM_STANDARDIZE, 0, [0] * 5)
    assert (cv.measure, cv.num_folds, cv.fold_of, list(cv.reserved)) == (_lib.EVAL_AP, 20, None, [0] * 4)
    L.nvsm_sweep_options_default(None)                                    # a null pointer is ignored, as by the other defaults
    L.nvsm_cv_options_default(None)


def test_null_arguments_are_status_1_with_the_arguments_name():
    L = ca.lib()
    q, ro, lo, fo, so, co, j = (ca.NvsmQueries(), ca.NvsmRankOptions(), ca.NvsmLexicalOptions(), ca.NvsmFeedbackOptions(),
                                ca.NvsmSweepOptions(), ca.NvsmCvOptions(), ca.NvsmJudgments())
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    out = (C.c_int64 * 4)()
    o = C.cast(out, C.c_void_p)
    sweep = [fake, C.byref(q), C.byref(ro), C.byref(lo), C.byref(fo), C.byref(so), C.byref(j), o]
    for at, name in ((0, "m"), (1, "queries"), (2, "rank_opt"), (3, "lex"), (5, "sweep"), (6, "judgments"), (7, "metrics")):
        args = list(sweep)
        args[at] = None
        assert L.nvsm_ensemble_sweep(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name
    cv = [fake, C.byref(q), C.byref(ro), C.byref(lo), None, C.byref(so), C.byref(co), C.byref(j), o, o, o, o, o, None, None]
    for at, name in ((0, "m"), (1, "queries"), (2, "rank_opt"), (3, "lex"), (5, "sweep"), (6, "cv"), (7, "judgments"), (8, "fold_alpha"),
                     (9, "fold_train_measure"), (10, "doc_ids"), (11, "scores"), (12, "counts")):
        args = list(cv)
        args[at] = None
        assert L.nvsm_rank_ensemble_cv(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name


def test_the_cpp_wrapper_compiles_with_the_new_members(tmp_path):
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m, const std::vector<int64_t>& w, const std::vector<int64_t>& o, const nvsm_judgments& j,\n'
                   '       const std::vector<float>& alphas, const std::vector<int32_t>& folds) {\n'
                   '  nvsm_lexical_options lex; nvsm_lexical_options_default(&lex); nvsm_feedback_options fb; nvsm_feedback_options_default(&fb);\n'
                   '  nvsm_rank_options r; nvsm_rank_options_default(&r);\n'
                   '  cunvsm_amd::Model::Sweep s = m.ensemble_sweep(w, o, r, lex, alphas, j); (void)s;\n'
                   '  s = m.ensemble_sweep(w, o, r, lex, alphas, j, NVSM_NORM_MINMAX, 1000, &fb);\n'
                   '  cunvsm_amd::Model::CrossValidation c = m.rank_ensemble_cv(w, o, r, lex, alphas, j); (void)c;\n'
                   '  c = m.rank_ensemble_cv(w, o, r, lex, alphas, j, 5, NVSM_EVAL_NDCG, NVSM_NORM_NONE, 0, &folds, &fb); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_option_checks_need_no_device():
    a = cm.sweep_alphas([0.5, 0.0, 1.0, 0.5])
    assert a.dtype == np.float32 and a.tolist() == [0.5, 0.0, 1.0, 0.5]
    opt = cm.sweep_options(a, "minmax", 1000)
    assert (opt.alphas, opt.num_alphas, opt.normalizer, opt.depth) == (a.ctypes.data, 4, ca.NORM_MINMAX, 1000)
    for bad in ([], [1.5], [-0.01], [0.5, float("nan")], [float("inf")], np.zeros(1025)):
        with pytest.raises(ValueError):
            cm.sweep_alphas(bad)
    assert cm.sweep_alphas(np.zeros(1024)).size == 1024
    for bad in (dict(normalizer="zscore"), dict(depth=-1)):
        with pytest.raises(ValueError):
            cm.sweep_options(a, **bad)
    with pytest.raises(ValueError):
        ca.alpha_grid(0.0005)
