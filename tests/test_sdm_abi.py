"""CPU-side checks of the sequential-dependence boundary (nvsm_sdm_rank / nvsm_sdm_pair_counts / nvsm_rank_ensemble_sdm and
nvsm_sdm_options): the symbols are declared and exported, the ctypes struct has the C size and offsets and the older structs did not
move, the defaults are the header's, null arguments are status codes that name the argument, the C++ wrapper compiles, and the Python
layer refuses without a device what needs none."""
import ctypes as C
import os
import subprocess

import pytest

import cunvsm_amd as ca
from cunvsm_amd import _lib
from cunvsm_amd import model as cm
from tests.conftest import ROOT

NEW = ("nvsm_sdm_options_default", "nvsm_sdm_rank", "nvsm_sdm_pair_counts", "nvsm_rank_ensemble_sdm")


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
    assert hasattr(ca.lib(), "nvsm_sdm_rank")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n",\n'
                   '  sizeof(nvsm_sdm_options), offsetof(nvsm_sdm_options, w_term), offsetof(nvsm_sdm_options, w_ordered),\n'
                   '  offsetof(nvsm_sdm_options, w_unordered), offsetof(nvsm_sdm_options, window), offsetof(nvsm_sdm_options, reserved),\n'
                   '  sizeof(nvsm_config), sizeof(nvsm_batch), sizeof(nvsm_lexical_options), sizeof(nvsm_ensemble_options),\n'
                   '  sizeof(nvsm_feedback_options), sizeof(nvsm_judgments), NVSM_SDM_MAX_WINDOW, NVSM_SDM_MAX_QUERY_PAIRS); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = ca.NvsmSdmOptions
    assert got[0] == C.sizeof(S) == 32
    assert got[1:6] == [S.w_term.offset, S.w_ordered.offset, S.w_unordered.offset, S.window.offset, S.reserved.offset] == [0, 4, 8, 12, 16]
    assert got[6:8] == [112, 48]                                          # nvsm_config and nvsm_batch did not move
    assert got[8:12] == [C.sizeof(ca.NvsmLexicalOptions), C.sizeof(ca.NvsmEnsembleOptions), C.sizeof(ca.NvsmFeedbackOptions),
                         C.sizeof(ca.NvsmJudgments)] == [32, 32, 32, 48]
    assert got[12] == _lib.SDM_MAX_WINDOW == ca.SDM_MAX_WINDOW == 64 and 16 <= got[12] <= 256
    assert got[13] == 1024


def test_defaults():
    L = ca.lib()
    o = ca.NvsmSdmOptions()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    L.nvsm_sdm_options_default(C.byref(o))
    assert (o.w_term, o.w_ordered, o.w_unordered) == (C.c_float(0.85).value, C.c_float(0.10).value, C.c_float(0.05).value)
    assert (o.window, list(o.reserved)) == (8, [0] * 4)
    L.nvsm_sdm_options_default(None)                                      # a null pointer is ignored, as by the other defaults
    d = cm.sdm_options()
    assert (d.w_term, d.w_ordered, d.w_unordered, d.window) == (o.w_term, o.w_ordered, o.w_unordered, o.window)


def test_null_arguments_are_status_1_with_the_arguments_name():
    L = ca.lib()
    q, ro, lo, so, eo, j = (ca.NvsmQueries(), ca.NvsmRankOptions(), ca.NvsmLexicalOptions(), ca.NvsmSdmOptions(), ca.NvsmEnsembleOptions(),
                            ca.NvsmJudgments())
    fake = C.c_void_p(8)                    # never dereferenced: the pointer checks come first
    out = (C.c_int64 * 4)()
    o = C.cast(out, C.c_void_p)
    rank = [fake, C.byref(q), C.byref(lo), C.byref(so), o, o, o]
    for at, name in ((0, "m"), (1, "queries"), (2, "lex"), (3, "sdm"), (4, "doc_ids"), (5, "scores"), (6, "counts")):
        args = list(rank)
        args[at] = None
        assert L.nvsm_sdm_rank(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name
    pairs = [fake, C.byref(q), C.byref(so), o, o]
    for at, name in ((0, "m"), (1, "queries"), (2, "sdm"), (3, "ordered"), (4, "unordered")):
        args = list(pairs)
        args[at] = None
        assert L.nvsm_sdm_pair_counts(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name
    fused = [fake, C.byref(q), C.byref(ro), C.byref(lo), C.byref(so), C.byref(eo), None, None, o, o, o]
    for at, name in ((0, "m"), (1, "queries"), (2, "rank_opt"), (3, "lex"), (4, "sdm"), (5, "ens"), (8, "doc_ids"), (9, "scores"), (10, "counts")):
        args = list(fused)
        args[at] = None
        assert L.nvsm_rank_ensemble_sdm(*args) == 1 and ("null argument: " + name).encode() in L.nvsm_last_error(), name
    args = list(fused)
    args[6] = C.byref(j)                    # judgments without metrics, and metrics without judgments
    assert L.nvsm_rank_ensemble_sdm(*args) == 1 and b"null argument: metrics" in L.nvsm_last_error()
    args = list(fused)
    args[7] = o
    assert L.nvsm_rank_ensemble_sdm(*args) == 1 and b"null argument: judgments" in L.nvsm_last_error()


def test_the_cpp_wrapper_compiles_with_the_new_members(tmp_path):
    assert hasattr(ca.lib(), "nvsm_sdm_rank")
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\n'
                   'void f(cunvsm_amd::Model& m, const std::vector<int64_t>& w, const std::vector<int64_t>& o, const nvsm_judgments& j) {\n'
                   '  nvsm_lexical_options lex; nvsm_lexical_options_default(&lex); nvsm_sdm_options sdm; nvsm_sdm_options_default(&sdm);\n'
                   '  nvsm_rank_options r; nvsm_rank_options_default(&r); nvsm_ensemble_options e; nvsm_ensemble_options_default(&e);\n'
                   '  sdm.window = NVSM_SDM_MAX_WINDOW;\n'
                   '  cunvsm_amd::Model::Ranking a = m.sdm_rank(w, o, lex, sdm); (void)a;\n'
                   '  cunvsm_amd::Model::PairCounts p = m.sdm_pair_counts(w, o, sdm); const uint64_t* c = p.ordered.data(); (void)c;\n'
                   '  cunvsm_amd::Model::Evaluation v = m.rank_ensemble_sdm(w, o, r, lex, sdm, e); (void)v;\n'
                   '  v = m.rank_ensemble_sdm(w, o, r, lex, sdm, e, &j); }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_option_checks_need_no_device():
    assert hasattr(ca.lib(), "nvsm_sdm_rank")
    opt = cm.sdm_options((1, 0, 0), 2)
    assert (opt.w_term, opt.w_ordered, opt.w_unordered, opt.window) == (1.0, 0.0, 0.0, 2)
    assert cm.sdm_options(window=64).window == 64 and cm.sdm_options(True).window == 8 and cm.sdm_options(dict(window=3)).window == 3
    assert cm.sdm_options(opt) is opt
    for bad in (dict(weights=(0, 0, 0)), dict(weights=(-0.1, 1, 1)), dict(weights=(float("nan"), 1, 1)), dict(weights=(float("inf"), 0, 0)),
                dict(weights=(1, 1)), dict(window=1), dict(window=65), dict(window=0)):
        with pytest.raises(ValueError):
            cm.sdm_options(**bad)
