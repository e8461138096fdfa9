"""CPU-side checks of the positional layer's entry points at the drop-in boundary (the pattern of tests/test_index_abi.py): the
product library exports them, the ctypes mirror has the header's size and offsets, null handles are status codes, and cuNVSMQuery
refuses --lexical_positions without the flags it belongs to before it opens a model."""
import ctypes as C
import os
import subprocess

import cunvsm_amd as ca
from tests.conftest import ROOT
from tests.test_fold_abi import declaration
from tests.test_query_sdm_host import run_query

NEW = ["nvsm_corpus_index_positions", "nvsm_corpus_index_positions_free", "nvsm_corpus_positions"]

CTYPE_OF = {"nvsm_model*": C.c_void_p, "nvsm_positions_info*": C.POINTER(ca.NvsmPositionsInfo), "int64_t": C.c_int64}


def test_the_library_exports_the_positions_symbols_and_the_header_declares_them():
    ca.build_library()
    L = ca.lib()
    declared = ca.abi_symbols()
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert n in declared, n
        assert hasattr(L, n) and " T " + n in exported, n


def test_binding_argument_types_match_the_header():
    L = ca.lib()
    for n in NEW:
        ret, params = declaration(n)
        fn = getattr(L, n)
        assert ret == "int" and fn.restype == C.c_int, n
        assert len(fn.argtypes) == len(params), (n, params)
        for got, ctype in zip(fn.argtypes, params):
            if ctype == "int64_t*":                   # the host destination array, or the count (an int64 out)
                assert got in (C.POINTER(C.c_int64), C.c_void_p), (n, ctype)
            else:
                assert got == CTYPE_OF[ctype], (n, ctype, got)
    assert [p for p in declaration("nvsm_corpus_positions")[1]] == ["nvsm_model*", "int64_t", "int64_t", "int64_t", "int64_t*", "int64_t*"]


def test_struct_layout(tmp_path):
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cunvsm_amd.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(nvsm_positions_info), offsetof(nvsm_positions_info, num_positions),\n'
                   '           offsetof(nvsm_positions_info, bytes), offsetof(nvsm_positions_info, reserved));\n'
                   '    return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    I = ca.NvsmPositionsInfo
    assert got == [C.sizeof(I), I.num_positions.offset, I.bytes.offset, I.reserved.offset] == [64, 0, 8, 16]
    assert len(I().reserved) == 12


def test_null_handles_are_status_codes():
    L = ca.lib()
    info, n = ca.NvsmPositionsInfo(), C.c_int64(-7)
    assert L.nvsm_corpus_index_positions(None, C.byref(info)) == 1
    assert b"null argument: m" in L.nvsm_last_error()
    assert L.nvsm_corpus_index_positions(None, None) == 1
    assert L.nvsm_corpus_index_positions_free(None) == 1
    assert L.nvsm_corpus_positions(None, 0, 0, 0, None, C.byref(n)) == 1 and n.value == -7
    assert b"null argument: m" in L.nvsm_last_error()


def test_the_query_tool_refuses_the_flag_without_its_companions(tmp_path):
    topics, model, out = tmp_path / "topics", tmp_path / "model_1.hdf5", str(tmp_path / "run")
    topics.write_text("1 a query\n")
    model.write_text("not a checkpoint: the flags are refused before it is read\n")
    flags = ["--index", str(tmp_path / "collection"), "--topics", topics]
    tail = [model, out]
    qlm = ["--qlm", "dirichlet", "--qlm_run_out", out + "_qlm"]
    cases = [
        (qlm + ["--lexical_index", "always", "--lexical_positions"], "--lexical_positions needs --qlm_sdm"),
        (qlm + ["--qlm_sdm", "--lexical_positions"], "--lexical_positions needs --lexical_index"),
        (qlm + ["--lexical_positions"], "--lexical_positions needs"),
    ]
    for extra, word in cases:
        r = run_query(flags + extra + tail)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr[-500:])
        assert not os.path.exists(out + "-topics") and not os.path.exists(out + "_qlm-topics")
    # the accepted combination gets as far as the model, which is none
    r = run_query(flags + qlm + ["--qlm_sdm", "--lexical_index", "always", "--lexical_positions"] + tail)
    assert r.returncode != 0 and "--lexical_positions" not in r.stderr
    r = run_query(["--help"])
    assert r.returncode == 0 and "-lexical_positions (" in r.stdout
