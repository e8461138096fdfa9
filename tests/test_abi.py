"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads, exports every symbol the
public header declares, and refuses to run without a GPU (no CPU fallback, no oracle in the product path)."""
import ctypes as C
import os
import re

import pytest

import cunvsm_amd as ca
from tests.conftest import ROOT, gpu_available


def test_library_exports_every_declared_symbol():
    ca.build_library()
    L = ca.lib()
    names = ca.abi_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(L, n), "libcunvsm_amd.so does not export %s" % n


def test_unit_test_hooks_live_in_their_own_library():
    """nvsm_debug_* were exported from the PRODUCT library. They are declared in include/cunvsm_amd_test_hooks.h, built
    into libcunvsm_amd_testhooks.so (no kernels of its own: it calls the product's launchers), and libcunvsm_amd.so exports none."""
    import subprocess
    ca.build_library()
    hooks = ca._lib.hook_symbols()
    assert len(hooks) >= 7 and all(h.startswith("nvsm_debug_") for h in hooks)
    assert not set(hooks) & set(ca.abi_symbols())
    exported = subprocess.run(["nm", "-D", "--defined-only", ca.library_path()], capture_output=True, text=True, check=True).stdout
    assert "nvsm_debug_" not in exported and "nvsm_step" in exported
    hooks_so = os.path.join(ROOT, "cunvsm_amd", "libcunvsm_amd_testhooks.so")
    exported = subprocess.run(["nm", "-D", "--defined-only", hooks_so], capture_output=True, text=True, check=True).stdout
    for h in hooks:
        assert " T " + h in exported, h
    L = ca.lib()
    for h in hooks:
        assert hasattr(L, h)          # (the binding finds them through the hooks library)
    with pytest.raises(AttributeError):
        L.product.nvsm_debug_gemm


def test_version_and_defaults():
    L = ca.lib()
    assert b"gfx950" in L.nvsm_version()
    cfg = ca.default_config()
    # scripts/functions.sh:380-399 + NVSM flags (:266)
    assert (cfg.word_repr_size, cfg.entity_repr_size, cfg.window_size) == (300, 256, 10)
    assert cfg.batch_normalization == 1 and cfg.nonlinearity == ca.HARD_TANH and cfg.clip_sigmoid == 1
    assert cfg.update_method == ca.ADAM and cfg.adam_mode == ca.ADAM_DENSE_UPDATE_DENSE_VARIANCE
    assert abs(cfg.regularization_lambda - 1e-2) < 1e-9 and cfg.max_batch_size == 51200


def test_null_arguments_are_status_codes_not_crashes():
    L = ca.lib()
    assert L.nvsm_create(None, None) == 1
    assert L.nvsm_compute_gradients(None) == 1
    assert b"null" in L.nvsm_last_error()


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU failure mode")
def test_bind_host_thread_without_a_device_is_a_status_code():
    import os
    before = os.sched_getaffinity(0)
    with pytest.raises(ca.NvsmError) as e:
        ca.bind_host_thread(0)
    assert e.value.status == 5          # NVSM_ERR_NO_DEVICE
    assert os.sched_getaffinity(0) == before


@pytest.mark.skipif(gpu_available(), reason="checks the no-GPU failure mode")
def test_no_cpu_fallback():
    cfg = ca.default_config(num_words=10, num_entities=10, max_batch_size=8)
    with pytest.raises(ca.NvsmError) as e:
        ca.Model(cfg)
    assert e.value.status == 5          # NVSM_ERR_NO_DEVICE


def test_product_package_never_touches_the_oracle():
    pkg = os.path.join(ROOT, "cunvsm_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", ".hpp", "Makefile")):
                with open(os.path.join(dirpath, f), errors="ignore") as fh:
                    src = fh.read()
                assert not re.search(r"nvsm_oracle|from oracle|import oracle|oracle/", src), os.path.join(dirpath, f)


def test_config_struct_matches_header_size():
    # 2 x int64 + 20 x int32/float + 4 reserved int32 = 16 + 24*4 = 112 bytes
    assert C.sizeof(ca.NvsmConfig) == 112
    assert C.sizeof(ca.NvsmBatch) == 48


def test_hook_structs_match_their_ctypes_mirrors(tmp_path):
    """The argument structs of include/cunvsm_amd_test_hooks.h against cunvsm_amd/_lib.py, field by field: size and every offset, as
    the C compiler lays them out (a field added to one side only, or in another place, shifts everything behind it)."""
    import subprocess
    pairs = [("nvsm_debug_gemm_epilogue_args", ca._lib.GemmEpilogueArgs), ("nvsm_debug_table_pass_args", ca._lib.TablePassArgs),
             ("nvsm_debug_loss_args", ca._lib.LossArgs), ("nvsm_debug_lazy_refresh_args", ca._lib.LazyRefreshArgs)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "cunvsm_amd_test_hooks.h"', 'int main(void) {']
    for cname, mirror in pairs:
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for field, _ in mirror._fields_:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field.rstrip("_")))
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for cname, mirror in pairs:
        assert int(got[cname]) == C.sizeof(mirror), cname
        for field, _ in mirror._fields_:
            assert int(got["%s.%s" % (cname, field)]) == getattr(mirror, field).offset, (cname, field)
    # the lazy-decay fields of the table pass stand at its end: callers that do not know them are unaffected
    assert [f for f, _ in ca._lib.TablePassArgs._fields_][-4:] == ["stamp", "lazy_decay", "now", "stamp_out"]
    with open(os.path.join(ROOT, "include", "cunvsm_amd_test_hooks.h")) as f:
        header = f.read()
    for cname, mirror in pairs:      # no field of the header is missing from the mirror: count the declarators of the struct's body
        body = re.sub(r"/\*.*?\*/", "", header[header.index("typedef struct " + cname):header.index("} " + cname)], flags=re.S)
        body = body[body.index("{") + 1:]
        names = [d.strip().split()[-1].lstrip("*") for stmt in body.split(";") if stmt.strip() for d in stmt.split(",")]
        assert names == [f.rstrip("_") for f, _ in mirror._fields_], cname


def test_public_headers_compile(tmp_path):
    """include/cunvsm_amd.h is plain C (a cgo / JNI / ctypes binding can consume it); the C++ wrapper needs C++11 only."""
    import subprocess
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", os.path.join(inc, "cunvsm_amd.h")])
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", "-I", inc, os.path.join(inc, "cunvsm_amd_test_hooks.h")])
    src = tmp_path / "use.cpp"
    src.write_text('#include "cunvsm_amd/model.hpp"\nint main() { nvsm_config c; nvsm_config_default(&c); return c.device; }\n')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, str(src)])
