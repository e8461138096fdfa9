"""cuNVSMQuery's --qlm_sdm, --sdm_weights and --sdm_window (cunvsm_amd/host/query_main.cpp) without a device: the flags are checked
before the model is opened, every refusal is an exit status with a sentence, and the help text names them."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

QUERY = os.path.join(ROOT, "cunvsm_amd", "bin", "cuNVSMQuery")


def run_query(args):
    if not os.path.exists(QUERY):
        pytest.fail("%s is missing: __graft_entry__.build() builds it" % QUERY)
    return subprocess.run([QUERY] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_refusals_need_no_device(tmp_path):
    topics, model, out = tmp_path / "topics", tmp_path / "model_1.hdf5", str(tmp_path / "run")
    topics.write_text("1 a query\n")
    model.write_text("not a checkpoint: the flags are refused before it is read\n")
    flags = ["--index", str(tmp_path / "collection"), "--topics", topics]
    tail = [model, out]
    qlm = ["--qlm", "dirichlet", "--qlm_run_out", out + "_qlm"]
    cases = [
        (["--qlm_sdm"], "--qlm_sdm needs --qlm"),
        (qlm + ["--qlm_sdm", "--qlm_prf"], "--qlm_sdm and --qlm_prf are mutually exclusive"),
        (["--qlm", "jm", "--qlm_sdm", "--ensemble_qrel", topics], "--qlm_sdm is not offered with --ensemble_qrel"),
        (qlm + ["--sdm_weights", "1,0,0"], "need --qlm_sdm"), (qlm + ["--sdm_window", "4"], "need --qlm_sdm"),
        (qlm + ["--qlm_sdm", "--sdm_weights", "0,0,0"], "--sdm_weights"), (qlm + ["--qlm_sdm", "--sdm_weights", "1,1"], "--sdm_weights"),
        (qlm + ["--qlm_sdm", "--sdm_weights", "1,1,1,1"], "--sdm_weights"), (qlm + ["--qlm_sdm", "--sdm_weights", "1,-1,1"], "--sdm_weights"),
        (qlm + ["--qlm_sdm", "--sdm_weights", "1,x,1"], "--sdm_weights"), (qlm + ["--qlm_sdm", "--sdm_weights", "1,nan,1"], "--sdm_weights"),
        (qlm + ["--qlm_sdm", "--sdm_weights", "1,1,"], "--sdm_weights"), (qlm + ["--qlm_sdm", "--sdm_weights", "1,,1"], "--sdm_weights"),
        (qlm + ["--qlm_sdm", "--sdm_weights", "inf,0,0"], "--sdm_weights"),
        (qlm + ["--qlm_sdm", "--sdm_window", "1"], "--sdm_window must be in [2, 64]"),
        (qlm + ["--qlm_sdm", "--sdm_window", "65"], "--sdm_window must be in [2, 64]"),
        (qlm + ["--qlm_sdm", "--sdm_window", "-8"], "--sdm_window must be in [2, 64]"),
    ]
    for extra, word in cases:
        r = run_query(flags + extra + tail)
        assert r.returncode == 1 and word in r.stderr, (extra, r.stderr[-500:])
        assert not os.path.exists(out + "-topics") and not os.path.exists(out + "_qlm-topics")
    # accepted flags get as far as the model, which is none
    r = run_query(flags + qlm + ["--qlm_sdm", "--sdm_weights", "0.8,0.15,0.05", "--sdm_window", "64"] + tail)
    assert r.returncode != 0 and "--sdm" not in r.stderr and "--qlm_sdm" not in r.stderr


def test_the_help_text_names_the_flags():
    r = run_query(["--help"])
    assert r.returncode == 0
    for flag in ("qlm_sdm", "sdm_weights", "sdm_window"):
        assert "-%s (" % flag in r.stdout
