"""The width and the packing of the persistent sweep's item-draw list entries (myfm_amd/csrc/mfm_res_entry.hpp), on the host:
tests/native/res_entry_main.cpp is a stand-alone program around the header, compiled with -fsanitize=address,undefined. It
covers run indices 0, 2^23 - 1 (the last that packs into 4 bytes) and 2^23 (the first that keeps 8), items 0 and 511, and the
row-sharded form's 8 bytes. A plan of more than 2^23 runs is out of reach of the GPU tests' table sizes: the width function is
held to it here."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "native", "res_entry_main.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_entry_width_and_packing_under_a_host_sanitizer(tmp_path):
    exe = str(tmp_path / "res_entry_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "myfm_amd", "csrc"), MAIN, "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0, out.stdout.decode()
    assert b"entry: ok" in out.stdout


def test_res_info_reports_the_entry_width_behind_the_existing_fields():
    from myfm_amd import _capi

    assert _capi.Context.RES_INFO[:15] == ("ready", "G", "RV", "RL", "RX", "umax", "n_items", "item_bits", "n_runs", "max_wg_users",
                                           "max_slice_items", "e_where", "n_rows", "s2_in_sweep_b", "lds_bytes")
    assert _capi.Context.RES_INFO[15:] == ("entry_bytes",)
    with open(os.path.join(ROOT, "include", "myfm_hip.h")) as fp:
        assert "#define MFM_RES_INFO_FIELDS %d\n" % len(_capi.Context.RES_INFO) in fp.read()
