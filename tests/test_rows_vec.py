"""Host-side (CPU) check of the rule for the streaming kernels' 16-byte form:
compiles tests/host/test_rows_vec.cpp -- a stand-alone program over the
inline predicates of quadiron_amd/csrc/qi_internal.h, which needs the HIP
headers (for the declarations around them) but neither a device nor the
library -- with g++ under ASan + UBSan and runs it."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")  # the Makefile's default


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_rows_vec_on_host(tmp_path):
    exe = str(tmp_path / "test_rows_vec")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem",
        os.path.join(ROCM, "include"),
        os.path.join(HERE, "host", "test_rows_vec.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ALL OK" in r.stdout, r.stdout[-2000:]
