"""CPU: stage::apply_fixes with several fixes in one column, as the
multi-fragment locate emits them (tests/host/test_apply_fixes_multi.cpp, a
stand-alone program over quadiron_amd/csrc/fec_stage.h under ASan + UBSan)."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_apply_fixes_multi_on_host(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "test_apply_fixes_multi")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all",
        os.path.join(HERE, "host", "test_apply_fixes_multi.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ALL OK" in r.stdout, r.stdout[-2000:]
