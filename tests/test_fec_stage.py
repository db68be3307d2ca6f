"""Host-side (CPU) checks of the host facade's staging helpers: compiles
tests/host/test_fec_stage.cpp -- a stand-alone program over
quadiron_amd/csrc/fec_stage.h, which needs neither HIP nor the library --
with g++ under ASan + UBSan and runs it.  See that file for what is checked."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_fec_stage_on_host(tmp_path):
    exe = str(tmp_path / "test_fec_stage")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all",
        os.path.join(HERE, "host", "test_fec_stage.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ALL OK" in r.stdout, r.stdout[-2000:]


def test_fec_stage_header_is_hip_free():
    """fec_stage.h stays usable without a device: no HIP, no plan."""
    with open(os.path.join(HERE, "..", "quadiron_amd", "csrc", "fec_stage.h")) as f:
        includes = [l for l in f if l.lstrip().startswith("#include")]
    assert includes and not any("hip" in l or "qi_plan" in l or "qi_internal" in l
                                for l in includes), includes
