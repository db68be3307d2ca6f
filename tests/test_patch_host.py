"""CPU: the device patch's per-fix decisions from the library's host header.
tests/host/test_patch_math.cpp -- a stand-alone program over
quadiron_amd/csrc/patch_math.h and fec_stage.h, which need neither HIP nor the
library -- is built with g++ under ASan + UBSan and run: random fix lists
through a plain C++ loop with the kernel's phases must leave exactly the rows,
marks, applied count and refusal of stage::apply_fixes / stage::apply_deltas.
See that file for what is checked."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_patch_math_on_host(tmp_path):
    assert shutil.which("g++") is not None, "g++ not found"
    exe = str(tmp_path / "test_patch_math")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all",
        os.path.join(HERE, "host", "test_patch_math.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ALL OK" in r.stdout, r.stdout[-2000:]
