"""CPU: the syndrome shares' host side (tests/host/test_syndrome_math.cpp
compiles quadiron_amd/csrc/syndrome_math.h and fec_stage.h alone, with
-fsanitize=address,undefined).  The program checks the coefficients x_i^j / w_i
against a brute-force product, checks that they annihilate every codeword, and
checks stage::apply_deltas against a direct model; here it runs at N = 5, 264
and 1108 listed fragments, and the context sizes are compared."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    out = str(tmp_path_factory.mktemp("syndrome") / "test_syndrome_math")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=undefined",
        os.path.join(HERE, "host", "test_syndrome_math.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("k,m,R", [(3, 5, 2), (260, 30, 4), (1100, 100, 8)])
def test_syndrome_math_on_host(exe, k, m, R):
    res = subprocess.run([exe, str(k), str(m), str(R)], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr
    lines = res.stdout.split("\n")
    assert "OK" in lines
    N = k + R
    RP = {1: 1, 2: 2, 3: 4, 4: 4}.get(R, 8)
    # share context: H x RP coefficients + RP filler words + H ids; resolve: 3 N
    w = [ln for ln in lines if ln.startswith("W")][0].split()[1:]
    assert [int(v) for v in w] == [1 + 1 + 1, 5 * 4 + 4 + 5, N * RP + RP + N, 3 * N]


def test_syndrome_math_header_is_hip_free():
    with open(os.path.join(HERE, "..", "quadiron_amd", "csrc", "syndrome_math.h")) as f:
        includes = [ln.strip() for ln in f if ln.lstrip().startswith("#include")]
    assert includes == ["#include <stdint.h>", '#include "partial_math.h"'], includes
