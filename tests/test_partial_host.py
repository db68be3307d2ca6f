"""CPU: the partial repair's coefficients c(t, i) from the library's host
header (tests/host/test_partial_math.cpp compiles quadiron_amd/csrc/
partial_math.h alone, with -fsanitize=address,undefined).  The program checks
them against a brute-force Lagrange product and checks that the sum over all k
positions reproduces P(y_t); here they are compared with the oracle's repair
matrix (rows `targets` of the generator times the decode matrix of `ids`) for
both code types."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from qi_testlib import repair_matrix

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    out = str(tmp_path_factory.mktemp("partial") / "test_partial_math")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=undefined",
        os.path.join(HERE, "host", "test_partial_math.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("k,m", [(3, 3), (16, 48), (300, 212)])
def test_partial_coefficients(exe, k, m, sys_):
    rng = np.random.default_rng([k, m, sys_, 17])
    perm = rng.permutation(k + m)
    ids, rest = perm[:k], perm[k:]
    # a data row and a parity among the targets where there are any
    targets = [int(v) for v in rest[:min(3, m)]]
    res = subprocess.run([exe, str(k), str(m), str(len(targets))] + [str(t) for t in targets] +
                         [str(int(i)) for i in ids], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr
    lines = res.stdout.split("\n")
    assert "OK" in lines
    got = np.array([ln.split()[1:] for ln in lines if ln.startswith("C")], np.int64)
    assert (got[:, 0] == targets).all()
    exp = repair_matrix(k, m, sys_, ids, targets)
    assert got[:, 1:].shape == exp.shape == (len(targets), k)
    assert (got[:, 1:] == exp).all()
    # context words per stripe: H x RP coefficients + RP targets + H ids
    w = [ln for ln in lines if ln.startswith("W")][0].split()[1:]
    assert [int(v) for v in w] == [1 + 1 + 1, 5 * 4 + 4 + 5, 16 * 8 + 8 + 16, 2 * k + 2 + k]
