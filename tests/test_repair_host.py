"""CPU: the repair matrix from the library's host math
(tests/host/test_repair_matrix.cpp: lagrange_matrix mode 1 at the targets'
points, pack_row, pack_mf_dword, mf_entry -- no GPU call) against the
oracle: rebuilding fragment t from the fragments `ids` is the oracle's
generator row t applied to the oracle's decode matrix of `ids`."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from qi_testlib import Q, decode_matrix, generator_matrix, matvec_mod, row_scale

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIBDIR = os.path.join(ROOT, "quadiron_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    if not os.path.exists(os.path.join(LIBDIR, "libquadiron_amd.so")):
        pytest.fail("libquadiron_amd.so not built")
    out = str(tmp_path_factory.mktemp("repair") / "test_repair_matrix")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", os.path.join(HERE, "host", "test_repair_matrix.cpp"),
        "-o", out, "-L" + LIBDIR, "-lquadiron_amd", "-Wl,-rpath," + LIBDIR])
    return out


def _expected(k, m, sys_, ids, targets):
    G = generator_matrix(k, m, sys_)
    F = np.vstack([np.eye(k, dtype=np.int64), G]) if sys_ else G
    return matvec_mod(F[targets], decode_matrix(k, m, sys_, ids))


@pytest.mark.parametrize("k,m,sys_", [(3, 3, 0), (3, 3, 1), (16, 48, 0), (16, 48, 1),
                                      (64, 960, 0), (200, 56, 1)])
def test_repair_matrix_vs_oracle(exe, k, m, sys_):
    rng = np.random.default_rng(31 * k + sys_)
    n = 1
    while n < k + m:
        n *= 2
    r = pow(3, 65536 // n, Q)
    R = min(m, 17)
    targets = rng.choice(k + m, R, replace=False)
    rest = np.setdiff1d(np.arange(k + m), targets)
    ids = rng.permutation(rng.choice(rest, k, replace=False))
    res = subprocess.run([exe, str(k), str(n), str(r), str(R)] + [str(int(v)) for v in ids] +
                         [str(int(v)) for v in targets], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")
    M = np.array([ln.split()[1:] for ln in lines if ln.startswith("M")], np.int64)
    P = np.array([ln.split()[1:] for ln in lines if ln.startswith("P")], np.int64)
    S = np.array([ln.split()[1:] for ln in lines if ln.startswith("S")], np.int64)
    exp = _expected(k, m, sys_, ids, targets)
    assert M.shape == exp.shape == (R, k)
    assert (M == exp).all()
    # packed rows read back through mf_entry: the row-scaled matrix, with
    # pack_row's scale and its balanced inverse in rscale / rscale_mf
    for j in range(R):
        s = row_scale(exp[j])
        assert S[j, 0] == s
        assert (P[j] == exp[j] * s % Q).all()
        inv = pow(int(s), Q - 2, Q)
        assert S[j, 1] % Q == inv and S[j, 2] % Q == inv
