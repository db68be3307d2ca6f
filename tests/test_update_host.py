"""CPU: the delta update's coefficients c(slot, id) from the library's host
header (tests/host/test_update_coef.cpp compiles quadiron_amd/csrc/
update_coef.h alone, with -fsanitize=undefined) against the oracle: the
coefficient of data row `id` in coded slot `slot` is the oracle's encode of
the unit vector at `id`, read at that slot."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from qi_testlib import codec, ctx_buffer, oracle

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    out = str(tmp_path_factory.mktemp("update") / "test_update_coef")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
        os.path.join(HERE, "host", "test_update_coef.cpp"), "-o", out])
    return out


def oracle_columns(k, m, sys_, ids):
    """(n_outputs, len(ids)) int64: column u is the oracle's encode of the
    unit vector at ids[u] (systematic: the parity rows)."""
    o = oracle()
    c = codec(k, m, sys_)
    first = k if sys_ else 0
    cw = (C.c_uint32 * c.n)()
    din = (C.c_uint32 * k)()
    ctx = ctx_buffer(c)
    if sys_:
        assert o.qo_ctx_init(C.byref(c), ctx, (C.c_uint32 * k)(*range(k))) == 0
    G = np.zeros((c.n_outputs, len(ids)), np.int64)
    for u, i in enumerate(ids):
        din[i] = 1
        o.qo_encode_column(C.byref(c), ctx if sys_ else None, din, cw)
        din[i] = 0
        G[:, u] = np.frombuffer(cw, np.uint32)[first:first + c.n_outputs]
    return G


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("k,m", [(3, 3), (16, 48), (64, 960), (200, 56), (600, 1448),
                                 (1000, 24)])
def test_update_coefficients_vs_oracle(exe, k, m, sys_):
    rng = np.random.default_rng(97 * k + sys_)
    no = m if sys_ else k + m
    ids = sorted({0, k - 1} | set(int(v) for v in rng.choice(k, min(k, 6), replace=False)))
    slots = sorted({0, no - 1} | set(int(v) for v in rng.choice(no, min(no, 12), replace=False)))
    res = subprocess.run([exe, str(sys_), str(k), str(m), str(len(ids))] +
                         [str(v) for v in ids] + [str(len(slots))] + [str(v) for v in slots],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    assert "runtime error" not in res.stderr, res.stderr
    lines = res.stdout.split("\n")
    got = np.array([ln.split()[1:] for ln in lines if ln.startswith("C")], np.int64)
    assert (got[:, 0] == slots).all()
    exp = oracle_columns(k, m, sys_, ids)[slots]
    assert got[:, 1:].shape == exp.shape == (len(slots), len(ids))
    assert (got[:, 1:] == exp).all()
    if sys_:
        assert [ln for ln in lines if ln.startswith("T")] == [f"T {m} {k}"]
    # context words per stripe: R x UP coefficients + R slots + UP ids
    w = [ln for ln in lines if ln.startswith("W")][0].split()[1:]
    assert [int(v) for v in w] == [1 + 1 + 1, 5 * 4 + 5 + 4, 7 * 8 + 7 + 8, 8 * m + m + 8]
