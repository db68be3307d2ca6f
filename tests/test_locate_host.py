"""CPU: the fragment locate's field arithmetic from the library's host header
(tests/host/test_locate_math.cpp compiles quadiron_amd/csrc/locate_math.h
alone, with -fsanitize=undefined) on columns of the oracle's encode: the
weights are tied to the oracle, not to the code under test.
  1. codeword columns have all-zero syndromes (clean);
  2. a single error at every listed position, e in {1, 65536, 32768, random},
     is classified (position, original symbol) exactly;
  3. with R >= 3, errors in 2 .. R - 1 fragments are always unlocated;
  4. a data-row correction to 65536 is unlocated (a coded-row one is a fix)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from qi_testlib import oracle_encode_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 65537


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    out = str(tmp_path_factory.mktemp("locate") / "test_locate_math")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
        os.path.join(HERE, "host", "test_locate_math.cpp"), "-o", out])
    return out


def oracle_fragments(k, m, sys_, P, rng):
    """(k + m, P) int64 restored symbols of P random codeword columns, by
    fragment id (decode id space), from the oracle's encode."""
    data = rng.integers(0, 65536, (k, P), dtype=np.uint16)
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, data.view(np.uint8).reshape(k, 2 * P),
                                          cap=P)
    coded = outs.view(np.uint16).reshape(-1, P).astype(np.int64)
    for j in range(coded.shape[0]):
        assert cnt[j] <= P
        coded[j, oor[j, :cnt[j]]] = 65536   # word offsets of the marks
    return np.concatenate([data.astype(np.int64), coded]) if sys_ else coded


def run(exe, sys_, k, m, R, ids, cols):
    text = "\n".join(" ".join(str(int(v)) for v in c) for c in cols) + "\n"
    res = subprocess.run([exe, str(sys_), str(k), str(m), str(R), str(len(ids))] +
                         [str(int(v)) for v in ids], input=text, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert "runtime error" not in res.stderr, res.stderr
    lines = res.stdout.split("\n")
    assert lines[0] == f"W {(k + R) * (3 + (2 if R <= 2 else 4 if R <= 4 else 8))}"
    got = np.array([ln.split() for ln in lines[1:] if ln], np.int64)
    assert got.shape == (len(cols), 3)
    return got


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("R0", [2, 3, 8])
@pytest.mark.parametrize("k,m", [(3, 3), (16, 48), (64, 960), (200, 56), (256, 768)])
def test_locate_math_vs_oracle(exe, k, m, R0, sys_):
    R = min(R0, m)
    N = k + R
    rng = np.random.default_rng(1000 * k + 10 * R + sys_)
    rest = rng.choice(np.arange(1, k + m - 1), N - 2, replace=False)
    ids = rng.permutation(np.concatenate([[0, k + m - 1], rest]))
    errs = (1, 65536, 32768, None)
    n_multi = 24 if R >= 3 else 0
    P = 8 + 4 * N + n_multi + 8
    frag = oracle_fragments(k, m, sys_, P, rng)[ids]      # (N, P), list order
    cols, exp = [], []
    c = 0
    # 1. clean
    for _ in range(8):
        cols.append(frag[:, c]); exp.append((0, -1, 0)); c += 1
    # 2. a single error at every listed position
    for p in range(N):
        for e in errs:
            y = frag[:, c].copy()
            e = int(rng.integers(1, Q)) if e is None else e
            y[p] = (y[p] + e) % Q
            cols.append(y); exp.append((1, p, int(frag[p, c]))); c += 1
    # 3. 2 .. R - 1 bad fragments
    for t in range(n_multi):
        nb = 2 + t % (R - 2)
        y = frag[:, c].copy()
        for p in rng.choice(N, nb, replace=False):
            y[p] = (y[p] + int(rng.integers(1, Q))) % Q
        cols.append(y); exp.append((2, -1, 0)); c += 1
    # 4. a codeword (a + lam b, by linearity) whose symbol at p is 65536, with
    # the stored symbol wrong: unlocated on a data row, a fix on a coded row
    for t in range(8):
        is_data = (ids < k) if sys_ else np.zeros(N, bool)
        p = int(rng.choice(np.nonzero(is_data if sys_ and t % 2 == 0 else ~is_data)[0]))
        a, b = frag[:, c], frag[:, (c + 1) % P]
        c += 1
        if b[p] == 0:
            continue
        lam = (65536 - a[p]) * pow(int(b[p]), Q - 2, Q) % Q
        cw = (a + lam * b) % Q
        assert cw[p] == 65536
        y = cw.copy()
        y[p] = int(rng.integers(0, 65536))
        data_row = bool(sys_) and ids[p] < k
        cols.append(y); exp.append((2, -1, 0) if data_row else (1, p, 65536))
        cols.append(cw); exp.append((0, -1, 0))
    got = run(exe, sys_, k, m, R, ids, cols)
    exp = np.array(exp, np.int64)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], exp[bad[:5]])
