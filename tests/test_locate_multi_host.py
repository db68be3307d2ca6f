"""CPU: the multi-fragment locate's decoder from the library's host header
(tests/host/test_locate_multi_math.cpp compiles quadiron_amd/csrc/
locate_multi_math.h alone, with -fsanitize=undefined) on columns of the
oracle's encode, both code types:
  (a) codeword columns are clean;
  (b) b = 1 .. t bad fragments, list positions 0 and N - 1 among them, errors
      1, 65536, 32768 and random: exact positions and original symbols;
  (c) b = t + 1 .. R - t bad fragments: always unlocated;
  (d) t = 1: the verdict of locate_classify + locate_fix on every column;
  (e) a crafted codeword with 65536 at one of two error positions: on a data
      row the whole column is unlocated, on a coded row the fix is 65536;
  (f) (3,5), R = 4, t = 2: uniformly random received columns against a brute
      force over all 28 subsets of at most 2 positions.
No case is dropped: the number of columns run is the number planned."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

from qi_testlib import oracle_encode_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
Q = 65537
ERRS = (1, 65536, 32768, None)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    out = str(tmp_path_factory.mktemp("locate_multi") / "test_locate_multi_math")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
        os.path.join(HERE, "host", "test_locate_multi_math.cpp"), "-o", out])
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


def run(exe, sys_, k, m, R, t, ids, cols):
    text = "\n".join(" ".join(str(int(v)) for v in c) for c in cols) + "\n"
    res = subprocess.run([exe, str(sys_), str(k), str(m), str(R), str(t), str(len(ids))] +
                         [str(int(v)) for v in ids], input=text, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert "runtime error" not in res.stderr, res.stderr
    got = np.array([ln.split() for ln in res.stdout.split("\n") if ln], np.int64)
    assert got.shape == (len(cols), 13)
    return got


def located(pairs):
    """expected line of a located column from {position: symbol}"""
    row = [1, len(pairs)]
    for p in sorted(pairs):
        row += [p, pairs[p]]
    return row + [-1, 0] * (4 - len(pairs))


CLEAN = [0, 0] + [-1, 0] * 4
NONE = [2, 0] + [-1, 0] * 4


def pick_ids(k, m, N, rng):
    rest = rng.choice(np.arange(1, k + m - 1), N - 2, replace=False)
    return rng.permutation(np.concatenate([[0, k + m - 1], rest]))


# every (R, t) the code's m allows
SHAPES = [(k, m, R, t) for k, m in [(3, 5), (16, 48), (200, 56), (256, 768)]
          for R, t in [(2, 1), (3, 1), (4, 2), (5, 2), (8, 2), (8, 4)] if R <= m]


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("k,m,R,t", SHAPES)
def test_locate_multi_math_vs_oracle(exe, k, m, R, t, sys_):
    N = k + R
    rng = np.random.default_rng(7000 * k + 100 * R + 10 * t + sys_)
    ids = pick_ids(k, m, N, rng)
    # the position sets of (b): every weight b <= t with list positions 0 and
    # N - 1, both, and random ones
    sets = []
    for b in range(1, t + 1):
        for forced in ([0], [N - 1], [0, N - 1]):
            if len(forced) > b:
                continue
            others = [p for p in range(N) if p not in forced]
            sets.append(forced + [int(p) for p in rng.choice(others, b - len(forced),
                                                             replace=False)])
        for _ in range(6):
            sets.append([int(p) for p in rng.choice(N, b, replace=False)])
    n_b = len(sets) * len(ERRS)
    n_c = 6 * max(0, R - 2 * t)
    n_e = 8 if t >= 2 else 0
    P = 8 + n_b + n_c + n_e + 8
    frag = oracle_fragments(k, m, sys_, P, rng)[ids]      # (N, P), list order
    is_data = (ids < k) if sys_ else np.zeros(N, bool)
    cols, exp = [], []
    c = 0
    for _ in range(8):                                    # (a)
        cols.append(frag[:, c]); exp.append(CLEAN); c += 1
    for ps in sets:                                       # (b)
        for e0 in ERRS:
            y = frag[:, c].copy()
            for a, p in enumerate(ps):
                e = e0 if a == 0 and e0 is not None else int(rng.integers(1, Q))
                y[p] = (y[p] + e) % Q
            cols.append(y)
            exp.append(located({p: int(frag[p, c]) for p in ps}))
            c += 1
    for b in range(t + 1, R - t + 1):                     # (c)
        for _ in range(6):
            y = frag[:, c].copy()
            for p in rng.choice(N, b, replace=False):
                y[p] = (y[p] + int(rng.integers(1, Q))) % Q
            cols.append(y); exp.append(NONE); c += 1
    n_e_run = 0
    for u in range(n_e):                                  # (e)
        want_data = bool(sys_) and u % 2 == 0
        p = int(rng.choice(np.nonzero(is_data if want_data else ~is_data)[0]))
        p2 = int(rng.choice([i for i in range(N) if i != p]))
        a = frag[:, c]
        # a second codeword that is not 0 at p (searched, never skipped)
        b2 = next(frag[:, j] for j in range(P) if j != c and frag[p, j] != 0)
        c += 1
        lam = (65536 - a[p]) * pow(int(b2[p]), Q - 2, Q) % Q
        cw = (a + lam * b2) % Q
        assert cw[p] == 65536
        if is_data[p2] and cw[p2] == 65536:
            p2 = int(np.nonzero(~is_data)[0][0])          # (a coded row can hold it)
            assert p2 != p
        y = cw.copy()
        y[p] = int(rng.integers(0, 65536))
        y[p2] = (y[p2] + int(rng.integers(1, Q))) % Q
        cols.append(y)
        exp.append(NONE if is_data[p] else located({p: 65536, p2: int(cw[p2])}))
        n_e_run += 1
    assert n_e_run == n_e
    assert len(cols) == 8 + n_b + n_c + n_e
    got = run(exe, sys_, k, m, R, t, ids, cols)
    exp = np.array(exp, np.int64)
    bad = np.nonzero((got[:, :10] != exp).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], exp[bad[:5]])
    if t == 1:                                            # (d)
        single = np.stack([got[:, 0], got[:, 2], got[:, 3]], axis=1)
        assert (got[:, 1] == (got[:, 0] == 1)).all()
        bad = np.nonzero((single != got[:, 10:13]).any(axis=1))[0]
        assert bad.size == 0, (bad[:5], got[bad[:5]])


def brute(y, x, w, data_row, R, t):
    """the verdict of one received column by definition: every subset of at
    most t positions, E from the first |subset| syndromes, all R checked"""
    N = len(x)
    S = [sum(int(y[i]) * pow(x[i], j, Q) * pow(w[i], Q - 2, Q) for i in range(N)) % Q
         for j in range(R)]
    if not any(S):
        return CLEAN
    hits = []
    for nu in range(1, t + 1):
        for ps in itertools.combinations(range(N), nu):
            if nu == 1:
                E = [S[0]]
            else:
                x1, x2 = x[ps[0]], x[ps[1]]
                # E1 + E2 = S0, E1 x1 + E2 x2 = S1
                E2 = (S[1] - S[0] * x1) * pow(x2 - x1, Q - 2, Q) % Q
                E = [(S[0] - E2) % Q, E2]
            if any(e == 0 for e in E):
                continue
            if all(sum(e * pow(x[p], j, Q) for e, p in zip(E, ps)) % Q == S[j]
                   for j in range(R)):
                hits.append((ps, E))
    assert len(hits) <= 1          # 2 nu <= R: unique
    if not hits:
        return NONE
    ps, E = hits[0]
    v = {p: (int(y[p]) - e * w[p]) % Q for p, e in zip(ps, E)}
    if any(data_row[p] and v[p] == 65536 for p in ps):
        return NONE
    return located(v)


@pytest.mark.parametrize("sys_", [0, 1])
def test_locate_multi_math_vs_brute_force(exe, sys_):
    """(f): N = 7 listed of the 8 fragments of (3,5), R = 4, t = 2"""
    k, m, R, t = 3, 5, 4, 2
    N = k + R
    rng = np.random.default_rng(4242 + sys_)
    ids = pick_ids(k, m, N, rng)
    r = pow(3, 65536 // 8, Q)
    x = [pow(r, int(f), Q) for f in ids]
    w = []
    for i in range(N):
        v = 1
        for l in range(N):
            if l != i:
                v = v * (x[i] - x[l]) % Q
        w.append(v)
    data_row = [bool(sys_) and f < k for f in ids]
    cols = [rng.integers(0, Q, N) for _ in range(400)]
    # and codewords with 0 .. 3 errors, so that the brute force also says
    # "located" and "clean"
    P = 120
    frag = oracle_fragments(k, m, sys_, P, rng)[ids]
    for c in range(P):
        y = frag[:, c].copy()
        for p in rng.choice(N, c % 4, replace=False):
            y[p] = (y[p] + int(rng.integers(1, Q))) % Q
        cols.append(y)
    exp = np.array([brute(y, x, w, data_row, R, t) for y in cols], np.int64)
    assert (exp[400:, 0] == 1).sum() >= 50 and (exp[400:, 0] == 0).sum() >= 25
    got = run(exe, sys_, k, m, R, t, ids, cols)
    bad = np.nonzero((got[:, :10] != exp).any(axis=1))[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], exp[bad[:5]])
