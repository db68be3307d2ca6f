"""The extreme-input builders of qi_testlib are what they claim to be,
independent of any kernel (CPU only: numpy and the oracle).

tests/test_gpu_extremes.py feeds the kernels columns crafted from the codes'
own matrices; this module pins those matrices to the oracle, the crafted
columns to their closed forms, and shows that they reach further than the
same number of uniform random columns do."""
import functools

import numpy as np
import pytest

from qi_testlib import (ALL_MODES, Q, balanced_np, closed_form, coef_ok_np, craft_column,
                        craft_columns, craft_oor_columns, craft_received, crafted_repair,
                        decode_matrix, extreme_targets, generator_matrix, matvec_mod,
                        model_sums, oracle_encode_blocks, pattern_rows, row_scale,
                        split_i8_np)

SHAPES = [(16, 48, 0), (100, 50, 1), (200, 56, 0), (640, 384, 0)]
COLS = 512


def _ids(k, m, seed):
    return np.sort(np.random.default_rng(seed).choice(k + m, k, replace=False))


@functools.lru_cache(maxsize=None)
def _gen(k, m, sys_):
    G = generator_matrix(k, m, sys_)
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def _dec(k, m, sys_):
    ids = _ids(k, m, 100 * k + m)
    M = decode_matrix(k, m, sys_, ids)
    M.setflags(write=False)
    return ids, M


@pytest.mark.parametrize("k,m,sys_", SHAPES)
def test_generator_matrix_is_the_oracle_encode(k, m, sys_):
    G = _gen(k, m, sys_)
    assert G.shape == ((m if sys_ else k + m), k) and G.min() >= 0 and G.max() <= 65536
    rng = np.random.default_rng(k + m)
    P = 96
    data = rng.integers(0, 65536, (k, P), dtype=np.uint16)
    craft_oor_columns(k, m, sys_, data, rng, 24)
    y = matvec_mod(G, data)
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, data.view(np.uint8).reshape(k, 2 * P), P)
    assert (outs.view(np.uint16) == (y & 0xFFFF)).all()
    assert (y == 65536).sum() > 0
    for i in range(G.shape[0]):
        assert oor[i, :cnt[i]].tolist() == np.flatnonzero(y[i] == 65536).tolist()


@pytest.mark.parametrize("k,m,sys_", SHAPES)
def test_decode_matrix_inverts_the_code(k, m, sys_):
    ids, M = _dec(k, m, sys_)
    assert M.shape == (k, k) and M.min() >= 0 and M.max() <= 65536
    rng = np.random.default_rng(3 * k + m)
    data = rng.integers(0, 65536, (k, 64), dtype=np.uint16).astype(np.int64)
    y = matvec_mod(_gen(k, m, sys_), data)
    cw = np.concatenate([data, y]) if sys_ else y
    assert (matvec_mod(M, cw[ids]) == data).all()


def test_split_i8_np_spans_every_residue_but_one():
    c = np.arange(Q)
    a, b = split_i8_np(c)
    ok = balanced_np(c) != 32640
    assert (np.abs(np.stack([a, b]) + 0.5) <= 127.5)[:, ok].all()
    assert ((256 * a + b - c) % Q == 0)[ok].all()


@pytest.mark.parametrize("k,m,sys_", SHAPES)
def test_row_scale_postconditions(k, m, sys_):
    """pack_row's search restated: every scaled entry coef_ok, |s^-1| <=
    32766, and no smaller s >= 2 with both."""
    def good(row, s):
        si = pow(s, Q - 2, Q)
        return abs(int(balanced_np(si))) <= 32766 and coef_ok_np(row * s % Q).all()
    seen = 0
    for M in (_gen(k, m, sys_), _dec(k, m, sys_)[1]):
        need = ~coef_ok_np(M).all(axis=1)
        for t in np.flatnonzero(need)[:48]:
            s = row_scale(M[t])
            assert s >= 2 and good(M[t], s)
            assert not any(good(M[t], u) for u in range(2, s))
            seen += 1
        for t in np.flatnonzero(~need)[:4]:
            assert row_scale(M[t]) == 1
    # the forced residues (the ones test_codelets.cpp plants) need a scale
    row = np.array([32767, 5, 32640, 65536 - 32767, 1])
    s = row_scale(row)
    assert s >= 2 and good(row, s) and not any(good(row, u) for u in range(2, s))
    print(f"\n({k},{m},{sys_}): {seen} rows needing a scale checked")


def _matrices(k, m, sys_):
    return (("generator", _gen(k, m, sys_)), ("decode", _dec(k, m, sys_)[1]))


def _magnitude(sums, mode):
    if mode.startswith("dot"):
        return np.abs(sums["dot"])
    if mode.startswith("d2"):
        return np.abs(sums["d2"])
    return np.abs(sums["d0"]) + np.abs(sums["d1"])


@pytest.mark.parametrize("k,m,sys_", SHAPES)
def test_crafted_columns_reach_their_closed_forms(k, m, sys_):
    """Every crafted column: a valid u16 column whose modelled sums on its
    target row equal the closed forms sum |c| w exactly, and whose magnitude
    is strictly above the maximum over as many seeded uniform random columns
    (d01: |D0| + |D1|).  A target row with fewer than four non-zero
    coefficients (the unit rows of a systematic decode) has so few byte
    combinations that random symbols reach its extreme too (and the "+"
    modes' 127 gives way to a random -128): there only the closed form is
    checked."""
    for name, M in _matrices(k, m, sys_):
        tg = extreme_targets(M)
        assert tg[-1][0] == M.shape[0] - 1 and (0, 1) in tg
        assert all(s == 1 or s == row_scale(M[t]) for t, s in tg)
        X, meta = craft_columns(M, tg, ALL_MODES, COLS)
        assert X.shape == (k, COLS) and X.min() >= 0 and X.max() <= 65535
        assert {(t, s) for t, s, _ in meta} == set(tg) or len(tg) * 6 > COLS
        assert {mo for _, _, mo in meta} == set(ALL_MODES)
        rnd = np.random.default_rng(k).integers(0, 65536, (k, COLS))
        best, rsums = {}, {}
        for j, (t, s, mode) in enumerate(meta):
            row = M[t] * s % Q
            sums = model_sums(row, X[:, j:j + 1])
            for key, want in closed_form(row, mode).items():
                assert int(sums[key][0]) == want, (name, t, s, mode, key)
                assert (want >= 0) == mode.endswith("+") or want == 0
            mag = int(_magnitude(sums, mode)[0])
            if (t, s) not in rsums:
                rsums[t, s] = model_sums(row, rnd)
            rmax = int(_magnitude(rsums[t, s], mode).max())
            if np.count_nonzero(row) >= 4:
                assert mag > rmax, (name, t, s, mode, mag, rmax)
            fam = mode[:-1]
            if mag > best.get(fam, (0, 0))[0]:
                best[fam] = (mag, rmax)
        print(f"\n({k},{m},{sys_}) {name}: crafted vs random max "
              + ", ".join(f"{f} {c} vs {r}" for f, (c, r) in sorted(best.items())))


@pytest.mark.parametrize("k,m,sys_", SHAPES + [(1000, 24, 0)])
def test_decode_side_construction_keeps_its_columns(k, m, sys_):
    """craft_received replaces at most 5 % of its columns (a column is lost
    when its data holds a 65536); the kept ones decode to valid data, carry
    marks, and hold the crafted received symbols."""
    rng = np.random.default_rng(k + 7)
    ids = _ids(k, m, 100 * k + m)
    d, r, kept, M, meta, solved = craft_received(k, m, sys_, ids, COLS, rng)
    assert (solved == -1).all()
    share = 1 - kept.mean()
    print(f"\n({k},{m},{sys_}): {100 * share:.1f} % of {COLS} columns replaced, "
          f"{int((r[:, kept] == 65536).sum())} marks kept")
    assert share <= 0.05
    assert (matvec_mod(M, r)[:, kept] == d[:, kept]).all()
    assert (r[:, kept] == 65536).sum() > 0
    cw = matvec_mod(_gen(k, m, sys_), d)
    cw = np.concatenate([d.astype(np.int64), cw]) if sys_ else cw
    assert (cw[ids][:, kept] == r[:, kept]).all()


# k, m, sys, R: the repairs tests/test_gpu_extremes.py runs (R = min(64, m),
# and at k = 256 one live row in the first and in a second 16-row block)
REPAIR_SHAPES = [(16, 48, 0, 48), (32, 32, 0, 32), (64, 960, 0, 64), (128, 128, 0, 64),
                 (256, 768, 0, 64), (256, 768, 0, 1), (256, 768, 0, 17),
                 (16, 48, 1, 48), (100, 50, 1, 50), (200, 56, 1, 56)]


def _target_rows(k, m, sys_, c, cols):
    """The oracle's encode of c.d on the target rows: per target its symbols
    (cols) u16 and its marks (a data target: the data row, no marks)."""
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, c.d.view(np.uint8).reshape(k, 2 * cols),
                                          cols)
    outs = outs.view(np.uint16)
    for t in c.targets:
        if sys_ and t < k:
            yield c.d[t], []
        else:
            sl = t - k if sys_ else t
            yield outs[sl], oor[sl, :cnt[sl]].tolist()


@pytest.mark.parametrize("k,m,sys_,R", REPAIR_SHAPES)
def test_repair_side_construction(k, m, sys_, R):
    """craft_received against a repair matrix A (qi_testlib crafted_repair):
      - A is the oracle's: A r mod q equals the oracle's encode of the decoded
        data on the target rows, symbols and marks, on every kept column;
      - a crafted column without a mark that was not altered reaches the
        closed form on the raw or scaled row it was crafted against, exactly;
      - a column altered for an output mark does so once its solved symbol is
        put back, and as it stands is within the replaced term of it: two
        values of c (x - 32768) differ by at most 65536 |c|; two values of a
        byte-plane term, h' and l' in [-128, 127], by at most 255 |coefficient|
        (D0: a, D1: b, D2: both), bounded here by 2 * 128 (|a| + |b|), twice
        the largest single term (compared where the solved symbol is no mark:
        a 65536 has no byte planes);
      - at most 5 % of the columns are replaced, and every crafted target that
        can hold one has an output mark in a kept column."""
    c = crafted_repair(k, m, sys_, R, COLS)
    A, r = c.A, c.r
    assert A.shape == (R, k) and A.min() >= 0 and A.max() <= 65536
    assert (r[:, c.kept] == 65536).sum() > 0
    assert c.share <= 0.05
    cols = np.flatnonzero(c.kept)
    for j, (exp, marks) in enumerate(_target_rows(k, m, sys_, c, COLS)):
        assert ((c.y[j, cols] & 0xFFFF) == exp[cols]).all(), j
        assert [w for w in marks if c.kept[w]] == cols[c.y[j, cols] == 65536].tolist(), j
    top = {"dot": 0, "d2": 0, "d0": 0, "d1": 0}
    n_altered = 0
    for j, (t, s, mode) in enumerate(c.meta):
        row = A[t] * s % Q
        col = r[:, j].copy()
        p = c.solved[j]
        if p >= 0:
            n_altered += 1
            assert j % 8 == 4 and t not in c.data_rows and c.y[t, j] == 65536
            col[p] = craft_column(row, mode)[p]
        else:
            assert j % 8 != 4 or len(c.data_rows) == R
        if (col == 65536).any():
            assert j % 8 == 0
            continue
        want = closed_form(row, mode)
        sums = model_sums(row, col[:, None])
        for key, w in want.items():
            assert int(sums[key][0]) == w, (j, t, s, mode, key)
            top[key] = max(top[key], abs(w))
        if p >= 0 and r[p, j] < 65536:
            a, b = (abs(int(v[p])) for v in split_i8_np(row))
            bound = 65536 * abs(int(balanced_np(row)[p])) if mode.startswith("dot") \
                else 2 * 128 * (a + b)
            got = model_sums(row, r[:, j:j + 1])
            for key, w in want.items():
                assert abs(int(got[key][0]) - w) <= bound, (j, t, s, mode, key)
    assert n_altered == len(range(4, COLS, 8))
    for t in {t for t, _ in extreme_targets(A)} - set(c.data_rows):
        hit = [j for j in cols if c.solved[j] >= 0 and c.meta[j][0] == t]
        assert hit and (c.y[t, hit] == 65536).all(), t
    need = np.flatnonzero(~coef_ok_np(A).all(axis=1))
    print(f"\n({k},{m},{sys_}) R={R}: {100 * c.share:.1f} % of {COLS} columns replaced, "
          f"{len(need)} rows need a scale, max |dot| {top['dot']}, |D2| {top['d2']}, "
          f"|D0| {top['d0']}, |D1| {top['d1']}")


@pytest.mark.parametrize("k,m", [(256, 768), (64, 960)])
def test_repair_matrix_rows_that_need_a_scale(k, m):
    """The 64-row repair matrices of these codes hold rows that pack_row must
    scale, and row_scale finds their scale."""
    A = crafted_repair(k, m, 0, 64, COLS).A
    need = np.flatnonzero(~coef_ok_np(A).all(axis=1))
    assert len(need) >= 1
    tg = extreme_targets(A)
    for t in need:
        s = row_scale(A[t])
        assert s >= 2 and coef_ok_np(A[t] * s % Q).all()
        assert abs(int(balanced_np(pow(s, Q - 2, Q)))) <= 32766
        assert (int(t), 1) in tg and (int(t), s) in tg


def test_pattern_rows():
    X = pattern_rows(70, 50)
    assert X.dtype == np.uint16 and X.shape == (70, 50)
    for j, v in enumerate((0x0000, 0xFFFF, 0x8000, 0x7FFF, 0x8080, 0x7F7F, 0x807F, 0x7F80)):
        assert (X[:, [j, j + 10, j + 40]] == v).all()
    assert X[:, 8].tolist() == [0, 0xFFFF] * 35 and (X[:, 18] == X[:, 8]).all()
    assert X[:, 9].tolist() == ([0] * 16 + [0xFFFF] * 16) * 2 + [0] * 6
    assert (craft_column(np.array([1, 65536, 0]), "dot+") == [65535, 0, 0]).all()
