"""Shared test helpers: ctypes access to the CPU oracle (test infrastructure)
and golden-fixture loading.  Product code never imports this module."""
import ctypes as C
import functools
import glob
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ORACLE_SO = os.path.join(ROOT, "oracle", "liboracle.so")
Q = 65537


class Codec(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ["sys", "k", "m", "code_len", "n_outputs", "n", "data_len",
                 "len_2k"]] + [("r", C.c_uint32)]


_oracle = None


def oracle():
    """Load (building if needed) the plain-C oracle."""
    global _oracle
    if _oracle is None:
        src = os.path.join(ROOT, "oracle", "qi_oracle.c")
        if (not os.path.exists(ORACLE_SO)
                or os.path.getmtime(ORACLE_SO) < os.path.getmtime(src)):
            subprocess.check_call(["make", "-s", "-C",
                                   os.path.join(ROOT, "oracle")])
        lib = C.CDLL(ORACLE_SO)
        for fn in ("qo_add", "qo_sub", "qo_mul", "qo_exp", "qo_inv",
                   "qo_nth_root", "qo_code_len"):
            getattr(lib, fn).restype = C.c_uint32
        lib.qo_ctx_bytes.restype = C.c_size_t
        _oracle = lib
    return _oracle


def ptrs(arrs):
    p = (C.POINTER(C.c_uint8) * len(arrs))()
    for i, a in enumerate(arrs):
        p[i] = (a.ctypes.data_as(C.POINTER(C.c_uint8))
                if a is not None else None)
    return p


def row_ptrs(a, present=None):
    """ptrs() of the rows of one C-contiguous 2-D uint8 array (rows where
    `present` is false: NULL), built from the addresses: a code of 65536 rows
    needs no 65536 ctypes casts.  The caller keeps `a` alive."""
    assert a.dtype == np.uint8 and a.ndim == 2 and a.flags.c_contiguous
    addr = a.ctypes.data + np.arange(a.shape[0], dtype=np.uint64) * np.uint64(a.strides[0])
    if present is not None:
        addr = np.where(np.asarray(present, bool), addr, np.uint64(0))
    return (C.POINTER(C.c_uint8) * a.shape[0]).from_buffer_copy(addr.astype(np.uint64).tobytes())


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def codec(k, m, sys_):
    c = Codec()
    assert oracle().qo_codec_init(C.byref(c), k, m, int(sys_)) == 0
    return c


def ctx_buffer(c):
    """Room for the oracle's qo_ctx of codec c (sized by the oracle itself)."""
    return C.create_string_buffer(oracle().qo_ctx_bytes(C.byref(c)))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"),
                        allow_pickle=False))


def golden_names(prefix):
    return sorted(os.path.basename(p)[:-4]
                  for p in glob.glob(os.path.join(GOLDEN, prefix + "*.npz")))


def check_cabi_scenarios(g, encode, decode, reconstruct):
    """Replay a `cabiscn_*` fixture (tests/golden/gen_golden.py
    `_gen_cabi_scn`): the reference's C-ABI test sequence
    (test/quadiron_c_utest.cpp:109-281) for every stored erasure pattern,
    through the given encode(D, P, wanted, B) / decode(D, P, miss, B) /
    reconstruct(D, P, miss, dest, B) callables (the product's
    quadiron_fnt32_* or the oracle's qo_fnt32_*), on the same mutated
    buffers, comparing every fragment byte for byte: FNT1 headers against
    the reference's, payloads against the data / encoded fragments the
    reference produced."""
    k, m, sys_, B, md = (int(v) for v in g["params"])
    L = md + B
    payload = g["data"][:, md:]
    d = [g["data"][i].copy() for i in range(k)]
    p = [np.zeros(L, np.uint8) for _ in range(m)]
    wanted = np.ones(m if sys_ else k + m, np.int32)
    assert encode(d, p, wanted, B) == 0
    assert (np.stack(d) == g["enc_data"]).all()
    assert (np.stack(p) == g["enc_parity"]).all()
    enc = list(g["enc_data"]) + list(g["enc_parity"])
    r = 0
    for t in range(len(g["missing"])):
        miss = np.ascontiguousarray(g["missing"][t], np.int32)
        gone = np.flatnonzero(miss).tolist()
        D = [g["enc_data"][i].copy() for i in range(k)]
        P = [g["enc_parity"][i].copy() for i in range(m)]
        for i in gone:
            (D + P)[i][:] = 0
        assert decode(D, P, miss, B) == 0, gone
        for i in range(k):
            assert (D[i][:md] == g["decoded_hdr"][t, i]).all(), (gone, i)
            assert (D[i][md:] == payload[i]).all(), (gone, i)
        if not sys_:
            D = [g["enc_data"][i].copy() for i in range(k)]
        for i in gone:
            (D + P)[i][:] = 0
        for dest in sorted(gone):
            assert (g["rec_pat"][r], g["rec_dest"][r]) == (t, dest)
            assert reconstruct(D, P, miss, dest, B) == 0, (gone, dest)
            got = (D + P)[dest]
            assert (got[:md] == g["rec_hdr"][r]).all(), (gone, dest)
            exp = payload[dest] if (sys_ and dest < k) else enc[dest][md:]
            assert (got[md:] == exp).all(), (gone, dest)
            r += 1
    assert r == len(g["rec_dest"])


def oracle_encode_blocks(k, m, sys_, data, cap=None):
    """data: (k, B) uint8 -> outputs (n_outputs, B), oor (n_out, cap), cnt."""
    c = codec(k, m, sys_)
    B = data.shape[1]
    cap = cap or (64 + B // 2048)
    outs = np.zeros((c.n_outputs, B), np.uint8)
    oor = np.zeros((c.n_outputs, cap), np.uint32)
    cnt = np.zeros(c.n_outputs, np.uint32)
    rows = np.ascontiguousarray(data)
    oracle().qo_encode_blocks(C.byref(c), row_ptrs(rows), row_ptrs(outs),
                              C.c_size_t(B), vp(oor), vp(cnt),
                              C.c_uint32(cap))
    return outs, oor, cnt


def oracle_decode_blocks(k, m, sys_, outputs, oor, cnt, missing, data=None):
    """Decode from the encoded outputs with `missing` (code_len flags)."""
    c = codec(k, m, sys_)
    B = outputs.shape[1]
    missing = np.ascontiguousarray(missing, np.int32)
    dec = np.zeros((k, B), np.uint8)
    if sys_ and data is not None:
        have = missing[:k] == 0
        dec[have] = data[have]
    par = np.ascontiguousarray(outputs).copy()
    first = k if sys_ else 0
    wanted = np.ones(k, np.int32)
    ok = oracle().qo_decode_blocks(
        C.byref(c), row_ptrs(dec),
        row_ptrs(par, missing[first:first + c.n_outputs] == 0), vp(oor),
        vp(cnt), C.c_uint32(oor.shape[1]), vp(missing), vp(wanted),
        C.c_size_t(B))
    return ok, dec


def oracle_nf4_encode_blocks(ws, k, m, data, cap):
    """RS-NF4 (oracle): data (k, B) uint8 -> outputs, oor words, flags, cnt."""
    c = codec(k, m, 0)
    B = data.shape[1]
    outs = np.zeros((c.n_outputs, B), np.uint8)
    oor = np.zeros((c.n_outputs, cap), np.uint32)
    flags = np.zeros((c.n_outputs, cap), np.uint32)
    cnt = np.zeros(c.n_outputs, np.uint32)
    rows = [np.ascontiguousarray(data[i]) for i in range(k)]
    oracle().qo_nf4_encode_blocks(C.byref(c), ws, ptrs(rows),
                                  ptrs([outs[i] for i in range(c.n_outputs)]),
                                  C.c_size_t(B), vp(oor), vp(flags), vp(cnt),
                                  C.c_uint32(cap))
    return outs, oor, flags, cnt


def oracle_nf4_decode_blocks(ws, k, m, outputs, oor, flags, cnt, missing):
    c = codec(k, m, 0)
    B = outputs.shape[1]
    dec = [np.zeros(B, np.uint8) for _ in range(k)]
    par = [None if missing[i] else outputs[i].copy()
           for i in range(c.n_outputs)]
    missing = np.ascontiguousarray(missing, np.int32)
    wanted = np.ones(k, np.int32)
    ok = oracle().qo_nf4_decode_blocks(
        C.byref(c), ws, ptrs(dec), ptrs(par), vp(oor), vp(flags), vp(cnt),
        C.c_uint32(oor.shape[1]), vp(missing), vp(wanted), C.c_size_t(B))
    return ok, np.stack(dec)


def craft_oor_columns(k, m, sys_, data_rows, rng, n_cols, rows=None, col_range=None):
    """Force some outputs to 65536 (OOR) by solving for data row 0
    (optionally only on output `rows`, in columns `col_range`)."""
    o = oracle()
    c = codec(k, m, sys_)
    first = k if sys_ else 0
    cw = (C.c_uint32 * c.n)()
    din = (C.c_uint32 * k)()
    ctx = ctx_buffer(c)
    if sys_:
        o.qo_ctx_init(C.byref(c), ctx, (C.c_uint32 * k)(*range(k)))

    def enc(vals):
        for t in range(k):
            din[t] = int(vals[t])
        o.qo_encode_column(C.byref(c), ctx if sys_ else None, din, cw)
        return [cw[first + i] for i in range(c.n_outputs)]

    a = enc([1] + [0] * (k - 1))
    P = data_rows.shape[1]
    lo, hi = col_range if col_range else (0, P)
    for j in lo + rng.choice(hi - lo, min(n_cols, hi - lo), replace=False):
        col = data_rows[:, j].astype(np.int64)
        col[0] = 0
        b = enc(col)
        i = int(rng.choice(rows)) if rows is not None else int(
            rng.integers(0, c.n_outputs))
        if a[i] == 0:
            continue
        d0 = ((65536 - b[i]) % Q) * pow(a[i], Q - 2, Q) % Q
        if d0 < 65536:
            data_rows[0, j] = d0


@functools.lru_cache(maxsize=None)
def retry_block(sys_):
    """The block of the facade's retry tests, computed once per code type and
    read-only: RS(4, 4) on 512 words, whose first-attempt bucket capacity is
    64 + 512 // 512 = 65, with 100 columns of output row r crafted to 65536.
    Returns (data bytes (k, 1024), oracle outputs, oor (n_outputs, 128),
    counts, r, first-attempt capacity)."""
    k, m, words = 4, 4, 512
    rng = np.random.default_rng(4100 + int(sys_))
    lanes = rng.integers(0, 65536, (k, words), dtype=np.uint16)
    r = codec(k, m, sys_).n_outputs - 2   # not among the first k fragments
    craft_oor_columns(k, m, sys_, lanes, rng, 100, rows=[r])
    data = lanes.view(np.uint8).reshape(k, 2 * words)
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, data, cap=128)
    for a in (data, outs, oor, cnt):
        a.setflags(write=False)
    return data, outs, oor, cnt, r, 64 + words // 512


def _solve_mod(A, b):
    """x with A x = b (mod Q) by Gaussian elimination, or None if singular."""
    n = len(A)
    M = [list(A[i]) + [b[i]] for i in range(n)]
    for c in range(n):
        piv = next((r for r in range(c, n) if M[r][c] % Q), None)
        if piv is None:
            return None
        M[c], M[piv] = M[piv], M[c]
        inv = pow(M[c][c], Q - 2, Q)
        M[c] = [v * inv % Q for v in M[c]]
        for r in range(n):
            if r != c and M[r][c]:
                f = M[r][c]
                M[r] = [(vr - f * vc) % Q for vr, vc in zip(M[r], M[c])]
    return [M[i][n] for i in range(n)]


def craft_dense_oor(k, m, data_rows, rng, cols, rows, per_col):
    """Non-systematic: make `per_col` distinct outputs among `rows` equal
    65536 (OOR) in every column of `cols`, by solving for data rows
    0..per_col-1 of that column.  Returns the number of columns crafted."""
    o = oracle()
    c = codec(k, m, 0)
    cw = (C.c_uint32 * c.n)()
    din = (C.c_uint32 * k)()

    def enc(vals):
        for t in range(k):
            din[t] = int(vals[t])
        o.qo_encode_column(C.byref(c), None, din, cw)
        return [cw[i] for i in range(c.n_outputs)]

    G = [enc([1 if t == u else 0 for t in range(k)]) for u in range(per_col)]
    rows = list(rows)
    done = 0
    for j in cols:
        col = data_rows[:, j].astype(np.int64)
        col[:per_col] = 0
        b = enc(col)
        sel = rng.choice(rows, per_col, replace=False)
        A = [[G[u][int(i)] for u in range(per_col)] for i in sel]
        x = _solve_mod(A, [(65536 - b[int(i)]) % Q for i in sel])
        if x is None or any(v == 65536 for v in x):
            continue
        data_rows[:per_col, j] = x
        done += 1
    return done


def chunk_windows(words, chunk=1 << 21, width=4096):
    """Column windows [lo, hi) around the start, every stream-chunk boundary
    and the tail of a `words`-column block."""
    wins = {(0, min(words, width))}
    for c in range(chunk, words, chunk):
        wins.add((max(0, c - width // 2), min(words, c + width // 2)))
        wins.add((c, min(words, c + width)))
    wins.add((max(0, words - width), words))
    return sorted(wins)


def check_windows_vs_oracle(k, m, sys_, data, outs, oor, cnt, wins, missing=None,
                            dec=None):
    """The codes are column-independent, so a large block's outputs (and OOR
    marks, and decode) can be pinned to the oracle window by window: `data`
    (k, 2*words) bytes, `outs` the product's (n_outputs, >= 2*words) coded
    bytes with OOR lists oor/cnt (absolute word offsets)."""
    no = outs.shape[0]
    for lo, hi in wins:
        d = np.ascontiguousarray(data[:, 2 * lo:2 * hi])
        o_out, o_oor, o_cnt = oracle_encode_blocks(k, m, sys_, d, 64 + (hi - lo))
        assert (outs[:, 2 * lo:2 * hi] == o_out).all(), (lo, hi)
        for i in range(no):
            got = [int(w) - lo for w in oor[i, :cnt[i]] if lo <= w < hi]
            assert got == [int(w) for w in o_oor[i, :o_cnt[i]]], (lo, hi, i)
        if missing is not None:
            ok, o_dec = oracle_decode_blocks(k, m, sys_, o_out, o_oor, o_cnt,
                                             missing, d)
            assert ok == 1 and (dec[:, 2 * lo:2 * hi] == o_dec).all(), (lo, hi)


# ------------------------------------------------------------------------
# Inputs at the accumulator extremes.  The codes are linear over GF(65537)
# and their matrices are known, so for any output row the input column that
# drives that row's accumulators as far as valid data can is computed, not
# hoped for (uniform random symbols make the sums a random walk, an order of
# magnitude short of the bounds the kernels' range arguments rest on).

DOT_MODES = ("dot+", "dot-")
MFMA_MODES = ("d2+", "d2-", "d01+", "d01-")
ALL_MODES = DOT_MODES + MFMA_MODES


def balanced_np(M):
    """gf65537.h balanced(): the representative in [-32768, 32768]."""
    M = np.asarray(M, np.int64)
    return np.where(M > 32768, M - Q, M)


def generator_matrix(k, m, sys_):
    """(n_outputs, k) int64, entries 0..65536: column i is the encode of unit
    vector i (systematic: the parity rows, through an encode context over ids
    0..k-1)."""
    o = oracle()
    c = codec(k, m, sys_)
    first = k if sys_ else 0
    cw = (C.c_uint32 * c.n)()
    din = (C.c_uint32 * k)()
    ctx = ctx_buffer(c)
    if sys_:
        assert o.qo_ctx_init(C.byref(c), ctx, (C.c_uint32 * k)(*range(k))) == 0
    G = np.zeros((c.n_outputs, k), np.int64)
    for i in range(k):
        din[i] = 1
        o.qo_encode_column(C.byref(c), ctx if sys_ else None, din, cw)
        din[i] = 0
        G[:, i] = np.frombuffer(cw, np.uint32)[first:first + c.n_outputs]
    return G


def decode_matrix(k, m, sys_, ids):
    """(k, k) int64: column i is the decode of unit vector i received at
    ids[i].  Column by column, not through the block API: that stores u16
    and loses the entries equal to 65536."""
    o = oracle()
    c = codec(k, m, sys_)
    ctx = ctx_buffer(c)
    assert o.qo_ctx_init(C.byref(c), ctx,
                         (C.c_uint32 * k)(*[int(v) for v in ids])) == 0
    win = (C.c_uint32 * k)()
    dout = (C.c_uint32 * k)()
    M = np.zeros((k, k), np.int64)
    for i in range(k):
        win[i] = 1
        o.qo_decode_column(C.byref(c), ctx, win, dout)
        win[i] = 0
        M[:, i] = np.frombuffer(dout, np.uint32)
    return M


def matvec_mod(M, X):
    """M @ X mod q for entries 0..65536, exact: every partial sum is an
    integer below 2^33 * rows < 2^53, so the float64 product is exact."""
    assert M.shape[1] < (1 << 19)
    Y = np.asarray(M, np.float64) @ np.asarray(X, np.float64)
    return Y.astype(np.int64) % Q


def repair_matrix(k, m, sys_, ids, targets):
    """(R, k) int64, entries 0..65536: row j rebuilds fragment targets[j]
    from the symbols received at `ids` -- the rows `targets` of the full
    generator (systematic: the k identity rows on top of the parity rows)
    times decode_matrix(ids).  What repair_ctx_kernel builds on the device."""
    G = generator_matrix(k, m, sys_)
    if sys_:
        G = np.concatenate([np.eye(k, dtype=np.int64), G])
    return matvec_mod(G[np.asarray(targets, np.int64)], decode_matrix(k, m, sys_, ids))


def split_i8_np(M):
    """matrix_pack.h split_i8: canonical c -> (a, b) in [-128, 127] with
    c = 256 a + b mod q (every residue but balanced 32640)."""
    v = balanced_np(M)
    v = np.where(v > 32639, v - Q, v)
    b = ((v + 128) & 255) - 128
    a = (v - b) // 256
    return a, b


def coef_ok_np(M):
    v = balanced_np(M)
    return (np.abs(v) <= 32766) & (v != 32640)


def row_scale(row):
    """pack_row's search: the smallest s >= 2 whose inverse is within
    |s^-1| <= 32766 and that makes every s * row entry coef_ok (1: the row
    needs no scale)."""
    row = np.asarray(row, np.int64)
    if coef_ok_np(row).all():
        return 1
    s = 1
    while True:
        s += 1
        si = pow(s, Q - 2, Q)
        if abs(si - Q if si > 32768 else si) > 32766:
            continue
        if coef_ok_np(row * s % Q).all():
            return s


def extreme_targets(M, n_spread=8, max_scaled=48):
    """[(row, s)]: every row that needs a row scale (at most max_scaled), raw
    (s = 1) and scaled, then n_spread rows spread evenly over the matrix --
    row 0 and the last row (of the last 16-row block) among them."""
    R = M.shape[0]
    need = np.flatnonzero(~coef_ok_np(M).all(axis=1))[:max_scaled]
    tg = []
    for t in need:
        tg += [(int(t), 1), (int(t), row_scale(M[t]))]
    for t in sorted(set(np.linspace(0, R - 1, min(n_spread, R)).round().astype(int))):
        tg.append((int(t), 1))
    return tg


def craft_column(row, mode):
    """One input column (values 0..65535) that drives the accumulators of
    the output whose canonical coefficients are `row` to the `mode` extreme:
      dot+-  x = 65535 where balanced(c) > 0 else 0 (negated: swapped): every
             v_dot2 step and every butterfly sum feeding the output adds in
             one direction, sum c (x - 32768) = +-sum |c| w, w in {32767, 32768}
      d2+-   bytes h' = 127 where b > 0 else -128, l' = 127 where a > 0 else
             -128 (c = 256 a + b): |D2| = sum |b| w_h + |a| w_l, w in {127, 128}
      d01+-  h' follows the sign of a, l' that of b: |D0| and |D1| together
    x = 256 h' + l' + 32896 is a valid u16 for every byte pair."""
    row = np.asarray(row, np.int64)
    neg = mode.endswith("-")
    if mode.startswith("dot"):
        pos = balanced_np(row) > 0
        return np.where(pos ^ neg, 65535, 0).astype(np.int64)
    a, b = split_i8_np(row)
    ch, cl = (b, a) if mode.startswith("d2") else (a, b)
    h = np.where((ch > 0) ^ neg, 127, -128)
    l = np.where((cl > 0) ^ neg, 127, -128)
    return (256 * h + l + 32896).astype(np.int64)


def craft_columns(M, targets, modes, cols):
    """(k, cols) int64 columns, one per (target, mode) pair, cycling through
    the pairs; `targets` as extreme_targets gives them (a scaled target is
    crafted against s * row).  Round r gives target i the mode i + r, so a
    prefix shorter than all pairs still holds every target and every mode.
    Returns (X, meta), meta[j] = (row, s, mode) of column j."""
    pairs = [(t, s, modes[(i + r) % len(modes)])
             for r in range(len(modes)) for i, (t, s) in enumerate(targets)]
    X = np.zeros((M.shape[1], cols), np.int64)
    meta = []
    for j in range(cols):
        t, s, mode = pairs[j % len(pairs)]
        X[:, j] = craft_column(M[t] * s % Q, mode)
        meta.append((t, s, mode))
    return X, meta


def model_sums(row, X):
    """The kernels' integer sums for one output row over the columns of X
    (k, n), before any fold: the dot2 sum of c (x - 32768) with balanced c,
    and the matrix cores' D0 = sum a h', D1 = sum b l', D2 = sum (b h' + a l')
    over the byte planes h' = (x >> 8) - 128, l' = (x & 255) - 128."""
    row = np.asarray(row, np.int64)
    X = np.asarray(X, np.int64)
    a, b = split_i8_np(row)
    h = (X >> 8) - 128
    l = (X & 255) - 128
    return {"dot": balanced_np(row) @ (X - 32768),
            "d0": a @ h, "d1": b @ l, "d2": b @ h + a @ l}


def closed_form(row, mode):
    """What craft_column(row, mode) must reach: {sum name: value}."""
    row = np.asarray(row, np.int64)
    sg = -1 if mode.endswith("-") else 1

    def l1(c, wpos, wneg):
        c = sg * c
        return sg * int((np.where(c > 0, c * wpos, 0) - np.where(c < 0, c * wneg, 0)).sum())
    if mode.startswith("dot"):
        return {"dot": l1(balanced_np(row), 32767, 32768)}
    a, b = split_i8_np(row)
    if mode.startswith("d2"):
        return {"d2": l1(b, 127, 128) + l1(a, 127, 128)}
    return {"d0": l1(a, 127, 128), "d1": l1(b, 127, 128)}


_PATTERN_PLANES = (0x0000, 0xFFFF, 0x8000, 0x7FFF, 0x8080, 0x7F7F, 0x807F, 0x7F80)


def pattern_rows(k, P):
    """(k, P) uint16: column j holds pattern j mod 10 down its k rows -- the
    constant planes 0x0000, 0xFFFF, 0x8000, 0x7FFF, 0x8080, 0x7F7F, 0x807F,
    0x7F80 (the ends of the u16 range and of both byte planes), 0x0000 /
    0xFFFF alternating by row parity, and by row index mod 32 < 16."""
    i = np.arange(k)[:, None]
    j = np.arange(P)[None, :] % (len(_PATTERN_PLANES) + 2)
    X = np.asarray(_PATTERN_PLANES + (0, 0), np.int64)[j] + 0 * i
    X = np.where(j == 8, np.where(i % 2 == 0, 0x0000, 0xFFFF), X)
    X = np.where(j == 9, np.where(i % 32 < 16, 0x0000, 0xFFFF), X)
    return X.astype(np.uint16)


def craft_received(k, m, sys_, ids, cols, rng, n_spread=8, against=None, no_mark_rows=(),
                   extra_marks=None):
    """Decode-side extremes inside valid use: received symbols r crafted
    against decode_matrix(ids) (every 8th column with its one to three
    largest-|c| entries at 65536, the true maximum of a received symbol,
    which arrives as an OOR mark; systematic: parity positions only, data
    rows carry no marks), d = M r mod q their data.  A column whose data
    holds a 65536 is not representable and is replaced by random data.

    against: an (R, k) matrix over the same received positions (a
    repair_matrix of the ids) whose rows the symbols are crafted against
    instead; d still comes from the decode matrix.  Then, besides,
      - extra_marks, a (k, cols) bool mask of markable positions, are
        received 65536 values on top of the crafted ones;
      - column 4 + 8 n is crafted for the n-th (target, mode) pair over the
        targets outside no_mark_rows (the rows whose output cannot be 65536:
        a systematic code's data rows), in craft_columns' order, and then one
        of its symbols is solved so that this target's output A[t] r is
        exactly 65536: the one at the markable position with the smallest
        non-zero |balanced c| in the row crafted against (a solved 65536 is
        an input mark there, which a markable position can carry).  The other
        k - 1 symbols keep their extreme values, so the output mark sits in a
        column within one term of the bound.
    Returns (d (k, cols) uint16, r (k, cols) int64 as received, kept (cols)
    bool, M, meta, solved (cols) int64: the solved position, -1 in a column
    not altered)."""
    ids = np.asarray(ids, np.int64)
    M = decode_matrix(k, m, sys_, ids)
    A = M if against is None else np.asarray(against, np.int64)
    tg = extreme_targets(A, n_spread)
    r, meta = craft_columns(A, tg, ALL_MODES, cols)
    markable = np.flatnonzero(ids >= k) if sys_ else np.arange(k)
    for n, j in enumerate(range(0, cols, 8)):
        t, s, _ = meta[j]
        mag = np.abs(balanced_np(A[t] * s % Q))[markable]
        top = markable[np.argsort(-mag, kind="stable")[:1 + n % 3]]
        r[top, j] = 65536
    solved = np.full(cols, -1, np.int64)
    if against is not None:
        if extra_marks is not None:
            assert not np.delete(extra_marks, markable, axis=0).any()
            r[extra_marks] = 65536
        out_tg = [(t, s) for t, s in tg if t not in no_mark_rows]
        for n, j in enumerate(range(4, cols, 8) if out_tg and len(markable) else ()):
            i = n % len(out_tg)
            t, s = out_tg[i]
            mode = ALL_MODES[(i + n // len(out_tg)) % len(ALL_MODES)]
            row = A[t] * s % Q
            col = np.where(r[:, j] == 65536, 65536, craft_column(row, mode))
            meta[j] = (t, s, mode)
            mag = np.abs(balanced_np(row))[markable]
            for p in markable[np.argsort(mag, kind="stable")]:
                if row[p] == 0 or col[p] == 65536:
                    continue
                rest = int(A[t] @ col) - int(A[t, p] * col[p])
                col[p] = (65536 - rest) % Q * pow(int(A[t, p]), Q - 2, Q) % Q
                solved[j] = p
                break
            r[:, j] = col
    d = matvec_mod(M, r)
    kept = (d < 65536).all(axis=0)
    nrep = int((~kept).sum())
    if nrep:
        d[:, ~kept] = rng.integers(0, 65536, (k, nrep))
    return d.astype(np.uint16), r, kept, M, meta, solved


@functools.lru_cache(maxsize=None)
def repair_case(k, m, sys_, R, need_scale=False):
    """A seeded repair of R fragments: (ids (k) ascending, targets (R) in
    seeded order, their repair_matrix), read-only.  Systematic: the targets
    hold data and parity rows (min(k, R) // 2 data rows) and the ids both
    regions.  need_scale: the first seed whose matrix has a row that needs
    pack_row's scale (five residues are not coef_ok, so a row of k entries
    needs one with probability about 5 k / 65537)."""
    n = k + m
    for seed in range(200):
        rng = np.random.default_rng([k, m, sys_, R, seed])
        if sys_ and R >= 2:
            a = min(k, R) // 2
            tg = np.concatenate([rng.choice(k, a, replace=False),
                                 k + rng.choice(m, R - a, replace=False)])
        else:
            tg = rng.choice(n, R, replace=False)
        tg = rng.permutation(tg)
        ids = np.sort(rng.choice(np.setdiff1d(np.arange(n), tg), k, replace=False))
        if sys_ and not ((ids < k).any() and (ids >= k).any()):
            continue
        M = repair_matrix(k, m, sys_, ids, tg)
        if need_scale and coef_ok_np(M).all():
            continue
        for a in (ids, tg, M):
            a.setflags(write=False)
        return ids, tg, M
    raise AssertionError("no seed gives such a repair")


class CraftedRepair:
    """repair_case(k, m, sys, R) and the `cols` columns craft_received crafts
    against its matrix A (read-only; one per shape, shared by the tests):
    ids, targets, A, d, r, kept, meta, solved as craft_received returns them,
    data_rows (the rows of A that rebuild a systematic data row) and y = A r,
    the rebuilt symbols in 0..65536.  dense: the first `dense` columns carry
    one more received 65536 each, at a seeded markable position."""

    def __init__(self, k, m, sys_, R, cols, dense=0):
        self.ids, self.targets, self.A = repair_case(k, m, sys_, R, R >= 32 and k >= 64)
        self.data_rows = tuple(np.flatnonzero(self.targets < k)) if sys_ else ()
        rng = np.random.default_rng([k, m, sys_, R, cols, dense])
        extra = None
        if dense:
            markable = np.flatnonzero(self.ids >= k) if sys_ else np.arange(k)
            extra = np.zeros((k, cols), bool)
            extra[rng.choice(markable, dense), np.arange(dense)] = True
        self.d, self.r, self.kept, _, self.meta, self.solved = craft_received(
            k, m, sys_, self.ids, cols, rng, against=self.A, no_mark_rows=self.data_rows,
            extra_marks=extra)
        self.y = matvec_mod(self.A, self.r)
        self.share = 1 - self.kept.mean()
        for a in (self.d, self.r, self.kept, self.solved, self.y):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def crafted_repair(k, m, sys_, R, cols, dense=0):
    return CraftedRepair(k, m, sys_, R, cols, dense)


# ------------------------------------------------------------------------
# Wide row layouts.  A [S, rows, P] tensor of the device C-ABI may have any
# positive strides; in a fragment-major layout (every fragment holds all its
# stripes back to back: stripe stride P, row stride >= S * P) a stripe's row
# region can span GiB, and the library then leaves the buffer-resource
# kernels for the flat ones.

FILL = 0x5A5A   # the word of a backing wherever no row lives


def row_extent(rows, rs, words):
    """The library's rule (row_extent, quadiron_amd/csrc/matrix_route.h;
    tests/golden/row_extent.txt pins both): the byte extent of `rows` rows of
    `words` u16 at row stride rs, 0 when it does not fit a 31-bit buffer
    range -- then every kernel of the launch is a flat one."""
    if rows <= 0:
        return 0
    e = ((rows - 1) * rs + words) * 2
    return e if 0 < e < 0x7fffffff else 0


def strided_rows(S, rows, P, rs, ss):
    """(backing, view): a 1-D int16 device tensor of (rows - 1) * rs +
    (S - 1) * ss + P words filled with FILL, and its [S, rows, P] view with
    strides (ss, rs, 1).  The backing covers the region from word 0 on, so
    an offset that lost its upper bits still lands inside the allocation."""
    import torch
    n = (rows - 1) * rs + (S - 1) * ss + P
    backing = torch.full((n,), FILL, dtype=torch.int16, device="cuda")
    return backing, torch.as_strided(backing, (S, rows, P), (ss, rs, 1))


def backing_is_fill(backing, chunk=1 << 27):
    """Whether every word of the backing is FILL, compared on the device in
    chunks (temporaries of 128 MiB)."""
    import torch
    bad = torch.zeros((), dtype=torch.bool, device=backing.device)
    for lo in range(0, backing.numel(), chunk):
        bad |= (backing[lo:lo + chunk] != FILL).any()
    return not bool(bad.item())


def wide_rs(cls, rows, P):
    """The smallest row stride (u16 words, a multiple of 4) that puts `rows`
    rows of P words into a region class:
      N   narrow: two stripes side by side, rs = 2 P
      B   the top of the buffer range: extent within 4096 bytes below 2^31 - 1
          (or within one stride step, 8 (rows - 1) bytes, where that is more)
      F2  extent in [2^31, 2^31 + 2^20): flat kernels, row offsets below 4 GiB
      F4  (rows - 1) * rs * 2 >= 2^32 + 2^28: flat, the upper rows past 4 GiB
          (rows = 2: the row stride itself past 2^32 bytes)
    and the extent the library must see for it (asserted)."""
    assert rows >= 2 or cls == "N", "one row cannot be wide"
    up4 = lambda v: -(-v // 4) * 4
    if cls == "N":
        rs = up4(2 * P)
        assert row_extent(rows, rs, P) != 0
        return rs
    if cls == "B":
        rs = up4(-(-((1 << 31) - 1 - 4096 - 2 * P) // (2 * (rows - 1))))
        if ((rows - 1) * rs + P) * 2 >= (1 << 31) - 1:
            # a step of 4 words moves the extent by 8 (rows - 1) bytes: past
            # 513 rows a stride can jump the 4096-byte window; then the
            # largest stride below the limit, as close as the layout gets
            rs -= 4
        e = ((rows - 1) * rs + P) * 2
        assert (1 << 31) - 1 - max(4096, 8 * (rows - 1)) <= e < (1 << 31) - 1, (rows, P, e)
        assert row_extent(rows, rs, P) == e
    elif cls == "F2":
        rs = up4(-(-((1 << 31) - 2 * P) // (2 * (rows - 1))))
        e = ((rows - 1) * rs + P) * 2
        assert (1 << 31) <= e < (1 << 31) + (1 << 20), (rows, P, e)
        assert row_extent(rows, rs, P) == 0
    else:
        assert cls == "F4"
        rs = up4(-(-((1 << 32) + (1 << 28)) // (2 * (rows - 1))))
        assert (rows - 1) * rs * 2 >= (1 << 32) + (1 << 28)
        assert row_extent(rows, rs, P) == 0
    return rs
