"""GPU: syndrome shares (qi_gpu_syndrome_ctx / qi_gpu_syndrome,
qi_gpu_syndrome_locate_ctx / qi_gpu_syndrome_locate, Fec.syndrome_blocks,
locate_syndromes, apply_deltas, scrub_blocks).  The stripes are the oracle's
encodes.  The expected syndromes are Python-integer sums e x_p^j / w_p over the
injected errors, the expected decisions those of a brute-force decoder over
every set of at most t positions, or known by construction from the injected
errors; below k = 256 the results are also compared with qi_gpu_locate_multi.
Nothing expected here comes from the code under test."""
import functools
import itertools

import numpy as np
import pytest

from qi_testlib import FILL, Q, craft_oor_columns, matvec_mod, oracle_encode_blocks
from test_gpu_partial import (_buckets, _dev16, _guards_intact, _read_buckets, _rows_dev,
                              _torch)

pytestmark = pytest.mark.gpu

CAP = 256
TILE = 2048      # the kernels' column tile
RAGGED = TILE + 9
MARK = 65536
S = 2

# (k, m, sys, width, unaligned): the ragged tile edge on the symbol-by-symbol
# path, whole tiles at 16-byte alignment on the 16-byte path, and an odd base
SHAPES = [(3, 5, 0, RAGGED, False), (16, 48, 0, TILE, False), (200, 56, 0, RAGGED, True),
          (260, 30, 1, TILE, False), (300, 212, 0, RAGGED, False), (1100, 100, 0, RAGGED, False)]


# ---- the code in Python integers -------------------------------------------

def _root(k, m):
    n = 1
    while n < k + m:
        n *= 2
    return pow(3, 65536 // n, Q)


def _points(k, m, ids):
    """(x [N], w [N]) int64: x_i = r^ids[i], w_i = prod_{l != i} (x_i - x_l)"""
    r = _root(k, m)
    x = np.array([pow(r, int(f), Q) for f in ids], np.int64)
    w = np.ones(len(x), np.int64)
    for l in range(len(x)):
        d = (x - x[l]) % Q
        d[l] = 1
        w = w * d % Q
    assert (w != 0).all()
    return x, w


@functools.lru_cache(maxsize=None)
def _truth(k, m, sys_, P):
    """S oracle-encoded stripes as restored symbols by fragment id, int64
    [S, k + m, P] (65536 where the encode marked), with marks crafted on some
    coded rows; shared and never written"""
    rng = np.random.default_rng([k, m, sys_, P, 11])
    out = []
    for _ in range(S):
        data = rng.integers(0, 65536, (k, P), dtype=np.uint16)
        craft_oor_columns(k, m, sys_, data, rng, 24)
        o, oor, cnt = oracle_encode_blocks(
            k, m, sys_, np.ascontiguousarray(data).view(np.uint8).reshape(k, 2 * P), CAP)
        assert cnt.max() <= CAP
        coded = o.view(np.uint16).reshape(-1, P)[:(m if sys_ else k + m)].astype(np.int64)
        for j in range(coded.shape[0]):
            cols = oor[j, :cnt[j]]
            assert (coded[j, cols] == 0).all()
            coded[j, cols] = MARK
        out.append(np.concatenate([data.astype(np.int64), coded]) if sys_ else coded)
    t = np.stack(out)
    assert (t == MARK).sum() >= 8
    t.setflags(write=False)
    return t


def _pick_ids(k, m, R, rng):
    """[S, k + R] listed ids, different per stripe"""
    return np.stack([rng.permutation(k + m)[:k + R] for _ in range(S)]).astype(np.uint16)


def _split(recv_rows):
    """restored symbols [H, P] -> (u16 rows, mark lists)"""
    rows = (recv_rows & 0xffff).astype(np.uint16)
    return rows, [[int(c) for c in np.flatnonzero(recv_rows[h] == MARK)]
                  for h in range(recv_rows.shape[0])]


# ---- the device calls --------------------------------------------------------

def _share(torch, plan, ids, held, recv, acc=None, unaligned=False, cap=CAP, out_cap=CAP,
           expect_err=0):
    """One qi_gpu_syndrome call over the held positions [S, H] of the restored
    stripes recv [S, k + m, P]; acc: (rows u16 [S, R, P], mark sets) of an
    earlier call, updated in place.  Returns (rows, mark sets [S][R])."""
    S_, H = held.shape
    R = ids.shape[1] - plan.k
    P = recv.shape[2]
    first = plan.k if plan.sys else 0
    rows = np.zeros((S_, H, P), np.uint16)
    marks = []
    for s in range(S_):
        fr = ids[s][held[s].astype(np.int64)].astype(np.int64)
        rows[s], mk = _split(recv[s][fr])
        # a data row has no marks: its bucket holds rubbish, never read
        marks.append([mk[h] if fr[h] >= first else [1, 2, 3] for h in range(H)])
    nb = plan.syndrome_ctx_bytes(H, R, S_)
    RP = {1: 1, 2: 2, 3: 4, 4: 4}.get(R, 8)
    assert nb == S_ * 4 * (H * RP + RP + H)
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    plan.syndrome_ctx(_dev16(torch, ids), _dev16(torch, held), ctx)
    rbig, drows = _rows_dev(torch, rows, unaligned)
    counts, entries = _buckets(torch, marks, cap)
    if acc is not None:
        obig, out = _rows_dev(torch, acc[0], unaligned)
        ac, ae = _buckets(torch, [[sorted(x) for x in row] for row in acc[1]], cap)
    else:
        obig, out = _rows_dev(torch, np.full((S_, R, P), FILL, np.uint16), unaligned)
        ac = ae = None
    oc = torch.zeros(S_ * R, dtype=torch.int32, device="cuda")
    oe = torch.full((S_ * R * out_cap,), -1, dtype=torch.int32, device="cuda")
    err = plan.syndrome(ctx, drows, out, acc=out if acc is not None else None, counts=counts,
                        entries=entries, cap=cap, acc_counts=ac, acc_entries=ae,
                        acc_cap=cap if ac is not None else 0, out_counts=oc, out_entries=oe,
                        out_cap=out_cap)
    torch.cuda.synchronize()
    assert err == expect_err
    assert _guards_intact(rbig, drows) and _guards_intact(obig, out)
    assert (drows.cpu().numpy().view(np.uint16) == rows).all()   # read only
    got = out.cpu().numpy().view(np.uint16).copy()
    cnt, sets = _read_buckets(oc, oe, S_, R, out_cap)
    assert all(cnt[s, j] == len(sets[s][j]) for s in range(S_) for j in range(R))
    return got, sets


def _all_held(ids):
    return np.tile(np.arange(ids.shape[1], dtype=np.uint16), (ids.shape[0], 1))


def _resolve(torch, plan, ids, syn, sets, t, fix_cap=None, unaligned=False, cap=CAP,
             expect_err=0):
    """qi_gpu_syndrome_locate over syndrome rows syn [S, R, P] u16 with mark sets
    [S][R]; returns (located [S, N], unlocated [S], weights [S, 4], fix_counts
    [S], fixes [S, fix_cap, 3]), every output inside guard words"""
    S_, N = ids.shape
    R, P = syn.shape[1], syn.shape[2]
    fix_cap = 4 * P if fix_cap is None else fix_cap
    nb = plan.syndrome_locate_ctx_bytes(R, S_)
    assert nb == S_ * 12 * N
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    plan.syndrome_locate_ctx(_dev16(torch, ids), ctx)
    sbig, dsyn = _rows_dev(torch, syn, unaligned)
    counts, entries = _buckets(torch, [[sorted(x) for x in row] for row in sets], cap)
    G = 16
    sizes = [S_ * N, S_, S_ * 4, S_, S_ * max(fix_cap, 1) * 3]
    bufs = [torch.full((n + 2 * G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for n in sizes]
    views = [b[G:G + n] for b, n in zip(bufs, sizes)]
    views[4].fill_(-1)
    rp = 2 if R <= 2 else 4 if R <= 4 else 8
    if not unaligned and P % 8 == 0:
        assert plan.syndrome_locate_kernels(R, t, P) == (
            f"syndrome_locate=syndrome_locate_ctx_kernel + syndrome_locate_kernel<{rp}, true>")
    err = plan.syndrome_locate(ctx, t, dsyn, views[0], views[1], views[2], views[3],
                               views[4] if fix_cap else None, fix_cap, counts=counts,
                               entries=entries, cap=cap)
    torch.cuda.synchronize()
    assert err == expect_err
    assert _guards_intact(sbig, dsyn)
    assert (dsyn.cpu().numpy().view(np.uint16) == syn).all()     # no row is written
    for b, n in zip(bufs, sizes):
        g = b.cpu().numpy()
        assert (g[:G] == 0x5A5A5A5A).all() and (g[G + n:] == 0x5A5A5A5A).all()
    o = [v.cpu().numpy().copy() for v in views]
    return (o[0].reshape(S_, N), o[1], o[2].reshape(S_, 4), o[3],
            o[4].reshape(S_, max(fix_cap, 1), 3))


def _fix_sets(res):
    """per stripe the set of (column, position, e), checked to be distinct"""
    out = []
    for s in range(res[0].shape[0]):
        n = int(res[3][s])
        got = [tuple(int(v) for v in f) for f in res[4][s, :n]]
        assert len(set(got)) == n
        out.append(set(got))
    return out


# ---- 1. codewords ------------------------------------------------------------

@pytest.mark.parametrize("k,m,sys_,P,unaligned", SHAPES)
def test_share_of_an_intact_stripe_is_zero(hip_lib, k, m, sys_, P, unaligned):
    torch = _torch()
    import quadiron_amd as qa
    truth = _truth(k, m, sys_, P)
    plan = qa.Plan(k, m, bool(sys_))
    for R in (1, 2, 3, 4, 8):
        if R > m:
            continue
        ids = _pick_ids(k, m, R, np.random.default_rng([k, R, 1]))
        first = k if sys_ else 0
        # rows with marks are among the listed ones
        assert sum(int((truth[s][ids[s][ids[s] >= first]] == MARK).sum()) for s in range(S)) >= 1
        got, sets = _share(torch, plan, ids, _all_held(ids), truth, unaligned=unaligned)
        assert not got.any(), (R, np.argwhere(got)[:4])
        assert all(not x for row in sets for x in row), R
        vec = "true" if P % 8 == 0 and not unaligned else "false"
        if vec == "true":
            rp = {1: 1, 2: 2, 3: 4, 4: 4}.get(R, 8)
            assert plan.syndrome_kernels(k + R, R, P) == (
                f"syndrome=syndrome_ctx_kernel + partial_kernel<{rp}, true>")


# ---- 2. additivity -----------------------------------------------------------

def _inject_for_sums(k, m, sys_, truth, ids, x, w, rng):
    """recv with known errors: per stripe a list of (position, column, e).  One
    error is e = 65536 w_p (S_0 is the mark value), one corrupted symbol is a
    mark, the others random; positions on coded rows where a mark is needed"""
    P = truth.shape[2]
    first = k if sys_ else 0
    recv = truth.copy()
    errs = []
    for s in range(S):
        coded = [p for p in range(ids.shape[1]) if ids[s, p] >= first]
        cols = [int(c) for c in rng.choice(P, 12, replace=False)] + [0, TILE - 1, P - 1]
        cols = list(dict.fromkeys(cols))
        es = []
        for i, c in enumerate(cols):
            f = lambda p: int(ids[s, p])
            if i == 0:       # S_0 = e / w_p = 65536
                p = int(rng.choice(coded))
                e = MARK * int(w[s][p]) % Q
            elif i == 1:     # the corrupted symbol is a mark
                p = int(rng.choice(coded))
                e = (MARK - int(truth[s, f(p), c])) % Q
                if e == 0:
                    e = 1
            else:
                p = int(rng.integers(0, ids.shape[1]))
                e = int(rng.integers(1, Q))
            v = (int(truth[s, f(p), c]) + e) % Q
            if v == MARK and f(p) < first:      # a data row holds no 65536
                e, v = (e + 1) % Q, 0
            recv[s, f(p), c] = v
            es.append((p, c, e))
            if i == 1:
                assert recv[s, f(p), c] == MARK or truth[s, f(p), c] == MARK
        errs.append(es)
    return recv, errs


@pytest.mark.parametrize("k,m,sys_,P,unaligned", [SHAPES[1], SHAPES[2], SHAPES[3], SHAPES[5]])
def test_shares_add_up(hip_lib, k, m, sys_, P, unaligned):
    torch = _torch()
    import quadiron_amd as qa
    R = 4
    N = k + R
    rng = np.random.default_rng([k, m, 2])
    truth = _truth(k, m, sys_, P)
    ids = _pick_ids(k, m, R, rng)
    xw = [_points(k, m, ids[s]) for s in range(S)]
    recv, errs = _inject_for_sums(k, m, sys_, truth, ids, [a for a, _ in xw], [b for _, b in xw],
                                  rng)
    plan = qa.Plan(k, m, bool(sys_))
    whole = _share(torch, plan, ids, _all_held(ids), recv, unaligned=unaligned)
    chains = []
    for order in ((1, 5, N - 6), (N - 6, 1, 5)):
        perm = [rng.permutation(N) for _ in range(S)]
        acc, at = None, 0
        for n in order:
            held = np.array([p[at:at + n] for p in perm], np.uint16)
            at += n
            acc = _share(torch, plan, ids, held, recv, acc=acc, unaligned=unaligned)
        assert at == N
        chains.append(acc)
    for got in chains:
        assert (got[0] == whole[0]).all() and got[1] == whole[1]
    # Python integers
    n_marks = 0
    for s in range(S):
        x, w = xw[s]
        exp = np.zeros((R, P), np.int64)
        for p, c, e in errs[s]:
            for j in range(R):
                exp[j, c] = (exp[j, c] + e * pow(int(x[p]), j, Q) * pow(int(w[p]), Q - 2, Q)) % Q
        assert (whole[0][s] == (exp & 0xffff)).all()
        for j in range(R):
            em = set(int(c) for c in np.flatnonzero(exp[j] == MARK))
            assert whole[1][s][j] == em, (s, j)
            n_marks += len(em)
        assert exp[0, errs[s][0][1]] == MARK
    assert n_marks >= S


# ---- 3. the resolve against a brute-force decoder ----------------------------

def _inv_matrix(V):
    """inverse mod Q of a small square matrix of Python ints"""
    n = len(V)
    M = [[int(v) % Q for v in V[i]] + [int(i == j) for j in range(n)] for i in range(n)]
    for c in range(n):
        piv = next(r for r in range(c, n) if M[r][c])
        M[c], M[piv] = M[piv], M[c]
        inv = pow(M[c][c], Q - 2, Q)
        M[c] = [v * inv % Q for v in M[c]]
        for r in range(n):
            if r != c and M[r][c]:
                f = M[r][c]
                M[r] = [(a - f * b) % Q for a, b in zip(M[r], M[c])]
    return np.array([row[n:] for row in M], np.int64)


def _brute_force(x, w, Ssyn, t):
    """Ssyn [R, P] int64 -> (located [N], unlocated, weights [4], fixes): every
    set of at most t positions is tried, the Vandermonde system solved exactly,
    and the set accepted only if all R syndromes match with no E_a zero"""
    R, P = Ssyn.shape
    N = len(x)
    dirty = Ssyn.any(axis=0)
    owner = np.full(P, -1, np.int64)
    sets, Es = [], []
    for nu in range(1, t + 1):
        for A in itertools.combinations(range(N), nu):
            V = np.array([[pow(int(x[a]), j, Q) for a in A] for j in range(R)], np.int64)
            E = matvec_mod(_inv_matrix(V[:nu]), Ssyn[:nu])
            ok = dirty & (E != 0).all(axis=0) & (matvec_mod(V, E) == Ssyn).all(axis=0)
            assert (owner[ok] == -1).all()          # 2 t <= R: at most one set
            owner[ok] = len(sets)
            sets.append(A)
            Es.append(E)
    located = np.zeros(N, np.int64)
    weights = np.zeros(4, np.int64)
    fixes = set()
    for c in np.flatnonzero(owner >= 0):
        A, E = sets[owner[c]], Es[owner[c]]
        weights[len(A) - 1] += 1
        for i, a in enumerate(A):
            located[a] += 1
            fixes.add((int(c), int(a), int(E[i, c]) * int(w[a]) % Q))
    return located, int((dirty & (owner < 0)).sum()), weights, fixes


SPECIAL = (0, 1, 32768, 32769, 65535, MARK)


@pytest.mark.parametrize("k,m,R", [(3, 5, 1), (3, 5, 2), (3, 5, 3), (3, 5, 4), (3, 5, 5),
                                   (4, 8, 8)])
def test_resolve_vs_brute_force(hip_lib, k, m, R):
    torch = _torch()
    import quadiron_amd as qa
    P = RAGGED
    N = k + R
    rng = np.random.default_rng([k, R, 3])
    ids = _pick_ids(k, m, R, rng)
    xw = [_points(k, m, ids[s]) for s in range(S)]
    syn = rng.integers(0, Q, (S, R, P)).astype(np.int64)
    for s in range(S):
        x, w = xw[s]
        # columns from 0 .. R errors at random positions (decodable ones and
        # the guard zone), then clean columns, then every special value in
        # every slot of random, of one-error and of clean columns
        for c in range(0, P - 400):
            nu = c % (R + 2)
            if nu > R:
                continue
            pos = rng.choice(N, nu, replace=False)
            E = rng.integers(1, Q, nu)
            syn[s, :, c] = [sum(int(e) * pow(int(x[p]), j, Q) for e, p in zip(E, pos)) % Q
                            for j in range(R)]
        c = P - 400
        for kind in range(3):
            for j in range(R):
                for v in SPECIAL:
                    if kind == 1:
                        p = int(rng.integers(0, N))
                        # E chosen so that slot j is v (v = 0 has no such E: E = 1)
                        E = v * pow(pow(int(x[p]), j, Q), Q - 2, Q) % Q or 1
                        syn[s, :, c] = [E * pow(int(x[p]), jj, Q) % Q for jj in range(R)]
                    elif kind == 2:
                        syn[s, :, c] = 0
                    syn[s, j, c] = v
                    c += 1
        assert c <= P
    rows = (syn & 0xffff).astype(np.uint16)
    sets = [[set(int(c) for c in np.flatnonzero(syn[s, j] == MARK)) for j in range(R)]
            for s in range(S)]
    assert sum(len(x) for row in sets for x in row) >= R
    plan = qa.Plan(k, m, False)
    for t in range(R // 2 + 1):
        res = _resolve(torch, plan, ids, rows, sets, t)
        fx = _fix_sets(res)
        for s in range(S):
            loc, nun, wts, fixes = _brute_force(xw[s][0], xw[s][1], syn[s], t)
            assert (res[0][s] == loc).all(), (t, s, res[0][s], loc)
            assert res[1][s] == nun, (t, s, res[1][s], nun)
            assert (res[2][s] == wts).all(), (t, s, res[2][s], wts)
            assert fx[s] == fixes, (t, s, sorted(fx[s] ^ fixes)[:5])
            if t == 0:
                assert nun == int(syn[s].any(axis=0).sum()) and not fixes
            else:
                assert all(wts[:t] > 0) and nun > 0


# ---- 4. agreement with qi_gpu_locate_multi -----------------------------------

def _inject(recv, ids, s, c, b, rng, sys_, k):
    """b bad listed fragments in column c of stripe s: other storable symbols"""
    for p in rng.choice(ids.shape[1], b, replace=False):
        f = int(ids[s, p])
        hi = 65536 if sys_ and f < k else Q
        recv[s, f, c] = (recv[s, f, c] + int(rng.integers(1, hi))) % hi


def _corrupt(k, m, sys_, R, t, truth, ids, rng, n_cols=40):
    P = truth.shape[2]
    recv = truth.copy()
    edge = list(dict.fromkeys(c for c in (0, TILE - 1, TILE, P - 1) if c < P))
    cols = edge + [int(c) for c in rng.permutation(P)[:n_cols] if c not in edge]
    for s in range(S):
        for i, c in enumerate(cols):
            _inject(recv, ids, s, c, 1 + (i + s) % (R - t), rng, sys_, k)
    return recv


def _by_construction(truth, recv, ids, t):
    res = []
    for s in range(S):
        bad = truth[s][ids[s]] != recv[s][ids[s]]
        nb = bad.sum(axis=0)
        loc = np.zeros(ids.shape[1], np.int64)
        wts = np.zeros(4, np.int64)
        fixes = set()
        for c in np.flatnonzero((nb >= 1) & (nb <= t)):
            wts[nb[c] - 1] += 1
            for p in np.flatnonzero(bad[:, c]):
                loc[p] += 1
                fixes.add((int(c), int(p), int(truth[s, ids[s, p], c])))
        res.append((loc, int((nb > t).sum()), wts, fixes))
    return res


@pytest.mark.parametrize("k,m,sys_,P,unaligned", SHAPES[:4])
def test_resolve_agrees_with_locate_multi(hip_lib, k, m, sys_, P, unaligned):
    torch = _torch()
    import quadiron_amd as qa
    from test_gpu_locate_multi import _locate_multi
    truth = _truth(k, m, sys_, P)
    plan = qa.Plan(k, m, bool(sys_))
    for R, t in ((2, 1), (4, 1), (4, 2), (8, 4)):
        if R > m:
            continue
        rng = np.random.default_rng([k, R, t, 4])
        ids = _pick_ids(k, m, R, rng)
        recv = _corrupt(k, m, sys_, R, t, truth, ids, rng)
        syn, sets = _share(torch, plan, ids, _all_held(ids), recv, unaligned=unaligned)
        res = _resolve(torch, plan, ids, syn, sets, t, unaligned=unaligned)
        # {column, p, (y_p - e) mod q}
        fx = [set((c, p, (int(recv[s, ids[s, p], c]) - e) % Q) for c, p, e in f)
              for s, f in enumerate(_fix_sets(res))]
        if k <= 256:
            ref = _locate_multi(k, m, sys_, R, t, ids, recv, unaligned=unaligned)
            assert ref[0] == 0
            assert (res[0] == ref[1]).all() and (res[1] == ref[2]).all()
            assert (res[2] == ref[3]).all() and (res[3] == ref[4]).all()
            for s in range(S):
                rf = set(tuple(int(v) for v in f) for f in ref[5][s, :ref[4][s]])
                assert fx[s] == rf, (R, t, s, sorted(fx[s] ^ rf)[:5])
        if R > 2:      # (R = 2: two bad fragments may pass as one)
            for s, (loc, nun, wts, fixes) in enumerate(_by_construction(truth, recv, ids, t)):
                assert (res[0][s] == loc).all() and res[1][s] == nun
                assert (res[2][s] == wts).all() and fx[s] == fixes
                assert wts[:t].min() > 0 and (R == 2 * t or nun > 0)


# ---- 5. end to end above k = 256 ---------------------------------------------

def _block_case(k, m, sys_, b_max, seed, words=RAGGED):
    """one oracle stripe with k + 4 fragments present, corrupted in columns with
    1 .. b_max bad fragments; returns the clean and corrupt (rows by fragment
    id, oor, counts), missing flags, listed ids"""
    rng = np.random.default_rng([k, m, sys_, b_max, seed])
    truth = _truth(k, m, sys_, words)[0]
    first = k if sys_ else 0
    no = m if sys_ else k + m
    present = np.sort(rng.permutation(k + m)[:k + 4])
    missing = np.ones(k + m, np.int32)
    missing[present] = 0
    recv = truth.copy()
    cols = [0, TILE - 1, TILE, words - 1] + [int(c) for c in rng.permutation(words)[:20]]
    for i, c in enumerate(dict.fromkeys(cols)):
        b = 1 + i % b_max
        for j, f in enumerate(rng.choice(present, b, replace=False)):
            f = int(f)
            hi = 65536 if f < first else Q
            if i < 4 and j == 0 and f >= first:     # to a mark, or away from one
                recv[f, c] = MARK if truth[f, c] != MARK else 5
            else:
                recv[f, c] = (truth[f, c] + int(rng.integers(1, hi))) % hi
    def pack(sym):
        rows = [np.ascontiguousarray((sym[f] & 0xffff).astype(np.uint16)).view(np.uint8).copy()
                for f in range(k + m)]
        oor = np.zeros((no, CAP), np.uint32)
        cnt = np.zeros(no, np.uint32)
        for j in range(no):
            mk = np.flatnonzero(sym[first + j] == MARK)
            cnt[j] = len(mk)
            oor[j, :len(mk)] = mk
        return rows, oor, cnt
    return pack(truth), pack(recv), missing, present, (truth != recv).any(axis=0)


def _call_args(k, sys_, rows, missing):
    first = k if sys_ else 0
    data = [rows[f] if not missing[f] else None for f in range(k)] if sys_ else None
    par = [rows[f] if not missing[f] else None for f in range(first, len(rows))]
    return data, par


WIDE = [(300, 212, 0), (1100, 100, 0), (260, 30, 1)]


@pytest.mark.parametrize("k,m,sys_", WIDE)
def test_scrub_blocks_corrects_wide_codes(hip_lib, k, m, sys_):
    import quadiron_amd as qa
    (trows, toor, tcnt), (rows, oor, cnt), missing, present, dirty = _block_case(k, m, sys_, 2, 5)
    fec = qa.Fec(k, m, bool(sys_))
    data, par = _call_args(k, sys_, rows, missing)
    # what the parent offers answers "shape not supported"
    with pytest.raises(ValueError):
        fec.locate_blocks(data, par, oor, cnt, missing, correct=True, max_errors=2)
    res, patched = fec.scrub_blocks(data, par, oor, cnt, missing, max_errors=2, correct=True)
    assert patched and res[k + m] == 0
    assert res[k + m + 1] > 0 and res[k + m + 2] > 0
    assert res[k + m + 1] + res[k + m + 2] == dirty.sum()
    assert (res[:k + m][missing == 1] == -1).all() and (res[:k + m][missing == 0] >= 0).all()
    for f in present:
        assert (rows[f] == trows[f]).all(), f
    assert (cnt == tcnt).all()
    for j in range(len(cnt)):
        assert (oor[j, :cnt[j]] == toor[j, :tcnt[j]]).all(), j
    # a clean stripe: nothing located, nothing patched
    res, patched = fec.scrub_blocks(data, par, oor, cnt, missing, max_errors=2, correct=True)
    assert not patched and not res[:k + m][missing == 0].any() and not res[k + m:].any()
    # detection only
    (_, _, _), (rows, oor, cnt), missing, present, dirty = _block_case(k, m, sys_, 2, 5)
    data, par = _call_args(k, sys_, rows, missing)
    res = fec.scrub_blocks(data, par, oor, cnt, missing, max_errors=0)
    assert len(res) == k + m + 1 and res[k + m] == dirty.sum()


@pytest.mark.parametrize("k,m,sys_", WIDE[:2])
def test_scrub_blocks_three_bad_fragments_patch_nothing(hip_lib, k, m, sys_):
    import quadiron_amd as qa
    _, (rows, oor, cnt), missing, present, dirty = _block_case(k, m, sys_, 3, 6)
    before = [r.copy() for r in rows], oor.copy(), cnt.copy()
    data, par = _call_args(k, sys_, rows, missing)
    res, patched = qa.Fec(k, m, bool(sys_)).scrub_blocks(data, par, oor, cnt, missing,
                                                         max_errors=2, correct=True)
    assert not patched and res[k + m] > 0
    assert res[k + m] + res[k + m + 1] + res[k + m + 2] == dirty.sum()
    assert all((a == b).all() for a, b in zip(rows, before[0]))
    assert (oor == before[1]).all() and (cnt == before[2]).all()


@pytest.mark.parametrize("k,m,sys_", WIDE)
def test_split_flow_gives_the_same_buffers(hip_lib, k, m, sys_):
    """two nodes form shares, a coordinator resolves, each holder applies"""
    import quadiron_amd as qa
    (trows, toor, tcnt), (rows, oor, cnt), missing, present, dirty = _block_case(k, m, sys_, 2, 5)
    first = k if sys_ else 0
    fec = qa.Fec(k, m, bool(sys_))
    listed = [int(f) for f in present]
    nodes = [listed[:7], listed[7:]]
    acc = None
    held = []
    for frs in nodes:
        n_oor = np.zeros((len(frs), CAP), np.uint32)
        n_cnt = np.zeros(len(frs), np.uint32)
        for h, f in enumerate(frs):
            if f >= first:
                n_cnt[h] = cnt[f - first]
                n_oor[h] = oor[f - first]
        held.append((frs, [rows[f] for f in frs], n_oor, n_cnt))
        acc = fec.syndrome_blocks(listed, frs, held[-1][1], n_oor, n_cnt, 4, acc=acc)
    res, fixes = fec.locate_syndromes(listed, acc[0], acc[1], acc[2], max_errors=2)
    assert res[k + m] == 0 and res[k + m + 1] + res[k + m + 2] == dirty.sum()
    assert len(fixes) == res[k + m + 1] + 2 * res[k + m + 2]
    assert set(int(f) for f in fixes[:, 1]) <= set(listed)
    applied = 0
    for frs, nrows, n_oor, n_cnt in held:
        n = fec.apply_deltas(frs, nrows, n_oor, n_cnt, fixes)
        assert n is not None          # nothing refused: a correct fix is storable
        applied += n
        for h, f in enumerate(frs):
            assert (nrows[h] == trows[f]).all(), f
            if f >= first:
                assert n_cnt[h] == tcnt[f - first]
                assert (n_oor[h, :n_cnt[h]] == toor[f - first, :n_cnt[h]]).all(), f
    assert applied == len(fixes)
    # scrub_blocks on the same corrupt stripe leaves the same buffers
    _, (rows2, oor2, cnt2), _, _, _ = _block_case(k, m, sys_, 2, 5)
    data, par = _call_args(k, sys_, rows2, missing)
    _, patched = fec.scrub_blocks(data, par, oor2, cnt2, missing, max_errors=2, correct=True)
    assert patched
    for f in listed:
        assert (rows2[f] == rows[f]).all()


# ---- 6. the fix list ----------------------------------------------------------

def test_fix_list_overflow(hip_lib):
    torch = _torch()
    import quadiron_amd as qa
    k, m, R, t, P = 16, 48, 4, 2, 512
    rng = np.random.default_rng(6)
    ids = _pick_ids(k, m, R, rng)
    plan = qa.Plan(k, m, False)
    syn = np.zeros((S, R, P), np.int64)
    x, _ = _points(k, m, ids[1])
    for c, p in ((3, 0), (100, 7), (511, 19)):       # three one-error columns in stripe 1
        syn[1, :, c] = [9 * pow(int(x[p]), j, Q) % Q for j in range(R)]
    rows = (syn & 0xffff).astype(np.uint16)
    sets = [[set(int(c) for c in np.flatnonzero(syn[s, j] == MARK)) for j in range(R)]
            for s in range(S)]
    res = _resolve(torch, plan, ids, rows, sets, t, fix_cap=1)
    assert list(res[3]) == [0, 3] and list(res[1]) == [0, 0] and res[2][1, 0] == 3
    assert (res[4][0] == -1).all()
    assert res[4][1, 0, 0] in (3, 100, 511)
    full = _resolve(torch, plan, ids, rows, sets, t)
    assert {c for c, _, _ in _fix_sets(full)[1]} == {3, 100, 511}
    # the block API: its own first capacity is 64 + 512 // 512 = 65 entries
    fec = qa.Fec(k, m, False)
    blk = np.zeros((R, P), np.int64)
    x, w = _points(k, m, ids[0])
    for c in range(100):
        blk[:, c] = [(1 + c) * pow(int(x[c % 20]), j, Q) % Q for j in range(R)]
    brow = [np.ascontiguousarray((blk[j] & 0xffff).astype(np.uint16)).view(np.uint8)
            for j in range(R)]
    boor = np.zeros((R, CAP), np.uint32)
    bcnt = np.zeros(R, np.uint32)
    for j in range(R):
        mk = np.flatnonzero(blk[j] == MARK)
        bcnt[j] = len(mk)
        boor[j, :len(mk)] = mk
    for cap0 in (1, 256):
        r2, fixes = fec.locate_syndromes([int(f) for f in ids[0]], brow, boor, bcnt,
                                         max_errors=2, fix_cap=cap0)
        assert len(fixes) == 100 and r2[k + m] == 0 and r2[k + m + 1] == 100
        want = {(c, int(ids[0][c % 20]), (1 + c) * int(w[c % 20]) % Q) for c in range(100)}
        assert set(tuple(int(v) for v in f) for f in fixes) == want


def test_syndrome_blocks_retry(hip_lib):
    """Fec.syndrome_blocks with an accumulator, second attempt: the last link's
    row makes syndrome 0 of the sum 65536 in 100 columns against a
    first-attempt capacity of 64 + 512 // 512 = 65, so the share runs again,
    from the acc rows (and their marks) as they were."""
    import quadiron_amd as qa
    k = m = 4
    R, P = 2, 512
    cap0 = 64 + P // 512
    n_hot = 100
    assert n_hot > cap0
    fec = qa.Fec(k, m, False)
    rng = np.random.default_rng(8)
    listed = [int(f) for f in rng.permutation(k + m)[:k + R]]
    N = len(listed)
    x, w = _points(k, m, listed)
    winv = [pow(int(v), Q - 2, Q) for v in w]
    y = rng.integers(0, 65536, (N, P)).astype(np.int64)
    for p in range(N - 1):          # marks on link 1's rows
        y[p, rng.choice(P, 3, replace=False)] = MARK

    def syndromes(pos):
        e = np.zeros((R, P), np.int64)
        for p in pos:
            for j in range(R):
                e[j] = (e[j] + y[p] * pow(int(x[p]), j, Q) % Q * winv[p]) % Q
        return e

    # link 1's own sum holds marks too: three columns of its last row are crafted
    acc_cols = rng.choice(P, 3, replace=False)
    part = syndromes(range(N - 2))[0]
    y[N - 2, acc_cols] = (MARK - part[acc_cols]) % Q * int(w[N - 2]) % Q
    a0 = syndromes(range(N - 1))[0]
    assert (a0[acc_cols] == MARK).all()
    hot = np.sort(np.concatenate([[0, P - 1], 1 + rng.choice(P - 2, n_hot - 2, replace=False)]))
    assert len(set(hot.tolist())) == n_hot
    y[N - 1, hot] = (MARK - a0[hot]) % Q * int(w[N - 1]) % Q
    exp1, exp = syndromes(range(N - 1)), syndromes(range(N))
    assert (exp[0, hot] == MARK).all() and (exp[0] == MARK).sum() >= n_hot > cap0

    def link(pos, acc):
        rows, marks = _split(y[pos])
        oor = np.zeros((len(pos), CAP), np.uint32)
        cnt = np.zeros(len(pos), np.uint32)
        for h, mk in enumerate(marks):
            cnt[h] = len(mk)
            oor[h, :len(mk)] = mk
        rows = [np.ascontiguousarray(r).view(np.uint8) for r in rows]
        return fec.syndrome_blocks(listed, [listed[p] for p in pos], rows, oor, cnt, R, acc=acc,
                                   out_cap=128)

    def check(got, want):
        rows, oor, cnt = got
        for j in range(R):
            em = [int(c) for c in np.flatnonzero(want[j] == MARK)]
            assert (rows[j].view(np.uint16) == (want[j] & 0xffff)).all(), j
            assert cnt[j] == len(em), (j, cnt[j], len(em))
            assert [int(c) for c in oor[j, :cnt[j]]] == em, j

    acc = link(list(range(N - 1)), None)
    check(acc, exp1)
    assert acc[2][0] >= 3
    before = [r.copy() for r in acc[0]], acc[1].copy(), acc[2].copy()
    check(link([N - 1], acc), exp)
    # the accumulator handed in is the caller's: left as it was
    assert all((a == b).all() for a, b in zip(acc[0], before[0]))
    assert (acc[1] == before[1]).all() and (acc[2] == before[2]).all()


# ---- 7. errors ----------------------------------------------------------------

BAD =["id_repeated", "id_high", "pos_repeated", "pos_high"]


@pytest.mark.parametrize("what", BAD)
def test_bad_ids_raise_bit_2(hip_lib, what):
    torch = _torch()
    import quadiron_amd as qa
    k, m, sys_, R = 16, 48, 0, 4
    N = k + R
    rng = np.random.default_rng(7)
    truth = _truth(k, m, sys_, TILE)
    ids = _pick_ids(k, m, R, rng)
    recv = _corrupt(k, m, sys_, R, 2, truth, ids, rng)
    plan = qa.Plan(k, m, False)
    held = _all_held(ids)
    good = _share(torch, plan, ids, held, recv)
    good_res = _resolve(torch, plan, ids, good[0], good[1], 2)
    bad_ids, bad_held = ids.copy(), held.copy()
    look = bad_ids
    if what == "id_repeated":
        bad_ids[0, 9] = bad_ids[0, 2]
    elif what == "id_high":
        bad_ids[0, 5] = k + m
        look = bad_ids.copy()      # the test's own row lookup needs a valid id
        look[0, 5] = 0
    elif what == "pos_repeated":
        bad_held[0, 3] = bad_held[0, 11]
    else:
        bad_held[0, 6] = N
    # the share: the other stripe's rows are intact, every buffer stays inside
    got = _share_with(torch, plan, bad_ids, look, bad_held, recv)
    assert plan.take_error() == 0
    assert (got[0][1] == good[0][1]).all() and got[1][1] == good[1][1]
    if what.startswith("id_"):
        res = _resolve(torch, plan, bad_ids, good[0], good[1], 2, expect_err=2)
        for i in (0, 1, 2, 3):
            assert (np.asarray(res[i][1]) == np.asarray(good_res[i][1])).all()
        assert _fix_sets(res)[1] == _fix_sets(good_res)[1]


def _share_with(torch, plan, ids, look, held, recv):
    """_share with the rows looked up through `look` and bit 2 expected"""
    S_, H = held.shape
    R = ids.shape[1] - plan.k
    P = recv.shape[2]
    rows = np.zeros((S_, H, P), np.uint16)
    marks = []
    for s in range(S_):
        pos = np.minimum(held[s].astype(np.int64), ids.shape[1] - 1)
        rows[s], mk = _split(recv[s][look[s][pos].astype(np.int64)])
        marks.append(mk)
    ctx = torch.randint(0, 256, (plan.syndrome_ctx_bytes(H, R, S_),), dtype=torch.uint8,
                        device="cuda")
    plan.syndrome_ctx(_dev16(torch, ids), _dev16(torch, held), ctx)
    torch.cuda.synchronize()
    assert plan.take_error() == 2
    assert plan.take_error() == 0
    rbig, drows = _rows_dev(torch, rows)
    obig, out = _rows_dev(torch, np.full((S_, R, P), FILL, np.uint16))
    counts, entries = _buckets(torch, marks, CAP)
    oc = torch.zeros(S_ * R, dtype=torch.int32, device="cuda")
    oe = torch.full((S_ * R * CAP,), -1, dtype=torch.int32, device="cuda")
    assert plan.syndrome(ctx, drows, out, counts=counts, entries=entries, cap=CAP, out_counts=oc,
                         out_entries=oe, out_cap=CAP) == 0
    torch.cuda.synchronize()
    assert _guards_intact(rbig, drows) and _guards_intact(obig, out)
    cnt, sets = _read_buckets(oc, oe, S_, R, CAP)
    return out.cpu().numpy().view(np.uint16).copy(), sets


def test_input_bucket_over_capacity_raises_bit_1(hip_lib):
    torch = _torch()
    import quadiron_amd as qa
    k, m, R, P, cap = 16, 48, 2, 64, 4
    plan = qa.Plan(k, m, False)
    ids = np.tile(np.arange(k + R, dtype=np.uint16), (1, 1))
    held = np.array([[0, 1]], np.uint16)
    ctx = torch.zeros(plan.syndrome_ctx_bytes(2, R, 1), dtype=torch.uint8, device="cuda")
    plan.syndrome_ctx(_dev16(torch, ids), _dev16(torch, held), ctx)
    rows = torch.zeros((1, 2, P), dtype=torch.int16, device="cuda")
    out = torch.zeros((1, R, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    entries = torch.zeros(2 * cap, dtype=torch.int32, device="cuda")
    counts[1] = cap + 1
    assert plan.syndrome(ctx, rows, out, counts=counts, entries=entries, cap=cap) == 1
    assert plan.take_error() == 0
    counts[1] = cap
    assert plan.syndrome(ctx, rows, out, counts=counts, entries=entries, cap=cap) == 0
    # the resolve's syndrome buckets
    lctx = torch.zeros(plan.syndrome_locate_ctx_bytes(R, 1), dtype=torch.uint8, device="cuda")
    plan.syndrome_locate_ctx(_dev16(torch, ids), lctx)
    z = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in (k + R, 1, 4, 1)]
    counts[1] = cap + 1
    assert plan.syndrome_locate(lctx, 1, out, *z, counts=counts, entries=entries, cap=cap) == 1
    counts[1] = cap
    assert plan.syndrome_locate(lctx, 1, out, *z, counts=counts, entries=entries, cap=cap) == 0


@pytest.mark.parametrize("k,m,H,R,t", [(16, 48, 2, 0, 0), (16, 48, 2, 9, 0), (16, 4, 2, 5, 0),
                                       (16, 48, 0, 4, 0), (16, 48, 21, 4, 0), (16, 48, 2, 4, 3),
                                       (16, 48, 2, 1, 1), (16, 48, 2, 4, -1)])
def test_counts_out_of_range(hip_lib, k, m, H, R, t):
    """-1 (0, "") from every entry point concerned, and nothing written"""
    torch = _torch()
    import quadiron_amd as qa
    plan = qa.Plan(k, m, False)
    lib = qa.lib()
    S_, P = 2, 64
    share_bad = not (1 <= R <= min(8, m)) or not (1 <= H <= k + R)
    locate_bad = not (1 <= R <= min(8, m)) or not (0 <= 2 * t <= R)
    assert share_bad or locate_bad
    z = torch.zeros(S_ * 64, dtype=torch.int16, device="cuda")
    ctx = torch.full((1 << 14,), 0x5A, dtype=torch.uint8, device="cuda")
    rows = torch.full((S_, 24, P), FILL, dtype=torch.int16, device="cuda")
    out = torch.full((S_, 9, P), FILL, dtype=torch.int16, device="cuda")
    res = torch.full((S_ * 64,), 7, dtype=torch.int32, device="cuda")
    if share_bad:
        assert lib.qi_gpu_syndrome_ctx_bytes(plan.h, H, R, S_) == 0
        assert plan.syndrome_kernels(H, R, P) == ""
        assert lib.qi_gpu_syndrome_ctx(plan.h, z.data_ptr(), z.data_ptr(), H, R, S_,
                                       ctx.data_ptr(), None) == -1
        assert lib.qi_gpu_syndrome(plan.h, ctx.data_ptr(), H, R, rows.data_ptr(), 24 * P, P, None,
                                   None, 0, None, 0, 0, None, None, 0, out.data_ptr(), 9 * P, P,
                                   None, None, 0, P, S_, None) == -1
    if locate_bad:
        assert plan.syndrome_locate_kernels(R, t, P) == ""
        if not 1 <= R <= min(8, m):
            assert lib.qi_gpu_syndrome_locate_ctx_bytes(plan.h, R, S_) == 0
            assert lib.qi_gpu_syndrome_locate_ctx(plan.h, z.data_ptr(), R, S_, ctx.data_ptr(),
                                                  None) == -1
        assert lib.qi_gpu_syndrome_locate(plan.h, ctx.data_ptr(), R, t, out.data_ptr(), 9 * P, P,
                                          None, None, 0, res.data_ptr(), res.data_ptr(),
                                          res.data_ptr(), res.data_ptr(), res.data_ptr(), 1, P,
                                          S_, None) == -1
    torch.cuda.synchronize()
    assert (ctx == 0x5A).all() and (out == FILL).all() and (rows == FILL).all()
    assert (res == 7).all()
    assert plan.take_error() == 0


def test_block_calls_reject(hip_lib):
    import quadiron_amd as qa
    fec = qa.Fec(16, 48, True)
    row = np.zeros(128, np.uint8)
    listed = list(range(20))
    with pytest.raises(ValueError):    # more than min(8, m) checks
        fec.syndrome_blocks(list(range(25)), [0], [row], None, None, 9)
    with pytest.raises(ValueError):    # no held row
        fec.syndrome_blocks(listed, [], [], None, None, 4)
    with pytest.raises(RuntimeError):  # a held fragment that is not listed
        fec.syndrome_blocks(listed, [30], [row], None, None, 4)
    with pytest.raises(RuntimeError):  # a repeated listed id
        fec.syndrome_blocks([0] * 20, [0], [row], None, None, 4)
    with pytest.raises(ValueError):    # max_errors above R / 2
        fec.locate_syndromes(listed, [row] * 4, None, None, max_errors=3)


@pytest.mark.parametrize("k,m,sys_,H,R,t,P", [(16, 48, False, 1, 1, 0, 1024),
                                              (1000, 24, True, 1008, 8, 4, 4099),
                                              (5000, 3000, False, 8, 3, 1, 2056)])
def test_reported_syndrome_kernels_exist(hip_lib, k, m, sys_, H, R, t, P):
    import subprocess
    import quadiron_amd as qa
    out = subprocess.run(["nm", "-DC", qa.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    syms = [ln.split(" ", 2)[2] for ln in out.splitlines() if " qi::" in ln]
    plan = qa.Plan(k, m, sys_)
    for kernels, role in ((plan.syndrome_kernels(H, R, P), "syndrome"),
                          (plan.syndrome_locate_kernels(R, t, P), "syndrome_locate")):
        got, names = kernels.split("=", 1)
        names = [n.strip() for n in names.split(" + ")]
        assert got == role and len(names) == 2, kernels
        for name in names:
            assert any("qi::" + name + "(" in s for s in syms), (name, kernels)
