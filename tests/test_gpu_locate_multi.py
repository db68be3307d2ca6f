"""GPU: multi-fragment locate (qi_gpu_locate_multi).  The codewords come from
the product's own encode (test_gpu_locate's shared truth); every expected
result is known by construction from the injected errors: a column with b <= t
bad listed fragments is located in exactly those, each fix the original
symbol; one with t < b <= R - t is unlocated.  No column with more than R - t
bad fragments is injected, except where both locates are compared (item 3)."""
import numpy as np
import pytest

from test_gpu_locate import (CAP, S, TILE, WIDTHS, _dev_rows, _host_fragments, _i32, _ids,
                             _locate, _store, _torch, _truth)

pytestmark = pytest.mark.gpu

Q = 65537
assert WIDTHS == (1, 7, 2048, 2061, 4097) and S == 3
CODES = [(3, 5, 4, 2), (16, 48, 4, 2), (16, 48, 8, 2), (16, 48, 8, 4), (200, 56, 8, 4),
         (256, 768, 8, 4)]


def _locate_multi(k, m, sys_, R, t, ids, recv, unaligned=False, rows=None, cap=None,
                  fix_cap=None, garbage=()):
    """runs the call over recv; returns (err, located [L, N], unlocated [L],
    weights [L, 4], fix_counts [L], fixes [L, fix_cap, 3])"""
    torch = _torch()
    import quadiron_amd as qa
    plan = qa.Plan(k, m, bool(sys_))
    L, N = ids.shape
    S_all, _, P = recv.shape
    no = plan.n_outputs
    data, coded, marks = _store(k, sys_, recv, garbage)
    cap = cap or max(CAP, max(len(c) for ms in marks for c in ms))
    fix_cap = 4 * P if fix_cap is None else fix_cap
    cnt = np.array([[len(c) for c in ms] for ms in marks], np.uint32)
    ent = np.full((S_all, no, cap), 0xFFFFFFFF, np.uint32)
    for s in range(S_all):
        for j in range(no):
            c = marks[s][j][:cap]
            ent[s, j, :len(c)] = c[::-1]                      # buckets are unordered
    keep = []
    dd = None
    if sys_:
        big, dd = _dev_rows(torch, data, unaligned)
        keep.append(big)
    cbig, dc = _dev_rows(torch, coded, unaligned)
    ctx = torch.randint(0, 256, (plan.locate_ctx_bytes(R, L),), dtype=torch.uint8, device="cuda")
    plan.locate_ctx(torch.from_numpy(ids.view(np.int16)).cuda(), ctx)
    located = torch.full((L * N,), 7, dtype=torch.int32, device="cuda")
    unloc = torch.full((L,), 7, dtype=torch.int32, device="cuda")
    wts = torch.full((L * 4,), 7, dtype=torch.int32, device="cuda")
    fcnt = torch.full((L,), 7, dtype=torch.int32, device="cuda")
    fixes = torch.full((L * max(fix_cap, 1) * 3,), -1, dtype=torch.int32, device="cuda")
    vec = "true" if not unaligned else "false"
    rp = 2 if R <= 2 else 4 if R <= 4 else 8
    if not unaligned:
        assert plan.locate_multi_kernels(R, t, P) == (
            f"locate_multi=locate_ctx_kernel<{rp}> + locate_multi_kernel<{rp}, {vec}>")
    err = plan.locate_multi(ctx, R, t, dc, located, unloc, wts, fcnt,
                            fixes if fix_cap else None, fix_cap, data=dd,
                            counts=_i32(torch, cnt), entries=_i32(torch, ent), cap=cap,
                            stripes=None if rows is None else _i32(torch, rows))
    torch.cuda.synchronize()
    # no row was written
    assert (dc.cpu().numpy().view(np.uint16) == coded).all()
    if sys_:
        assert (dd.cpu().numpy().view(np.uint16) == data).all()
    plan.close()
    return (err, located.cpu().numpy().reshape(L, N), unloc.cpu().numpy(),
            wts.cpu().numpy().reshape(L, 4), fcnt.cpu().numpy(),
            fixes.cpu().numpy().reshape(L, max(fix_cap, 1), 3))


def _expect(truth, recv, ids, R, t, rows=None):
    """per list position: located [N], unlocated, weights [4], fixes"""
    res = []
    for s in range(ids.shape[0]):
        sr = s if rows is None else int(rows[s])
        bad = truth[sr][ids[s]] != recv[sr][ids[s]]           # [N, P]
        nb = bad.sum(axis=0)
        assert nb.max() <= R - t                              # nothing past the guard zone
        loc = np.zeros(ids.shape[1], np.int64)
        wts = np.zeros(4, np.int64)
        fixes = set()
        for c in np.nonzero((nb >= 1) & (nb <= t))[0]:
            wts[nb[c] - 1] += 1
            for p in np.nonzero(bad[:, c])[0]:
                loc[p] += 1
                fixes.add((int(c), int(p), int(truth[sr, ids[s, p], c])))
        res.append((loc, int((nb > t).sum()), wts, fixes))
    return res


def _check(res, exp):
    err, located, unloc, wts, fcnt, fixes = res
    assert err == 0
    for s, (loc, nun, w, fx) in enumerate(exp):
        assert (located[s] == loc).all(), (s, located[s], loc)
        assert unloc[s] == nun, (s, unloc[s], nun)
        assert (wts[s] == w).all(), (s, wts[s], w)
        assert fcnt[s] == len(fx)
        got = [tuple(int(v) for v in f) for f in fixes[s, :fcnt[s]]]
        assert len(set(got)) == len(got) and set(got) == fx, (s, sorted(set(got) ^ fx)[:5])


def _inject(recv, ids, s, c, b, rng, sys_, k):
    """b bad listed fragments in column c of stripe s: other storable symbols"""
    for p in rng.choice(ids.shape[1], b, replace=False):
        f = int(ids[s, p])
        hi = 65536 if sys_ and f < k else Q                   # data rows hold no 65536
        recv[s, f, c] = (recv[s, f, c] + int(rng.integers(1, hi))) % hi


def _columns(P, rng, n):
    edge = list(dict.fromkeys(c for c in (0, TILE - 1, TILE, P - 1) if c < P))
    rest = [int(c) for c in rng.permutation(P)[:n] if c not in edge]
    return edge + rest


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("k,m,R,t", CODES)
def test_weights_up_to_t_and_guard_zone(k, m, R, t, sys_, unaligned):
    """items 1 and 2: weights 1 .. t located exactly, t + 1 .. R - t unlocated,
    at every width, aligned rows and odd-offset odd-stride rows"""
    for P in WIDTHS:
        rng = np.random.default_rng(1000 * k + 10 * R + t + P)
        truth = np.ascontiguousarray(_truth(k, m, sys_)[:, :, :P])
        recv = truth.copy()
        ids = _ids(k, m, R, rng)
        cols = _columns(P, rng, 40)
        for s in range(S):
            for i, c in enumerate(cols):
                _inject(recv, ids, s, c, 1 + (i + s) % (R - t), rng, sys_, k)
        exp = _expect(truth, recv, ids, R, t)
        if P >= TILE:
            assert all(e[2][:t].min() > 0 for e in exp)       # every weight occurs
            assert R == 2 * t or all(e[1] > 0 for e in exp)
        _check(_locate_multi(k, m, sys_, R, t, ids, recv, unaligned=unaligned), exp)


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("R", [2, 4, 8])
def test_max_errors_1_is_the_single_locate(R, sys_):
    """item 3: t = 1 against Plan.locate on identical inputs, R = 2 included
    (there two bad fragments may pass as one: in both alike)"""
    k, m = 16, 48
    for P in (7, 2061):
        rng = np.random.default_rng(50 + R + P)
        truth = np.ascontiguousarray(_truth(k, m, sys_)[:, :, :P])
        recv = truth.copy()
        ids = _ids(k, m, R, rng)
        for s in range(S):
            for i, c in enumerate(_columns(P, rng, 60)):
                _inject(recv, ids, s, c, 1 + i % 3, rng, sys_, k)
        a = _locate(k, m, sys_, R, ids, recv)
        b = _locate_multi(k, m, sys_, R, 1, ids, recv)
        assert a[0] == b[0] == 0
        assert (a[1] == b[1]).all() and (a[2] == b[2]).all() and (a[3] == b[4]).all()
        assert (b[3][:, 0] == b[4]).all() and not b[3][:, 1:].any()
        for s in range(S):
            fa = set(tuple(int(v) for v in f) for f in a[4][s, :a[3][s]])
            fb = set(tuple(int(v) for v in f) for f in b[5][s, :b[4][s]])
            assert fa == fb and len(fa) == a[3][s]
        assert b[4].sum() > 0 and b[2].sum() > 0


def test_smaller_t_widens_the_guard_zone():
    """R = 8, t = 1: weights 2 .. 7 are all unlocated"""
    k, m, R, t, P = 16, 48, 8, 1, 2061
    rng = np.random.default_rng(77)
    truth = np.ascontiguousarray(_truth(k, m, 0)[:, :, :P])
    recv = truth.copy()
    ids = _ids(k, m, R, rng)
    for s in range(S):
        for i, c in enumerate(_columns(P, rng, 40)):
            _inject(recv, ids, s, c, 1 + i % 7, rng, 0, k)
    _check(_locate_multi(k, m, 0, R, t, ids, recv), _expect(truth, recv, ids, R, t))


def _craft(truth, s, f, c, c2):
    """column c of stripe s becomes the codeword a + lam b (columns c, c2) that
    is 65536 in fragment f"""
    a, b = truth[s, :, c].astype(np.int64), truth[s, :, c2].astype(np.int64)
    assert b[f] != 0
    lam = (65536 - a[f]) * pow(int(b[f]), Q - 2, Q) % Q
    cw = (a + lam * b) % Q
    assert cw[f] == 65536
    truth[s, :, c] = cw


@pytest.mark.parametrize("sys_", [0, 1])
def test_marks(sys_):
    """item 4"""
    k, m, R, t, P = 16, 48, 4, 2, 2061
    rng = np.random.default_rng(90 + sys_)
    truth = np.array(_truth(k, m, sys_)[:, :, :P])
    ids = _ids(k, m, R, rng)
    first = k if sys_ else 0
    coded_pos = [[p for p in range(k + R) if ids[s, p] >= first] for s in range(S)]
    s = 0
    pc = coded_pos[s][0]
    fc = int(ids[s, pc])
    # columns 10, 11, 12: the truth is 65536 in coded fragment fc
    for c in (10, 11, 12):
        _craft(truth, s, fc, c, c + 100)
        if sys_:
            assert truth[s, :k, c].max() < 65536
    recv = truth.copy()
    other = int(ids[s, [p for p in range(k + R) if p != pc][3]])
    # 10: the mark is lost (a word stored instead) and a second fragment is bad
    recv[s, fc, 10] = 1234
    recv[s, other, 10] = (recv[s, other, 10] + 5) % 65536
    # 11: garbage is stored under the mark: nothing is wrong there
    garbage = [(s, fc - first, 11, 4321)]
    # 12: the mark is there, another fragment is bad
    recv[s, other, 12] = (recv[s, other, 12] + 9) % 65536
    # 20: a stored mark where the truth has none
    assert truth[s, fc, 20] != 65536
    recv[s, fc, 20] = 65536
    exp = _expect(truth, recv, ids, R, t)
    assert (10, pc, 65536) in exp[0][3] and exp[0][2].tolist() == [2, 1, 0, 0]
    if sys_:
        # 30: the truth is 65536 on a data row (no stored word can say so) and
        # a second, storable error: unlocated as a whole, nothing emitted
        pd = next(p for p in range(k + R) if ids[1, p] < k)
        fd = int(ids[1, pd])
        _craft(truth, 1, fd, 30, 130)
        recv[1, :, 30] = truth[1, :, 30]
        recv[1, fd, 30] = 17
        f2 = int(ids[1, coded_pos[1][0]])
        recv[1, f2, 30] = (recv[1, f2, 30] + 3) % Q
        loc, nun, w, fx = exp[1]
        exp[1] = (loc, nun + 1, w, fx)
    res = _locate_multi(k, m, sys_, R, t, ids, recv, garbage=garbage)
    _check(res, exp)
    # a bucket over oor_cap raises bit 1
    recv2 = recv.copy()
    recv2[0, fc, 40] = 65536
    recv2[0, fc, 41] = 65536
    assert (recv2[0, fc] == 65536).sum() >= 5
    res = _locate_multi(k, m, sys_, R, t, ids, recv2, cap=4)
    assert res[0] & 1


@pytest.mark.parametrize("sys_", [0, 1])
def test_dense(sys_):
    """item 5: one fragment bad in every column, a second error in 64 columns"""
    k, m, R, t, P = 16, 48, 4, 2, 4097
    rng = np.random.default_rng(5 + sys_)
    truth = np.ascontiguousarray(_truth(k, m, sys_)[:, :, :P])
    recv = truth.copy()
    ids = _ids(k, m, R, rng)
    second = np.sort(rng.permutation(P)[:64])
    for s in range(S):
        p = 3 + s
        f = int(ids[s, p])
        hi = 65536 if sys_ and f < k else Q
        recv[s, f] = (recv[s, f] + rng.integers(1, hi, P)) % hi
        for c in second:
            q = int(rng.choice([i for i in range(k + R) if i != p]))
            f2 = int(ids[s, q])
            hi2 = 65536 if sys_ and f2 < k else Q
            recv[s, f2, c] = (recv[s, f2, c] + int(rng.integers(1, hi2))) % hi2
    exp = _expect(truth, recv, ids, R, t)
    for s in range(S):
        assert exp[s][0][3 + s] == P and exp[s][2].tolist() == [P - 64, 64, 0, 0]
    _check(_locate_multi(k, m, sys_, R, t, ids, recv), exp)


def test_fix_cap():
    """item 6: the count is exact past fix_cap, kept entries are valid, the
    kept entries of a column are adjacent; fix_cap = 0 with no list"""
    k, m, R, t, P = 16, 48, 4, 2, 2061
    rng = np.random.default_rng(6)
    truth = np.ascontiguousarray(_truth(k, m, 0)[:, :, :P])
    recv = truth.copy()
    ids = _ids(k, m, R, rng)
    for s in range(S):
        for c in _columns(P, rng, 60):
            _inject(recv, ids, s, c, 2, rng, 0, k)
    exp = _expect(truth, recv, ids, R, t)
    full = _locate_multi(k, m, 0, R, t, ids, recv)
    _check(full, exp)
    for s in range(S):                                        # adjacency, full list
        f = full[5][s, :full[4][s]]
        assert (f[0::2, 0] == f[1::2, 0]).all()
    fc = 31                                                   # odd: one column is cut
    res = _locate_multi(k, m, 0, R, t, ids, recv, fix_cap=fc)
    assert res[0] == 0
    for s in range(S):
        assert res[4][s] == len(exp[s][3]) > fc
        kept = [tuple(int(v) for v in f) for f in res[5][s]]
        assert len(set(kept)) == fc and set(kept) <= exp[s][3]
        cols = [c for c, _, _ in kept]
        for c in set(cols):                                   # one run per column
            idx = [i for i, x in enumerate(cols) if x == c]
            assert idx == list(range(idx[0], idx[0] + len(idx)))
    res = _locate_multi(k, m, 0, R, t, ids, recv, fix_cap=0)
    assert res[0] == 0 and (res[5] == -1).all()
    for s in range(S):
        assert res[4][s] == len(exp[s][3]) and (res[1][s] == exp[s][0]).all()


@pytest.mark.parametrize("sys_", [0, 1])
def test_stripe_list(sys_):
    """item 7: d_stripes lists two of the three stripes"""
    k, m, R, t, P = 16, 48, 8, 4, 2061
    rng = np.random.default_rng(8 + sys_)
    truth = np.ascontiguousarray(_truth(k, m, sys_)[:, :, :P])
    recv = truth.copy()
    rows = np.array([2, 0], np.uint32)
    ids = _ids(k, m, R, rng, n=2)
    for l, sr in enumerate(rows):
        for i, c in enumerate(_columns(P, rng, 30)):
            bad = rng.choice(k + R, 1 + i % 4, replace=False)
            for p in bad:
                f = int(ids[l, p])
                hi = 65536 if sys_ and f < k else Q
                recv[sr, f, c] = (recv[sr, f, c] + int(rng.integers(1, hi))) % hi
    recv[1] = (recv[1] + 1) % 65536                           # the unlisted stripe is not read
    exp = _expect(truth, recv, ids, R, t, rows=rows)
    _check(_locate_multi(k, m, sys_, R, t, ids, recv, rows=rows), exp)


def test_bad_arguments():
    """item 8"""
    torch = _torch()
    import quadiron_amd as qa
    plan = qa.Plan(16, 48, False)
    lib = qa.lib()
    buf = torch.full((4096,), 7, dtype=torch.int32, device="cuda")
    rows = torch.zeros((1, 64, 8), dtype=torch.int16, device="cuda")

    def call(p, R, t):
        return lib.qi_gpu_locate_multi(p.h, buf.data_ptr(), R, t, None, None, 0, 0,
                                       rows.data_ptr(), 512, 8, None, None, 0, buf.data_ptr(),
                                       buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None, 0,
                                       8, 1, None)
    for R, t in ((4, 0), (4, 3), (8, 5), (2, 2), (5, 3), (1, 1), (9, 4), (4, -1)):
        assert call(plan, R, t) == -1, (R, t)
        assert plan.locate_multi_kernels(R, t, 64) == ""
    torch.cuda.synchronize()
    assert (buf == 7).all()                                   # outputs untouched
    assert plan.locate_multi_kernels(5, 2, 64) == (
        "locate_multi=locate_ctx_kernel<8> + locate_multi_kernel<8, true>")
    assert plan.locate_multi_kernels(2, 1, 64) == (
        "locate_multi=locate_ctx_kernel<2> + locate_multi_kernel<2, true>")
    plan.close()
    big = qa.Plan(300, 212, False)
    assert big.locate_multi_kernels(4, 2, 64) == ""
    rows = torch.zeros((1, 512, 8), dtype=torch.int16, device="cuda")
    assert call(big, 4, 2) == -5                              # QI_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (buf == 7).all()
    big.close()


@pytest.mark.parametrize("sys_", [0, 1])
def test_fec_locate_blocks_max_errors(sys_):
    """item 9: two bad fragments in a column are restored with max_errors=2;
    without max_errors the call and its result are the single locate's"""
    import quadiron_amd as qa
    _torch()
    k, m = 16, 48
    P = 1024 + 40
    rng = np.random.default_rng(140 + sys_)
    truth, rows, oor, cnt = _host_fragments(k, m, sys_, P, rng)
    first = k if sys_ else 0
    miss = np.zeros(k + m, np.int32)
    miss[[1, 17, 20]] = 1
    present = [f for f in range(k + m) if not miss[f]]
    listed = present[:k + 8]
    clean_rows = [r.copy() for r in rows]
    clean_oor, clean_cnt = oor.copy(), cnt.copy()

    def args():
        data = [None if miss[f] else rows[f] for f in range(k)] if sys_ else None
        pars = [None if miss[first + j] else rows[first + j] for j in range(k + m - first)]
        return data, pars

    fec = qa.Fec(k, m, bool(sys_))
    exp = np.full(k + m + 1 + 2, -1, np.int64)
    exp[listed] = 0
    exp[k + m:] = 0
    assert fec.locate_blocks(*args(), oor, cnt, miss, max_errors=2).tolist() == exp.tolist()
    # fragment A is bad in 200 columns (more fixes than the first attempt's
    # list), fragment B in 30 of them and in 10 others
    fa, fb = listed[2], listed[-1]
    ok = [c for c in range(P) if truth[fa, c] != 65536 and truth[fb, c] != 65536]
    ca = rng.permutation(ok)[:210]
    for c in ca[:200]:
        rows[fa].view(np.uint16)[c] ^= 0x0101
    for c in ca[170:210]:
        rows[fb].view(np.uint16)[c] ^= 0x1000
    exp[fa], exp[fb] = 200, 40
    exp[k + m + 1], exp[k + m + 2] = 180, 30
    snap = [r.copy() for r in rows]
    # today's call: the 30 shared columns are unlocated, nothing is patched
    res, patched = fec.locate_blocks(*args(), oor, cnt, miss, correct=True)
    old = np.full(k + m + 1, -1, np.int64)
    old[listed] = 0
    old[fa], old[fb], old[-1] = 170, 10, 30
    assert not patched and res.tolist() == old.tolist()
    assert all((a == b).all() for a, b in zip(rows, snap))
    assert fec.locate_blocks(*args(), oor, cnt, miss, max_errors=2).tolist() == exp.tolist()
    res, patched = fec.locate_blocks(*args(), oor, cnt, miss, correct=True, max_errors=2)
    assert patched and res.tolist() == exp.tolist()
    for f in present:
        assert (rows[f] == clean_rows[f]).all(), f
    assert (cnt == clean_cnt).all()
    for j in range(len(cnt)):
        assert (oor[j, :cnt[j]] == clean_oor[j, :cnt[j]]).all(), j
    # three bad fragments in one column at t = 2 (R = 8): unlocated, not patched
    c = int(ca[0])
    for f in (listed[0], listed[5], listed[9]):
        assert truth[f, c] != 65536
        rows[f].view(np.uint16)[c] ^= 1
    snap = [r.copy() for r in rows]
    res, patched = fec.locate_blocks(*args(), oor, cnt, miss, correct=True, max_errors=2)
    assert not patched and res[k + m] == 1 and res[listed].sum() == 0
    assert all((a == b).all() for a, b in zip(rows, snap))
    # R = 8 < 2 * 5 cannot be asked for; R = 2 < 2 * 2: nothing to locate with
    with pytest.raises(ValueError):
        fec.locate_blocks(*args(), oor, cnt, miss, max_errors=5)
    miss2 = np.ones(k + m, np.int32)
    miss2[present[:k + 2]] = 0
    miss = miss2
    assert fec.locate_blocks(*args(), oor, cnt, miss, max_errors=2) is None
    assert fec.locate_blocks(*args(), oor, cnt, miss, max_errors=1) is not None
    fec.close()
