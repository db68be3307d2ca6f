"""GPU: partial repair (qi_gpu_partial_ctx / qi_gpu_partial,
Fec.partial_repair_blocks).  The model of one call is
  matvec_mod(repair_matrix(...)[:, held], restored rows) + acc  mod 65537
with the oracle's repair matrix, compared exactly, the set of 65536 positions
included; complete sums are compared with the oracle's encoded rows and with
the fused repair.  Nothing expected here comes from the code under test."""
import functools

import numpy as np
import pytest

from qi_testlib import (FILL, Q, balanced_np, craft_oor_columns, matvec_mod,
                        oracle_encode_blocks, repair_matrix, retry_block)

pytestmark = pytest.mark.gpu

CAP = 1024
TILE = 2048      # the kernel's column tile
WORDS = 2952     # one whole tile and a 904-column tail
MARK = 65536


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    torch.cuda.set_device(0)
    return torch


def _dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda()


def _rows_dev(torch, arr, unaligned=False):
    """(backing, view): the [S, rows, P] device view of arr inside a FILL-filled
    backing with a guard row before and after and guard columns on both sides;
    unaligned: at an odd u16 offset with a row stride that is no multiple of 8"""
    S, rows, P = arr.shape
    W, lead = P, 0
    if unaligned:
        W = P + 4 + (1 if (P + 4) % 8 == 0 else 0)
        lead = 1 if W % 2 == 0 else 2       # the view starts W + lead words in: odd
    big = torch.full((S, rows + 2, W), FILL, dtype=torch.int16, device="cuda")
    view = big[:, 1:rows + 1, lead:lead + P]
    view.copy_(_dev16(torch, arr))
    if unaligned:
        assert view.data_ptr() % 4 == 2 and view.stride(1) % 8 != 0
    else:
        assert view.data_ptr() % 16 == 0 or P % 8
    return big, view


def _guards_intact(big, view):
    """every word of the backing outside the view still holds FILL"""
    g = big.cpu().numpy().view(np.uint16).copy()
    rows, P = view.shape[1], view.shape[2]
    lead = view.storage_offset() % big.stride(1)
    g[:, 1:rows + 1, lead:lead + P] = FILL
    return bool((g == FILL).all())


def _buckets(torch, marks, cap):
    """marks[s][j]: the columns of bucket (s, j) -> counts, entries"""
    S, J = len(marks), len(marks[0])
    cnt = np.zeros((S, J), np.uint32)
    ent = np.zeros((S, J, cap), np.uint32)
    for s in range(S):
        for j in range(J):
            cols = list(marks[s][j])
            cnt[s, j] = len(cols)
            ent[s, j, :min(len(cols), cap)] = cols[:cap]
    return (torch.from_numpy(cnt.view(np.int32).reshape(-1)).cuda(),
            torch.from_numpy(ent.view(np.int32).reshape(-1)).cuda())


def _read_buckets(counts, entries, S, J, cap):
    cnt = counts.cpu().numpy().view(np.uint32).reshape(S, J)
    ent = entries.cpu().numpy().view(np.uint32).reshape(S, J, cap)
    return cnt, [[set(int(v) for v in ent[s, j, :min(cnt[s, j], cap)]) for j in range(J)]
                 for s in range(S)]


def _context(torch, plan, ids, held, targets):
    S, H = held.shape
    R = targets.shape[1]
    nb = plan.partial_ctx_bytes(H, R, S)
    RP = {1: 1, 2: 2, 3: 4, 4: 4}.get(R, 8)
    assert nb == S * 4 * (H * RP + RP + H)
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    plan.partial_ctx(_dev16(torch, ids), _dev16(torch, held), _dev16(torch, targets), ctx)
    return ctx


def _partial(torch, plan, ids, held, targets, rows, marks, acc=None, acc_marks=None,
             unaligned=False, cap=CAP, out_cap=CAP, null_in=False):
    """One call.  rows [S, H, P] u16 with marks[s][h]; acc [S, R, P] u16 with
    acc_marks[s][t] (None: no acc), in place.  Returns (rows u16 [S, R, P],
    counts [S, R], mark sets [S][R])."""
    S, H, P = rows.shape
    R = targets.shape[1]
    ctx = _context(torch, plan, ids, held, targets)
    rbig, drows = _rows_dev(torch, rows, unaligned)
    counts, entries = (None, None) if null_in else _buckets(torch, marks, cap)
    if acc is not None:
        obig, out = _rows_dev(torch, acc, unaligned)
        ac, ae = _buckets(torch, acc_marks, cap)
    else:
        obig, out = _rows_dev(torch, np.full((S, R, P), FILL, np.uint16), unaligned)
        ac = ae = None
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.full((S * R * out_cap,), -1, dtype=torch.int32, device="cuda")
    err = plan.partial(ctx, drows, out, acc=out if acc is not None else None, counts=counts,
                       entries=entries, cap=cap if counts is not None else 0, acc_counts=ac,
                       acc_entries=ae, acc_cap=cap if ac is not None else 0, out_counts=oc,
                       out_entries=oe, out_cap=out_cap)
    torch.cuda.synchronize()
    assert err == 0
    assert _guards_intact(rbig, drows) and _guards_intact(obig, out)
    assert (drows.cpu().numpy().view(np.uint16) == rows).all()   # read only
    got = out.cpu().numpy().view(np.uint16).copy()
    cnt, sets = _read_buckets(oc, oe, S, R, out_cap)
    return got, cnt, sets


def _restored(rows, marks):
    """[rows, P] int64 symbols: 65536 at the marked columns"""
    y = rows.astype(np.int64)
    for h, cols in enumerate(marks):
        if len(cols):
            y[h, list(cols)] = MARK
    return y


@functools.lru_cache(maxsize=None)
def _matrix(k, m, sys_, ids, targets):
    M = repair_matrix(k, m, sys_, np.array(ids), np.array(targets))
    M.setflags(write=False)
    return M


def _model(k, m, sys_, ids, held, targets, rows, marks, acc=None, acc_marks=None):
    """the expected [R, P] symbols of one stripe, in [0, 65536]"""
    M = _matrix(k, m, sys_, tuple(int(v) for v in ids), tuple(int(v) for v in targets))
    y = _restored(rows, marks)
    out = matvec_mod(M[:, held.astype(np.int64)], y)
    if acc is not None:
        out = (out + _restored(acc, acc_marks)) % Q
    return out


def _check(got, cnt, sets, exp, s):
    """one stripe's rows, counts and mark sets against the model symbols"""
    for t in range(exp.shape[0]):
        assert (got[s, t] == (exp[t] & 0xffff)).all(), (s, t, np.flatnonzero(
            got[s, t] != (exp[t] & 0xffff))[:8])
        em = set(int(v) for v in np.flatnonzero(exp[t] == MARK))
        assert cnt[s, t] == len(em), (s, t, cnt[s, t], len(em))
        assert sets[s][t] == em, (s, t)


def _pick(k, m, H, R, S, rng):
    """ids [S, k], held positions [S, H] (unordered) and targets [S, R], all
    differing per stripe"""
    ids, held, targets = [], [], []
    for _ in range(S):
        perm = rng.permutation(k + m)
        ids.append(perm[:k])
        targets.append(perm[k:k + R])
        held.append(rng.permutation(k)[:H])
    return (np.array(ids, np.uint16), np.array(held, np.uint16), np.array(targets, np.uint16))


def _data_row(sys_, k, fid):
    return bool(sys_) and fid < k


# ---- 1. against the model ------------------------------------------------

@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("H", [1, 5, 16])
@pytest.mark.parametrize("sys_", [0, 1])
def test_partial_vs_model(hip_lib, sys_, H, R, with_acc):
    torch = _torch()
    import quadiron_amd as qa
    k, m, S, P = 16, 48, 3, WORDS
    rng = np.random.default_rng([sys_, H, R, int(with_acc), 1])
    ids, held, targets = _pick(k, m, H, R, S, rng)
    rows = rng.integers(0, 65536, (S, H, P), dtype=np.uint16)
    acc = rng.integers(0, 65536, (S, R, P), dtype=np.uint16) if with_acc else None
    # columns 0 .. 8 R of the tile and of the tail are kept for the crafting
    free = np.concatenate([np.arange(8 * R + 8, TILE), np.arange(TILE + 8 * R + 8, P)])
    marks = [[[] for _ in range(H)] for _ in range(S)]
    acc_marks = [[[] for _ in range(R)] for _ in range(S)] if with_acc else None
    for s in range(S):
        for h in range(H):
            cols = [int(v) for v in rng.choice(free, 4, replace=False)] + [TILE - 1, P - 1]
            if _data_row(sys_, k, ids[s, held[s, h]]):
                # a data row has no marks: its bucket holds rubbish, never read
                marks[s][h] = cols
                continue
            marks[s][h] = cols
            rows[s, h, cols] = 0
        for t in range(R if with_acc else 0):
            cols = [int(v) for v in rng.choice(free, 3, replace=False)] + [TILE, 0]
            acc_marks[s][t] = cols
            acc[s, t, cols] = 0
    true_marks = [[[] if _data_row(sys_, k, ids[s, held[s, h]]) else marks[s][h]
                   for h in range(H)] for s in range(S)]
    # craft: one held symbol per chosen column so that the partial is 65536
    for s in range(S):
        M = _matrix(k, m, sys_, tuple(int(v) for v in ids[s]), tuple(int(v) for v in targets[s]))
        for t in range(R):
            for c in [1 + 4 * t + i for i in range(4)] + [TILE + 1 + 4 * t + i for i in range(4)]:
                hs = int(rng.integers(0, H))
                co = int(M[t, held[s, hs]])
                assert co != 0
                rows[s, hs, c] = 0
                base = _model(k, m, sys_, ids[s], held[s], targets[s], rows[s][:, c:c + 1],
                              [[] for _ in range(H)],
                              acc[s][:, c:c + 1] if with_acc else None,
                              [[] for _ in range(R)] if with_acc else None)[t, 0]
                y = (MARK - int(base)) * pow(co, Q - 2, Q) % Q
                if y < MARK:
                    rows[s, hs, c] = y
    got, cnt, sets = _partial(torch, qa.Plan(k, m, bool(sys_)), ids, held, targets, rows, marks,
                              acc, acc_marks)
    for s in range(S):
        exp = _model(k, m, sys_, ids[s], held[s], targets[s], rows[s], true_marks[s],
                     acc[s] if with_acc else None, acc_marks[s] if with_acc else None)
        for t in range(R):
            em = np.flatnonzero(exp[t] == MARK)
            assert len(em) >= 3 and (em < TILE).any() and (em >= TILE).any(), (s, t, em)
        _check(got, cnt, sets, exp, s)


# ---- 2. partition independence, the fused repair, the oracle --------------

def _fragments(k, m, sys_, data, cap=CAP):
    """one stripe's fragments by id: rows u16 [k + m, P], their mark lists, and
    the oracle's (outputs u16, oor, counts)"""
    P = data.shape[1]
    o, oor, cnt = oracle_encode_blocks(
        k, m, sys_, np.ascontiguousarray(data).view(np.uint8).reshape(k, 2 * P), cap)
    assert cnt.max() <= cap
    o16 = o.view(np.uint16).reshape(-1, P)[:(m if sys_ else k + m)]
    coded_marks = [[int(v) for v in oor[j, :cnt[j]]] for j in range(o16.shape[0])]
    if sys_:
        return np.concatenate([data, o16]), [[] for _ in range(k)] + coded_marks, (o16, oor, cnt)
    return o16, coded_marks, (o16, oor, cnt)


def _chain(torch, plan, ids, targets, groups, frows, fmarks, unaligned=False):
    """groups: per link the positions [S, H_link]; every link adds its share to
    the same R rows, in place through acc.  Returns the final (rows, counts,
    mark sets)."""
    S = ids.shape[0]
    acc = acc_marks = None
    for held in groups:
        rows = np.stack([frows[s][ids[s][held[s].astype(np.int64)]] for s in range(S)])
        marks = [[fmarks[s][int(ids[s][p])] for p in held[s]] for s in range(S)]
        got, cnt, sets = _partial(torch, plan, ids, held, targets, rows, marks, acc, acc_marks,
                                  unaligned=unaligned)
        acc, acc_marks = got, [[sorted(x) for x in row] for row in sets]
    return got, cnt, sets


def _splits(k, S, rng, sizes):
    perm = [rng.permutation(k) for _ in range(S)]
    out, at = [], 0
    for n in sizes:
        out.append(np.array([p[at:at + n] for p in perm], np.uint16))
        at += n
    assert at == k
    return out


@pytest.mark.parametrize("sys_", [0, 1])
def test_partial_partitions_equal_repair_and_oracle(hip_lib, sys_):
    torch = _torch()
    import quadiron_amd as qa
    k, m, S, P, R = 16, 48, 2, WORDS, 3
    rng = np.random.default_rng([sys_, 2])
    no = m if sys_ else k + m
    first = k if sys_ else 0
    ids, targets = [], []
    for s in range(S):
        perm = rng.permutation(k + m)
        if sys_:   # a data row among the targets, data rows and parities among the helpers
            rest = perm[perm != 3 + s]
            targets.append(np.concatenate([[3 + s], rest[k:k + R - 1]]))
            ids.append(rest[:k])
            assert (ids[s] < k).any() and (ids[s] >= k).any()
        else:
            ids.append(perm[:k])
            targets.append(perm[k:k + R])
    ids, targets = np.array(ids, np.uint16), np.array(targets, np.uint16)
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    frows, fmarks, enc = [], [], []
    for s in range(S):
        slots = [int(f) - first for f in list(targets[s]) + list(ids[s][:4]) if f >= first]
        craft_oor_columns(k, m, sys_, data[s], rng, 24, rows=slots)
        fr, fm, e = _fragments(k, m, sys_, data[s])
        frows.append(fr), fmarks.append(fm), enc.append(e)
        assert sum(len(fm[int(f)]) for f in targets[s]) >= 3
        assert sum(len(fm[int(f)]) for f in ids[s]) >= 3
    plan = qa.Plan(k, m, bool(sys_))
    a = _chain(torch, plan, ids, targets, _splits(k, S, rng, (1, 5, k - 6)), frows, fmarks)
    b = _chain(torch, plan, ids, targets, _splits(k, S, rng, (k - 6, 1, 5)), frows, fmarks)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]
    # the oracle's encoded rows (a data-row target: the data, no marks)
    for s in range(S):
        for t, f in enumerate(int(v) for v in targets[s]):
            assert (a[0][s, t] == frows[s][f]).all(), (s, f)
            assert a[2][s][t] == set(fmarks[s][f]) and a[1][s, t] == len(fmarks[s][f]), (s, f)
            if sys_ and f < k:
                assert (a[0][s, t] == data[s, f]).all() and a[1][s, t] == 0
    # the fused repair
    coded = _dev16(torch, np.stack([e[0] for e in enc]))
    dd = _dev16(torch, data) if sys_ else None
    counts = torch.from_numpy(np.stack([e[2][:no] for e in enc]).astype(np.uint32)
                              .view(np.int32).reshape(-1)).cuda()
    entries = torch.from_numpy(np.stack([e[1][:no] for e in enc]).astype(np.uint32)
                               .view(np.int32).reshape(-1)).cuda()
    di, dt = _dev16(torch, ids), _dev16(torch, targets)
    ctx = torch.zeros(plan.repair_ctx_bytes(R, S, P), dtype=torch.uint8, device="cuda")
    plan.repair_ctx(di, dt, ctx, P, counts, entries, CAP)
    out = torch.zeros((S, R, P), dtype=torch.int16, device="cuda")
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * R * CAP, dtype=torch.int32, device="cuda")
    assert plan.repair(ctx, coded, out, data=dd, counts=counts, entries=entries, cap=CAP,
                       out_counts=oc, out_entries=oe, out_cap=CAP) == 0
    rc, rsets = _read_buckets(oc, oe, S, R, CAP)
    assert (out.cpu().numpy().view(np.uint16) == a[0]).all()
    assert (rc == a[1]).all() and rsets == a[2]


# ---- 3. wide codes ---------------------------------------------------------

def _wide_case(k, m, sys_, P):
    """ids [1, k], targets [1, 2] (a data row and a parity where systematic)
    and the oracle's fragments, with marks crafted on the targets and on four
    helpers"""
    rng = np.random.default_rng([k, m, sys_, 3])
    first = k if sys_ else 0
    perm = rng.permutation(k + m)
    if sys_:
        tg = np.array([int(perm[perm < k][0]), int(perm[perm >= k][0])])
    else:
        tg = perm[:2]
    ids = perm[~np.isin(perm, tg)][:k]
    data = rng.integers(0, 65536, (k, P), dtype=np.uint16)
    # (systematic: the helpers hold every parity but the target)
    helpers = [int(f) for f in ids if f >= first][-4:]
    for frags, cols in (([int(f) for f in tg if f >= first], (0, P // 2)), (helpers, (P // 2, P))):
        craft_oor_columns(k, m, sys_, data, rng, 12, rows=[f - first for f in frags],
                          col_range=cols)
    fr, fm, _ = _fragments(k, m, sys_, data, cap=256)
    assert sum(len(fm[int(f)]) for f in tg) >= 3
    assert sum(len(fm[f]) for f in helpers) >= 3
    return ids[None].astype(np.uint16), tg[None].astype(np.uint16), fr, fm, rng


@pytest.mark.parametrize("k,m,sys_", [(300, 212, 0), (1000, 24, 1), (5000, 3000, 0)])
def test_partial_wide_codes(hip_lib, k, m, sys_):
    torch = _torch()
    import quadiron_amd as qa
    P, S = 2056, 1
    ids, tg, fr, fm, rng = _wide_case(k, m, sys_, P)
    got, cnt, sets = _chain(torch, qa.Plan(k, m, bool(sys_)), ids, tg,
                            _splits(k, S, rng, (8, k - 8)), [fr], [fm])
    for t, f in enumerate(int(v) for v in tg[0]):
        assert (got[0, t] == fr[f]).all(), (f, np.flatnonzero(got[0, t] != fr[f])[:8])
        assert sets[0][t] == set(fm[f]) and cnt[0, t] == len(fm[f]), f


# ---- 4. unaligned layout ---------------------------------------------------

@pytest.mark.parametrize("R", [1, 4, 8])
def test_partial_unaligned_layout(hip_lib, R):
    torch = _torch()
    import quadiron_amd as qa
    k, m, sys_, S, P, H = 16, 48, 0, 2, WORDS, 5
    rng = np.random.default_rng([R, 4])
    ids, held, targets = _pick(k, m, H, R, S, rng)
    rows = rng.integers(0, 65536, (S, H, P), dtype=np.uint16)
    acc = rng.integers(0, 65536, (S, R, P), dtype=np.uint16)
    marks = [[[int(v) for v in rng.choice(P, 5, replace=False)] for _ in range(H)]
             for _ in range(S)]
    acc_marks = [[[int(v) for v in rng.choice(P, 5, replace=False)] for _ in range(R)]
                 for _ in range(S)]
    plan = qa.Plan(k, m, False)
    a = _partial(torch, plan, ids, held, targets, rows, marks, acc, acc_marks)
    b = _partial(torch, plan, ids, held, targets, rows, marks, acc, acc_marks, unaligned=True)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]
    for s in range(S):
        _check(b[0], b[1], b[2], _model(k, m, sys_, ids[s], held[s], targets[s], rows[s],
                                        marks[s], acc[s], acc_marks[s]), s)


# ---- 5. dense marks --------------------------------------------------------

def test_partial_dense_marks(hip_lib):
    """600 consecutive marks on one held row and on one acc row across the
    tile boundary"""
    torch = _torch()
    import quadiron_amd as qa
    k, m, sys_, S, P, H, R = 16, 48, 0, 2, WORDS, 5, 3
    rng = np.random.default_rng(5)
    ids, held, targets = _pick(k, m, H, R, S, rng)
    rows = rng.integers(0, 65536, (S, H, P), dtype=np.uint16)
    acc = rng.integers(0, 65536, (S, R, P), dtype=np.uint16)
    dense = [int(v) for v in rng.permutation(np.arange(TILE - 300, TILE + 300))]
    marks = [[dense if h == 1 + s else [] for h in range(H)] for s in range(S)]
    acc_marks = [[dense[::-1] if t == s else [7] for t in range(R)] for s in range(S)]
    got, cnt, sets = _partial(torch, qa.Plan(k, m, False), ids, held, targets, rows, marks, acc,
                              acc_marks)
    for s in range(S):
        _check(got, cnt, sets, _model(k, m, sys_, ids[s], held[s], targets[s], rows[s],
                                      marks[s], acc[s], acc_marks[s]), s)


# ---- 6. range extremes -----------------------------------------------------

def test_partial_range_extremes(hip_lib):
    """H = 8, every held symbol from {0, 1, 32768, 32769, 65535, mark} against
    coefficients within 768 of +-32768 (found by a search over ids), from an
    acc of 65536 everywhere; exact against Python integers."""
    torch = _torch()
    import quadiron_amd as qa
    k, m, sys_, H, R, P = 16, 48, 0, 8, 1, 6 ** 4 + 6
    rng = np.random.default_rng(6)
    found = {}
    for _ in range(4000):
        perm = rng.permutation(k + m)
        ids, tg = perm[:k], perm[k:k + 1]
        b = balanced_np(_matrix(k, m, sys_, tuple(int(v) for v in ids), (int(tg[0]),)))[0]
        i = int(np.argmax(np.abs(b)))
        sign = 1 if b[i] > 0 else -1
        if abs(int(b[i])) >= 32000 and sign not in found:
            found[sign] = (ids, tg, i, int(b[i]))
        if len(found) == 2:
            break
    assert set(found) == {1, -1}, found
    cases = [found[1], found[-1]]
    S = len(cases)
    ids = np.array([c[0] for c in cases], np.uint16)
    targets = np.array([c[1] for c in cases], np.uint16)
    held = np.array([[c[2]] + [int(p) for p in np.setdiff1d(np.arange(k), [c[2]])[:H - 1]]
                     for c in cases], np.uint16)
    for s, c in enumerate(cases):
        M = _matrix(k, m, sys_, tuple(int(v) for v in ids[s]), (int(targets[s, 0]),))
        assert abs(int(balanced_np(M)[0, held[s, 0]])) >= 32000
    # columns: every combination of the six symbols on rows 0 .. 3 (rows 4 .. 7
    # repeat them rolled), then all eight rows at the same symbol
    sym = np.array([0, 1, 32768, 32769, 65535, MARK], np.int64)
    grid = np.stack(np.meshgrid(*[sym] * 4, indexing="ij")).reshape(4, -1)
    y = np.concatenate([np.concatenate([grid, np.roll(grid, 1, axis=0)]),
                        np.tile(sym, (H, 1))], axis=1)
    assert y.shape == (H, P)
    rows = np.tile((y & 0xffff).astype(np.uint16), (S, 1, 1))
    rows[np.tile(y == MARK, (S, 1, 1))] = 0
    marks = [[[int(c) for c in np.flatnonzero(y[h] == MARK)] for h in range(H)] for _ in range(S)]
    acc = np.zeros((S, R, P), np.uint16)
    acc_marks = [[list(range(P))] for _ in range(S)]
    got, cnt, sets = _partial(torch, qa.Plan(k, m, False), ids, held, targets, rows, marks, acc,
                              acc_marks, cap=2048, out_cap=2048)
    for s in range(S):
        M = _matrix(k, m, sys_, tuple(int(v) for v in ids[s]), (int(targets[s, 0]),))
        co = [int(M[0, p]) for p in held[s]]
        exp = np.array([[(MARK + sum(c * int(v) for c, v in zip(co, y[:, col]))) % Q
                         for col in range(P)]], np.int64)
        _check(got, cnt, sets, exp, s)


# ---- 7. errors -------------------------------------------------------------

BAD = ["id_high", "id_repeated", "pos_high", "pos_repeated", "target_high", "target_repeated",
       "target_is_helper"]


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("what", BAD)
def test_partial_bad_ids(hip_lib, sys_, what):
    torch = _torch()
    import quadiron_amd as qa
    k, m, H, R, S, P = 16, 48, 3, 2, 2, 2100
    plan = qa.Plan(k, m, bool(sys_))
    ids = np.stack([np.arange(2, 2 + k), np.arange(40, 40 + k)]).astype(np.uint16)
    held = np.array([[0, 7, 15], [3, 1, 2]], np.uint16)
    targets = np.array([[0, 60], [1, 63]], np.uint16)
    if what == "id_high":
        ids[1, 5] = k + m
    elif what == "id_repeated":
        ids[0, 9] = ids[0, 2]
    elif what == "pos_high":
        held[1, 1] = k
    elif what == "pos_repeated":
        held[0, 2] = held[0, 0]
    elif what == "target_high":
        targets[0, 1] = k + m
    elif what == "target_repeated":
        targets[1, 1] = targets[1, 0]
    else:
        targets[0, 0] = ids[0, 4]
    ctx = _context(torch, plan, ids, held, targets)
    torch.cuda.synchronize()
    assert plan.take_error() == 2
    assert plan.take_error() == 0
    # the result of such a stripe is unspecified but stays inside the rows
    rbig, rows = _rows_dev(torch, np.ones((S, H, P), np.uint16))
    obig, out = _rows_dev(torch, np.ones((S, R, P), np.uint16))
    plan.partial(ctx, rows, out, acc=out, check=False)
    torch.cuda.synchronize()
    assert _guards_intact(rbig, rows) and _guards_intact(obig, out)
    assert (rows.cpu().numpy().view(np.uint16) == 1).all()


def _small(torch, k=16, m=48, H=2, R=2, S=1, P=64):
    import quadiron_amd as qa
    plan = qa.Plan(k, m, False)
    ids = np.tile(np.arange(k, dtype=np.uint16), (S, 1))
    held = np.tile(np.arange(H, dtype=np.uint16), (S, 1))
    targets = np.tile(np.arange(k, k + R, dtype=np.uint16), (S, 1))
    ctx = _context(torch, plan, ids, held, targets)
    rows = torch.zeros((S, H, P), dtype=torch.int16, device="cuda")
    out = torch.zeros((S, R, P), dtype=torch.int16, device="cuda")
    return plan, ctx, rows, out


@pytest.mark.parametrize("which", ["in", "acc"])
def test_partial_bucket_over_capacity(hip_lib, which):
    torch = _torch()
    H, R, cap = 2, 2, 4
    plan, ctx, rows, out = _small(torch, H=H, R=R)
    counts = torch.zeros(H, dtype=torch.int32, device="cuda")
    entries = torch.zeros(H * cap, dtype=torch.int32, device="cuda")
    ac = torch.zeros(R, dtype=torch.int32, device="cuda")
    ae = torch.zeros(R * cap, dtype=torch.int32, device="cuda")
    over = counts if which == "in" else ac
    over[1] = cap + 1

    def run():
        return plan.partial(ctx, rows, out, acc=out, counts=counts, entries=entries, cap=cap,
                            acc_counts=ac, acc_entries=ae, acc_cap=cap)
    assert run() == 1
    assert plan.take_error() == 0
    over[1] = cap
    assert run() == 0


def test_partial_out_count_goes_past_cap(hip_lib):
    """ten columns of 65536 against an out capacity of 4: the count is exact,
    the four entries are among the ten"""
    torch = _torch()
    H, R, cap, out_cap = 2, 2, 16, 4
    plan, ctx, rows, out = _small(torch, H=H, R=R)
    cols = [1, 5, 9, 13, 17, 21, 40, 41, 62, 63]
    ac, ae = _buckets(torch, [[cols, []]], cap)
    oc = torch.zeros(R, dtype=torch.int32, device="cuda")
    oe = torch.full((R * out_cap,), -1, dtype=torch.int32, device="cuda")
    assert plan.partial(ctx, rows, out, acc=out, acc_counts=ac, acc_entries=ae, acc_cap=cap,
                        out_counts=oc, out_entries=oe, out_cap=out_cap) == 0
    cnt = oc.cpu().numpy().view(np.uint32)
    ent = oe.cpu().numpy().view(np.uint32).reshape(R, out_cap)
    assert cnt[0] == len(cols) and cnt[1] == 0
    assert len(set(ent[0])) == out_cap and set(int(v) for v in ent[0]) <= set(cols)
    assert (ent[1] == 0xFFFFFFFF).all()
    assert (out.cpu().numpy() == 0).all()


@pytest.mark.parametrize("k,m,H,R", [(16, 48, 0, 2), (16, 48, 17, 2), (16, 48, 2, 0),
                                     (16, 48, 2, 9), (16, 4, 2, 5)])
def test_partial_counts_out_of_range(hip_lib, k, m, H, R):
    """-1 from every entry point, and nothing written"""
    torch = _torch()
    import quadiron_amd as qa
    plan = qa.Plan(k, m, False)
    S, P = 2, 64
    lib = qa.lib()
    assert lib.qi_gpu_partial_ctx_bytes(plan.h, H, R, S) == 0
    assert plan.partial_kernels(H, R, P) == ""
    z = torch.zeros(S * 64, dtype=torch.int16, device="cuda")
    ctx = torch.full((1 << 14,), 0x5A, dtype=torch.uint8, device="cuda")
    rows = torch.full((S, 17, P), FILL, dtype=torch.int16, device="cuda")
    out = torch.full((S, 9, P), FILL, dtype=torch.int16, device="cuda")
    assert lib.qi_gpu_partial_ctx(plan.h, z.data_ptr(), z.data_ptr(), z.data_ptr(), H, R, S,
                                  ctx.data_ptr(), None) == -1
    assert lib.qi_gpu_partial(plan.h, ctx.data_ptr(), H, R, rows.data_ptr(), 17 * P, P, None,
                              None, 0, None, 0, 0, None, None, 0, out.data_ptr(), 9 * P, P, None,
                              None, 0, P, S, None) == -1
    torch.cuda.synchronize()
    assert (ctx == 0x5A).all() and (out == FILL).all() and (rows == FILL).all()
    assert plan.take_error() == 0


@pytest.mark.parametrize("k,m,sys_,H,R,P", [(16, 48, False, 1, 1, 1024), (16, 48, True, 16, 3, 37),
                                            (1000, 24, True, 1000, 8, 4099),
                                            (5000, 3000, False, 8, 2, 2056)])
def test_reported_partial_kernels_exist(hip_lib, k, m, sys_, H, R, P):
    import subprocess
    import quadiron_amd as qa
    out = subprocess.run(["nm", "-DC", qa.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    syms = [ln.split(" ", 2)[2] for ln in out.splitlines() if " qi::" in ln]
    kernels = qa.Plan(k, m, sys_).partial_kernels(H, R, P)
    role, names = kernels.split("=", 1)
    names = [n.strip() for n in names.split(" + ")]
    assert role == "partial" and len(names) == 2 and names[0] == "partial_ctx_kernel", kernels
    for name in names:
        assert any("qi::" + name + "(" in s for s in syms), (name, kernels)


# ---- 8. upper layers -------------------------------------------------------

def _block_chain(k, m, sys_, data, ids, targets, sizes, rng, cap=256):
    """Fec.partial_repair_blocks along a chain of holders; returns the final
    (rows, oor, counts) and the oracle's fragments"""
    import quadiron_amd as qa
    fr, fm, _ = _fragments(k, m, sys_, data, cap=cap)
    fec = qa.Fec(k, m, bool(sys_))
    perm = rng.permutation(k)
    acc, at = None, 0
    for n in sizes:
        pos = perm[at:at + n]
        at += n
        held_ids = [int(ids[p]) for p in pos]
        rows = [np.ascontiguousarray(fr[f]).view(np.uint8) for f in held_ids]
        oor = np.zeros((n, cap), np.uint32)
        cnt = np.zeros(n, np.uint32)
        for h, f in enumerate(held_ids):
            cnt[h] = len(fm[f])
            oor[h, :cnt[h]] = fm[f]
        acc = fec.partial_repair_blocks(ids, held_ids, rows, oor, cnt, targets, acc=acc)
    assert at == k
    return acc, fr, fm


def _check_blocks(res, fr, fm, targets):
    rows, oor, cnt = res
    for t, f in enumerate(int(v) for v in targets):
        assert (rows[t].view(np.uint16) == fr[f]).all(), f
        assert cnt[t] == len(fm[f]), (f, cnt[t], len(fm[f]))
        assert [int(v) for v in oor[t, :cnt[t]]] == sorted(fm[f]), f   # ascending


@pytest.mark.parametrize("k,m,sys_", [(16, 48, 0), (16, 48, 1), (300, 212, 0)])
def test_partial_repair_blocks_chain(hip_lib, k, m, sys_):
    rng = np.random.default_rng([k, m, sys_, 8])
    words = 1500
    first = k if sys_ else 0
    perm = rng.permutation(k + m)
    if sys_:
        targets = [int(perm[perm < k][0]), int(perm[perm >= k][0]), int(perm[perm >= k][1])]
    else:
        targets = [int(v) for v in perm[:3]]
    ids = [int(v) for v in perm[~np.isin(perm, targets)][:k]]
    data = rng.integers(0, 65536, (k, words), dtype=np.uint16)
    slots = [f - first for f in targets + ids[:3] if f >= first]
    craft_oor_columns(k, m, sys_, data, rng, 16, rows=slots)
    res, fr, fm = _block_chain(k, m, sys_, data, ids, targets, (1, 5, k - 6), rng)
    assert sum(len(fm[f]) for f in targets) >= 3
    _check_blocks(res, fr, fm, targets)


@pytest.mark.parametrize("sys_", [0, 1])
def test_partial_repair_blocks_retry(hip_lib, sys_):
    """retry_block's crafted fragment as the target: 100 marks against a
    first-attempt capacity of 65, so the last link's second attempt runs, from
    the acc rows as they were."""
    data, _, _, cnt_new, r, cap0 = retry_block(sys_)
    k = m = 4
    assert cnt_new[r] > cap0
    target = (k if sys_ else 0) + r
    ids = [f for f in range(k + m) if f != target][:k]
    res, fr, fm = _block_chain(k, m, sys_, np.array(data).view(np.uint16), ids, [target],
                               (2, 2), np.random.default_rng(9), cap=128)
    assert res[2][0] == cnt_new[r]
    _check_blocks(res, fr, fm, [target])


def test_partial_repair_blocks_rejects(hip_lib):
    import quadiron_amd as qa
    fec = qa.Fec(16, 48, True)
    row = np.zeros(128, np.uint8)
    ids = list(range(16))
    with pytest.raises(ValueError):    # more than min(8, m) targets
        fec.partial_repair_blocks(ids, [0], [row], None, None, list(range(16, 25)))
    with pytest.raises(ValueError):    # no held row
        fec.partial_repair_blocks(ids, [], [], None, None, [16])
    with pytest.raises(RuntimeError):  # a held fragment that is no helper
        fec.partial_repair_blocks(ids, [20], [row], None, None, [16])
    with pytest.raises(RuntimeError):  # a target that is a helper
        fec.partial_repair_blocks(ids, [0], [row], None, None, [3])
    with pytest.raises(RuntimeError):  # a repeated helper
        fec.partial_repair_blocks([0] * 16, [0], [row], None, None, [16])
