"""GPU: fused fragment verify (qi_gpu_verify on a qi_gpu_repair_ctx context)
against the CPU oracle and numpy.  True data is encoded by the oracle; the
stored copies are then corrupted, and the three numbers per (stripe, check
row) are computed here from their definitions (include/qi_gpu.h): with v the
canonical recomputed symbol in [0, 65536],
  value mismatch  (v & 0xffff) != stored[c]
  mark mismatch   (v == 65536) != (c in the stored row's bucket)
  first           the smallest column with either, else 0xFFFFFFFF.
Nothing expected here comes from the product.  Contexts, work buffers and
result arrays start from garbage."""
import numpy as np
import pytest

from qi_testlib import (craft_dense_oor, craft_oor_columns, decode_matrix, generator_matrix,
                        matvec_mod, oracle_encode_blocks, retry_block)

pytestmark = pytest.mark.gpu

CAP = 1024     # stored buckets
WCAP = 1024    # work buckets
NONE = 0xFFFFFFFF
Q = 65537


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    torch.cuda.set_device(0)
    return torch


def _slot(k, sys_, f):
    """coded-row slot (= oracle output index) of fragment f, None for data"""
    if sys_:
        return f - k if f >= k else None
    return f


class Stripes:
    """S stripes of true data, their oracle encoding, and the stored copies
    (rows and buckets) a test corrupts."""

    def __init__(self, k, m, sys_, data):
        self.k, self.m, self.sys = k, m, sys_
        self.S, _, self.P = data.shape
        self.data = data
        outs, oors, cnts = [], [], []
        for s in range(self.S):
            o, oor, cnt = oracle_encode_blocks(
                k, m, sys_, np.ascontiguousarray(data[s]).view(np.uint8).reshape(k, 2 * self.P),
                CAP)
            assert cnt.max() <= CAP
            outs.append(o.view(np.uint16).reshape(-1, self.P))
            oors.append(oor)
            cnts.append(cnt)
        self.coded = np.stack(outs)
        self.no = self.coded.shape[1]
        # the true symbols in [0, 65536] of every fragment id
        self.true = np.zeros((self.S, k + m, self.P), np.int64)
        for s in range(self.S):
            for f in range(k + m):
                sl = _slot(k, sys_, f)
                if sl is None:
                    self.true[s, f] = data[s, f]
                else:
                    self.true[s, f] = self.coded[s, sl]
                    self.true[s, f, oors[s][sl, :cnts[s][sl]]] = 65536
        # stored copies
        self.st_data = data.copy()
        self.st_coded = self.coded.copy()
        self.marks = [[set(int(c) for c in oors[s][sl, :cnts[s][sl]]) for sl in range(self.no)]
                      for s in range(self.S)]

    def stored_row(self, s, f):
        sl = _slot(self.k, self.sys, f)
        return self.st_data[s, f] if sl is None else self.st_coded[s, sl]

    def stored_marks(self, s, f):
        sl = _slot(self.k, self.sys, f)
        return set() if sl is None else self.marks[s][sl]

    def stored_full(self, s, f):
        """the stored fragment as symbols in [0, 65536] (what a basis row
        feeds into the recomputation)"""
        x = self.stored_row(s, f).astype(np.int64)
        mk = [c for c in self.stored_marks(s, f) if c < self.P]
        x[mk] = 65536
        return x


def _matrix(k, m, sys_, basis, checks):
    """(R, k) repair matrix: check rows from the basis fragments' symbols"""
    G = generator_matrix(k, m, sys_)          # (n_outputs, k): coded rows from data
    D = decode_matrix(k, m, sys_, np.asarray(basis))  # (k, k): data from the basis
    rows = []
    for f in checks:
        sl = _slot(k, sys_, int(f))
        rows.append(D[int(f)] if sl is None else matvec_mod(G[sl:sl + 1], D)[0])
    return np.stack(rows)


def _expect(st, basis, checks, recompute_cols=()):
    """(value_mismatch, mark_mismatch, first) per (stripe, check), by the
    definitions.  v is the true symbol wherever the stored basis equals the
    true one; the columns listed in recompute_cols[s] are recomputed from the
    stored basis symbols with the repair matrix."""
    S, R = checks.shape
    vm = np.zeros((S, R), np.int64)
    mm = np.zeros((S, R), np.int64)
    first = np.full((S, R), NONE, np.int64)
    vfull = np.zeros((S, R, st.P), np.int64)
    for s in range(S):
        for i, f in enumerate(basis[s]):
            diff = np.flatnonzero(st.stored_full(s, int(f)) != st.true[s, int(f)])
            assert set(diff) <= set(recompute_cols[s] if len(recompute_cols) else ()), \
                "a corrupted basis column must be listed for recomputation"
        cols = list(recompute_cols[s]) if len(recompute_cols) else []
        M = _matrix(st.k, st.m, st.sys, basis[s], checks[s]) if cols else None
        for j, f in enumerate(checks[s]):
            v = st.true[s, int(f)].copy()
            if cols:
                X = np.stack([st.stored_full(s, int(b))[cols] for b in basis[s]])
                v[cols] = matvec_mod(M[j:j + 1], X)[0]
            vfull[s, j] = v
            stored = st.stored_row(s, int(f)).astype(np.int64)
            inb = np.zeros(st.P, bool)
            inb[[c for c in st.stored_marks(s, int(f)) if c < st.P]] = True
            bad_v = (v & 0xffff) != stored
            bad_m = (v == 65536) != inb
            vm[s, j], mm[s, j] = bad_v.sum(), bad_m.sum()
            both = np.flatnonzero(bad_v | bad_m)
            if len(both):
                first[s, j] = both[0]
    return vm, mm, first, vfull


def _run(plan, st, basis, checks, unaligned=False, wcap=WCAP, cap=CAP, ctx_counts=True):
    """The device call on the stored copies; returns (vm, mm, first, error
    flags)."""
    torch = _torch()
    S, R, P, k = st.S, checks.shape[1], st.P, st.k
    pad_c, pad_d = (1, 3) if unaligned else (0, 0)
    cbig = torch.zeros((S, st.no, P + pad_c), dtype=torch.int16, device="cuda")
    dbig = torch.zeros((S, k, P + pad_d), dtype=torch.int16, device="cuda")
    coded, dd = cbig[:, :, pad_c:], dbig[:, :, pad_d:]
    coded.copy_(torch.from_numpy(st.st_coded.view(np.int16)))
    dd.copy_(torch.from_numpy(st.st_data.view(np.int16)))
    cnt = np.zeros((S, st.no), np.uint32)
    ent = np.zeros((S, st.no, cap), np.uint32)
    for s in range(S):
        for sl in range(st.no):
            mk = sorted(st.marks[s][sl])
            cnt[s, sl] = len(mk)
            ent[s, sl, :min(len(mk), cap)] = mk[:cap]
    counts = torch.from_numpy(cnt.view(np.int32).reshape(-1)).cuda()
    entries = torch.from_numpy(ent.view(np.int32).reshape(-1)).cuda()
    di = torch.from_numpy(np.ascontiguousarray(basis, np.uint16).view(np.int16)).cuda()
    dc = torch.from_numpy(np.ascontiguousarray(checks, np.uint16).view(np.int16)).cuda()
    nb = plan.repair_ctx_bytes(R, S, P)
    assert nb > 0
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    if ctx_counts:
        plan.repair_ctx(di, dc, ctx, P, counts, entries, cap)
    else:
        plan.repair_ctx(di, dc, ctx, P)
    wb = plan.verify_work_bytes(R, S, wcap)
    assert wb > 0
    work = torch.randint(0, 256, (wb,), dtype=torch.uint8, device="cuda")
    res = [torch.randint(0, 1 << 30, (S * R,), dtype=torch.int32, device="cuda")
           for _ in range(3)]
    err = plan.verify(ctx, dc, coded, work, wcap, res[0], res[1], res[2],
                      data=dd if st.sys else None, counts=counts, entries=entries, cap=cap)
    torch.cuda.synchronize()
    # nothing is written to the rows
    assert (coded.cpu().numpy().view(np.uint16) == st.st_coded).all()
    assert (dd.cpu().numpy().view(np.uint16) == st.st_data).all()
    vm, mm, first = (r.cpu().numpy().view(np.uint32).reshape(S, R).astype(np.int64) for r in res)
    return vm, mm, first, err


def _check(plan, st, basis, checks, unaligned=False, recompute_cols=()):
    evm, emm, efirst, _ = _expect(st, basis, checks, recompute_cols)
    vm, mm, first, err = _run(plan, st, basis, checks, unaligned)
    print("value", vm.tolist(), "expected", evm.tolist())
    print("mark", mm.tolist(), "expected", emm.tolist())
    print("first", first.tolist(), "expected", efirst.tolist())
    assert err == 0
    assert (vm == evm).all(), (vm, evm)
    assert (mm == emm).all(), (mm, emm)
    assert (first == efirst).all(), (first, efirst)
    return evm, emm, efirst


def _pick(k, m, R, rng, S):
    """per stripe: k ascending basis ids and R check ids among the others"""
    basis, checks = [], []
    for _ in range(S):
        b = np.sort(rng.choice(k + m, k, replace=False))
        rest = np.setdiff1d(np.arange(k + m), b)
        basis.append(b)
        checks.append(rng.permutation(rng.choice(rest, R, replace=False)))
    return np.stack(basis), np.stack(checks)


def _expected_names(k, P):
    ks = {16: 1, 24: 2, 64: 4, 100: 8, 200: 16}[k]
    core = (f"matrix_mfma_kernel_verify<{ks}, " if ks <= 2 else
            f"matrix_os_kernel_verify<{ks}, ")
    kp = {16: 8, 24: 16, 64: 32, 100: 64, 200: 128}[k]
    return core, f"matrix_kernel_verify<{kp}, "


def _names_check(plan, k, R, P):
    names = plan.verify_kernels(R, P)
    rep = plan.repair_kernels(R, P)
    # the repair's route in its verify forms, then the bucket comparison
    assert names == (rep.replace("repair=", "verify=").replace("_both", "_verify") +
                     " + verify_marks_kernel"), (names, rep)
    core, tail = _expected_names(k, P)
    assert (core in names) == (P >= 1024), names
    assert (tail in names) == (P % 1024 != 0), names
    assert ("matrix_redo_kernel_verify" in names) == (P % 1024 != 0), names
    assert "_both" not in names


CLEAN = [
    # k, m, sys, P, unaligned
    (16, 48, 0, 1024 + 40, False),   # mfma KS = 1 tile + dot2 tail
    (16, 48, 1, 1024 + 40, False),
    (16, 48, 0, 1024 + 40, True),    # rows at an odd word offset: dot2 only
    (24, 8, 1, 1024 + 40, False),    # KS = 2
    (64, 64, 0, 1024, False),        # os KS = 4
    (64, 64, 1, 1024, False),
    (100, 28, 1, 1024 + 40, False),  # os KS = 8
    (200, 56, 0, 1024, False),       # os KS = 16
    (200, 56, 1, 1024 + 8, False),   # ... plus a tail at KP = 128
]


@pytest.fixture(scope="module")
def clean_stripes():
    """one encoding per (k, m, sys, P), shared by the R cases (read only)"""
    cache = {}

    def get(k, m, sys_, P):
        key = (k, m, sys_, P)
        if key not in cache:
            rng = np.random.default_rng(31 * k + sys_ + P)
            data = rng.integers(0, 65536, (2, k, P), dtype=np.uint16)
            for s in range(2):  # the coded rows do hold marks, in tile and tail
                craft_oor_columns(k, m, sys_, data[s], rng, 12)
            cache[key] = Stripes(k, m, sys_, data)
        return cache[key]
    return get


@pytest.mark.parametrize("Rsel", ["one", "four", "max"])
@pytest.mark.parametrize("k,m,sys_,P,unaligned", CLEAN)
def test_clean_stripes(clean_stripes, k, m, sys_, P, unaligned, Rsel):
    import quadiron_amd as qa
    _torch()
    R = {"one": 1, "four": 4, "max": min(64, m)}[Rsel]
    st = clean_stripes(k, m, sys_, P)
    assert sum(len(mk) for mk in st.marks[0]) >= 3
    rng = np.random.default_rng(k + R + sys_)
    basis, checks = _pick(k, m, R, rng, st.S)
    plan = qa.Plan(k, m, sys_)
    if not unaligned:
        _names_check(plan, k, R, P)
    evm, emm, efirst = _check(plan, st, basis, checks, unaligned)
    assert not evm.any() and not emm.any() and (efirst == NONE).all()


@pytest.mark.parametrize("k,m,sys_", [(16, 48, 0), (64, 64, 1), (200, 56, 0)])
def test_corrupt_check_words(k, m, sys_):
    """Single corrupted words in check rows of stripe 0: row j is corrupted
    in columns cols[j:], so its count is 6 - j and its first column cols[j];
    the other rows and stripe 1 stay clean."""
    import quadiron_amd as qa
    _torch()
    P, R = 1024 + 40, 8
    rng = np.random.default_rng(5 + k)
    data = rng.integers(0, 65536, (2, k, P), dtype=np.uint16)
    st = Stripes(k, m, sys_, data)
    basis, checks = _pick(k, m, R, rng, 2)
    cols = [0, 63, 64, 1023, 1024, P - 1]
    for j in range(len(cols)):
        row = st.stored_row(0, int(checks[0, j]))
        for c in cols[j:]:
            assert st.true[0, int(checks[0, j]), c] != 65536
            row[c] ^= 1 + j
    evm, emm, efirst = _check(qa.Plan(k, m, sys_), st, basis, checks)
    assert evm[0].tolist() == [6, 5, 4, 3, 2, 1, 0, 0] and not evm[1].any()
    assert efirst[0].tolist() == cols + [NONE, NONE]
    assert not emm.any()


@pytest.mark.parametrize("unaligned", [False, True])
def test_mark_cases(unaligned):
    """Check rows that hold true 65536 values, in the tile and in the tail.
    Telling these apart needs the marks, not only the low 16 bits."""
    import quadiron_amd as qa
    _torch()
    k, m, P, R = 16, 48, 1024 + 40, 5
    rng = np.random.default_rng(99)
    data = rng.integers(0, 65536, (2, k, P), dtype=np.uint16)
    basis = np.tile(np.arange(0, 2 * k, 2), (2, 1))
    checks = np.tile(np.array([1, 21, 33, 47, 63]), (2, 1))
    zero_cols = [10, 1030]
    for s in range(2):
        data[s][:, zero_cols] = 0  # every fragment is 0 there (a linear code)
        for f in checks[s]:
            craft_oor_columns(k, m, 0, data[s], rng, 6, rows=[int(f)], col_range=(20, 1000))
            craft_oor_columns(k, m, 0, data[s], rng, 4, rows=[int(f)], col_range=(1040, P))
    st = Stripes(k, m, 0, data)
    for s in range(2):
        for f in checks[s]:
            mk = sorted(st.marks[s][int(f)])
            assert sum(c < 1024 for c in mk) >= 2 and sum(c >= 1024 for c in mk) >= 1, (f, mk)
            assert (st.true[s, int(f), zero_cols] == 0).all()
    # stripe 0, per check row: (a) a stored mark removed, in the tile and in
    # the tail; (b) a spurious mark where the value is 0; (c) a spurious mark
    # on a nonzero column; (d) a stored nonzero word where v = 65536; row 4
    # and stripe 1 stay clean
    a, b, c_, d = (int(f) for f in checks[0, :4])
    mk = sorted(st.marks[0][a])
    st.marks[0][a] -= {mk[0], mk[-1]}
    st.marks[0][b] |= set(zero_cols)
    nz = [c for c in (5, 1050) if st.true[0, c_, c] not in (0, 65536)]
    assert len(nz) == 2
    st.marks[0][c_] |= set(nz)
    mk = sorted(st.marks[0][d])
    st.st_coded[0, d, mk[0]] = 7
    st.st_coded[0, d, mk[-1]] = 65535
    evm, emm, efirst = _check(qa.Plan(k, m, False), st, basis, checks, unaligned)
    assert evm[0].tolist() == [0, 0, 0, 2, 0] and emm[0].tolist() == [2, 2, 2, 0, 0]
    assert not evm[1].any() and not emm[1].any()


def test_corrupt_basis_row():
    """One word of a basis row: every check row reports exactly one value
    mismatch, at that column."""
    import quadiron_amd as qa
    _torch()
    k, m, P = 16, 48, 1024 + 40
    rng = np.random.default_rng(321)
    data = rng.integers(0, 65536, (2, k, P), dtype=np.uint16)
    st = Stripes(k, m, 0, data)
    basis, checks = _pick(k, m, 48, rng, 2)
    cols = [[300], [1050]]  # stripe 0 in the tile, stripe 1 in the tail
    for s in range(2):
        c = cols[s][0]
        assert (st.true[s, :, c] != 65536).all()
        st.stored_row(s, int(basis[s, 5]))[c] ^= 0x0101
    evm, emm, efirst, vfull = _expect(st, basis, checks, cols)
    for s in range(2):  # no recomputed symbol at that column is out of range
        assert (vfull[s][:, cols[s][0]] != 65536).all()
    assert (evm == 1).all() and not emm.any()
    assert (efirst[0] == 300).all() and (efirst[1] == 1050).all()
    _check(qa.Plan(k, m, False), st, basis, checks, recompute_cols=cols)


@pytest.mark.parametrize("unaligned", [False, True])
def test_slow_tile_counts_once(unaligned):
    """More than 256 input marks in the first 256 columns (the construction
    of the repair's slow-tile test): the first pass of that tile neither
    counts nor records, its redo does both, once.  Aligned rows: the
    matrix-core kernel's own redo of its 1024-column tile; unaligned rows:
    the dot2 kernel's 256-column tile and matrix_redo_kernel_verify."""
    import quadiron_amd as qa
    _torch()
    k, m, S, P, t = 16, 48, 2, 2048, 20
    rng = np.random.default_rng(77)
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    assert craft_dense_oor(k, m, data[0], rng, range(0, 40), [t, 3, 5], 3) > 30
    assert craft_dense_oor(k, m, data[0], rng, range(40, 200), range(k), 2) > 140
    craft_oor_columns(k, m, 0, data[0], rng, 20, rows=[t], col_range=(200, 256))
    st = Stripes(k, m, 0, data)
    in_tile = sum(sum(c < 256 for c in st.marks[0][f]) for f in range(k))
    assert in_tile > 256, in_tile
    assert len(st.marks[0][t]) >= 40
    basis = np.tile(np.arange(k), (S, 1))
    checks = np.tile(np.array([t, 40]), (S, 1))
    # one corruption inside the slow tile, in a column without input marks and
    # with an in-range symbol -- the first pass computes that column right, so
    # a build that also counted there would report it twice -- and one outside
    inside = next(c for c in range(200, 256)
                  if all(c not in st.marks[0][f] for f in range(k)) and
                  st.true[0, 40, c] != 65536 and st.true[0, t, c] != 65536)
    outside = 1500
    for f in (t, 40):
        st.stored_row(0, f)[inside] ^= 3
        st.stored_row(0, f)[outside] ^= 5
    # and a stored mark removed inside the tile: one mark mismatch, once
    gone = min(c for c in st.marks[0][t] if c >= 200)
    st.marks[0][t].discard(gone)
    evm, emm, efirst = _check(qa.Plan(k, m, False), st, basis, checks, unaligned)
    assert evm[0].tolist() == [2, 2] and emm[0].tolist() == [1, 0]
    assert efirst[0].tolist() == [min(inside, gone), inside]
    assert not evm[1].any() and not emm[1].any()


def test_verify_errors():
    import quadiron_amd as qa
    torch = _torch()
    L = qa.lib()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()

    def raw(plan, R, words=200):
        return L.qi_gpu_verify(plan.h, p, R, p, p, 0, words, p, 0, words, None, None, 0, p, 4,
                               p, p, p, words, 1, None)
    # k > 256: unsupported
    p300 = qa.Plan(300, 100, False)
    assert p300.verify_work_bytes(1, 1, 16) == 0
    assert p300.verify_kernels(1, 1024) == ""
    assert raw(p300, 1, 1024) == qa.Plan.ERR_UNSUPPORTED
    # n_checks out of range: refused, nothing launched
    big = qa.Plan(64, 960, False)
    assert big.verify_work_bytes(64, 2, 16) == 2 * 64 * 17 * 4
    for R in (0, 65):
        assert big.verify_work_bytes(R, 1, 16) == 0
        assert raw(big, R) == -1
    torch.cuda.synchronize()
    assert big.take_error() == 0
    # more recomputed 65536 values than the work buckets hold: bit 1
    k, m, P = 16, 48, 1024 + 40
    rng = np.random.default_rng(8)
    data = rng.integers(0, 65536, (2, k, P), dtype=np.uint16)
    craft_oor_columns(k, m, 0, data[0], rng, 8, rows=[30])
    st = Stripes(k, m, 0, data)
    assert len(st.marks[0][30]) >= 5
    basis = np.tile(np.arange(k), (2, 1))
    checks = np.tile(np.array([30, 31]), (2, 1))
    plan = qa.Plan(k, m, False)
    *_, err = _run(plan, st, basis, checks, wcap=2)
    assert err & 1
    *_, err = _run(plan, st, basis, checks)
    assert err == 0
    # a stored bucket over its capacity: bit 1
    *_, err = _run(plan, st, basis, checks, cap=2, ctx_counts=False)
    assert err & 1
    # a check id that is also a basis id: bit 2, from the context builder
    *_, err = _run(plan, st, basis, np.tile(np.array([30, 3]), (2, 1)))
    assert err & 2


# ---- upper layers -------------------------------------------------------

@pytest.mark.parametrize("sys_", [0, 1])
def test_fec_verify_blocks_retry(sys_):
    """Every fragment present; one checked fragment recomputes to 65536 in
    more columns than the first attempt's work buckets hold (64 + words / 512
    = 65): Fec.verify_blocks runs the group again with the exact capacity.
    Clean fragments report (0, 0, none); one flipped stored word of that
    fragment then reports one value mismatch at its column, there alone."""
    import quadiron_amd as qa
    _torch()
    k, m = 4, 4
    data, outs, oor, cnt, r, first_cap = retry_block(sys_)
    assert first_cap < cnt[r] <= 128 and cnt.max() <= 128, cnt
    crafted = k + r if sys_ else r
    miss = np.zeros(k + m, np.int32)
    checked = list(range(k, k + m))   # the basis is the first k fragments
    assert crafted in checked
    pars = [outs[i].copy() for i in range(outs.shape[0])]
    drows = [data[i].copy() for i in range(k)] if sys_ else None
    fec = qa.Fec(k, m, bool(sys_))
    res = fec.verify_blocks(drows, pars, oor, cnt, miss)
    assert res is not None
    for f in range(k + m):
        assert res[f].tolist() == ([0, 0, NONE] if f in checked else [-1, -1, -1]), (f, res[f])
    col = next(c for c in range(100, 512) if c not in set(oor[r, :cnt[r]].tolist()))
    pars[r].view(np.uint16)[col] ^= 0x0400
    res = fec.verify_blocks(drows, pars, oor, cnt, miss)
    assert res is not None
    for f in range(k + m):
        exp = ([1, 0, col] if f == crafted else [0, 0, NONE] if f in checked
               else [-1, -1, -1])
        assert res[f].tolist() == exp, (f, res[f])


@pytest.mark.parametrize("k,m,sys_", [(6, 3, 1), (16, 48, 0), (16, 100, 0)])
def test_fec_verify_blocks(k, m, sys_):
    """Fec.verify_blocks: one fragment missing, one corrupted (a row word,
    and a mark where it has one).  -1 rows for the basis and the missing
    fragment, exact numbers elsewhere; m = 100 takes two groups of checks."""
    import quadiron_amd as qa
    _torch()
    B = 2 * (1024 + 40)
    P = B // 2
    rng = np.random.default_rng(700 + k + m)
    data = rng.integers(0, 65536, (1, k, P), dtype=np.uint16)
    craft_oor_columns(k, m, sys_, data[0], rng, 30)
    st = Stripes(k, m, sys_, data)
    n = k + m
    miss = np.zeros(n, np.int32)
    miss[2] = 1
    present = [f for f in range(n) if not miss[f]]
    basis, checks = present[:k], present[k:]
    bad = checks[len(checks) // 2]
    st.stored_row(0, bad)[[7, 1030]] ^= 9
    dropped = 0
    if st.stored_marks(0, bad):
        st.stored_marks(0, bad).discard(min(st.stored_marks(0, bad)))
        dropped = 1
    evm, emm, efirst, _ = _expect(st, np.array([basis]), np.array([checks]))
    assert evm.sum() == 2 and emm.sum() == dropped
    cap = 64
    oor = np.zeros((st.no, cap), np.uint32)
    cnt = np.zeros(st.no, np.uint32)
    for sl in range(st.no):
        mk = sorted(st.marks[0][sl])
        assert len(mk) <= cap
        cnt[sl] = len(mk)
        oor[sl, :len(mk)] = mk
    first = k if sys_ else 0
    pars = [None if miss[first + i] else st.st_coded[0, i].view(np.uint8).copy()
            for i in range(st.no)]
    drows = ([None if miss[i] else st.st_data[0, i].view(np.uint8).copy() for i in range(k)]
             if sys_ else None)
    fec = qa.Fec(k, m, bool(sys_))
    res = fec.verify_blocks(drows, pars, oor, cnt, miss)
    assert res is not None and res.shape == (n, 3)
    for f in range(n):
        if f in checks:
            j = checks.index(f)
            assert res[f].tolist() == [evm[0, j], emm[0, j], efirst[0, j]], (f, res[f])
        else:
            assert res[f].tolist() == [-1, -1, -1], (f, res[f])
    # fewer than k + 1 fragments: nothing to check against
    miss2 = np.ones(n, np.int32)
    miss2[present[:k]] = 0
    assert fec.verify_blocks(drows, pars, oor, cnt, miss2) is None
