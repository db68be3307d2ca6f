"""GPU: every entry point of the device C-ABI on wide row layouts, against
the CPU oracle, bit for bit.

A fragment-major layout keeps each fragment's stripes back to back (stripe
stride P, row stride >= S * P words), so one stripe's row region can span
GiB.  Once a region of a launch does not fit a 31-bit buffer range
(row_extent == 0) the library runs its flat kernels -- encode_fnt_kernel<K,
1, false, false>, matrix_kernel*<KP, 1, false>, matrix_redo_kernel* -- or the
NTT engine, and row offsets need 64 bits.  Region classes (qi_testlib.wide_rs):
B, the top of the buffer range, still on the matrix cores; F2, just past it;
F4, the upper rows 4.3 GiB from the stripe base.  Each case states from the
library's own rule (row_extent, pinned for both in tests/test_matrix_route.py)
that the region it made wide is what it claims.

Every tensor is a view of a backing that covers its region from word 0 and
holds 0x5A5A wherever no row lives, so an offset that lost its upper bits
lands on a lower row or in a gap of the same allocation: data is corrupted,
nothing faults.  After the rows are compared, they are set back to 0x5A5A
and every backing, the inputs' too, must hold nothing else.

Expected rows, marks and decodes are the oracle's; the received rows and
buckets of decodes, repairs and verifies are the oracle's too."""
import functools
import gc

import numpy as np
import pytest

from qi_testlib import (FILL, backing_is_fill, craft_dense_oor, craft_oor_columns,
                        oracle_decode_blocks, oracle_encode_blocks, row_extent, strided_rows,
                        wide_rs)

pytestmark = pytest.mark.gpu

S = 2        # two stripes side by side in every row's area: a wrong stripe base shows
CAP = 1024
NONE = 0xFFFFFFFF
GIB4 = 1 << 32


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    torch.cuda.set_device(0)
    return torch


_LIVE = []


def _freed(fn):
    """Frees the case's backings at its end, passed or failed (a failure's
    traceback would keep them alive), and prints the most it held."""
    @functools.wraps(fn)
    def run(*a, **kw):
        torch = _torch()
        torch.cuda.reset_peak_memory_stats()
        try:
            return fn(*a, **kw)
        finally:
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() / 2.0**30
            print("peak device memory %.2f GiB" % peak)
            for r in _LIVE:
                r.free()
            _LIVE.clear()
            gc.collect()
            torch.cuda.empty_cache()
            assert peak <= 16.0
    return run


class Rows:
    """One [S, rows, P] tensor of a call in a region class; host: the rows
    an input holds (None: an output)."""

    def __init__(self, rows, P, cls, host=None):
        torch = _torch()
        if rows == 1:
            cls = "N"   # one row cannot be wide: the case widens the other side
        self.cls, self.rows, self.P, self.host = cls, rows, P, host
        self.rs = wide_rs(cls, rows, P)
        # the precondition, by the library's rule: flat or buffer kernels
        assert (row_extent(rows, self.rs, P) == 0) == cls.startswith("F")
        assert self.rs % 4 == 0 and P % 4 == 0
        self.backing, self.view = strided_rows(S, rows, P, self.rs, P)
        assert self.backing.data_ptr() % 8 == 0
        _LIVE.append(self)
        if host is not None:
            assert host.shape == (S, rows, P)
            self.view.copy_(torch.from_numpy(np.array(host).view(np.int16)))

    def offset(self, row):
        """byte offset of a row from its stripe base"""
        return row * self.rs * 2

    def read(self):
        return self.view.cpu().numpy().view(np.uint16)

    def finish(self):
        """an input reads back unchanged; then, with the rows set back to the
        fill word, the whole backing holds nothing else"""
        if self.host is not None:
            assert (self.read() == self.host).all(), "an input was written"
        self.view.fill_(FILL)
        assert backing_is_fill(self.backing), "a store outside the rows (%s)" % self.cls

    def free(self):
        self.backing.untyped_storage().resize_(0)


def _finish_all():
    for r in list(_LIVE):
        r.finish()


def _slot(k, sys_, f):
    """coded-row slot (= oracle output index) of fragment f, None for data"""
    if sys_:
        return f - k if f >= k else None
    return f


@functools.lru_cache(maxsize=None)
def _pick(k, m, sys_):
    """Per stripe: k received ids (stripe 0 ascending, stripe 1 shuffled;
    systematic: data and parity fragments both) and up to 17 other fragments,
    the first of them the last fragment of the code -- the last row of the
    coded region, the one farthest from its base."""
    rng = np.random.default_rng(5 * k + 3 * m + sys_)
    n = k + m
    ids, tgs = [], []
    for s in range(S):
        last = n - 1
        if sys_ and k >= 2:
            npar = min(m - 1, max(1, k // 2))
            got = np.concatenate([rng.choice(k, k - npar, replace=False),
                                  k + rng.choice(m - 1, npar, replace=False)])
        else:
            got = rng.choice(n - 1, k, replace=False)
        got = np.sort(got) if s == 0 else rng.permutation(got)
        rest = np.setdiff1d(np.arange(n - 1), got)
        tg = np.concatenate([[last], rng.permutation(rest)[:min(16, m - 1)]])
        ids.append(got)
        tgs.append(tg)
    return np.stack(ids).astype(np.uint16), np.stack(tgs).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def _stripes(k, m, sys_, P, dense=False):
    """S stripes of data and their oracle encoding (rows u16, mark lists,
    counts), shared by the cases of a shape and never written.  Marks are
    crafted on the received rows of _pick and on its first target; dense:
    more than 256 marks of received rows 0 .. k-1 in the first 200 columns."""
    rng = np.random.default_rng(7919 * k + 31 * m + sys_ + P)
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    ids, tgs = _pick(k, m, sys_)
    for s in range(S):
        if dense:
            assert craft_dense_oor(k, m, data[s], rng, range(0, 200), range(k), 2) > 140
            continue
        recv = [f for f in (_slot(k, sys_, int(f)) for f in ids[s]) if f is not None]
        half = P // 2
        for lo, hi in ((0, half), (half, P)):
            if recv:
                craft_oor_columns(k, m, sys_, data[s], rng, 6, rows=recv, col_range=(lo, hi))
            craft_oor_columns(k, m, sys_, data[s], rng, 3, rows=[_slot(k, sys_, int(tgs[s, 0]))],
                              col_range=(lo, hi))
    enc = []
    for s in range(S):
        o, oor, cnt = oracle_encode_blocks(
            k, m, sys_, np.ascontiguousarray(data[s]).view(np.uint8).reshape(k, 2 * P), CAP)
        # (k = 1: every output is the data symbol itself, never 65536)
        assert cnt.max() <= CAP and (cnt.sum() > 0 or k == 1)
        enc.append((o.view(np.uint16).reshape(-1, P), oor, cnt))
    data.setflags(write=False)
    return data, enc


def _buckets(torch, enc):
    cnt = np.stack([e[2] for e in enc]).astype(np.uint32)
    ent = np.stack([e[1] for e in enc]).astype(np.uint32)
    return (torch.from_numpy(cnt.view(np.int32).reshape(-1)).cuda(),
            torch.from_numpy(ent.view(np.int32).reshape(-1)).cuda())


def _dev16(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda()


# ---- encode --------------------------------------------------------------

def _encode_case(k, m, sys_, P, src, dst, encoder=None, want=None):
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, bool(sys_), encoder=encoder)
    no = plan.n_outputs
    if want is not None:   # the kernel family, as reported for rows in buffer range
        assert want in plan.kernels(P).split(";")[0], plan.kernels(P)
    data, enc = _stripes(k, m, sys_, P)
    d = Rows(k, P, src, data)
    o = Rows(no, P, dst)
    assert d.cls == src or k == 1
    counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * no * CAP, dtype=torch.int32, device="cuda")
    plan.encode(d.view, o.view, counts, entries, CAP)
    torch.cuda.synchronize()
    got = o.read()
    gc_ = counts.cpu().numpy().view(np.uint32).reshape(S, no)
    ge = entries.cpu().numpy().view(np.uint32).reshape(S, no, CAP)
    for s in range(S):
        rows, oor, cnt = enc[s]
        bad = np.flatnonzero((got[s] != rows).any(axis=1))
        assert len(bad) == 0, ("rows differ", s, bad[:8], [o.offset(int(r)) for r in bad[:8]])
        assert (gc_[s] == cnt).all(), s
        assert cnt.sum() > 0 or k == 1
        for i in range(no):
            assert (np.sort(ge[s, i, :cnt[i]]) == oor[i, :cnt[i]]).all(), (s, i)
    _finish_all()
    assert plan.take_error() == 0


def _ids(*cases):
    return ["-".join(str(v) for v in c) for c in cases]


# K = 1 .. 64 of encode_fnt_kernel<K, 1, false, false>
CODELET = []
for _k, _m in [(1, 1), (2, 2), (3, 3), (7, 9), (16, 48), (32, 32), (33, 31), (64, 64)]:
    CODELET += [(_k, _m, 300, "N", "F4"), (_k, _m, 1100, "F4", "N")]
CODELET = [c for c in CODELET if not (c[0] == 1 and c[3] == "F4")]
CODELET += [(16, 48, 1100, "F4", "F4"), (16, 48, 300, "F2", "F2"), (16, 48, 1100, "F2", "F2"),
            (3, 3, 300, "F2", "F2"), (32, 32, 1100, "F2", "N"), (64, 64, 300, "N", "F2"),
            (1, 1, 1100, "N", "F2")]


@pytest.mark.parametrize("k,m,P,src,dst", CODELET, ids=_ids(*CODELET))
@_freed
def test_codelet_encode(k, m, P, src, dst):
    """(1,1) and (2,2): two-row regions, the row stride itself past 2^32
    bytes."""
    _encode_case(k, m, 0, P, src, dst, encoder="codelets" if k > 32 else None,
                 want="encode_fnt_kernel<")


# KP = 2 .. 128 of matrix_kernel<KP, 1, false>, output marks recorded
GENERATOR = []
for _k, _m, _sys in [(3, 3, 1), (7, 5, 1), (16, 48, 1), (32, 32, 1), (64, 64, 1), (100, 50, 1),
                     (200, 56, 1), (65, 63, 0), (200, 56, 0)]:
    GENERATOR += [(_k, _m, _sys, 300, "F4", "N"), (_k, _m, _sys, 1100, "N", "F4")]
GENERATOR += [(16, 48, 1, 1100, "F4", "F4"), (16, 48, 1, 1100, "F2", "F2"),
              (200, 56, 0, 300, "F2", "F2"), (7, 5, 1, 300, "F2", "N"),
              (100, 50, 1, 1100, "N", "F2")]


@pytest.mark.parametrize("k,m,sys_,P,src,dst", GENERATOR, ids=_ids(*GENERATOR))
@_freed
def test_generator_encode(k, m, sys_, P, src, dst):
    _encode_case(k, m, sys_, P, src, dst, want="matrix_")


# ---- decode --------------------------------------------------------------

def _decode_case(k, m, sys_, P, dcls, ccls, ocls, dense=False, then_contiguous=False,
                 oracle_decode=True):
    """qi_gpu_decode from contexts with routed buckets; dcls: the systematic
    data region's class (ignored otherwise), ccls the coded region's, ocls the
    output's."""
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, bool(sys_))
    no = plan.n_outputs
    data, enc = _stripes(k, m, sys_, P, dense)
    ids = (np.tile(np.arange(k, dtype=np.uint16), (S, 1)) if dense else _pick(k, m, sys_)[0])
    recv_marks = 0
    for s in range(S):
        recv = [f for f in (_slot(k, sys_, int(f)) for f in ids[s]) if f is not None]
        recv_marks += int(enc[s][2][recv].sum())
        if dense:   # more than 256 marks inside one 256-column block of the flat kernel
            assert sum(int((enc[s][1][f, :enc[s][2][f]] < 256).sum()) for f in recv) > 256
    assert recv_marks > 0
    coded = Rows(no, P, ccls, np.stack([e[0] for e in enc]))
    dd = Rows(k, P, dcls, data) if sys_ else None
    out = Rows(k, P, ocls)
    counts, entries = _buckets(torch, enc)
    di = _dev16(torch, ids)
    ctx = torch.randint(0, 256, (plan.ctx_bytes(S, P),), dtype=torch.uint8, device="cuda")
    plan.decode_ctx(di, ctx, P, counts, entries, CAP)

    def run(c, d, o):
        assert plan.decode(ctx, di, c, o, data=d, counts=counts, entries=entries, cap=CAP) == 0
        torch.cuda.synchronize()

    run(coded.view, dd.view if sys_ else None, out.view)
    got = out.read()
    for s in range(S):
        if oracle_decode:
            missing = np.ones(k + m, np.int32)
            missing[ids[s].astype(np.int64)] = 0
            ok, dec = oracle_decode_blocks(
                k, m, sys_, enc[s][0].view(np.uint8).reshape(no, 2 * P), enc[s][1], enc[s][2],
                missing, data[s].view(np.uint8).reshape(k, 2 * P))
            assert ok == 1
            exp = dec.view(np.uint16).reshape(k, P)
            assert (exp == data[s]).all()
        else:
            exp = data[s]   # what the oracle encoded
        bad = np.flatnonzero((got[s] != exp).any(axis=1))
        assert len(bad) == 0, ("rows differ", s, bad[:8])
    if then_contiguous:
        # the same contexts decode contiguous copies on the matrix cores
        c2 = coded.view.contiguous()
        o2 = torch.zeros((S, k, P), dtype=torch.int16, device="cuda")
        run(c2, dd.view.contiguous() if sys_ else None, o2)
        assert (o2.cpu().numpy().view(np.uint16) == data).all()
    _finish_all()
    assert plan.take_error() == 0


DECODE = []
for _k, _m in [(3, 3), (7, 9), (16, 48), (32, 32), (64, 64), (65, 63), (200, 56)]:
    DECODE += [(_k, _m, 0, 300, "-", "F4", "N"), (_k, _m, 0, 1100, "-", "N", "F4")]
for _k, _m in [(3, 3), (7, 5), (32, 32), (64, 64), (100, 50)]:
    DECODE += [(_k, _m, 1, 300, "N", "F4", "N"), (_k, _m, 1, 1100, "F4", "N", "N"),
               (_k, _m, 1, 1100, "N", "N", "F4")]
for _k, _m in [(16, 48), (200, 56)]:
    DECODE += [(_k, _m, 1, 300, "F4", "N", "N"), (_k, _m, 1, 1100, "N", "F4", "N"),
               (_k, _m, 1, 1100, "F4", "F4", "N"), (_k, _m, 1, 300, "N", "N", "F4"),
               (_k, _m, 1, 300, "F2", "N", "N"), (_k, _m, 1, 300, "N", "F2", "N"),
               (_k, _m, 1, 1100, "N", "N", "F2")]
DECODE += [(16, 48, 0, 1100, "-", "F4", "F4"), (16, 48, 0, 300, "-", "F2", "F2"),
           (3, 3, 0, 1100, "-", "F2", "N"), (64, 64, 0, 300, "-", "N", "F2"),
           (200, 56, 0, 1100, "-", "F2", "F2")]


@pytest.mark.parametrize("k,m,sys_,P,dcls,ccls,ocls", DECODE, ids=_ids(*DECODE))
@_freed
def test_decode(k, m, sys_, P, dcls, ccls, ocls):
    _decode_case(k, m, sys_, P, dcls, ccls, ocls)


@pytest.mark.parametrize("ccls,ocls", [("F4", "N"), ("N", "F4"), ("F2", "F2")])
@_freed
def test_slow_tile_behind_flat_rows(ccls, ocls):
    """More than 256 marks of the received rows in one block of the flat
    dot2 kernel: matrix_redo_kernel recomputes the tile, on the same rows."""
    _decode_case(16, 48, 0, 1100, "-", ccls, ocls, dense=True)


@pytest.mark.parametrize("rcls,ocls", [("F4", "N"), ("N", "F4")])
@_freed
def test_decode_packed(rcls, ocls):
    """qi_gpu_decode_packed: the received rows back to back in id order,
    buckets by position."""
    import quadiron_amd as qa
    torch = _torch()
    k, m, P = 16, 48, 1100
    plan = qa.Plan(k, m, False)
    data, enc = _stripes(k, m, 0, P)
    ids = _pick(k, m, 0)[0]
    idx = ids.astype(np.int64)
    recv_h = np.stack([enc[s][0][idx[s]] for s in range(S)])
    pcnt = np.stack([enc[s][2][idx[s]] for s in range(S)]).astype(np.uint32)
    pent = np.stack([enc[s][1][idx[s]] for s in range(S)]).astype(np.uint32)
    assert pcnt.sum() > 0
    recv = Rows(k, P, rcls, recv_h)
    out = Rows(k, P, ocls)
    dc = torch.from_numpy(pcnt.view(np.int32).reshape(-1)).cuda()
    de = torch.from_numpy(pent.view(np.int32).reshape(-1)).cuda()
    di = _dev16(torch, ids)
    ctx = torch.randint(0, 256, (plan.ctx_bytes(S, P),), dtype=torch.uint8, device="cuda")
    plan.decode_ctx_packed(di, ctx, P, dc, de, CAP)
    assert plan.decode_packed(ctx, recv.view, out.view, dc, de, CAP) == 0
    torch.cuda.synchronize()
    assert (out.read() == data).all()
    _finish_all()
    assert plan.take_error() == 0


# ---- repair and verify ---------------------------------------------------

REPAIR_SHAPES = [(3, 3, 1), (16, 48, 0), (16, 48, 1), (64, 960, 0), (200, 56, 1)]


def _region_variants(sys_):
    """(data, coded, out) classes: each region wide alone, then together"""
    if sys_:
        return [("F4", "N", "N"), ("N", "F4", "N"), ("N", "N", "F4"), ("F4", "F4", "N"),
                ("N", "F2", "F2")]
    return [("-", "F4", "N"), ("-", "N", "F4"), ("-", "F4", "F4"), ("-", "F2", "F2")]


REPAIR = []
for _k, _m, _sys in REPAIR_SHAPES:
    for _i, (_d, _c, _o) in enumerate(_region_variants(_sys)):
        for _R in (1, 17):
            if _R == 1 and _o != "N":
                continue   # one output row cannot be wide
            REPAIR.append((_k, _m, _sys, 300 if (_i + _R) % 2 else 1100, _R, _d, _c, _o))


def _repair_setup(plan, k, m, sys_, P, R):
    torch = _torch()
    R = min(R, m, 64)
    data, enc = _stripes(k, m, sys_, P)
    ids, tgs = _pick(k, m, sys_)
    targets = np.ascontiguousarray(tgs[:, :R])
    for s in range(S):
        recv = [f for f in (_slot(k, sys_, int(f)) for f in ids[s]) if f is not None]
        assert enc[s][2][recv].sum() > 0                             # input marks
        assert enc[s][2][_slot(k, sys_, int(targets[s, 0]))] > 0     # output marks
    counts, entries = _buckets(torch, enc)
    di, dt = _dev16(torch, ids), _dev16(torch, targets)
    nb = plan.repair_ctx_bytes(R, S, P)
    assert nb > 0
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    plan.repair_ctx(di, dt, ctx, P, counts, entries, CAP)
    return R, data, enc, targets, counts, entries, dt, ctx


@pytest.mark.parametrize("k,m,sys_,P,R,dcls,ccls,ocls", REPAIR, ids=_ids(*REPAIR))
@_freed
def test_repair(k, m, sys_, P, R, dcls, ccls, ocls):
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, bool(sys_))
    no = plan.n_outputs
    R, data, enc, targets, counts, entries, _, ctx = _repair_setup(plan, k, m, sys_, P, R)
    coded = Rows(no, P, ccls, np.stack([e[0] for e in enc]))
    dd = Rows(k, P, dcls, data) if sys_ else None
    out = Rows(R, P, ocls)
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * R * CAP, dtype=torch.int32, device="cuda")
    assert plan.repair(ctx, coded.view, out.view, data=dd.view if sys_ else None, counts=counts,
                       entries=entries, cap=CAP, out_counts=oc, out_entries=oe,
                       out_cap=CAP) == 0
    torch.cuda.synchronize()
    got = out.read()
    gc_ = oc.cpu().numpy().view(np.uint32).reshape(S, R)
    ge = oe.cpu().numpy().view(np.uint32).reshape(S, R, CAP)
    for s in range(S):
        for j in range(R):
            t = int(targets[s, j])
            sl = _slot(k, sys_, t)
            if sl is None:
                exp, em = data[s, t], np.zeros(0, np.uint32)
            else:
                exp, em = enc[s][0][sl], enc[s][1][sl, :enc[s][2][sl]]
            assert (got[s, j] == exp).all(), (s, j, t, np.flatnonzero(got[s, j] != exp)[:8])
            assert gc_[s, j] == len(em), (s, j, t, gc_[s, j], len(em))
            assert (np.sort(ge[s, j, :gc_[s, j]]) == em).all(), (s, j, t)
    _finish_all()
    assert plan.take_error() == 0


VERIFY = []
for _k, _m, _sys in REPAIR_SHAPES:
    for _i, (_d, _c, _o) in enumerate(_region_variants(_sys)):
        if _o != "N":
            continue   # a verify writes no rows
        for _R in (1, 17):
            VERIFY.append((_k, _m, _sys, 300 if (_i + _R) % 2 else 1100, _R, _d, _c))
VERIFY += [(16, 48, 0, 300, 17, "-", "F2"), (200, 56, 1, 1100, 17, "F2", "F2")]


@pytest.mark.parametrize("k,m,sys_,P,R,dcls,ccls", VERIFY, ids=_ids(*VERIFY))
@_freed
def test_verify(k, m, sys_, P, R, dcls, ccls):
    """Clean stripes report nothing.  Then one word of check row 0, the last
    row of the coded region (F4: above the 4 GiB line), is corrupted in
    stripe 1: one value mismatch at that stripe, fragment and column, which
    only a compare with the right stored row reports."""
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, bool(sys_))
    no = plan.n_outputs
    R, data, enc, checks, counts, entries, dc, ctx = _repair_setup(plan, k, m, sys_, P, R)
    stored = np.stack([e[0] for e in enc])
    sl = _slot(k, sys_, int(checks[1, 0]))
    assert sl == k + m - 1 - (k if sys_ else 0)
    col = next(c for c in range(P // 2 + 7, P)
               if c not in set(int(v) for v in enc[1][1][sl, :enc[1][2][sl]]))
    for corrupt in (False, True):
        st = stored.copy()
        if corrupt:
            st[1, sl, col] ^= 0x0100
        coded = Rows(no, P, ccls, st)
        dd = Rows(k, P, dcls, data) if sys_ else None
        if ccls == "F4":
            assert sl == no - 1 and coded.offset(sl) >= GIB4
        wb = plan.verify_work_bytes(R, S, CAP)
        assert wb > 0
        work = torch.randint(0, 256, (wb,), dtype=torch.uint8, device="cuda")
        res = [torch.randint(0, 1 << 30, (S * R,), dtype=torch.int32, device="cuda")
               for _ in range(3)]
        err = plan.verify(ctx, dc, coded.view, work, CAP, res[0], res[1], res[2],
                          data=dd.view if sys_ else None, counts=counts, entries=entries,
                          cap=CAP)
        torch.cuda.synchronize()
        assert err == 0
        vm, mm, first = (r.cpu().numpy().view(np.uint32).reshape(S, R).astype(np.int64)
                         for r in res)
        evm = np.zeros((S, R), np.int64)
        efirst = np.full((S, R), NONE, np.int64)
        if corrupt:
            evm[1, 0], efirst[1, 0] = 1, col
        assert (vm == evm).all(), (corrupt, vm.tolist())
        assert (mm == 0).all(), (corrupt, mm.tolist())
        assert (first == efirst).all(), (corrupt, first.tolist(), col)
        _finish_all()
        for r in _LIVE:
            r.free()
        _LIVE.clear()
    assert plan.take_error() == 0


# ---- the NTT engine and the lazily built contexts --------------------------

NTT = [
    # k, m, sys, P, then_contiguous
    (300, 100, 0, 300, False),
    (1000, 24, 1, 512, False),
    (2000, 48, 0, 520, False),    # the multi-pass engine
    # whole tiles whose rows the matrix cores must refuse: the lazily built
    # NTT context; then a contiguous copy from the same context on the cores
    (300, 212, 0, 1024, True),
]
NTT_CLS = [("F4", "N"), ("N", "F4"), ("F2", "F2")]


@pytest.mark.parametrize("src,dst", NTT_CLS)
@pytest.mark.parametrize("k,m,sys_,P,cont", NTT, ids=_ids(*NTT))
@_freed
def test_ntt_encode(k, m, sys_, P, cont, src, dst):
    _encode_case(k, m, sys_, P, src, dst)


@pytest.mark.parametrize("src,dst", NTT_CLS)
@pytest.mark.parametrize("k,m,sys_,P,cont", NTT, ids=_ids(*NTT))
@_freed
def test_ntt_decode(k, m, sys_, P, cont, src, dst):
    """(systematic: both source regions in the class)"""
    _decode_case(k, m, sys_, P, src, src, dst, then_contiguous=cont, oracle_decode=k <= 300)


# ---- the top of the buffer range, on the matrix cores ----------------------

@pytest.mark.parametrize("k,m,sys_,P,src,dst", [
    (16, 48, 0, 1024, "B", "N"), (16, 48, 0, 1024, "N", "B"), (16, 48, 0, 1024, "B", "B"),
    (64, 960, 0, 2048, "B", "B"), (200, 56, 1, 1024, "B", "B"),
])
@_freed
def test_buffer_range_top_encode(k, m, sys_, P, src, dst):
    """Buffer loads out of range return 0 and stores are dropped, silently:
    a bounds slip would hide at the top of the range."""
    _encode_case(k, m, sys_, P, src, dst, encoder="matrix" if not sys_ else None,
                 want="_mfma_kernel<" if k <= 64 else "matrix_os_kernel<")


@pytest.mark.parametrize("k,m,sys_,P,dcls,ccls,ocls", [
    (16, 48, 0, 1024, "-", "B", "N"), (16, 48, 0, 1024, "-", "N", "B"),
    (16, 48, 0, 1024, "-", "B", "B"), (64, 960, 0, 2048, "-", "B", "B"),
    (200, 56, 1, 1024, "B", "B", "B"), (200, 56, 1, 1024, "B", "N", "N"),
    (600, 1400, 0, 1024, "-", "B", "B"),
])
@_freed
def test_buffer_range_top_decode(k, m, sys_, P, dcls, ccls, ocls):
    import quadiron_amd as qa
    names = qa.Plan(k, m, bool(sys_)).kernels(P).split("decode=")[1]
    assert "matrix_mfma_kernel<" in names or "matrix_os_kernel<" in names, names
    _decode_case(k, m, sys_, P, dcls, ccls, ocls, oracle_decode=k <= 300)
