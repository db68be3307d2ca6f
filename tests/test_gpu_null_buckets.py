"""GPU: the NULL bucket arguments of the device C-ABI (include/qi_gpu.h), on
every entry point that has them and in every kernel family: an encode that
records nothing, decodes and repairs whose rows carry marks nobody passes,
a verify without stored buckets, partial and syndrome shares without out
buckets.  Each is a runtime branch of its own in the kernels.

Every case has two stripes, OOR columns crafted into stripe 0 and at least
one mark among the rows concerned (a NULL branch with nothing to drop cannot
go wrong); tests/test_null_buckets_inputs.py checks that on the CPU, from the
oracle alone.  The expectations are the oracle's (encode; the decode of the
stored symbols with all counts zero -- the unique interpolation of what is
stored, so every decode algorithm must agree) or the exact integer model of
the repair matrix.  Everything is compared bit for bit.  Each case asserts
the kernel family it is there for and ends with take_error() == 0."""
import functools

import numpy as np
import pytest

from qi_testlib import (FILL, Q, craft_dense_oor, craft_oor_columns, crafted_repair,
                        matvec_mod, oracle_decode_blocks, oracle_encode_blocks, pattern_rows)
from test_gpu_partial import _matrix as _partial_matrix, _model as _partial_model
from test_gpu_syndrome import _points
from test_gpu_verify import NONE, _matrix as _repair_matrix, _slot

pytestmark = pytest.mark.gpu

S = 2          # stripe 0: crafted OOR columns; stripe 1: plain
MARK = 65536
FILL32 = 0x5A5A5A5A


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    torch.cuda.set_device(0)
    return torch


def _u8(rows):
    return np.ascontiguousarray(rows).view(np.uint8).reshape(rows.shape[0], -1)


def _dev16(torch, a):
    return torch.from_numpy(np.array(a, np.uint16).view(np.int16)).cuda()   # (a copy:
    # the cases are read-only)


def _dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).reshape(-1)).cuda()


def _family(names, fam):
    print("\n" + names)
    assert fam in names, (fam, names)


def _encode_oracle(k, m, sys_, data, cap):
    """per stripe: (rows u16 (n_outputs, P), oor (n_outputs, cap), counts)"""
    P = data.shape[2]
    res = []
    for s in range(data.shape[0]):
        o, oor, cnt = oracle_encode_blocks(k, m, sys_, _u8(data[s]), cap)
        assert cnt.max() <= cap
        res.append((o.view(np.uint16).reshape(-1, P), oor, cnt))
    return res


def _bucket_tensors(torch, enc):
    return (_dev32(torch, np.stack([e[2] for e in enc])),
            _dev32(torch, np.stack([e[1] for e in enc])))


# ---- A1. encode with NULL counts ----------------------------------------------

ENCODE_CASES = [
    # k, m, sys, P, encoder, family
    # the register codelets
    (3, 3, 0, 300, None, "encode_fnt_kernel<4,"),
    (16, 48, 0, 1100, None, "encode_fnt_kernel<16,"),
    (32, 32, 0, 513, None, "encode_fnt_kernel<32,"),
    (33, 31, 0, 513, "codelets", "encode_fnt_kernel<64,"),
    # the matrix cores
    (16, 48, 1, 1024, None, "matrix_mfma_kernel<1,"),
    (16, 48, 0, 1024, "matrix", "matrix_mfma_kernel<1,"),
    (64, 960, 0, 1024, None, "gen_mfma_kernel"),
    # the dot2 kernel over a ragged width
    (100, 28, 0, 300, None, "matrix_kernel<64,"),
    (200, 56, 1, 513, None, "matrix_kernel<128,"),
    # the operand-stationary kernel at KS = 8 / 16 / 20 / 24 / 40
    (100, 28, 0, 1024, None, "matrix_os_kernel<8,"),
    (200, 56, 0, 1024, None, "matrix_os_kernel<16,"),
    (300, 212, 0, 1024, None, "matrix_os_kernel<20,"),
    (384, 100, 1, 1024, None, "matrix_os_kernel<24,"),
    (385, 127, 1, 1024, None, "matrix_os_kernel<40,"),
    # the NTT engine: LDS at n = 512 and 1024, the erasure solve, multi-pass
    (257, 255, 0, 24, None, "ntt_lds_kernel"),
    (513, 511, 0, 19, None, "ntt_lds_kernel"),
    (450, 62, 1, 24, None, "ntt_eras_kernel"),
    (1990, 58, 0, 24, None, "ntt_pass_kernel"),
]


@functools.lru_cache(maxsize=None)
def encode_case(k, m, sys_, P):
    """(data (S, k, P) u16, the oracle's encode per stripe), read-only"""
    rng = np.random.default_rng([k, m, sys_, P, 1])
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    craft_oor_columns(k, m, sys_, data[0], rng, min(P, 24))
    enc = _encode_oracle(k, m, sys_, data, P)
    data.setflags(write=False)
    return data, enc


def encode_case_marks(k, m, sys_, P):
    """the marks of stripe 0's outputs, and whether each is stored as 0"""
    _, enc = encode_case(k, m, sys_, P)
    rows, oor, cnt = enc[0]
    zero = all((rows[i, oor[i, :cnt[i]]] == 0).all() for i in range(rows.shape[0]))
    return int(cnt.sum()), zero


@pytest.mark.parametrize("k,m,sys_,P,encoder,fam", ENCODE_CASES)
def test_encode_null_counts(hip_lib, k, m, sys_, P, encoder, fam):
    """Rows equal the oracle's, which hold 0 where the symbol is 65536; the
    guard row behind each stripe's outputs keeps its fill."""
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, sys_, encoder=encoder)
    names = plan.kernels(P)
    _family(names[:names.index("; decode=")], fam)
    data, enc = encode_case(k, m, sys_, P)
    n_marks, zero = encode_case_marks(k, m, sys_, P)
    assert n_marks > 0 and zero
    no = plan.n_outputs
    big = torch.full((S, no + 1, P), FILL, dtype=torch.int16, device="cuda")
    plan.encode(_dev16(torch, data), big[:, :no])
    torch.cuda.synchronize()
    got = big.cpu().numpy().view(np.uint16)
    for s in range(S):
        bad = np.argwhere(got[s, :no] != enc[s][0])
        assert len(bad) == 0, (s, len(bad), bad[:4].tolist())
    assert (got[:, no] == FILL).all()
    assert plan.take_error() == 0


# ---- A2 / A3. decode and decode_packed with NULL counts ------------------------

DECODE_CASES = [
    # k, m, sys, P, family
    (16, 48, 0, 1100, "matrix_mfma_kernel<1,"),
    (32, 32, 0, 1024, "matrix_mfma_kernel<2,"),
    (100, 28, 0, 1024, "matrix_os_kernel<8,"),
    (200, 56, 1, 1000, "matrix_kernel<128,"),
    (300, 212, 0, 1024, "matrix_os_kernel<20,"),
    (600, 1400, 0, 1024, "matrix_os_kernel<40,"),
    (300, 100, 1, 300, "ntt_lds_kernel"),
    (450, 62, 0, 24, "ntt_eras_kernel"),
    (1100, 100, 0, 64, "ntt_pass_kernel"),   # multi-pass interpolate
]
# a context built WITH routed buckets, then a decode given NULL counts
MIXED_CASES = [
    (16, 48, 0, 1024, "matrix_mfma_kernel<1,"),
    (200, 56, 0, 1024, "matrix_os_kernel<16,"),
    (300, 100, 0, 300, "ntt_lds_kernel"),
]
DENSE_CASE = (16, 48, 0, 2048, "matrix_mfma_kernel<1,")


class DecodeCase:
    """Two stripes of oracle-encoded data whose received coded rows carry
    marks, and the decode of the stored symbols alone: `exp` is the oracle's
    decode of the same rows with every count zero, `dropped[s]` the columns
    where a received row of stripe s has a mark."""

    def __init__(self, k, m, sys_, P, dense=False):
        self.k, self.m, self.sys_, self.P = k, m, sys_, P
        rng = np.random.default_rng([k, m, sys_, P, 2])
        while True:
            ids = np.sort(rng.choice(k + m, k, replace=False))
            if not sys_ or (ids >= k).sum() >= 2:
                break
        self.ids = np.ascontiguousarray(np.stack([ids, ids]), np.uint16)
        slots = [sl for sl in (_slot(k, sys_, int(f)) for f in ids) if sl is not None]
        self.slots = slots
        data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
        if dense:
            # two received rows at 65536 in each of the first 200 columns
            assert craft_dense_oor(k, m, data[0], rng, range(200), slots, 2) > 150
        else:
            craft_oor_columns(k, m, sys_, data[0], rng, min(P, 24), rows=slots)
        self.data = data
        self.enc = _encode_oracle(k, m, sys_, data, P)
        missing = np.ones(k + m, np.int32)
        missing[ids] = 0
        self.exp, self.dropped = [], []
        for s in range(S):
            rows, oor, cnt = self.enc[s]
            ok, full = oracle_decode_blocks(k, m, sys_, _u8(rows), oor, cnt, missing,
                                            _u8(data[s]))
            assert ok == 1 and (full == _u8(data[s])).all()
            ok, exp = oracle_decode_blocks(k, m, sys_, _u8(rows), oor, np.zeros_like(cnt),
                                           missing, _u8(data[s]))
            assert ok == 1
            self.exp.append(exp.view(np.uint16).reshape(k, P))
            cols = [oor[sl, :cnt[sl]] for sl in slots]
            self.dropped.append(np.unique(np.concatenate(cols)) if cols else
                                np.zeros(0, np.uint32))
        for a in (self.data, self.ids):
            a.setflags(write=False)

    def check_inputs(self):
        """not vacuous: dropping the marks changes stripe 0's decode, and only
        in columns that had one"""
        assert len(self.dropped[0]) > 0
        for s in range(S):
            diff = np.flatnonzero((self.exp[s] != self.data[s]).any(axis=0))
            assert np.isin(diff, self.dropped[s]).all(), s
        assert (self.exp[0] != self.data[0]).any()


@functools.lru_cache(maxsize=None)
def decode_case(k, m, sys_, P, dense=False):
    return DecodeCase(k, m, sys_, P, dense)


def dense_marks(c):
    """the marks of stripe 0's received rows in the first 256 columns"""
    _, oor, cnt = c.enc[0]
    return sum(int((oor[sl, :cnt[sl]] < 256).sum()) for sl in c.slots)


def _decode_both(plan, c, ctx_counts, dec_counts):
    """qi_gpu_decode and qi_gpu_decode_packed over the oracle's coded rows,
    the buckets given to the context builder and / or to the decode; returns
    both outputs (S, k, P) u16.  Contexts start from garbage."""
    torch = _torch()
    k, sys_, P = c.k, c.sys_, c.P
    no = plan.n_outputs
    coded = _dev16(torch, np.stack([e[0] for e in c.enc]))
    dd = _dev16(torch, c.data)
    counts, entries = _bucket_tensors(torch, c.enc)
    cap = P
    di = _dev16(torch, c.ids)
    marks = (counts, entries, cap)
    ctx = torch.randint(0, 256, (plan.ctx_bytes(S, P),), dtype=torch.uint8, device="cuda")
    plan.decode_ctx(di, ctx, P, *(marks if ctx_counts else ()))
    dec = torch.full((S, k, P), FILL, dtype=torch.int16, device="cuda")
    kw = dict(counts=counts, entries=entries, cap=cap) if dec_counts else {}
    assert plan.decode(ctx, di, coded, dec, data=dd if sys_ else None, **kw) == 0
    # the packed layout: received rows back to back, buckets by position
    idx = torch.from_numpy(c.ids.astype(np.int64)).cuda()
    cnt2, ent3 = counts.view(S, no), entries.view(S, no, cap)
    if sys_:
        full = torch.cat([dd, coded], dim=1)
        cnt2 = torch.cat([torch.zeros((S, k), dtype=torch.int32, device="cuda"), cnt2], dim=1)
        ent3 = torch.cat([torch.zeros((S, k, cap), dtype=torch.int32, device="cuda"), ent3],
                         dim=1)
    else:
        full = coded
    recv = torch.gather(full, 1, idx[:, :, None].expand(S, k, P)).contiguous()
    pmarks = (torch.gather(cnt2, 1, idx).contiguous().view(-1),
              torch.gather(ent3, 1, idx[:, :, None].expand(S, k, cap)).contiguous().view(-1), cap)
    ctx2 = torch.randint(0, 256, (plan.ctx_bytes(S, P),), dtype=torch.uint8, device="cuda")
    plan.decode_ctx_packed(di, ctx2, P, *(pmarks if ctx_counts else ()))
    dec2 = torch.full((S, k, P), FILL, dtype=torch.int16, device="cuda")
    assert plan.decode_packed(ctx2, recv, dec2, *(pmarks if dec_counts else ())) == 0
    torch.cuda.synchronize()
    return dec.cpu().numpy().view(np.uint16), dec2.cpu().numpy().view(np.uint16)


def _check_decode(c, outs, exp):
    for name, got in zip(("decode", "decode_packed"), outs):
        for s in range(S):
            bad = np.argwhere(got[s] != exp[s])
            assert len(bad) == 0, (name, s, len(bad), bad[:4].tolist())


def _decode_plan(k, m, sys_, P, fam):
    import quadiron_amd as qa
    plan = qa.Plan(k, m, sys_)
    names = plan.kernels(P)
    _family(names[names.index("; decode="):], fam)
    return plan


@pytest.mark.parametrize("k,m,sys_,P,fam", DECODE_CASES)
def test_decode_null_counts(hip_lib, k, m, sys_, P, fam):
    """NULL counts at context time and at decode time: no mark is restored,
    both layouts return the decode of the stored symbols."""
    plan = _decode_plan(k, m, sys_, P, fam)
    c = decode_case(k, m, sys_, P)
    c.check_inputs()
    _check_decode(c, _decode_both(plan, c, False, False), c.exp)
    assert plan.take_error() == 0


def test_decode_null_counts_dense(hip_lib):
    """More than 256 dropped marks in one tile: with NULL counts no slow-tile
    or redo path may run, from garbage."""
    k, m, sys_, P, fam = DENSE_CASE
    plan = _decode_plan(k, m, sys_, P, fam)
    c = decode_case(k, m, sys_, P, True)
    c.check_inputs()
    assert dense_marks(c) > 256
    _check_decode(c, _decode_both(plan, c, False, False), c.exp)
    assert plan.take_error() == 0


@pytest.mark.parametrize("k,m,sys_,P,fam", MIXED_CASES)
def test_decode_null_counts_after_routed_context(hip_lib, k, m, sys_, P, fam):
    """The buckets given to the context builder only (qi_gpu.h: NULL counts
    at decode time mean no marks, whatever the context holds): the same
    result on the matrix cores, the operand-stationary kernel and the NTT
    engine.  The same context then decodes to the data once the buckets are
    passed."""
    plan = _decode_plan(k, m, sys_, P, fam)
    c = decode_case(k, m, sys_, P)
    c.check_inputs()
    _check_decode(c, _decode_both(plan, c, True, False), c.exp)
    _check_decode(c, _decode_both(plan, c, True, True), c.data)
    assert plan.take_error() == 0


# ---- A4 / A5. repair and verify -------------------------------------------------

REPAIR_CASES = [
    # k, m, sys, R, P, family ({}: _both or _verify)
    (16, 48, 0, 3, 1100, "matrix_mfma_kernel{}<1,"),
    (16, 48, 1, 17, 1024, "matrix_mfma_kernel{}<1,"),
    (200, 56, 1, 8, 513, "matrix_kernel{}<128,"),
]
VERIFY_CASES = [
    (16, 48, 0, 3, 1100, "matrix_mfma_kernel{}<1,"),
    (200, 56, 1, 8, 1024, "matrix_os_kernel{}<16,"),
]


class RepairCase:
    """crafted_repair(k, m, sys, R, P) as stripe 0 (input marks at the
    largest coefficients, targets that are exactly 65536), with further OOR
    columns crafted on the received rows, and pattern_rows as stripe 1; the
    coded rows and buckets are the oracle's.  y_stored / y_restored (S, R, P):
    the repair matrix applied to the stored symbols of the received rows, and
    to the restored ones (65536 where the oracle marked)."""

    def __init__(self, k, m, sys_, R, P):
        self.k, self.m, self.sys_, self.R, self.P = k, m, sys_, R, P
        c = crafted_repair(k, m, sys_, R, P)
        self.ids = np.ascontiguousarray(np.stack([c.ids, c.ids]), np.uint16)
        self.targets = np.ascontiguousarray(np.stack([c.targets, c.targets]), np.uint16)
        rng = np.random.default_rng([k, m, sys_, R, P, 4])
        d0 = c.d.copy()
        slots = [sl for sl in (_slot(k, sys_, int(f)) for f in c.ids) if sl is not None]
        plain = np.flatnonzero(np.arange(P) % 4 != 0)   # not a crafted-mark or solved column
        for j in rng.choice(plain, 12, replace=False):
            craft_oor_columns(k, m, sys_, d0, rng, 1, rows=slots, col_range=(int(j), int(j) + 1))
        self.data = np.stack([d0, pattern_rows(k, P)])
        self.enc = _encode_oracle(k, m, sys_, self.data, P)
        A = _repair_matrix(k, m, sys_, c.ids, c.targets)
        assert (A == c.A).all()
        self.y_stored = np.zeros((S, R, P), np.int64)
        self.y_restored = np.zeros((S, R, P), np.int64)
        self.in_marks = 0
        for s in range(S):
            rows, oor, cnt = self.enc[s]
            x = np.zeros((k, P), np.int64)
            xr = np.zeros((k, P), np.int64)
            for i, f in enumerate(c.ids):
                sl = _slot(k, sys_, int(f))
                x[i] = self.data[s, int(f)] if sl is None else rows[sl]
                xr[i] = x[i]
                if sl is not None:
                    xr[i, oor[sl, :cnt[sl]]] = MARK
                    self.in_marks += int(cnt[sl]) if s == 0 else 0
            self.y_stored[s] = matvec_mod(A, x)
            self.y_restored[s] = matvec_mod(A, xr)
        self.data.setflags(write=False)

    def stored_target(self, s, j):
        """(stored row u16, its mark columns) of target j: the oracle's"""
        t = int(self.targets[s, j])
        sl = _slot(self.k, self.sys_, t)
        if sl is None:
            return self.data[s, t], np.zeros(0, np.int64)
        rows, oor, cnt = self.enc[s]
        return rows[sl], np.sort(oor[sl, :cnt[sl]].astype(np.int64))

    def check_inputs(self):
        assert self.in_marks > 0
        # a 65536 is rebuilt from the stored symbols and from the restored ones
        assert (self.y_stored[0] == MARK).any() and (self.y_restored[0] == MARK).any()
        # dropping the input marks changes the result
        assert (self.y_stored[0] != self.y_restored[0]).any()
        # the restored model is the oracle's encode of the targets
        for s in range(S):
            for j in range(self.R):
                row, mk = self.stored_target(s, j)
                assert ((self.y_restored[s, j] & 0xffff) == row).all()
                assert np.array_equal(np.flatnonzero(self.y_restored[s, j] == MARK), mk)


@functools.lru_cache(maxsize=None)
def repair_case(k, m, sys_, R, P):
    return RepairCase(k, m, sys_, R, P)


def _repair_setup(torch, plan, c, ctx_counts):
    coded = _dev16(torch, np.stack([e[0] for e in c.enc]))
    dd = _dev16(torch, c.data) if c.sys_ else None
    counts, entries = _bucket_tensors(torch, c.enc)
    di, dt = _dev16(torch, c.ids), _dev16(torch, c.targets)
    nb = plan.repair_ctx_bytes(c.R, S, c.P)
    assert nb > 0
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    plan.repair_ctx(di, dt, ctx, c.P, *((counts, entries, c.P) if ctx_counts else ()))
    return coded, dd, counts, entries, dt, ctx


def _repair_family(plan, R, P, fam):
    """qi_gpu_repair_kernels names the route of a repair with both bucket
    sets, the _both forms.  With one set NULL the launch takes the same route
    in its plain forms (matrix_route: both = in marks and out marks), e.g.
    matrix_mfma_kernel<1, ...> for matrix_mfma_kernel_both<1, ...>: the
    report is checked for the family, and the plain name is what runs."""
    names = plan.repair_kernels(R, P)
    _family(names, fam.format("_both"))
    print("launched with one bucket set NULL: " + names.replace("_both", ""))


@pytest.mark.parametrize("ctx_counts", [False, True])
@pytest.mark.parametrize("k,m,sys_,R,P,fam", REPAIR_CASES)
def test_repair_null_in_counts(hip_lib, k, m, sys_, R, P, fam, ctx_counts):
    """NULL in-counts at the repair call, out buckets given -- the context
    built without buckets, or WITH them (qi_gpu.h: NULL counts mean no marks
    whatever the context holds): the rows are the repair matrix applied to
    the stored symbols, with marks exactly where that gives 65536."""
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, sys_)
    _repair_family(plan, R, P, fam)
    c = repair_case(k, m, sys_, R, P)
    c.check_inputs()
    coded, dd, _, _, _, ctx = _repair_setup(torch, plan, c, ctx_counts)
    out = torch.full((S, R, P), FILL, dtype=torch.int16, device="cuda")
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.full((S * R * P,), -1, dtype=torch.int32, device="cuda")
    assert plan.repair(ctx, coded, out, data=dd, out_counts=oc, out_entries=oe, out_cap=P) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    gc = oc.cpu().numpy().view(np.uint32).reshape(S, R)
    ge = oe.cpu().numpy().view(np.uint32).reshape(S, R, P)
    for s in range(S):
        for j in range(R):
            y = c.y_stored[s, j]
            assert (got[s, j] == (y & 0xffff)).all(), (s, j, np.flatnonzero(
                got[s, j] != (y & 0xffff))[:8])
            em = np.flatnonzero(y == MARK)
            assert gc[s, j] == len(em), (s, j, gc[s, j], len(em))
            assert np.array_equal(np.sort(ge[s, j, :gc[s, j]]), em), (s, j)
    assert plan.take_error() == 0


@pytest.mark.parametrize("k,m,sys_,R,P,fam", REPAIR_CASES)
def test_repair_null_out_counts(hip_lib, k, m, sys_, R, P, fam):
    """In buckets given, NULL out counts: the rows are the repair matrix
    applied to the restored symbols (the oracle's rows of the targets, 65536
    stored as 0), and the out-entries tensor keeps its fill."""
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, sys_)
    _repair_family(plan, R, P, fam)
    c = repair_case(k, m, sys_, R, P)
    c.check_inputs()
    coded, dd, counts, entries, _, ctx = _repair_setup(torch, plan, c, True)
    out = torch.full((S, R, P), FILL, dtype=torch.int16, device="cuda")
    oe = torch.full((S * R * P,), FILL32, dtype=torch.int32, device="cuda")
    assert plan.repair(ctx, coded, out, data=dd, counts=counts, entries=entries, cap=P,
                       out_counts=None, out_entries=oe, out_cap=P) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    for s in range(S):
        for j in range(R):
            y = c.y_restored[s, j]
            assert (got[s, j] == (y & 0xffff)).all(), (s, j, np.flatnonzero(
                got[s, j] != (y & 0xffff))[:8])
    assert (oe.cpu().numpy() == FILL32).all()
    assert plan.take_error() == 0


def verify_expect(c):
    """(value_mismatch, mark_mismatch, first) (S, R) of a verify without
    buckets, by the header's definitions: v is the repair matrix applied to
    the stored basis symbols (a dropped basis mark shows as a value
    mismatch), and every v == 65536 is a mark mismatch."""
    vm = np.zeros((S, c.R), np.int64)
    mm = np.zeros((S, c.R), np.int64)
    first = np.full((S, c.R), NONE, np.int64)
    for s in range(S):
        for j in range(c.R):
            v = c.y_stored[s, j]
            stored, _ = c.stored_target(s, j)
            bad_v = (v & 0xffff) != stored
            bad_m = v == MARK
            vm[s, j], mm[s, j] = bad_v.sum(), bad_m.sum()
            both = np.flatnonzero(bad_v | bad_m)
            if len(both):
                first[s, j] = both[0]
    return vm, mm, first


@pytest.mark.parametrize("k,m,sys_,R,P,fam", VERIFY_CASES)
def test_verify_null_counts(hip_lib, k, m, sys_, R, P, fam):
    """NULL d_oor_counts (context and verify): every recomputed 65536 is a
    mark mismatch, dropped basis marks show as value mismatches."""
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, sys_)
    _family(plan.verify_kernels(R, P), fam.format("_verify"))
    c = repair_case(k, m, sys_, R, P)
    c.check_inputs()
    evm, emm, efirst = verify_expect(c)
    assert evm.sum() > 0 and emm.sum() > 0
    coded, dd, _, _, dt, ctx = _repair_setup(torch, plan, c, False)
    wcap = P
    work = torch.randint(0, 256, (plan.verify_work_bytes(R, S, wcap),), dtype=torch.uint8,
                         device="cuda")
    res = [torch.randint(0, 1 << 30, (S * R,), dtype=torch.int32, device="cuda")
           for _ in range(3)]
    assert plan.verify(ctx, dt, coded, work, wcap, res[0], res[1], res[2], data=dd) == 0
    torch.cuda.synchronize()
    vm, mm, first = (r.cpu().numpy().view(np.uint32).reshape(S, R).astype(np.int64) for r in res)
    print("value", vm.tolist(), "expected", evm.tolist())
    print("mark", mm.tolist(), "expected", emm.tolist())
    print("first", first.tolist(), "expected", efirst.tolist())
    assert (vm == evm).all() and (mm == emm).all() and (first == efirst).all()
    assert plan.take_error() == 0


# ---- A6. partial and syndrome shares with NULL out counts ----------------------

PARTIAL_CASES = [
    # k, m, sys, H, R, P, family
    (16, 48, 1, 5, 3, 37, "partial_kernel<4,"),
    (300, 212, 0, 16, 8, 1024, "partial_kernel<8,"),
]
SYNDROME_CASE = (16, 48, 0, 4, 4, 37, "partial_kernel<4,")


def _fragments(k, m, sys_, data):
    """one stripe's fragments by id: stored rows u16 (k + m, P) and their
    mark lists, from the oracle's encode"""
    P = data.shape[1]
    rows, oor, cnt = _encode_oracle(k, m, sys_, data[None], P)[0]
    marks = [[int(v) for v in oor[j, :cnt[j]]] for j in range(rows.shape[0])]
    if sys_:
        return np.concatenate([data, rows]), [[] for _ in range(k)] + marks
    return rows, marks


class ShareCase:
    """Held rows of two oracle-encoded stripes (stripe 0 with OOR columns
    crafted on the held coded rows), by position: ids (S, N), held (S, H),
    rows (S, H, P) u16 as stored and marks[s][h]."""

    def __init__(self, k, m, sys_, H, P, N, seed):
        rng = np.random.default_rng([k, m, sys_, H, P, seed])
        perm = rng.permutation(k + m)
        ids1 = perm[:N]
        held1 = rng.permutation(N)
        if sys_:   # two parity rows first: data rows carry no marks
            par = np.flatnonzero(ids1 >= k)[:2]
            assert len(par) == 2
            held1 = np.concatenate([par, held1[~np.isin(held1, par)]])
        held1 = held1[:H]
        self.extra = perm[N:]
        self.ids = np.ascontiguousarray(np.stack([ids1, ids1]), np.uint16)
        self.held = np.ascontiguousarray(np.stack([held1, held1]), np.uint16)
        fr = ids1[held1]
        slots = [sl for sl in (_slot(k, sys_, int(f)) for f in fr) if sl is not None]
        data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
        craft_oor_columns(k, m, sys_, data[0], rng, min(P, 24), rows=slots)
        self.rows = np.zeros((S, H, P), np.uint16)
        self.marks = []
        for s in range(S):
            frows, fmarks = _fragments(k, m, sys_, data[s])
            self.rows[s] = frows[fr]
            self.marks.append([fmarks[int(f)] for f in fr])
        self.n_marks = sum(len(mk) for mk in self.marks[0])
        marked = {c for mk in self.marks[0] for c in mk}
        self.free = [c for c in range(P) if c not in marked]   # stripe 0: no held mark


@functools.lru_cache(maxsize=None)
def partial_case(k, m, sys_, H, R, P):
    """(ShareCase, targets (S, R), expected symbols (S, R, P) in 0..65536):
    one held symbol of R columns of stripe 0 is solved so that target
    t's partial sum is exactly 65536 in the t-th column without a held mark"""
    c = ShareCase(k, m, sys_, H, P, k, 6)
    tg = c.extra[:R]
    targets = np.ascontiguousarray(np.stack([tg, tg]), np.uint16)
    M = _partial_matrix(k, m, sys_, tuple(int(v) for v in c.ids[0]), tuple(int(v) for v in tg))
    held = c.held[0].astype(np.int64)

    def model(s):
        return _partial_model(k, m, sys_, c.ids[s], c.held[s], targets[s], c.rows[s],
                              c.marks[s])
    for t in range(R):
        col = c.free[t]
        co = int(M[t, held[0]])
        assert co != 0
        c.rows[0, 0, col] = 0
        base = int(model(0)[t, col])
        y = (MARK - base) * pow(co, Q - 2, Q) % Q
        if y < MARK:
            c.rows[0, 0, col] = y
    exp = np.stack([model(s) for s in range(S)])
    return c, targets, exp


@pytest.mark.parametrize("k,m,sys_,H,R,P,fam", PARTIAL_CASES)
def test_partial_null_out_counts(hip_lib, k, m, sys_, H, R, P, fam):
    """In buckets given, NULL out counts: the rows are the model's symbols
    with 65536 stored as 0; the out-entries tensor keeps its fill."""
    import quadiron_amd as qa
    torch = _torch()
    plan = qa.Plan(k, m, bool(sys_))
    _family(plan.partial_kernels(H, R, P), fam)
    c, targets, exp = partial_case(k, m, sys_, H, R, P)
    assert c.n_marks > 0 and (exp[0] == MARK).any()
    ctx = torch.randint(0, 256, (plan.partial_ctx_bytes(H, R, S),), dtype=torch.uint8,
                        device="cuda")
    plan.partial_ctx(_dev16(torch, c.ids), _dev16(torch, c.held), _dev16(torch, targets), ctx)
    cnt = np.zeros((S, H), np.uint32)
    ent = np.zeros((S, H, P), np.uint32)
    for s in range(S):
        for h in range(H):
            cnt[s, h] = len(c.marks[s][h])
            ent[s, h, :cnt[s, h]] = c.marks[s][h]
    out = torch.full((S, R, P), FILL, dtype=torch.int16, device="cuda")
    oe = torch.full((S * R * P,), FILL32, dtype=torch.int32, device="cuda")
    assert plan.partial(ctx, _dev16(torch, c.rows), out, counts=_dev32(torch, cnt),
                        entries=_dev32(torch, ent), cap=P, out_counts=None, out_entries=oe,
                        out_cap=P) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    bad = np.argwhere(got != (exp & 0xffff))
    assert len(bad) == 0, (len(bad), bad[:4].tolist())
    assert (oe.cpu().numpy() == FILL32).all()
    assert plan.take_error() == 0


@functools.lru_cache(maxsize=None)
def syndrome_case(k, m, sys_, H, R, P):
    """(ShareCase over N = k + R listed ids, expected symbols (S, R, P)): the
    shares sum_h (x_h^j / w_h) y_h of the STORED symbols y_h (no in buckets),
    with one held symbol of column 1 + j of stripe 0 solved so that syndrome
    j is exactly 65536 there"""
    c = ShareCase(k, m, sys_, H, P, k + R, 7)
    x, w = _points(k, m, c.ids[0])
    held = c.held[0].astype(np.int64)
    C = np.array([[pow(int(x[p]), j, Q) * pow(int(w[p]), Q - 2, Q) % Q for p in held]
                  for j in range(R)], np.int64)
    for j in range(R):
        col = 1 + j
        rest = int(matvec_mod(C[j:j + 1, 1:], c.rows[0, 1:, col:col + 1].astype(np.int64))[0, 0])
        y = (MARK - rest) * pow(int(C[j, 0]), Q - 2, Q) % Q
        if y < MARK:
            c.rows[0, 0, col] = y
    exp = np.stack([matvec_mod(C, c.rows[s].astype(np.int64)) for s in range(S)])
    return c, exp


def test_syndrome_null_counts(hip_lib):
    """NULL in counts and NULL out counts: the shares of the stored symbols,
    65536 stored as 0."""
    import quadiron_amd as qa
    torch = _torch()
    k, m, sys_, H, R, P, fam = SYNDROME_CASE
    plan = qa.Plan(k, m, bool(sys_))
    _family(plan.syndrome_kernels(H, R, P), fam)
    c, exp = syndrome_case(k, m, sys_, H, R, P)
    assert c.n_marks > 0 and (exp[0] == MARK).any()
    ctx = torch.randint(0, 256, (plan.syndrome_ctx_bytes(H, R, S),), dtype=torch.uint8,
                        device="cuda")
    plan.syndrome_ctx(_dev16(torch, c.ids), _dev16(torch, c.held), ctx)
    out = torch.full((S, R, P), FILL, dtype=torch.int16, device="cuda")
    oe = torch.full((S * R * P,), FILL32, dtype=torch.int32, device="cuda")
    assert plan.syndrome(ctx, _dev16(torch, c.rows), out, out_counts=None, out_entries=oe,
                         out_cap=P) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    bad = np.argwhere(got != (exp & 0xffff))
    assert len(bad) == 0, (len(bad), bad[:4].tolist())
    assert (oe.cpu().numpy() == FILL32).all()
    assert plan.take_error() == 0
