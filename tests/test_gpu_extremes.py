"""The kernels at their accumulator extremes, bit-exact against the oracle.

The kernels' correctness rests on range arguments (the dot2 accumulator
below 2^31, the matrix cores' 256 D2 + D1 - D0 with D2 folded first from
KS = 16 up and carried over two K chunks at KS = 40, the NTT engine's lazy
24-bit multiplies) that uniform random symbols never come near: their sums
are a random walk.  These tests feed columns crafted from the codes' own
matrices (qi_testlib craft_columns; tests/test_extreme_inputs.py shows on
the CPU that they reach what they claim) and the 0x00 / 0xFF / 0x80 / 0x7F
planes stored files are full of.  Fused repair and verify get the same from
columns crafted against their own R x k matrix (qi_testlib crafted_repair),
with the helpers of test_gpu_repair.py and test_gpu_verify.py.  Each case
names the kernel family it is there for and asserts that the plan routes to
it.  Run with -m gpu."""
import functools

import numpy as np
import pytest

from qi_testlib import (ALL_MODES, craft_columns, craft_received, crafted_repair,
                        extreme_targets, generator_matrix, oracle_decode_blocks,
                        oracle_encode_blocks, pattern_rows)
from test_gpu_repair import _encode_oracle, _repair_and_check, _slot
from test_gpu_verify import NONE, Stripes, _check as _verify_check

pytestmark = pytest.mark.gpu

S = 2   # stripe 0: crafted columns, stripe 1: pattern_rows


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@functools.lru_cache(maxsize=None)
def _gen(k, m, sys_):
    G = generator_matrix(k, m, sys_)
    G.setflags(write=False)
    return G


def _routes(plan, P, side, fam):
    """The kernel family a case is there for, in the encode or decode half
    of the plan's kernel list (a routing change must not move the coverage
    elsewhere unnoticed)."""
    names = plan.kernels(P)
    enc, dec = names[len("encode="):].split("; decode=")
    print(f"\n{(plan.k, plan.m, int(plan.sys), P)}: {names}")
    assert fam in (enc if side == "encode" else dec), (side, fam, names)


class _Batch:
    """S stripes encoded on the device, their outputs and OOR buckets on the
    host, and the oracle's encode of each stripe."""

    def __init__(self, plan, k, m, sys_, data):
        torch = _torch()
        self.plan, self.k, self.m, self.sys_, self.data = plan, k, m, sys_, data
        P = self.P = data.shape[2]
        no = self.no = plan.n_outputs
        self.cap = cap = P   # a row holds at most P marks: no bucket overflows
        self.dd = torch.from_numpy(data.view(np.int16)).cuda()
        self.out = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
        self.counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
        self.entries = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
        plan.encode(self.dd, self.out, self.counts, self.entries, cap)
        torch.cuda.synchronize()
        assert plan.take_error() == 0
        self.out_h = self.out.cpu().numpy().view(np.uint16)
        self.cnt_h = self.counts.cpu().numpy().view(np.uint32).reshape(S, no)
        self.ent_h = self.entries.cpu().numpy().view(np.uint32).reshape(S, no, cap)
        self.oracle = [oracle_encode_blocks(k, m, sys_, self.bytes(data[s]), cap)
                       for s in range(S)]

    def bytes(self, rows):
        return np.ascontiguousarray(rows).view(np.uint8).reshape(rows.shape[0], 2 * self.P)

    def marks(self, s, i):
        return np.sort(self.ent_h[s, i, :self.cnt_h[s, i]])

    def check_encode(self):
        """Outputs, counts and sorted mark lists of every stripe, whole block."""
        for s in range(S):
            o_out, o_oor, o_cnt = self.oracle[s]
            bad = np.argwhere(self.bytes(self.out_h[s]) != o_out)
            assert len(bad) == 0, (s, len(bad), bad[:4].tolist())
            assert (self.cnt_h[s] == o_cnt).all(), s
            for i in range(self.no):
                assert (self.marks(s, i) == o_oor[i, :o_cnt[i]]).all(), (s, i)

    def check_decode(self, ids):
        """Both decode layouts from the received `ids` (S, k), every stripe,
        against the data and the oracle's decode of the oracle's encode."""
        torch = _torch()
        plan, k, m, P, cap, no = self.plan, self.k, self.m, self.P, self.cap, self.no
        ids = np.ascontiguousarray(ids, np.uint16)
        di = torch.from_numpy(ids.view(np.int16)).cuda()
        ctx = torch.randint(0, 256, (plan.ctx_bytes(S, P),), dtype=torch.uint8, device="cuda")
        plan.decode_ctx(di, ctx, P, self.counts, self.entries, cap, h_ids=ids)
        dec = torch.zeros((S, k, P), dtype=torch.int16, device="cuda")
        assert plan.decode(ctx, di, self.out, dec, data=self.dd, counts=self.counts,
                           entries=self.entries, cap=cap) == 0
        torch.cuda.synchronize()
        dec_h = dec.cpu().numpy().view(np.uint16)
        # the packed layout: received rows back to back, buckets by position
        idx = torch.from_numpy(ids.astype(np.int64)).cuda()
        cnt2, ent3 = self.counts.view(S, no), self.entries.view(S, no, cap)
        if self.sys_:
            full = torch.cat([self.dd, self.out], dim=1)
            fcnt = torch.cat([torch.zeros((S, k), dtype=torch.int32, device="cuda"), cnt2], dim=1)
            fent = torch.cat([torch.zeros((S, k, cap), dtype=torch.int32, device="cuda"), ent3],
                             dim=1)
        else:
            full, fcnt, fent = self.out, cnt2, ent3
        recv = torch.gather(full, 1, idx[:, :, None].expand(S, k, P)).contiguous()
        pcnt = torch.gather(fcnt, 1, idx).contiguous()
        pent = torch.gather(fent, 1, idx[:, :, None].expand(S, k, cap)).contiguous()
        ctx2 = torch.full_like(ctx, 0xA5)
        plan.decode_ctx_packed(di, ctx2, P, pcnt, pent, cap, h_ids=ids)
        dec2 = torch.zeros_like(dec)
        assert plan.decode_packed(ctx2, recv, dec2, pcnt, pent, cap) == 0
        torch.cuda.synchronize()
        dec2_h = dec2.cpu().numpy().view(np.uint16)
        for s in range(S):
            missing = np.ones(k + m, np.int32)
            missing[ids[s].astype(np.int64)] = 0
            o_out, o_oor, o_cnt = self.oracle[s]
            ok, o_dec = oracle_decode_blocks(k, m, self.sys_, o_out, o_oor, o_cnt, missing,
                                             self.bytes(self.data[s]))
            assert ok == 1 and (o_dec == self.bytes(self.data[s])).all(), s
            for name, got in (("decode", dec_h[s]), ("decode_packed", dec2_h[s])):
                bad = np.argwhere(got != self.data[s])
                assert len(bad) == 0, (name, s, len(bad), bad[:4].tolist())
                assert (self.bytes(got) == o_dec).all(), (name, s)


def _sorted_subset(rng, k, m):
    return np.sort(rng.choice(k + m, k, replace=False))


@pytest.mark.parametrize("k,m,sys_,P,encoder,fam", [
    # the register FNT codelets
    (16, 48, 0, 300, None, "encode_fnt_kernel<16,"),
    (32, 32, 0, 1024, None, "encode_fnt_kernel<32,"),
    (33, 31, 0, 513, "codelets", "encode_fnt_kernel<64,"),
    (64, 960, 0, 1024, None, "gen_mfma_kernel"),
    # the matrix cores at KS = 8 / 16 / 20 / 24, the largest k of each
    (128, 128, 0, 1024, None, "matrix_os_kernel<8,"),
    (256, 768, 0, 1024, None, "matrix_os_kernel<16,"),
    (320, 100, 0, 1024, None, "matrix_os_kernel<20,"),
    (384, 128, 0, 1024, None, "matrix_os_kernel<24,"),
    # the dot2 kernel (ragged widths below one tile)
    (128, 128, 0, 300, None, "matrix_kernel<64,"),
    (200, 56, 0, 300, None, "matrix_kernel<128,"),
    # the NTT engine: LDS (n = 512, 1024) and multi-pass (len_2k = 4096)
    (257, 255, 0, 300, None, "ntt_lds_kernel"),
    (385, 127, 0, 1024, None, "ntt_lds_kernel"),
    (1000, 24, 0, 264, None, "ntt_lds_kernel"),
    (2000, 48, 0, 256, None, "ntt_pass_kernel"),
    # systematic: generators on the matrix cores (KS = 1, 8, 40), the
    # erasure solve as the encode, the interpolating NTT encode
    (16, 48, 1, 1024, None, "matrix_mfma_kernel<1,"),
    (100, 50, 1, 1024, None, "matrix_os_kernel<8,"),
    (640, 384, 1, 1024, None, "matrix_os_kernel<40,"),
    (448, 64, 1, 1000, None, "ntt_eras_kernel"),
    (300, 100, 1, 300, None, "ntt_lds_kernel"),
])
def test_encode_extremes_vs_oracle(k, m, sys_, P, encoder, fam):
    """Stripe 0: one column per (generator row, mode) pair that drives that
    output's accumulators to the dot2 / D2 / D0 + D1 extremes; stripe 1: the
    constant and alternating planes.  Outputs, counts and marks equal the
    oracle's over the whole block, and each stripe decodes back to its data
    from a seeded sorted k-subset."""
    import quadiron_amd as qa
    plan = qa.Plan(k, m, sys_, encoder=encoder)
    _routes(plan, P, "encode", fam)
    G = _gen(k, m, sys_)
    X, _ = craft_columns(G, extreme_targets(G), ALL_MODES, P)
    data = np.stack([X.astype(np.uint16), pattern_rows(k, P)])
    b = _Batch(plan, k, m, sys_, data)
    b.check_encode()
    rng = np.random.default_rng(1000 * k + m + P)
    b.check_decode(np.stack([_sorted_subset(rng, k, m) for _ in range(S)]))


def _ids_for(kind, rng, k, m):
    if kind == "random":
        return _sorted_subset(rng, k, m)
    if kind == "parity":   # as many parity rows as the code has
        par = k + (rng.choice(m, k, replace=False) if m >= k else np.arange(m))
        return np.sort(np.concatenate([rng.choice(k, k - len(par), replace=False), par]))
    assert kind == "one_data" and m >= k - 1
    return np.sort(np.concatenate([[rng.integers(k)], k + rng.choice(m, k - 1, replace=False)]))


@pytest.mark.parametrize("k,m,sys_,P,ids_kind,fam", [
    # the matrix cores at KS = 1 / 2 / 4 / 8 / 16 / 20 / 24 / 40 (one whole
    # 1024-column tile), the largest k of each K-step
    (16, 48, 0, 1024, "random", "matrix_mfma_kernel<1,"),
    (32, 32, 0, 1024, "random", "matrix_mfma_kernel<2,"),
    (64, 960, 0, 1024, "random", "matrix_os_kernel<4,"),
    (128, 128, 0, 1024, "random", "matrix_os_kernel<8,"),
    (256, 768, 0, 1024, "random", "matrix_os_kernel<16,"),
    (320, 100, 0, 1024, "random", "matrix_os_kernel<20,"),
    (384, 128, 0, 1024, "random", "matrix_os_kernel<24,"),
    (640, 384, 0, 1024, "random", "matrix_os_kernel<40,"),
    # the dot2 kernel
    (16, 48, 0, 300, "random", "matrix_kernel<8,"),
    (128, 128, 0, 300, "random", "matrix_kernel<64,"),
    (256, 768, 0, 300, "random", "matrix_kernel<128,"),
    # systematic: two source regions; m < k - 1 for both codes, so "parity"
    # receives every parity row the code has and fills up with data rows
    (100, 50, 1, 1024, "random", "matrix_os_kernel<8,"),
    (100, 50, 1, 1024, "parity", "matrix_os_kernel<8,"),
    (640, 384, 1, 1024, "random", "matrix_os_kernel<40,"),
    (640, 384, 1, 1024, "parity", "matrix_os_kernel<40,"),
    # the NTT decode and the erasure solve
    (257, 255, 0, 300, "random", "ntt_lds_kernel"),
    (600, 1400, 0, 256, "random", "ntt_lds_kernel"),
    (450, 62, 0, 1024, "random", "ntt_eras_kernel"),
    (1000, 24, 0, 264, "random", "ntt_eras_kernel"),
])
def test_decode_extremes_vs_oracle(k, m, sys_, P, ids_kind, fam):
    """The received symbols at the extremes, inside valid use: stripe 0's
    received rows are crafted against the decode matrix of the ids (every
    8th column with marks at its largest coefficients), its data is what
    they decode to (craft_received).  The device encode of that data must
    reproduce the crafted symbols and marks on the kept columns; both decode
    layouts must return the data, as the oracle does.  Stripe 1: the pattern
    planes through the same ids."""
    import quadiron_amd as qa
    plan = qa.Plan(k, m, sys_)
    _routes(plan, P, "decode", fam)
    rng = np.random.default_rng(77 * k + m + P)
    ids = _ids_for(ids_kind, rng, k, m)
    d, r, kept, _, _, _ = craft_received(k, m, sys_, ids, P, rng)
    share = 1 - kept.mean()
    print(f"replaced {100 * share:.1f} % of {P} columns")
    assert share <= 0.05
    b = _Batch(plan, k, m, sys_, np.stack([d, pattern_rows(k, P)]))
    b.check_encode()
    # the received rows of stripe 0 are the crafted ones, marks included
    cols = np.flatnonzero(kept)
    full = np.concatenate([d, b.out_h[0]]) if sys_ else b.out_h[0]
    assert (full[ids][:, cols] == (r[:, cols] & 0xFFFF)).all()
    n_marks = 0
    for pos, fid in enumerate(ids):
        want = cols[r[pos, cols] == 65536]
        if sys_ and fid < k:
            assert len(want) == 0
            continue
        got = b.marks(0, fid - (k if sys_ else 0))
        assert np.array_equal(got[kept[got]], want), (pos, fid)
        n_marks += len(want)
    assert n_marks > 0
    b.check_decode(np.stack([ids, ids]))


# Fused repair and verify.  Their kernels are instantiations of their own
# (the _both epilogue records output marks, the _verify one compares with the
# stored row), their matrix is the R x k Lagrange matrix repair_ctx_kernel
# builds and packs on the device, and a repair at 128 < k <= 256 is all that
# reaches the KS = 16 geometry with one row block per wave.  {} is _both or
# _verify.
_OS16 = "matrix_os_kernel{}<16, 8, 1, false>"
REPAIR_CASES = [
    # the matrix cores, one whole 1024-column tile, the largest k of each
    # K-step; at k = 256 also 15 dead rows (R = 1) and a second row block
    # with one live row (R = 17)
    (16, 48, 0, 1024, 48, "matrix_mfma_kernel{}<1,"),
    (32, 32, 0, 1024, 32, "matrix_mfma_kernel{}<2,"),
    (64, 960, 0, 1024, 64, "matrix_os_kernel{}<4, 4, 1, false>"),
    (128, 128, 0, 1024, 64, "matrix_os_kernel{}<8, 8, 1, false>"),
    (256, 768, 0, 1024, 64, _OS16),
    (256, 768, 0, 1024, 1, _OS16),
    (256, 768, 0, 1024, 17, _OS16),
    # systematic: data and parity rows among the targets and among the ids
    # (two source regions)
    (16, 48, 1, 1024, 48, "matrix_mfma_kernel{}<1,"),
    (100, 50, 1, 1024, 50, "matrix_os_kernel{}<8, 8, 1, true>"),
    (200, 56, 1, 1024, 56, "matrix_os_kernel{}<16, 8, 1, true>"),
    # the dot2 kernel (a ragged width below one tile)
    (16, 48, 0, 300, 48, "matrix_kernel{}<8,"),
    (128, 128, 0, 300, 64, "matrix_kernel{}<64,"),
    (256, 768, 0, 300, 64, "matrix_kernel{}<128,"),
    (200, 56, 1, 300, 56, "matrix_kernel{}<128,"),
]


def _crafted_stripes(k, m, sys_, P, R, dense=0):
    """The inputs of a repair / verify case, checked before any launch.
    Stripe 0's data is what received symbols crafted against the repair
    matrix decode to (qi_testlib crafted_repair: the accumulator extremes of
    its rows, input marks at the largest coefficients, and columns one term
    off the extreme whose target is exactly 65536), stripe 1's pattern_rows;
    the coded rows and buckets are the oracle's encode of that data.  On the
    kept columns the oracle's received rows and marks are the crafted ones,
    and its target rows hold the crafted output marks.
    Returns (crafted, data (S, k, P), oracle encode per stripe)."""
    c = crafted_repair(k, m, sys_, R, P, dense)
    print(f"replaced {100 * c.share:.1f} % of {P} columns")
    assert c.share <= 0.05
    data = np.stack([c.d, pattern_rows(k, P)])
    enc = _encode_oracle(k, m, sys_, data)
    outs, oor, cnt = enc[0]
    cols = np.flatnonzero(c.kept)
    full = np.concatenate([c.d, outs]) if sys_ else outs
    assert (full[c.ids][:, cols] == (c.r[:, cols] & 0xFFFF)).all()

    def marks(fid):   # the oracle's, on the kept columns
        sl = _slot(k, sys_, int(fid))
        got = np.zeros(0, np.int64) if sl is None else oor[sl, :cnt[sl]].astype(np.int64)
        return got[c.kept[got]]
    n_in = n_out = 0
    for pos, fid in enumerate(c.ids):
        want = cols[c.r[pos, cols] == 65536]
        assert np.array_equal(marks(fid), want), (pos, fid)
        n_in += len(want)
    for j, t in enumerate(c.targets):
        want = cols[c.y[j, cols] == 65536]
        assert np.array_equal(marks(t), want), (j, t)
        n_out += int((c.solved[want] >= 0).sum())
    assert n_in > 0 and n_out > 0, (n_in, n_out)
    return c, data, enc


def _both_stripes(a):
    return np.ascontiguousarray(np.stack([a, a]), np.uint16)


@pytest.mark.parametrize("k,m,sys_,P,R,fam", REPAIR_CASES)
def test_repair_extremes_vs_oracle(k, m, sys_, P, R, fam):
    """Every rebuilt row, count and sorted mark list of both stripes equals
    the oracle's output for that target (a data target: the data row, no
    marks), over the whole block, from a context buffer that held garbage."""
    import quadiron_amd as qa
    plan = qa.Plan(k, m, sys_)
    names = plan.repair_kernels(R, P)
    print(f"\n{(k, m, sys_, P, R)}: {names}")
    assert fam.format("_both") in names, (fam, names)
    c, data, enc = _crafted_stripes(k, m, sys_, P, R)
    _repair_and_check(plan, k, m, sys_, data, enc, _both_stripes(c.ids),
                      _both_stripes(c.targets))
    assert plan.take_error() == 0


@pytest.mark.parametrize("k,m,sys_,P,R,fam", REPAIR_CASES)
def test_verify_extremes(k, m, sys_, P, R, fam):
    """The same stored rows, checked: clean, no (stripe, check) reports a
    mismatch -- a spurious one at a crafted column is what an accumulator
    error would produce.  Then every check row that has a crafted column
    without a mark has one bit of its stored word flipped there, and one row
    loses one stored output mark: one value mismatch per flipped row with
    `first` at its column, one mark mismatch for the row that lost its mark
    (`first` the smaller of its two columns), and nothing anywhere else."""
    import quadiron_amd as qa
    plan = qa.Plan(k, m, sys_)
    names = plan.verify_kernels(R, P)
    print(f"\n{(k, m, sys_, P, R)}: {names}")
    assert fam.format("_verify") in names, (fam, names)
    c, data, _ = _crafted_stripes(k, m, sys_, P, R)
    st = Stripes(k, m, sys_, data)
    basis, checks = _both_stripes(c.ids), _both_stripes(c.targets)
    evm, emm, efirst = _verify_check(plan, st, basis, checks)
    assert not evm.any() and not emm.any() and (efirst == NONE).all()
    cols = np.flatnonzero(c.kept)
    plain = [j for j in cols if c.solved[j] < 0 and (c.r[:, j] < 65536).all()]
    want_vm, want_mm = np.zeros((S, R), int), np.zeros((S, R), int)
    want_first = np.full((S, R), NONE)
    for t in sorted({t for t, _, _ in c.meta}):
        j = next((j for j in plain if c.meta[j][0] == t and c.y[t, j] < 65536), None)
        if j is not None:
            st.stored_row(0, int(c.targets[t]))[j] ^= 1 << (j % 16)
            want_vm[0, t], want_first[0, t] = 1, j
    assert want_vm.any()
    j = next(j for j in cols if c.solved[j] >= 0)
    t = c.meta[j][0]
    assert j in st.stored_marks(0, int(c.targets[t]))
    st.stored_marks(0, int(c.targets[t])).discard(j)
    want_mm[0, t], want_first[0, t] = 1, min(j, want_first[0, t])
    evm, emm, efirst = _verify_check(plan, st, basis, checks)
    assert (evm == want_vm).all() and (emm == want_mm).all() and (efirst == want_first).all()


@pytest.mark.parametrize("unaligned", [False, True])
def test_repair_verify_extremes_slow_tile(unaligned):
    """The slow-tile forms: the first 320 columns of stripe 0 are crafted
    columns that each carry one more received 65536 (besides the marks at the
    largest coefficients), so the first 256 columns hold more than 256 input
    marks, and every 8th of them is one whose target is 65536.  Whole tiles
    on aligned rows: the matrix-core kernel redoes its own tile; rows off the
    4-word boundary: the dot2 kernel and matrix_redo_kernel_both / _verify
    (the plan names the aligned route only; its dot2 forms are read off a
    ragged width).  The repair equals the oracle's -- each output mark
    recorded exactly once -- and the clean verify reports nothing."""
    import quadiron_amd as qa
    k, m, P, R = 16, 48, 1024, 48
    plan = qa.Plan(k, m, False)
    for names, sfx in ((plan.repair_kernels(R, P), "_both"),
                       (plan.verify_kernels(R, P), "_verify")):
        print(f"\n{(k, m, 0, P, R)}: {names}")
        assert f"matrix_mfma_kernel{sfx}<1," in names
    for names, sfx in ((plan.repair_kernels(R, P - 1), "_both"),
                       (plan.verify_kernels(R, P - 1), "_verify")):
        assert f"matrix_kernel{sfx}<8," in names and f"matrix_redo_kernel{sfx}" in names, names
    c, data, enc = _crafted_stripes(k, m, 0, P, R, dense=320)
    _, oor, cnt = enc[0]
    in_tile = sum(int((oor[f, :cnt[f]] < 256).sum()) for f in c.ids)
    out_tile = sum(int((oor[t, :cnt[t]] < 320).sum()) for t in c.targets)
    print(f"{in_tile} input marks in the first 256 columns, {out_tile} output marks in 320")
    assert in_tile > 256 and out_tile >= 320 // 8
    basis, checks = _both_stripes(c.ids), _both_stripes(c.targets)
    _repair_and_check(plan, k, m, 0, data, enc, basis, checks, unaligned)
    assert plan.take_error() == 0
    evm, emm, efirst = _verify_check(plan, Stripes(k, m, 0, data), basis, checks, unaligned)
    assert not evm.any() and not emm.any() and (efirst == NONE).all()
