"""The kernels at their accumulator extremes, bit-exact against the oracle.

The kernels' correctness rests on range arguments (the dot2 accumulator
below 2^31, the matrix cores' 256 D2 + D1 - D0 with D2 folded first from
KS = 16 up and carried over two K chunks at KS = 40, the NTT engine's lazy
24-bit multiplies) that uniform random symbols never come near: their sums
are a random walk.  These tests feed columns crafted from the codes' own
matrices (qi_testlib craft_columns; tests/test_extreme_inputs.py shows on
the CPU that they reach what they claim) and the 0x00 / 0xFF / 0x80 / 0x7F
planes stored files are full of.  Each case names the kernel family it is
there for and asserts that the plan routes to it.  Run with -m gpu."""
import functools

import numpy as np
import pytest

from qi_testlib import (ALL_MODES, craft_columns, craft_received, extreme_targets,
                        generator_matrix, oracle_decode_blocks, oracle_encode_blocks,
                        pattern_rows)

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
    d, r, kept, _, _ = craft_received(k, m, sys_, ids, P, rng)
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
