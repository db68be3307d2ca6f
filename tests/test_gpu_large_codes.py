"""GPU: the largest codes the plan accepts -- n up to 65536, k up to 32768,
fragment ids past 32767 -- against the oracle and the original data.

The rest of the suite stops at k = 2000 and n = 16384, so no id of 32768 or
more (ids travel as uint16 viewed as int16 on the torch side), no 32768- or
65536-point transform (the multi-pass engine's 32.32.32 plan and its only
four-pass plan, 16.16.16.16) and no context of more than 14336 points (where
ntt_ctx_kernel's static LDS first pushes the launch past 64 KiB) had run.

Every round-trip case encodes S = 2 stripes and compares outputs and sorted
mark lists with the oracle: the whole width where n P <= 2^22 symbols per
stripe, else the column windows [0, 24) and [240, 264), both sides of the
256-column block seam.  It decodes through both layouts from contexts that
held garbage; every decode is compared with the original data over the whole
block, and with the oracle's own decode where k <= 5000 (its context is
O(k^2)).  Stripe 0 receives a sorted subset forced to hold ids 0, 32767,
32768 and k + m - 1 (where the code has them) and, where m >= k, a majority
of ids >= 32768; stripe 1 a plain seeded subset, and its data ends in 40
columns of pattern_rows.  Marks are crafted into the windows on received
rows, so the compared windows hold output marks and the decodes read input
marks.  The oracle is called once per case for the crafting and once for the
windows of both stripes (the codes are column-independent), which keeps a
case near a second.  Each case names the kernels it is there for.

The fused repair and verify cases rebuild and check fragments with ids
>= 32768 from received ids >= 32768.  Their reference is the code's own
definition in exact integer arithmetic (_rows_matrix: the Vandermonde rows
r^(f j), systematic: the Lagrange rows through the points r^0 .. r^(k-1)),
pinned to the oracle on two columns of each case; the oracle's block encode
of 65536 rows by 1024 columns would take seconds.  Run with -m gpu."""
import functools

import numpy as np
import pytest

import test_gpu_repair
from qi_testlib import (Q, matvec_mod, oracle_decode_blocks, oracle_encode_blocks,
                        pattern_rows)
from test_gpu_repair import _repair_and_check, _slot
from test_gpu_verify import NONE, WCAP, Stripes, _expect, _run

pytestmark = pytest.mark.gpu

S = 2
CAP = 64   # marks per row: a handful crafted, about n P / 65537 by chance, and at
           # most one per pattern column (a constant column can mark a whole row)
PATTERN_COLS = 40

NTT_ENC = "ntt_pass_kernel"
NTT_DEC = "ntt_ctx_kernel + ntt_expand_kernel + ntt_fix_kernel + ntt_pass_kernel"


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _ids(rng, k, m, s):
    """Stripe s's received ids, ascending (module docstring)."""
    n = k + m
    if s == 1:
        return np.sort(rng.choice(n, k, replace=False))
    forced = np.array(sorted({i for i in (0, 32767, 32768, n - 1) if i < n})[:k])
    pool = np.setdiff1d(np.arange(n), forced)
    rest = k - len(forced)
    hi, lo = pool[pool >= 32768], pool[pool < 32768]
    if m >= k and len(hi):
        n_hi = min(len(hi), rest - rest // 4)
        sel = np.concatenate([rng.choice(hi, n_hi, replace=False),
                              rng.choice(lo, rest - n_hi, replace=False)])
    else:
        sel = rng.choice(pool, rest, replace=False)
    ids = np.sort(np.concatenate([forced, sel]))
    assert len(np.unique(ids)) == k and set(forced) <= set(ids)
    if m >= k and len(hi):
        assert (ids >= 32768).sum() > k // 2
    return ids


def _windows(n, P):
    return [(0, P)] if n * P <= 1 << 22 else [(0, 24), (240, 264)]


def _slots(k, sys_, ids):
    """coded-row slots (oracle output indices) of the received coded rows"""
    ids = np.asarray(ids, np.int64)
    return ids[ids >= k] - k if sys_ else ids


def _lanes_bytes(a):
    return np.ascontiguousarray(a, np.uint16).view(np.uint8).reshape(a.shape[0], -1)


def _oracle_values(k, m, sys_, lanes):
    """The oracle's encode of the (k, W) u16 columns: (outs (no, W) u16,
    marks as (row, column) pairs in row-major order, cnt)."""
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, _lanes_bytes(lanes), lanes.shape[1])
    mask = np.arange(oor.shape[1])[None, :] < cnt[:, None]
    return outs.view(np.uint16), np.nonzero(mask)[0], oor[mask].astype(np.int64), cnt


def _craft(k, m, sys_, data, ids, wins, rng, per_win=3):
    """Solve data row 0 of per_win columns in the first 24 of every window of
    every stripe so that one received coded row is 65536 there: one oracle
    call on the unit column e0 and the chosen columns with row 0 zeroed."""
    picks = [(s, int(j)) for s in range(S) for lo, hi in wins
             for j in lo + rng.choice(min(hi - lo, 24), per_win, replace=False)]
    blk = np.zeros((k, 1 + len(picks)), np.uint16)
    blk[0, 0] = 1
    for t, (s, j) in enumerate(picks):
        blk[:, 1 + t] = data[s, :, j]
        blk[0, 1 + t] = 0
    outs, rows, cols, _ = _oracle_values(k, m, sys_, blk)
    v = outs.astype(np.int64)
    v[rows, cols] = 65536
    a = v[:, 0]
    for t, (s, j) in enumerate(picks):
        cand = _slots(k, sys_, ids[s])
        i = int(rng.choice(cand[a[cand] != 0]))
        d0 = (65536 - int(v[i, 1 + t])) % Q * pow(int(a[i]), Q - 2, Q) % Q
        if d0 < 65536:
            data[s, 0, j] = d0


def _roundtrip(k, m, sys_, P, enc_fam, dec_fam, seed):
    torch = _torch()
    import quadiron_amd as qa
    rng = np.random.default_rng(seed)
    plan = qa.Plan(k, m, sys_)
    names = plan.kernels(P)
    print(f"\n{(k, m, sys_, P)}: {names}")
    enc_names, dec_names = names[len("encode="):].split("; decode=")
    assert enc_fam in enc_names and dec_fam in dec_names, names
    no, n = plan.n_outputs, 1 << (k + m - 1).bit_length()
    wins = _windows(n, P)
    wcols = np.concatenate([np.arange(lo, hi) for lo, hi in wins])
    Wc = len(wcols)
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    data[1, :, P - PATTERN_COLS:] = pattern_rows(k, PATTERN_COLS)
    ids = np.stack([_ids(rng, k, m, s) for s in range(S)]).astype(np.uint16)
    _craft(k, m, sys_, data, ids, wins, rng)
    dd = torch.from_numpy(data.view(np.int16)).cuda()
    out = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * no * CAP, dtype=torch.int32, device="cuda")
    plan.encode(dd, out, counts, entries, CAP)
    torch.cuda.synchronize()
    assert plan.take_error() == 0
    wsel = torch.from_numpy(wcols).cuda()
    out_w = out.index_select(2, wsel).cpu().numpy().view(np.uint16)
    cnt_h = counts.cpu().numpy().view(np.uint32).reshape(S, no)
    ent_h = entries.cpu().numpy().view(np.uint32).reshape(S, no, CAP)
    assert (cnt_h <= CAP).all()

    di = torch.from_numpy(ids.view(np.int16)).cuda()
    ctx = torch.randint(0, 256, (plan.ctx_bytes(S, P),), dtype=torch.uint8, device="cuda")
    plan.decode_ctx(di, ctx, P, counts, entries, CAP, h_ids=ids)
    dec = torch.zeros((S, k, P), dtype=torch.int16, device="cuda")
    assert plan.decode(ctx, di, out, dec, data=dd, counts=counts, entries=entries,
                       cap=CAP) == 0
    torch.cuda.synchronize()
    assert plan.take_error() == 0
    bad = (dec != dd).nonzero()
    assert len(bad) == 0, ("decode", len(bad), bad[:4].tolist())
    dec_w = dec.index_select(2, wsel).cpu().numpy().view(np.uint16)
    # the packed layout: received rows back to back, buckets by position
    idx = torch.from_numpy(ids.astype(np.int64)).cuda()
    cnt2, ent3 = counts.view(S, no), entries.view(S, no, CAP)
    if sys_:
        full = torch.cat([dd, out], dim=1)
        fcnt = torch.cat([torch.zeros((S, k), dtype=torch.int32, device="cuda"), cnt2], dim=1)
        fent = torch.cat([torch.zeros((S, k, CAP), dtype=torch.int32, device="cuda"), ent3],
                         dim=1)
    else:
        full, fcnt, fent = out, cnt2, ent3
    recv = torch.gather(full, 1, idx[:, :, None].expand(S, k, P)).contiguous()
    pcnt = torch.gather(fcnt, 1, idx).contiguous()
    pent = torch.gather(fent, 1, idx[:, :, None].expand(S, k, CAP)).contiguous()
    del full, fent
    ctx2 = torch.full_like(ctx, 0xA5)
    plan.decode_ctx_packed(di, ctx2, P, pcnt, pent, CAP, h_ids=ids)
    dec2 = torch.zeros_like(dec)
    assert plan.decode_packed(ctx2, recv, dec2, pcnt, pent, CAP) == 0
    torch.cuda.synchronize()
    assert plan.take_error() == 0
    bad = (dec2 != dd).nonzero()
    assert len(bad) == 0, ("decode_packed", len(bad), bad[:4].tolist())

    # the oracle on the window columns of both stripes, side by side
    o_out, o_rows, o_cols, _ = _oracle_values(
        k, m, sys_, np.concatenate([data[s][:, wcols] for s in range(S)], axis=1))
    for s in range(S):
        o_s = o_out[:, s * Wc:(s + 1) * Wc]
        bad = np.argwhere(out_w[s] != o_s)
        assert len(bad) == 0, ("encode", s, len(bad), bad[:4].tolist())
        here = o_cols // Wc == s
        want = sorted(zip(o_rows[here].tolist(), wcols[o_cols[here] % Wc].tolist()))
        mask = np.arange(CAP)[None, :] < cnt_h[s][:, None]
        g_rows, g_cols = np.nonzero(mask)[0], ent_h[s][mask].astype(np.int64)
        in_win = np.isin(g_cols, wcols)
        got = sorted(zip(g_rows[in_win].tolist(), g_cols[in_win].tolist()))
        assert got == want, ("marks", s, len(got), len(want))
        if Wc == P:   # the whole width: the counts themselves
            assert (cnt_h[s] == np.bincount(o_rows[here], minlength=no)).all(), s
        if k <= 5000:   # the oracle's own decode of its own encode
            o_cnt = np.bincount(o_rows[here], minlength=no).astype(np.uint32)
            o_oor = np.zeros((no, max(1, int(o_cnt.max()))), np.uint32)
            fill = np.zeros(no, np.int64)
            for i, c in zip(o_rows[here].tolist(), (o_cols[here] % Wc).tolist()):
                o_oor[i, fill[i]] = c
                fill[i] += 1
            missing = np.ones(k + m, np.int32)
            missing[ids[s].astype(np.int64)] = 0
            d_w = _lanes_bytes(data[s][:, wcols])
            ok, o_dec = oracle_decode_blocks(k, m, sys_, _lanes_bytes(o_s), o_oor, o_cnt,
                                             missing, d_w)
            assert ok == 1 and (o_dec == d_w).all(), s
            assert (_lanes_bytes(dec_w[s]) == o_dec).all(), s
        n_in = int(cnt_h[s][_slots(k, sys_, ids[s])].sum())
        print(f"stripe {s}: {len(g_cols)} output marks, {len(got)} in the windows, "
              f"{n_in} on received rows; largest id {int(ids[s].max())}")
        assert len(got) > 0 and n_in > 0
    return plan


@pytest.mark.parametrize("k,m,sys_", [
    (260, 32508, 0),     # NTT_n = 32768 (32.32.32), small len_2k
    (260, 65276, 0),     # NTT_n = 65536 (the four-pass plan), ids to 65535
    (260, 65276, 1),     # the same through interpolation + NTT_n, rows k ...
    (5000, 3000, 0),     # len_2k = 16384 > n = 8192
    (14336, 2048, 0),    # len_2k = 32768; context LDS exactly 64 KiB (57344 + 8192)
    (14337, 2047, 0),    # first k whose context launch needs the static LDS counted
    (16384, 16384, 0),   # last k of that range; n = len_2k = 32768
    (16385, 16383, 1),   # first k whose dynamic LDS alone opts in; d_sysctx at creation
    (32768, 32768, 0),   # largest k: n = len_2k = 65536, 136 KiB of context LDS
])
def test_ntt_engine_large(k, m, sys_):
    _roundtrip(k, m, sys_, 264, NTT_ENC, NTT_DEC, seed=[k, m, sys_])


@pytest.mark.parametrize("k", [14337, 16384])
def test_systematic_plan_in_the_static_lds_range(k):
    """ntt_plan_init builds the systematic encode's context with
    ntt_ctx_kernel: for 14336 < k <= 16384 the plan itself could not be
    created while the launch ignored the kernel's static LDS."""
    _torch()
    import quadiron_amd as qa
    plan = qa.Plan(k, 32768 - k, True)
    assert NTT_DEC in plan.kernels(264)
    assert plan.take_error() == 0


@pytest.mark.parametrize("k,m,sys_,P,enc_fam,dec_fam", [
    # the register codelet with 4096 twisted passes; dot2 and KS = 1 decodes
    (16, 65520, 0, 300, "encode_fnt_kernel<16,", "matrix_kernel<8,"),
    (16, 65520, 0, 1024, "encode_fnt_kernel<16,", "matrix_mfma_kernel<1,"),
    # a 65536-row generator on the matrix cores
    (64, 65472, 0, 1024, "gen_mfma_kernel", "matrix_os_kernel<4,"),
    # a 65336 x 200 systematic generator; two-region decode, parity ids >= 32768
    (200, 65336, 1, 1024, "matrix_os_kernel<16, 8, 2, false>",
     "decode_ctx_kernel<1024, true> + matrix_os_kernel<16, 8, 2, true>"),
])
def test_matrix_paths_n65536(k, m, sys_, P, enc_fam, dec_fam):
    _roundtrip(k, m, sys_, P, enc_fam, dec_fam, seed=[k, m, sys_, P])


# ---------------------------------------------------------------------------
# fused repair and verify with ids and targets >= 32768

FCAP = 32   # bucket capacity of these cases (the helpers' own is sized for
            # dense tiles; 65536 rows of it would be a GiB of empty buckets)


def _powm(b, e):
    """b ** e mod q elementwise (b int64 array in [0, q), e a Python int)."""
    r = np.ones_like(b)
    while e:
        if e & 1:
            r = r * b % Q
        b = b * b % Q
        e >>= 1
    return r


def _rows_matrix(k, m, sys_, fids):
    """(len(fids), k) int64: fragment f of a column as a combination of its k
    data symbols, from the definition.  Non-systematic: c_f = sum_j d_j
    r^(f j), r the n-th root 3^(65536 / n).  Systematic: c_f = D(r^f) for the
    D of degree < k with D(r^j) = d_j, j < k, in Lagrange form."""
    n = 1 << (k + m - 1).bit_length()
    r = pow(3, 65536 // n, Q)
    f = np.asarray(fids, np.int64)
    j = np.arange(k, dtype=np.int64)
    if not sys_:
        pw = np.ones(n, np.int64)   # r^e, e < n
        for e in range(1, n):
            pw[e] = pw[e - 1] * r % Q
        return pw[f[:, None] * j[None, :] % n]
    x = np.array([pow(r, int(t), Q) for t in range(k)], np.int64)
    w = np.ones(k, np.int64)   # prod_{l != j} (x_j - x_l)
    for l in range(k):
        w = w * np.where(j == l, 1, (x - x[l]) % Q) % Q
    winv = _powm(w, Q - 2)
    M = np.zeros((len(f), k), np.int64)
    for t, fid in enumerate(f.tolist()):
        if fid < k:
            M[t, fid] = 1
            continue
        d = (pow(r, fid, Q) - x) % Q          # x_f - x_l, none zero
        full = 1
        for v in d.tolist():
            full = full * v % Q
        M[t] = full * _powm(d, Q - 2) % Q * winv % Q
    return M


class _SparseStripes(Stripes):
    """test_gpu_verify.Stripes holding only the fragments a case touches."""

    def __init__(self, k, m, sys_, data, enc, true):
        self.k, self.m, self.sys = k, m, sys_
        self.S, _, self.P = data.shape
        self.data = data
        self.coded = np.stack([e[0] for e in enc])
        self.no = self.coded.shape[1]
        self.true = true   # {(stripe, fragment id): symbols in [0, 65536]}
        self.st_data = data.copy()
        self.st_coded = self.coded.copy()
        self.marks = [[set() for _ in range(self.no)] for _ in range(self.S)]
        for s, e in enumerate(enc):
            for sl in np.flatnonzero(e[2]):
                self.marks[s][sl] = set(int(c) for c in e[1][sl, :e[2][sl]])


@functools.lru_cache(maxsize=None)
def _fused_case(k, m, sys_, R, P):
    """Data, received ids, targets and the exact coded rows of a repair of R
    fragments at n = 65536, shared by the repair and the verify case
    (read-only).  Targets: ids 65535 and 32768, systematic: four data rows,
    the rest above 32768.  Received: ids 0 and 32767 (systematic: k / 2 data
    rows) and ids >= 32768.  Every stripe has a crafted 65536 on a received
    coded row and on a target row."""
    n = k + m
    assert n == 65536
    rng = np.random.default_rng([k, m, sys_, R, P])
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    ids, tgs, enc, true = [], [], [], {}
    no = m if sys_ else n
    for s in range(S):
        tg = [n - 1, 32768] + (rng.choice(k, 4, replace=False).tolist() if sys_ else [])
        tg += rng.choice(np.arange(32769, n - 1), R - len(tg), replace=False).tolist()
        tg = rng.permutation(tg)
        pool = np.setdiff1d(np.arange(n), tg)
        hi = pool[pool >= 32768]
        if sys_:
            sel = np.concatenate([rng.choice(pool[pool < k], k // 2, replace=False),
                                  rng.choice(hi, k - k // 2, replace=False)])
        else:
            sel = np.concatenate([[0, 32767], rng.choice(hi, k - 2, replace=False)])
        sel = np.sort(sel)
        assert len(np.unique(np.concatenate([sel, tg]))) == k + R
        fids = np.concatenate([sel, tg])
        M = _rows_matrix(k, m, sys_, fids)
        # one mark on a received coded row, one on a coded target row
        coded_recv = [t for t in range(k) if sel[t] >= (k if sys_ else 0)]
        coded_tg = [k + t for t in range(R) if tg[t] >= (k if sys_ else 0)]
        for rows, lo in ((coded_recv, 0), (coded_tg, P // 2)):
            for j in range(lo, lo + 8):
                t = int(rng.choice(rows))
                col = data[s, :, j].astype(np.int64)
                col[0] = 0
                if M[t, 0] == 0:
                    continue
                d0 = (65536 - int(M[t] @ col % Q)) % Q * pow(int(M[t, 0]), Q - 2, Q) % Q
                if d0 < 65536:
                    data[s, 0, j] = d0
                    break
            else:
                raise AssertionError("no column could be crafted")
        vals = matvec_mod(M, data[s].astype(np.int64))
        coded = np.zeros((no, P), np.uint16)
        oor = np.zeros((no, FCAP), np.uint32)
        cnt = np.zeros(no, np.uint32)
        for t, fid in enumerate(fids.tolist()):
            true[s, fid] = vals[t]
            sl = _slot(k, sys_, fid)
            if sl is None:
                assert (vals[t] == data[s, fid]).all()
                continue
            coded[sl] = vals[t] & 0xffff
            mk = np.flatnonzero(vals[t] == 65536)
            assert len(mk) <= FCAP
            oor[sl, :len(mk)], cnt[sl] = mk, len(mk)
        assert cnt[[_slot(k, sys_, int(sel[t])) for t in coded_recv]].sum() > 0
        assert cnt[[_slot(k, sys_, int(f)) for f in tg if f >= (k if sys_ else 0)]].sum() > 0
        # the definition above is the oracle's: two whole columns, a crafted one among them
        o_out, o_rows, o_cols, _ = _oracle_values(k, m, sys_, data[s][:, [0, P - 1]])
        o = o_out.astype(np.int64)
        o[o_rows, o_cols] = 65536
        for t, fid in enumerate(fids.tolist()):
            sl = _slot(k, sys_, fid)
            if sl is not None:
                assert (o[sl] == vals[t][[0, P - 1]]).all(), (s, fid)
        ids.append(sel)
        tgs.append(tg)
        enc.append((coded, oor, cnt))
    ids = np.stack(ids).astype(np.uint16)
    tgs = np.stack(tgs).astype(np.uint16)
    for a in (data, ids, tgs):
        a.setflags(write=False)
    return data, ids, tgs, enc, true


FUSED = [
    (16, 65520, 0, 48, "matrix_mfma_kernel{}<1,"),
    (200, 65336, 1, 56, "matrix_os_kernel{}<16,"),
]


@pytest.mark.parametrize("k,m,sys_,R,fam", FUSED)
def test_repair_large_ids(k, m, sys_, R, fam, monkeypatch):
    """Every rebuilt row, count and sorted mark list against the exact rows,
    with targets and received ids >= 32768 (id 65535 among the targets)."""
    _torch()
    import quadiron_amd as qa
    P = 1024
    monkeypatch.setattr(test_gpu_repair, "CAP", FCAP)
    plan = qa.Plan(k, m, sys_)
    names = plan.repair_kernels(R, P)
    print(f"\n{(k, m, sys_, P, R)}: {names}")
    assert fam.format("_both") in names, names
    data, ids, tgs, enc, _ = _fused_case(k, m, sys_, R, P)
    assert int(tgs.max()) == 65535 and (ids >= 32768).any()
    _repair_and_check(plan, k, m, sys_, data.copy(), enc, ids.copy(), tgs.copy(),
                      min_out_marks=[1] * S)
    assert plan.take_error() == 0


def _verify_check(plan, st, basis, checks):
    """test_gpu_verify._check at the bucket capacity FCAP."""
    evm, emm, efirst, _ = _expect(st, basis, checks)
    vm, mm, first, err = _run(plan, st, basis, checks, wcap=WCAP, cap=FCAP)
    print("value mismatches", int(vm.sum()), "mark mismatches", int(mm.sum()),
          "first", sorted(set(first.ravel().tolist()) - {NONE}))
    assert err == 0
    assert (vm == evm).all() and (mm == emm).all() and (first == efirst).all()
    return evm, emm, efirst


@pytest.mark.parametrize("k,m,sys_,R,fam", FUSED)
def test_verify_large_ids(k, m, sys_, R, fam):
    """The same stored rows, checked: clean, nothing is reported; after one
    flipped bit in the stored row of fragment 65535 of stripe 0, exactly that
    (stripe, check) reports one value mismatch, `first` at its column."""
    _torch()
    import quadiron_amd as qa
    P = 1024
    plan = qa.Plan(k, m, sys_)
    names = plan.verify_kernels(R, P)
    print(f"\n{(k, m, sys_, P, R)}: {names}")
    assert fam.format("_verify") in names, names
    data, ids, tgs, enc, true = _fused_case(k, m, sys_, R, P)
    st = _SparseStripes(k, m, sys_, data, enc, true)
    evm, emm, efirst = _verify_check(plan, st, ids, tgs)
    assert not evm.any() and not emm.any() and (efirst == NONE).all()
    j = int(np.flatnonzero(tgs[0] == 65535)[0])
    col = next(c for c in range(700, P) if true[0, 65535][c] != 65536)
    st.stored_row(0, 65535)[col] ^= 0x0100
    evm, emm, efirst = _verify_check(plan, st, ids, tgs)
    want = np.zeros((S, R), int)
    want[0, j] = 1
    assert (evm == want).all() and not emm.any()
    assert efirst[0, j] == col and (np.delete(efirst.ravel(), j) == NONE).all()
