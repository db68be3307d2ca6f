"""GPU: delta update (qi_gpu_update_ctx / qi_gpu_update, Fec.update_blocks)
against the CPU oracle.  The coded rows and in-buckets given to the update
are the oracle's encode of the old data; the result must equal the oracle's
encode of the new data symbol for symbol, with the oracle's OOR lists (as
sets, counts exact).  Nothing expected here comes from the product."""
import subprocess

import numpy as np
import pytest

from qi_testlib import (FILL, backing_is_fill, craft_oor_columns, oracle_encode_blocks,
                        pattern_rows, retry_block, strided_rows, wide_rs)

pytestmark = pytest.mark.gpu

CAP = 2048
TILE = 2048          # the update kernel's column tile
SENTINEL = 7         # count of an out-bucket the update must not touch


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    torch.cuda.set_device(0)
    return torch


def _n_out(k, m, sys_):
    return m if sys_ else k + m


def _encode(k, m, sys_, data):
    """per stripe (rows u16 (no, P), oor (no, CAP), counts) from the oracle"""
    S, _, P = data.shape
    res = []
    for s in range(S):
        o, oor, cnt = oracle_encode_blocks(
            k, m, sys_, np.ascontiguousarray(data[s]).view(np.uint8).reshape(k, 2 * P), CAP)
        assert cnt.max() <= CAP
        res.append((o.view(np.uint16).reshape(-1, P), oor, cnt))
    return res


def _marks(enc_s, slot):
    return set(int(v) for v in enc_s[1][slot, :enc_s[2][slot]])


def _pick(k, m, sys_, U, R, S, rng, row0=False):
    """ids [S, U] and slots [S, R], differing per stripe; ids hold 0 and k - 1
    somewhere, slots 0 and n_outputs - 1"""
    no = _n_out(k, m, sys_)
    ids = np.stack([rng.permutation(k)[:U] for _ in range(S)])
    slots = np.stack([rng.permutation(no)[:R] for _ in range(S)])
    if row0:
        for s in range(S):
            if 0 not in ids[s]:
                ids[s, s % U] = 0
    else:
        if 0 not in ids[0]:
            ids[0, 0] = 0
        if k - 1 not in ids[S - 1]:
            ids[S - 1, U - 1] = k - 1
    if 0 not in slots[0]:
        slots[0, 0] = 0
    if no - 1 not in slots[S - 1]:
        slots[S - 1, R - 1] = no - 1
    return ids.astype(np.uint16), slots.astype(np.uint16)


def _datasets(k, P, ids, rng):
    S = ids.shape[0]
    old = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    new = old.copy()
    for s in range(S):
        new[s, ids[s]] = rng.integers(0, 65536, (len(ids[s]), P), dtype=np.uint16)
    return old, new


def _dev_rows(torch, arr, unaligned):
    """[S, rows, P] device view of arr inside a FILL-filled backing; unaligned:
    at an odd u16 offset with a row stride that is no multiple of 8"""
    S, rows, P = arr.shape
    pad = 0
    if unaligned:
        pad = 1 if (P + 1) % 8 else 3
    big = torch.full((S, rows, P + pad), FILL, dtype=torch.int16, device="cuda")
    view = big[:, :, pad:]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr).view(np.int16)))
    if unaligned:
        assert view.data_ptr() % 4 == 2 and view.stride(1) % 8 != 0
    return big, view, pad


def _buckets(torch, enc):
    cnt = np.stack([e[2] for e in enc]).astype(np.uint32)
    ent = np.stack([e[1] for e in enc]).astype(np.uint32)
    return (torch.from_numpy(cnt.view(np.int32).reshape(-1)).cuda(),
            torch.from_numpy(ent.view(np.int32).reshape(-1)).cuda())


def _run_and_check(k, m, sys_, ids, slots, old, new, inplace, unaligned, explicit_all=False,
                   null_in=False, null_out=False, enc_old=None, enc_new=None):
    """slots None: every slot (d_slots NULL), or an explicit permutation of
    them when explicit_all."""
    torch = _torch()
    import quadiron_amd as qa
    S, _, P = old.shape
    U = ids.shape[1]
    no = _n_out(k, m, sys_)
    enc_old = enc_old or _encode(k, m, sys_, old)
    enc_new = enc_new or _encode(k, m, sys_, new)
    if null_in:
        assert all(e[2].sum() == 0 for e in enc_old)
    plan = qa.Plan(k, m, bool(sys_))
    if slots is None and explicit_all:
        rng = np.random.default_rng(5)
        slots = np.stack([rng.permutation(no) for _ in range(S)]).astype(np.uint16)
    listed = slots if slots is not None else np.tile(np.arange(no), (S, 1))
    R = listed.shape[1]
    di = torch.from_numpy(ids.view(np.int16)).cuda()
    ds = torch.from_numpy(slots.view(np.int16)).cuda() if slots is not None else None
    nb = plan.update_ctx_bytes(U, R, S)
    UP = {1: 1, 2: 2, 3: 4, 4: 4}.get(U, 8)
    assert nb == S * 4 * (R * UP + R + UP)
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    plan.update_ctx(di, ds, ctx)
    obig, dold, opad = _dev_rows(torch, np.stack([old[s, ids[s]] for s in range(S)]), unaligned)
    nbig, dnew, _ = _dev_rows(torch, np.stack([new[s, ids[s]] for s in range(S)]), unaligned)
    coded_np = np.stack([e[0] for e in enc_old])
    cbig, coded, cpad = _dev_rows(torch, coded_np, unaligned)
    counts, entries = (None, None) if null_in else _buckets(torch, enc_old)
    if inplace:
        out, xbig = None, cbig
    else:
        xbig, out, _ = _dev_rows(torch, np.full((S, no, P), FILL, np.uint16), unaligned)
    oc = oe = None
    if not null_out:
        oc = torch.full((S * no,), SENTINEL, dtype=torch.int32, device="cuda")
        oe = torch.full((S * no * CAP,), -1, dtype=torch.int32, device="cuda")
        lin = (np.arange(S)[:, None] * no + listed).reshape(-1)
        oc[torch.from_numpy(lin.astype(np.int64)).cuda()] = 0   # the caller's clear
    err = plan.update(ctx, R, dold, dnew, coded, out, counts=counts, entries=entries,
                      cap=CAP if counts is not None else 0, out_counts=oc, out_entries=oe,
                      out_cap=CAP if oc is not None else 0)
    assert err == 0
    torch.cuda.synchronize()
    got = (coded if inplace else out).cpu().numpy().view(np.uint16)
    for big, pad in ((obig, opad), (nbig, opad), (cbig, cpad), (xbig, cpad)):
        if pad:
            assert (big[:, :, :pad].cpu().numpy().view(np.uint16) == FILL).all()
    # the inputs are read only
    assert (dold.cpu().numpy().view(np.uint16) ==
            np.stack([old[s, ids[s]] for s in range(S)])).all()
    assert (dnew.cpu().numpy().view(np.uint16) ==
            np.stack([new[s, ids[s]] for s in range(S)])).all()
    if not inplace:
        assert (coded.cpu().numpy().view(np.uint16) == coded_np).all()
    if counts is not None:
        assert (counts.cpu().numpy().view(np.uint32).reshape(S, no) ==
                np.stack([e[2] for e in enc_old])).all()
    gc = oc.cpu().numpy().view(np.uint32).reshape(S, no) if oc is not None else None
    ge = oe.cpu().numpy().view(np.uint32).reshape(S, no, CAP) if oe is not None else None
    for s in range(S):
        on = set(int(v) for v in listed[s])
        for j in range(no):
            if j in on:
                exp = enc_new[s][0][j]
                assert (got[s, j] == exp).all(), (s, j, np.flatnonzero(got[s, j] != exp)[:8])
                if gc is not None:
                    em = _marks(enc_new[s], j)
                    assert gc[s, j] == len(em), (s, j, gc[s, j], len(em))
                    assert set(int(v) for v in ge[s, j, :gc[s, j]]) == em, (s, j)
            else:
                keep = enc_old[s][0][j] if inplace else np.full(P, FILL, np.uint16)
                assert (got[s, j] == keep).all(), (s, j)
                if gc is not None:
                    assert gc[s, j] == SENTINEL and (ge[s, j] == 0xFFFFFFFF).all(), (s, j)
    assert plan.take_error() == 0


BASE = [
    # k, m, sys, U, R (None: all), P, S, inplace, unaligned, explicit_all
    (3, 3, 0, 3, None, 37, 2, True, False, False),
    (3, 3, 1, 3, 1, 1, 3, False, True, False),
    (3, 3, 1, 3, None, 1031, 2, True, False, True),
    (16, 48, 0, 1, 5, 1024, 3, True, False, False),
    (16, 48, 0, 8, None, 4099, 2, False, True, False),
    (16, 48, 1, 3, None, 1031, 3, True, True, False),
    (16, 48, 1, 8, 5, 1024, 2, False, False, False),
    (16, 48, 1, 1, 1, 4099, 2, True, False, False),
    (200, 56, 1, 8, None, 1031, 2, True, False, False),
    (200, 56, 1, 1, 5, 37, 2, False, False, False),
    (256, 768, 0, 3, None, 1024, 2, True, False, True),
    (256, 768, 0, 8, 5, 37, 2, False, True, False),
    (1000, 24, 1, 1, None, 1031, 2, True, False, False),
    (1000, 24, 1, 8, 5, 37, 2, False, False, False),
    (600, 1448, 0, 3, 5, 1024, 2, True, False, False),
    (600, 1448, 0, 1, None, 37, 2, False, False, False),
]


@pytest.mark.parametrize("k,m,sys_,U,R,P,S,inplace,unaligned,explicit_all", BASE)
def test_update_vs_oracle(hip_lib, k, m, sys_, U, R, P, S, inplace, unaligned, explicit_all):
    rng = np.random.default_rng([k, m, sys_, U, P])
    ids, slots = _pick(k, m, sys_, U, R or 1, S, rng)
    old, new = _datasets(k, P, ids, rng)
    _run_and_check(k, m, sys_, ids, slots if R else None, old, new, inplace, unaligned,
                   explicit_all)


def _crafted(k, m, sys_, U, P, S, slot, rin, rout, rboth, rng):
    """Old and new data with data row 0 among the updated rows and output
    `slot` crafted to 65536 in the column ranges rin (old only), rout (new
    only) and rboth (both)."""
    ids, _ = _pick(k, m, sys_, U, 1, S, rng, row0=True)
    old, new = _datasets(k, P, ids, rng)
    for s in range(S):
        for data, ranges in ((old[s], (rin, rboth)), (new[s], (rout, rboth))):
            for lo, hi in (r for r in ranges if r[1] > r[0]):
                craft_oor_columns(k, m, sys_, data, rng, hi - lo, rows=[slot], col_range=(lo, hi))
        assert (old[s, 1:] == new[s, 1:])[np.setdiff1d(np.arange(1, k), ids[s]) - 1].all()
    return ids, old, new


MARKS = [
    # k, m, sys, U, P, slot, inplace, null_in, null_out
    (16, 48, 0, 3, 1031, 9, True, False, False),
    (16, 48, 1, 1, 4099, 47, False, False, False),
    (200, 56, 1, 8, 1031, 0, True, False, False),
    (16, 48, 0, 1, 1031, 63, True, False, True),
]


@pytest.mark.parametrize("k,m,sys_,U,P,slot,inplace,null_in,null_out", MARKS)
def test_update_marks(hip_lib, k, m, sys_, U, P, slot, inplace, null_in, null_out):
    rng = np.random.default_rng([k, m, sys_, U, P, 77])
    S = 2
    rin, rout, rboth = (P - 60, P - 40), (P - 30, P - 2), (5, 15)
    ids, old, new = _crafted(k, m, sys_, U, P, S, slot, rin, rout, rboth, rng)
    enc_old, enc_new = _encode(k, m, sys_, old), _encode(k, m, sys_, new)
    for s in range(S):
        a, b = _marks(enc_old[s], slot), _marks(enc_new[s], slot)
        assert len(a - b) >= 8 and len(b - a) >= 8 and len(a & b) >= 4, (len(a - b), len(b - a))
    no = _n_out(k, m, sys_)
    others = np.setdiff1d(np.arange(no), [slot])
    slots = np.stack([np.concatenate([rng.permutation(others)[:4], [slot]])
                      for _ in range(S)]).astype(np.uint16)
    _run_and_check(k, m, sys_, ids, slots, old, new, inplace, False, null_out=null_out,
                   enc_old=enc_old, enc_new=enc_new)


def test_update_null_in_bucket(hip_lib):
    """NULL in counts: the coded rows hold no 65536 (columns of the old data
    whose encode has one are redrawn), output marks crafted."""
    k, m, sys_, U, P, S, slot = 16, 48, 1, 3, 1031, 2, 11
    rng = np.random.default_rng(901)
    ids, old, new = _crafted(k, m, sys_, U, P, S, slot, (0, 0), (100, 130), (0, 0), rng)
    for _ in range(8):
        enc_old = _encode(k, m, sys_, old)
        cols = [np.unique(np.concatenate([e[1][j, :e[2][j]] for j in range(m)])) for e in enc_old]
        if not any(len(c) for c in cols):
            break
        for s in range(S):
            c = cols[s].astype(np.int64)
            fresh = rng.integers(0, 65536, (k, len(c)), dtype=np.uint16)
            keep = np.setdiff1d(np.arange(k), ids[s])
            old[s][:, c] = fresh
            new[s][np.ix_(keep, c)] = fresh[keep]
    enc_new = _encode(k, m, sys_, new)
    assert min(len(_marks(e, slot)) for e in enc_new) >= 8
    _run_and_check(k, m, sys_, ids, None, old, new, True, False, null_in=True, enc_old=enc_old,
                   enc_new=enc_new)


def test_update_dense_input_marks(hip_lib):
    """600 and more consecutive input-marked columns of one slot across the
    boundary of a column tile, at width 4099."""
    k, m, sys_, U, P, S, slot = 16, 48, 0, 1, 4099, 2, 33
    rng = np.random.default_rng(902)
    ids, old, new = _crafted(k, m, sys_, U, P, S, slot, (TILE - 350, TILE + 350), (10, 30),
                             (0, 0), rng)
    enc_old = _encode(k, m, sys_, old)
    for e in enc_old:
        cols = np.array(sorted(_marks(e, slot) & set(range(TILE - 350, TILE + 350))))
        runs = np.split(cols, np.flatnonzero(np.diff(cols) != 1) + 1)
        best = max(runs, key=len)
        assert len(best) >= 600 and best[0] < TILE <= best[-1], len(best)
    slots = np.array([[slot, 2, 5], [7, slot, 0]], np.uint16)
    _run_and_check(k, m, sys_, ids, slots, old, new, True, False, enc_old=enc_old)


@pytest.mark.parametrize("k,m,sys_", [(16, 48, 0), (16, 48, 1), (200, 56, 1)])
def test_update_range_extremes(hip_lib, k, m, sys_):
    """Old rows pattern_rows, new rows the same rolled by 1 .. 8 columns: every
    pair of the u16 extremes meets as (old, new); U = 8, all slots."""
    U, P, S = 8, 330, 2
    rng = np.random.default_rng([k, m, sys_, 903])
    ids, _ = _pick(k, m, sys_, U, 1, S, rng)
    old = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    new = old.copy()
    pat = pattern_rows(U, P)
    for s in range(S):
        old[s, ids[s]] = pat
        new[s, ids[s]] = np.stack([np.roll(pat[u], 1 + (u + s) % 9) for u in range(U)])
    d = new.astype(np.int64) - old.astype(np.int64)
    bal = np.where(d > 32768, d - 65537, np.where(d < -32768, d + 65537, d))
    assert d.max() == 65535 and d.min() == -65535 and bal.max() == 32768 and bal.min() == -32768
    _run_and_check(k, m, sys_, ids, None, old, new, True, False)


def test_update_wide_rows(hip_lib):
    """The coded / output tensor in region class F2 (a stripe's row region
    past the 31-bit range), in place; bit for bit, nothing else written."""
    torch = _torch()
    import quadiron_amd as qa
    k, m, sys_, U, P, S = 16, 48, 0, 3, 264, 2
    no = k + m
    rng = np.random.default_rng(904)
    ids, _ = _pick(k, m, sys_, U, 1, S, rng)
    old, new = _datasets(k, P, ids, rng)
    enc_old, enc_new = _encode(k, m, sys_, old), _encode(k, m, sys_, new)
    rs = wide_rs("F2", no, P)
    backing, coded = strided_rows(S, no, P, rs, P)
    coded.copy_(torch.from_numpy(np.stack([e[0] for e in enc_old]).view(np.int16)))
    plan = qa.Plan(k, m, False)
    di = torch.from_numpy(ids.view(np.int16)).cuda()
    ctx = torch.zeros(plan.update_ctx_bytes(U, no, S), dtype=torch.uint8, device="cuda")
    plan.update_ctx(di, None, ctx)
    dold = torch.from_numpy(np.stack([old[s, ids[s]] for s in range(S)]).view(np.int16)).cuda()
    dnew = torch.from_numpy(np.stack([new[s, ids[s]] for s in range(S)]).view(np.int16)).cuda()
    counts, entries = _buckets(torch, enc_old)
    oc = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * no * CAP, dtype=torch.int32, device="cuda")
    assert plan.update(ctx, no, dold, dnew, coded, None, counts=counts, entries=entries, cap=CAP,
                       out_counts=oc, out_entries=oe, out_cap=CAP) == 0
    got = coded.cpu().numpy().view(np.uint16)
    gc = oc.cpu().numpy().view(np.uint32).reshape(S, no)
    ge = oe.cpu().numpy().view(np.uint32).reshape(S, no, CAP)
    for s in range(S):
        assert (got[s] == enc_new[s][0]).all(), s
        assert (gc[s] == enc_new[s][2]).all(), s
        for j in range(no):
            assert set(int(v) for v in ge[s, j, :gc[s, j]]) == _marks(enc_new[s], j)
    coded.fill_(FILL)
    assert backing_is_fill(backing)


def _small(torch, k, m, sys_, U, S, P):
    import quadiron_amd as qa
    no = _n_out(k, m, sys_)
    plan = qa.Plan(k, m, bool(sys_))
    rows = torch.zeros((S, U, P), dtype=torch.int16, device="cuda")
    coded = torch.full((S, no, P), FILL, dtype=torch.int16, device="cuda")
    return plan, no, rows, coded


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("what", ["id_repeated", "id_high", "slot_high", "slot_repeated"])
def test_update_bad_ids(hip_lib, sys_, what):
    torch = _torch()
    k, m, U, R, S, P = 16, 48, 3, 4, 2, 64
    plan, no, rows, coded = _small(torch, k, m, sys_, U, S, P)
    ids = np.array([[1, 5, 9], [0, 2, 15]], np.uint16)
    slots = np.array([[0, 3, 7, no - 1], [4, 5, 6, 8]], np.uint16)
    if what == "id_repeated":
        ids[1, 2] = ids[1, 0]
    elif what == "id_high":
        ids[0, 1] = k
    elif what == "slot_high":
        slots[1, 3] = no
    else:
        slots[0, 2] = slots[0, 0]
    ctx = torch.zeros(plan.update_ctx_bytes(U, R, S), dtype=torch.uint8, device="cuda")
    plan.update_ctx(torch.from_numpy(ids.view(np.int16)).cuda(),
                    torch.from_numpy(slots.view(np.int16)).cuda(), ctx)
    torch.cuda.synchronize()
    assert plan.take_error() == 2
    assert plan.take_error() == 0
    # the update of such a stripe is unspecified but stays inside the rows
    big = torch.full((S * no * P + 2 * P,), FILL, dtype=torch.int16, device="cuda")
    inner = big[P:P + S * no * P].view(S, no, P)
    plan.update(ctx, R, rows, rows, inner, None, check=False)
    torch.cuda.synchronize()
    assert (big[:P] == FILL).all() and (big[-P:] == FILL).all()


def test_update_in_bucket_over_capacity(hip_lib):
    torch = _torch()
    k, m, sys_, U, R, S, P = 16, 48, 0, 1, 2, 1, 64
    plan, no, rows, coded = _small(torch, k, m, sys_, U, S, P)
    ids = torch.zeros((S, U), dtype=torch.int16, device="cuda")
    slots = torch.tensor([[3, 9]], dtype=torch.int16, device="cuda")
    ctx = torch.zeros(plan.update_ctx_bytes(U, R, S), dtype=torch.uint8, device="cuda")
    plan.update_ctx(ids, slots, ctx)
    cap = 4
    counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    counts[9] = cap + 1
    counts[10] = cap + 5     # not listed: not read
    assert plan.update(ctx, R, rows, rows, coded, None, counts=counts, entries=entries,
                       cap=cap) == 1
    assert plan.take_error() == 0
    counts[9] = cap
    assert plan.update(ctx, R, rows, rows, coded, None, counts=counts, entries=entries,
                       cap=cap) == 0


@pytest.mark.parametrize("U,R", [(0, 4), (9, 4), (3, 0), (3, "over")])
def test_update_counts_out_of_range(hip_lib, U, R):
    """-1 from every entry point, and nothing written."""
    torch = _torch()
    import quadiron_amd as qa
    k, m, S, P = 16, 48, 2, 64
    plan, no, rows, coded = _small(torch, k, m, 0, 8, S, P)
    R = no + 1 if R == "over" else R
    lib = qa.lib()
    assert lib.qi_gpu_update_ctx_bytes(plan.h, U, R, S) == 0
    assert plan.update_kernels(U, R, P) == ""
    ids = torch.zeros(S * 16, dtype=torch.int16, device="cuda")
    slots = torch.zeros(S * (no + 1), dtype=torch.int16, device="cuda")
    ctx = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device="cuda")
    assert lib.qi_gpu_update_ctx(plan.h, ids.data_ptr(), slots.data_ptr(), U, R, S,
                                 ctx.data_ptr(), None) == -1
    assert lib.qi_gpu_update(plan.h, ctx.data_ptr(), U, R, rows.data_ptr(), 8 * P, P,
                             rows.data_ptr(), 8 * P, P, coded.data_ptr(), no * P, P, None, None,
                             0, coded.data_ptr(), no * P, P, None, None, 0, P, S, None) == -1
    torch.cuda.synchronize()
    assert (ctx == 0x5A).all() and (coded == FILL).all()
    # d_slots NULL needs n_slots = n_outputs
    if 1 <= U <= 8 and 1 <= R < no:
        assert lib.qi_gpu_update_ctx(plan.h, ids.data_ptr(), None, U, R, S, ctx.data_ptr(),
                                     None) == -1
    assert plan.take_error() == 0


def test_update_slots_null_needs_all(hip_lib):
    torch = _torch()
    import quadiron_amd as qa
    plan, no, rows, coded = _small(torch, 16, 48, 1, 2, 1, 64)
    ids = torch.zeros(2, dtype=torch.int16, device="cuda")
    ctx = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    assert qa.lib().qi_gpu_update_ctx(plan.h, ids.data_ptr(), None, 2, no - 1, 1,
                                      ctx.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert (ctx == 0x5A).all()


# ---- block API ----------------------------------------------------------

def _block_case(k, m, sys_, new_data, ids, rng, held):
    """Fec.update_blocks from old data (new_data with rows `ids` redrawn) to
    new_data, holding the coded fragments `held`; checked against the oracle's
    encode of new_data."""
    import quadiron_amd as qa
    no = _n_out(k, m, sys_)
    B = new_data.shape[1]
    old_data = new_data.copy()
    old_data[ids] = rng.integers(0, 256, (len(ids), B), dtype=np.uint8)
    cap = 128
    o_old, oor_old, cnt_old = oracle_encode_blocks(k, m, sys_, old_data, cap)
    o_new, oor_new, cnt_new = oracle_encode_blocks(k, m, sys_, new_data, cap)
    assert cnt_old.max() <= cap and cnt_new.max() <= cap
    par = [o_old[j].copy() if j in held else None for j in range(no)]
    oor, cnt = oor_old.copy(), cnt_old.copy()
    fec = qa.Fec(k, m, bool(sys_))
    fec.update_blocks(ids, [old_data[i].copy() for i in ids], [new_data[i].copy() for i in ids],
                      par, oor, cnt)
    for j in range(no):
        if j in held:
            assert (par[j] == o_new[j]).all(), j
            assert cnt[j] == cnt_new[j], (j, cnt[j], cnt_new[j])
            assert (oor[j, :cnt[j]] == oor_new[j, :cnt_new[j]]).all(), j   # ascending
            assert (np.diff(oor[j, :cnt[j]].astype(np.int64)) > 0).all()
        else:
            assert cnt[j] == cnt_old[j] and (oor[j] == oor_old[j]).all(), j
    return cnt


@pytest.mark.parametrize("k,m,sys_", [(4, 4, 1), (16, 48, 1), (16, 48, 0)])
def test_update_blocks_vs_oracle(hip_lib, k, m, sys_):
    rng = np.random.default_rng([k, m, sys_, 905])
    words = 1500
    lanes = rng.integers(0, 65536, (k, words), dtype=np.uint16)
    no = _n_out(k, m, sys_)
    held = set(int(v) for v in rng.choice(no, no // 2, replace=False))
    craft_oor_columns(k, m, sys_, lanes, rng, 12, rows=sorted(held)[:1])
    ids = [0] + [int(v) for v in 1 + rng.choice(k - 1, min(2, k - 1), replace=False)]
    cnt = _block_case(k, m, sys_, lanes.view(np.uint8).reshape(k, 2 * words), ids, rng, held)
    assert cnt[sorted(held)[0]] >= 8


@pytest.mark.parametrize("sys_", [0, 1])
def test_update_blocks_retry(hip_lib, sys_):
    """retry_block's crafted row as the new data: 100 marks in one updated
    fragment against a first-attempt capacity of 65, so the second attempt
    runs, from the rows as they were."""
    data, _, _, cnt_new, r, cap0 = retry_block(sys_)
    assert cnt_new[r] > cap0
    no = _n_out(4, 4, sys_)
    held = {r, (r + 1) % no}
    cnt = _block_case(4, 4, sys_, np.array(data), [0, 2], np.random.default_rng(906), held)
    assert cnt[r] == cnt_new[r]


def test_update_blocks_rejects(hip_lib):
    import quadiron_amd as qa
    fec = qa.Fec(16, 48, True)
    row = np.zeros(128, np.uint8)
    par = [row.copy() if j < 3 else None for j in range(48)]
    oor, cnt = np.zeros((48, 8), np.uint32), np.zeros(48, np.uint32)
    with pytest.raises(ValueError):
        fec.update_blocks(list(range(9)), [row] * 9, [row] * 9, par, oor, cnt)
    with pytest.raises(RuntimeError):
        fec.update_blocks([1, 1], [row] * 2, [row] * 2, par, oor, cnt)
    with pytest.raises(RuntimeError):
        fec.update_blocks([16], [row], [row], par, oor, cnt)


# ---- kernel names -------------------------------------------------------

def _kernel_symbols(path):
    out = subprocess.run(["nm", "-DC", path], check=True, capture_output=True,
                         text=True).stdout
    return [ln.split(" ", 2)[2] for ln in out.splitlines() if " qi::" in ln]


@pytest.mark.parametrize("k,m,sys_,U,R,P", [(16, 48, False, 1, 48 + 16, 1024),
                                            (16, 48, True, 3, 5, 37), (200, 56, True, 8, 56, 4099),
                                            (1000, 24, True, 2, 1, 1031)])
def test_reported_update_kernels_exist(hip_lib, k, m, sys_, U, R, P):
    import quadiron_amd as qa
    plan = qa.Plan(k, m, sys_)
    syms = _kernel_symbols(qa.LIB_PATH)
    kernels = plan.update_kernels(U, R, P)
    role, names = kernels.split("=", 1)
    names = [n.strip() for n in names.split(" + ")]
    assert role == "update" and len(names) >= 2, kernels
    assert names[0] == "update_ctx_kernel", kernels
    for name in names:
        pre = "qi::" + name + "("
        assert any(pre in s for s in syms), (name, kernels)
