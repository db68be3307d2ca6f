"""GPU: fused fragment repair (qi_gpu_repair_ctx / qi_gpu_repair) against the
CPU oracle.  A rebuilt fragment t must equal the oracle's encode output t of
the original data symbol for symbol, with the oracle's OOR list for that
output; a rebuilt systematic data row is the data row, with no marks.  The
received rows and their buckets are the oracle's too, so nothing expected
here comes from the product."""
import numpy as np
import pytest

from qi_testlib import (craft_dense_oor, craft_oor_columns, oracle_encode_blocks,
                        repair_matrix, retry_block, row_scale)

pytestmark = pytest.mark.gpu

CAP = 2048


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


def _pick(k, m, sys_, R, kind, rng):
    """targets first (all data / all parity / mixed), then k received ids
    among the other fragments, ascending"""
    n = k + m
    if kind == "data":
        tg = rng.choice(k, R, replace=False)
    elif kind == "parity":
        tg = k + rng.choice(m, R, replace=False)
    elif kind == "mixed" and sys_ and R >= 2:
        a = max(1, min(R - 1, k, R // 2))
        tg = np.concatenate([rng.choice(k, a, replace=False),
                             k + rng.choice(m, R - a, replace=False)])
    else:
        tg = rng.choice(n, R, replace=False)
    rest = np.setdiff1d(np.arange(n), tg)
    ids = np.sort(rng.choice(rest, k, replace=False))
    return ids.astype(np.uint16), rng.permutation(tg).astype(np.uint16)


def _encode_oracle(k, m, sys_, data):
    """per stripe: (outputs u16 (no, P), oor lists, counts) from the oracle"""
    S, _, P = data.shape
    res = []
    for s in range(S):
        o, oor, cnt = oracle_encode_blocks(
            k, m, sys_, np.ascontiguousarray(data[s]).view(np.uint8).reshape(k, 2 * P), CAP)
        assert cnt.max() <= CAP
        res.append((o.view(np.uint16).reshape(-1, P), oor, cnt))
    return res


def _upload(torch, enc, data, unaligned):
    S, k, P = data.shape
    no = enc[0][0].shape[0]
    pad_c, pad_d = (1, 3) if unaligned else (0, 0)
    cbig = torch.zeros((S, no, P + pad_c), dtype=torch.int16, device="cuda")
    dbig = torch.zeros((S, k, P + pad_d), dtype=torch.int16, device="cuda")
    coded, dd = cbig[:, :, pad_c:], dbig[:, :, pad_d:]
    coded.copy_(torch.from_numpy(np.stack([e[0] for e in enc]).view(np.int16)))
    dd.copy_(torch.from_numpy(data.view(np.int16)))
    cnt = np.stack([e[2] for e in enc]).astype(np.uint32)
    ent = np.stack([e[1] for e in enc]).astype(np.uint32)
    counts = torch.from_numpy(cnt.view(np.int32).reshape(-1)).cuda()
    entries = torch.from_numpy(ent.view(np.int32).reshape(-1)).cuda()
    return coded, dd, counts, entries


def _repair_and_check(plan, k, m, sys_, data, enc, ids, targets, unaligned=False,
                      ctx_counts=True, min_out_marks=0):
    """Runs the repair and checks every rebuilt row and bucket against the
    oracle; returns the marks found per (stripe, target)."""
    torch = _torch()
    S, _, P = data.shape
    R = targets.shape[1]
    coded, dd, counts, entries = _upload(torch, enc, data, unaligned)
    di = torch.from_numpy(ids.view(np.int16)).cuda()
    dt = torch.from_numpy(targets.view(np.int16)).cuda()
    nb = plan.repair_ctx_bytes(R, S, P)
    assert nb > 0
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    if ctx_counts:
        plan.repair_ctx(di, dt, ctx, P, counts, entries, CAP)
    else:
        plan.repair_ctx(di, dt, ctx, P)
    pad = 3 if unaligned else 0
    obig = torch.full((S, R, P + pad), 0x5a5a, dtype=torch.int16, device="cuda")
    out = obig[:, :, pad:]
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * R * CAP, dtype=torch.int32, device="cuda")
    assert plan.repair(ctx, coded, out, data=dd if sys_ else None, counts=counts,
                       entries=entries, cap=CAP, out_counts=oc, out_entries=oe,
                       out_cap=CAP) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    gc = oc.cpu().numpy().view(np.uint32).reshape(S, R)
    ge = oe.cpu().numpy().view(np.uint32).reshape(S, R, CAP)
    if pad:
        assert (obig[:, :, :pad].cpu().numpy().view(np.uint16) == 0x5a5a).all()
    marks = np.zeros((S, R), int)
    for s in range(S):
        for j in range(R):
            t = int(targets[s, j])
            sl = _slot(k, sys_, t)
            if sl is None:
                exp, em = data[s, t], np.zeros(0, np.uint32)
            else:
                exp, em = enc[s][0][sl], enc[s][1][sl, :enc[s][2][sl]]
            assert (got[s, j] == exp).all(), (s, j, t, np.flatnonzero(got[s, j] != exp)[:8])
            assert gc[s, j] == len(em), (s, j, t, gc[s, j], len(em))
            assert (np.sort(ge[s, j, :gc[s, j]]) == em).all(), (s, j, t)
            marks[s, j] = len(em)
    assert (marks.max(axis=1) >= np.asarray(min_out_marks)).all(), (marks, min_out_marks)
    return marks


def _ranges(P):
    """(output-mark ranges, input-mark ranges): tile region and tail apart"""
    W = P // 1024 * 1024
    if W == 0:
        return [(0, P // 3)], [(P // 3, P)]
    if W == P:
        return [(0, 300)], [(300, P)]
    h = W + (P - W) // 2
    return [(0, 200), (W, h)], [(200, W), (h, P)]


CASES = [
    # k, m, sys, P, R, kind, unaligned, ctx_counts
    (3, 3, 0, 1024, 1, "any", False, True),
    (3, 3, 0, 200, 2, "any", False, True),
    (3, 3, 1, 2088, 3, "mixed", False, True),
    (3, 3, 1, 200, 1, "data", False, True),
    (16, 48, 0, 1024, 1, "any", False, True),
    (16, 48, 0, 2088, 16, "any", False, True),
    (16, 48, 0, 200, 17, "any", False, True),
    (16, 48, 1, 1024, 2, "data", False, True),
    (16, 48, 1, 2088, 17, "mixed", False, True),
    (16, 48, 1, 200, 16, "parity", False, True),
    (16, 48, 1, 1024, 1, "parity", False, False),
    (16, 48, 1, 1024, 2, "mixed", True, True),
    (64, 960, 0, 1024, 17, "any", False, True),
    (64, 960, 0, 2088, 2, "any", False, True),
    (128, 128, 1, 1024, 16, "mixed", False, True),
    (128, 128, 1, 200, 1, "parity", False, True),
    (200, 56, 0, 2088, 17, "any", False, True),
    (200, 56, 0, 1024, 1, "any", False, False),
    (256, 768, 0, 1024, 2, "any", False, True),
    (256, 768, 0, 200, 16, "any", False, True),
    # the largest context: 4 row blocks, repair_ctx_kernel<256> with more
    # than 64 KiB of rows in LDS
    (256, 768, 0, 1024, 64, "any", False, True),
]


@pytest.mark.parametrize("k,m,sys_,P,R,kind,unaligned,ctx_counts", CASES)
def test_repair_vs_oracle(k, m, sys_, P, R, kind, unaligned, ctx_counts):
    import quadiron_amd as qa
    _torch()
    S = 2
    rng = np.random.default_rng(1000 * k + 10 * R + sys_ + P)
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    pick = [_pick(k, m, sys_, R, kind, rng) for _ in range(S)]
    ids = np.stack([p[0] for p in pick])
    targets = np.stack([p[1] for p in pick])
    out_rg, in_rg = _ranges(P)
    want = []  # per stripe: marks its crafted target row must hold
    for s in range(S):
        coded_t = [_slot(k, sys_, int(t)) for t in targets[s]]
        coded_t = [t for t in coded_t if t is not None]
        recv = [_slot(k, sys_, int(f)) for f in ids[s]]
        recv = [f for f in recv if f is not None]
        for lo, hi in out_rg:
            if coded_t:  # one target row holds 65536 in >= 3 columns of each range
                craft_oor_columns(k, m, sys_, data[s], rng, 5, rows=coded_t[:1],
                                  col_range=(lo, hi))
        for lo, hi in in_rg:
            if recv:
                craft_oor_columns(k, m, sys_, data[s], rng, 12, rows=recv, col_range=(lo, hi))
        want.append(3 * len(out_rg) if coded_t else 0)
    enc = _encode_oracle(k, m, sys_, data)
    for s in range(S):  # the received coded rows do hold marks
        recv = [_slot(k, sys_, int(f)) for f in ids[s]]
        recv = [f for f in recv if f is not None]
        if recv:
            assert enc[s][2][recv].sum() >= 3
    plan = qa.Plan(k, m, sys_)
    names = plan.repair_kernels(R, P)
    assert names.startswith("repair=repair_ctx_kernel<")
    cores = "matrix_mfma_kernel_both<" in names or "matrix_os_kernel_both<" in names
    if P == 1024:
        assert cores and "matrix_kernel_both<" not in names, names
    if P == 200:
        assert not cores and "matrix_kernel_both<" in names, names
    if P == 2088:
        assert cores and "matrix_kernel_both<" in names, names
    _repair_and_check(plan, k, m, sys_, data, enc, ids, targets, unaligned, ctx_counts,
                      min_out_marks=want)
    assert plan.take_error() == 0


@pytest.mark.parametrize("unaligned", [False, True])
def test_both_marks_in_one_slow_tile(unaligned):
    """More than 256 input marks in one tile and, in the same tile, columns
    where the target is 65536 -- with and without input marks in that column.
    Whole tiles: the matrix-core kernel's own redo; unaligned rows: the dot2
    kernel (one 1024-column tile at k = 16) and matrix_redo_kernel_both.  Each output mark must
    appear exactly once (the first pass of a slow tile records nothing, the
    redo records)."""
    import quadiron_amd as qa
    _torch()
    k, m, S, P, t = 16, 48, 2, 1024, 20
    rng = np.random.default_rng(77)
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    # columns 0..39: the target and received rows 3, 5 all 65536
    assert craft_dense_oor(k, m, data[0], rng, range(0, 40), [t, 3, 5], 3) > 30
    # columns 40..199: two received rows each
    assert craft_dense_oor(k, m, data[0], rng, range(40, 200), range(k), 2) > 140
    # columns 200..255: the target alone
    craft_oor_columns(k, m, 0, data[0], rng, 20, rows=[t], col_range=(200, 256))
    enc = _encode_oracle(k, m, 0, data)
    cnt = enc[0][2]
    in_tile = sum(int((enc[0][1][f, :cnt[f]] < 256).sum()) for f in range(k))
    assert in_tile > 256, in_tile
    assert cnt[t] >= 40, cnt[t]
    ids = np.tile(np.arange(k, dtype=np.uint16), (S, 1))
    targets = np.full((S, 1), t, np.uint16)
    plan = qa.Plan(k, m, False)
    _repair_and_check(plan, k, m, 0, data, enc, ids, targets, unaligned, True)
    assert plan.take_error() == 0


def _find_scaled(k, m, seed):
    """(ids, scaled target, unscaled target): a seeded search over erasure
    patterns for a repair row that needs pack_row's row scale"""
    rng = np.random.default_rng(seed)
    for _ in range(40):
        ids = np.sort(rng.choice(k + m, k, replace=False))
        rest = np.setdiff1d(np.arange(k + m), ids)
        M = repair_matrix(k, m, 0, ids, rest)
        sc = np.array([row_scale(r) for r in M])
        if (sc != 1).any() and (sc == 1).any():
            return (ids.astype(np.uint16), int(rest[np.flatnonzero(sc != 1)[0]]),
                    int(rest[np.flatnonzero(sc == 1)[0]]))
    return None


@pytest.mark.parametrize("k,m", [(64, 960), (200, 56)])
def test_repair_row_scale(k, m):
    import quadiron_amd as qa
    _torch()
    found = _find_scaled(k, m, 4242 + k)
    assert found is not None, "no repair row needing a scale found"
    ids1, t_scaled, t_plain = found
    S, P = 2, 1024 + 40
    rng = np.random.default_rng(k)
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    ids = np.stack([ids1, ids1])
    targets = np.array([[t_scaled], [t_plain]], np.uint16)
    for s in range(S):
        craft_oor_columns(k, m, 0, data[s], rng, 4, rows=[int(targets[s, 0])])
        craft_oor_columns(k, m, 0, data[s], rng, 8, rows=[int(f) for f in ids1])
    enc = _encode_oracle(k, m, 0, data)
    plan = qa.Plan(k, m, False)
    _repair_and_check(plan, k, m, 0, data, enc, ids, targets)
    assert plan.take_error() == 0


def _ctx_error(plan, ids, targets, P=200, counts=None, entries=None, cap=0):
    torch = _torch()
    S, R = targets.shape
    di = torch.from_numpy(np.ascontiguousarray(ids, np.uint16).view(np.int16)).cuda()
    dt = torch.from_numpy(np.ascontiguousarray(targets, np.uint16).view(np.int16)).cuda()
    ctx = torch.zeros(plan.repair_ctx_bytes(R, S, P), dtype=torch.uint8, device="cuda")
    plan.repair_ctx(di, dt, ctx, P, counts, entries, cap)
    torch.cuda.synchronize()
    return plan.take_error()


def test_repair_errors():
    import quadiron_amd as qa
    torch = _torch()
    L = qa.lib()
    plan = qa.Plan(3, 3, False)  # k + m = 6 < n = 8
    ids = np.array([[0, 2, 4]])
    assert _ctx_error(plan, ids, np.array([[1, 5]])) == 0
    assert _ctx_error(plan, ids, np.array([[2, 5]])) & 2   # a received id
    assert _ctx_error(plan, ids, np.array([[1, 1]])) & 2   # repeated
    assert _ctx_error(plan, ids, np.array([[1, 6]])) & 2   # >= k + m (< n)
    assert _ctx_error(plan, np.array([[0, 0, 4]]), np.array([[1, 5]])) & 2
    assert _ctx_error(plan, ids, np.array([[1, 5]])) == 0
    # an input bucket over its capacity: bit 1, as for a decode
    cap = 4
    counts = torch.zeros(6, dtype=torch.int32, device="cuda")
    counts[2] = cap + 1
    entries = torch.zeros(6 * cap, dtype=torch.int32, device="cuda")
    assert _ctx_error(plan, ids, np.array([[1, 5]]), counts=counts, entries=entries,
                      cap=cap) & 1
    # n_targets out of range: refused, nothing launched
    big = qa.Plan(64, 960, False)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert big.repair_ctx_bytes(64, 1, 200) > 0
    for R in (0, 65, -1):
        assert big.repair_ctx_bytes(R, 1, 200) == 0
        assert L.qi_gpu_repair_ctx(big.h, p, p, R, 1, None, None, 0, 200, p, None) == -1
        assert L.qi_gpu_repair(big.h, p, R, p, 0, 200, p, 0, 200, None, None, 0, p, 0, 200,
                               None, None, 0, 200, 1, None) == -1
    assert plan.repair_ctx_bytes(4, 1, 200) == 0  # more targets than parities
    with pytest.raises(ValueError):
        big.repair_ctx(buf.view(torch.int16)[:64].reshape(1, 64),
                       buf.view(torch.int16)[:65].reshape(1, 65), buf, 200)
    torch.cuda.synchronize()
    assert big.take_error() == 0
    # k > 256: unsupported
    p300 = qa.Plan(300, 100, False)
    assert p300.repair_ctx_bytes(1, 1, 1024) == 0
    assert p300.repair_kernels(1, 1024) == ""
    assert L.qi_gpu_repair_ctx(p300.h, p, p, 1, 1, None, None, 0, 1024, p,
                               None) == qa.Plan.ERR_UNSUPPORTED
    assert L.qi_gpu_repair(p300.h, p, 1, p, 0, 1024, p, 0, 1024, None, None, 0, p, 0, 1024,
                           None, None, 0, 1024, 1, None) == qa.Plan.ERR_UNSUPPORTED


# ---- upper layers -------------------------------------------------------

FEC_CASES = [
    # sys, targets, further missing fragments
    (0, [5], []),                 # a low coded row (a "data" buffer of the C-ABI)
    (0, [40], []),                # a parity
    (0, [3, 50], [0, 7, 20, 33, 60]),
    (1, [5], []),                 # a data row
    (1, [40], []),                # a parity
    (1, [3, 50], [0, 7, 20, 33, 60]),
    (1, [20], [1, 2]),            # a parity with data rows missing
]


@pytest.mark.parametrize("sys_,targets,extra", FEC_CASES)
def test_fec_repair_blocks_vs_oracle(sys_, targets, extra):
    """Fec.repair_blocks (qi_fec_repair_blocks, RsFnt::repair_blocks_vertical)
    on a 10000-byte block (4 whole tiles and a 904-column tail): rows and
    ascending marks equal the oracle's outputs; a data row has no marks."""
    import quadiron_amd as qa
    _torch()
    k, m, B = 16, 48, 10000
    P = B // 2
    rng = np.random.default_rng(500 + sys_ + 7 * len(targets) + targets[0])
    data = rng.integers(0, 65536, (k, P), dtype=np.uint16)
    miss = np.zeros(k + m, np.int32)
    miss[targets + extra] = 1
    present = [f for f in range(k + m) if not miss[f]]
    recv = [_slot(k, sys_, f) for f in present[:k + 8]]
    recv = [f for f in recv if f is not None]
    for t in targets:
        sl = _slot(k, sys_, t)
        if sl is not None:
            craft_oor_columns(k, m, sys_, data, rng, 4, rows=[sl], col_range=(0, 2000))
            craft_oor_columns(k, m, sys_, data, rng, 3, rows=[sl], col_range=(4096, 4500))
    craft_oor_columns(k, m, sys_, data, rng, 20, rows=recv, col_range=(2000, 4096))
    craft_oor_columns(k, m, sys_, data, rng, 6, rows=recv, col_range=(4500, P))
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, data.view(np.uint8).reshape(k, B), 256)
    assert cnt.max() <= 256
    no = outs.shape[0]
    first = k if sys_ else 0
    pars = [None if miss[first + i] else outs[i].copy() for i in range(no)]
    drows = ([None if miss[i] else data[i].view(np.uint8).copy() for i in range(k)]
             if sys_ else None)
    fec = qa.Fec(k, m, bool(sys_))
    res = fec.repair_blocks(drows, pars, oor, cnt, miss, targets, out_cap=64)
    assert res is not None
    rows, o_oor, o_cnt = res
    for j, t in enumerate(targets):
        sl = _slot(k, sys_, t)
        if sl is None:
            assert (rows[j] == data[t].view(np.uint8)).all() and o_cnt[j] == 0
        else:
            assert (rows[j] == outs[sl]).all(), (t, np.flatnonzero(rows[j] != outs[sl])[:8])
            assert o_cnt[j] == cnt[sl] and cnt[sl] >= 3, (t, o_cnt[j], cnt[sl])
            assert (o_oor[j, :o_cnt[j]] == oor[sl, :cnt[sl]]).all()  # ascending
    # fewer than k fragments: not rebuilt
    miss2 = np.ones(k + m, np.int32)
    miss2[present[:k - 1]] = 0
    assert fec.repair_blocks(drows, pars, oor, cnt, miss2, targets) is None
    # a target that is present, and shapes the fused path does not take
    with pytest.raises(RuntimeError):
        fec.repair_blocks(drows, pars, oor, cnt, miss, [present[0]])
    with pytest.raises(ValueError):
        fec.repair_blocks(drows, pars, oor, cnt, miss, [])


@pytest.mark.parametrize("sys_", [0, 1])
def test_fec_repair_blocks_retry(sys_):
    """The single target holds more marks than the first attempt's output
    buckets (64 + words / 512 = 65): Fec.repair_blocks runs the repair again
    with the exact capacity; the row and its ascending marks equal the
    oracle's."""
    import quadiron_amd as qa
    _torch()
    k, m = 4, 4
    data, outs, oor, cnt, r, first_cap = retry_block(sys_)
    assert first_cap < cnt[r] <= 128 and cnt.max() <= 128, cnt
    target = k + r if sys_ else r
    miss = np.zeros(k + m, np.int32)
    miss[target] = 1
    pars = [None if i == r else outs[i].copy() for i in range(outs.shape[0])]
    drows = [data[i].copy() for i in range(k)] if sys_ else None
    fec = qa.Fec(k, m, bool(sys_))
    res = fec.repair_blocks(drows, pars, oor, cnt, miss, [target], out_cap=128)
    assert res is not None
    rows, o_oor, o_cnt = res
    assert (rows[0] == outs[r]).all(), np.flatnonzero(rows[0] != outs[r])[:8]
    assert o_cnt[0] == cnt[r], (o_cnt[0], cnt[r])
    assert (o_oor[0, :o_cnt[0]] == oor[r, :cnt[r]]).all()  # ascending


@pytest.mark.parametrize("k,m,sys_", [(16, 48, 0), (16, 48, 1), (6, 3, 1)])
def test_reconstruct_fused_equals_two_pass(k, m, sys_, monkeypatch):
    """quadiron_fnt32_reconstruct through the fused route (the default where
    the plan supports it) and through the decode + encode route
    (QI_RECONSTRUCT_ROUTE=two-pass, read at call time) on the same buffers:
    the same bytes and FNT1 headers, equal to the oracle's frames."""
    import ctypes as C
    import quadiron_amd as qa
    from qi_testlib import codec, oracle, ptrs, vp
    _torch()
    rng = np.random.default_rng(900 + k + sys_)
    words = 5000
    B = 2 * words
    lanes = rng.integers(0, 65536, (k, words), dtype=np.uint16)
    # (an FNT1 header of this block size holds about a dozen marks)
    craft_oor_columns(k, m, sys_, lanes, rng, min(40, 3 * (m if sys_ else k + m)))
    h = qa.QuadironFnt32(2, k, m, sys_)
    md = h.metadata_size(B)
    c = codec(k, m, sys_)
    od = [np.concatenate([np.zeros(md, np.uint8), lanes[i].view(np.uint8)]) for i in range(k)]
    op = [np.zeros(md + B, np.uint8) for _ in range(m)]
    assert oracle().qo_fnt32_encode(C.byref(c), ptrs(od), ptrs(op),
                                    vp(np.ones(c.n_outputs, np.int32)), C.c_size_t(B)) == 0
    frames = od + op
    assert sum(int.from_bytes(bytes(f[4:8]), "big") for f in frames) >= 5
    dests = [1, k + 1, k + m - 1]
    for dest in dests:
        miss = np.zeros(k + m, np.int32)
        gone = [dest] + [f for f in (0, k, 2) if f != dest][:min(2, m - 1)]
        miss[gone] = 1
        got = {}
        for route in ("fused", "two-pass"):
            if route == "two-pass":
                monkeypatch.setenv("QI_RECONSTRUCT_ROUTE", "two-pass")
            else:
                monkeypatch.delenv("QI_RECONSTRUCT_ROUTE", raising=False)
            D = [frames[i].copy() if not miss[i] else np.zeros(md + B, np.uint8)
                 for i in range(k)]
            Pp = [frames[k + i].copy() if not miss[k + i] else np.zeros(md + B, np.uint8)
                  for i in range(m)]
            assert h.reconstruct(D, Pp, miss, dest, B) == 0, (dest, route)
            got[route] = (D + Pp)[dest].copy()
        assert (got["fused"] == got["two-pass"]).all(), dest
        assert (got["fused"][md:] == frames[dest][md:]).all(), dest
        if not (sys_ and dest < k):  # a coded fragment: the oracle's header too
            assert (got["fused"][:md] == frames[dest][:md]).all(), dest
