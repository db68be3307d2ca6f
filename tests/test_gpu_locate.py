"""GPU: fragment locate (qi_gpu_locate_ctx / qi_gpu_locate).  The codewords
come from the product's own encode (pinned to the oracle by the encode tests);
every expected result is known by construction, from the injected errors: a
column with one bad listed fragment is located there with the original symbol
as its correction, one with 2 .. R - 1 bad fragments is unlocated."""
import functools
import subprocess

import numpy as np
import pytest

from qi_testlib import FILL, craft_oor_columns, strided_rows

pytestmark = pytest.mark.gpu

Q = 65537
TILE = 2048          # the locate kernel's column tile
WIDTHS = (1, 7, TILE, TILE + 13, 2 * TILE + 1)
PMAX = WIDTHS[-1]
S = 3
CAP = 64
CODES = [(3, 3, 2), (3, 3, 3), (16, 48, 2), (16, 48, 4), (16, 48, 8), (200, 56, 8),
         (256, 768, 8)]


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device")
    torch.cuda.set_device(0)
    return torch


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).reshape(-1)).cuda()


def _encode(k, m, sys_, data, cap):
    """The product's encode of data [S, k, P] u16 -> the restored symbols by
    fragment id, int32 [S, k + m, P] (65536 where the encode marked)."""
    torch = _torch()
    import quadiron_amd as qa
    plan = qa.Plan(k, m, bool(sys_))
    S_, _, P = data.shape
    no = plan.n_outputs
    dd = torch.from_numpy(data.view(np.int16)).cuda()
    out = torch.zeros((S_, no, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S_ * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S_ * no * cap, dtype=torch.int32, device="cuda")
    plan.encode(dd, out, counts, entries, cap)
    torch.cuda.synchronize()
    assert plan.take_error() == 0
    coded = out.cpu().numpy().view(np.uint16).astype(np.int32)
    cnt = counts.cpu().numpy().reshape(S_, no)
    ent = entries.cpu().numpy().view(np.uint32).reshape(S_, no, cap)
    assert cnt.max() <= cap
    for s in range(S_):
        for j in range(no):
            cols = ent[s, j, :cnt[s, j]]
            assert (coded[s, j, cols] == 0).all()
            coded[s, j, cols] = 65536
    plan.close()
    return np.concatenate([data.astype(np.int32), coded], axis=1) if sys_ else coded


@functools.lru_cache(maxsize=None)
def _truth(k, m, sys_):
    """random codewords [S, k + m, PMAX], shared by the tests (never written)"""
    rng = np.random.default_rng(7 * k + sys_)
    data = rng.integers(0, 65536, (S, k, PMAX), dtype=np.uint16)
    t = _encode(k, m, sys_, data, CAP)
    t.setflags(write=False)
    return t


def _ids(k, m, R, rng, n=S):
    """[n, k + R] listed ids, different per stripe; 0 and k + m - 1 are used"""
    ids = np.stack([rng.permutation(k + m)[:k + R] for _ in range(n)])
    if 0 not in ids[0]:
        ids[0, 0] = 0
    if k + m - 1 not in ids[n - 1]:
        ids[n - 1, -1] = k + m - 1
    return ids.astype(np.uint16)


def _dev_rows(torch, arr, unaligned):
    """[S, rows, P] device view of arr inside a FILL-filled backing; unaligned:
    at an odd u16 offset with an odd row stride"""
    S_, rows, P = arr.shape
    pad = 1 if unaligned else 0
    width = P + pad
    if unaligned and width % 2 == 0:
        width += 1
    big = torch.full((S_, rows, width), FILL, dtype=torch.int16, device="cuda")
    view = big[:, :, pad:pad + P]
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr).astype(np.uint16).view(np.int16)))
    if unaligned:
        assert view.data_ptr() % 4 == 2 and view.stride(1) % 2 == 1
    return big, view


def _store(k, sys_, recv, garbage=()):
    """received restored symbols [S, k + m, P] -> (data u16 or None, coded u16,
    marks: list per (s, slot) of columns).  garbage: (s, slot, col, value)
    stored under a mark."""
    first = k if sys_ else 0
    data = None
    if sys_:
        assert recv[:, :k].max() < 65536
        data = recv[:, :k].astype(np.uint16)
    cr = recv[:, first:]
    marks = [[np.nonzero(cr[s, j] == 65536)[0] for j in range(cr.shape[1])]
             for s in range(cr.shape[0])]
    coded = (cr & 0xffff).astype(np.uint16)
    for s, j, c, v in garbage:
        assert cr[s, j, c] == 65536
        coded[s, j, c] = v
    return data, coded, marks


def _expect(truth, recv, ids, R, rows=None):
    """per list position: located [N], unlocated, fixes {(col, pos, v)} and the
    number of columns too bad to assert (>= R bad fragments; 2 at R = 2)"""
    res = []
    for s in range(ids.shape[0]):
        sr = s if rows is None else int(rows[s])
        bad = truth[sr][ids[s]] != recv[sr][ids[s]]           # [N, P]
        nb = bad.sum(axis=0)
        loc = np.zeros(ids.shape[1], np.int64)
        fixes = set()
        for c in np.nonzero(nb == 1)[0]:
            p = int(np.nonzero(bad[:, c])[0][0])
            loc[p] += 1
            fixes.add((int(c), p, int(truth[sr, ids[s, p], c])))
        strict = (nb >= 2) & (nb <= R - 1)
        res.append((loc, int(strict.sum()), fixes, int(((nb >= 2) & ~strict).sum())))
    return res


def _locate(k, m, sys_, R, ids, recv, unaligned=False, rows=None, cap=None, fix_cap=None,
            garbage=(), null_counts=False):
    """runs the locate over recv; returns (err, located [L, N], unlocated [L],
    fix_counts [L], fixes [L, fix_cap, 3])"""
    torch = _torch()
    import quadiron_amd as qa
    plan = qa.Plan(k, m, bool(sys_))
    L, N = ids.shape
    S_all, _, P = recv.shape
    no = plan.n_outputs
    data, coded, marks = _store(k, sys_, recv, garbage)
    cap = cap or max(CAP, max(len(c) for ms in marks for c in ms))
    fix_cap = P if fix_cap is None else fix_cap
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
    nb = plan.locate_ctx_bytes(R, L)
    RP = 2 if R <= 2 else 4 if R <= 4 else 8
    assert nb == L * 4 * N * (3 + RP)
    ctx = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    plan.locate_ctx(torch.from_numpy(ids.view(np.int16)).cuda(), ctx)
    located = torch.full((L * N,), 7, dtype=torch.int32, device="cuda")
    unloc = torch.full((L,), 7, dtype=torch.int32, device="cuda")
    fcnt = torch.full((L,), 7, dtype=torch.int32, device="cuda")
    fixes = torch.full((L * max(fix_cap, 1) * 3,), -1, dtype=torch.int32, device="cuda")
    err = plan.locate(ctx, R, dc, located, unloc, fcnt, fixes if fix_cap else None, fix_cap,
                      data=dd, counts=None if null_counts else _i32(torch, cnt),
                      entries=None if null_counts else _i32(torch, ent), cap=cap,
                      stripes=None if rows is None else _i32(torch, rows))
    torch.cuda.synchronize()
    # no row was written
    assert (dc.cpu().numpy().view(np.uint16) == coded).all()
    if sys_:
        assert (dd.cpu().numpy().view(np.uint16) == data).all()
    plan.close()
    return (err, located.cpu().numpy().reshape(L, N), unloc.cpu().numpy(), fcnt.cpu().numpy(),
            fixes.cpu().numpy().reshape(L, max(fix_cap, 1), 3))


def _check(res, exp, R):
    err, located, unloc, fcnt, fixes = res
    assert err == 0
    for s, (loc, nun, fx, loose) in enumerate(exp):
        if loose == 0:
            assert (located[s] == loc).all(), (s, located[s], loc)
            assert unloc[s] == nun, (s, unloc[s], nun)
            assert fcnt[s] == len(fx)
            got = set(tuple(int(v) for v in f) for f in fixes[s, :fcnt[s]])
            assert got == fx, (s, sorted(got ^ fx)[:5])
        else:
            # more bad fragments than the guards can tell apart: only the sum
            assert located[s].sum() + unloc[s] == loc.sum() + nun + loose
            assert fcnt[s] == located[s].sum()


def _single_errors(truth, ids, rng, n_data):
    """one error per bad column, cycled over the listed positions and over e
    in {1, 65536, 32768, random}; fragments below n_data are data rows and stay
    below 65536 (another e)"""
    recv = truth.copy()
    L, N = ids.shape
    P = truth.shape[2]
    for s in range(L):
        cols = rng.permutation(P)[:min(P, 4 * N)]
        for i, c in enumerate(cols):
            p = (i + s) % N
            e = (1, 65536, 32768, int(rng.integers(1, Q)))[(i // N + s) % 4]
            f = ids[s, p]
            v = (truth[s, f, c] + e) % Q
            if v == 65536 and f < n_data:
                v = (truth[s, f, c] + 2) % 65536
            recv[s, f, c] = v
    return recv


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("k,m,R", CODES)
def test_clean_and_single_errors(k, m, R, sys_, unaligned):
    full = _truth(k, m, sys_)
    rng = np.random.default_rng(k + R + sys_)
    ids = _ids(k, m, R, rng)
    for P in WIDTHS:
        truth = np.ascontiguousarray(full[:, :, :P])
        # clean rows: every output is zero
        err, located, unloc, fcnt, _ = _locate(k, m, sys_, R, ids, truth, unaligned)
        assert err == 0 and not located.any() and not unloc.any() and not fcnt.any()
        recv = _single_errors(truth, ids, rng, k if sys_ else 0)
        exp = _expect(truth, recv, ids, R)
        assert all(e[1] == 0 and e[3] == 0 for e in exp)
        if P >= 4 * (k + R):
            assert all((e[0] >= 1).all() for e in exp)    # every position is hit
        _check(_locate(k, m, sys_, R, ids, recv, unaligned), exp, R)


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("k,m,R", [(16, 48, 2), (16, 48, 4), (16, 48, 8), (200, 56, 8)])
def test_more_than_one_bad_fragment(k, m, R, sys_):
    P = TILE + 13
    truth = np.ascontiguousarray(_truth(k, m, sys_)[:, :, :P])
    rng = np.random.default_rng(3 * k + R)
    ids = _ids(k, m, R, rng)
    recv = truth.copy()
    for s in range(S):
        for i, c in enumerate(rng.permutation(P)[:60]):
            nb = (2, max(2, R - 1), 1)[i % 3]
            for p in rng.choice(k + R, nb, replace=False):
                f = ids[s, p]
                lim = 65536 if sys_ and f < k else Q
                recv[s, f, c] = (truth[s, f, c] + int(rng.integers(1, lim))) % lim
    exp = _expect(truth, recv, ids, R)
    if R >= 3:
        assert all(e[1] == 40 and e[3] == 0 for e in exp)
    else:
        assert all(e[3] == 40 for e in exp)
    _check(_locate(k, m, sys_, R, ids, recv), exp, R)


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("sys_", [0, 1])
def test_errors_that_are_marks(sys_, unaligned):
    k, m, R = 16, 48, 4
    P = TILE + 13
    rng = np.random.default_rng(11 + sys_)
    data = rng.integers(0, 65536, (S, k, P), dtype=np.uint16)
    for s in range(S):
        craft_oor_columns(k, m, sys_, data[s], rng, 200)
    truth = _encode(k, m, sys_, data, 512)
    first = k if sys_ else 0
    if sys_:   # mostly coded fragments (the ones with marks) and two data rows
        ids = np.stack([np.concatenate([k + rng.permutation(m)[:k + R - 2],
                                        rng.permutation(k)[:2]]) for _ in range(S)])
    else:
        ids = np.stack([rng.permutation(k + m)[:k + R] for _ in range(S)])
    ids = ids.astype(np.uint16)
    recv = truth.copy()
    garbage = []
    kinds = 0
    for s in range(S):
        lt = truth[s][ids[s]]                                  # [N, P]
        marked = np.argwhere(lt == 65536)
        assert len(marked) >= 12
        used = set()
        for i, (p, c) in enumerate(marked):
            if c in used:
                continue
            used.add(c)
            f = ids[s, p]
            if i % 3 == 0:
                recv[s, f, c] = 0                              # a dropped mark
            elif i % 3 == 1:
                recv[s, f, c] = int(rng.integers(1, 65536))    # dropped, wrong value
            else:
                garbage.append((s, f - first, int(c), 12345))  # kept, wrong value: no error
            kinds |= 1 << i % 3
        for c in rng.permutation(P)[:40]:                      # spurious marks
            if c in used:
                continue
            p = int(rng.integers(0, k + R))
            f = ids[s, p]
            if f >= first and truth[s, f, c] != 65536:
                recv[s, f, c] = 65536
                used.add(c)
    assert kinds == 7
    exp = _expect(truth, recv, ids, R)
    assert all(any(v == 65536 for _, _, v in e[2]) for e in exp)   # 65536 is a fix
    _check(_locate(k, m, sys_, R, ids, recv, unaligned, garbage=garbage), exp, R)


@pytest.mark.parametrize("sys_", [0, 1])
def test_accumulator_ends(sys_):
    """All-65535 codewords (the constant polynomial), and columns whose coded
    symbols are all 65536 -- the constant polynomial 65536, every coded row
    marked in every column, more than 256 marks per tile and row -- with a
    single error on top."""
    k, m, R = 16, 48, 8
    P = TILE + 13
    rng = np.random.default_rng(5)
    ids = _ids(k, m, R, rng)
    first = k if sys_ else 0
    for const in (65535, 65536):
        truth = np.full((S, k + m, P), const, np.int32)
        if const == 65536:
            if sys_:
                continue        # a data row cannot hold 65536
        recv = truth.copy()
        for s in range(S):
            for i, c in enumerate(rng.permutation(P)[:3 * (k + R)]):
                p = i % (k + R)
                f = ids[s, p]
                lim = 65536 if f < first else Q
                recv[s, f, c] = (truth[s, f, c] + (1, 32768, 65535)[i // (k + R)]) % lim
        exp = _expect(truth, recv, ids, R)
        err, *clean = _locate(k, m, sys_, R, ids, truth, cap=P)
        assert err == 0 and not any(a.any() for a in clean[:3])
        _check(_locate(k, m, sys_, R, ids, recv, cap=P), exp, R)


def test_buckets_and_capacities():
    k, m, R, sys_ = 16, 48, 4, 0
    P = TILE + 13
    truth = np.ascontiguousarray(_truth(k, m, sys_)[:, :, :P]).copy()
    rng = np.random.default_rng(9)
    ids = _ids(k, m, R, rng)
    # a dense bucket: 300 spurious marks in one listed row of stripe 1 (all in
    # tile 0: more than 256 marks of one row in one tile), each an error
    recv = truth.copy()
    f = ids[1, 3]
    cols = rng.permutation(TILE)[:300]
    cols = cols[truth[1, f, cols] != 65536]
    recv[1, f, cols] = 65536
    exp = _expect(truth, recv, ids, R)
    assert exp[1][0][3] == len(cols) > 256
    _check(_locate(k, m, sys_, R, ids, recv, cap=512), exp, R)
    # the same bucket over oor_cap raises bit 1
    res = _locate(k, m, sys_, R, ids, recv, cap=CAP)
    assert res[0] & 1
    # fix_cap smaller than the fixes: exact count, valid kept entries
    err, located, unloc, fcnt, fixes = _locate(k, m, sys_, R, ids, recv, cap=512, fix_cap=10)
    assert err == 0 and fcnt[1] == len(cols) and located[1, 3] == len(cols)
    kept = set(tuple(int(v) for v in fx) for fx in fixes[1])
    assert len(kept) == 10 and kept <= exp[1][2]
    # fix_cap 0: counts only
    err, located, unloc, fcnt, _ = _locate(k, m, sys_, R, ids, recv, cap=512, fix_cap=0)
    assert err == 0 and fcnt[1] == len(cols) and fcnt[0] == 0


@pytest.mark.parametrize("sys_", [0, 1])
def test_stripe_list(sys_):
    """d_stripes = {2, 0} of 3: outputs by list position, stripe 1's
    corruption is not reported."""
    k, m, R = 16, 48, 4
    P = TILE + 13
    truth = np.ascontiguousarray(_truth(k, m, sys_)[:, :, :P])
    rng = np.random.default_rng(21 + sys_)
    ids3 = _ids(k, m, R, rng)
    recv = _single_errors(truth, ids3, rng, k if sys_ else 0)
    rows = np.array([2, 0], np.uint32)
    ids = np.ascontiguousarray(ids3[[2, 0]])
    exp = _expect(truth, recv, ids, R, rows)
    assert exp[0][2] != exp[1][2]
    _check(_locate(k, m, sys_, R, ids, recv, rows=rows), exp, R)


def test_bad_input():
    torch = _torch()
    import quadiron_amd as qa
    k, m, R = 16, 48, 4
    truth = np.ascontiguousarray(_truth(k, m, 0)[:, :, :7])
    rng = np.random.default_rng(2)
    for kind in ("repeat", "range"):
        ids = _ids(k, m, R, rng)
        ids[1, 5] = ids[1, 2] if kind == "repeat" else k + m
        res = _locate(k, m, 0, R, ids, truth)
        assert res[0] & 2, kind
    plan = qa.Plan(3, 3, False)
    lib = qa.lib()
    buf = torch.zeros(4096, dtype=torch.int32, device="cuda")
    rows = torch.zeros((1, 6, 8), dtype=torch.int16, device="cuda")
    for bad in (1, 9, 4):
        assert plan.locate_ctx_bytes(bad, 1) == 0
        assert plan.locate_kernels(bad, 64) == ""
        assert lib.qi_gpu_locate_ctx(plan.h, buf.data_ptr(), bad, 1, buf.data_ptr(), None) == -1
        assert lib.qi_gpu_locate(plan.h, buf.data_ptr(), bad, None, None, 0, 0, rows.data_ptr(),
                                 48, 8, None, None, 0, buf.data_ptr(), buf.data_ptr(),
                                 buf.data_ptr(), None, 0, 8, 1, None) == -1
    torch.cuda.synchronize()
    assert not buf.any()                                      # nothing was launched
    plan.close()
    big = qa.Plan(300, 212, False)
    assert big.locate_ctx_bytes(4, 1) == 0 and big.locate_kernels(4, 64) == ""
    unsupported = -5                                          # QI_ERR_UNSUPPORTED
    assert lib.qi_gpu_locate_ctx(big.h, buf.data_ptr(), 4, 1, buf.data_ptr(), None) == unsupported
    rows = torch.zeros((1, 512, 8), dtype=torch.int16, device="cuda")
    assert lib.qi_gpu_locate(big.h, buf.data_ptr(), 4, None, None, 0, 0, rows.data_ptr(),
                             4096, 8, None, None, 0, buf.data_ptr(), buf.data_ptr(),
                             buf.data_ptr(), None, 0, 8, 1, None) == unsupported
    torch.cuda.synchronize()
    assert not buf.any()
    big.close()


def test_wide_rows():
    """Rows more than 2^31 bytes apart (flat 64-bit row offsets)."""
    torch = _torch()
    import quadiron_amd as qa
    k, m, R, P = 3, 3, 2, 40
    truth = np.ascontiguousarray(_truth(k, m, 0)[:1, :, :P])
    ids = np.array([[5, 0, 3, 1, 4]], np.uint16)
    recv = truth.copy()
    recv[0, 5, 9] = (truth[0, 5, 9] + 1) % Q
    recv[0, 1, 33] = (truth[0, 1, 33] + 32768) % Q
    assert recv.max() < 65536 and truth.max() < 65536
    rs = (1 << 30) + 8
    backing, view = strided_rows(1, k + m, P, rs, (k + m) * rs)
    view.copy_(torch.from_numpy(recv.astype(np.uint16).view(np.int16)))
    plan = qa.Plan(k, m, False)
    ctx = torch.zeros(plan.locate_ctx_bytes(R, 1), dtype=torch.uint8, device="cuda")
    plan.locate_ctx(torch.from_numpy(ids.view(np.int16)).cuda(), ctx)
    out = [torch.zeros(n, dtype=torch.int32, device="cuda") for n in (5, 1, 1, 3 * 8)]
    assert plan.locate(ctx, R, view, out[0], out[1], out[2], out[3], 8) == 0
    assert out[0].tolist() == [1, 0, 0, 1, 0] and out[1].item() == 0 and out[2].item() == 2
    got = set(tuple(f) for f in out[3].cpu().numpy().reshape(8, 3)[:2].tolist())
    assert got == {(9, 0, int(truth[0, 5, 9])), (33, 3, int(truth[0, 1, 33]))}
    plan.close()
    del backing, view


@pytest.mark.parametrize("R,rp", [(2, 2), (3, 4), (4, 4), (5, 8), (8, 8)])
def test_locate_kernel_names(R, rp):
    """qi_gpu_locate_kernels names kernels the library contains, spelled as
    the demangler (and so a profile) spells them."""
    import quadiron_amd as qa
    out = subprocess.run(["nm", "-DC", qa.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    syms = [ln.split(" ", 2)[2] for ln in out.splitlines() if " qi::" in ln]
    plan = qa.Plan(16, 48, False)
    names = plan.locate_kernels(R, TILE)
    assert names == f"locate=locate_ctx_kernel<{rp}> + locate_kernel<{rp}, true>"
    for name in names.split("=")[1].split(" + "):
        assert any("qi::" + name + "(" in s for s in syms), name
    assert any(f"qi::locate_kernel<{rp}, false>(" in s for s in syms)
    plan.close()


# ---- host layers ---------------------------------------------------------

def _host_fragments(k, m, sys_, P, rng, n_marks=40):
    """one stripe through the product's encode: (rows by fragment id as uint8
    arrays, oor (n_out, cap) and counts of the coded rows, ascending)"""
    data = rng.integers(0, 65536, (1, k, P), dtype=np.uint16)
    craft_oor_columns(k, m, sys_, data[0], rng, n_marks)
    truth = _encode(k, m, sys_, data, 256)[0]                 # [k + m, P]
    first = k if sys_ else 0
    no = k + m - first
    cap = 128
    oor = np.zeros((no, cap), np.uint32)
    cnt = np.zeros(no, np.uint32)
    for j in range(no):
        cols = np.nonzero(truth[first + j] == 65536)[0]
        assert len(cols) < cap - 8
        oor[j, :len(cols)] = cols
        cnt[j] = len(cols)
    rows = [np.ascontiguousarray((truth[f] & 0xffff).astype(np.uint16)).view(np.uint8).copy()
            for f in range(k + m)]
    assert cnt.sum() >= 10
    return truth, rows, oor, cnt


@pytest.mark.parametrize("sys_", [0, 1])
def test_fec_locate_blocks(sys_):
    """Fec.locate_blocks at (16, 48): counts per fragment id, -1 for missing
    and unlisted fragments, the unlocated count last; more fixes than the
    first attempt's list holds (64 + words / 512 = 66) run again; with
    correct=True the buffers and the mark lists equal the uncorrupted ones and
    a following verify_blocks is clean."""
    import quadiron_amd as qa
    _torch()
    k, m = 16, 48
    P = 1024 + 40
    rng = np.random.default_rng(40 + sys_)
    truth, rows, oor, cnt = _host_fragments(k, m, sys_, P, rng)
    first = k if sys_ else 0
    miss = np.zeros(k + m, np.int32)
    miss[[1, 17, 20]] = 1
    present = [f for f in range(k + m) if not miss[f]]
    listed = present[:k + 8]                                  # data before parities
    clean_rows = [r.copy() for r in rows]
    clean_oor, clean_cnt = oor.copy(), cnt.copy()

    def args():
        data = [None if miss[f] else rows[f] for f in range(k)] if sys_ else None
        pars = [None if miss[first + j] else rows[first + j] for j in range(k + m - first)]
        return data, pars

    fec = qa.Fec(k, m, bool(sys_))
    res = fec.locate_blocks(*args(), oor, cnt, miss)
    exp = np.full(k + m + 1, -1, np.int64)
    exp[listed] = 0
    exp[-1] = 0
    assert res.tolist() == exp.tolist()

    # 100 single errors over the listed fragments (more than 66 fixes), among
    # them a dropped mark, a spurious mark and a wrong word under no mark
    bad = {}
    cols = rng.permutation(P)[:100]
    coded_listed = [f for f in listed if f >= first]
    for i, c in enumerate(cols):
        f = listed[i % len(listed)]
        w = rows[f].view(np.uint16)
        if f >= first and truth[f, c] == 65536:
            continue
        if i % 10 == 3 and f >= first:                        # a spurious mark
            j = f - first
            oor[j, cnt[j]] = c
            cnt[j] += 1
            oor[j, :cnt[j]] = np.sort(oor[j, :cnt[j]])
        else:
            w[c] ^= 0x0101
        bad[f] = bad.get(f, 0) + 1
    dropped = 0
    for f in coded_listed:                                    # dropped marks
        j = f - first
        if clean_cnt[j] and dropped < 3 and clean_oor[j, 0] not in cols:
            c = int(clean_oor[j, 0])
            lst = [int(x) for x in oor[j, :cnt[j]] if x != c]
            assert len(lst) == cnt[j] - 1
            cnt[j] -= 1
            oor[j, :cnt[j]] = lst
            rows[f].view(np.uint16)[c] = 77 if dropped else 0
            bad[f] = bad.get(f, 0) + 1
            dropped += 1
    assert dropped == 3 and sum(bad.values()) > 66
    for f, nb in bad.items():
        exp[f] = nb
    res = fec.locate_blocks(*args(), oor, cnt, miss)
    assert res.tolist() == exp.tolist()
    # an unlisted fragment's corruption is not seen; a missing one is not read
    res, patched = fec.locate_blocks(*args(), oor, cnt, miss, correct=True)
    assert patched and res.tolist() == exp.tolist()
    for f in present:
        assert (rows[f] == clean_rows[f]).all(), f
    assert (cnt == clean_cnt).all()
    for j in range(len(cnt)):
        assert (oor[j, :cnt[j]] == clean_oor[j, :cnt[j]]).all(), j
    ver = fec.verify_blocks(*args(), oor, cnt, miss)
    checked = present[k:]
    for f in range(k + m):
        assert ver[f].tolist() == ([0, 0, 0xFFFFFFFF] if f in checked else [-1, -1, -1]), f
    # clean again: nothing to patch
    res, patched = fec.locate_blocks(*args(), oor, cnt, miss, correct=True)
    assert not patched and res[-1] == 0 and res[listed].sum() == 0

    # two bad fragments in one column (R = 8): unlocated, and nothing patched
    c = next(int(x) for x in cols
             if truth[listed[0], x] != 65536 and truth[listed[5], x] != 65536)
    rows[listed[0]].view(np.uint16)[c] ^= 1
    rows[listed[5]].view(np.uint16)[c] ^= 1
    snap = [r.copy() for r in rows]
    res, patched = fec.locate_blocks(*args(), oor, cnt, miss, correct=True)
    assert not patched and res[-1] == 1 and res[listed].sum() == 0
    assert all((a == b).all() for a, b in zip(rows, snap))
    rows[listed[0]].view(np.uint16)[c] ^= 1
    rows[listed[5]].view(np.uint16)[c] ^= 1

    # fewer than k + 2 present: nothing to locate with
    miss2 = np.ones(k + m, np.int32)
    miss2[present[:k + 1]] = 0
    miss, keep_miss = miss2, miss
    assert fec.locate_blocks(*args(), oor, cnt, miss) is None
    miss = keep_miss
    fec.close()


def test_fec_locate_blocks_mark_capacity():
    """A fix that needs a mark in a list already at oor_cap: -1 and nothing
    patched; with room for it the list is restored."""
    import quadiron_amd as qa
    _torch()
    k, m, sys_ = 3, 3, 0
    P = 512
    rng = np.random.default_rng(77)
    truth, rows, oor, cnt = _host_fragments(k, m, sys_, P, rng, n_marks=24)
    cmax = int(cnt.max())
    clean_rows = [r.copy() for r in rows]
    full = [int(j) for j in np.nonzero(cnt == cmax)[0]]
    cols = [int(oor[j, 0]) for j in full]
    assert cmax >= 2 and len(set(cols)) == len(cols)
    # every fullest row loses its first mark; the stored word stays 0
    d_oor, d_cnt = oor.copy(), cnt.copy()
    for j in full:
        d_oor[j, :cmax - 1] = oor[j, 1:cmax]
        d_oor[j, cmax - 1] = 0
        d_cnt[j] -= 1
    miss = np.zeros(k + m, np.int32)
    fec = qa.Fec(k, m, False)
    tight = np.ascontiguousarray(d_oor[:, :cmax - 1])
    tight_cnt = d_cnt.copy()
    keep = tight.copy()
    with pytest.raises(RuntimeError):
        fec.locate_blocks(None, rows, tight, tight_cnt, miss, correct=True)
    assert (tight == keep).all() and (tight_cnt == d_cnt).all()
    assert all((a == b).all() for a, b in zip(rows, clean_rows))
    res = fec.locate_blocks(None, rows, tight, tight_cnt, miss)     # locating alone is fine
    assert res[-1] == 0 and [int(res[j]) for j in full] == [1] * len(full)
    res, patched = fec.locate_blocks(None, rows, d_oor, d_cnt, miss, correct=True)
    assert patched and (d_cnt == cnt).all()
    for j in range(k + m):
        assert (d_oor[j, :cnt[j]] == oor[j, :cnt[j]]).all(), j
    assert all((a == b).all() for a, b in zip(rows, clean_rows))
    fec.close()


def test_fec_locate_blocks_unsupported():
    import quadiron_amd as qa
    _torch()
    fec = qa.Fec(300, 212, False)
    rows = [np.zeros(64, np.uint8) for _ in range(512)]
    oor = np.zeros((512, 4), np.uint32)
    cnt = np.zeros(512, np.uint32)
    with pytest.raises(ValueError):
        fec.locate_blocks(None, rows, oor, cnt, np.zeros(512, np.int32))
    fec.close()
