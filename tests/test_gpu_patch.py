"""GPU: the device patch (qi_gpu_patch, Plan.patch) against a NumPy model of
its rule written here (include/qi_gpu.h, "Device patch"): the expected rows,
buckets, status and applied count never come from the code under test.
Buckets are compared as sets with count == len(set); everything a fix does not
name is compared byte for byte.  S = 3 stripes throughout.
  model      hand-made random lists with all four mark transitions, both
             modes, both code types, d_stripes a permutation with one stripe
             not listed, d_mine masks, a dense bucket, idempotence;
  refusals   each of the codes 2 .. 6 on one stripe between two healthy ones,
             precedence, the oor_cap boundary, a bucket over its capacity;
  null       NULL counts; arguments out of range;
  limit      a stripe whose count is above QI_PATCH_MAX_FIXES is refused as
             truncated whatever fix_cap, its neighbours are patched;
  end to end the lists that the project's own locate kernels produce, on the
             oracle's encodes (_truth of test_gpu_syndrome.py): locate_multi ->
             patch -> decode in absolute mode at (3, 5), (16, 48, systematic)
             and (200, 56, unaligned rows); syndrome -> syndrome_locate ->
             patch -> decode in delta mode at k = 300, 1100 and 260
             (systematic), then two holders with complementary d_mine.  R = 4,
             t = 2; the damage (a changed word, a dropped mark, a spurious
             mark over a garbage word; at most two bad listed fragments per
             column) is asserted from the truth before any device call, and
             the expected state is the truth itself.  _truth holds two
             stripes: the third list position is stripe 0 once more, under
             other ids and other damage."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = 65537
S, K, M, P = 3, 16, 48, 2057
ABS, DELTA = 0, 1
NONE, DONE, UNLOCATED, TRUNCATED, BAD_FIX, DATA_MARK, BUCKET_FULL = range(7)
GUARD = 0x5A5A5A5A


class State:
    """Host image of a batch: rows and unordered buckets by stripe."""

    def __init__(self, sys_, n_out, cap, rng, marks=6):
        self.sys, self.n_out, self.cap = sys_, n_out, cap
        self.data = rng.integers(0, 65536, (S, K, P)).astype(np.uint16) if sys_ else None
        self.coded = rng.integers(0, 65536, (S, n_out, P)).astype(np.uint16)
        self.buckets = [[list(rng.choice(P, min(marks, cap), replace=False))
                         for _ in range(n_out)] for _ in range(S)]
        for s in range(S):
            for j in range(n_out):
                self.coded[s, j, self.buckets[s][j]] = 0

    def copy(self):
        import copy
        return copy.deepcopy(self)

    def row(self, st, fid):
        if self.sys and fid < K:
            return self.data[st, fid], None
        j = fid - K if self.sys else fid
        return self.coded[st, j], self.buckets[st][j]


def model(mode, state, st, ids, mine, fixes, words=P, has_counts=True, regions=(True, True)):
    """The rule, for one stripe: (status, applied); edits `state` when DONE."""
    code, todo, seen_cols = 7, [], {}
    grow = {}
    for col, p, w in fixes:
        if p >= len(ids):
            code = min(code, BAD_FIX)
            continue
        if mine is not None and not mine[p]:
            continue
        fid = int(ids[p])
        is_data = state.sys and fid < K
        ok_w = 1 <= w <= 65536 if mode == DELTA else w <= 65536
        if col >= words or not ok_w or fid >= K + M or not regions[0 if is_data else 1]:
            code = min(code, BAD_FIX)
            continue
        row, bucket = state.row(st, fid)
        if bucket is not None and has_counts and len(bucket) > state.cap:
            code = min(code, BAD_FIX)
            continue
        present = bucket is not None and has_counts and col in bucket
        y = 65536 if present else int(row[col])
        v = (y - w) % Q if mode == DELTA else w
        if is_data:
            if v == 65536:
                code = min(code, DATA_MARK)
        else:
            grow[fid] = grow.get(fid, 0) + (v == 65536 and not present) - (v != 65536 and present)
        todo.append((col, fid, v, present))
    if code == 7:
        for fid, g in grow.items():
            if len(state.row(st, fid)[1] if has_counts else []) + g > (state.cap if has_counts
                                                                        else 0):
                code = BUCKET_FULL
    if code != 7:
        return code, 0
    if not todo:
        return NONE, 0
    for col, fid, v, present in todo:
        row, bucket = state.row(st, fid)
        row[col] = v & 0xffff
        if bucket is not None and has_counts:
            if v == 65536 and not present:
                bucket.append(col)
            elif v != 65536 and present:
                bucket.remove(col)
    return DONE, len(todo)


class Dev:
    """The batch on the device, a guard word behind the last bucket."""

    def __init__(self, torch, state):
        self.torch, self.n_out, self.cap = torch, state.n_out, state.cap
        dev = "cuda"
        self.coded = torch.from_numpy(state.coded.view(np.int16).copy()).to(dev)
        self.data = (torch.from_numpy(state.data.view(np.int16).copy()).to(dev)
                     if state.data is not None else None)
        cnt = np.zeros(S * state.n_out, np.int32)
        ent = np.full(S * state.n_out * max(state.cap, 1) + 8, GUARD, np.uint32)
        for s in range(S):
            for j in range(state.n_out):
                b = state.buckets[s][j]
                cnt[s * state.n_out + j] = len(b)
                n = min(len(b), state.cap)
                o = (s * state.n_out + j) * state.cap
                ent[o:o + n] = b[:n]
        self.ent0 = ent.copy()
        self.counts = torch.from_numpy(cnt).to(dev)
        self.entries = torch.from_numpy(ent.view(np.int32)).to(dev)

    def check(self, state, touched=()):
        """Rows byte for byte; buckets as sets with exact counts; the entries
        of a bucket that is not in `touched` (stripe, slot) byte for byte."""
        assert np.array_equal(self.coded.cpu().numpy().view(np.uint16), state.coded)
        if state.data is not None:
            assert np.array_equal(self.data.cpu().numpy().view(np.uint16), state.data)
        cnt = self.counts.cpu().numpy()
        ent = self.entries.cpu().numpy().view(np.uint32)
        assert (ent[-8:] == GUARD).all()
        for s in range(S):
            for j in range(self.n_out):
                o = (s * self.n_out + j) * self.cap
                b = state.buckets[s][j]
                assert cnt[s * self.n_out + j] == len(b), (s, j)
                if (s, j) in touched:
                    got = ent[o:o + min(len(b), self.cap)]
                    assert len(set(got.tolist())) == len(got) and set(got.tolist()) == set(b), (s, j)
                else:
                    assert np.array_equal(ent[o:o + self.cap], self.ent0[o:o + self.cap]), (s, j)


def _call(torch, plan, mode, dev, ids, lists, fix_cap, mine=None, stripes=None, unlocated=None,
          counts_override=None, null_counts=False, data=True, coded=True):
    """lists: per list position the fix triples.  Returns status, applied, err."""
    L = len(lists)
    fc = np.array([len(x) if c is None else c
                   for x, c in zip(lists, counts_override or [None] * L)], np.int32)
    fx = np.zeros((L, max(fix_cap, 1), 3), np.uint32)
    for s, x in enumerate(lists):
        n = min(len(x), fix_cap)
        if n:
            fx[s, :n] = np.array(x[:n], np.uint32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    status = torch.full((L,), -1, dtype=torch.int32, device="cuda")
    applied = torch.full((L,), -1, dtype=torch.int32, device="cuda")
    N = ids.shape[1]
    work = torch.full((plan.patch_work_bytes(N, L),), 0xA5, dtype=torch.uint8, device="cuda")
    err = plan.patch(mode, t(ids.astype(np.int16)), t(fc), t(fx.view(np.int32)), fix_cap,
                     dev.coded if coded else None, status, applied, work,
                     data=dev.data if data else None,
                     mine=t(mine.astype(np.uint8)) if mine is not None else None,
                     stripes=t(np.asarray(stripes, np.int32)) if stripes is not None else None,
                     unlocated=t(np.asarray(unlocated, np.int32)) if unlocated is not None else None,
                     counts=None if null_counts else dev.counts,
                     entries=None if null_counts else dev.entries,
                     cap=0 if null_counts else dev.cap)
    torch.cuda.synchronize()
    return status.cpu().numpy(), applied.cpu().numpy(), err


def _ids(rng, N, sys_):
    return np.stack([rng.permutation(K + M)[:N] for _ in range(S)]).astype(np.int64)


def _random_list(rng, mode, state, st, ids, n, per_row=None):
    """n fixes on distinct (position, column) pairs of stripe st, all four
    transitions on coded rows, never 65536 on a data row."""
    out, named = [], set()
    while len(out) < n:
        p = int(rng.integers(len(ids))) if per_row is None else per_row
        fid = int(ids[p])
        row, bucket = state.row(st, fid)
        col = int(rng.choice(bucket)) if bucket and rng.random() < 0.5 else int(rng.integers(P))
        if (p, col) in named:
            continue
        named.add((p, col))
        y = 65536 if bucket is not None and col in bucket else int(row[col])
        v = 65536 if bucket is not None and rng.random() < 0.4 else int(rng.integers(65536))
        if mode == DELTA and v == y:
            v = (v + 1) % 65536
        out.append((col, p, v if mode == ABS else (y - v) % Q))
    return out


def _touched(state, st, ids, fixes, mine=None):
    return {(st, (int(ids[p]) - K if state.sys else int(ids[p]))) for _, p, _ in fixes
            if (mine is None or mine[p]) and not (state.sys and ids[p] < K)}


@pytest.mark.parametrize("sys_", [0, 1])
@pytest.mark.parametrize("mode", [ABS, DELTA])
def test_model_random_lists(hip_lib, mode, sys_):
    import torch
    import quadiron_amd as qa
    rng = np.random.default_rng(100 + 2 * mode + sys_)
    plan = qa.Plan(K, M, bool(sys_))
    state = State(sys_, plan.n_outputs, 40, rng)
    dev = Dev(torch, state)
    N = K + 4
    ids = _ids(rng, N, sys_)[:2]
    stripes = [2, 0]                      # stripe 1 is not listed
    mine = (rng.random((2, N)) < 0.7) if mode == DELTA else None
    lists = [_random_list(rng, mode, state, stripes[s], ids[s], 300) for s in range(2)]
    exp, touched = [], set()
    kinds = set()
    for s in range(2):
        before = state.copy()
        exp.append(model(mode, state, stripes[s], ids[s], None if mine is None else mine[s],
                         lists[s]))
        touched |= _touched(state, stripes[s], ids[s], lists[s], None if mine is None else mine[s])
        for col, p, _ in lists[s]:
            b0, b1 = before.row(stripes[s], ids[s][p])[1], state.row(stripes[s], ids[s][p])[1]
            if b0 is not None and (mine is None or mine[s][p]):
                kinds.add((col in b0, col in b1))
    # mark->mark, mark->value, value->mark, value->value (a delta never keeps a mark: e != 0)
    assert len(kinds) == (4 if mode == ABS else 3), kinds
    assert all(e[0] == DONE for e in exp)
    st_, ap, err = _call(torch, plan, mode, dev, ids, lists, 320, mine=mine, stripes=stripes)
    assert err == 0
    assert st_.tolist() == [e[0] for e in exp] and ap.tolist() == [e[1] for e in exp]
    dev.check(state, touched)
    if mode == ABS:                        # idempotent: the same list once more
        st_, ap, err = _call(torch, plan, mode, dev, ids, lists, 320, stripes=stripes)
        assert st_.tolist() == [DONE, DONE] and ap.tolist() == [e[1] for e in exp]
        dev.check(state, touched)
    plan.close()


@pytest.mark.parametrize("mode", [ABS, DELTA])
def test_dense_bucket(hip_lib, mode):
    """1500 marks in one bucket of capacity P, 1000 fixes on that row."""
    import torch
    import quadiron_amd as qa
    rng = np.random.default_rng(7 + mode)
    plan = qa.Plan(K, M, False)
    state = State(0, plan.n_outputs, P, rng)
    ids = _ids(rng, K + 4, 0)
    for s in range(S):
        j = int(ids[s][3])
        state.buckets[s][j] = list(rng.choice(P, 1500, replace=False))
        state.coded[s, j, state.buckets[s][j]] = 0
    dev = Dev(torch, state)
    lists = [_random_list(rng, mode, state, s, ids[s], 1000, per_row=3) for s in range(S)]
    exp = [model(mode, state, s, ids[s], None, lists[s]) for s in range(S)]
    assert all(e == (DONE, 1000) for e in exp)
    st_, ap, err = _call(torch, plan, mode, dev, ids, lists, 1000)
    assert err == 0 and st_.tolist() == [DONE] * S and ap.tolist() == [1000] * S
    dev.check(state, {(s, int(ids[s][3])) for s in range(S)})
    plan.close()


def _refusal_case(torch, rng, sys_, mode, make_bad, expect, cap=40, marks=6, err_bit=0, **kw):
    """Stripe 1 offends, 0 and 2 are healthy: 1 is untouched, 0 and 2 patched."""
    import quadiron_amd as qa
    plan = qa.Plan(K, M, bool(sys_))
    state = State(sys_, plan.n_outputs, cap, rng, marks)
    ids = _ids(rng, K + 4, sys_)
    if sys_:
        ids[1][0] = 2                        # a data row at position 0
        ids[1][1:] = K + rng.permutation(M)[:K + 3]
    lists = [_random_list(rng, mode, state, s, ids[s], 20) for s in range(S)]
    extra = make_bad(state, ids[1], lists[1]) or {}
    dev = Dev(torch, state)
    touched = set()
    for s in (0, 2):
        assert model(mode, state, s, ids[s], None, lists[s])[0] == DONE
        touched |= _touched(state, s, ids[s], lists[s])
    args = dict(kw)
    args.update(extra)
    st_, ap, err = _call(torch, plan, mode, dev, ids, lists, args.pop("fix_cap", 64), **args)
    assert st_.tolist() == [DONE, expect, DONE], st_
    assert ap.tolist() == [20, 0, 20]
    assert err & 1 == err_bit
    dev.check(state, touched)
    plan.close()


def _coded_pos(state, ids):
    return next(p for p in range(len(ids)) if not (state.sys and ids[p] < K))


def _free_col(state, st, fid, lst):
    b = state.row(st, fid)[1]
    return next(c for c in range(P) if c not in b and all(c != f[0] for f in lst))


@pytest.mark.parametrize("mode", [ABS, DELTA])
def test_refused_unlocated(hip_lib, mode):
    import torch
    _refusal_case(torch, np.random.default_rng(1), 0, mode, lambda *a: None, UNLOCATED,
                  unlocated=[0, 3, 0])


def test_refused_truncated_and_precedence(hip_lib):
    import torch
    # the count says 70 where fix_cap is 64; the list also holds a bad fix: 3 wins
    def bad(state, ids, lst):
        lst[5] = (P, lst[5][1], 1)
        return {"counts_override": [None, 70, None]}
    _refusal_case(torch, np.random.default_rng(2), 0, ABS, bad, TRUNCATED)


@pytest.mark.parametrize("what", ["position", "column", "word", "delta0", "id", "region"])
def test_refused_bad_fix(hip_lib, what):
    import torch
    mode = DELTA if what == "delta0" else ABS
    sys_ = 1 if what == "region" else 0

    def bad(state, ids, lst):
        col, p, w = lst[7]
        if what == "position":
            lst[7] = (col, K + 4, w)
        elif what == "column":
            lst[7] = (P, p, w)
        elif what == "word":
            lst[7] = (col, p, 65537)
        elif what == "delta0":
            lst[7] = (col, p, 0)
        elif what == "id":
            ids[p] = K + M
        else:                                  # a fix on the data row, d_data NULL
            lst[:] = [f for f in lst if f[1] != 0]
            lst.insert(0, (5, 0, 1))
            while len(lst) < 20:
                lst.append((_free_col(state, 1, int(ids[1]), lst), 1, 7))
            del lst[20:]
    if what == "region":
        # the healthy neighbours must not name data rows either
        import quadiron_amd as qa
        rng = np.random.default_rng(3)
        plan = qa.Plan(K, M, True)
        state = State(1, plan.n_outputs, 40, rng)
        ids = np.stack([K + rng.permutation(M)[:K + 4] for _ in range(S)]).astype(np.int64)
        ids[1][0] = 2
        lists = [_random_list(rng, ABS, state, s, ids[s], 20) for s in range(S)]
        bad(state, ids[1], lists[1])
        dev = Dev(torch, state)
        touched = set()
        for s in (0, 2):
            assert model(ABS, state, s, ids[s], None, lists[s])[0] == DONE
            touched |= _touched(state, s, ids[s], lists[s])
        st_, ap, err = _call(torch, plan, ABS, dev, ids, lists, 64, data=False)
        assert st_.tolist() == [DONE, BAD_FIX, DONE] and ap.tolist() == [20, 0, 20]
        dev.check(state, touched)
        plan.close()
        return
    _refusal_case(torch, np.random.default_rng(3), sys_, mode, bad, BAD_FIX)


@pytest.mark.parametrize("mode", [ABS, DELTA])
def test_refused_data_mark(hip_lib, mode):
    import torch

    def bad(state, ids, lst):
        lst[:] = [f for f in lst if f[1] != 0]
        y = int(state.data[1, 2, 9])
        lst.insert(0, (9, 0, 65536 if mode == ABS else (y - 65536) % Q))
        while len(lst) < 20:
            lst.append((_free_col(state, 1, int(ids[1]), lst), 1, 7))
        del lst[20:]
    _refusal_case(torch, np.random.default_rng(4), 1, mode, bad, DATA_MARK)


@pytest.mark.parametrize("extra_insert", [0, 1])
def test_bucket_full_boundary(hip_lib, extra_insert):
    """A bucket at oor_cap: one removal and one insertion in the same list is
    DONE (the insertion listed first); one more insertion is refused."""
    import torch
    import quadiron_amd as qa
    rng = np.random.default_rng(5)
    plan = qa.Plan(K, M, False)
    cap = 6
    state = State(0, plan.n_outputs, cap, rng, marks=6)     # every bucket is full
    ids = _ids(rng, K + 4, 0)
    lists = []
    for s in range(S):
        fid = int(ids[s][2])
        b = state.buckets[s][fid]
        free = [c for c in range(P) if c not in b][:2]
        lst = [(free[0], 2, 65536), (int(b[3]), 2, 123)]
        if extra_insert and s == 1:
            lst.append((free[1], 2, 65536))
        lists.append(lst)
    dev = Dev(torch, state)
    exp = [model(ABS, state, s, ids[s], None, lists[s]) for s in range(S)]
    want = [DONE, BUCKET_FULL if extra_insert else DONE, DONE]
    assert [e[0] for e in exp] == want
    st_, ap, err = _call(torch, plan, ABS, dev, ids, lists, 4)
    assert err == 0 and st_.tolist() == want and ap.tolist() == [e[1] for e in exp]
    dev.check(state, {(s, int(ids[s][2])) for s in range(S) if want[s] == DONE})
    plan.close()


def test_bucket_over_capacity_raises_bit_1(hip_lib):
    import torch

    def bad(state, ids, lst):
        fid = int(ids[lst[0][1]])
        state.buckets[1][fid] = list(range(100, 100 + state.cap + 3))
    _refusal_case(torch, np.random.default_rng(6), 0, ABS, bad, BAD_FIX, err_bit=1)


@pytest.mark.parametrize("mode", [ABS, DELTA])
def test_null_counts(hip_lib, mode):
    """No buckets: value fixes are applied, y is the stored word, and a fix to
    65536 on a coded row refuses its stripe with code 6."""
    import torch
    import quadiron_amd as qa
    rng = np.random.default_rng(8 + mode)
    plan = qa.Plan(K, M, False)
    state = State(0, plan.n_outputs, 4, rng, marks=0)
    ids = _ids(rng, K + 4, 0)
    lists = []
    for s in range(S):
        lst = []
        for e in range(30):
            col, p = 3 * e + s, e % (K + 4)
            y = int(state.coded[s, ids[s][p], col])
            v = 65536 if (s == 1 and e == 11) else int(rng.integers(65536))
            if v == y:
                v ^= 1
            lst.append((col, p, v if mode == ABS else (y - v) % Q))
        lists.append(lst)
    dev = Dev(torch, state)
    exp = [model(mode, state, s, ids[s], None, lists[s], has_counts=False) for s in range(S)]
    assert [e[0] for e in exp] == [DONE, BUCKET_FULL, DONE]
    st_, ap, err = _call(torch, plan, mode, dev, ids, lists, 32, null_counts=True)
    assert err == 0 and st_.tolist() == [DONE, BUCKET_FULL, DONE] and ap.tolist() == [30, 0, 30]
    dev.check(state)
    plan.close()


def test_empty_and_skipped_lists_and_fix_cap_0(hip_lib):
    import torch
    import quadiron_amd as qa
    rng = np.random.default_rng(9)
    plan = qa.Plan(K, M, False)
    state = State(0, plan.n_outputs, 8, rng)
    dev = Dev(torch, state)
    ids = _ids(rng, K + 4, 0)
    lists = [[], _random_list(rng, DELTA, state, 1, ids[1], 10), []]
    mine = np.zeros((S, K + 4), bool)
    st_, ap, _ = _call(torch, plan, DELTA, dev, ids, lists, 16, mine=mine)
    assert st_.tolist() == [NONE] * 3 and ap.tolist() == [0] * 3
    st_, ap, _ = _call(torch, plan, DELTA, dev, ids, [[], [], []], 0,
                       counts_override=[0, 4, 0])
    assert st_.tolist() == [NONE, TRUNCATED, NONE] and ap.tolist() == [0] * 3
    dev.check(state)
    plan.close()


def test_arguments_out_of_range(hip_lib):
    """-1, no work bytes, no kernel names, nothing written."""
    import torch
    import quadiron_amd as qa
    lib = qa.lib()
    plan = qa.Plan(K, M, False)
    assert plan.patch_kernels(K + 4, ABS, P) == "patch=patch_kernel"
    assert plan.patch_work_bytes(K + 4, S) > 0
    for n in (0, K + M + 1):
        assert plan.patch_work_bytes(n, S) == 0 and plan.patch_kernels(n, ABS, P) == ""
    assert plan.patch_work_bytes(K + 4, 0) == 0
    assert plan.patch_kernels(K + 4, 2, P) == "" and plan.patch_kernels(K + 4, ABS, 0) == ""
    assert plan.patch_kernels(K + 4, ABS, (1 << 32) + 1) == ""
    rng = np.random.default_rng(10)
    state = State(0, plan.n_outputs, 8, rng)
    dev = Dev(torch, state)
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    status = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    ids = torch.zeros(S * (K + 4), dtype=torch.int16, device="cuda")

    def rc(mode=ABS, n=K + 4, fix_cap=1, words=P, n_stripes=S, h=plan.h):
        return lib.qi_gpu_patch(h, mode, ids.data_ptr(), n, None, None, None, z.data_ptr(),
                                z.data_ptr(), fix_cap, None, 0, 0, dev.coded.data_ptr(),
                                dev.coded.stride(0), dev.coded.stride(1), dev.counts.data_ptr(),
                                dev.entries.data_ptr(), dev.cap, z.data_ptr(), status.data_ptr(),
                                status.data_ptr(), words, n_stripes, None)
    assert rc(h=None) == -1 and rc(mode=2) == -1 and rc(mode=-1) == -1
    assert rc(n=0) == -1 and rc(n=K + M + 1) == -1 and rc(fix_cap=-1) == -1
    assert rc(words=0) == -1 and rc(words=(1 << 32) + 1) == -1 and rc(n_stripes=0) == -1
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [-1] * S
    dev.check(state)
    plan.close()


# ---- end to end: lists that the project's own locate kernels produce ---------
# The stripes are the oracle's encodes (_truth of test_gpu_syndrome.py, two
# stripes; the third list position is stripe 0 again under other ids and other
# damage).  Everything expected is the truth itself.

import functools

E2E_R, E2E_T = 4, 2
MARK = 65536


@functools.lru_cache(maxsize=None)
def _truth3(k, m, sys_, P):
    from test_gpu_syndrome import _truth
    t = _truth(k, m, sys_, P)
    t3 = np.concatenate([t, t[:1]])
    t3.setflags(write=False)
    return t3


@functools.lru_cache(maxsize=None)
def _truth_data(k, m, sys_, P):
    """The data rows behind _truth: its generator replayed (the oracle's encode
    draws nothing from it)."""
    from qi_testlib import craft_oor_columns
    rng = np.random.default_rng([k, m, sys_, P, 11])
    out = []
    for _ in range(2):
        data = rng.integers(0, 65536, (k, P), dtype=np.uint16)
        craft_oor_columns(k, m, sys_, data, rng, 24)
        out.append(data.copy())
    d = np.stack(out + out[:1])
    if sys_:
        assert (d == _truth3(k, m, sys_, P)[:, :k]).all()
    return d


def _e2e_ids(truth, k, m, sys_, rng):
    """[S, k + R] listed ids, different per stripe; up to four coded fragments
    that carry marks are always among them."""
    first = k if sys_ else 0
    ids = []
    for s in range(S):
        marked = [f for f in range(first, k + m) if (truth[s, f] == MARK).any()]
        keep = [int(f) for f in rng.permutation(marked)[:4]]
        rest = [int(f) for f in rng.permutation(k + m) if f not in keep][:k + E2E_R - len(keep)]
        ids.append(rng.permutation(keep + rest))
    return np.stack(ids).astype(np.uint16)


def _e2e_damage(truth, ids, k, sys_, rng):
    """(recv restored symbols, garbage [(s, slot, col, word)], forms {a, b, c})
    with at most two bad listed fragments per column:
      a  the stored word changed at an unmarked column;
      b  a mark dropped from a coded row's bucket (the word is the 0 it was);
      c  a spurious mark at an unmarked column, the word under it garbage."""
    first = k if sys_ else 0
    P = truth.shape[2]
    recv = truth.copy()
    garbage = []
    forms = {"a": 0, "b": 0, "c": 0}
    N = ids.shape[1]

    def form_a(s, c, avoid=-1):
        p = next(int(p) for p in rng.permutation(N)
                 if p != avoid and truth[s, ids[s, p], c] != MARK)
        f = int(ids[s, p])
        recv[s, f, c] = (int(truth[s, f, c]) + int(rng.integers(1, 65536))) % 65536
        forms["a"] += 1

    for s in range(S):
        used = set()
        marks = [(int(p), int(c)) for p in range(N) if ids[s, p] >= first
                 for c in np.flatnonzero(truth[s, ids[s, p]] == MARK)]
        i = 0
        for p, c in (marks[j] for j in rng.permutation(len(marks))):
            if c in used or i == 3:
                continue
            used.add(c)
            recv[s, ids[s, p], c] = 0                     # b
            forms["b"] += 1
            if i == 0:
                form_a(s, c, avoid=p)
            i += 1
        free = [int(c) for c in [0, P - 1] + list(rng.permutation(P)) if c not in used]
        free = list(dict.fromkeys(free))
        for i, c in enumerate(free[:6]):                  # a, one or two fragments
            form_a(s, c)
            if i % 2:
                bad = int(np.flatnonzero(recv[s][ids[s], c] != truth[s][ids[s], c])[0])
                form_a(s, c, avoid=bad)
        for i, c in enumerate(free[6:9]):                 # c
            p = next(int(p) for p in rng.permutation(N)
                     if ids[s, p] >= first and truth[s, ids[s, p], c] != MARK)
            f = int(ids[s, p])
            recv[s, f, c] = MARK
            garbage.append((s, f - first, c, int(rng.integers(0, 65536))))
            forms["c"] += 1
            if i == 0:
                form_a(s, c, avoid=p)
    return recv, garbage, forms


class _Batch:
    """A batch on the device by fragment id, rows inside guard words."""

    def __init__(self, torch, plan, k, sys_, recv, garbage, unaligned):
        from test_gpu_locate import _store
        from test_gpu_partial import _buckets, _rows_dev
        from test_gpu_syndrome import CAP
        data, coded, marks = _store(k, sys_, recv, garbage)
        assert coded.shape[1] == plan.n_outputs
        self.torch, self.cap, self.n_out = torch, CAP, plan.n_outputs
        self.dbig, self.data = _rows_dev(torch, data, unaligned) if sys_ else (None, None)
        self.cbig, self.coded = _rows_dev(torch, coded, unaligned)
        self.counts, self.entries = _buckets(torch, [[c[::-1] for c in ms] for ms in marks],
                                             CAP)

    def rows(self):
        d = self.data.cpu().numpy().view(np.uint16) if self.data is not None else None
        return d, self.coded.cpu().numpy().view(np.uint16)

    def check_is(self, k, sys_, want, garbage=()):
        """rows, buckets (as sets, exact counts) and guards against the
        restored symbols `want` (garbage: words still stored under a mark)"""
        from test_gpu_locate import _store
        from test_gpu_partial import _guards_intact, _read_buckets
        data, coded, marks = _store(k, sys_, want, garbage)
        d, c = self.rows()
        assert (c == coded).all()
        assert _guards_intact(self.cbig, self.coded)
        if sys_:
            assert (d == data).all() and _guards_intact(self.dbig, self.data)
        cnt, sets = _read_buckets(self.counts, self.entries, S, self.n_out, self.cap)
        for s in range(S):
            for j in range(self.n_out):
                assert cnt[s, j] == len(sets[s][j]) == len(marks[s][j]), (s, j)
                assert sets[s][j] == set(int(v) for v in marks[s][j]), (s, j)

    def patch(self, plan, mode, ids, unloc, fcnt, fixes, mine=None):
        torch = self.torch
        t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).cuda()
        fix_cap = fixes.shape[1]
        status = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        applied = torch.full((S,), -1, dtype=torch.int32, device="cuda")
        work = torch.full((plan.patch_work_bytes(ids.shape[1], S),), 0xA5, dtype=torch.uint8,
                          device="cuda")
        err = plan.patch(mode, torch.from_numpy(ids.view(np.int16)).cuda(), t32(fcnt),
                         t32(fixes), fix_cap, self.coded, status, applied, work, data=self.data,
                         mine=(torch.from_numpy(mine.astype(np.uint8)).cuda()
                               if mine is not None else None),
                         unlocated=t32(unloc), counts=self.counts, entries=self.entries,
                         cap=self.cap)
        torch.cuda.synchronize()
        assert err == 0
        return status.cpu().numpy(), applied.cpu().numpy()

    def decode(self, plan, ids_k):
        """the data from the fragments ids_k [S, k], with a fresh context"""
        from test_gpu_partial import _dev16, _guards_intact, _rows_dev
        torch = self.torch
        P = self.coded.shape[2]
        ctx = torch.zeros(plan.ctx_bytes(S, P), dtype=torch.uint8, device="cuda")
        d_ids = _dev16(torch, ids_k)
        plan.decode_ctx(d_ids, ctx, P, counts=self.counts, entries=self.entries, cap=self.cap)
        obig, out = _rows_dev(torch, np.zeros((S, plan.k, P), np.uint16))
        assert plan.decode(ctx, d_ids, self.coded, out, data=self.data, counts=self.counts,
                           entries=self.entries, cap=self.cap) == 0
        assert _guards_intact(obig, out)
        return out.cpu().numpy().view(np.uint16)


def _e2e_case(k, m, sys_, P, seed):
    """truth, ids, damage and the number of bad (fragment, column) pairs per
    stripe, with the issue's conditions asserted from the truth alone"""
    truth = _truth3(k, m, sys_, P)
    rng = np.random.default_rng([k, m, sys_, seed])
    ids = _e2e_ids(truth, k, m, sys_, rng)
    recv, garbage, forms = _e2e_damage(truth, ids, k, sys_, rng)
    assert min(forms.values()) >= 4, forms
    bad = np.stack([recv[s][ids[s]] != truth[s][ids[s]] for s in range(S)])
    assert bad.sum(axis=1).max() <= 2
    listed = np.zeros(truth.shape[:2], bool)
    for s in range(S):
        listed[s, ids[s]] = True
    assert ((recv != truth).any(axis=2) <= listed).all()   # only listed fragments are damaged
    return truth, ids, recv, garbage, bad.sum(axis=(1, 2))


@pytest.mark.parametrize("k,m,sys_,P,unaligned", [(3, 5, 0, 2057, False), (16, 48, 1, 2048, False),
                                                  (200, 56, 0, 2057, True)])
def test_end_to_end_absolute(hip_lib, k, m, sys_, P, unaligned):
    """locate_multi -> patch -> decode."""
    import torch
    import quadiron_amd as qa
    from test_gpu_locate_multi import _locate_multi
    truth, ids, recv, garbage, n_bad = _e2e_case(k, m, sys_, P, 1)
    err, _, unloc, _, fcnt, fixes = _locate_multi(k, m, sys_, E2E_R, E2E_T, ids, recv,
                                                  unaligned=unaligned, garbage=garbage)
    assert err == 0
    plan = qa.Plan(k, m, bool(sys_))
    b = _Batch(torch, plan, k, sys_, recv, garbage, unaligned)
    status, applied = b.patch(plan, ABS, ids, unloc, fcnt, fixes)
    assert status.tolist() == [DONE] * S
    assert applied.tolist() == n_bad.tolist()
    b.check_is(k, sys_, truth)      # every fragment, listed or not, and its bucket
    got = b.decode(plan, ids[:, :k])
    assert (got == _truth_data(k, m, sys_, P)).all()
    plan.close()


@pytest.mark.parametrize("k,m,sys_,P", [(300, 212, 0, 2057), (1100, 100, 0, 2057),
                                        (260, 30, 1, 2048)])
def test_end_to_end_delta(hip_lib, k, m, sys_, P):
    """syndrome (H = N) -> syndrome_locate -> patch(DELTA) -> decode, then the
    same lists applied by two holders with complementary d_mine."""
    import torch
    import quadiron_amd as qa
    from test_gpu_syndrome import _all_held, _resolve, _share
    truth, ids, recv, garbage, n_bad = _e2e_case(k, m, sys_, P, 2)
    plan = qa.Plan(k, m, bool(sys_))
    syn, sets = _share(torch, plan, ids, _all_held(ids), recv)
    _, unloc, _, fcnt, fixes = _resolve(torch, plan, ids, syn, sets, E2E_T)
    b = _Batch(torch, plan, k, sys_, recv, garbage, False)
    status, applied = b.patch(plan, DELTA, ids, unloc, fcnt, fixes)
    assert status.tolist() == [DONE] * S
    assert applied.tolist() == n_bad.tolist()
    b.check_is(k, sys_, truth)
    assert (b.decode(plan, ids[:, :k]) == _truth_data(k, m, sys_, P)).all()

    # two holders
    rng = np.random.default_rng([k, 3])
    mine = rng.random(ids.shape) < 0.5
    b = _Batch(torch, plan, k, sys_, recv, garbage, False)
    st1, ap1 = b.patch(plan, DELTA, ids, unloc, fcnt, fixes, mine=mine)
    # the first holder healed its fragments and touched no other
    half = recv.copy()
    for s in range(S):
        half[s, ids[s][mine[s]]] = truth[s, ids[s][mine[s]]]
    first = k if sys_ else 0
    held = [set(int(f) for f in ids[s][mine[s]]) for s in range(S)]
    b.check_is(k, sys_, half, [g for g in garbage if g[1] + first not in held[g[0]]])
    st2, ap2 = b.patch(plan, DELTA, ids, unloc, fcnt, fixes, mine=~mine)
    assert set(st1.tolist()) | set(st2.tolist()) <= {NONE, DONE}
    assert (ap1 + ap2).tolist() == n_bad.tolist()
    for s in range(S):
        bad = recv[s][ids[s]] != truth[s][ids[s]]
        assert ap1[s] == bad[mine[s]].sum() and ap2[s] == bad[~mine[s]].sum()
    b.check_is(k, sys_, truth)
    plan.close()


def test_list_longer_than_max_fixes_is_truncated(hip_lib):
    """fix_cap, the stride of d_fixes, is not bounded; a stripe whose count is
    above QI_PATCH_MAX_FIXES is refused as truncated and its neighbours are
    patched."""
    import torch
    import quadiron_amd as qa
    rng = np.random.default_rng(11)
    plan = qa.Plan(K, M, False)
    state = State(0, plan.n_outputs, 40, rng)
    ids = _ids(rng, K + 4, 0)
    lists = [_random_list(rng, ABS, state, s, ids[s], 20) for s in range(S)]
    dev = Dev(torch, state)
    touched = set()
    for s in (0, 2):
        assert model(ABS, state, s, ids[s], None, lists[s])[0] == DONE
        touched |= _touched(state, s, ids[s], lists[s])
    big = qa.Plan.PATCH_MAX_FIXES + 1
    st_, ap, err = _call(torch, plan, ABS, dev, ids, lists, big + 7,
                         counts_override=[None, big, None])
    assert err == 0 and st_.tolist() == [DONE, TRUNCATED, DONE] and ap.tolist() == [20, 0, 20]
    dev.check(state, touched)
    plan.close()
