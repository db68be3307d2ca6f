"""GPU: fragment fingerprints (qi_gpu_fingerprint, Fec.fingerprint_blocks,
Fec.check_fingerprints).  Every expected value is NumPy int64 over restored
symbols, straight from the definition (fp_testlib); the rows come from the
product's own encode, whose marks are part of the input."""
import numpy as np
import pytest

from fp_testlib import KEYS8, Q, fingerprints, restored
from qi_testlib import oracle_encode_blocks

pytestmark = pytest.mark.gpu

S = 3
WIDTHS = (1, 9, 2047, 2048, 2049, 4100)
PMAX = 4100
GARBAGE = 0x5A5A


def _torch():
    import torch
    return torch


def _dev_rows(rows, off):
    """(S, R, P) u16 -> a device view at element offset `off`: off 0 with
    strides that are multiples of 8 words (the 16-byte form), otherwise odd
    row and stripe strides (the scalar form)."""
    torch = _torch()
    Sx, R, P = rows.shape
    rs = (P + 7) // 8 * 8 + (0 if off == 0 else 3)
    ss = R * rs + (0 if off == 0 else 5)
    backing = torch.full((off + Sx * ss + 8,), GARBAGE, dtype=torch.int16, device="cuda")
    view = torch.as_strided(backing, (Sx, R, P), (ss, rs, 1), off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(rows).view(np.int16)))
    assert (view.data_ptr() % 16 == 0) == (off == 0)
    return backing, view


def _i32(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def _buckets(mask, cap, extra=None):
    """(S, slots, P) bool -> counts (S, slots), entries (S, slots, cap) u32 in
    descending order (buckets are unordered); extra[(s, j)]: further entries"""
    Sx, no, _ = mask.shape
    cnt = np.zeros((Sx, no), np.uint32)
    ent = np.full((Sx, no, cap), 0xFFFFFFFF, np.uint32)
    for s in range(Sx):
        for j in range(no):
            c = list(np.flatnonzero(mask[s, j])[::-1]) + list((extra or {}).get((s, j), []))
            assert len(c) <= cap
            cnt[s, j] = len(c)
            ent[s, j, :len(c)] = c
    return cnt, ent


class Stripes:
    """S stripes of RS(k, m) on P columns from the product's encode: data
    (S, k, P) u16, coded (S, n_out, P) u16, mask (S, n_out, P) of its marks"""

    def __init__(self, k, m, sys_, Sx, P, seed):
        import quadiron_amd as qa
        torch = _torch()
        self.k, self.m, self.sys, self.S, self.P = k, m, sys_, Sx, P
        self.plan = qa.Plan(k, m, bool(sys_))
        self.no = no = self.plan.n_outputs
        rng = np.random.default_rng(seed)
        self.data = rng.integers(0, 65536, (Sx, k, P), dtype=np.uint16)
        dd = torch.from_numpy(self.data.view(np.int16)).cuda()
        out = torch.zeros((Sx, no, P), dtype=torch.int16, device="cuda")
        cap = 64
        counts = torch.zeros(Sx * no, dtype=torch.int32, device="cuda")
        entries = torch.zeros(Sx * no * cap, dtype=torch.int32, device="cuda")
        self.plan.encode(dd, out, counts, entries, cap)
        torch.cuda.synchronize()
        self.coded = out.cpu().numpy().view(np.uint16)
        cnt = counts.cpu().numpy().reshape(Sx, no)
        ent = entries.cpu().numpy().reshape(Sx, no, cap)
        assert cnt.max() <= cap
        self.mask = np.zeros((Sx, no, P), bool)
        for s in range(Sx):
            for j in range(no):
                self.mask[s, j, ent[s, j, :cnt[s, j]]] = True

    def symbols(self, mask=None, words=None):
        """(S, k + m, words) int64 restored symbols by fragment id"""
        w = self.P if words is None else words
        y = np.where((self.mask if mask is None else mask)[:, :, :w], 65536,
                     self.coded[:, :, :w].astype(np.int64))
        return np.concatenate([self.data[:, :, :w].astype(np.int64), y], 1) if self.sys else y


class Dev:
    """the stripes on the device at one row offset, with buckets"""

    def __init__(self, st, off, mask=None, cap=None, extra=None, coded=None, data=None):
        mask = st.mask if mask is None else mask
        self.st, self.cap = st, cap or max(64, int(mask.sum(axis=2).max()) + 2)
        cnt, ent = _buckets(mask, self.cap, extra)
        self.cnt, self.ent = _i32(cnt), _i32(ent)
        self.keep, self.dc = _dev_rows(st.coded if coded is None else coded, off)
        self.dd = None
        if st.sys:
            self.keep2, self.dd = _dev_rows(st.data if data is None else data, off)

    def fp(self, ids, keys, words=None, first_col=0, marks=True, err=0):
        """(S, N, F) int64 of the call, after checking the error flags"""
        torch = _torch()
        plan = self.st.plan
        ids = np.ascontiguousarray(ids, np.uint16)
        Sx, N = ids.shape
        F = len(keys)
        w = self.st.P if words is None else words
        out = torch.full((Sx, N, F), 7, dtype=torch.int32, device="cuda")
        work = torch.randint(0, 256, (plan.fingerprint_work_bytes(N, F, Sx, w),),
                             dtype=torch.uint8, device="cuda")
        got = plan.fingerprint(torch.from_numpy(ids.view(np.int16)).cuda(), keys, out, work,
                               coded=self.dc, data=self.dd,
                               counts=self.cnt if marks else None,
                               entries=self.ent if marks else None,
                               cap=self.cap if marks else 0, first_col=first_col, words=w)
        torch.cuda.synchronize()
        assert got == err, got
        return out.cpu().numpy().view(np.uint32).astype(np.int64)


def _id_sets(k, m, rng):
    n = k + m
    a, b = int(rng.integers(0, n)), int(rng.integers(0, n))
    return [np.array([[n - 1]] * S), np.stack([rng.permutation(n) for _ in range(S)]),
            np.array([[a, b, a]] * S)]


def _expect(y, ids, keys, first_col=0):
    """y (S, n, words) -> (S, N, F)"""
    full = fingerprints(y, keys, first_col)                 # (S, n, F)
    return np.stack([full[s, ids[s]] for s in range(len(ids))])


@pytest.mark.parametrize("k,m,sys_", [(3, 3, 0), (10, 6, 1), (16, 48, 0), (300, 20, 0)])
def test_values_vs_numpy(k, m, sys_):
    """item 1: every width, row offsets 0 / 1 / 3, N = 1, all fragments
    shuffled and a repeated id, F in 1, 2, 3, 4, 8; marks from the encode and
    forged buckets (column 0, the last column, every column, a column >=
    words)"""
    st = Stripes(k, m, sys_, S, PMAX, 100 * k + m)
    mask = st.mask.copy()
    no = st.no
    mask[1, 0, 0] = True
    mask[1, 1, PMAX - 1] = True
    mask[1, 2, :] = True
    mask[1, no - 1, 5] = True
    extra = {(1, no - 1): [PMAX + 5, 0x7FFFFFFF]}           # no columns: ignored
    rng = np.random.default_rng(k)
    sets = _id_sets(k, m, rng)
    assert st.plan.fingerprint_kernels(k + m, 3, 2048) == (
        "fingerprint=fingerprint_tab_kernel + fingerprint_kernel<4, true>")
    devs = [Dev(st, off, mask, extra=extra) for off in (0, 1, 3)]
    for w in WIDTHS:
        y = st.symbols(mask, w)
        full = fingerprints(y, KEYS8)
        for dev in devs:
            for i, ids in enumerate(sets):
                for F in (1, 2, 3, 4, 8):
                    got = dev.fp(ids, KEYS8[:F], words=w)
                    exp = np.stack([full[s, ids[s], :F] for s in range(S)])
                    assert (got == exp).all(), (w, i, F)
    # without buckets the stored words alone count
    y = np.concatenate([st.data, st.coded], 1) if sys_ else st.coded
    got = devs[0].fp(sets[1], KEYS8[:2], marks=False)
    assert (got == _expect(y.astype(np.int64), sets[1], KEYS8[:2])).all()


@pytest.mark.parametrize("k,m,sys_", [(3, 3, 0), (10, 6, 1), (16, 48, 0), (300, 20, 0)])
def test_one_wide_stripe(k, m, sys_):
    """item 1: one stripe of 65536 + 2048 + 3 columns (C2 steps inside the row)"""
    P = 65536 + 2048 + 3
    st = Stripes(k, m, sys_, 1, P, 7 * k)
    mask = st.mask.copy()
    mask[0, 0, [0, 65535, 65536, P - 1]] = True
    ids = np.random.default_rng(k).permutation(k + m)[None, :]
    exp = _expect(st.symbols(mask), ids, KEYS8[5:8])
    for off in (0, 1):
        assert (Dev(st, off, mask).fp(ids, KEYS8[5:8]) == exp).all(), off


def _chunk_words(plan):
    """the launcher's columns per block, from the work size: the first whole
    number of tiles past which a row needs partial sums (two chunks of one
    key: 8 bytes more; a further d power is 4)"""
    for w in range(2048, 64 * 2048 + 1, 2048):
        if plan.fingerprint_work_bytes(1, 1, 1, w + 1) - plan.fingerprint_work_bytes(
                1, 1, 1, w) >= 8:
            return w
    raise AssertionError("no chunk size found")


def test_slices_add_up_and_rows_of_several_blocks():
    """item 2"""
    k, m = 16, 48
    st = Stripes(k, m, 0, 2, PMAX, 5)
    mask = st.mask.copy()
    mask[0, 3, [0, 1, 2047, 2048, PMAX - 1]] = True
    ids = np.stack([np.random.default_rng(s).permutation(k + m) for s in range(2)])
    keys = KEYS8[4:8]
    dev = Dev(st, 0, mask)
    whole = dev.fp(ids, keys)
    assert (whole == _expect(st.symbols(mask), ids, keys)).all()
    total = np.zeros_like(whole)
    for lo, hi in ((0, 1), (1, 2048), (2048, PMAX)):
        # the slice's own rows and buckets: bucket columns are relative
        sl = Stripes.__new__(Stripes)
        sl.__dict__.update(st.__dict__)
        sl.coded, sl.P = np.ascontiguousarray(st.coded[:, :, lo:hi]), hi - lo
        for off in (0, 1):
            part = Dev(sl, off, mask[:, :, lo:hi]).fp(ids, keys, first_col=lo)
            assert (part == _expect(st.symbols(mask)[:, :, lo:hi], ids, keys, lo)).all()
        total = (total + part) % Q
    assert (total == whole).all()

    ch = _chunk_words(st.plan)
    assert ch % 2048 == 0
    P = 2 * ch + 2048 + 5                                   # three blocks per row
    big = Stripes(k, m, 0, 2, P, 6)
    bm = big.mask.copy()
    bm[1, 5, [0, ch - 1, ch, 2 * ch, P - 1]] = True
    assert big.plan.fingerprint_kernels(k + m, 2, P).endswith(" + fingerprint_finish_kernel")
    for F in (2, 8):
        exp = _expect(big.symbols(bm), ids, KEYS8[:F])
        for off in (0, 1):
            dev = Dev(big, off, bm)
            a = dev.fp(ids, KEYS8[:F])
            assert (a == exp).all(), (F, off)
            assert (dev.fp(ids, KEYS8[:F]) == a).all()      # the same bits again
    # first_col that is no multiple of 8 on aligned rows, across a C2 step
    exp = _expect(big.symbols(bm), ids, KEYS8[:3], 65536 * 5 - 2049)
    assert (Dev(big, 0, bm).fp(ids, KEYS8[:3], first_col=65536 * 5 - 2049) == exp).all()


def test_extremes():
    """item 3: all symbols 0xFFFF; every column marked with key components
    65536 and 32768; F = 8 at width 4096"""
    k, m, P = 16, 48, 4096
    st = Stripes(k, m, 0, 1, P, 9)
    ids = np.arange(k + m)[None, :]
    ones = np.full_like(st.coded, 0xFFFF)
    none = np.zeros_like(st.mask)
    for off in (0, 1):
        got = Dev(st, off, none, coded=ones).fp(ids, KEYS8)
        assert (got == fingerprints(np.full((1, k + m, P), 65535), KEYS8)).all()
        keys = [(65536, 65536, 65536), (32768, 32768, 32768), (65536, 32768, 65536),
                (32769, 65536, 32768)]
        got = Dev(st, off, ~none, cap=P).fp(ids, keys)
        assert (got == fingerprints(np.full((1, k + m, P), 65536), keys)).all()


def _clean_seed(k, m, sys_, Sx, P, keys):
    """a seed, chosen on the CPU, whose data rows' fingerprints hold no 65536"""
    for seed in range(1000, 1100):
        data = np.random.default_rng(seed).integers(0, 65536, (Sx, k, P), dtype=np.uint16)
        if (fingerprints(data, keys) < 65536).all():
            return seed
    raise AssertionError("no seed")


@pytest.mark.parametrize("k,m,sys_", [(16, 48, 0), (10, 6, 1)])
def test_homomorphism_on_the_device(k, m, sys_):
    """item 4: Plan.encode of the data rows' fingerprints, as a stripe of F
    words, is the fingerprints of the encoded fragments, marks included"""
    import quadiron_amd as qa
    torch = _torch()
    P, keys = 4096, KEYS8[4:8]
    F = len(keys)
    seed = _clean_seed(k, m, sys_, S, P, keys)
    st = Stripes(k, m, sys_, S, P, seed)
    # the data rows' fingerprints: rows of a systematic plan of the same shape
    sp = qa.Plan(k, m, True)
    ids = np.tile(np.arange(k, dtype=np.uint16), (S, 1))
    out = torch.zeros((S, k, F), dtype=torch.int32, device="cuda")
    work = torch.zeros(sp.fingerprint_work_bytes(k, F, S, P), dtype=torch.uint8, device="cuda")
    dd = torch.from_numpy(st.data.view(np.int16)).cuda()
    assert sp.fingerprint(torch.from_numpy(ids.view(np.int16)).cuda(), keys, out, work,
                          data=dd) == 0
    h = out.cpu().numpy().astype(np.int64)
    assert (h == fingerprints(st.data, keys)).all()
    assert (h < 65536).all()                                # the seed was chosen so
    # ... encoded as a stripe of F words
    hd = torch.from_numpy(h.astype(np.uint16).view(np.int16)).cuda()
    enc = torch.zeros((S, st.no, F), dtype=torch.int16, device="cuda")
    cnt = torch.zeros(S * st.no, dtype=torch.int32, device="cuda")
    ent = torch.zeros(S * st.no * F, dtype=torch.int32, device="cuda")
    st.plan.encode(hd, enc, cnt, ent, F)
    torch.cuda.synchronize()
    e16 = enc.cpu().numpy().view(np.uint16).reshape(S * st.no, F)
    y = restored(e16, ent.cpu().numpy().reshape(S * st.no, F), cnt.cpu().numpy())
    y = y.reshape(S, st.no, F)
    # ... equals the fragments' fingerprints
    all_ids = np.tile(np.arange(k + m), (S, 1))
    got = Dev(st, 0).fp(all_ids, keys)
    assert (got == fingerprints(st.symbols(), keys)).all()
    assert (got[:, k if sys_ else 0:] == y).all()


@pytest.mark.parametrize("k,m,sys_", [(16, 48, 0), (10, 6, 1)])
def test_scrub_story(k, m, sys_):
    """item 5: one flipped symbol in one fragment of two stripes; the
    fingerprints of k + 4 fragments, laid out as rows of F words with buckets,
    name that fragment in all F columns through Plan.locate, and through
    Fec.fingerprint_blocks + Fec.check_fingerprints"""
    import quadiron_amd as qa
    torch = _torch()
    Sx, P, keys, R = 4, 4096, KEYS8[4:8], 4
    F, n, N = len(keys), k + m, k + 4
    first = k if sys_ else 0
    seed = _clean_seed(k, m, sys_, Sx, P, keys)
    st = Stripes(k, m, sys_, Sx, P, seed)
    rng = np.random.default_rng(k)
    ids = np.stack([np.sort(rng.choice(n, N, replace=False)) for _ in range(Sx)])
    if sys_:
        ids[3, 0] = 0 if 0 not in ids[3] else ids[3, 0]
        ids[3] = np.sort(ids[3])
    coded, data = st.coded.copy(), st.data.copy()
    bad = {1: int(ids[1][ids[1] >= first][-1]), 3: int(ids[3, 0])}
    for s, f in bad.items():
        row = data[s, f] if f < first else coded[s, f - first]
        assert f < first or not st.mask[s, f - first, 1234 + s]
        row[1234 + s] ^= 1
    got = Dev(st, 0, coded=coded, data=data).fp(ids, keys)   # (S, N, F)
    assert (got[[0, 2]] == _expect(st.symbols(), ids, keys)[[0, 2]]).all()
    if sys_:
        assert (got[ids < k] < 65536).all()                 # data rows carry no mark
    # the coordinator's stripe of F columns
    frows = np.zeros((Sx, st.no, F), np.uint16)
    fdata = np.zeros((Sx, k, F), np.uint16)
    fmask = np.zeros((Sx, st.no, F), bool)
    for s in range(Sx):
        for i, f in enumerate(ids[s]):
            if f < first:
                fdata[s, f] = got[s, i]
            else:
                frows[s, f - first] = got[s, i] & 0xffff
                fmask[s, f - first] = got[s, i] == 65536
    fs = Stripes.__new__(Stripes)
    fs.__dict__.update(st.__dict__)
    fs.coded, fs.data, fs.mask, fs.P = frows, fdata, fmask, F
    fdev = Dev(fs, 0, fmask)
    plan = st.plan
    ctx = torch.zeros(plan.locate_ctx_bytes(R, Sx), dtype=torch.uint8, device="cuda")
    plan.locate_ctx(torch.from_numpy(ids.astype(np.uint16).view(np.int16)).cuda(), ctx)
    located = torch.zeros(Sx * N, dtype=torch.int32, device="cuda")
    unloc = torch.zeros(Sx, dtype=torch.int32, device="cuda")
    fcnt = torch.zeros(Sx, dtype=torch.int32, device="cuda")
    assert plan.locate(ctx, R, fdev.dc, located, unloc, fcnt, data=fdev.dd, counts=fdev.cnt,
                       entries=fdev.ent, cap=fdev.cap) == 0
    torch.cuda.synchronize()
    loc = located.cpu().numpy().reshape(Sx, N)
    assert (unloc.cpu().numpy() == 0).all()
    for s in range(Sx):
        exp = np.where(ids[s] == bad.get(s, -1), F, 0)
        assert (loc[s] == exp).all(), (s, loc[s])

    # the same through the block API, stripe by stripe
    fec = qa.Fec(k, m, bool(sys_))
    for s in range(Sx):
        miss = np.ones(n, np.int32)
        miss[ids[s]] = 0
        cap = max(1, int(st.mask[s].sum(axis=1).max()))
        oor = np.zeros((st.no, cap), np.uint32)
        cnt = np.zeros(st.no, np.uint32)
        for j in range(st.no):
            c = np.flatnonzero(st.mask[s, j])
            cnt[j] = len(c)
            oor[j, :len(c)] = c
        drows = [np.ascontiguousarray(data[s, i]).view(np.uint8) for i in range(k)]
        prows = [np.ascontiguousarray(coded[s, j]).view(np.uint8) for j in range(st.no)]
        fp = fec.fingerprint_blocks(drows if sys_ else None, prows, oor, cnt, miss, keys)
        assert (fp[miss == 1] == -1).all()
        assert (fp[ids[s]] == got[s]).all()
        res = fec.check_fingerprints(fp, miss)
        exp = np.full(n + 1, -1, np.int64)
        exp[ids[s]] = 0
        exp[n] = 0
        if s in bad:
            exp[bad[s]] = F
        assert res.tolist() == exp.tolist(), s
    fec.close()


def test_errors():
    """item 6"""
    k, m = 16, 48
    st = Stripes(k, m, 0, 2, 2049, 11)
    mask = np.zeros_like(st.mask)
    mask[1, 7, :9] = True
    dev = Dev(st, 0, mask)
    ids = np.tile(np.arange(k + m), (2, 1))
    exp = _expect(st.symbols(mask), ids, KEYS8[:3])
    assert (dev.fp(ids, KEYS8[:3]) == exp).all()
    # a bucket count above the capacity given
    dev.cap = 8
    dev.ent = _i32(_buckets(mask, 9)[1][:, :, :8])
    dev.fp(ids, KEYS8[:3], err=1)
    assert st.plan.take_error() == 0
    # an id of k + m: bit 2, 0xFFFFFFFF, the neighbours as before
    dev = Dev(st, 0, mask)
    ids2 = ids.copy()
    ids2[1, 5] = k + m
    for words in (2049, 2 * _chunk_words(st.plan) + 1):
        if words > st.P:
            st2 = Stripes(k, m, 0, 2, words, 12)
            d2, e2 = Dev(st2, 0), _expect(st2.symbols(), ids, KEYS8[:3])
        else:
            d2, e2 = dev, exp
        got = d2.fp(ids2, KEYS8[:3], err=2)
        assert (got[1, 5] == 0xFFFFFFFF).all()
        e = e2.copy()
        e[1, 5] = 0xFFFFFFFF
        assert (got == e).all()
    # first_col + words > 2^32
    with pytest.raises(RuntimeError):
        dev.fp(ids, KEYS8[:1], first_col=(1 << 32) - 2048)
    assert (dev.fp(ids, KEYS8[:1], words=2048, first_col=(1 << 32) - 2048) ==
            _expect(st.symbols(mask, 2048), ids, KEYS8[:1], (1 << 32) - 2048)).all()


def _oracle_block(k, m, sys_, words, seed):
    data = np.random.default_rng(seed).integers(0, 65536, (k, words), dtype=np.uint16)
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, data.view(np.uint8).reshape(k, 2 * words),
                                          cap=64 + words // 256)
    y = restored(outs.view(np.uint16).reshape(-1, words), oor, cnt)
    if sys_:
        y = np.concatenate([data.astype(np.int64), y])
    return data.view(np.uint8).reshape(k, 2 * words), outs, oor, cnt, y


@pytest.mark.parametrize("k,m,sys_,words", [(10, 6, 1, 5000), (300, 20, 0, 3000)])
def test_block_api(k, m, sys_, words, monkeypatch):
    """item 7: -1 rows for missing fragments; (300, 20), above the other fused
    calls' k <= 256, against NumPy; a staging chunk forced small against the
    single-chunk result"""
    import quadiron_amd as qa
    data, outs, oor, cnt, y = _oracle_block(k, m, sys_, words, k)
    n = k + m
    miss = np.zeros(n, np.int32)
    miss[[1, n - 2]] = 1
    fec = qa.Fec(k, m, bool(sys_))
    args = (list(data) if sys_ else None, list(outs), np.ascontiguousarray(oor),
            np.ascontiguousarray(cnt), miss, KEYS8[:5])
    monkeypatch.delenv("QI_FINGERPRINT_CHUNK_WORDS", raising=False)
    one = fec.fingerprint_blocks(*args)
    exp = fingerprints(y, KEYS8[:5])
    exp[miss == 1] = -1
    assert (one == exp).all()
    for chunk in ("1000", "2048", "7"):
        if chunk == "7" and k > 16:
            continue
        monkeypatch.setenv("QI_FINGERPRINT_CHUNK_WORDS", chunk)
        assert (fec.fingerprint_blocks(*args) == one).all(), chunk
    monkeypatch.delenv("QI_FINGERPRINT_CHUNK_WORDS", raising=False)
    # no marks at all
    assert (fec.fingerprint_blocks(args[0], args[1], None, None, miss, KEYS8[:1])[miss == 0] ==
            fingerprints(np.where(y == 65536, 0, y), KEYS8[:1])[miss == 0]).all()
    if sys_:
        with pytest.raises(ValueError):                      # a data fingerprint of 65536
            bad = one[:, :2].copy()
            bad[0, 1] = 65536
            fec.check_fingerprints(bad, miss)
        # 14 present fragments, all listed: clean
        assert fec.check_fingerprints(one[:, :2], miss).tolist() == [
            -1 if miss[f] else 0 for f in range(n)] + [0]
    fec.close()
