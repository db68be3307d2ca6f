"""GPU: unwanted outputs at the host boundaries -- NULL entries of
qi_fec_encode_blocks' outputs, `wanted` of qi_fec_decode_blocks, `wanted_idxs`
of quadiron_fnt32_encode, NULL output streams of the stream API.  The
reference (src/fec_base.h:1066-1151, :1177-1321, src/quadiron_c.cpp:73-140)
still fills every output's property list, writes only the wanted buffers and
leaves the others untouched.  The expectation is the oracle's C glue, which
takes the same masks; buffers that must not be written start as 0xA5."""
import ctypes as C

import numpy as np
import pytest

from qi_testlib import (check_windows_vs_oracle, chunk_windows, codec, craft_oor_columns,
                        golden_names, load, oracle, oracle_encode_blocks, ptrs, retry_block,
                        row_ptrs, vp)

pytestmark = pytest.mark.gpu

A5 = 0xA5
MASKS = ("none", "first", "last", "alternating", "all")


def _mask(kind, n):
    w = np.zeros(n, np.int32)
    if kind == "first":
        w[0] = 1
    elif kind == "last":
        w[-1] = 1
    elif kind == "alternating":
        w[::2] = 1
    elif kind == "all":
        w[:] = 1
    return w


def _block(k, m, sys_, words, seed, n_craft=24):
    rng = np.random.default_rng([k, m, sys_, words, seed])
    lanes = rng.integers(0, 65536, (k, words), dtype=np.uint16)
    craft_oor_columns(k, m, sys_, lanes, rng, n_craft)
    return lanes.view(np.uint8).reshape(k, 2 * words), rng


def _oracle_encode_masked(k, m, sys_, data, wanted, cap):
    """qo_encode_blocks with NULL outputs where not wanted: (outs, oor, cnt);
    the rows of unwanted outputs stay 0xA5"""
    c = codec(k, m, sys_)
    B = data.shape[1]
    outs = np.full((c.n_outputs, B), A5, np.uint8)
    oor = np.zeros((c.n_outputs, cap), np.uint32)
    cnt = np.zeros(c.n_outputs, np.uint32)
    oracle().qo_encode_blocks(C.byref(c), row_ptrs(np.ascontiguousarray(data)),
                              row_ptrs(outs, wanted), C.c_size_t(B), vp(oor), vp(cnt),
                              C.c_uint32(cap))
    return outs, oor, cnt


def _fec_encode_masked(hip_lib, f, data, wanted, cap, fn="qi_fec_encode_blocks", rc=0):
    import quadiron_amd as qa
    no, B = f.n_outputs, data.shape[1]
    outs = np.full((no, B), A5, np.uint8)
    oor = np.zeros((no, cap), np.uint32)
    cnt = np.zeros(no, np.uint32)
    rows = [np.ascontiguousarray(data[i]) for i in range(f.k)]
    op = qa.ptr_array([outs[i] if wanted[i] else None for i in range(no)])
    if fn == "qi_fec_encode_blocks":
        got = hip_lib.qi_fec_encode_blocks(f.h, qa.ptr_array(rows), op, B, vp(oor), vp(cnt), cap)
    else:
        got = hip_lib.qi_fec_encode_streams(f.h, qa.ptr_array(rows), B, op, vp(oor), vp(cnt), cap)
    assert got == rc
    return outs, oor, cnt


def _check_encode(got, exp, wanted):
    outs, oor, cnt = got
    o_outs, o_oor, o_cnt = exp
    for i in range(outs.shape[0]):
        if wanted[i]:
            assert (outs[i] == o_outs[i]).all(), i
        else:   # never handed over: the oracle's copy is untouched too
            assert (outs[i] == A5).all() and (o_outs[i] == A5).all(), i
    # the property lists of ALL outputs, wanted or not
    assert (cnt == o_cnt).all(), (cnt, o_cnt)
    for i in range(outs.shape[0]):
        assert (oor[i, :cnt[i]] == o_oor[i, :o_cnt[i]]).all(), i


def _erasures(k, m, sys_, rng):
    """m erasures, data fragment 0 among them"""
    miss = np.zeros(k + m, np.int32)
    miss[[0] + list(rng.choice(np.arange(1, k + m), m - 1, replace=False))] = 1
    return miss


def _decode_buffers(k, sys_, data, outs, miss):
    """(data rows, parity pointers' rows): present systematic data rows hold
    the data, every other data buffer 0xA5; missing coded rows are NULL"""
    B = data.shape[1]
    dec = np.full((k, B), A5, np.uint8)
    if sys_:
        have = miss[:k] == 0
        dec[have] = data[have]
    first = k if sys_ else 0
    present = miss[first:first + outs.shape[0]] == 0
    return dec, np.ascontiguousarray(outs).copy(), present


def _check_decode_masked(hip_lib, f, k, m, sys_, data, outs, oor, cnt, miss, wanted):
    import quadiron_amd as qa
    B = data.shape[1]
    c = codec(k, m, sys_)
    o_dec, o_par, present = _decode_buffers(k, sys_, data, outs, miss)
    assert oracle().qo_decode_blocks(C.byref(c), row_ptrs(o_dec), row_ptrs(o_par, present),
                                     vp(oor), vp(cnt), C.c_uint32(oor.shape[1]), vp(miss),
                                     vp(wanted), C.c_size_t(B)) == 1
    dec, par, _ = _decode_buffers(k, sys_, data, outs, miss)
    pp = qa.ptr_array([par[i] if present[i] else None for i in range(par.shape[0])])
    assert hip_lib.qi_fec_decode_blocks(
        f.h, qa.ptr_array([dec[i] for i in range(k)]), pp, vp(oor), vp(cnt), oor.shape[1],
        vp(miss), vp(wanted), B) == 1
    for i in range(k):
        assert (dec[i] == o_dec[i]).all(), i
        if wanted[i]:
            assert (dec[i] == data[i]).all(), i
        elif not sys_ or miss[i]:
            assert (dec[i] == A5).all(), i
    assert (par == outs).all()   # inputs are read only


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("k,m,sys_", [(4, 4, 0), (4, 4, 1), (10, 6, 1)])
def test_blocks_masked(hip_lib, k, m, sys_, mask):
    import quadiron_amd as qa
    data, rng = _block(k, m, sys_, 2048, 1)
    f = qa.Fec(k, m, bool(sys_))
    cap = 64
    wanted = _mask(mask, f.n_outputs)
    exp = _oracle_encode_masked(k, m, sys_, data, wanted, cap)
    assert exp[2].sum() > 0
    _check_encode(_fec_encode_masked(hip_lib, f, data, wanted, cap), exp, wanted)
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, data, cap)
    miss = _erasures(k, m, sys_, rng)
    _check_decode_masked(hip_lib, f, k, m, sys_, data, outs, oor, cnt, miss, _mask(mask, k))


@pytest.mark.parametrize("name", golden_names("mask_"))
def test_masks_vs_reference_golden(hip_lib, name):
    """The reference's own results under an alternating encode mask and a
    one-hot decode mask (tests/golden/gen_golden.py `_gen_masked`; the same
    fixture pins the oracle in tests/test_oracle_golden.py)."""
    import quadiron_amd as qa
    g = load(name)
    k, m, sys_, pkt, B, cap, md = (int(v) for v in g["params"])
    f = qa.Fec(k, m, bool(sys_))
    ew = g["enc_wanted"]
    outs, oor, cnt = _fec_encode_masked(hip_lib, f, g["data"], ew, cap)
    assert (outs == g["outputs"]).all()
    assert (cnt == g["oor_count"]).all() and (oor == g["oor"]).all()
    miss, dw = g["missing"], g["dec_wanted"]
    dec, par, present = _decode_buffers(k, sys_, g["data"], g["full_outputs"], miss)
    assert hip_lib.qi_fec_decode_blocks(
        f.h, qa.ptr_array([dec[i] for i in range(k)]),
        qa.ptr_array([par[i] if present[i] else None for i in range(par.shape[0])]),
        vp(g["oor"]), vp(g["oor_count"]), cap, vp(miss), vp(dw), B) == 1
    assert (dec == g["decoded"]).all()
    h = qa.QuadironFnt32(2, k, m, sys_)
    assert h.metadata_size(B) == md
    cd = [np.concatenate([np.full(md, A5, np.uint8), g["data"][i]]) for i in range(k)]
    cp = [np.full(md + B, A5, np.uint8) for _ in range(m)]
    assert h.encode(cd, cp, ew, B) == 0
    assert (np.stack(cd) == g["cabi_data"]).all()
    assert (np.stack(cp) == g["cabi_parity"]).all()


@pytest.mark.parametrize("sys_", [0, 1])
def test_retry_block_one_hot(hip_lib, sys_):
    """The retry block (more marks in one output than the first attempt's
    buckets hold) under a one-hot mask: the second attempt writes the wanted
    row alone, and every output's marks are complete."""
    import quadiron_amd as qa
    k, m = 4, 4
    data, outs, oor, cnt, r, first_cap = retry_block(sys_)
    assert first_cap < cnt[r] <= 128
    f = qa.Fec(k, m, bool(sys_))
    for want in (r, 0):
        wanted = np.zeros(f.n_outputs, np.int32)
        wanted[want] = 1
        exp = _oracle_encode_masked(k, m, sys_, data, wanted, 128)
        assert (exp[1] == oor).all() and (exp[2] == cnt).all()
        _check_encode(_fec_encode_masked(hip_lib, f, data, wanted, 128), exp, wanted)


def test_two_chunk_block_alternating(hip_lib):
    """4 MiB + 1 KiB per fragment: two pipeline chunks, marks in both, under
    an alternating mask -- the writer's NULL rows.  The wanted rows and the
    marks of all rows against the oracle window by window; unwanted rows are
    never handed over."""
    import quadiron_amd as qa
    k, m, sys_ = 4, 4, 0
    words = 2**21 + 512
    rng = np.random.default_rng(77)
    lanes = rng.integers(0, 65536, (k, words), dtype=np.uint16)
    for c0 in (0, 2**21 - 40, 2**21 + 8, words - 100):
        craft_oor_columns(k, m, sys_, lanes, rng, 6, col_range=(c0, min(words, c0 + 80)))
    data = lanes.view(np.uint8).reshape(k, 2 * words)
    f = qa.Fec(k, m, False)
    wanted = _mask("alternating", f.n_outputs)
    cap = 256
    outs, oor, cnt = _fec_encode_masked(hip_lib, f, data, wanted, cap)
    assert cnt.max() <= cap
    assert sum(int((oor[i, :cnt[i]] < 2**21).sum()) for i in range(f.n_outputs)) >= 3
    assert sum(int((oor[i, :cnt[i]] >= 2**21).sum()) for i in range(f.n_outputs)) >= 3
    assert (outs[wanted == 0] == A5).all()
    # the windows compare rows too: give them the oracle's for the unwanted
    wins = chunk_windows(words)
    filled = outs.copy()
    for lo, hi in wins:
        o_out, _, _ = oracle_encode_blocks(k, m, sys_, np.ascontiguousarray(
            data[:, 2 * lo:2 * hi]), 64 + hi - lo)
        filled[wanted == 0, 2 * lo:2 * hi] = o_out[wanted == 0]
    check_windows_vs_oracle(k, m, sys_, data, filled, oor, cnt, wins)


@pytest.mark.parametrize("mask", ["first", "alternating"])
@pytest.mark.parametrize("sys_", [0, 1])
def test_fnt32_encode_partial_wanted(hip_lib, sys_, mask):
    """quadiron_fnt32_encode with a partial wanted_idxs: the FNT1 header of
    every fragment is written, the payload of an unwanted one is untouched;
    every byte equals qo_fnt32_encode's on the same buffers."""
    import quadiron_amd as qa
    k, m, words = 4, 4, 2048
    B = 2 * words
    data, _ = _block(k, m, sys_, words, 3)
    h = qa.QuadironFnt32(2, k, m, sys_)
    md = h.metadata_size(B)
    c = codec(k, m, sys_)
    wanted = _mask(mask, c.n_outputs)

    def frags():
        return ([np.concatenate([np.full(md, A5, np.uint8), data[i]]) for i in range(k)],
                [np.full(md + B, A5, np.uint8) for _ in range(m)])
    d, p = frags()
    assert h.encode(d, p, wanted, B) == 0
    od, op = frags()
    assert oracle().qo_fnt32_encode(C.byref(c), ptrs(od), ptrs(op), vp(wanted),
                                    C.c_size_t(B)) == 0
    for i, (x, y) in enumerate(zip(d + p, od + op)):
        assert (x == y).all(), i
    assert sum(int.from_bytes(bytes(fr[4:8]), "big") for fr in (p if sys_ else d + p)) > 0
    for i in range(c.n_outputs):
        buf = p[i] if sys_ else (d + p)[i]
        assert bytes(buf[:4]) != bytes([A5] * 4), i        # a header, wanted or not
        if not wanted[i]:
            keep = data[i] if (not sys_ and i < k) else A5
            assert (buf[md:] == keep).all(), i


@pytest.mark.parametrize("mask", ["first", "alternating"])
def test_streams_null_outputs(hip_lib, mask):
    """NULL entries among the output streams, one chunk with a ragged tail.
    qi_fec_encode_streams needs every output (include/qi_gpu.h, as the
    reference's encode_streams_vertical): a NULL one is refused with -1
    before anything is written, and with all of them the result is the
    oracle's.  qi_fec_decode_streams: a NULL out_data[i] is not wanted."""
    import quadiron_amd as qa
    k, m, sys_, B = 4, 4, 0, 2**20 + 6
    words = B // 2
    data, rng = _block(k, m, sys_, words, 5)
    f = qa.Fec(k, m, False)
    cap = 128
    wanted = _mask(mask, f.n_outputs)
    got = _fec_encode_masked(hip_lib, f, data, wanted, cap, "qi_fec_encode_streams", rc=-1)
    assert (got[0] == A5).all() and not got[2].any()
    every = _mask("all", f.n_outputs)
    exp = _oracle_encode_masked(k, m, sys_, data, every, cap)
    assert exp[2].sum() > 0
    _check_encode(_fec_encode_masked(hip_lib, f, data, every, cap, "qi_fec_encode_streams"),
                  exp, every)
    # decode: NULL output streams are not written, the others hold the data
    outs, oor, cnt = exp
    miss = _erasures(k, m, sys_, rng)
    par = [None if miss[i] else outs[i] for i in range(f.n_outputs)]
    want = _mask(mask, k)
    dec = np.full((k, B), A5, np.uint8)
    rc = hip_lib.qi_fec_decode_streams(
        f.h, None, qa.ptr_array(par), B, vp(oor), vp(cnt), cap,
        qa.ptr_array([dec[i] if want[i] else None for i in range(k)]))
    assert rc == 1
    for i in range(k):
        assert (dec[i] == (data[i] if want[i] else A5)).all(), i
