"""CPU: the fragment fingerprint's arithmetic from the library's host header
(tests/host/test_fingerprint_math.cpp compiles quadiron_amd/csrc/
fingerprint_math.h alone, with -fsanitize=undefined -DQI_HOST_CHECK) against
NumPy int64 (fp_testlib): the 64-bit reference and the kernel's lane steps in
both forms (columns 256 apart; 16-byte pieces), walked chunk by chunk as
fingerprint.hip walks them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from fp_testlib import KEYS8, Q, fingerprints, restored
from qi_testlib import oracle_encode_blocks

HERE = os.path.dirname(os.path.abspath(__file__))
WIDTHS = (1, 7, 8, 255, 256, 257, 2047, 2049, 65535, 65537, 131075)
FIRST = (0, 1, 255, 256, 65535, 3 * 65536 + 17)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    out = str(tmp_path_factory.mktemp("fingerprint") / "test_fingerprint_math")
    subprocess.check_call([
        "g++", "-std=c++20", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
        "-DQI_HOST_CHECK", os.path.join(HERE, "host", "test_fingerprint_math.cpp"), "-o", out])
    return out


def run(exe, y, first_col, keys):
    """{'ref' | 'scalar' | 'vec': F values or None}"""
    keys = np.asarray(keys, np.int64)
    res = subprocess.run([exe, str(len(y)), str(first_col), str(len(keys))] +
                         [str(int(v)) for v in keys.reshape(-1)],
                         input=np.asarray(y, "<u4").tobytes(), capture_output=True, timeout=300)
    assert res.returncode == 0, res.stderr
    assert b"runtime error" not in res.stderr, res.stderr
    out = {}
    for ln in res.stdout.decode().split("\n"):
        if ln:
            name, *vals = ln.split()
            out[name] = None if vals == ["-"] else [int(v) for v in vals]
    assert set(out) == {"ref", "scalar", "vec"}
    assert (out["vec"] is None) == (first_col % 8 != 0)
    return out


def check(exe, y, first_col, keys):
    exp = fingerprints(y, keys, first_col).tolist()
    got = run(exe, y, first_col, keys)
    assert got["ref"] == exp, (len(y), first_col)
    assert got["scalar"] == exp, (len(y), first_col)
    assert got["vec"] in (None, exp), (len(y), first_col)
    return exp


@pytest.mark.parametrize("words", WIDTHS)
def test_values_vs_numpy(exe, words):
    """random symbols with marks, at every first_col (and a multiple of 8 past
    a 65536 boundary, so that the piece form meets a C2 step too)"""
    rng = np.random.default_rng(words)
    y = rng.integers(0, 65536, words)
    y[rng.random(words) < 0.02] = 65536
    y[[0, -1]] = 65536, 65535
    for fc in FIRST + (3 * 65536 - 8,):
        check(exe, y, fc, KEYS8)


@pytest.mark.parametrize("words", (2049, 65537))
def test_extremes(exe, words):
    """rows of all 0xFFFF, and every column marked under key (65536, 65536,
    65536) (every product is +-1 times +-1: the accumulator extreme) and under
    32768 (the largest balanced weight)"""
    for fc in (0, 255):
        check(exe, np.full(words, 65535), fc, KEYS8)
        check(exe, np.full(words, 65536), fc, [(65536, 65536, 65536), (32768, 32768, 32768),
                                               (32769, 32769, 32769)])
        check(exe, np.full(words, 32768), fc, KEYS8)
        check(exe, np.full(words, 32769), fc, KEYS8)


def test_additive_over_every_cut(exe):
    """slices [0, cut) and [cut, 600) with first_col set add to the whole row"""
    rng = np.random.default_rng(600)
    y = rng.integers(0, 65537, 600)
    keys = KEYS8[[1, 4, 6]]
    for fc in (0, 65536 - 300):
        whole = np.array(check(exe, y, fc, keys))
        for cut in range(1, 600):
            a = np.array(run(exe, y[:cut], fc, keys)["scalar"])
            b = np.array(run(exe, y[cut:], fc + cut, keys)["scalar"])
            assert ((a + b) % Q == whole).all(), (fc, cut)


@pytest.mark.parametrize("k,m,sys_,seed", [(5, 6, 0, 1), (10, 6, 1, 1)])
def test_homomorphic_on_the_oracles_encode(exe, k, m, sys_, seed):
    """the fingerprints of the encoded fragments are the encode of the data
    rows' fingerprints (as a stripe of F words), marks included"""
    P = 300
    keys = KEYS8[[5, 6, 7]]
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 65536, (k, P), dtype=np.uint16)
    outs, oor, cnt = oracle_encode_blocks(k, m, sys_, data.view(np.uint8).reshape(k, 2 * P),
                                          cap=P)
    frag = restored(outs.view(np.uint16).reshape(-1, P), oor, cnt)
    fp_frag = np.array([check(exe, r, 0, keys) for r in frag])
    fp_data = np.array([check(exe, r, 0, keys) for r in data.astype(np.int64)])
    assert (fp_data < 65536).all()          # the seed is chosen so; a data row holds no 65536
    F = len(keys)
    h = np.ascontiguousarray(fp_data.astype(np.uint16))
    o2, oor2, cnt2 = oracle_encode_blocks(k, m, sys_, h.view(np.uint8).reshape(k, 2 * F), cap=F)
    enc = restored(o2.view(np.uint16).reshape(-1, F), oor2, cnt2)
    assert (enc == fp_frag).all()
