"""The reference of the fingerprint tests: NumPy int64, straight from the
definition in include/qi_gpu.h.  Never the code under test."""
import numpy as np

Q = 65537

# components 1, 2, 32768, 32769, 65536, mixed, and two random keys
KEYS8 = np.array([(1, 1, 1), (2, 2, 2), (32768, 32768, 32768), (32769, 32769, 32769),
                  (65536, 65536, 65536), (1, 65536, 2), (40503, 17, 60001), (3, 54321, 12345)],
                 np.int64)


def _powers(base, n):
    p = np.ones(n, np.int64)
    for x in range(1, n):
        p[x] = p[x - 1] * int(base) % Q
    return p


def weights(key, first_col, words):
    """w(first_col + c) for c < words: a^C0 b^C1 d^C2 mod 65537."""
    a, b, d = (int(v) for v in key)
    C = int(first_col) + np.arange(words, dtype=np.int64)
    c2 = C >> 16
    pd = np.array([pow(d, int(e), Q) for e in range(int(c2[0]), int(c2[-1]) + 1)], np.int64)
    return _powers(a, 256)[C & 255] * _powers(b, 256)[(C >> 8) & 255] % Q * pd[c2 - c2[0]] % Q


def fingerprints(y, keys, first_col=0):
    """y: (..., words) restored symbols in 0 .. 65536 -> (..., F) int64."""
    y = np.asarray(y, np.int64)
    out = [(y * weights(k, first_col, y.shape[-1]) % Q).sum(axis=-1) % Q for k in keys]
    return np.stack(out, axis=-1)


def restored(coded_u16, oor, cnt):
    """(rows, P) u16 + the oracle's / the block API's mark lists -> int64
    symbols with 65536 at the marks."""
    y = np.asarray(coded_u16).astype(np.int64)
    for j in range(y.shape[0]):
        y[j, oor[j, :cnt[j]]] = 65536
    return y
