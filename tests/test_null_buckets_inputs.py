"""CPU: the inputs of tests/test_gpu_null_buckets.py do what they claim, from
the oracle alone -- marks in every encode case, a NULL decode that differs
from the data, a rebuilt 65536 in every repair, verify, partial and syndrome
case, both mismatch counts non-zero in the verify cases -- and the oracle
stores a decoded 65536 as 0, as the reference's unpack does."""
import numpy as np
import pytest

import test_gpu_null_buckets as nb
from qi_testlib import Q, decode_matrix, oracle_decode_blocks

# (the module's gpu mark does not apply here: only its case builders are used)


@pytest.mark.parametrize("sys_", [0, 1])
def test_oracle_stores_decoded_65536_as_0(sys_):
    """Received symbols solved so that data row 0 decodes to exactly 65536
    in column 0: the oracle's block decode writes the low 16 bits, 0."""
    k, m = 3, 3
    ids = np.array([1, 3, 4])
    M = decode_matrix(k, m, sys_, ids)
    rng = np.random.default_rng(12 + sys_)
    for _ in range(100):
        r = rng.integers(0, 65536, k).astype(np.int64)
        p = int(np.flatnonzero(M[0])[-1])
        rest = int(M[0] @ r) - int(M[0, p] * r[p])
        r[p] = (65536 - rest) % Q * pow(int(M[0, p]), Q - 2, Q) % Q
        d = M @ r % Q
        if r[p] < 65536 and d[0] == 65536:
            break
    else:
        raise AssertionError("no such column found")
    frag = np.zeros((k + m, 1), np.uint16)
    frag[ids, 0] = r
    data = frag[:k].copy().view(np.uint8)
    coded = np.ascontiguousarray(frag[k:] if sys_ else frag).view(np.uint8)
    missing = np.ones(k + m, np.int32)
    missing[ids] = 0
    no = coded.shape[0]
    ok, dec = oracle_decode_blocks(k, m, sys_, coded, np.zeros((no, 1), np.uint32),
                                   np.zeros(no, np.uint32), missing, data)
    assert ok == 1
    got = dec.view(np.uint16)[:, 0].astype(np.int64)
    assert (got == (d & 0xffff)).all() and got[0] == 0


@pytest.mark.parametrize("k,m,sys_,P,encoder,fam", nb.ENCODE_CASES)
def test_encode_cases_hold_marks(k, m, sys_, P, encoder, fam):
    n_marks, zero = nb.encode_case_marks(k, m, sys_, P)
    assert n_marks > 0 and zero


@pytest.mark.parametrize("k,m,sys_,P,fam", nb.DECODE_CASES + nb.MIXED_CASES)
def test_decode_cases_differ_from_the_data(k, m, sys_, P, fam):
    nb.decode_case(k, m, sys_, P).check_inputs()


def test_dense_decode_case():
    k, m, sys_, P, _ = nb.DENSE_CASE
    c = nb.decode_case(k, m, sys_, P, True)
    c.check_inputs()
    assert nb.dense_marks(c) > 256


@pytest.mark.parametrize("k,m,sys_,R,P,fam", sorted(set(nb.REPAIR_CASES + nb.VERIFY_CASES)))
def test_repair_cases_rebuild_a_65536(k, m, sys_, R, P, fam):
    c = nb.repair_case(k, m, sys_, R, P)
    c.check_inputs()
    vm, mm, first = nb.verify_expect(c)
    assert vm[0].sum() > 0 and mm[0].sum() > 0 and (first[0] != nb.NONE).any()


@pytest.mark.parametrize("k,m,sys_,H,R,P,fam", nb.PARTIAL_CASES)
def test_partial_cases_hold_a_65536(k, m, sys_, H, R, P, fam):
    c, _, exp = nb.partial_case(k, m, sys_, H, R, P)
    assert c.n_marks > 0 and (exp[0] == 65536).any()


def test_syndrome_case_holds_a_65536():
    k, m, sys_, H, R, P, _ = nb.SYNDROME_CASE
    c, exp = nb.syndrome_case(k, m, sys_, H, R, P)
    assert c.n_marks > 0 and (exp[0] == 65536).any()
