"""CPU: the fragment fingerprint's entry points are exported, their ctypes
signatures load, the Python wrappers exist, and without a plan (no device)
the calls refuse instead of launching."""
import ctypes as C
import inspect

import numpy as np


def test_fingerprint_symbols_and_signatures():
    import quadiron_amd
    lib = quadiron_amd.lib()
    for name in ("qi_gpu_fingerprint", "qi_gpu_fingerprint_work_bytes",
                 "qi_gpu_fingerprint_kernels", "qi_fec_fingerprint_blocks"):
        assert hasattr(lib, name), name
    assert lib.qi_gpu_fingerprint.restype is C.c_int
    assert len(lib.qi_gpu_fingerprint.argtypes) == 20
    assert lib.qi_gpu_fingerprint_work_bytes.restype is C.c_size_t
    assert len(lib.qi_gpu_fingerprint_work_bytes.argtypes) == 5
    assert lib.qi_gpu_fingerprint_kernels.restype is C.c_char_p
    assert len(lib.qi_gpu_fingerprint_kernels.argtypes) == 4
    assert lib.qi_fec_fingerprint_blocks.restype is C.c_int
    assert len(lib.qi_fec_fingerprint_blocks.argtypes) == 11


def test_python_wrappers_present():
    import quadiron_amd as qa
    for name in ("fingerprint", "fingerprint_work_bytes", "fingerprint_kernels"):
        assert callable(getattr(qa.Plan, name)), name
    assert qa.Plan.FINGERPRINT_MAX_KEYS == 8
    assert callable(qa.Fec.fingerprint_blocks)
    p = inspect.signature(qa.Fec.check_fingerprints).parameters
    assert list(p)[1:] == ["fp", "missing", "max_errors"] and p["max_errors"].default == 1
    p = inspect.signature(qa.Plan.fingerprint).parameters
    assert p["first_col"].default == 0


def test_no_plan_launches_nothing():
    """A NULL plan: -1, "" and 0, before any device call."""
    import quadiron_amd
    lib = quadiron_amd.lib()
    keys = np.ones((1, 3), np.uint32)
    assert lib.qi_gpu_fingerprint_kernels(None, 4, 2, 4096) == b""
    assert lib.qi_gpu_fingerprint_work_bytes(None, 4, 2, 1, 4096) == 0
    assert lib.qi_gpu_fingerprint(None, None, 4, keys.ctypes.data_as(C.c_void_p), 1, 0, None, 0,
                                  0, None, 0, 0, None, None, 0, None, None, 4096, 1, None) == -1


def test_block_call_refuses_bad_keys():
    """a key of 0 or 65537 and F = 0 or 9 are refused before the handle is
    used"""
    import quadiron_amd
    lib = quadiron_amd.lib()

    def call(keys, n):
        k = np.ascontiguousarray(keys, np.uint32)
        return lib.qi_fec_fingerprint_blocks(None, None, None, None, None, 0, None,
                                             k.ctypes.data_as(C.c_void_p), n, None, 64)
    good = np.full((9, 3), 7)
    for bad in (0, 65537):
        k = good.copy()
        k[1, 2] = bad
        assert call(k, 2) == -1
    assert call(good, 0) == -1 and call(good, 9) == -1
    assert lib.qi_fec_fingerprint_blocks(None, None, None, None, None, 0, None, None, 1, None,
                                         64) == -1
    # the Python wrappers check before the library is asked
    import pytest
    for keys in ([(0, 1, 1)], [(1, 65537, 1)], [], [(1, 1, 1)] * 9, [(1, 1)]):
        with pytest.raises(ValueError):
            quadiron_amd.Plan._keys(keys)
