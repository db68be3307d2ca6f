"""CPU: the device patch's entry points are exported, their ctypes signatures
load, the header declares its constants, the Python wrappers exist and reject
bad dtypes and shapes, and without a plan (no device) the calls refuse instead
of launching."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONSTANTS = {"QI_PATCH_ABSOLUTE": 0, "QI_PATCH_DELTA": 1, "QI_PATCH_NONE": 0,
             "QI_PATCH_DONE": 1, "QI_PATCH_UNLOCATED": 2, "QI_PATCH_TRUNCATED": 3,
             "QI_PATCH_BAD_FIX": 4, "QI_PATCH_DATA_MARK": 5, "QI_PATCH_BUCKET_FULL": 6}


def test_patch_symbols_exported():
    import quadiron_amd
    lib = quadiron_amd.lib()
    for name in ("qi_gpu_patch_work_bytes", "qi_gpu_patch", "qi_gpu_patch_kernels"):
        assert hasattr(lib, name), name


def test_patch_signatures():
    import quadiron_amd
    lib = quadiron_amd.lib()
    assert lib.qi_gpu_patch_work_bytes.restype is C.c_size_t
    assert len(lib.qi_gpu_patch_work_bytes.argtypes) == 3
    assert lib.qi_gpu_patch.restype is C.c_int
    assert len(lib.qi_gpu_patch.argtypes) == 25
    assert lib.qi_gpu_patch_kernels.restype is C.c_char_p
    assert len(lib.qi_gpu_patch_kernels.argtypes) == 4


def test_header_declares_the_constants():
    text = open(os.path.join(ROOT, "include", "qi_gpu.h")).read()
    for name, value in CONSTANTS.items():
        m = re.search(rf"^#define {name}\s+(\d+)\b", text, re.M)
        assert m and int(m.group(1)) == value, name
    for fn in ("qi_gpu_patch_work_bytes", "qi_gpu_patch", "qi_gpu_patch_kernels"):
        assert re.search(rf"\b{fn}\(", text), fn


def test_python_wrappers_present():
    import quadiron_amd as qa
    for name in ("patch_work_bytes", "patch", "patch_kernels"):
        assert callable(getattr(qa.Plan, name)), name
    for name, value in CONSTANTS.items():
        assert getattr(qa.Plan, name[3:]) == value, name


def test_no_plan_launches_nothing():
    """A NULL plan: 0 bytes, "", -1 -- before any device call."""
    import quadiron_amd
    lib = quadiron_amd.lib()
    assert lib.qi_gpu_patch_work_bytes(None, 4, 1) == 0
    assert lib.qi_gpu_patch_kernels(None, 4, 0, 4096) == b""
    assert lib.qi_gpu_patch(None, 0, None, 4, None, None, None, None, None, 0, None, 0, 0,
                            None, 0, 0, None, None, 0, None, None, None, 4096, 1, None) == -1


def test_wrapper_rejects_bad_tensors():
    """Plan.patch checks dtypes, shapes and devices before it reaches the
    library: a plan object without a handle never gets that far."""
    import torch
    import quadiron_amd as qa
    p = qa.Plan.__new__(qa.Plan)
    p.h, p.k, p.m, p.sys, p.n, p.n_outputs = None, 3, 5, False, 8, 8
    S, N, P = 2, 5, 16
    ids = torch.zeros(S, N, dtype=torch.int16)
    i32 = torch.zeros(S, dtype=torch.int32)
    coded = torch.zeros(S, 8, P, dtype=torch.int16)
    with pytest.raises(ValueError):     # mode
        p.patch(2, ids, i32, None, 0, coded, i32, i32, None)
    with pytest.raises(ValueError):     # ids' shape
        p.patch(0, ids.reshape(-1), i32, None, 0, coded, i32, i32, None)
    with pytest.raises(TypeError):      # rows on the host
        p.patch(0, ids, i32, None, 0, coded, i32, i32, None)
    with pytest.raises(TypeError):      # rows of the wrong type
        p.patch(0, ids, i32, None, 0, coded.float(), i32, i32, None)
    with pytest.raises(ValueError):     # no rows
        p.patch(0, ids, i32, None, 0, None, i32, i32, None)
    p.close()
