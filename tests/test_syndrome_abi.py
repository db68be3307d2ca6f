"""CPU: the syndrome shares' entry points are exported with the signatures of
include/qi_gpu.h and wrapped, and calls without a plan are refused before
anything touches a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("qi_gpu_syndrome_ctx_bytes", "qi_gpu_syndrome_ctx", "qi_gpu_syndrome",
         "qi_gpu_syndrome_kernels", "qi_gpu_syndrome_locate_ctx_bytes",
         "qi_gpu_syndrome_locate_ctx", "qi_gpu_syndrome_locate",
         "qi_gpu_syndrome_locate_kernels", "qi_fec_syndrome_blocks", "qi_fec_locate_syndromes",
         "qi_fec_apply_deltas", "qi_fec_scrub_blocks")


def test_syndrome_symbols_exported():
    import quadiron_amd
    lib = quadiron_amd.lib()
    for name in NAMES:
        assert hasattr(lib, name), name


def test_python_wrappers_present():
    import quadiron_amd as qa
    for name in ("syndrome_ctx_bytes", "syndrome_ctx", "syndrome", "syndrome_kernels",
                 "syndrome_locate_ctx_bytes", "syndrome_locate_ctx", "syndrome_locate",
                 "syndrome_locate_kernels"):
        assert callable(getattr(qa.Plan, name)), name
    for name in ("syndrome_blocks", "locate_syndromes", "apply_deltas", "scrub_blocks"):
        assert callable(getattr(qa.Fec, name)), name
    assert qa.Plan.SYNDROME_MAX_CHECKS == 8 and qa.Plan.SYNDROME_MAX_ERRORS == 4


def _header_params(name):
    """the parameter list of `name` in include/qi_gpu.h, comments removed"""
    text = open(os.path.join(ROOT, "include", "qi_gpu.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"^((?:const )?\w+ ?\*?) ?" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.M)
    assert m, name
    return m.group(1).strip(), [" ".join(p.split()) for p in m.group(2).split(",")]


def _ctype(decl):
    """the ctypes type of a parameter declaration: every pointer is passed as
    an address"""
    if "*" in decl:
        return C.c_void_p
    if decl.startswith("long long"):
        return C.c_longlong
    return {"int": C.c_int, "size_t": C.c_size_t, "uint32_t": C.c_uint32}[decl.split()[0]]


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_signatures_match_header(name):
    import quadiron_amd
    fn = getattr(quadiron_amd.lib(), name)
    res, params = _header_params(name)
    got = [C.c_void_p if a is quadiron_amd.c_u8pp else a for a in fn.argtypes]
    assert got == [_ctype(p) for p in params], (name, params)
    want_res = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[res]
    assert fn.restype is want_res, (name, res)


def test_header_constants():
    text = open(os.path.join(ROOT, "include", "qi_gpu.h")).read()
    assert re.search(r"#define\s+QI_SYNDROME_MAX_CHECKS\s+8\b", text)
    assert re.search(r"#define\s+QI_SYNDROME_MAX_ERRORS\s+4\b", text)


def test_null_plan_is_refused():
    """no plan: 0 bytes, "" and -1, without a device"""
    import quadiron_amd
    lib = quadiron_amd.lib()
    assert lib.qi_gpu_syndrome_ctx_bytes(None, 1, 1, 1) == 0
    assert lib.qi_gpu_syndrome_locate_ctx_bytes(None, 2, 1) == 0
    assert lib.qi_gpu_syndrome_kernels(None, 1, 1, 64) == b""
    assert lib.qi_gpu_syndrome_locate_kernels(None, 2, 1, 64) == b""
    assert lib.qi_gpu_syndrome_ctx(None, None, None, 1, 1, 1, None, None) == -1
    assert lib.qi_gpu_syndrome(None, None, 1, 1, None, 0, 0, None, None, 0, None, 0, 0, None,
                               None, 0, None, 0, 0, None, None, 0, 64, 1, None) == -1
    assert lib.qi_gpu_syndrome_locate_ctx(None, None, 2, 1, None, None) == -1
    assert lib.qi_gpu_syndrome_locate(None, None, 2, 1, None, 0, 0, None, None, 0, None, None,
                                      None, None, None, 0, 64, 1, None) == -1
    assert lib.qi_fec_syndrome_blocks(None, None, 4, None, 1, None, None, None, 0, 1, 0, None,
                                      None, None, 0, 128) == -1
    assert lib.qi_fec_locate_syndromes(None, None, 4, None, None, None, 0, 0, None, None, 0,
                                       None, 128) == -1
    assert lib.qi_fec_apply_deltas(None, None, 0, None, None, None, 0, None, 0, 128) == -1
    assert lib.qi_fec_scrub_blocks(None, None, None, None, None, 0, None, 1, None, 0, 128) == -1
