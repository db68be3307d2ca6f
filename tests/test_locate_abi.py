"""CPU: the fragment locate's entry points are exported, their ctypes
signatures load, the Python wrappers exist, and without a plan (no device)
the calls refuse instead of launching."""
import ctypes as C


def test_locate_symbols_exported():
    import quadiron_amd
    lib = quadiron_amd.lib()
    for name in ("qi_gpu_locate_ctx_bytes", "qi_gpu_locate_ctx", "qi_gpu_locate",
                 "qi_gpu_locate_kernels", "qi_fec_locate_blocks"):
        assert hasattr(lib, name), name


def test_locate_signatures():
    import quadiron_amd
    lib = quadiron_amd.lib()
    assert lib.qi_gpu_locate_ctx_bytes.restype is C.c_size_t
    assert len(lib.qi_gpu_locate_ctx_bytes.argtypes) == 3
    assert lib.qi_gpu_locate_ctx.restype is C.c_int
    assert len(lib.qi_gpu_locate_ctx.argtypes) == 6
    assert lib.qi_gpu_locate.restype is C.c_int
    assert len(lib.qi_gpu_locate.argtypes) == 21
    assert lib.qi_gpu_locate_kernels.restype is C.c_char_p
    assert len(lib.qi_gpu_locate_kernels.argtypes) == 3


def test_python_wrappers_present():
    import quadiron_amd as qa
    for name in ("locate_ctx_bytes", "locate_ctx", "locate", "locate_kernels"):
        assert callable(getattr(qa.Plan, name)), name
    assert callable(qa.Fec.locate_blocks)
    assert qa.Plan.LOCATE_MAX_CHECKS == 8


def test_no_plan_launches_nothing():
    """A NULL plan: 0 bytes, "", -1 -- before any device call."""
    import quadiron_amd
    lib = quadiron_amd.lib()
    assert lib.qi_gpu_locate_ctx_bytes(None, 4, 1) == 0
    assert lib.qi_gpu_locate_kernels(None, 4, 4096) == b""
    assert lib.qi_gpu_locate_ctx(None, None, 4, 1, None, None) == -1
    assert lib.qi_gpu_locate(None, None, 4, None, None, 0, 0, None, 0, 0, None, None, 0,
                             None, None, None, None, 0, 4096, 1, None) == -1
    assert lib.qi_fec_locate_blocks(None, None, None, None, None, 0, None, None, 0, 64) == -1
