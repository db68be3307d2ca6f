"""CPU: the multi-fragment locate's entry points are exported, their ctypes
signatures load, the Python wrappers exist, and without a plan (no device)
the calls refuse instead of launching."""
import ctypes as C
import inspect


def test_locate_multi_symbols_and_signatures():
    import quadiron_amd
    lib = quadiron_amd.lib()
    for name in ("qi_gpu_locate_multi", "qi_gpu_locate_multi_kernels",
                 "qi_fec_locate_multi_blocks"):
        assert hasattr(lib, name), name
    assert lib.qi_gpu_locate_multi.restype is C.c_int
    assert len(lib.qi_gpu_locate_multi.argtypes) == 23
    assert lib.qi_gpu_locate_multi_kernels.restype is C.c_char_p
    assert len(lib.qi_gpu_locate_multi_kernels.argtypes) == 4
    assert lib.qi_fec_locate_multi_blocks.restype is C.c_int
    assert len(lib.qi_fec_locate_multi_blocks.argtypes) == 11


def test_python_wrappers_present():
    import quadiron_amd as qa
    assert callable(qa.Plan.locate_multi) and callable(qa.Plan.locate_multi_kernels)
    assert qa.Plan.LOCATE_MAX_ERRORS == 4
    p = inspect.signature(qa.Fec.locate_blocks).parameters
    assert p["max_errors"].default is None and p["correct"].default is False


def test_no_plan_launches_nothing():
    """A NULL plan or handle: "" and -1, before any device call; max_errors
    outside 1 .. 4 is refused by the block call before the handle is used."""
    import quadiron_amd
    lib = quadiron_amd.lib()
    assert lib.qi_gpu_locate_multi_kernels(None, 4, 2, 4096) == b""
    assert lib.qi_gpu_locate_multi(None, None, 4, 2, None, None, 0, 0, None, 0, 0, None, None,
                                   0, None, None, None, None, None, 0, 4096, 1, None) == -1
    for t in (2, 0, 5):
        assert lib.qi_fec_locate_multi_blocks(None, None, None, None, None, 0, None, t, None, 0,
                                              64) == -1
