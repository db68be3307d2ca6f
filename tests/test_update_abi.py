"""CPU: the delta update's entry points are exported and wrapped, and the
compiler's resource report of its kernels (build/obj/update.res for
update.hip, update_ctx_kernel's entry in build/obj/ctx.res) shows no scratch
memory and no spilled VGPR."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "build", "obj")


def test_update_symbols_exported():
    import quadiron_amd
    lib = quadiron_amd.lib()
    for name in ("qi_gpu_update_ctx_bytes", "qi_gpu_update_ctx", "qi_gpu_update",
                 "qi_gpu_update_kernels", "qi_fec_update_blocks"):
        assert hasattr(lib, name), name


def test_python_wrappers_present():
    import quadiron_amd as qa
    for name in ("update_ctx_bytes", "update_ctx", "update", "update_kernels"):
        assert callable(getattr(qa.Plan, name)), name
    assert callable(qa.Fec.update_blocks)
    assert qa.Plan.UPDATE_MAX_ROWS == 8


def _report(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (?:\S+:\d+:\d+: )?Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark: (?:\S+:\d+:\d+: )?\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur:
            out[cur][m.group(1).strip()] = int(m.group(2))
    return out


def test_update_kernels_use_no_scratch():
    upd = _report(os.path.join(OBJ, "update.res"))
    # update_kernel<UP, VEC>: UP in 1, 2, 4, 8, both addressing forms
    want = {f"update_kernelILi{up}ELb{v}E" for up in (1, 2, 4, 8) for v in (0, 1)}
    assert {w for w in want if any(w in k for k in upd)} == want, sorted(upd)
    ctx = {k: v for k, v in _report(os.path.join(OBJ, "ctx.res")).items()
           if "update_ctx_kernel" in k}
    assert len(ctx) == 1, sorted(ctx)
    for k, v in {**upd, **ctx}.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
        assert v["Dynamic Stack"] == 0 if "Dynamic Stack" in v else True
