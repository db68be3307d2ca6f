"""CPU: the compiler's resource report of the device patch's kernel
(build/obj/patch.res for patch.hip): exactly patch_kernel, without scratch
memory or a spilled register."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "build", "obj")


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


def test_patch_kernel_uses_no_scratch():
    rep = _report(os.path.join(OBJ, "patch.res"))
    assert len(rep) == 1, sorted(rep)
    (name, v), = rep.items()
    assert "12patch_kernelE" in name, name
    assert v["ScratchSize"] == 0, v
    assert v["VGPRs Spill"] == 0, v
    assert v["SGPRs Spill"] == 0, v
    assert v.get("Dynamic Stack", 0) == 0, v
