"""CPU: the compiler's resource report of the syndrome shares' kernels
(build/obj/syndrome.res for syndrome.hip): exactly the two context kernels and
the six syndrome_locate_kernel forms, none with scratch memory or a spilled
register."""
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


def test_syndrome_kernels_use_no_scratch():
    rep = _report(os.path.join(OBJ, "syndrome.res"))
    # syndrome_locate_kernel<RP, VEC>: RP in 2, 4, 8, both addressing forms
    want = {f"syndrome_locate_kernelILi{rp}ELb{v}E" for rp in (2, 4, 8) for v in (0, 1)}
    want |= {"19syndrome_ctx_kernelE", "26syndrome_locate_ctx_kernelE"}
    assert len(rep) == len(want), sorted(rep)
    for w in want:
        assert sum(w in k for k in rep) == 1, (w, sorted(rep))
    for k, v in rep.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
        assert v["SGPRs Spill"] == 0, (k, v)
        assert v["Dynamic Stack"] == 0 if "Dynamic Stack" in v else True
