"""CPU: the compiler's resource report of the fragment fingerprint's kernels
(build/obj/fingerprint.res, written by quadiron_amd/csrc/Makefile): exactly
the eight forms of fingerprint_kernel, the table kernel and the finish kernel
are there, none uses scratch memory or spills a VGPR."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = os.path.join(ROOT, "build", "obj", "fingerprint.res")


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


def test_fingerprint_kernels_use_no_scratch():
    ks = _report(RES)
    # fingerprint_kernel<FP, VEC>, FP in 1, 2, 4, 8
    want = {f"fingerprint_kernelILi{fp}ELb{v}E" for fp in (1, 2, 4, 8) for v in (0, 1)}
    want |= {"fingerprint_tab_kernel", "fingerprint_finish_kernel"}
    assert {w for w in want if any(w in k for k in ks)} == want, sorted(ks)
    assert len(ks) == len(want), sorted(ks)
    for k, v in ks.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
