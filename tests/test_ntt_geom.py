"""CPU: the LDS engine's launch geometry (quadiron_amd/csrc/ntt_geom.h), which
sizes every ntt_lds_kernel / ntt_eras_kernel launch and names the
instantiation a plan reports.  The header is host-only: plain g++ compiles it
into tests/host/test_ntt_geom.cpp, no GPU call.

The driver sweeps every k from 257 to 2047 with every n in {512, 1024, 2048},
n > k, that the engine takes (max(n, len_2k) <= 2048, every mode; or an
erasure shape, n - k <= 64, both completions) and fails at the first shape
where no geometry is found, the tile is not 8 .. 64 columns or not the widest
that fits, the LDS bytes differ from the driver's own count of what the kernels
carve out of LDS, they pass 160 KiB, they are within 80 KiB without the
two-workgroup form being reported (or the reverse), or a transform's radices
are not <= 32 with product N.  For the erasure shapes it also checks that reading the tables from global
memory would never gain the second workgroup: the reason ntt_eras_kernel has
no such form."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_geometry_of_every_lds_engine_code(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    out = str(tmp_path / "test_ntt_geom")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-Werror",
                           os.path.join(HERE, "host", "test_ntt_geom.cpp"), "-o", out])
    res = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.split("\n")[:-1]
    print(res.stdout)
    forms = {tuple(ln.split()) for ln in lines[:-1]}
    # (kernel, TWG, C2): every instantiation the library builds, and no other
    assert forms == {("ntt_lds_kernel", "0", "0"), ("ntt_lds_kernel", "1", "0"),
                     ("ntt_eras_kernel", "0", "0"), ("ntt_eras_kernel", "0", "1")}
    # 4 modes of 255 + 767 + 768 codes (n = 2048: k <= 1024), 2 completions
    # of 64 erasure shapes per n
    assert lines[-1] == "checked %d" % (4 * (255 + 767 + 768) + 2 * 3 * 64)
