"""CPU: matrix_route (quadiron_amd/csrc/matrix_route.h), the one decision of
which kernels a matrix launch runs -- launch_matrix dispatches on it and
matrix_kernel_names prints it.  The header is host-only: plain g++ compiles
it into tests/host/test_matrix_route.cpp, no GPU call."""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "quadiron_amd", "libquadiron_amd.so")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ not found")
    out = str(tmp_path_factory.mktemp("route") / "test_matrix_route")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-Werror",
                           os.path.join(HERE, "host", "test_matrix_route.cpp"), "-o", out])
    return out


def _routes(exe, lines):
    """(err, kernels string) of each input line."""
    res = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = res.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [(int(o.split("|", 1)[0]), o.split("|", 1)[1]) for o in out]


def test_pinned_routes(exe):
    pins = []
    with open(os.path.join(HERE, "golden", "matrix_routes.txt")) as f:
        for ln in f:
            if not ln.startswith("#"):
                inp, want = ln.rstrip("\n").split(" | ")
                pins.append((inp, want))
    assert len(pins) >= 100
    for (inp, want), (err, got) in zip(pins, _routes(exe, [p[0] for p in pins])):
        assert (err, got) == (0, want), inp


def test_flat_routes_pinned():
    """buf = 0 routes are pinned at every KP of the dot2 kernel, as an encode,
    a decode with marks and a repair."""
    flat = {}
    with open(os.path.join(HERE, "golden", "matrix_routes.txt")) as f:
        for ln in f:
            if not ln.startswith("#") and ln.split()[3] == "0":
                flat.setdefault(ln.split(" | ")[1].strip(), []).append(ln)
    for kp in (2, 4, 8, 16, 32, 64, 128):
        assert f"matrix_kernel<{kp}, 1, false> (tail)" in flat, kp
        assert f"matrix_kernel<{kp}, 1, false> (tail) + matrix_redo_kernel" in flat, kp
        assert (f"matrix_kernel_both<{kp}, 1, false> (tail) + matrix_redo_kernel_both"
                in flat), kp


def _extent_table():
    rows = []
    with open(os.path.join(HERE, "golden", "row_extent.txt")) as f:
        for ln in f:
            if not ln.startswith("#"):
                inp, want = ln.split(" | ")
                rows.append((tuple(int(v) for v in inp.split()), int(want)))
    return rows


def test_row_extent_boundaries(tmp_path):
    """row_extent, which decides between the buffer and the flat kernels:
    2^31 - 2 bytes is an extent, 2^31 is not, no rows give 0, and a product
    past 2^62 does not wrap into a positive value."""
    table = _extent_table()
    args = {a for a, _ in table}
    assert {(1, 0, (1 << 30) - 1), (1, 0, 1 << 30), (0, 1024, 1024), (-1, 1024, 1024),
            (5, 1 << 62, 100)} <= args
    assert dict(table)[(1, 0, (1 << 30) - 1)] == (1 << 31) - 2
    out = str(tmp_path / "test_row_extent")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-Wall", "-Werror",
                           os.path.join(HERE, "host", "test_row_extent.cpp"), "-o", out])
    res = subprocess.run([out], input="".join("%d %d %d\n" % a for a, _ in table),
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    got = [int(v) for v in res.stdout.split()]
    assert got == [w for _, w in table], list(zip(table, got))


def test_row_extent_python_rule():
    """qi_testlib.row_extent, the rule the wide-row GPU tests state their
    preconditions with, gives the same table."""
    from qi_testlib import row_extent
    for a, want in _extent_table():
        assert row_extent(*a) == want, a


def _kernel_symbols(path):
    # (as tests/test_kernel_names.py)
    out = subprocess.run(["nm", "-DC", path], check=True, capture_output=True,
                         text=True).stdout
    return [ln.split(" ", 2)[2] for ln in out.splitlines() if " qi::" in ln]


def test_every_route_has_a_kernel(exe):
    """Every kernel of an error-free route is an instantiation the built
    library exports, over the class boundaries of kin (KP, KS), the row-block
    counts where the geometry changes, widths below a tile / whole tiles /
    tiles and a tail, and the flags the public entry points produce: an
    encode (no ids, no route table, no input marks, one region; output marks
    or none), a decode or a repair (ids and a route table; input marks or
    none; output marks only for a repair; one or two regions), each with rows
    in or out of buffer range at every alignment class."""
    if not os.path.exists(LIB):
        pytest.fail("libquadiron_amd.so not built")
    kins = [1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 320, 321, 384, 385, 640]
    rbs = [1, 3, 4, 5, 8, 9, 64]
    flags = [(0, out, 0, 0, 0) for out in (0, 1)]
    flags += [(in_, out, 1, 1, two) for in_ in (0, 1) for out in (0, 1) for two in (0, 1)]
    lines = [f"{16 * rb} {kin} {w} {buf} {al} " + " ".join(map(str, f))
             for kin, rb, w, buf, al, f in itertools.product(
                 kins, rbs, (200, 1024, 2088), (0, 1), (1, 2, 4), flags)]
    routes = _routes(exe, lines)
    ok = {names for err, names in routes if err == 0}
    # (the shapes no entry point reaches are refused, not misnamed: input and
    # output marks on more than 4 row blocks or above k = 256, a tail above
    # k = 256)
    assert {err for err, _ in routes} == {0, -1, -3}
    names = {n.replace(" (tail)", "") for r in ok for n in r.split(" + ")}
    assert len(names) > 60, names
    syms = _kernel_symbols(LIB)
    for name in sorted(names):
        # (every name is complete here, so the argument list follows it)
        assert any("qi::" + name + "(" in s for s in syms), name
