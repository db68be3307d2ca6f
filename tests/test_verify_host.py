"""CPU: the verify form of matrix_route (quadiron_amd/csrc/matrix_route.h).
The header is host-only: g++ compiles it into tests/host/test_verify_route.cpp
with the address and undefined-behaviour sanitizers, no GPU call."""
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
    out = str(tmp_path_factory.mktemp("vroute") / "test_verify_route")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "host", "test_verify_route.cpp"), "-o", out])
    return out


def _routes(exe, lines):
    """(err, kernels string) of each input line."""
    res = subprocess.run([exe], input="".join(ln + "\n" for ln in lines), capture_output=True,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    out = res.stdout.split("\n")[:-1]
    assert len(out) == len(lines)
    return [(int(o.split("|", 1)[0]), o.split("|", 1)[1]) for o in out]


def test_pinned_routes_unaffected(exe):
    """matrix_route with verify = false gives the pinned routes."""
    pins = []
    with open(os.path.join(HERE, "golden", "matrix_routes.txt")) as f:
        for ln in f:
            if not ln.startswith("#"):
                inp, want = ln.rstrip("\n").split(" | ")
                pins.append((inp, want))
    assert len(pins) >= 100
    for (inp, want), (err, got) in zip(pins, _routes(exe, [p[0] + " 0" for p in pins])):
        assert (err, got) == (0, want), inp
        assert "_verify" not in got


def _kernel_symbols(path):
    out = subprocess.run(["nm", "-DC", path], check=True, capture_output=True,
                         text=True).stdout
    return [ln.split(" ", 2)[2] for ln in out.splitlines() if " qi::" in ln]


def _sweep():
    """the sweep of tests/test_matrix_route.py over what a check produces:
    ids and a route table, input marks or none, output marks (the work
    buckets) always, one or two regions"""
    kins = [1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 320, 321, 384, 385, 640]
    rbs = [1, 3, 4, 5, 8, 9, 64]
    flags = [(in_, 1, 1, 1, two) for in_ in (0, 1) for two in (0, 1)]
    return [(f"{16 * rb} {kin} {w} {buf} {al} " + " ".join(map(str, f)), kin, rb)
            for kin, rb, w, buf, al, f in itertools.product(
                kins, rbs, (200, 1024, 2088), (0, 1), (1, 2, 4), flags)]


def test_every_verify_route_has_a_kernel(exe):
    """Every kernel of an error-free verify route is an instantiation the
    built library exports, under its _verify name; what a check can reach (at
    most 4 row blocks, k <= 256) is never refused."""
    if not os.path.exists(LIB):
        pytest.fail("libquadiron_amd.so not built")
    sweep = _sweep()
    routes = _routes(exe, [ln + " 1" for ln, _, _ in sweep])
    for (ln, kin, rb), (err, names) in zip(sweep, routes):
        if kin <= 256 and rb <= 4:
            assert err == 0, ln
    ok = {names for err, names in routes if err == 0}
    names = {n.replace(" (tail)", "") for r in ok for n in r.split(" + ")}
    assert len(names) > 25, names
    syms = _kernel_symbols(LIB)
    for name in sorted(names):
        assert "_verify" in name and "_both" not in name, name
        assert any("qi::" + name + "(" in s for s in syms), name


def test_verify_route_is_the_repair_route(exe):
    """A verify route is the route of the same launch with input and output
    marks (a repair), form for form: the two cannot drift."""
    sweep = [(ln, kin, rb) for ln, kin, rb in _sweep() if kin <= 256 and rb <= 4]
    ver = _routes(exe, [ln + " 1" for ln, _, _ in sweep])
    # the repair of the same shape: input marks on (the verify form is chosen
    # with or without them, the _both form only with)
    rep_lines = []
    for ln, _, _ in sweep:
        p = ln.split()
        p[5] = "1"
        rep_lines.append(" ".join(p) + " 0")
    rep = _routes(exe, rep_lines)
    for (ln, _, _), (ev, nv), (er, nr) in zip(sweep, ver, rep):
        assert ev == er == 0, ln
        if ln.split()[5] == "1":
            assert nv == nr.replace("_both", "_verify"), ln
        else:  # no input marks: no redo launch for the tail, the same kernels otherwise
            assert nv == nr.replace("_both", "_verify").replace(
                " + matrix_redo_kernel_verify", ""), ln
