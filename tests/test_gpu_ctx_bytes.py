"""GPU: the bytes of the matrix contexts (decode and repair, ctx.hip) against
tests/ctx_digests.json.  Decode, repair and verify check a context only
through what the kernels read from it; here every stripe's whole context
block, built over a buffer of 0xA5 bytes, must hash to the recorded digest and
the sticky error word must match -- which sections are written, which are
left alone, and every byte of both (tools/ctx_digest.py has the cases and
how the route table is kept independent of the order of its atomics).

The digests are re-recorded only by a change that means to change the
context layout."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ctx_digest  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in ctx_digest.CASES}
# the five context kernels; each must meet a row that needs the row scale
KERNELS = ("decode_ctx_lds_kernel<128>", "decode_ctx_lds_kernel<256>",
           "decode_ctx_kernel<1024, true>", "repair_ctx_kernel<64>", "repair_ctx_kernel<256>")


@pytest.fixture(scope="module")
def recorded():
    with open(ctx_digest.DIGESTS) as f:
        return json.load(f)["cases"]


def test_recorded_cases_are_the_table(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert {v["kernel"] for v in recorded.values()} == set(KERNELS)
    for name in KERNELS:
        assert any(v["kernel"] == name and CASES[n].scale
                   for n, v in recorded.items()), name


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.scale])
def test_scale_cases_need_a_row_scale(name):
    """CPU side: stripe 0 of the cases chosen for it really holds a row that
    needs the unit row scale."""
    assert ctx_digest.needs_scale(CASES[name]), name


@pytest.mark.parametrize("name", list(CASES))
def test_context_bytes(name, recorded, hip_lib):
    import torch
    import quadiron_amd as qa
    torch.cuda.set_device(0)
    got = ctx_digest.run_case(CASES[name], qa, torch)
    want = recorded[name]
    assert got["kernel"] == want["kernel"], (got["kernel"], want["kernel"])
    assert got["err"] == want["err"], (got["err"], want["err"])
    diff = [s for s, (g, w) in enumerate(zip(got["stripes"], want["stripes"])) if g != w]
    assert not diff and len(got["stripes"]) == len(want["stripes"]), (name, "stripes", diff)
