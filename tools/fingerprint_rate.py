#!/usr/bin/env python3
"""Time the fragment fingerprint against what a caller runs without it.

Shape (defaults): k = 16, m = 48, 32768 words per row, 4096 stripes,
non-systematic.  Timed with HIP events on one stream in one process, as
tools/repair_rate.py: the series warm up together for at least --warmup-ms of
device work, then --steps rounds run them in turn; every figure is the median
over the rounds.
  (a) the fingerprints of all 64 fragments, F = 1, 4 and 8 keys
  (b) repair context + qi_gpu_verify with R = 48 on the same stripes: what a
      caller has to run today to check a stripe
  (c) a plain device read of the same rows (torch.sum over the tensor): the
      floor
Writes one JSON document (--out) and prints it.

    python tools/fingerprint_rate.py --out profiles/fingerprint_rate.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from repair_rate import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--words", type=int, default=32768)
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-ms", dest="warmup", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import quadiron_amd as qa
    torch.cuda.set_device(0)
    k, m, S, P = a.k, a.m, a.stripes, a.words
    plan = qa.Plan(k, m, False)
    n, cap = plan.n_outputs, 64
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randint(-32768, 32768, (S, k, P), dtype=torch.int16, device="cuda",
                         generator=g)
    coded = torch.zeros((S, n, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S * n, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * n * cap, dtype=torch.int32, device="cuda")
    plan.encode(data, coded, counts, entries, cap)
    torch.cuda.synchronize()
    del data
    rng = np.random.default_rng(1)
    keys = rng.integers(1, 65537, (8, 3))
    ids = torch.from_numpy(np.tile(np.arange(n, dtype=np.uint16), (S, 1)).view(np.int16)).cuda()
    fp = torch.zeros((S, n, 8), dtype=torch.int32, device="cuda")
    work = torch.zeros(plan.fingerprint_work_bytes(n, 8, S, P), dtype=torch.uint8,
                       device="cuda")

    def fingerprint(F):
        return lambda: plan.fingerprint(ids, keys[:F], fp, work, coded=coded, counts=counts,
                                        entries=entries, cap=cap, check=False)

    # (b): the first k fragments are the basis, the other R = n - k are checked
    R = min(n - k, 64)
    basis = torch.from_numpy(np.tile(np.arange(k, dtype=np.uint16), (S, 1)).view(np.int16)).cuda()
    checks = torch.from_numpy(np.tile(np.arange(k, k + R, dtype=np.uint16),
                                      (S, 1)).view(np.int16)).cuda()
    rctx = torch.zeros(plan.repair_ctx_bytes(R, S, P), dtype=torch.uint8, device="cuda")
    vwork = torch.zeros(plan.verify_work_bytes(R, S, cap), dtype=torch.uint8, device="cuda")
    vm, mm, first = (torch.zeros(S * R, dtype=torch.int32, device="cuda") for _ in range(3))

    def b_ctx():
        plan.repair_ctx(basis, checks, rctx, P, counts, entries, cap)

    def b_verify():
        plan.verify(rctx, checks, coded, vwork, cap, vm, mm, first, counts=counts,
                    entries=entries, cap=cap, check=False)

    def c_read():
        torch.sum(coded, dtype=torch.int64)

    series = [[fingerprint(1)], [fingerprint(4)], [fingerprint(8)], [b_ctx, b_verify], [c_read]]
    (_, a1), (_, a4), (_, a8), (pb, tb), (_, tc) = timed(torch, series, a.steps, a.warmup)
    assert plan.take_error() == 0
    assert int(vm.sum()) == 0 and int(mm.sum()) == 0
    gb = S * n * P * 2 / 1e9
    doc = {"device": torch.cuda.get_device_name(0), "build": qa.build_id(), "steps": a.steps,
           "warmup_ms": a.warmup, "k": k, "m": m, "stripes": S, "words": P, "rows_gb": gb,
           "kernels": {F: plan.fingerprint_kernels(n, F, P) for F in (1, 4, 8)},
           "a_fingerprint_ms": {"1": a1, "4": a4, "8": a8},
           "a_fingerprint_gbps": {"1": gb / a1 * 1e3, "4": gb / a4 * 1e3, "8": gb / a8 * 1e3},
           "b_verify_ms": tb, "b_ctx_ms": pb[0], "b_apply_ms": pb[1],
           "c_read_ms": tc, "c_read_gbps": gb / tc * 1e3,
           "a_over_c": {"1": a1 / tc, "4": a4 / tc, "8": a8 / tc},
           "a_over_b": {"1": a1 / tb, "4": a4 / tb, "8": a8 / tb}}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
