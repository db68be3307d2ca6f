#!/usr/bin/env python3
"""Time the partial repair against a plain copy and against what a caller runs
without it.

Per configuration (k, m, code type, stripes, H held rows, R targets; 32768
words per row = 64 KiB packets), up to three series:
  (a) partial context + clear of the out counts + partial repair (no acc)
  (b) for H = k only, what rebuilds the same fragments today: the fused repair
      (context + clear + repair) at k <= 256, else decode context + decode +
      full encode (the targets are parities, one data row is lost too)
  (c) a plain device copy of the same (H + R) row units read + written
Timed with HIP events on one stream in one process; the series warm up together
for at least --warmup-ms, then --steps rounds run them in turn; every figure is
the median over the rounds, with the smallest and the largest (update_rate.py's
`timed`).  Writes one JSON document (--out) and prints it.

    python tools/partial_rate.py --out profiles/partial_rate.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from update_rate import timed  # noqa: E402

CONFIGS = [
    # k, m, systematic, stripes, H, R
    (200, 56, 1, 64, 8, 1),
    (200, 56, 1, 64, 8, 4),
    (200, 56, 1, 64, 200, 1),
    (200, 56, 1, 64, 200, 4),
    (1000, 24, 1, 64, 1000, 1),
    (1000, 24, 1, 64, 1000, 4),
    (16, 48, 1, 4096, 4, 1),
    (16, 48, 1, 4096, 4, 4),
]


def run(qa, torch, np, k, m, sys_, S, H, R, P, steps, warmup):
    plan = qa.Plan(k, m, bool(sys_))
    no, cap = plan.n_outputs, 64
    g = torch.Generator(device="cuda").manual_seed(1)
    # helpers: data rows 1 .. k - 1 and the last parity; targets: parities 0 .. R - 1
    ids = np.tile(np.concatenate([np.arange(1, k), [k + m - 1]]).astype(np.uint16), (S, 1))
    targets = np.tile(np.arange(k, k + R).astype(np.uint16), (S, 1))
    held = np.tile(np.arange(k - H, k).astype(np.uint16), (S, 1))   # the parity among them
    di, dh, dt = (torch.from_numpy(a.view(np.int16)).cuda() for a in (ids, held, targets))
    rows = torch.randint(-32768, 32768, (S, H, P), dtype=torch.int16, device="cuda", generator=g)
    out = torch.zeros((S, R, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S * H, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * H * cap, dtype=torch.int32, device="cuda")
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * R * cap, dtype=torch.int32, device="cuda")
    ctx = torch.zeros(plan.partial_ctx_bytes(H, R, S), dtype=torch.uint8, device="cuda")
    src = torch.zeros((S, H + R, P), dtype=torch.int16, device="cuda")
    dst = torch.zeros_like(src)

    def a_ctx():
        plan.partial_ctx(di, dh, dt, ctx)

    def a_apply():
        oc.zero_()
        plan.partial(ctx, rows, out, counts=counts, entries=entries, cap=cap, out_counts=oc,
                     out_entries=oe, out_cap=cap, check=False)

    def c_copy():
        dst.copy_(src)

    series = [[a_ctx, a_apply], [c_copy]]
    b_name = None
    if H == k:
        data = torch.randint(-32768, 32768, (S, k, P), dtype=torch.int16, device="cuda",
                             generator=g)
        coded = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
        cc = torch.zeros(S * no, dtype=torch.int32, device="cuda")
        ce = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
        plan.encode(data, coded, cc, ce, cap)
        if k <= 256:
            b_name = "repair"
            rctx = torch.zeros(plan.repair_ctx_bytes(R, S, P), dtype=torch.uint8, device="cuda")
            rout = torch.zeros((S, R, P), dtype=torch.int16, device="cuda")

            def b_ctx():
                plan.repair_ctx(di, dt, rctx, P, cc, ce, cap)

            def b_apply():
                oc.zero_()
                plan.repair(rctx, coded, rout, data=data, counts=cc, entries=ce, cap=cap,
                            out_counts=oc, out_entries=oe, out_cap=cap, check=False)
            series.append([b_ctx, b_apply])
        else:
            b_name = "decode + encode"
            dctx = torch.zeros(plan.ctx_bytes(S, P), dtype=torch.uint8, device="cuda")
            dec = torch.zeros((S, k, P), dtype=torch.int16, device="cuda")
            enc2 = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
            c2 = torch.zeros(S * no, dtype=torch.int32, device="cuda")
            e2 = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")

            def b_ctx():
                plan.decode_ctx(di, dctx, P, cc, ce, cap)

            def b_decode():
                plan.decode(dctx, di, coded, dec, data=data, counts=cc, entries=ce, cap=cap)

            def b_encode():
                c2.zero_()
                plan.encode(dec, enc2, c2, e2, cap)
            series.append([b_ctx, b_decode, b_encode])
    torch.cuda.synchronize()
    res = timed(torch, series, steps, warmup)
    assert plan.take_error() == 0
    (pa, ta), (_, tc) = res[0], res[1]
    moved = (H + R) * P * 2 * S
    doc = {
        "k": k, "m": m, "systematic": bool(sys_), "stripes": S, "words": P, "held": H,
        "targets": R, "kernels": plan.partial_kernels(H, R, P), "row_bytes": moved,
        "a_partial_ms": ta, "a_ctx_ms": pa[0], "a_apply_ms": pa[1], "c_copy_ms": tc,
        "a_over_c": ta["median"] / tc["median"],
        "a_apply_gb_s": moved / pa[1]["median"] / 1e6, "c_copy_gb_s": 2 * moved / tc["median"] / 1e6,
    }
    if b_name:
        pb, tb = res[2]
        doc.update({"b": b_name, "b_ms": tb, "b_parts_ms": pb,
                    "a_over_b": ta["median"] / tb["median"]})
    return doc


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--words", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-ms", dest="warmup", type=float, default=400.0)
    ap.add_argument("--only", type=int, nargs="+", default=None,
                    help="indices into the configuration list")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import quadiron_amd as qa
    torch.cuda.set_device(0)
    rows = []
    for i, (k, m, sys_, S, H, R) in enumerate(CONFIGS):
        if a.only is None or i in a.only:
            rows.append(run(qa, torch, np, k, m, sys_, S, H, R, a.words, a.steps, a.warmup))
            torch.cuda.empty_cache()
    doc = {"device": torch.cuda.get_device_name(0), "build": qa.build_id(),
           "steps": a.steps, "warmup_ms": a.warmup, "results": rows}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
