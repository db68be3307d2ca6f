#!/usr/bin/env python3
"""Time the fused fragment repair against what a caller runs without it.

Shape (defaults): k = 16, m = 48, 32768 words per row (64 KiB packets), 4096
stripes, non-systematic and systematic, R = 1 and R = 4 lost fragments.
Timed with HIP events on one stream in one process.  All three series warm
up together for at least --warmup-ms of device work (clocks ramped), then
--steps rounds run them in turn -- (a), (b), (c), (a), ... -- so none
always follows the same neighbour; every figure is the median over the
rounds.  (a)'s apply includes the clear of its output counters, which a
caller has to run too; (b) has no counterpart, a small bias against (a).
  (a) repair context + repair
  (b) decode context + decode
  (c) (b) followed by the full encode
with the per-kernel split of each (context / apply / encode).  Writes one
JSON document (--out) and prints it.

    python tools/repair_rate.py --out profiles/repair_rate.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, series, steps, warmup_ms):
    """series: lists of functions.  Per series: the median ms of each
    function (run back to back, in order) and of the whole sequence, the
    series taking turns within every round."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spent = 0.0
    while spent < warmup_ms:
        t0.record()
        for fns in series:
            for f in fns:
                f()
        t1.record()
        torch.cuda.synchronize()
        spent += t0.elapsed_time(t1)
    ev = [[[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)]
           for fns in series] for _ in range(steps)]
    for it in range(steps):
        for si, fns in enumerate(series):
            ev[it][si][0].record()
            for i, f in enumerate(fns):
                f()
                ev[it][si][i + 1].record()
    torch.cuda.synchronize()
    res = []
    for si, fns in enumerate(series):
        parts = [statistics.median(ev[it][si][i].elapsed_time(ev[it][si][i + 1])
                                   for it in range(steps)) for i in range(len(fns))]
        total = statistics.median(ev[it][si][0].elapsed_time(ev[it][si][-1])
                                  for it in range(steps))
        res.append((parts, total))
    return res


def run(qa, torch, np, k, m, sys_, S, P, R, steps, warmup):
    rng = np.random.default_rng(k + R + sys_)
    plan = qa.Plan(k, m, bool(sys_))
    no, cap = plan.n_outputs, 64
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randint(-32768, 32768, (S, k, P), dtype=torch.int16, device="cuda",
                         generator=g)
    coded = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    plan.encode(data, coded, counts, entries, cap)
    torch.cuda.synchronize()
    # per stripe: R lost fragments, k of the others received
    tg = np.stack([rng.choice(k + m, R, replace=False) for _ in range(S)])
    ids = np.stack([np.sort(rng.choice(np.setdiff1d(np.arange(k + m), tg[s]), k,
                                       replace=False)) for s in range(S)])
    di = torch.from_numpy(ids.astype(np.uint16).view(np.int16)).cuda()
    dt = torch.from_numpy(tg.astype(np.uint16).view(np.int16)).cuda()
    rctx = torch.zeros(plan.repair_ctx_bytes(R, S, P), dtype=torch.uint8, device="cuda")
    dctx = torch.zeros(plan.ctx_bytes(S, P), dtype=torch.uint8, device="cuda")
    rout = torch.zeros((S, R, P), dtype=torch.int16, device="cuda")
    dec = torch.zeros((S, k, P), dtype=torch.int16, device="cuda")
    enc2 = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * R * cap, dtype=torch.int32, device="cuda")
    c2 = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    e2 = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    dd = data if sys_ else None

    def a_ctx():
        plan.repair_ctx(di, dt, rctx, P, counts, entries, cap)

    def a_apply():
        oc.zero_()
        plan.repair(rctx, coded, rout, data=dd, counts=counts, entries=entries, cap=cap,
                    out_counts=oc, out_entries=oe, out_cap=cap, check=False)

    def b_ctx():
        plan.decode_ctx(di, dctx, P, counts, entries, cap)

    def b_apply():
        plan.decode(dctx, di, coded, dec, data=dd, counts=counts, entries=entries, cap=cap,
                    check=False)

    def c_encode():
        c2.zero_()
        plan.encode(dec, enc2, c2, e2, cap)

    (pa, ta), (pb, tb), (pc, tc) = timed(
        torch, [[a_ctx, a_apply], [b_ctx, b_apply], [b_ctx, b_apply, c_encode]], steps, warmup)
    assert plan.take_error() == 0
    return {
        "k": k, "m": m, "systematic": bool(sys_), "stripes": S, "words": P, "targets": R,
        "kernels": plan.repair_kernels(R, P),
        "a_repair_ms": ta, "a_ctx_ms": pa[0], "a_apply_ms": pa[1],
        "b_decode_ms": tb, "b_ctx_ms": pb[0], "b_apply_ms": pb[1],
        "c_decode_encode_ms": tc, "c_encode_ms": pc[2],
        "a_below_b": ta < tb,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--words", type=int, default=32768)
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--targets", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-ms", dest="warmup", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import quadiron_amd as qa
    torch.cuda.set_device(0)
    rows = [run(qa, torch, np, a.k, a.m, s, a.stripes, a.words, R, a.steps, a.warmup)
            for s in (0, 1) for R in a.targets]
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
