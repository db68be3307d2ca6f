#!/usr/bin/env python3
"""Time the fused fragment verify against what a caller runs without it.

Shape (defaults): k = 16, m = 48, 32768 words per row (64 KiB packets), 4096
stripes, non-systematic and systematic, R = 4 and R = 48 check fragments
(basis: fragments 0 .. k - 1; checks: k .. k + R - 1, so the stored check
rows are one strided view for series (c)).  Timed with HIP events on one
stream in one process.  All series warm up together for at least --warmup-ms
of device work (clocks ramped), then --steps rounds run them in turn -- (a),
(b), (c), (a), ... -- so none always follows the same neighbour; every figure
is the median over the rounds, and (b)'s own spread (min / max over its
rounds) is the margin for a / b.
  (a) repair context + verify
  (b) repair context + repair into scratch rows
  (c) (b) followed by a device compare of the R rows,
      torch.ne(scratch, stored).sum() -- the cheapest check a caller has
      without the fused one, and it still ignores the marks
Writes one JSON document (--out) and prints it.

    python tools/verify_rate.py --out profiles/verify_rate.json
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
    function (run back to back, in order) and the whole sequence's ms of
    every round, the series taking turns within every round."""
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
        totals = [ev[it][si][0].elapsed_time(ev[it][si][-1]) for it in range(steps)]
        res.append((parts, totals))
    return res


def run(qa, torch, np, k, m, sys_, S, P, R, steps, warmup):
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
    ids = np.tile(np.arange(k), (S, 1))
    chk = np.tile(np.arange(k, k + R), (S, 1))
    di = torch.from_numpy(ids.astype(np.uint16).view(np.int16)).cuda()
    dc = torch.from_numpy(chk.astype(np.uint16).view(np.int16)).cuda()
    # the stored check rows, by slot
    first = 0 if sys_ else k
    stored = coded[:, first:first + R, :]
    ctx = torch.zeros(plan.repair_ctx_bytes(R, S, P), dtype=torch.uint8, device="cuda")
    work = torch.zeros(plan.verify_work_bytes(R, S, cap), dtype=torch.uint8, device="cuda")
    res = [torch.zeros(S * R, dtype=torch.int32, device="cuda") for _ in range(3)]
    rout = torch.zeros((S, R, P), dtype=torch.int16, device="cuda")
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * R * cap, dtype=torch.int32, device="cuda")
    dd = data if sys_ else None
    diff = []

    def f_ctx():
        plan.repair_ctx(di, dc, ctx, P, counts, entries, cap)

    def a_verify():
        plan.verify(ctx, dc, coded, work, cap, res[0], res[1], res[2], data=dd, counts=counts,
                    entries=entries, cap=cap, check=False)

    def b_repair():
        oc.zero_()
        plan.repair(ctx, coded, rout, data=dd, counts=counts, entries=entries, cap=cap,
                    out_counts=oc, out_entries=oe, out_cap=cap, check=False)

    def c_compare():
        diff[:] = [torch.ne(rout, stored).sum()]

    (pa, ta), (pb, tb), (pc, tc) = timed(
        torch, [[f_ctx, a_verify], [f_ctx, b_repair], [f_ctx, b_repair, c_compare]], steps,
        warmup)
    assert plan.take_error() == 0
    # clean rows: all three agree that nothing differs
    assert int(diff[0]) == 0
    assert int(res[0].ne(0).sum()) == 0 and int(res[1].ne(0).sum()) == 0
    assert int(res[2].ne(-1).sum()) == 0  # 0xFFFFFFFF
    ma, mb, mc = (statistics.median(t) for t in (ta, tb, tc))
    return {
        "k": k, "m": m, "systematic": bool(sys_), "stripes": S, "words": P, "checks": R,
        "kernels": plan.verify_kernels(R, P),
        "a_verify_ms": ma, "a_ctx_ms": pa[0], "a_apply_ms": pa[1],
        "b_repair_ms": mb, "b_apply_ms": pb[1], "b_min_ms": min(tb), "b_max_ms": max(tb),
        "c_repair_compare_ms": mc, "c_compare_ms": pc[2],
        "a_over_b": ma / mb, "a_over_c": ma / mc,
        "a_below_c": ma < mc, "a_within_b_spread": ma <= max(tb),
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--words", type=int, default=32768)
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--checks", type=int, nargs="+", default=[4, 48])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup-ms", dest="warmup", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import quadiron_amd as qa
    torch.cuda.set_device(0)
    rows = []
    for s in (0, 1):
        for R in a.checks:
            rows.append(run(qa, torch, np, a.k, a.m, s, a.stripes, a.words, R, a.steps,
                            a.warmup))
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
