#!/usr/bin/env python3
"""Time the delta update against what a caller runs without it.

Per configuration (k, m, code type, stripes, U changed rows; every coded row
updated, R = n_outputs; 32768 words per row = 64 KiB packets), three series:
  (a) update context + clear of the out counts + in-place update
  (b) the full qi_gpu_encode (with the clear of its counts) a caller has to
      run today -- it needs all k data rows on the device
  (c) a plain device copy that moves the update's (2 U + 2 R) * words * 2
      bytes per stripe (U + R rows read, U + R rows written): the floor
Timed with HIP events on one stream in one process.  The series warm up
together for at least --warmup-ms of device work (clocks ramped), then
--steps rounds run them in turn -- (a), (b), (c), (a), ... -- so none always
follows the same neighbour; every figure is the median over the rounds, with
the smallest and the largest.  Writes one JSON document (--out) and prints it.

    python tools/update_rate.py --out profiles/update_rate.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [
    # k, m, systematic, stripes, U
    (200, 56, 1, 64, 1),
    (200, 56, 1, 64, 4),
    (16, 48, 1, 4096, 1),
    (16, 48, 0, 4096, 1),
    (1000, 24, 1, 64, 1),
]


def timed(torch, series, steps, warmup_ms):
    """series: lists of functions.  Per series: (median, min, max) ms of each
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

    def stat(v):
        v = list(v)
        return {"median": statistics.median(v), "min": min(v), "max": max(v)}
    res = []
    for si, fns in enumerate(series):
        parts = [stat(ev[it][si][i].elapsed_time(ev[it][si][i + 1]) for it in range(steps))
                 for i in range(len(fns))]
        total = stat(ev[it][si][0].elapsed_time(ev[it][si][-1]) for it in range(steps))
        res.append((parts, total))
    return res


def run(qa, torch, np, k, m, sys_, S, U, P, steps, warmup):
    rng = np.random.default_rng(k + U + sys_)
    plan = qa.Plan(k, m, bool(sys_))
    no, cap = plan.n_outputs, 64
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randint(-32768, 32768, (S, k, P), dtype=torch.int16, device="cuda",
                         generator=g)
    coded = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    plan.encode(data, coded, counts, entries, cap)
    ids = np.stack([rng.choice(k, U, replace=False) for _ in range(S)]).astype(np.uint16)
    di = torch.from_numpy(ids.view(np.int16)).cuda()
    idx = torch.from_numpy(ids.astype(np.int64)).cuda()
    old = torch.gather(data, 1, idx[:, :, None].expand(S, U, P)).contiguous()
    new = torch.randint(-32768, 32768, (S, U, P), dtype=torch.int16, device="cuda",
                        generator=g)
    ctx = torch.zeros(plan.update_ctx_bytes(U, no, S), dtype=torch.uint8, device="cuda")
    oc = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    c2 = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    e2 = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    enc2 = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    src = torch.zeros((S, U + no, P), dtype=torch.int16, device="cuda")
    dst = torch.zeros_like(src)
    torch.cuda.synchronize()

    def a_ctx():
        plan.update_ctx(di, None, ctx)

    def a_apply():
        oc.zero_()
        plan.update(ctx, no, old, new, coded, None, counts=counts, entries=entries, cap=cap,
                    out_counts=oc, out_entries=oe, out_cap=cap, check=False)

    def b_encode():
        c2.zero_()
        plan.encode(data, enc2, c2, e2, cap)

    def c_copy():
        dst.copy_(src)

    (pa, ta), (_, tb), (_, tc) = timed(torch, [[a_ctx, a_apply], [b_encode], [c_copy]], steps,
                                       warmup)
    # (the rows drift away from the fixed in-buckets over the rounds: a mark
    # restored where the row no longer holds one is still a valid symbol)
    assert plan.take_error() == 0
    moved = (2 * U + 2 * no) * P * 2 * S
    return {
        "k": k, "m": m, "systematic": bool(sys_), "stripes": S, "words": P, "rows": U,
        "slots": no, "kernels": plan.update_kernels(U, no, P),
        "encode_kernels": plan.kernels(P).split("; ")[0],
        "update_bytes": moved, "encode_bytes": (k + no) * P * 2 * S,
        "a_update_ms": ta, "a_ctx_ms": pa[0], "a_apply_ms": pa[1],
        "b_encode_ms": tb, "c_copy_ms": tc,
        "a_over_b": ta["median"] / tb["median"], "a_over_c": ta["median"] / tc["median"],
        "a_apply_gb_s": moved / pa[1]["median"] / 1e6,
        "c_copy_gb_s": moved / tc["median"] / 1e6,
    }


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
    for i, (k, m, sys_, S, U) in enumerate(CONFIGS):
        if a.only is None or i in a.only:
            rows.append(run(qa, torch, np, k, m, sys_, S, U, a.words, a.steps, a.warmup))
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
