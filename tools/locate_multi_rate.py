#!/usr/bin/env python3
"""Time the multi-fragment locate against the single locate on the same rows.

Shape (defaults): k = 16, m = 48, 32768 words per row, 4096 stripes,
non-systematic; the listed fragments are 0 .. k + R - 1; (R, t) = (4, 2) and
(8, 4).  Timed with HIP events on one stream in one process
(tools/verify_rate.py's `timed`): all series warm up together for at least
--warmup-ms of device work, then --steps rounds run them in turn; medians,
minima and maxima over the rounds.  The contexts are built once, outside the
timed region: both calls read the same one.
  sparse  4 stripes (0, S/4, S/2, 3S/4) have one bad column per 1024, all in
          fragment 3: qi_gpu_locate_multi against qi_gpu_locate at the same R
  dense   fragment 3 is bad in every column of every stripe, fragment 5 as
          well in one column per 1024: qi_gpu_locate_multi (every column runs
          the decoder; the fix list holds them all) against qi_gpu_locate,
          which locates the single errors and counts the double ones unlocated
Writes one JSON document (--out) and prints it.

    python tools/locate_multi_rate.py --out profiles/locate_multi_rate.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from verify_rate import timed  # noqa: E402


def run(qa, torch, np, k, m, S, P, shapes, steps, warmup):
    plan = qa.Plan(k, m, False)
    no, cap = plan.n_outputs, 64
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randint(-32768, 32768, (S, k, P), dtype=torch.int16, device="cuda",
                         generator=g)
    coded = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    plan.encode(data, coded, counts, entries, cap)
    torch.cuda.synchronize()
    del data
    bad_stripes = sorted({0, S // 4, S // 2, 3 * S // 4})
    bad_cols = torch.arange(512, P, 1024, device="cuda")
    nbad = len(bad_cols)
    fix_cap = P + 64
    fixes = torch.zeros(S * fix_cap * 3, dtype=torch.int32, device="cuda")
    series, names, outs = [], [], {}
    for R, t in shapes:
        N = k + R
        ids = torch.from_numpy(np.tile(np.arange(N), (S, 1)).astype(np.uint16)
                               .view(np.int16)).cuda()
        ctx = torch.zeros(plan.locate_ctx_bytes(R, S), dtype=torch.uint8, device="cuda")
        plan.locate_ctx(ids, ctx)
        o = {n: torch.zeros(sz, dtype=torch.int32, device="cuda")
             for n, sz in (("loc", S * N), ("unl", S), ("wts", S * 4), ("cnt", S))}
        outs[(R, t)] = o

        def single(R=R, ctx=ctx, o=o):
            plan.locate(ctx, R, coded, o["loc"], o["unl"], o["cnt"], fixes, fix_cap,
                        counts=counts, entries=entries, cap=cap, check=False)

        def multi(R=R, t=t, ctx=ctx, o=o):
            plan.locate_multi(ctx, R, t, coded, o["loc"], o["unl"], o["wts"], o["cnt"], fixes,
                              fix_cap, counts=counts, entries=entries, cap=cap, check=False)
        series += [[single], [multi]]
        names += [(R, t, "single"), (R, t, "multi")]
    torch.cuda.synchronize()

    def measure(tag):
        res = timed(torch, series, steps, warmup)
        assert plan.take_error() == 0
        rows = []
        for (R, t, which), (_, ts) in zip(names, res):
            N = k + R
            rows.append({"case": tag, "checks": R, "max_errors": t, "call": which,
                         "kernels": (plan.locate_kernels(R, P) if which == "single"
                                     else plan.locate_multi_kernels(R, t, P)),
                         "ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts),
                         "row_bytes": S * N * P * 2,
                         "rows_gbps": S * N * P * 2 / statistics.median(ts) / 1e6})
        return rows

    # sparse
    for s in bad_stripes:
        coded[s, 3, bad_cols] += 1
    rows = measure("sparse")
    for (R, t), o in outs.items():       # the last run of each shape was `multi`
        N = k + R
        loc = o["loc"].cpu().numpy().reshape(S, N)
        assert (loc[bad_stripes, 3] == nbad).all() and loc.sum() == 4 * nbad
        assert int(o["unl"].sum()) == 0 and int(o["cnt"].sum()) == 4 * nbad
    # dense: every column of fragment 3 (a column whose symbol is marked stays
    # clean: the stored word under a mark is not read), fragment 5 per 1024
    for s in bad_stripes:
        coded[s, 3, bad_cols] -= 1
    coded[:, 3, :] += 1
    coded[:, 5, bad_cols] += 1
    marked = int(counts.cpu().numpy().reshape(S, no)[:, [3, 5]].sum())
    rows += measure("dense")
    for (R, t), o in outs.items():
        w = o["wts"].cpu().numpy().reshape(S, 4).sum(axis=0)
        assert int(o["unl"].sum()) == 0 and not w[2:].any()
        assert S * P - marked <= w[0] + w[1] <= S * P
        assert S * nbad - marked <= w[1] <= S * nbad
        assert int(o["cnt"].max()) <= fix_cap
    plan.close()
    return {"k": k, "m": m, "systematic": False, "stripes": S, "words": P,
            "bad_columns_per_1024": 1, "fix_cap": fix_cap, "series": rows}


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
    res = run(qa, torch, np, a.k, a.m, a.stripes, a.words, [(4, 2), (8, 4)], a.steps, a.warmup)
    doc = {"device": torch.cuda.get_device_name(0), "build": qa.build_id(),
           "steps": a.steps, "warmup_ms": a.warmup, "result": res}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
