#!/usr/bin/env python3
"""Time the syndrome shares against what the parent offers for the same rows
and against a plain copy.

Per configuration (k, m, systematic, stripes, H held rows, R checks, t, dirty;
32768 words per row = 64 KiB packets) over encoded stripes whose listed
fragments are the k data rows and the first R parities:
  (a) share context + clear of the out counts + share of the H held rows, and,
      for H = N, resolve context + resolve over the R syndrome rows
  (b) for H = N only, what a caller runs without it: locate context +
      qi_gpu_locate_multi at k <= 256, else decode context + decode + full
      encode (whose output the caller would then compare)
  (c) a plain device copy of the same (H + R) row units read + written
dirty: one listed data row is overwritten with random words, so every column
has one bad fragment and every lane runs the decoder; otherwise the stripes are
intact and the resolve leaves after its ballot.
Timed with HIP events on one stream in one process; the series warm up together
for at least --warmup-ms, then --steps rounds run them in turn; every figure is
the median over the rounds, with the smallest and the largest (update_rate.py's
`timed`).  Writes one JSON document (--out) and prints it.

    python tools/syndrome_rate.py --out profiles/syndrome_rate.json
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
    # k, m, systematic, stripes, H (0: all N), R, t, dirty
    (200, 56, 1, 64, 0, 4, 2, 0),
    (200, 56, 1, 64, 0, 4, 2, 1),
    (200, 56, 1, 64, 8, 4, 2, 0),
    (1000, 24, 1, 64, 0, 4, 2, 0),
    (1000, 24, 1, 64, 0, 4, 2, 1),
    (1000, 24, 1, 64, 8, 4, 2, 0),
]


def run(qa, torch, np, k, m, sys_, S, H, R, t, dirty, P, steps, warmup):
    plan = qa.Plan(k, m, bool(sys_))
    no, cap = plan.n_outputs, 64
    N = k + R
    whole = H == 0
    H = H or N
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randint(-32768, 32768, (S, k, P), dtype=torch.int16, device="cuda", generator=g)
    coded = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    cc = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    ce = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    plan.encode(data, coded, cc, ce, cap)
    if dirty:
        data[:, 1].copy_(torch.randint(-32768, 32768, (S, P), dtype=torch.int16, device="cuda",
                                       generator=g))
    # listed: data rows 0 .. k - 1, parities 0 .. R - 1; held: the last H of them
    ids = np.tile(np.arange(N).astype(np.uint16), (S, 1))
    held = np.tile(np.arange(N - H, N).astype(np.uint16), (S, 1))
    di, dh = (torch.from_numpy(a.view(np.int16)).cuda() for a in (ids, held))
    listed = torch.cat([data, coded[:, :R]], dim=1)
    rows = listed[:, N - H:].contiguous()
    counts = torch.zeros((S, N), dtype=torch.int32, device="cuda")
    entries = torch.zeros((S, N, cap), dtype=torch.int32, device="cuda")
    counts[:, k:] = cc.view(S, no)[:, :R]
    entries[:, k:] = ce.view(S, no, cap)[:, :R]
    counts = counts[:, N - H:].contiguous().view(-1)
    entries = entries[:, N - H:].contiguous().view(-1)
    del listed
    out = torch.zeros((S, R, P), dtype=torch.int16, device="cuda")
    oc = torch.zeros(S * R, dtype=torch.int32, device="cuda")
    oe = torch.zeros(S * R * cap, dtype=torch.int32, device="cuda")
    ctx = torch.zeros(plan.syndrome_ctx_bytes(H, R, S), dtype=torch.uint8, device="cuda")
    lctx = torch.zeros(plan.syndrome_locate_ctx_bytes(R, S), dtype=torch.uint8, device="cuda")
    fix_cap = 2 * P
    located = torch.zeros(S * N, dtype=torch.int32, device="cuda")
    unloc = torch.zeros(S, dtype=torch.int32, device="cuda")
    wts = torch.zeros(S * 4, dtype=torch.int32, device="cuda")
    fcnt = torch.zeros(S, dtype=torch.int32, device="cuda")
    fixes = torch.zeros(S * fix_cap * 3, dtype=torch.int32, device="cuda")
    src = torch.zeros((S, H + R, P), dtype=torch.int16, device="cuda")
    dst = torch.zeros_like(src)

    def a_ctx():
        plan.syndrome_ctx(di, dh, ctx)

    def a_share():
        oc.zero_()
        plan.syndrome(ctx, rows, out, counts=counts, entries=entries, cap=cap, out_counts=oc,
                      out_entries=oe, out_cap=cap, check=False)

    def a_lctx():
        plan.syndrome_locate_ctx(di, lctx)

    def a_resolve():
        plan.syndrome_locate(lctx, t, out, located, unloc, wts, fcnt, fixes, fix_cap, counts=oc,
                             entries=oe, cap=cap, check=False)

    def c_copy():
        dst.copy_(src)

    series = [[a_ctx, a_share] + ([a_lctx, a_resolve] if whole else []), [c_copy]]
    b_name = None
    if whole and k <= 256:
        b_name = "locate_multi"
        mctx = torch.zeros(plan.locate_ctx_bytes(R, S), dtype=torch.uint8, device="cuda")
        ml = torch.zeros(S * N, dtype=torch.int32, device="cuda")
        mu, mf = torch.zeros_like(unloc), torch.zeros_like(fcnt)
        mw, mx = torch.zeros_like(wts), torch.zeros_like(fixes)

        def b_ctx():
            plan.locate_ctx(di, mctx)

        def b_locate():
            plan.locate_multi(mctx, R, t, coded, ml, mu, mw, mf, mx, fix_cap, data=data,
                              counts=cc, entries=ce, cap=cap, check=False)
        series.append([b_ctx, b_locate])
    elif whole:
        b_name = "decode + encode"
        # (data row 0 not trusted: rows 1 .. k - 1 and the last parity)
        dids = torch.from_numpy(np.tile(np.concatenate([np.arange(1, k), [k + m - 1]])
                                        .astype(np.uint16), (S, 1)).view(np.int16)).cuda()
        dctx = torch.zeros(plan.ctx_bytes(S, P), dtype=torch.uint8, device="cuda")
        dec = torch.zeros((S, k, P), dtype=torch.int16, device="cuda")
        enc2 = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
        c2 = torch.zeros(S * no, dtype=torch.int32, device="cuda")
        e2 = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")

        def b_ctx():
            plan.decode_ctx(dids, dctx, P, cc, ce, cap)

        def b_decode():
            plan.decode(dctx, dids, coded, dec, data=data, counts=cc, entries=ce, cap=cap)

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
        "checks": R, "max_errors": t, "dirty": bool(dirty),
        "kernels": plan.syndrome_kernels(H, R, P), "row_bytes": moved,
        "a_ms": ta, "a_ctx_ms": pa[0], "a_share_ms": pa[1], "c_copy_ms": tc,
        "a_over_c": ta["median"] / tc["median"],
        "a_share_gb_s": moved / pa[1]["median"] / 1e6,
        "c_copy_gb_s": 2 * moved / tc["median"] / 1e6,
    }
    if whole:
        doc.update({"resolve_kernels": plan.syndrome_locate_kernels(R, t, P),
                    "a_resolve_ctx_ms": pa[2], "a_resolve_ms": pa[3],
                    "unlocated": int(unloc.sum()), "fixes": int(fcnt.sum())})
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
    for i, cfg in enumerate(CONFIGS):
        if a.only is None or i in a.only:
            rows.append(run(qa, torch, np, *cfg, a.words, a.steps, a.warmup))
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
