#!/usr/bin/env python3
"""Time the fragment locate against what a caller had without it.

Shape (defaults): k = 16, m = 48, R = 4 syndromes, 32768 words per row, 4096
stripes, non-systematic and systematic; the listed fragments are 0 .. k + R -
1.  The rows are clean except in 4 stripes (0, S/4, S/2, 3S/4), which have one
bad column per 1024, all in fragment 3.  Timed with HIP events on one stream
in one process, as tools/verify_rate.py does (its `timed`): all series warm up
together for at least --warmup-ms of device work, then --steps rounds run them
in turn; every figure is the median over the rounds.
  (a)  locate context + locate
  (a4) the same with d_stripes listing only the 4 corrupted stripes
  (b)  repair context + qi_gpu_verify of the same k + R rows (basis 0 .. k - 1,
       checks k .. k + R - 1): reads the same bytes, writes no row
  (c)  what a caller had: k + R leave-one-out runs of (b), run i without
       fragment i (R - 1 checks) -- and still only per-row counts
Writes one JSON document (--out) and prints it.

    python tools/locate_rate.py --out profiles/locate_rate.json
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


def run(qa, torch, np, k, m, sys_, S, P, R, steps, warmup):
    plan = qa.Plan(k, m, bool(sys_))
    no, cap, N = plan.n_outputs, 64, k + R
    g = torch.Generator(device="cuda").manual_seed(1)
    data = torch.randint(-32768, 32768, (S, k, P), dtype=torch.int16, device="cuda",
                         generator=g)
    coded = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    plan.encode(data, coded, counts, entries, cap)
    torch.cuda.synchronize()
    # fragment 3 of the bad stripes: one symbol per 1024 columns, + 1 mod 2^16
    # (a clean symbol of 65535 or a marked one would make it no error; with
    # these seeds there is none, checked below through the counts)
    bad_stripes = sorted({0, S // 4, S // 2, 3 * S // 4})
    bad_cols = torch.arange(512, P, 1024, device="cuda")
    rows3 = data if sys_ else coded
    for s in bad_stripes:
        rows3[s, 3, bad_cols] += 1
    dd = data if sys_ else None

    def i16(a):
        return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).cuda()

    ids = i16(np.tile(np.arange(N), (S, 1)))
    lctx = torch.zeros(plan.locate_ctx_bytes(R, S), dtype=torch.uint8, device="cuda")
    located = torch.zeros(S * N, dtype=torch.int32, device="cuda")
    unloc = torch.zeros(S, dtype=torch.int32, device="cuda")
    fcnt = torch.zeros(S, dtype=torch.int32, device="cuda")
    fix_cap = 64
    fixes = torch.zeros(S * fix_cap * 3, dtype=torch.int32, device="cuda")
    ids4 = ids[:len(bad_stripes)].contiguous()
    list4 = torch.tensor(bad_stripes, dtype=torch.int32, device="cuda")
    out4 = [torch.zeros(n, dtype=torch.int32, device="cuda")
            for n in (4 * N, 4, 4, 4 * fix_cap * 3)]

    def a_ctx():
        plan.locate_ctx(ids, lctx)

    def a_locate():
        plan.locate(lctx, R, coded, located, unloc, fcnt, fixes, fix_cap, data=dd,
                    counts=counts, entries=entries, cap=cap, check=False)

    def a4_ctx():
        plan.locate_ctx(ids4, lctx)

    def a4_locate():
        plan.locate(lctx, R, coded, out4[0], out4[1], out4[2], out4[3], fix_cap, data=dd,
                    counts=counts, entries=entries, cap=cap, stripes=list4, check=False)

    # (b) and the k + R leave-one-out runs of (c)
    def verify_pair(basis, checks):
        Rv = len(checks)
        di, dc = i16(np.tile(basis, (S, 1))), i16(np.tile(checks, (S, 1)))
        ctx = torch.zeros(plan.repair_ctx_bytes(Rv, S, P), dtype=torch.uint8, device="cuda")
        work = torch.zeros(plan.verify_work_bytes(Rv, S, cap), dtype=torch.uint8, device="cuda")
        res = [torch.zeros(S * Rv, dtype=torch.int32, device="cuda") for _ in range(3)]

        def f_ctx():
            plan.repair_ctx(di, dc, ctx, P, counts, entries, cap)

        def f_verify():
            plan.verify(ctx, dc, coded, work, cap, res[0], res[1], res[2], data=dd,
                        counts=counts, entries=entries, cap=cap, check=False)
        return f_ctx, f_verify, res

    b_ctx, b_verify, b_res = verify_pair(np.arange(k), np.arange(k, N))
    loo = []
    for i in range(N):
        rest = [f for f in range(N) if f != i]
        loo.append(verify_pair(np.array(rest[:k]), np.array(rest[k:])))

    def c_all():
        for f_ctx, f_verify, _ in loo:
            f_ctx()
            f_verify()

    (pa, ta), (p4, t4), (pb, tb), (pc, tc) = timed(
        torch, [[a_ctx, a_locate], [a4_ctx, a4_locate], [b_ctx, b_verify], [c_all]], steps,
        warmup)
    assert plan.take_error() == 0
    # the last locate run was (a4): its outputs, then (a) once more
    nbad = len(bad_cols)
    o4 = out4[0].cpu().numpy().reshape(4, N)
    assert (o4[:, 3] == nbad).all() and o4.sum() == 4 * nbad and int(out4[1].sum()) == 0
    a_ctx()
    a_locate()
    torch.cuda.synchronize()
    loc = located.cpu().numpy().reshape(S, N)
    assert (loc[bad_stripes, 3] == nbad).all() and loc.sum() == 4 * nbad
    assert int(unloc.sum()) == 0 and int(fcnt.sum()) == 4 * nbad
    # (b) sees the same stripes (fragment 3 is in its basis: every check row)
    vm = b_res[0].cpu().numpy().reshape(S, R)
    assert (vm[bad_stripes] == nbad).all() and vm.sum() == 4 * nbad * R
    ma, m4, mb, mc = (statistics.median(t) for t in (ta, t4, tb, tc))
    return {
        "k": k, "m": m, "systematic": bool(sys_), "stripes": S, "words": P, "checks": R,
        "bad_stripes": bad_stripes, "bad_columns_per_stripe": nbad,
        "kernels": plan.locate_kernels(R, P),
        "a_locate_ms": ma, "a_ctx_ms": pa[0], "a_apply_ms": pa[1],
        "a_min_ms": min(ta), "a_max_ms": max(ta),
        "a4_listed_ms": m4, "a4_ctx_ms": p4[0], "a4_apply_ms": p4[1],
        "b_verify_ms": mb, "b_ctx_ms": pb[0], "b_apply_ms": pb[1],
        "b_min_ms": min(tb), "b_max_ms": max(tb),
        "c_leave_one_out_ms": mc, "c_runs": N,
        "a_over_b": ma / mb, "a_over_c": ma / mc,
        "row_bytes": S * N * P * 2, "a_apply_gbps": S * N * P * 2 / pa[1] / 1e6,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--words", type=int, default=32768)
    ap.add_argument("--stripes", type=int, default=4096)
    ap.add_argument("--checks", type=int, default=4)
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
        rows.append(run(qa, torch, np, a.k, a.m, s, a.stripes, a.words, a.checks, a.steps,
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
