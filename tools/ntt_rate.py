#!/usr/bin/env python3
"""Time Plan.encode and Plan.decode of the general-k NTT engine's LDS kernels
(ntt_lds_kernel, ntt_eras_kernel) with HIP events; the library comes from
QI_LIB_PATH (A/B of kernel variants built by tools/ab_build.sh).  Prints one
JSON document: per shape the kernels the plan names, the median / min / max of
the timed windows in ms, and with --digest SHA-256 digests of the encode's
outputs, counts and per-bucket sorted mark lists and of the decode's output,
so that two libraries can be compared bit for bit on the same seeded input.

Every shape runs at 64 KiB packets (or the width given: one that is not a
multiple of 1024 keeps a 256 < k <= 640 code off the matrix cores), where
rows move as 16-byte pieces, and at one more column, where every lane moves
single symbols.
    python tools/ntt_rate.py [--digest] [k,m,sys,words ...]"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import quadiron_amd as qa

S = 2            # stripes
WINDOWS = 7      # timed windows per figure
WINDOW_MS = 40   # each about this long
WARM_MS = 300    # the GPU clock settles after a few tens of ms of load

SHAPES = [
    (1000, 24, 0, 32768),      # staged / global-table encode, two-pass erasure decode
    (1000, 24, 1, 32768),      # erasure encode and decode
    (600, 1400, 0, 32768 + 8), # ntt_lds_kernel<true> decode
    (300, 212, 0, 32768 + 8),  # ntt_lds_kernel<false>
    (2000, 48, 0, 32768),      # erasure decode with the second load + INTT_n
]


def timed(fn):
    """Median, min and max over WINDOWS windows of the time of one fn() in ms."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(n):
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    one = window(3)
    window(max(3, int(WARM_MS / one)))
    n = max(3, int(WINDOW_MS / one))
    ts = sorted(window(n) for _ in range(WINDOWS))
    return {"median_ms": round(ts[len(ts) // 2], 5), "min_ms": round(ts[0], 5),
            "max_ms": round(ts[-1], 5), "iters": n}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def run(k, m, sys_, P, digest):
    plan = qa.Plan(k, m, bool(sys_))
    no, cap = plan.n_outputs, 64 + P // 512
    gen = torch.Generator(device="cuda").manual_seed(k * 1000 + m + sys_)
    dd = torch.randint(0, 65536, (S, k, P), generator=gen, device="cuda",
                       dtype=torch.int32).to(torch.int16)
    rng = np.random.default_rng([k, m, sys_])
    ids = np.stack([np.sort(rng.choice(k + m, k, replace=False))
                    for _ in range(S)]).astype(np.uint16)
    di = torch.from_numpy(ids.view(np.int16)).cuda()
    out = torch.zeros((S, no, P), dtype=torch.int16, device="cuda")
    counts = torch.zeros(S * no, dtype=torch.int32, device="cuda")
    entries = torch.zeros(S * no * cap, dtype=torch.int32, device="cuda")
    plan.encode(dd, out, counts, entries, cap)
    ctx = torch.zeros(plan.ctx_bytes(S, P), dtype=torch.uint8, device="cuda")
    plan.decode_ctx(di, ctx, P, counts, entries, cap, h_ids=ids)
    dec = torch.zeros_like(dd)

    def decode():
        return plan.decode(ctx, di, out, dec, data=dd, counts=counts, entries=entries, cap=cap)

    assert decode() == 0
    torch.cuda.synchronize()
    assert plan.take_error() == 0 and torch.equal(dec, dd)
    row = {"kernels": plan.kernels(P)}
    if digest:
        cnt = counts.cpu().numpy().view(np.uint32)
        ent = entries.cpu().numpy().view(np.uint32).reshape(S * no, cap).copy()
        assert (cnt <= cap).all()
        ent[np.arange(cap)[None, :] >= cnt[:, None]] = 0xffffffff
        ent.sort(axis=1)
        row["digest"] = {"out": sha(out.cpu().numpy()), "counts": sha(cnt),
                         "marks": int(cnt.sum()), "sorted_entries": sha(ent),
                         "dec": sha(dec.cpu().numpy())}
    # the timed encodes count their marks into buckets of their own (which
    # fill up: entries past cap are dropped, as the protocol has it)
    c2, e2 = torch.zeros_like(counts), torch.zeros_like(entries)
    row["encode"] = timed(lambda: plan.encode(dd, out, c2, e2, cap))
    row["decode"] = timed(decode)
    assert plan.take_error() == 0
    return row


def main():
    args = [a for a in sys.argv[1:] if a != "--digest"]
    shapes = [tuple(int(v) for v in a.split(",")) for a in args] or SHAPES
    torch.cuda.set_device(0)
    doc = {"build": qa.build_id(), "device": torch.cuda.get_device_name(0), "stripes": S,
           "rows": {}}
    for k, m, sys_, P in shapes:
        for width in (P, P + 1):
            doc["rows"]["k%d_m%d_sys%d_w%d" % (k, m, sys_, width)] = run(
                k, m, sys_, width, "--digest" in sys.argv)
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
