#!/usr/bin/env python3
"""SHA-256 digests of the matrix contexts the device builds (ctx.hip).

Nothing else looks at the bytes of a context: decode, repair and verify only
show what the kernels happen to read from one.  For every case of CASES the
context buffer is pre-filled with 0xA5 bytes, the contexts are built through
the public API (Plan.decode_ctx, decode_ctx_packed or repair_ctx), and each
stripe's whole context block is hashed, together with the sticky error word
-- so a section that is not written (the zero halves of the [a | 0] / [0 | b]
tiles at KS >= 4, the [b | a] tiles at KS >= 2, the `plain` / packed sections
of whole-tile widths, the NTT engine's half of a 256 < k context) is pinned
as much as one that is.

The route table is filled by atomics.  The marks are laid out so that its
bytes do not depend on their order: within a stripe every mark of one
1024-column route tile comes from one received row (one lane adds them, in
bucket order), 0 to 3 marks per tile, no bad ids, no tile above kRouteCap.

tests/ctx_digests.json holds the digests; tests/test_gpu_ctx_bytes.py
compares.  The file is recorded again only by a change that means to change
the context layout:

    python tools/ctx_digest.py --record tests/ctx_digests.json
    python tools/ctx_digest.py            # compare, print the differences
    python tools/ctx_digest.py --find-seeds   # CPU: the need-scale seeds
"""
import argparse
import hashlib
import json
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
DIGESTS = os.path.join(ROOT, "tests", "ctx_digests.json")

FILL = 0xA5
NO_ENTRY = 0xFFFFFFFF  # an unused bucket entry: past every width, skipped

# kind: "decode" (Plan.decode_ctx), "packed" (decode_ctx_packed) or "repair".
# buckets: build with the OOR buckets (else ids only: the unrouted table).
# scale: the seed of stripe 0's ids, found by --find-seeds: its matrix has a
#   row that needs the unit row scale (None: any ids).
# trunc: one bucket of stripe 2 claims more marks than the capacity (the
#   count clamp and kErrOorTruncated).
# stripes: 3, or "nb1": as many as make launch_decode_ctx choose one block
#   per stripe (CUs // 2 + 1), stripe s a copy of stripe s % 3.
Case = namedtuple("Case", "name kind k m sys words R buckets scale trunc stripes")


def _decode_cases():
    out = []

    def add(tag, k, m, words, scale=None, trunc=False, packed=True):
        for sys_ in (False, True):
            for buckets in (True, False):
                out.append(Case(f"{tag}_k{k}_w{words}_{'sys' if sys_ else 'nonsys'}_"
                                f"{'buckets' if buckets else 'ids'}", "decode", k, m, sys_,
                                words, 0, buckets, scale.get(sys_) if scale else None,
                                trunc and buckets and not sys_, 3))
        if packed:
            out.append(Case(f"{tag}_k{k}_w{words}_packed", "packed", k, m, False, words, 0,
                            True, None, False, 3))

    # decode_ctx_lds_kernel<128>: KS = 1 ([b | a] written) and KS = 2; a
    # width with a column tail (every section) and a whole-tile one
    add("lds128", 16, 48, 2088)
    add("lds128", 32, 32, 2088, scale={False: 8, True: 4}, trunc=True)
    add("lds128", 16, 48, 2048, packed=False)
    # decode_ctx_lds_kernel<256>: the 4-step chain with a remainder (k = 40)
    # and full (64), the two-slot A(x) chain (100), LDS above 64 KiB (128)
    add("lds256", 40, 24, 2088)
    add("lds256", 64, 64, 2088, scale={False: 1, True: 25}, trunc=True)
    add("lds256", 100, 28, 2088, packed=False)
    add("lds256", 128, 128, 2088, packed=False)
    add("lds256", 64, 64, 2048, packed=False)
    # decode_ctx_kernel<1024, true>, the dot2 form (a column tail)
    add("big_dot2", 130, 126, 1088, scale={False: 1, True: 4}, trunc=True)
    add("big_dot2", 256, 768, 1088, packed=False)
    # ... and the whole-tile form: 64-row chunks (KS = 16, 20), 32-row (40)
    add("big_tiles", 130, 126, 1024, scale={False: 1, True: 4})
    add("big_tiles", 256, 768, 1024, packed=False)
    add("big_tiles", 300, 212, 1024, packed=False)
    add("big_tiles", 600, 1400, 1024, packed=False)
    out.append(Case("big_tiles_k130_w1024_nonsys_buckets_nb1", "decode", 130, 126, False,
                    1024, 0, True, 1, False, "nb1"))
    return out


def _repair_cases():
    out = []
    for k, m, R, scale in ((16, 48, 1, False), (16, 48, 4, False), (16, 48, 16, True),
                           (64, 64, 17, False), (200, 56, 56, True), (256, 768, 64, False)):
        for sys_ in (False, True):
            out.append(Case(f"repair_k{k}_R{R}_{'sys' if sys_ else 'nonsys'}", "repair", k, m,
                            sys_, 2088, R, True, scale, R == 4 and not sys_, 3))
    return out


CASES = _decode_cases() + _repair_cases()


def _testlib():
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import qi_testlib
    return qi_testlib


def decode_ids(case, s, seed=None):
    """Stripe s's received ids, ascending (a permutation for the packed
    form, which takes its rows by position); systematic: data and parity."""
    k, n = case.k, case.k + case.m
    if seed is None:
        seed = case.scale if s == 0 and case.scale else 1000 + s
    rng = np.random.default_rng([case.k, case.m, int(case.sys), seed])
    if case.sys:
        nd = int(rng.integers(max(1, k - case.m), k))  # at least one of each
        ids = np.concatenate([rng.choice(k, nd, replace=False),
                              k + rng.choice(case.m, k - nd, replace=False)])
    else:
        ids = rng.choice(n, k, replace=False)
    return rng.permutation(ids) if case.kind == "packed" else np.sort(ids)


def inputs(case, n_outputs=None):
    """(ids [3, k] u16, targets [3, R] u16 or None, counts, entries, cap) of
    the case's three distinct stripes; counts / entries None for the cases
    built from the ids alone, and when n_outputs (the plan's bucket slots per
    stripe) is not given."""
    k = case.k
    ids, tgs = [], []
    for s in range(3):
        if case.kind == "repair":
            if s == 0 and case.scale:
                i, t, _ = _testlib().repair_case(k, case.m, int(case.sys), case.R,
                                                 bool(case.scale))
            else:
                rng = np.random.default_rng([k, case.m, int(case.sys), case.R, 1000 + s])
                t = rng.permutation(rng.choice(k + case.m, case.R, replace=False))
                i = np.sort(rng.choice(np.setdiff1d(np.arange(k + case.m), t), k,
                                       replace=False))
            ids.append(i)
            tgs.append(t)
        else:
            ids.append(decode_ids(case, s))
    ids = np.stack(ids).astype(np.uint16)
    tgs = np.stack(tgs).astype(np.uint16) if tgs else None
    if not case.buckets or n_outputs is None:
        return ids, tgs, None, None, 0
    by_pos = case.kind == "packed"
    base = k if case.sys and not by_pos else 0
    slots = k if by_pos else n_outputs
    ntiles = (case.words + 1023) // 1024
    bk = [[[] for _ in range(slots)] for _ in range(3)]
    for s in range(3):
        # the rows that have a bucket: every position, or the ids from base on
        rows = np.arange(k) if by_pos else np.flatnonzero(ids[s] >= base)
        for t in range(ntiles):
            width = min(1024, case.words - 1024 * t)
            row = rows[(s + 5 * t) % len(rows)]
            slot = row if by_pos else int(ids[s, row]) - base
            for e in range((s + t) % 4):
                bk[s][slot].append(1024 * t + (37 * s + 211 * e + 5 * t) % width)
        if s == 1:  # a mark past the width: skipped
            bk[s][int(rows[0]) if by_pos else int(ids[s, rows[0]]) - base].append(case.words + 5)
    cap = max(8, max(len(b) for st in bk for b in st))
    counts = np.zeros((3, slots), np.uint32)
    entries = np.full((3, slots, cap), NO_ENTRY, np.uint32)
    for s in range(3):
        for sl, b in enumerate(bk[s]):
            counts[s, sl] = len(b)
            entries[s, sl, :len(b)] = b
    if case.trunc:
        sl = int(np.flatnonzero(counts[2])[0])
        counts[2, sl] = cap + 2
    return ids, tgs, counts, entries, cap


def n_stripes(case, torch):
    if case.stripes == "nb1":
        return torch.cuda.get_device_properties(0).multi_processor_count // 2 + 1
    return case.stripes


def run_case(case, qa, torch):
    """{"err": sticky error word, "kernel": the context builder the plan
    reports, "stripes": [sha256 hex of stripe s's context block]}; an "nb1"
    case returns its stripes folded: 3 digests, after checking that stripe s
    equals stripe s % 3."""
    S = n_stripes(case, torch)
    rep = [s % 3 for s in range(S)]
    plan = qa.Plan(case.k, case.m, case.sys)
    ids3, tgs3, counts3, entries3, cap = inputs(case, plan.n_outputs)
    plan.take_error()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    di = dev(ids3[rep].view(np.int16))
    counts = entries = None
    if counts3 is not None:
        counts = dev(counts3[rep].view(np.int32).reshape(-1))
        entries = dev(entries3[rep].view(np.int32).reshape(-1))
    if case.kind == "repair":
        nbytes = plan.repair_ctx_bytes(case.R, S, case.words)
        kernel = plan.repair_kernels(case.R, case.words).split("=", 1)[1].split(" + ")[0]
    else:
        nbytes = plan.ctx_bytes(S, case.words)
        kernel = plan.kernels(case.words).split("; ")[1].split("=", 1)[1].split(" + ")[0]
    assert nbytes > 0 and nbytes % S == 0, (case.name, nbytes)
    ctx = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    if case.kind == "repair":
        plan.repair_ctx(di, dev(tgs3[rep].view(np.int16)), ctx, case.words, counts, entries, cap)
    elif case.kind == "packed":
        plan.decode_ctx_packed(di, ctx, case.words, counts, entries, cap)
    else:
        plan.decode_ctx(di, ctx, case.words, counts, entries, cap)
    torch.cuda.synchronize()
    err = int(plan.take_error())
    blocks = ctx.cpu().numpy().reshape(S, nbytes // S)
    plan.close()
    dig = [hashlib.sha256(b.tobytes()).hexdigest() for b in blocks]
    if case.stripes == "nb1":
        assert all(dig[s] == dig[s % 3] for s in range(S)), case.name
        dig = dig[:3]
    return {"err": err, "kernel": kernel, "stripes": dig}


def needs_scale(case):
    """CPU: whether stripe 0's matrix has a row that needs the unit row scale
    (a residue the dot2 pairs or the i8 split cannot hold)."""
    tl = _testlib()
    if case.kind == "repair":
        M = tl.repair_case(case.k, case.m, int(case.sys), case.R, bool(case.scale))[2]
    else:
        M = tl.decode_matrix(case.k, case.m, int(case.sys), decode_ids(case, 0))
    return any(tl.row_scale(row) != 1 for row in M)


def find_seeds():
    tl = _testlib()
    seen = set()
    for case in CASES:
        if not case.scale or case.kind == "repair" or (case.k, case.m, case.sys) in seen:
            continue
        seen.add((case.k, case.m, case.sys))
        for seed in range(1, 1000):
            M = tl.decode_matrix(case.k, case.m, int(case.sys), decode_ids(case, 0, seed))
            if not tl.coef_ok_np(M).all():
                print(f"k={case.k} m={case.m} sys={case.sys}: seed {seed}")
                break


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", metavar="PATH", help="write the digests there")
    ap.add_argument("--find-seeds", action="store_true")
    a = ap.parse_args()
    if a.find_seeds:
        return find_seeds()
    import torch
    import quadiron_amd as qa
    torch.cuda.set_device(0)
    got = {c.name: run_case(c, qa, torch) for c in CASES}
    if a.record:
        doc = {"build": qa.build_id(), "device": torch.cuda.get_device_name(0), "cases": got}
        with open(a.record, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
        print(f"recorded {len(got)} cases from build {doc['build']}")
        return 0
    want = json.load(open(DIGESTS))["cases"]
    bad = [n for n in got if got[n] != want.get(n)]
    for n in bad:
        print("DIFFERS", n, got[n], want.get(n))
    print(f"{len(got) - len(bad)} of {len(got)} cases match {DIGESTS}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
