#!/usr/bin/env python3
"""Wall-clock time of the Fec.* row calls on host buffers: what a caller of the
block API waits for, staging, copies, kernels and collection included.

One RS-FNT(16, 48) non-systematic stripe of 64 KiB blocks (its own encode),
four fragments missing, ten symbols of one present fragment corrupted:
  repair_blocks          the 4 missing fragments from the first k present
  update_blocks          2 data rows changed, all 64 coded rows held
  partial_repair_blocks  H = k helpers held, the same 4 targets
  syndrome_blocks        H = k + 4 listed fragments held, 4 checks
  locate_blocks          the first k + 8 present fragments listed
  locate_syndromes       over the rows syndrome_blocks returned, max_errors 2
  scrub_blocks           max_errors 2, detection only
Each call runs --warmup times, then --reps times; the figure is the median in
milliseconds.  Prints one JSON document.

    python tools/fec_rowcalls_rate.py [--reps 30]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import quadiron_amd as qa
    k, m, B, cap, R = 16, 48, 65536, 256, 4
    fec = qa.Fec(k, m, False)
    no = fec.n_outputs
    rng = np.random.default_rng(1)
    data = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(k)]
    par = [np.zeros(B, np.uint8) for _ in range(no)]
    oor = np.zeros((no, cap), np.uint32)
    cnt = np.zeros(no, np.uint32)
    vp = C.c_void_p
    assert qa.lib().qi_fec_encode_blocks(fec.h, qa.ptr_array(data), qa.ptr_array(par), B,
                                         oor.ctypes.data_as(vp), cnt.ctypes.data_as(vp), cap) == 0
    assert cnt.max() <= cap
    targets = [3, 17, 40, 63]
    missing = np.zeros(k + m, np.int32)
    missing[targets] = 1
    present = [f for f in range(k + m) if not missing[f]]
    helpers, listed = present[:k], present[:k + R]
    bad = par[present[5]].view(np.uint16)
    marked = set(int(c) for c in oor[present[5], :cnt[present[5]]])
    cols = [int(c) for c in rng.permutation(B // 2) if int(c) not in marked][:10]
    bad[cols] ^= 0x0101
    new = [rng.integers(0, 256, B, dtype=np.uint8) for _ in range(2)]
    upd = [r.copy() for r in par], oor.copy(), cnt.copy()

    def held(frs):
        return [par[f] for f in frs], np.ascontiguousarray(oor[frs]), np.ascontiguousarray(cnt[frs])

    h_rows, h_oor, h_cnt = held(helpers)
    l_rows, l_oor, l_cnt = held(listed)
    syn = fec.syndrome_blocks(listed, listed, l_rows, l_oor, l_cnt, R)
    calls = {
        "repair_blocks": lambda: fec.repair_blocks(None, par, oor, cnt, missing, targets),
        "update_blocks": lambda: fec.update_blocks([2, 9], [data[2], data[9]], new, upd[0],
                                                    upd[1], upd[2]),
        "partial_repair_blocks": lambda: fec.partial_repair_blocks(
            helpers, helpers, h_rows, h_oor, h_cnt, targets),
        "syndrome_blocks": lambda: fec.syndrome_blocks(listed, listed, l_rows, l_oor, l_cnt, R),
        "locate_blocks": lambda: fec.locate_blocks(None, par, oor, cnt, missing),
        "locate_syndromes": lambda: fec.locate_syndromes(listed, syn[0], syn[1], syn[2],
                                                         max_errors=2),
        "scrub_blocks": lambda: fec.scrub_blocks(None, par, oor, cnt, missing, max_errors=2),
    }
    rows = {}
    for name, call in calls.items():
        for _ in range(a.warmup):
            assert call() is not None or name == "update_blocks"
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t) * 1e3)
        rows[name + "_ms"] = {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}
    # the corrupt fragment is found by all three decisions
    assert fec.locate_blocks(None, par, oor, cnt, missing)[present[5]] == 10
    assert fec.scrub_blocks(None, par, oor, cnt, missing, max_errors=2)[present[5]] == 10
    assert len(fec.locate_syndromes(listed, syn[0], syn[1], syn[2], max_errors=2)[1]) == 10
    print(json.dumps({"what": "Fec.* row calls, RS-FNT(16, 48) non-systematic, 64 KiB blocks, "
                              "wall-clock ms per call", "build": qa.build_id(),
                      "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
