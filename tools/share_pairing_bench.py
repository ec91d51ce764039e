#!/usr/bin/env python3
"""Latency of czk_share_pairing (include/czk.h, csrc/pairing_share.hip) for SPDZ shares of 2 and 3 parties at n = 1 and at a batch that fills the GPU
(--threads pairing threads, L n of them per call) -- beside the same result COMPOSED from what existed before: the reference's formula
z / e(xa, y) / e(x, yb) * e(xa, yb) costs 2 L + 1 separate pairings per element, run here as ONE czk_pairing call over (2 L + 1) n pairs in device
memory.  The composition does the pairings only: the two opens, the scalings [mac_share_j] xa, the Fq12 inversions and products are left out -- every
simplification favours the composition.  Also czk_gt_share_open on the result.  The inputs are random subgroup points and gt powers, not consistent
sharings (the MAC checks fail and are counted): neither side's time depends on the values.  Each measurement: one warm-up, then --reps repetitions
between stream synchronisations; the median in ms.

One JSON line.

    python tools/share_pairing_bench.py [--reps 5] [--threads 65536] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(ctx, fn, reps):
    fn()
    ctx.sync()
    t = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=65536, help="pairing threads (L n) of the full batch")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import czk_amd as czk
    from czk_amd import polyvm
    from czk_amd.provers import rand_fr_canonical
    ctx = polyvm.shared_stream_context(czk)
    seed = [1]

    def scalars(n):
        seed[0] += 1
        return torch.from_numpy(rand_fr_canonical(0x5EED + seed[0], n).view(np.int64)).cuda()     # (canonical limbs read as Montgomery: still random elements)

    def points(group, n):
        aw = 12 if group == czk.CZK_G1 else 24
        gen = torch.from_numpy(ctx.fixed_base_points(group, np.array([[1, 0, 0, 0]], np.uint64))[0].view(np.int64).copy()).cuda()
        out, k = torch.empty((n, aw), dtype=torch.int64, device="cuda"), scalars(n)
        ctx.points_mul(group, gen.data_ptr(), k.data_ptr(), stride=0, scalar_form=czk.CZK_SCALAR_MONTGOMERY, n=n, out=out.data_ptr(), out_inf=None, mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        return out

    res = {"tool": "share_pairing_bench", "reps": a.reps, "results": []}
    for parties in (2, 3):
        L = 2 * parties
        mac = np.ascontiguousarray(rand_fr_canonical(3, parties))
        for n in (1, max(1, a.threads // L)):
            pa, tx, pb, ty = points(czk.CZK_G1, L * n), points(czk.CZK_G1, L * n), points(czk.CZK_G2, L * n), points(czk.CZK_G2, L * n)
            pairs = (2 * L + 1) * n
            g1, g2 = points(czk.CZK_G1, pairs), points(czk.CZK_G2, pairs)
            tz = torch.empty((L * n, 72), dtype=torch.int64, device="cuda")
            assert ctx._L.czk_pairing(ctx._h, C.c_void_p(g1.data_ptr()), None, C.c_void_p(g2.data_ptr()), None, C.c_size_t(L * n), C.c_void_p(tz.data_ptr()),
                                      C.c_int(czk.CZK_MEM_DEVICE)) == 0                                     # some gt elements for tz
            out = torch.empty((L * n, 72), dtype=torch.int64, device="cuda")
            gout = torch.empty((pairs, 72), dtype=torch.int64, device="cuda")
            opened = torch.empty((n, 72), dtype=torch.int64, device="cuda")
            fused = lambda: ctx.share_pairing(2, parties, mac, pa.data_ptr(), None, pb.data_ptr(), None, tx.data_ptr(), None, ty.data_ptr(), None, tz.data_ptr(),  # noqa: E731
                                              out.data_ptr(), n)

            def composed():
                rc = ctx._L.czk_pairing(ctx._h, C.c_void_p(g1.data_ptr()), None, C.c_void_p(g2.data_ptr()), None, C.c_size_t(pairs), C.c_void_p(gout.data_ptr()),
                                        C.c_int(czk.CZK_MEM_DEVICE))
                assert rc == 0
            row = {"scheme": f"spdz{parties}", "lanes": L, "n": n, "pairing_threads": L * n, "composed_pairs": pairs,
                   "share_pairing_ms": timed(ctx, fused, a.reps), "composed_pairings_ms": timed(ctx, composed, a.reps),
                   "gt_share_open_ms": timed(ctx, lambda: ctx.gt_share_open(2, parties, mac, out.data_ptr(), n, opened.data_ptr()), a.reps)}
            row["composed_over_fused"] = round(row["composed_pairings_ms"] / row["share_pairing_ms"], 3)
            res["results"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
