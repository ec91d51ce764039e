#!/usr/bin/env python3
"""czk_fixed_base_msm (windowed, one table per base) against czk_fixed_base_points (double-and-add over the generator) for the same scalars.

Per group: n = 2^log_n random canonical scalars in device memory, outputs in device memory (CZK_MEM_DEVICE), so the timed region is the
library call.  Reported per width: the table build (czk_fixed_base_create, blocking) and the multiplication (enqueue + czk_ctx_sync), each as
the wall-clock times of --reps calls after one warm-up call; the widths are the library's choice for n and its neighbours (--widths to
override).  The baseline is timed the same way.  Every result is compared with the baseline's on the device before its time is reported.
Prints one JSON object per (group, width) and per baseline.

    python tools/fixed_base_bench.py [--log-n 20] [--groups 1,2] [--widths 14,16,18] [--reps 5]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--widths", default="")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import czk_amd
    from util import rand_fr_canonical

    n = 1 << args.log_n
    ts = torch.cuda.Stream()
    ctx = czk_amd.Context(0, ts.cuda_stream)
    one = np.array([[1, 0, 0, 0]], dtype=np.uint64)
    with torch.cuda.stream(ts):
        k = torch.from_numpy(rand_fr_canonical(0xFB5, n).view(np.int64)).to("cuda")
    torch.cuda.synchronize()

    def timed(fn):
        fn()                                    # warm-up
        ctx.sync()
        out = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            out.append((time.perf_counter() - t0) * 1e3)
        return sorted(out)

    stats = lambda t: {"min_ms": round(t[0], 3), "median_ms": round(t[len(t) // 2], 3), "max_ms": round(t[-1], 3)}   # noqa: E731
    for group in (int(g) for g in args.groups.split(",")):
        aw = 12 * group
        with torch.cuda.stream(ts):
            want = torch.empty((n, aw), dtype=torch.int64, device="cuda")
            got = torch.empty((n, aw), dtype=torch.int64, device="cuda")
            inf = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        base_t = timed(lambda: ctx.fixed_base_points(group, k.data_ptr(), out=want.data_ptr(), n=n, mem=czk_amd.CZK_MEM_DEVICE))
        print(json.dumps({"group": group, "n": n, "path": "czk_fixed_base_points", **stats(base_t)}), flush=True)
        gen = ctx.fixed_base_points(group, one)[0]
        auto = ctx.fixed_base(group, gen, n_hint=n)
        chosen = auto.layout()[0]
        auto.release()
        widths = [int(w) for w in args.widths.split(",")] if args.widths else [w for w in (chosen - 2, chosen - 1, chosen, chosen + 1, chosen + 2) if 1 <= w <= 20]
        for w in widths:
            handles = []

            def create():
                handles.append(ctx.fixed_base(group, gen, window=w))
                if len(handles) > 1:
                    handles.pop(0).release()
            build_t = timed(create)
            fb = handles[0]
            mul_t = timed(lambda: ctx.fixed_base_msm(fb, k.data_ptr(), out=got.data_ptr(), n=n, mem=czk_amd.CZK_MEM_DEVICE, out_inf=inf.data_ptr()))
            with torch.cuda.stream(ts):
                same = bool(torch.equal(got, want)) and int(inf.sum().item()) == 0
            lw, lwin, lbytes = fb.layout()
            fb.release()
            assert same, f"group {group}, width {w}: the windowed result differs from czk_fixed_base_points"
            total = build_t[len(build_t) // 2] + mul_t[len(mul_t) // 2]
            print(json.dumps({"group": group, "n": n, "path": "czk_fixed_base_msm", "window": lw, "chosen": lw == chosen, "windows": lwin, "table_bytes": lbytes,
                              "table_build": stats(build_t), "msm": stats(mul_t), "build_plus_msm_median_ms": round(total, 3),
                              "speedup_vs_points_incl_build": round(base_t[len(base_t) // 2] / total, 2)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
