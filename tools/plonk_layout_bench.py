#!/usr/bin/env python3
"""Time of Plonk's circuit layout on the GPU (czk_amd.plonk.layout) and of the assignment side (czk_amd.plonk.prover_inputs) at 2^--log gates (18: the
benchmark's Plonk size), split by phase, for a chain of alternating products and sums over --lanes share lanes.

  layout          wiring        plonk.wiring: host numpy on the gate arrays (slot layout, stable argsort, the permutation)
                  kernel        upload of succ and var_layout + czk_plonk_layout (w_evals on the 3 n wire slots, s_evals on the n gates)
                  transforms    the inverse transform of s on the radix-2 gate domain and of w on the mixed-radix wire domain
                  commitments   two G1 MSMs (n and 3 n scalars) and their conversion to affine
  prover_inputs   gather        czk_fr_gather of the assignment's lanes through var_layout (the assignment is on the device already)
                  transform     the inverse transform of the lanes on the wire domain
  numpy           the path the gather replaces, as marlin.prover_inputs does that step: numpy fancy indexing of the host assignment per lane + one upload

Each phase ends in a synchronisation (timings=...); the figure is the median of --reps runs after one warm-up run, and "total" is the wall time of a call
without the phase synchronisations.  One JSON object per line; --out PATH also writes the lines to PATH.

    python tools/plonk_layout_bench.py [--log 18] [--lanes 3] [--reps 3] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=18)
    ap.add_argument("--lanes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import czk_amd
    from czk_amd import plonk, polyvm
    from czk_amd.provers import rand_fr_canonical

    G = 1 << args.log
    W = 3 * G
    c = plonk.Circuit()
    u, v = c.new_pub_var("in"), c.new_var()
    for i in range(G):
        v = c.new_sum(v, u) if i & 1 else c.new_prod(v, v)
    c.publicize_var(v, "out")
    ctx = polyvm.shared_stream_context(czk_amd)
    B = polyvm.GpuBackend(czk_amd, ctx, args.lanes, W)                          # the layout commits polynomials of at most 3 n coefficients
    B.prepare([G, W])
    rows = []

    def report(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    ms = lambda laps, keys: {k + "_ms": round(med([t[k] for t in laps]) * 1e3, 3) for k in keys}   # noqa: E731

    def wall(fn):
        ctx.sync()
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        return r, time.perf_counter() - t0
    lay = plonk.layout(B, c)                                                    # warm-up: domain tables, table sets of these lengths
    laps, totals = [], []
    for _ in range(args.reps):
        t = {}
        plonk.layout(B, c, timings=t)
        laps.append(t)
        lay, dt = wall(lambda: plonk.layout(B, c))
        totals.append(dt)
    report(op="plonk.layout", log_gates=args.log, **ms(laps, ("wiring", "kernel", "transforms", "commitments")), total_ms=round(med(totals) * 1e3, 3))
    # the assignment: random share lanes (the values do not affect the work), on the device for the kernel and on the host for the numpy path
    host = np.stack([rand_fr_canonical(0x9A7 + ln, c.n_vars) for ln in range(args.lanes)])
    dev = B.upload(host)
    plonk.prover_inputs(B, lay, dev)
    laps, totals = [], []
    for _ in range(args.reps):
        t = {}
        plonk.prover_inputs(B, lay, dev, timings=t)
        laps.append(t)
        totals.append(wall(lambda: plonk.prover_inputs(B, lay, dev))[1])
    report(op="plonk.prover_inputs", log_gates=args.log, lanes=args.lanes, **ms(laps, ("gather", "transform")), total_ms=round(med(totals) * 1e3, 3))
    var_layout = lay["var_layout"].cpu().numpy().view(np.uint32)
    laps = []
    for _ in range(args.reps + 1):
        ctx.sync()
        t0 = time.perf_counter()
        picked = host[:, var_layout]
        t1 = time.perf_counter()
        up = B.upload(picked)
        ctx.sync()
        laps.append({"index": t1 - t0, "upload": time.perf_counter() - t1})
    assert np.array_equal(up.cpu().numpy().view(np.uint64)[:, :64], picked[:, :64])
    report(op="numpy fancy indexing + upload", log_gates=args.log, lanes=args.lanes, **ms(laps[1:], ("index", "upload")),
           total_ms=round(med([t["index"] + t["upload"] for t in laps[1:]]) * 1e3, 3))
    ctx.close()
    if args.out:
        open(args.out, "w").write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
