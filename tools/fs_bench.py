#!/usr/bin/env python3
"""Times of the Fiat-Shamir transcript (csrc/fs.hip, czk_amd.transcript) with its state on the device against the same transcript on the host.

  fri     fri.prove(queries=0) at 2^log coefficients x --lanes lanes for every log of --logs: the FRI commit phase and the transcript's tail.
          "device" keeps the transcript's state on the GPU (roots absorbed from tree memory, alphas squeezed into device memory, czk_fr_fri_fold_at: one
          enqueued sequence and one wait); "host" is the same transcript in host memory through commit_phase's hook, one stop per round.  Host clock around
          the call, which ends synchronised (the index draws' read-back); the forms alternate run by run.  The proofs' roots and constants must be equal.
  absorb  one absorb of the lanes' 32-byte roots and one alpha: "device" = put_bytes from device memory, absorb, squeeze_fr into device memory, then a
          synchronise (three launches); "host" = the roots' read-back, then put_bytes, absorb, squeeze_fr on the host.  Host clock, `inner` in a row.

ms = median of --reps runs after one warm-up of each form, with the smallest and the largest.  One JSON object per line; --out PATH also writes them to PATH.

    python tools/fs_bench.py [--logs 10,21] [--lanes 2] [--reps 21] [--out PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="10,21")
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import czk_amd
    from czk_amd import fri
    from czk_amd.transcript import Transcript

    lanes = args.lanes
    ts = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(ts)
    ctx = czk_amd.Context(0, ts.cuda_stream)
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for log_n in [int(x) for x in args.logs.split(",") if x]:
        # limbs below r read as Montgomery forms: the values do not affect the work
        host = torch.randint(0, 2**62, (lanes, 1 << log_n, 4), dtype=torch.int64)
        host[:, :, 3] &= (1 << 60) - 1
        coeffs = ctx.lanes_alloc(lanes, 1 << log_n)
        for ln in range(lanes):
            coeffs.upload(host[ln].numpy().view("uint64"), lane=ln)
        secs, seen = {"device": [], "host": []}, {}
        for rep in range(args.reps + 1):
            for form in ("device", "host"):
                ctx.sync()
                t0 = time.perf_counter()
                proof = fri.prove(ctx, coeffs, queries=0, seed=b"bench", device=form == "device")
                dt = time.perf_counter() - t0
                if rep:
                    secs[form].append(dt)
                else:
                    seen[form] = (proof["roots"], proof["constant"])
        assert seen["device"] == seen["host"], "the two forms disagree"
        coeffs.free()
        for form, xs in secs.items():
            emit({"op": "fri_prove_commit_phase", "form": form, "log_coeffs": log_n, "lanes": lanes, "rounds": log_n, "ms": round(med(xs) * 1e3, 3),
                  "ms_min_max": [round(min(xs) * 1e3, 3), round(max(xs) * 1e3, 3)], "reps": args.reps})

    roots = torch.randint(0, 256, (lanes, 32), dtype=torch.uint8, device="cuda")
    alpha = torch.zeros(4, dtype=torch.int64, device="cuda")
    dev, hst = Transcript(ctx, device=True), Transcript()
    for t in (dev, hst):
        t.put_bytes(b"bench").seed()
    inner = 200

    def device_step():
        dev.put_bytes(roots.data_ptr(), 32 * lanes).absorb().squeeze_fr_mont(1, out=alpha.data_ptr())
        ctx.sync()

    def host_step():
        hst.put_bytes(roots.cpu().numpy()).absorb().squeeze_fr_mont(1)

    secs = {"device": [], "host": []}
    for rep in range(args.reps + 1):
        for form, step in (("device", device_step), ("host", host_step)):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(inner):
                step()
            if rep:
                secs[form].append((time.perf_counter() - t0) / inner)
    assert dev.state() == hst.state(), "the two forms disagree"
    for form, xs in secs.items():
        emit({"op": "absorb_roots_squeeze_alpha", "form": form, "lanes": lanes, "inner": inner, "us": round(med(xs) * 1e6, 2),
              "us_min_max": [round(min(xs) * 1e6, 2), round(max(xs) * 1e6, 2)], "reps": args.reps})
    dev.release()
    hst.release()
    ctx.close()
    if args.out:
        open(args.out, "w").write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
