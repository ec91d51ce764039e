#!/usr/bin/env python3
"""Times of the Merkle commitment of share vectors and of the collaborative FRI commit phase (csrc/merkle.hip, czk_amd.fri) on vectors in device memory.

  tree      czk_fr_merkle_commit's tree, n = 2^log leaves x --lanes lanes for every log of --logs, in both forms: "plain" is the product library's
            (one launch per level, merkle_tree_plain.h), "fused" the lab library's czk_lab_merkle_commit (one workgroup per subtree,
            lab/merkle_tree_fused.h).  Both contexts share one stream.  A sample is `inner` enqueue-only calls between two device events (inner chosen so
            that a sample hashes about 2^24 leaves: small trees are timed back to back, as FRI's late rounds run); the forms alternate sample by sample;
            ms = per call, median / min / max of --reps samples after one warm-up of each.  compressions = lanes (3n - 1).
  commit    fri.commit_phase at 2^--fri-log coefficients per lane: transforms, trees, root read-backs, folds; host clock around the call, which ends
            synchronised (the last constant's download).  Median of --reps.
  hashlib   the same tree on one host thread (hashlib over the serialized elements), once, at 2^--host-log leaves x --lanes lanes.

One JSON object per line; --out PATH also writes the lines to PATH.

    python tools/fri_bench.py [--logs 10,12,...,21] [--lanes 2] [--reps 7] [--fri-log 20] [--host-log 21] [--out PATH]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_tree_seconds(data: bytes) -> float:
    t0 = time.perf_counter()
    level = [hashlib.sha256(data[i:i + 32]).digest() for i in range(0, len(data), 32)]
    while len(level) > 1:
        level = [hashlib.sha256(level[i] + level[i + 1]).digest() for i in range(0, len(level), 2)]
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default=",".join(str(k) for k in range(10, 22)))
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--fri-log", type=int, default=20)
    ap.add_argument("--host-log", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import czk_amd
    from czk_amd import fri

    logs, lanes = [int(x) for x in args.logs.split(",") if x], args.lanes
    ts = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(ts)
    ctx, lab = czk_amd.Context(0, ts.cuda_stream), czk_amd.Context(0, ts.cuda_stream, lab=True)
    top = max(logs + [args.host_log]) if logs or args.host_log else 0
    # random limbs with the top limb below the modulus': values below r, read as Montgomery forms (the values do not affect the work)
    data = torch.randint(0, 2**62, (lanes, 1 << top, 4), dtype=torch.int64, device="cuda")
    data[:, :, 3] &= (1 << 60) - 1
    tree = torch.empty((lanes, (2 << top) - 1, 4), dtype=torch.int64, device="cuda")
    med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for log_n in logs:
        n = 1 << log_n
        inner = max(4, min(512, (1 << 24) // (n * lanes)))
        forms = {"plain": lambda: ctx.fr_merkle_commit(data.data_ptr(), lanes=lanes, n=n, stride=1 << top, tree=tree.data_ptr(), tree_stride=(2 << top) - 1,
                                                        roots=False, mem=czk_amd.CZK_MEM_DEVICE),
                 "fused": lambda: lab.lab_merkle_commit(data.data_ptr(), lanes, n, 1 << top, tree.data_ptr(), (2 << top) - 1)}
        ms = {name: [] for name in forms}
        digests = {}
        for rep in range(args.reps + 1):
            for name, call in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    call()
                e1.record()
                e1.synchronize()
                if rep:
                    ms[name].append(e0.elapsed_time(e1) / inner)
                else:
                    digests[name] = tree[:, 2 * n - 2].cpu().numpy().tobytes()
        assert digests["fused"] == digests["plain"], "the two forms disagree on the roots"
        comp = lanes * (3 * n - 1)
        for name in forms:
            emit({"op": "merkle_tree", "form": name, "log_n": log_n, "lanes": lanes, "inner": inner, "compressions": comp, "ms": round(med(ms[name]), 5),
                  "ms_min_max": [round(min(ms[name]), 5), round(max(ms[name]), 5)], "compressions_per_s": round(comp / (med(ms[name]) * 1e-3)), "reps": args.reps})
    if args.fri_log:
        coeffs = ctx.lanes_alloc(lanes, 1 << args.fri_log)
        host = data[:, :1 << args.fri_log].cpu().numpy().view("uint64")
        for ln in range(lanes):
            coeffs.upload(host[ln], lane=ln)
        secs = []
        for rep in range(args.reps + 1):
            ctx.sync()
            t0 = time.perf_counter()
            state = fri.commit_phase(ctx, coeffs)
            dt = time.perf_counter() - t0
            fri.release(state)
            if rep:
                secs.append(dt)
        coeffs.free()
        emit({"op": "fri_commit_phase", "log_coeffs": args.fri_log, "lanes": lanes, "rounds": args.fri_log, "ms": round(med(secs) * 1e3, 3),
              "ms_min_max": [round(min(secs) * 1e3, 3), round(max(secs) * 1e3, 3)], "reps": args.reps})
    if args.host_log:
        n = 1 << args.host_log
        canon = ctx.fr_into_repr(data[:, :n].cpu().numpy().view("uint64").reshape(-1, 4)).reshape(lanes, n, 4)
        secs = sum(host_tree_seconds(canon[ln].tobytes()) for ln in range(lanes))
        emit({"op": "merkle_tree", "form": "hashlib, one host thread", "log_n": args.host_log, "lanes": lanes, "ms": round(secs * 1e3, 1), "reps": 1})
    ctx.close()
    lab.close()
    if args.out:
        open(args.out, "w").write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
