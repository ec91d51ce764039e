#!/usr/bin/env python3
"""Time of Context.fr_vec_commit (czk.h "czk tree commitment v1", csrc/commit_tree.hip) on vectors in device memory: n = 2^--log elements per lane for
each lane count of --lanes, the sizes of the SPDZ open's commit round (own vector: 1 lane; the W gathered vectors: W lanes).

  call_ms      device events on the context's stream around the call; the call ends in a synchronisation (upload of the randomness, the leaf / node /
               root kernels, download of the commitments), so this is what a caller waits for
  kernels_ms   the library's own event bracket around the kernels alone (profile entry "commit_tree")
  compressions SHA-256 compressions of the call, computed from n, E, F and the lane count: per leaf ceil((32 c + 9) / 64) for its c elements, the same
               per node for its c children, 2 for the root (the tag blocks are precomputed and not counted)

Median of --reps calls after one warm-up.  One JSON object per line; --out PATH also writes the lines to PATH.

    python tools/commit_tree_bench.py [--log 21] [--lanes 1,2,3,8] [--reps 5] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compressions(n: int, E: int, F: int) -> int:
    """of one lane: blocks hashed after the tag block, padding included"""
    def blocks(items):
        return (32 * items + 9 + 63) // 64
    total, m, per = 0, n, E
    while True:
        full, rest = divmod(m, per)
        total += full * blocks(per) + (blocks(rest) if rest or m == 0 else 0)
        m = max(1, full + (1 if rest else 0))
        if m == 1:
            break
        per = F
    return total + 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=21)
    ap.add_argument("--lanes", default="1,2,3,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import czk_amd
    from czk_amd import polyvm

    E, F = czk_amd.binding.CZK_COMMIT_LEAF_ELEMS, czk_amd.binding.CZK_COMMIT_FANOUT
    n = 1 << args.log
    lane_counts = [int(x) for x in args.lanes.split(",")]
    ctx = polyvm.shared_stream_context(czk_amd)
    # random limbs with the top limb below the modulus': values below r, read as Montgomery forms (the values do not affect the work)
    data = torch.randint(0, 2**62, (max(lane_counts), n, 4), dtype=torch.int64, device="cuda")
    data[:, :, 3] &= (1 << 60) - 1
    rows = []
    for lanes in lane_counts:
        rnd = os.urandom(32 * lanes)
        call, kern = [], []
        for rep in range(args.reps + 1):
            ctx.profile_enable(True)
            ctx.profile_reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = ctx.fr_vec_commit(data.data_ptr(), rnd, lanes=lanes, n=n, stride=n, mem=czk_amd.CZK_MEM_DEVICE)
            e1.record()
            e1.synchronize()
            if rep:
                call.append(e0.elapsed_time(e1))
                kern.append(ctx.profile_read("commit_tree")[0])
        ctx.profile_enable(False)
        assert len(out) == 32 * lanes and len({out[32 * k:32 * k + 32] for k in range(lanes)}) == lanes
        med = lambda xs: sorted(xs)[len(xs) // 2]   # noqa: E731
        comp = lanes * compressions(n, E, F)
        row = {"op": "fr_vec_commit", "log_n": args.log, "lanes": lanes, "E": E, "F": F, "compressions": comp, "call_ms": round(med(call), 4),
               "call_ms_min_max": [round(min(call), 4), round(max(call), 4)], "kernels_ms": round(med(kern), 4),
               "compressions_per_s": round(comp / (med(kern) * 1e-3)), "input_gb_per_s": round(lanes * n * 32 / (med(kern) * 1e-3) / 1e9, 1), "reps": args.reps}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.close()
    if args.out:
        open(args.out, "w").write("\n".join(json.dumps(r) for r in rows) + "\n")


if __name__ == "__main__":
    main()
