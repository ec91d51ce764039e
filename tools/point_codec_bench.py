#!/usr/bin/env python3
"""Points per second of czk_points_serialize / czk_points_deserialize, with czk_bases_check_subgroup on the same points as the yardstick.

Per group, encoding (compressed / uncompressed) and n: n points [k_i] G in device memory, bytes and outputs in device memory (CZK_MEM_DEVICE), so
the timed region is the library call plus czk_ctx_sync: the median wall-clock time of --reps calls after one warm-up call.  Decoding is timed
unchecked and checked; every decode is compared with the points it came from before its rate is reported.  The yardstick is
czk_bases_check_subgroup on a handle registered from the same points without window tables.  Last, keyio.groth16_pk_from_bytes (checked, host
bytes in, queries left on the GPU) for the squaring circuit with 2^--key-log constraints.  One JSON object per line.

    python tools/point_codec_bench.py [--logs 12,14,16,18,20] [--groups 1,2] [--reps 5] [--key-log 16]"""
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
    ap.add_argument("--logs", default="12,14,16,18,20")
    ap.add_argument("--groups", default="1,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--key-log", type=int, default=16)
    args = ap.parse_args()
    import numpy as np
    import torch
    import czk_amd
    from czk_amd import keyio
    from util import R_MOD, ints_to_limbs, rand_fr_canonical

    ts = torch.cuda.Stream()
    ctx = czk_amd.Context(0, ts.cuda_stream)
    dev = czk_amd.CZK_MEM_DEVICE
    logs = [int(v) for v in args.logs.split(",")]
    n_max = 1 << max(logs)
    with torch.cuda.stream(ts):
        k = torch.from_numpy(rand_fr_canonical(0xC0DEC, n_max).view(np.int64)).to("cuda")
    torch.cuda.synchronize()

    def timed(fn):
        fn()
        ctx.sync()
        out = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            out.append(time.perf_counter() - t0)
        return sorted(out)[len(out) // 2]

    for group in (int(g) for g in args.groups.split(",")):
        aw = 12 * group
        with torch.cuda.stream(ts):
            pts = torch.empty((n_max, aw), dtype=torch.int64, device="cuda")
            back = torch.empty((n_max, aw), dtype=torch.int64, device="cuda")
            inf = torch.zeros(n_max, dtype=torch.uint8, device="cuda")
            binf = torch.empty(n_max, dtype=torch.uint8, device="cuda")
            data = torch.empty(n_max * aw * 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.fixed_base_points(group, k.data_ptr(), out=pts.data_ptr(), n=n_max, mem=dev)
        ctx.sync()
        for log_n in logs:
            n = 1 << log_n
            bases = ctx.register_bases(group, pts.data_ptr(), inf.data_ptr(), n=n, mem=dev | czk_amd.CZK_MEM_NO_TABLES)
            t = timed(lambda: bases.check_subgroup())
            assert bases.check_subgroup() == 0
            bases.release()
            print(json.dumps({"group": group, "n": n, "op": "czk_bases_check_subgroup", "ms": round(t * 1e3, 3), "points_per_s": round(n / t)}), flush=True)
            for compressed in (True, False):
                t = timed(lambda: ctx.points_serialize(group, pts.data_ptr(), inf.data_ptr(), compressed, n=n, out=data.data_ptr(), mem=dev))
                row = {"group": group, "n": n, "compressed": compressed}
                print(json.dumps({**row, "op": "encode", "ms": round(t * 1e3, 3), "points_per_s": round(n / t)}), flush=True)
                for checked in (False, True):
                    t = timed(lambda: ctx.points_deserialize(group, data.data_ptr(), n, compressed, checked, out=back.data_ptr(), out_inf=binf.data_ptr(),
                                                             count=False, mem=dev))
                    with torch.cuda.stream(ts):
                        same = bool(torch.equal(back[:n], pts[:n])) and int(binf[:n].sum().item()) == 0
                    assert same, f"group {group}, n {n}, compressed {compressed}, checked {checked}: decode(encode(P)) != P"
                    print(json.dumps({**row, "op": "decode_checked" if checked else "decode_unchecked", "ms": round(t * 1e3, 3), "points_per_s": round(n / t)}),
                          flush=True)
        del pts, back, data

    if args.key_log:
        from czk_amd.keygen import groth16_setup
        N = (1 << args.key_log) - 2                                   # the squaring circuit: N constraints + 2 instance rows fill the domain
        one = ints_to_limbs([(1 << 256) % R_MOD], 4)[0]
        csr = lambda cols: (np.arange(N + 1, dtype=np.uint64), np.array(cols, dtype=np.uint32), np.tile(one, (N, 1)))   # noqa: E731
        ab = [2 + i for i in range(N)]
        c = [3 + i for i in range(N - 1)] + [1]
        t0 = time.perf_counter()
        key = groth16_setup(ctx, csr(ab), csr(ab), csr(c), 2, N, [7, 11, 13, 17, 19])
        t_setup = time.perf_counter() - t0
        blob = {}
        for compressed in (True, False):
            t0 = time.perf_counter()
            blob[compressed] = keyio.groth16_pk_to_bytes(ctx, key, compressed)
            t_enc = time.perf_counter() - t0
            t0 = time.perf_counter()
            got = keyio.groth16_pk_from_bytes(ctx, blob[compressed], compressed, checked=True, to_host=False)
            ctx.sync()
            t_dec = time.perf_counter() - t0
            assert np.array_equal(got["a_query"][0].cpu().numpy().view(np.uint64), key["a_query"][0])
            points = sum(key[q][0].shape[0] for q in ("gamma_abc_g1", "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query")) + 6
            print(json.dumps({"op": "groth16_pk_from_bytes", "constraints": N, "compressed": compressed, "bytes": len(blob[compressed]), "points": points,
                              "setup_s": round(t_setup, 3), "pk_to_bytes_ms": round(t_enc * 1e3, 1), "pk_from_bytes_checked_ms": round(t_dec * 1e3, 1)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
