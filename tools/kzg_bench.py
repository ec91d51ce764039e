#!/usr/bin/env python3
"""Rates of the elementwise point arithmetic and of KZG10 verification on the GPU, beside the host path they replace.

  points_mul      czk_points_mul, G1 and G2, n = 2^--log-n points [k_i] G and random 253-bit scalars, everything in device memory: the timed region
                  is the call plus czk_ctx_sync, the median of --reps calls after one warm-up call.
  kzg10_check     czk_kzg10_check of --check-k honest openings (host arrays in, verdicts out: staging included), every verdict asserted.
  batch_check     czk_kzg10_batch_check of --batches batches of --batch-size openings each, same conditions.
  host path       what a caller had before: czk_jac_scalar_mul in a loop (host arithmetic, one point per call).  Timed over --host-sample calls per
                  group and scaled to the shapes above -- the full loops would take minutes: 2 G1 + 1 G2 multiplications per opening for check
                  (mod.rs:303-309), 3 G1 multiplications per opening for batch_check (:340-348); the pairings are not part of the host figure.

The openings come from the known-beta identity: C = [p(beta)] g, W = [(p(beta) - v) / (beta - z)] g for random p(beta), v, z.  One JSON object per
line; --write also replaces the table between the kzg_bench markers of EXPERIMENTS.md.

    python tools/kzg_bench.py [--log-n 16] [--check-k 4096] [--batches 1024] [--batch-size 8] [--reps 5] [--host-sample 64] [--write]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
Q_MOD = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
BEGIN, END = "<!-- kzg_bench:begin -->", "<!-- kzg_bench:end -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--check-k", type=int, default=4096)
    ap.add_argument("--batches", type=int, default=1024)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--write", action="store_true", help="replace the kzg_bench table of EXPERIMENTS.md")
    args = ap.parse_args()
    import random
    import numpy as np
    import torch
    import czk_amd
    from czk_amd import kzg
    from util import R_MOD, ints_to_limbs, rand_fr_canonical

    ts = torch.cuda.Stream()
    ctx = czk_amd.Context(0, ts.cuda_stream)
    dev = czk_amd.CZK_MEM_DEVICE
    rows = []

    def report(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def timed(fn, reps=args.reps):
        fn()
        ctx.sync()
        out = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            out.append(time.perf_counter() - t0)
        return sorted(out)[len(out) // 2]

    # ---- czk_points_mul against czk_jac_scalar_mul
    n = 1 << args.log_n
    host_us = {}
    for group in (1, 2):
        aw = 12 * group
        with torch.cuda.stream(ts):
            k = torch.from_numpy(rand_fr_canonical(0x4B5A + group, n).view(np.int64)).to("cuda")
            s = torch.from_numpy(rand_fr_canonical(0x4B5C + group, n).view(np.int64)).to("cuda")
            pts = torch.empty((n, aw), dtype=torch.int64, device="cuda")
            out = torch.empty((n, aw), dtype=torch.int64, device="cuda")
            inf = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.fixed_base_points(group, k.data_ptr(), out=pts.data_ptr(), n=n, mem=dev)
        ctx.sync()
        for stride in (1, 0):
            t = timed(lambda: ctx.points_mul(group, pts.data_ptr(), s.data_ptr(), stride=stride, n=n, out=out.data_ptr(), out_inf=inf.data_ptr(), mem=dev))
            report(op="points_mul", group=group, n=n, stride=stride, ms=round(t * 1e3, 3), per_s=round(n / t))
        # the host path on a sample, and the device result for the same rows
        m = min(args.host_sample, n)
        ctx.points_mul(group, pts.data_ptr(), s.data_ptr(), n=m, out=out.data_ptr(), out_inf=inf.data_ptr(), mem=dev)
        ctx.sync()
        hp, hs = pts[:m].cpu().numpy().view(np.uint64), s[:m].cpu().numpy().view(np.uint64)
        one = np.zeros(6 * group, dtype=np.uint64)
        one[:6] = ints_to_limbs([(1 << 384) % Q_MOD], 6)[0]                        # z = 1 in Montgomery form
        t0 = time.perf_counter()
        jac = [ctx.jac_scalar_mul(group, np.concatenate([hp[i], one]), hs[i]) for i in range(m)]
        t = time.perf_counter() - t0
        aff, _ = ctx.jac_to_affine(group, np.stack(jac))
        assert np.array_equal(aff, out[:m].cpu().numpy().view(np.uint64)), "czk_points_mul != czk_jac_scalar_mul"
        host_us[group] = t / m * 1e6
        report(op="host czk_jac_scalar_mul loop", group=group, sample=m, us_per_mul=round(host_us[group], 1), per_s=round(m / t),
               ms_at_n_extrapolated=round(t / m * n * 1e3))
        del pts, out, k, s

    # ---- KZG10 check / batch_check on honest openings from the known-beta identity
    rng = random.Random(0x4B5E)
    beta, gamma = rng.randrange(1, R_MOD), rng.randrange(1, R_MOD)
    pp = kzg.setup(ctx, 2, beta, gamma)
    vk = ctx.kzg10_vk(**kzg.trim(pp, 2)[1])
    mont = lambda vals: ints_to_limbs([v * (1 << 256) % R_MOD for v in vals], 4)

    def honest(count):
        pb = [rng.randrange(R_MOD) for _ in range(count)]
        v = [rng.randrange(R_MOD) for _ in range(count)]
        z = [rng.randrange(R_MOD) for _ in range(count)]
        wk = [(a - b) * pow(beta - c, -1, R_MOD) % R_MOD for a, b, c in zip(pb, v, z)]
        return ctx.fixed_base_points(1, ints_to_limbs(pb, 4)), mont(z), mont(v), ctx.fixed_base_points(1, ints_to_limbs(wk, 4))

    k = args.check_k
    o = honest(k)
    assert ctx.kzg10_check(vk, *o).all()
    t = timed(lambda: ctx.kzg10_check(vk, *o), reps=max(1, args.reps // 2))
    report(op="kzg10_check", k=k, ms=round(t * 1e3, 2), per_s=round(k / t),
           host_group_steps_ms_extrapolated=round(k * (2 * host_us[1] + host_us[2]) / 1e3))
    nb, bs = args.batches, args.batch_size
    o = honest(nb * bs)
    offs = [bs * j for j in range(nb + 1)]
    r = kzg.draw_randomizers(offs, rng)
    assert ctx.kzg10_batch_check(vk, *o, r, offs).all()
    t = timed(lambda: ctx.kzg10_batch_check(vk, *o, r, offs), reps=max(1, args.reps // 2))
    report(op="kzg10_batch_check", batches=nb, batch_size=bs, ms=round(t * 1e3, 2), openings_per_s=round(nb * bs / t), batches_per_s=round(nb / t),
           host_group_steps_ms_extrapolated=round(nb * bs * 3 * host_us[1] / 1e3))
    vk.release()
    ctx.close()

    if args.write:
        path = os.path.join(ROOT, "EXPERIMENTS.md")
        txt = open(path).read()
        if BEGIN not in txt or END not in txt:
            raise SystemExit("EXPERIMENTS.md has no kzg_bench markers")
        table = ["| measurement | result |", "|---|---|"]
        for row in rows:
            head = ", ".join(f"{key} {row[key]}" for key in ("op", "group", "n", "stride", "k", "batches", "batch_size", "sample") if key in row)
            rest = ", ".join(f"{key} = {val}" for key, val in row.items()
                             if key not in ("op", "group", "n", "stride", "k", "batches", "batch_size", "sample"))
            table.append(f"| {head} | {rest} |")
        txt = txt[:txt.index(BEGIN) + len(BEGIN)] + "\n" + "\n".join(table) + "\n" + txt[txt.index(END):]
        open(path, "w").write(txt)


if __name__ == "__main__":
    main()
