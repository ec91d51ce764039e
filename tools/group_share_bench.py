#!/usr/bin/env python3
"""Latency of the group-share calls (include/czk.h czk_share_group_batch_scale, czk_gsz_group_batch_mul, czk_gsz_group_product_check;
csrc/group_share.hip) for G1 and G2 at n = 3, 48, 2^10, 2^16 -- beside the same protocol COMPOSED from the calls that existed before
(czk_points_mul / _add / _sum on device arrays), and for n = 3 beside the host's one-point-at-a-time czk_jac_* arithmetic.

  scale   SPDZ, 2 parties (4 lanes): one call | composed: mask (add), open (adds), MAC check (mul, add, flags read back), two multiplications and two
          additions per lane
  mul     GSZ, 3 parties: one call | composed: [x_j] Y_j (mul), + r2 (add), the king's sum (adds) and 1 / P (mul), - r_j (adds)
  check   GSZ, 3 parties: one call | composed: per round the two inner products (mul + segmented sum each, after 2 Yr - Yl by adds), the king's sums
          and 1 / P, the parabola (three muls, adds per lane), the fold (adds, one mul); then the final two group mults and opens
The compositions do the POINT work only: the scalars they multiply by (the opened oy, the coins, k_l oy - y_l, ...) are taken as given, no field kernel is
launched and nothing but the MAC / degree flags is read back -- every simplification favours the composition.  The inputs are random subgroup points
and scalars, not consistent sharings: neither side's time depends on the values.  Each measurement: one warm-up, then --reps repetitions between
stream synchronisations; the median in ms.

  --proof LOG   also create_proof_shared beside create_proof at 2^LOG constraints (SPDZ, 2 parties), host wall time after step()

One JSON line.

    python tools/group_share_bench.py [--reps 5] [--sizes 3,48,1024,65536] [--proof 20] [--out PATH]"""
import argparse
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


class Dev:
    """device arrays of random subgroup points / scalars, and the existing point calls on them"""

    def __init__(self, czk, ctx, group):
        import torch
        from czk_amd.provers import rand_fr_canonical
        self.czk, self.ctx, self.g, self.torch, self.rand = czk, ctx, group, torch, rand_fr_canonical
        self.aw = 12 if group == czk.CZK_G1 else 24
        self.gen = torch.from_numpy(ctx.fixed_base_points(group, np.array([[1, 0, 0, 0]], np.uint64))[0].view(np.int64).copy()).cuda()
        self.seed = 1

    def scalars(self, n):
        self.seed += 1
        return self.torch.from_numpy(self.rand(0x5EED + self.seed, n).view(np.int64)).cuda()     # (canonical limbs read as Montgomery: still random elements)

    def new(self, n):
        return self.torch.empty((n, self.aw), dtype=self.torch.int64, device="cuda"), self.torch.zeros(n, dtype=self.torch.uint8, device="cuda")

    def points(self, n):
        out = self.new(n)
        k = self.scalars(n)
        self.ctx.points_mul(self.g, self.gen.data_ptr(), k.data_ptr(), stride=0, scalar_form=self.czk.CZK_SCALAR_MONTGOMERY, n=n, out=out[0].data_ptr(),
                            out_inf=out[1].data_ptr(), mem=self.czk.CZK_MEM_DEVICE)
        self.ctx.sync()
        return out

    def mul(self, p, k, out, n):
        self.ctx.points_mul(self.g, p[0].data_ptr(), k.data_ptr(), inf=p[1].data_ptr(), scalar_form=self.czk.CZK_SCALAR_MONTGOMERY, n=n, out=out[0].data_ptr(),
                            out_inf=out[1].data_ptr(), mem=self.czk.CZK_MEM_DEVICE)

    def add(self, a, b, out, n, neg=False, ao=0, bo=0, oo=0):
        """out[oo:oo+n] = a[ao:ao+n] +- b[bo:bo+n]"""
        w = self.aw * 8
        self.ctx.points_add(self.g, a[0].data_ptr() + ao * w, b[0].data_ptr() + bo * w, a_inf=a[1].data_ptr() + ao, b_inf=b[1].data_ptr() + bo, negate_b=neg, n=n,
                            out=out[0].data_ptr() + oo * w, out_inf=out[1].data_ptr() + oo, mem=self.czk.CZK_MEM_DEVICE)

    def sums(self, p, offsets, out):
        self.ctx.points_sum(self.g, p[0].data_ptr(), offsets, inf=p[1].data_ptr(), out=out[0].data_ptr(), out_inf=out[1].data_ptr(), mem=self.czk.CZK_MEM_DEVICE)


def bench_scale(czk, ctx, d, n, reps, host):
    L, P = 4, 2
    s, tx, tz, out, a, t1, t2 = (d.points(L * n) if i < 3 else d.new(L * n) for i in range(7))
    o, ty, k1, k2 = (d.scalars(L * n) for _ in range(4))
    sx, ms, chk, alpha = d.new(n), d.new(n), d.new(n), d.scalars(n)
    mac = np.ascontiguousarray(d.rand(3, P))
    call = lambda: ctx.share_group_batch_scale(d.g, 2, P, mac, s[0].data_ptr(), s[1].data_ptr(), o.data_ptr(), tx[0].data_ptr(), tx[1].data_ptr(), ty.data_ptr(),  # noqa: E731
                                               tz[0].data_ptr(), tz[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), n)

    def composed():
        d.add(s, tx, a, L * n)                                       # mask
        d.add(a, a, sx, n, ao=0, bo=2 * n)                           # open: the sh lanes
        d.add(a, a, ms, n, ao=n, bo=3 * n)                           # ... and the mac lanes
        d.mul(sx, alpha, chk, n)                                     # [alpha] sx - macs: the check
        d.add(chk, ms, chk, n, neg=True)
        d.mul(tx, k1, t1, L * n)                                     # [-oy] x_l
        for ln in range(L):                                          # [k_l oy - y_l] sx: sx per lane
            ctx.points_mul(d.g, sx[0].data_ptr(), k2.data_ptr() + 32 * ln * n, inf=sx[1].data_ptr(), scalar_form=czk.CZK_SCALAR_MONTGOMERY, n=n,
                           out=t2[0].data_ptr() + d.aw * 8 * ln * n, out_inf=t2[1].data_ptr() + ln * n, mem=czk.CZK_MEM_DEVICE)
        d.add(tz, t1, out, L * n)
        d.add(out, t2, out, L * n)
        return int(chk[1].sum().item())                              # the flags read back: the count
    res = {"call_ms": timed(ctx, call, reps), "composed_ms": timed(ctx, composed, reps)}
    if host:
        res["host_jac_ms"] = host_scale(czk, ctx, d, L, n, reps)
    return res


def host_scale(czk, ctx, d, L, n, reps):
    """the same arithmetic with czk_jac_* on host values, one point at a time: 3 scalar multiplications and the additions per output, plus the check"""
    g = d.g
    pts = d.points(4)[0].cpu().numpy().view(np.uint64)
    one = _jac(czk, g, pts[0])
    k = d.rand(9, 3)

    def run():
        for _ in range(n):
            sx = one
            for _ in range(L):
                sx = ctx.jac_add_mixed(g, sx, pts[1], False)
            ctx.jac_scalar_mul(g, sx, k[0])
            for _ in range(L):
                r = ctx.jac_add(g, ctx.jac_scalar_mul(g, one, k[1]), ctx.jac_scalar_mul(g, sx, k[2]))
                ctx.jac_add_mixed(g, r, pts[2], False)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 3)


def _jac(czk, g, aff):
    from czk_amd.provers import to_mont_limbs_fq
    one = to_mont_limbs_fq(1)
    return np.concatenate([aff, one if g == czk.CZK_G1 else np.concatenate([one, np.zeros(6, np.uint64)])]).astype(np.uint64)


def bench_mul(czk, ctx, d, n, reps, host):
    P = 3
    y, gr, gr2 = d.points(P * n), d.points(P * n), d.points(P * n)
    x, pinv = d.scalars(P * n), d.scalars(n)
    out, dd, v = d.new(P * n), d.new(P * n), d.new(n)
    call = lambda: ctx.gsz_group_batch_mul(d.g, P, 1, x.data_ptr(), y[0].data_ptr(), y[1].data_ptr(), gr[0].data_ptr(), gr[1].data_ptr(), gr2[0].data_ptr(),  # noqa: E731
                                           gr2[1].data_ptr(), out[0].data_ptr(), out[1].data_ptr(), n)

    def composed():
        d.mul(y, x, dd, P * n)
        d.add(dd, gr2, dd, P * n)
        d.add(dd, dd, v, n, ao=0, bo=n)
        d.add(v, dd, v, n, bo=2 * n)
        d.mul(v, pinv, v, n)
        for j in range(P):
            d.add(v, gr, out, n, neg=True, bo=j * n, oo=j * n)
    res = {"call_ms": timed(ctx, call, reps), "composed_ms": timed(ctx, composed, reps)}
    if host:
        g = d.g
        pts = d.points(2)[0].cpu().numpy().view(np.uint64)
        p0, k = _jac(czk, g, pts[0]), d.rand(9, 2)

        def run():
            for _ in range(n):
                acc = p0
                for _ in range(P):
                    acc = ctx.jac_add(g, acc, ctx.jac_add_mixed(g, ctx.jac_scalar_mul(g, p0, k[0]), pts[1], False))
                acc = ctx.jac_scalar_mul(g, acc, k[1])
                for _ in range(P):
                    ctx.jac_add_mixed(g, acc, pts[1], False)
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            t.append((time.perf_counter() - t0) * 1e3)
        res["host_jac_ms"] = round(statistics.median(t), 3)
    return res


def bench_check(czk, ctx, d, n, reps, host):
    P = 3
    R = (n - 1).bit_length() if n > 1 else 0
    gd, fd, nr = ctx.gsz_group_material_counts(czk.binding.CZK_GSZ_GROUP_OP_PRODUCT_CHECK, n)
    ys, zs, gr, gr2 = d.points(P * n), d.points(P * n), d.points(P * gd), d.points(P * gd)
    xs, fr, fr2, rands = d.scalars(P * n), d.scalars(P * fd), d.scalars(P * fd), d.scalars(P * nr)
    call = lambda: ctx.gsz_group_product_check(d.g, P, 1, xs.data_ptr(), ys[0].data_ptr(), ys[1].data_ptr(), zs[0].data_ptr(), zs[1].data_ptr(), n, gr[0].data_ptr(),  # noqa: E731
                                               gr[1].data_ptr(), gr2[0].data_ptr(), gr2[1].data_ptr(), fr.data_ptr(), fr2.data_ptr(), rands.data_ptr())
    h0 = (n + 1) // 2
    w1, w2, w3, yw = d.new(P * n), d.new(P * n), d.new(P * n), d.new(P * n)
    ipl, ip3, ip, tmp, one_pt = d.new(P), d.new(P), d.points(P), d.new(P), d.new(1)
    kp, k3 = d.scalars(P * n), d.scalars(3 * P)

    def lane_sums(src, m, out):
        d.sums(src, [j * m for j in range(P + 1)], out)

    def king(v):                                                     # + r2, the sum over parties, 1 / P, - r_j
        d.add(v, gr2, v, P)
        d.add(v, v, one_pt, 1, ao=0, bo=1)
        d.add(one_pt, v, one_pt, 1, bo=2)
        d.mul(one_pt, k3, one_pt, 1)
        for j in range(P):
            d.add(one_pt, gr, v, 1, neg=True, bo=j, oo=j)

    def composed():
        d.mul(zs, kp, w1, P * n)                                     # [rho^i] Z_i and the lanes' sums
        lane_sums(w1, n, ip)
        cur, m = ys, n
        for _ in range(R):
            h = (m + 1) // 2
            # (the lanes are treated as one array of P m points split at h: the same number of point operations as the per-lane halves)
            d.mul(cur, kp, w1, P * h)                                # [xl] Yl
            lane_sums(w1, h, ipl)
            d.add(cur, cur, w2, P * h, ao=P * (m - h), bo=P * (m - h))   # 2 Yr
            d.add(w2, cur, w2, P * h, neg=True)                      # - Yl
            d.mul(w2, kp, w3, P * h)
            lane_sums(w3, h, ip3)
            king(ipl)
            king(ip3)
            for src in (ipl, ip, ip3):                               # the parabola: three multiplications and two additions per lane
                d.mul(src, k3, tmp, P)
                d.add(ip, tmp, ip, P)
            d.add(cur, cur, w1, P * h, neg=True, ao=P * (m - h))     # Yr - Yl
            d.mul(w1, kp, w1, P * h)                                 # [c] (...)
            d.add(cur, cur, w2, P * h)                               # 2 Yl
            d.add(w2, cur, w2, P * h, neg=True, bo=P * (m - h))      # - Yr
            d.add(w1, w2, yw, P * h)
            cur, m = yw, h
        for src in (cur, ip):                                        # the two final group mults and their opens
            d.mul(src, k3, tmp, P)
            king(tmp)
            d.add(tmp, tmp, one_pt, 1, ao=0, bo=1)
            d.add(one_pt, tmp, one_pt, 1, bo=2)
            d.mul(one_pt, k3, one_pt, 1)
        return int(one_pt[1].sum().item())                           # the verdict read back
    res = {"call_ms": timed(ctx, call, reps), "composed_ms": timed(ctx, composed, reps), "rounds": R, "launches": 3 * R + 2}
    return res


def bench_proof(czk, log_n, reps):
    import random

    import torch
    from czk_amd.provers import DummyGroupSource, Groth16Local, rand_fr_canonical
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        ctx = czk.Context(0, ts.cuda_stream)
        p = Groth16Local(czk, ctx, 1 << log_n, 2, scheme="spdz")
        p.step()
        torch.cuda.synchronize()
        res = {k: v.copy() for k, v in p.results.items()}
        rs = rand_fr_canonical(77, 2)
        rng = random.Random(1)
        r_l, s_l = p.share_scalar(int(rs[0][0]), rng), p.share_scalar(int(rs[1][0]), rng)
        src = DummyGroupSource()

        def wall(fn):
            fn()
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e3)
            return round(statistics.median(t), 3)
        out = {"log_constraints": log_n, "create_proof_ms": wall(lambda: p.create_proof({k: v.copy() for k, v in res.items()}, rs[0], rs[1])),
               "create_proof_shared_ms": wall(lambda: p.create_proof_shared({k: v.copy() for k, v in res.items()}, r_l, s_l, src))}
        t0 = time.perf_counter()
        p.step()
        torch.cuda.synchronize()
        out["step_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        del p
        ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="3,48,1024,65536")
    ap.add_argument("--proof", type=int, default=0, metavar="LOG")
    ap.add_argument("--out")
    a = ap.parse_args()
    import czk_amd as czk
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk)
    res = {"tool": "group_share_bench", "reps": a.reps, "results": []}
    for gname, g in (("G1", czk.CZK_G1), ("G2", czk.CZK_G2)):
        d = Dev(czk, ctx, g)
        for n in [int(v) for v in a.sizes.split(",")]:
            row = {"group": gname, "n": n}
            for name, fn in (("scale", bench_scale), ("mul", bench_mul), ("check", bench_check)):
                row[name] = fn(czk, ctx, d, n, a.reps, host=n == 3)
            res["results"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    ctx.close()
    if a.proof:
        res["proof"] = bench_proof(czk, a.proof, max(2, a.reps // 2))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
