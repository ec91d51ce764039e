#!/usr/bin/env python3
"""Times of the GSZ shared-value protocols (include/czk.h czk_gsz_*, csrc/gsz_mul.hip) and of a Plonk proof on real Shamir shares.

  calls   czk_gsz_share_batch_mul / _batch_inv / _partial_products and czk_gsz_product_check alone, lanes form, on n elements per lane (default
          3 * 2^18) for 3 and 4 parties: wall time of the blocking call (it ends with the read-back of its counts), median and minimum of --reps
          after one warm-up.  Beside each, THE SAME PROTOCOL composed from calls that existed before these (czk_fr_vec_op, czk_fr_vec_scale,
          czk_fr_powers, czk_fr_lanes_sum, czk_fr_gsz_open, czk_fr_batch_inverse, czk_fr_prefix_product), with the number of library calls it makes
          ("calls": each is at least one launch) and of host synchronisations it cannot avoid ("syncs": every czk_fr_gsz_open ends with one, and
          a coin has to reach the host before it can scale anything).  torch copies that only gather material or make halves contiguous are not
          counted against the composition.  The lanes hold random field elements, not sharings: the kernels do the same work whatever the
          values, the counts are just not zero.
  plonk   polyvm.plonk_prove at 2^--log-gates gates on 3 lanes: sharing=None (today's GSZ-3 benchmark workload: lane-wise products), the GSZ sharing
          with DummySource, and with material that SeededDealer dealt during the warm-up proof, replayed (dealing is not the protocol's cost).
          Reported with each: the product checks per proof, the most triples one check covered (the queue holds 3 * parties * 32 bytes of device
          memory per triple until then) and, from one more instrumented proof, the time inside the checks.

  --net WORLD   instead of the above: czk_net_gsz_share_batch_mul / _batch_inv / _partial_products and czk_net_gsz_product_check with WORLD processes,
          one party each, sharing GPU 0 over CZK_NET_IPC (device mailboxes), on n elements per party: per call the wall time on every rank between
          two barriers (median and minimum of --reps after one warm-up; the slowest rank is the call's time), the exchanges and the bytes sent and
          received per rank as czk_net_stats counts them.  With it, from the same run: the lanes form at WORLD parties in one process (measured
          first, alone on the GPU), and the latency of one king round trip and of one broadcast of a single element on that transport (--lat-reps
          of each, back to back), bare and as czk_gsz_batch_king_compute / czk_gsz_batch_open (with the open's kernel and a read-back), so that a
          call's time can be set against its exchanges.

One JSON line.

    python tools/gsz_mul_bench.py [--n 786432] [--reps 5] [--log-gates 18] [--skip-plonk] [--skip-calls] [--skip-composed] [--out PATH]
    python tools/gsz_mul_bench.py --net 3 [--n 786432] [--reps 5] [--lat-reps 200] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041


class Composed:
    """gsz20's protocols from the calls of before, on (parties, k, 4) device tensors"""

    def __init__(self, czk, ctx, torch, parties, degree):
        from czk_amd import polyvm
        self.czk, self.ctx, self.torch, self.P, self.t, self.pv = czk, ctx, torch, parties, degree, polyvm
        self.calls = self.syncs = 0
        self.M = czk.CZK_MEM_DEVICE

    def new(self, *shape):
        return self.torch.empty(shape + (4,), dtype=self.torch.int64, device="cuda")

    def op(self, code, a, b):
        """0 add, 1 sub, 2 mul over whole contiguous tensors of one shape"""
        a, b = a.contiguous(), b.contiguous()
        out = self.torch.empty_like(a)
        self.ctx.fr_vec_op(code, a.data_ptr(), b.data_ptr(), out=out.data_ptr(), n=a.numel() // 4, mem=self.M)
        self.calls += 1
        return out

    def scale(self, a, k: int):
        out = self.torch.empty_like(a)
        self.ctx.fr_vec_scale(a.data_ptr(), self.pv.mont(k), out=out.data_ptr(), n=a.numel() // 4, mem=self.M | self.czk.binding.CZK_MEM_SCALAR_HOST)
        self.calls += 1
        return out

    def open(self, lanes, bound):
        k = lanes.shape[1]
        out = self.new(k)
        self.ctx.fr_gsz_open(lanes.contiguous().data_ptr(), self.P, k, out.data_ptr(), degree=bound)
        self.calls, self.syncs = self.calls + 1, self.syncs + 1
        return out

    def king(self, masked, r):
        v = self.open(masked, 2 * self.t)
        return self.op(1, v.unsqueeze(0).expand(self.P, -1, -1), r)

    def mul(self, x, y, r, r2):
        return self.king(self.op(0, self.op(2, x, y), r2), r)

    def inv(self, x, rs, r, r2):
        opened = self.open(self.mul(x, rs, r, r2), self.t)
        inv = self.torch.empty_like(opened)
        self.ctx.fr_batch_inverse(opened.data_ptr(), n=opened.shape[0], out=inv.data_ptr(), mem=self.M)
        self.calls += 1
        return self.op(2, rs, inv.unsqueeze(0).expand(self.P, -1, -1))

    def partial_products(self, x, dr, dr2, rands):
        n = x.shape[1]
        m = rands[:, :n + 1]
        m_inv = self.inv(m, rands[:, n + 1:2 * n + 2], dr[:, :n + 1], dr2[:, :n + 1])
        mx = self.mul(m[:, :n], x, dr[:, n + 1:2 * n + 1], dr2[:, n + 1:2 * n + 1])
        mxm = self.open(self.mul(mx, m_inv[:, 1:], dr[:, 2 * n + 1:3 * n + 1], dr2[:, 2 * n + 1:3 * n + 1]), self.t)
        run = self.torch.empty_like(mxm)
        self.ctx.fr_prefix_product(mxm.data_ptr(), n=n, out=run.data_ptr(), mem=self.M)
        self.calls += 1
        mms = self.mul(m[:, :1].expand(-1, n, -1), m_inv[:, 1:], dr[:, 3 * n + 1:4 * n + 1], dr2[:, 3 * n + 1:4 * n + 1])
        out = self.inv(mms, rands[:, 2 * n + 2:], dr[:, 4 * n + 1:], dr2[:, 4 * n + 1:])
        return self.op(2, out, run.unsqueeze(0).expand(self.P, -1, -1))

    def host(self, one):
        """a single opened element to the host"""
        self.syncs += 1
        return self.pv.unmont(one.reshape(-1, 4)[0].cpu().numpy().view(np.uint64))

    def lane_totals(self, v):
        """(P, k, 4) -> (P, 1, 4): the sum over every lane's elements with czk_fr_lanes_sum, which adds k vectors of n elements with one thread per
        element: a long lane goes as rows of 1024 (zero-padded) so that 1024 threads share the work, then the 1024 partial sums as k = 1024, n = 1"""
        P, k = v.shape[0], v.shape[1]
        acc = self.new(P, 1)
        if k > 2048:
            rows = -(-k // 1024)
            v = self.torch.cat([v, self.torch.zeros((P, rows * 1024 - k, 4), dtype=v.dtype, device=v.device)], 1).contiguous()
            part = self.new(P, 1024)
            for j in range(P):
                self.ctx.fr_lanes_sum(v[j].data_ptr(), rows, 1024, part[j].data_ptr())
            self.calls += P
            v, k = part, 1024
        for j in range(P):
            self.ctx.fr_lanes_sum(v[j].data_ptr(), k, 1, acc[j].data_ptr())
        self.calls += P
        return acc

    def ip(self, xs, ys, r, r2):
        return self.king(self.op(0, self.lane_totals(self.op(2, xs, ys)), r2), r)

    def check(self, xs, ys, zs, dr, dr2, rands):
        P, n, torch = self.P, xs.shape[1], self.torch
        d, r = 0, 0
        c = self.host(self.open(rands[:, r:r + 1], self.t))
        r += 1
        pw = self.new(1, n)
        self.ctx.fr_powers(self.pv.mont(c), n, out=pw.data_ptr(), mem=self.M)
        self.calls += 1
        pw = pw.expand(P, -1, -1)
        xs = self.op(2, xs, pw)
        rz = self.op(2, zs, pw)
        ip = self.lane_totals(rz)
        while xs.shape[1] > 1:
            if xs.shape[1] % 2:
                z = torch.zeros((P, 1, 4), dtype=torch.int64, device="cuda")
                xs, ys = torch.cat([xs, z], 1), torch.cat([ys, z], 1)
            h = xs.shape[1] // 2
            xl, xr, yl, yr = (t.contiguous() for t in (xs[:, :h], xs[:, h:], ys[:, :h], ys[:, h:]))
            ip_l = self.ip(xl, yl, dr[:, d:d + 1], dr2[:, d:d + 1])
            ip3 = self.ip(self.op(1, self.op(0, xr, xr), xl), self.op(1, self.op(0, yr, yr), yl), dr[:, d + 1:d + 2], dr2[:, d + 1:d + 2])
            d += 2
            c = self.host(self.open(rands[:, r:r + 1], self.t))
            r += 1
            xs = self.op(0, self.scale(self.op(1, xr, xl), c), self.op(1, self.op(0, xl, xl), xr))
            ys = self.op(0, self.scale(self.op(1, yr, yl), c), self.op(1, self.op(0, yl, yl), yr))
            i2 = pow(2, -1, R_MOD)
            f1, f2, f3 = (c - 2) * (c - 3) * i2 % R_MOD, -(c - 1) * (c - 3) % R_MOD, (c - 1) * (c - 2) * i2 % R_MOD
            ip = self.op(0, self.op(0, self.scale(ip_l, f1), self.scale(self.op(1, ip, ip_l), f2)), self.scale(ip3, f3))
        xr_, yr_ = rands[:, r:r + 1], rands[:, r + 1:r + 2]
        dd = lambda k: (dr[:, d + k:d + k + 1], dr2[:, d + k:d + k + 1])    # noqa: E731
        ipr = self.mul(xr_, yr_, *dd(0))
        xb, yb, zb = self.mul(xs, xr_, *dd(1)), self.mul(ys, yr_, *dd(2)), self.mul(ip, ipr, *dd(3))
        x, y, z = (self.host(self.open(b, self.t)) for b in (xb, yb, zb))
        return x * y % R_MOD == z


def timed(fn, reps):
    times = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3)}


NET_CALLS = ("batch_mul", "batch_inv", "partial_products", "product_check")


def random_lanes(czk_amd, torch, ctx, parties, n, seed):
    """-> lanes(k, roll): (parties, k, 4) device tensors of random field elements, no two of them the same memory"""
    from czk_amd.provers import rand_fr_canonical
    raw = torch.from_numpy(rand_fr_canonical(seed, parties * n).view(np.int64)).cuda()
    blk = torch.empty((parties, n, 4), dtype=torch.int64, device="cuda")
    ctx.fr_from_repr(raw.data_ptr(), out=blk.data_ptr(), n=parties * n, mem=czk_amd.CZK_MEM_DEVICE)
    ctx.sync()
    return lambda k, roll: torch.cat([torch.roll(blk, roll + r, 1) for r in range(-(-k // n))], dim=1)[:, :k].contiguous()


def lanes_form(czk_amd, torch, parties, n, reps):
    """the four lanes-form calls at `parties` parties in this process -> {call: {ms_median, ms_min}}"""
    bd, t = czk_amd.binding, (parties - 1) // 2
    ctx = czk_amd.Context(0)
    lanes = random_lanes(czk_amd, torch, ctx, parties, n, 1)
    x, y, z, out = lanes(n, 1), lanes(n, 2), lanes(n, 3), torch.empty((parties, n, 4), dtype=torch.int64, device="cuda")
    per = {}
    for name, op in zip(NET_CALLS, (bd.CZK_GSZ_OP_MUL, bd.CZK_GSZ_OP_INV, bd.CZK_GSZ_OP_PARTIAL_PRODUCTS, bd.CZK_GSZ_OP_PRODUCT_CHECK)):
        nd, nr = ctx.gsz_material_counts(op, n)
        dr, dr2, rands = lanes(nd, 4), lanes(nd, 5), lanes(max(nr, 1), 6)
        p = [v.data_ptr() for v in (x, y, z, dr, dr2, rands, out)]
        call = {"batch_mul": lambda: ctx.gsz_share_batch_mul(parties, t, p[0], p[1], p[3], p[4], p[6], n),
                "batch_inv": lambda: ctx.gsz_share_batch_inv(parties, t, p[0], p[3], p[4], p[5], p[6], n),
                "partial_products": lambda: ctx.gsz_share_partial_products(parties, t, p[0], p[3], p[4], p[5], p[6], n),
                "product_check": lambda: ctx.gsz_product_check(parties, t, p[0], p[1], p[2], n, p[3], p[4], p[5])}[name]
        torch.cuda.synchronize()
        per[name] = timed(call, reps)
        del dr, dr2, rands
    ctx.close()
    return per


def net_party(rank, world, q, idb, n, reps, lat_reps):
    """one party of --net: times the four calls on its own lane and the two single-element exchanges"""
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    import torch
    import czk_amd
    bd, t = czk_amd.binding, (world - 1) // 2
    torch.cuda.set_device(0)
    ctx = czk_amd.Context(0)
    slot = max(16 << 20, ((n + 1) * 32 + (1 << 20)) & ~((1 << 20) - 1))       # a whole lane per chunk step
    net = czk_amd.Net(ctx, czk_amd.CZK_NET_IPC, rank, world, idb, options={"slot_bytes": slot, "timeout_ms": 120000})
    lanes = random_lanes(czk_amd, torch, ctx, 1, n, 11 + rank)
    x, y, z, out = lanes(n, 1)[0], lanes(n, 2)[0], lanes(n, 3)[0], torch.empty((n, 4), dtype=torch.int64, device="cuda")
    per = {}
    for name, op in zip(NET_CALLS, (bd.CZK_GSZ_OP_MUL, bd.CZK_GSZ_OP_INV, bd.CZK_GSZ_OP_PARTIAL_PRODUCTS, bd.CZK_GSZ_OP_PRODUCT_CHECK)):
        nd, nr = ctx.gsz_material_counts(op, n)
        dr, dr2, rands = lanes(nd, 4)[0], lanes(nd, 5)[0], lanes(max(nr, 1), 6)[0]
        p = [v.data_ptr() for v in (x, y, z, dr, dr2, rands, out)]
        call = {"batch_mul": lambda: net.gsz_share_batch_mul(t, p[0], p[1], p[3], p[4], p[6], n),
                "batch_inv": lambda: net.gsz_share_batch_inv(t, p[0], p[3], p[4], p[5], p[6], n),
                "partial_products": lambda: net.gsz_share_partial_products(t, p[0], p[3], p[4], p[5], p[6], n),
                "product_check": lambda: net.gsz_product_check(t, p[0], p[1], p[2], n, p[3], p[4], p[5])}[name]
        times = []
        for rep in range(reps + 1):
            torch.cuda.synchronize()
            net.barrier()
            net.stats_reset()
            t0 = time.perf_counter()
            call()
            net.barrier()                                                      # the call is over when every party has its answer
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        per[name] = dict(net.stats(), ms_median=round(statistics.median(times), 3), ms_min=round(min(times), 3))
        del dr, dr2, rands
    one, king = out[:1], torch.empty((2 * world, 4), dtype=torch.int64, device="cuda")
    lat = {}
    for name, step in (("king_round_trip", lambda: (net.fr_send_to_king(one.data_ptr(), 1, king.data_ptr()), net.fr_recv_from_king(king.data_ptr(), 1, one.data_ptr()))),
                       ("broadcast", lambda: net.broadcast(one.data_ptr(), 32, king.data_ptr(), mem=czk_amd.CZK_MEM_DEVICE)),
                       # the same two with the open's kernel and a read-back of its count: the blocking calls a party had to compose before
                       ("king_compute", lambda: net.gsz_batch_king_compute(one.data_ptr(), 1, one.data_ptr(), degree=2 * t)),
                       ("batch_open", lambda: net.gsz_batch_open(one.data_ptr(), 1, king.data_ptr(), degree=t))):
        step()
        ctx.sync()
        net.barrier()
        t0 = time.perf_counter()
        for _ in range(lat_reps):
            step()
        ctx.sync()
        lat[name + "_us"] = round((time.perf_counter() - t0) * 1e6 / lat_reps, 2)
    net.barrier()
    net.close()
    ctx.close()
    q.put((rank, per, lat))


def net_mode(a):
    import multiprocessing as mp
    import torch
    import czk_amd
    res = {"n": a.n, "world": a.net, "transport": "ipc", "device": torch.cuda.get_device_name(0)}
    res["lanes_form"] = lanes_form(czk_amd, torch, a.net, a.n, a.reps)
    torch.cuda.empty_cache()
    c = mp.get_context("spawn")
    q = c.Queue()
    idb = czk_amd.Net.unique_id(czk_amd.CZK_NET_IPC)
    procs = [c.Process(target=net_party, args=(r, a.net, q, idb, a.n, a.reps, a.lat_reps)) for r in range(a.net)]
    for p in procs:
        p.start()
    got = []
    while len(got) < a.net:
        try:
            got.append(q.get(timeout=1.0))
        except Exception:
            if any(p.exitcode not in (None, 0) for p in procs):
                for p in procs:
                    if p.is_alive():
                        p.kill()
                raise SystemExit("a party died: " + str([p.exitcode for p in procs]))
    for p in procs:
        p.join()
    got.sort()
    res["net"] = {name: {"ms_median": max(per[name]["ms_median"] for _, per, _ in got), "ms_min": max(per[name]["ms_min"] for _, per, _ in got),
                         "ranks": [per[name] for _, per, _ in got]} for name in NET_CALLS}
    res["latency"] = {k: [lat[k] for _, _, lat in got] for k in got[0][2]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", type=int, default=0, metavar="WORLD")
    ap.add_argument("--lat-reps", type=int, default=200)
    ap.add_argument("--n", type=int, default=3 << 18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-gates", type=int, default=18)
    ap.add_argument("--skip-plonk", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--skip-composed", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.net:
        line = json.dumps(net_mode(a))
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    import torch
    import czk_amd
    from czk_amd import polyvm
    from czk_amd.provers import rand_fr_canonical
    bd = czk_amd.binding
    res = {"n": a.n, "device": torch.cuda.get_device_name(0), "calls": {}}
    n = a.n
    for parties in (() if a.skip_calls else (3, 4)):
        t = (parties - 1) // 2
        ctx = czk_amd.Context(0)
        raw = torch.from_numpy(rand_fr_canonical(1, parties * n).view(np.int64)).cuda()
        blk = torch.empty((parties, n, 4), dtype=torch.int64, device="cuda")
        ctx.fr_from_repr(raw.data_ptr(), out=blk.data_ptr(), n=parties * n, mem=czk_amd.CZK_MEM_DEVICE)
        ctx.sync()

        def lanes(k, roll):
            """(parties, k, 4): the random block repeated along the element axis and rotated, so that no two vectors are the same memory"""
            return torch.cat([torch.roll(blk, roll + r, 1) for r in range(-(-k // n))], dim=1)[:, :k].contiguous()
        x, y, z, out = lanes(n, 1), lanes(n, 2), lanes(n, 3), torch.empty((parties, n, 4), dtype=torch.int64, device="cuda")
        per = {}
        for name, op in (("batch_mul", bd.CZK_GSZ_OP_MUL), ("batch_inv", bd.CZK_GSZ_OP_INV), ("partial_products", bd.CZK_GSZ_OP_PARTIAL_PRODUCTS),
                         ("product_check", bd.CZK_GSZ_OP_PRODUCT_CHECK)):
            nd, nr = ctx.gsz_material_counts(op, n)
            dr, dr2, rands = lanes(nd, 4), lanes(nd, 5), lanes(max(nr, 1), 6)
            p = [v.data_ptr() for v in (x, y, z, dr, dr2, rands, out)]
            fused = {"batch_mul": lambda: ctx.gsz_share_batch_mul(parties, t, p[0], p[1], p[3], p[4], p[6], n),
                     "batch_inv": lambda: ctx.gsz_share_batch_inv(parties, t, p[0], p[3], p[4], p[5], p[6], n),
                     "partial_products": lambda: ctx.gsz_share_partial_products(parties, t, p[0], p[3], p[4], p[5], p[6], n),
                     "product_check": lambda: ctx.gsz_product_check(parties, t, p[0], p[1], p[2], n, p[3], p[4], p[5])}[name]
            torch.cuda.synchronize()
            per[name] = {"doubles": nd, "rands": nr, "fused": timed(fused, a.reps)}
            if not a.skip_composed:
                C = Composed(czk_amd, ctx, torch, parties, t)
                comp = {"batch_mul": lambda: C.mul(x, y, dr, dr2), "batch_inv": lambda: C.inv(x, rands, dr, dr2),
                        "partial_products": lambda: C.partial_products(x, dr, dr2, rands), "product_check": lambda: C.check(x, y, z, dr, dr2, rands)}[name]
                tm = timed(comp, a.reps)
                per[name]["composed"] = dict(tm, calls=C.calls // (a.reps + 1), syncs=C.syncs // (a.reps + 1))
            del dr, dr2, rands
        res["calls"][str(parties)] = per
        ctx.close()
        del x, y, z, out, blk, raw
        torch.cuda.empty_cache()
    if not a.skip_plonk:
        G, parties = 1 << a.log_gates, 3
        pctx = polyvm.shared_stream_context(czk_amd)
        md = polyvm.plonk_max_degree(G)

        class Replay:
            """deals through `inner` until told to replay; then hands out the same arrays in the same order, proof after proof"""

            def __init__(self, inner):
                self.inner, self.rec, self.at, self.replay = inner, [], 0, False

            def _next(self, make):
                if not self.replay:
                    self.rec.append(make())
                    return self.rec[-1]
                self.at += 1
                return self.rec[self.at - 1]

            def doubles(self, B, k):
                return self._next(lambda: self.inner.doubles(B, k))

            def rands(self, B, k):
                return self._next(lambda: self.inner.rands(B, k))
        dealer = polyvm.SeededDealer(5)
        src = Replay(dealer)
        Bd = polyvm.GpuBackend(czk_amd, pctx, parties, md, sharing=polyvm.Sharing(1, parties, src, scheme="gsz"))
        Bu = polyvm.GpuBackend(czk_amd, pctx, parties, md, sharing=polyvm.Sharing(1, parties, polyvm.DummySource(), scheme="gsz"), share_srs=Bd)
        B0 = polyvm.GpuBackend(czk_amd, pctx, parties, md, share_srs=Bd)
        for B in (Bd, Bu, B0):
            B.prepare(polyvm.plonk_commit_sizes(G))
        p_lanes = dealer._shamir(Bd, Bd.random(100, 3 * G), Bd.sharing.degree)      # a real degree-t sharing of a random p
        runs = (("none", B0), ("gsz_dummy", Bu), ("gsz_dealer", Bd))
        t = {k: [] for k, _ in runs}
        for rep in range(a.reps + 1):
            for key, B in runs:
                inp = dict(polyvm.plonk_inputs(B, G), p=p_lanes)
                if B is Bd:
                    src.at, src.replay = 0, rep > 0
                pctx.sync()
                t0 = time.perf_counter()
                polyvm.plonk_prove(B, inp)
                pctx.sync()
                if rep:
                    t[key].append((time.perf_counter() - t0) * 1e3)
        res["plonk"] = {"log_gates": a.log_gates, "parties": parties}
        for key, B in runs:
            res["plonk"][key] = {"ms_median": round(statistics.median(t[key]), 2), "ms_min": round(min(t[key]), 2)}
        for key, B in runs[1:]:                                     # one more proof with the checks bracketed by synchronisations
            spent, inner, checks0 = [0.0], B.gsz_check, B.gsz_checks

            def bracketed():
                if B._gsz_queue:
                    pctx.sync()
                    t0 = time.perf_counter()
                    inner()
                    spent[0] += (time.perf_counter() - t0) * 1e3
            B.gsz_check = bracketed
            if B is Bd:
                src.at, src.replay = 0, True
            polyvm.plonk_prove(B, dict(polyvm.plonk_inputs(B, G), p=p_lanes))
            pctx.sync()
            B.gsz_check = inner
            res["plonk"][key].update(checks_per_proof=B.gsz_checks - checks0, queue_peak_triples=B.gsz_queue_peak,
                                     queue_peak_mib=round(B.gsz_queue_peak * 3 * parties * 32 / 2**20, 1), ms_in_checks=round(spent[0], 2))
        pctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
