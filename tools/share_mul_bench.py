#!/usr/bin/env python3
"""Times of the shared-value protocols (include/czk.h czk_share_*, csrc/share_mul.hip) and of a Plonk proof on real shares.

  calls   czk_share_batch_mul / batch_inv / partial_products alone, lanes form, on n elements per lane (default 3 * 2^18), `parties` SPDZ parties:
          wall time of the blocking call (it ends with the read-back of its counts), median and minimum of --reps after one warm-up.  The lanes hold
          random field elements, not valid MACs: the kernels do the same work whatever the values, the counts are just not zero.
  plonk   polyvm.plonk_prove at 2^--log-gates gates, SPDZ, with sharing=Sharing(2, parties, source) against sharing=None on the same build and the
          same random share lanes of p, alternated.  The source replays material that SeededDealer dealt during the warm-up proof, so that dealing
          (it draws on the host) is not in the figure and every lane still holds random elements.  (With DummySource the other parties' lanes stay
          zero, and an MSM over zero scalars is cheaper: --dummy shows that figure, which is NOT the protocol's cost.)

One JSON line.

    python tools/share_mul_bench.py [--n 786432] [--parties 2] [--reps 5] [--log-gates 18] [--skip-plonk] [--out PATH]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3 << 18)
    ap.add_argument("--parties", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log-gates", type=int, default=18)
    ap.add_argument("--skip-plonk", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--dummy", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import czk_amd
    from czk_amd import polyvm
    from czk_amd.provers import rand_fr_canonical
    res = {"n": a.n, "parties": a.parties, "lpp": 2, "device": torch.cuda.get_device_name(0)}
    ctx = czk_amd.Context(0)
    L, n = 2 * a.parties, a.n
    raw = torch.from_numpy(rand_fr_canonical(1, L * n).view(np.int64)).cuda()
    blk = torch.empty((L, n, 4), dtype=torch.int64, device="cuda")
    ctx.fr_from_repr(raw.data_ptr(), out=blk.data_ptr(), n=L * n, mem=czk_amd.CZK_MEM_DEVICE)
    ctx.sync()

    def lanes(k, roll):
        """(L, k-ish, 4): the random block repeated along the element axis and rotated, so that no two vectors are the same memory"""
        reps = -(-k // n)
        return torch.cat([torch.roll(blk, roll + r, 1) for r in range(reps)], dim=1)[:, :k].contiguous()
    mac = np.stack([polyvm.mont(3 + p) for p in range(a.parties)])
    x, y, out = lanes(n, 1), lanes(n, 2), torch.empty((L, n, 4), dtype=torch.int64, device="cuda")
    calls = {}
    for name, op in (() if a.skip_calls else (("batch_mul", 0), ("batch_inv", 1), ("partial_products", 2))):
        T, P = ctx.share_material_counts(op, n)
        tx, ty, tz = lanes(T, 3), lanes(T, 4), lanes(T, 5)
        pb, pc = (lanes(P, 6), lanes(P, 7)) if P else (None, None)
        torch.cuda.synchronize()
        times = []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            if op == 0:
                ctx.share_batch_mul(2, a.parties, mac, x.data_ptr(), y.data_ptr(), tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), out.data_ptr(), n)
            else:
                fn = ctx.share_batch_inv if op == 1 else ctx.share_partial_products
                fn(2, a.parties, mac, x.data_ptr(), pb.data_ptr(), pc.data_ptr(), tx.data_ptr(), ty.data_ptr(), tz.data_ptr(), out.data_ptr(), n)
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
        calls[name] = {"ms_median": round(statistics.median(times), 3), "ms_min": round(min(times), 3), "triples": T, "pairs": P}
        del tx, ty, tz, pb, pc
    res["calls"] = calls
    ctx.close()
    del x, y, out, blk, raw
    torch.cuda.empty_cache()
    if not a.skip_plonk:
        G = 1 << a.log_gates
        pctx = polyvm.shared_stream_context(czk_amd)
        lanes_n = 2 * a.parties
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

            def triples(self, B, k):
                return self._next(lambda: self.inner.triples(B, k))

            def inv_pairs(self, B, k, inverses=0):
                return self._next(lambda: self.inner.inv_pairs(B, k, inverses))
        src = polyvm.DummySource() if a.dummy else Replay(polyvm.SeededDealer(5))
        Bs = polyvm.GpuBackend(czk_amd, pctx, lanes_n, md, sharing=polyvm.Sharing(2, a.parties, src))
        B0 = polyvm.GpuBackend(czk_amd, pctx, lanes_n, md, lift=Bs.lift, share_srs=Bs)
        for B in (Bs, B0):
            B.prepare(polyvm.plonk_commit_sizes(G))
        # a valid SPDZ sharing of a random p under the 0 / 1 key with random elements on every lane: the last party's mac lane makes the mac lanes
        # sum to what the sh lanes sum to
        W = 3 * G
        rnd = [Bs.random(100 + i, W) for i in range(lanes_n - 1)]
        sh_sum, mac_sum = None, None
        for i, r in enumerate(rnd):
            if i % 2 == 0:
                sh_sum = r if sh_sum is None else Bs.add(sh_sum, r)
            else:
                mac_sum = r if mac_sum is None else Bs.add(mac_sum, r)
        p_lanes = Bs.lane_stack(rnd + [Bs.sub(sh_sum, mac_sum)])
        t = {"sharing": [], "none": []}
        for rep in range(a.reps + 1):
            for key, B in (("sharing", Bs), ("none", B0)):
                inp = dict(polyvm.plonk_inputs(B, G), p=p_lanes)
                if key == "sharing" and not a.dummy:
                    src.at, src.replay = 0, rep > 0
                pctx.sync()
                t0 = time.perf_counter()
                polyvm.plonk_prove(B, inp)
                pctx.sync()
                if rep:
                    t[key].append((time.perf_counter() - t0) * 1e3)
        res["plonk"] = {"log_gates": a.log_gates, "source": "DummySource" if a.dummy else "SeededDealer, replayed",
                        **{k: {"ms_median": round(statistics.median(v), 2), "ms_min": round(min(v), 2)} for k, v in t.items()}}
        pctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
