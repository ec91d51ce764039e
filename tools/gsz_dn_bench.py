#!/usr/bin/env python3
"""The time to MAKE the double and random shares a Plonk proof on GSZ shares consumes (include/czk.h czk_gsz_dn_*, csrc/gsz_dn.hip), beside SeededDealer.

A Plonk proof at 2^--log-gates gates on --parties lanes is run once with DummySource behind a recorder: the sequence of doubles(n) / rands(n) requests
the prover and its product checks make is the workload (D = the doubles, Rn = the random shares over the whole proof).  Then, on the same box, the same
requests are served --reps times each (after one warm-up) by
  dn        polyvm.DnSource: czk_gsz_dn_generate + czk_gsz_dn_check per request, the lanes form (one process holds every key)
  dn_nocheck  the same without the consistency check
  dealer    polyvm.SeededDealer: SplitMix64 on the host, an upload, one scale and one add per coefficient and party
every request bracketed by stream synchronisations; reported: wall time of the whole sequence, median and minimum.

  --net WORLD   the net form instead: WORLD processes, one party and one key each, sharing GPU 0 over CZK_NET_SHM, serve the same requests with
          czk_net_gsz_dn_generate + czk_net_gsz_dn_check; per rank the wall time of the sequence between two barriers (the slowest rank is the time)
          and the bytes sent per party as czk_net_stats counts them.  The lanes form at WORLD parties is measured first, alone on the GPU.

One JSON line.

    python tools/gsz_dn_bench.py [--log-gates 18] [--parties 3] [--reps 3] [--out PATH]
    python tools/gsz_dn_bench.py --net 3 [--log-gates 18] [--reps 3] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Recorder:
    """DummySource's material, and the list of what was asked for"""

    def __init__(self, inner):
        self.inner, self.requests = inner, []

    def doubles(self, B, n):
        self.requests.append(("doubles", n))
        return self.inner.doubles(B, n)

    def rands(self, B, n):
        self.requests.append(("rands", n))
        return self.inner.rands(B, n)


def record_requests(czk_amd, log_gates, parties):
    from czk_amd import polyvm
    G = 1 << log_gates
    ctx = polyvm.shared_stream_context(czk_amd)
    rec = Recorder(polyvm.DummySource())
    B = polyvm.GpuBackend(czk_amd, ctx, parties, polyvm.plonk_max_degree(G), sharing=polyvm.Sharing(1, parties, rec, scheme="gsz"))
    B.prepare(polyvm.plonk_commit_sizes(G))
    polyvm.plonk_prove(B, polyvm.plonk_inputs(B, G))
    ctx.sync()
    peak = B.gsz_queue_peak
    del B
    ctx.close()
    return rec.requests, peak


def serve(ctx, B, source, requests):
    ctx.sync()
    t0 = time.perf_counter()
    for kind, n in requests:
        out = source.doubles(B, n) if kind == "doubles" else source.rands(B, n)
        del out
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3


def lanes_times(czk_amd, requests, parties, reps):
    import torch
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    keys = [bytes([17 * p + 1]) * 32 for p in range(parties)]
    res = {}
    for name, make in (("dn", lambda: polyvm.DnSource(keys=keys)), ("dn_nocheck", lambda: polyvm.DnSource(keys=keys, check=False)), ("dealer", lambda: polyvm.SeededDealer(5))):
        src = make()
        B = polyvm.GpuBackend(czk_amd, ctx, parties, 64, sharing=polyvm.Sharing(1, parties, src, scheme="gsz"))
        t = [serve(ctx, B, src, requests) for _ in range(reps + 1)][1:]
        res[name] = {"ms_median": round(statistics.median(t), 2), "ms_min": round(min(t), 2)}
        del B
        torch.cuda.empty_cache()
    ctx.close()
    return res


def _net_party(rank, world, q, idb, requests, reps):
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    sys.path.insert(0, ROOT)
    import torch
    import czk_amd
    torch.cuda.set_device(0)
    c = czk_amd.Context(0)
    net = czk_amd.Net(c, czk_amd.CZK_NET_SHM, rank, world, idb, options={"timeout_ms": 600000})
    d, key = (world - 1) // 2, bytes([17 * rank + 1]) * 32
    times, seq, stats = [], 0, None
    for rep in range(reps + 1):
        net.barrier()
        net.stats_reset()
        t0 = time.perf_counter()
        for name, n in requests:
            kind = 0 if name == "doubles" else 1
            deal, outputs = net.gsz_dn_counts(kind, d, n + 2)
            r = torch.empty((outputs, 4), dtype=torch.int64, device="cuda")
            r2 = torch.empty_like(r) if kind == 0 else None
            nonce = kind.to_bytes(4, "little") + seq.to_bytes(8, "little")
            seq += 1
            net.gsz_dn_generate(kind, d, key, nonce, deal, r.data_ptr(), None if r2 is None else r2.data_ptr())
            ok, bad = net.gsz_dn_check(kind, d, r.data_ptr(), None if r2 is None else r2.data_ptr(), outputs)
            assert ok and not bad
            del r, r2
        c.sync()
        net.barrier()
        if rep:
            times.append((time.perf_counter() - t0) * 1e3)
        stats = net.stats()
    net.close()
    c.close()
    q.put((rank, times, stats))


def net_times(world, requests, reps):
    import multiprocessing as mp
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    idb = os.urandom(16)
    procs = [mpc.Process(target=_net_party, args=(r, world, q, idb, requests, reps)) for r in range(world)]
    for p in procs:
        p.start()
    import queue
    got = []
    while len(got) < world:
        try:
            got.append(q.get(timeout=1.0))
        except queue.Empty:
            if any(p.exitcode not in (None, 0) for p in procs):          # a rank that died never reports
                for p in procs:
                    if p.is_alive():
                        p.kill()
                raise SystemExit("a rank died: " + str([p.exitcode for p in procs]))
    got.sort()
    for p in procs:
        p.join(timeout=60)
    per_rep = [max(t[i] for _, t, _ in got) for i in range(reps)]              # a repetition ends when its slowest rank does
    return {"transport": "shm", "ms_median": round(statistics.median(per_rep), 2), "ms_min": round(min(per_rep), 2),
            "bytes_sent_per_party": [s["bytes_sent"] for _, _, s in got], "broadcasts_per_party": [s["broadcasts"] for _, _, s in got]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-gates", type=int, default=18)
    ap.add_argument("--parties", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--net", type=int, default=0, metavar="WORLD")
    ap.add_argument("--out")
    a = ap.parse_args()
    import czk_amd
    parties = a.net or a.parties
    requests, peak = record_requests(czk_amd, a.log_gates, parties)
    D, Rn = (sum(n for k, n in requests if k == which) for which in ("doubles", "rands"))
    res = {"tool": "gsz_dn_bench", "log_gates": a.log_gates, "parties": parties, "requests": len(requests), "doubles": D, "rands": Rn,
           "largest_request": max(n for _, n in requests), "queue_peak_triples": peak}
    res["lanes"] = lanes_times(czk_amd, requests, parties, a.reps)
    if a.net:
        res["net"] = net_times(a.net, requests, a.reps)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
