#!/usr/bin/env python3
"""Time of Marlin's index on the GPU (czk_amd.marlin.index) for the squaring chain, |H| = |K| = 2^--min-log .. 2^--max-log, split by phase, beside the wall
time of the hand-built index of the same circuit (tests/polyiop_real.py::marlin_real_inputs, big integers element by element) at 2^--old-log.

  balance       square_and_balance: host numpy on the CSR index arrays
  arithmetize   upload of the three CSR matrices + three czk_marlin_arithmetize calls (row / col / val / row_col on K)
  transforms    12 inverse transforms on K and 12 forward transforms on B (|B| = 4 |K|), one lane call each
  commitments   12 G1 MSMs of |K| scalars (one czk_msm_async call of 12 lanes) and their conversion to affine
  matrices_T    the transposed, re-indexed matrices for calculate_t: host transposes + czk_r1cs_matrix_register

Each phase ends in a synchronisation (index(timings=...)); the figure per size is the median of --reps runs after one warm-up run at that size, and
"total" is the wall time of a call without the phase synchronisations.  One JSON object per line; --write replaces the table between the
marlin_index_bench markers of EXPERIMENTS.md and writes profiles/marlin_index_bench.txt; --out PATH also writes the lines to PATH, and --from-file PATH takes them from such a file instead of measuring.

    python tools/marlin_index_bench.py [--min-log 16] [--max-log 20] [--reps 3] [--old-log 16] [--write] [--out PATH] [--from-file PATH]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
BEGIN, END = "<!-- marlin_index_bench:begin -->", "<!-- marlin_index_bench:end -->"
PHASES = ("balance", "arithmetize", "transforms", "commitments", "matrices_T")


def chain_matrices(np, mont, H):
    """the CSR matrices of marlin_real_inputs' circuit (formatted input [1, out], H - 2 witnesses, one entry per row), without a Python loop"""
    X, nw = 2, H - 2
    rp = np.arange(H + 1, dtype=np.uint64)
    wcols = np.arange(X, H, dtype=np.uint32)
    ones = np.tile(mont(1), (H, 1))
    three = ones.copy()
    three[-1] = mont(3)
    a = (rp, np.concatenate([wcols, np.array([0, 0], dtype=np.uint32)]), three)
    b = (rp, np.concatenate([wcols, np.array([1, 0], dtype=np.uint32)]), ones)
    c = (rp, np.concatenate([wcols[1:], np.array([1, 1, 0], dtype=np.uint32)]), three)
    return a, b, c, X, nw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-log", type=int, default=16)
    ap.add_argument("--max-log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--old-log", type=int, default=16, help="size at which the hand-built index is timed (0 = skip)")
    ap.add_argument("--write", action="store_true", help="replace the marlin_index_bench table of EXPERIMENTS.md and profiles/marlin_index_bench.txt")
    ap.add_argument("--out", default=None)
    ap.add_argument("--from-file", default=None, help="do not measure: take the lines an earlier run wrote with --out (for --write on another machine)")
    args = ap.parse_args()
    if args.from_file:
        return write(args, [json.loads(ln) for ln in open(args.from_file) if ln.strip()])
    import numpy as np
    import czk_amd
    from czk_amd import marlin, polyvm

    ctx = polyvm.shared_stream_context(czk_amd)
    B = polyvm.GpuBackend(czk_amd, ctx, 1, 1 << args.max_log)                  # the index commits polynomials of |K| coefficients
    rows = []

    def report(**row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def release(idx):
        ctx.sync()
        for handle, _, _ in idx["matrices_T"].values():
            handle.release()

    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    for log_h in range(args.min_log, args.max_log + 1):
        H = 1 << log_h
        a, b, c, X, nw = chain_matrices(np, polyvm.mont, H)
        B.prepare([H])
        release(marlin.index(B, a, b, c, X, nw))                               # warm-up: domain tables, table sets of this length
        laps, totals = [], []
        for _ in range(args.reps):
            t = {}
            release(marlin.index(B, a, b, c, X, nw, timings=t))
            laps.append(t)
            ctx.sync()
            t0 = time.perf_counter()
            idx = marlin.index(B, a, b, c, X, nw)
            ctx.sync()
            totals.append(time.perf_counter() - t0)
            release(idx)
        assert idx["H"] == idx["K"] == H and idx["b_size"] == 4 * H
        report(op="marlin.index", log_h=log_h, **{p + "_ms": round(med([t[p] for t in laps]) * 1e3, 2) for p in PHASES}, total_ms=round(med(totals) * 1e3, 2))
        del idx
    if args.old_log:
        import polyiop_real
        H = 1 << args.old_log
        ctx.sync()
        t0 = time.perf_counter()
        old = polyiop_real.marlin_real_inputs(B, polyvm, H, 0x3A21 + H)
        ctx.sync()
        report(op="polyiop_real.marlin_real_inputs (index and assignment, host big integers)", log_h=args.old_log, total_ms=round((time.perf_counter() - t0) * 1e3))
        del old
    ctx.close()
    write(args, rows)


def write(args, rows):
    lines = [json.dumps(r) for r in rows]
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")
    if args.write:
        open(os.path.join(ROOT, "profiles", "marlin_index_bench.txt"), "w").write("\n".join(lines) + "\n")
        path = os.path.join(ROOT, "EXPERIMENTS.md")
        txt = open(path).read()
        if BEGIN not in txt or END not in txt:
            raise SystemExit("EXPERIMENTS.md has no marlin_index_bench markers")
        table = ["| measurement | " + " | ".join(p + " ms" for p in PHASES) + " | total ms |", "|---|" + "---|" * (len(PHASES) + 1)]
        for r in rows:
            table.append(f"| {r['op']}, 2^{r['log_h']} | " + " | ".join(str(r.get(p + "_ms", "")) for p in PHASES) + f" | {r['total_ms']} |")
        txt = txt[:txt.index(BEGIN) + len(BEGIN)] + "\n" + "\n".join(table) + "\n" + txt[txt.index(END):]
        open(path, "w").write(txt)


if __name__ == "__main__":
    main()
