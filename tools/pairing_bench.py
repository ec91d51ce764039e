#!/usr/bin/env python3
"""Pairings/s (czk_pairing) and Groth16 verifications/s (czk_groth16_verify) at k = 1, 64, 1024, 16384, 65536 on one GPU.

Inputs live in device memory (CZK_MEM_DEVICE) so the timed region is the library call: its workspace allocations, the G2 preparation, the
Miller loops and final exponentiations.  Timing: torch.cuda events on the context's stream; one warm-up call per size, then three windows of
at least --window seconds each (as many whole calls as fit), reporting every window's rate.  The Fq-multiplication count per operation is
COMPUTED from the formulas of csrc/tower.h / pairing.hip (op_counts()), not measured.  Prints one JSON object per size and a summary line.

    python tools/pairing_bench.py [--sizes 1,64,1024,16384,65536] [--window 1.0]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def op_counts():
    """Fq multiplications (squarings counted as multiplications) per operation, from the formulas."""
    m2, s2, mf = 3, 2, 2                  # Fq2 mul (Karatsuba), Fq2 square, Fq2 x Fq
    m6 = 6 * m2                           # Fq6 mul
    mul01 = 5 * m2                        # Fq6 mul_by_01
    m12, s12 = 3 * m6, 2 * m6             # Fq12 mul, square
    line = 2 * mf + 3 * m2 + 2 * mul01    # ell: c0 p.y, c1 p.x, mul_by_034
    cyc = 6 * m2                          # cyclotomic_square
    fq_inv = 376 + 376 // 2               # Fermat a^(q-2): ~376 squarings + ~half as many products (q - 2 has 190 one bits)
    fq6_inv = 3 * s2 + 6 * m2 + 3 * m2 + (s2 + 1) + fq_inv + 2 * m2 + 3 * m2
    fq12_inv = 2 * m6 + fq6_inv + 2 * m6
    frob = 10 * mf                        # frobenius_map(1 | 2): 10 Fq2 x Fq products
    exp_x = 63 * cyc + 6 * m12
    fexp = fq12_inv + m12 + frob + m12 + cyc + 5 * exp_x + 7 * m12 + 3 * frob
    miller = lambda pairs: 63 * s12 + 69 * pairs * line   # noqa: E731
    dbl = 3 * m2 + 6 * s2 + 2 * mf        # doubling_step
    add = 11 * m2 + 2 * s2                # addition_step
    prep = 63 * dbl + 6 * add
    g1_dbl, g1_add = 6, 11                # Jacobian doubling (a = 0), mixed addition
    return {"miller_1": miller(1), "final_exp": fexp, "g2_prepare": prep, "pairing": prep + miller(1) + fexp,
            "g16_verify_m1": prep + miller(3) + fexp + 253 * g1_dbl + 127 * g1_add + 12 + fq_inv + 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,16384,65536")
    ap.add_argument("--window", type=float, default=1.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import czk_amd
    from util import R_MOD, ints_to_limbs, limbs_to_ints, rand_fr_canonical

    ts = torch.cuda.Stream()
    ctx = czk_amd.Context(0, ts.cuda_stream)
    L = ctx._L
    ops = op_counts()
    sizes = [int(s) for s in args.sizes.split(",")]
    kmax = max(sizes)
    # inputs: [a_i] G1, [b_i] G2; a valid Groth16 proof by discrete logs (alpha..delta, abc, x chosen) replicated k times
    a = limbs_to_ints(rand_fr_canonical(0xBE1, kmax))
    b = limbs_to_ints(rand_fr_canonical(0xBE2, kmax))
    g1 = ctx.fixed_base_points(czk_amd.CZK_G1, ints_to_limbs(a, 4))
    g2 = ctx.fixed_base_points(czk_amd.CZK_G2, ints_to_limbs(b, 4))
    al, be, ga, de, cc, x, abc = 11, 13, 17, 19, 23, 29, [31, 37]
    pa = 41
    pb = (al * be + (abc[0] + x * abc[1]) * ga + cc * de) * pow(pa, -1, R_MOD) % R_MOD
    fb = lambda grp, ks: ctx.fixed_base_points(grp, ints_to_limbs(ks, 4))   # noqa: E731
    pvk = ctx.groth16_pvk(fb(czk_amd.CZK_G1, [al])[0], *fb(czk_amd.CZK_G2, [be, ga, de]), fb(czk_amd.CZK_G1, abc))
    A = np.repeat(fb(czk_amd.CZK_G1, [pa]), kmax, axis=0)
    B = np.repeat(fb(czk_amd.CZK_G2, [pb]), kmax, axis=0)
    Cp = np.repeat(fb(czk_amd.CZK_G1, [cc]), kmax, axis=0)
    X = np.repeat(ints_to_limbs([x * (1 << 256) % R_MOD], 4), kmax, axis=0)
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to("cuda")   # noqa: E731
    with torch.cuda.stream(ts):
        d_g1, d_g2, d_a, d_b, d_c, d_x = (dev(v) for v in (g1, g2, A, B, Cp, X))
        d_out = torch.empty(kmax * 72, dtype=torch.int64, device="cuda")
        d_ok = torch.zeros(kmax, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

    def run_pairing(k):
        ctx._ck(L.czk_pairing(ctx._h, P(d_g1), None, P(d_g2), None, C.c_size_t(k), P(d_out), C.c_int(czk_amd.CZK_MEM_DEVICE)))

    def run_verify(k):
        ctx._ck(L.czk_groth16_verify(ctx._h, pvk._h, P(d_a), P(d_b), P(d_c), None, P(d_x), C.c_size_t(1), C.c_size_t(k), P(d_ok),
                                     C.c_int(czk_amd.CZK_MEM_DEVICE)))

    def windows(fn, k):
        fn(k)                                   # warm-up
        rates = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            calls = 0
            e0.record(ts)
            while True:
                fn(k)
                calls += 1
                e1.record(ts)
                e1.synchronize()
                ms = e0.elapsed_time(e1)
                if ms >= 1000 * args.window:
                    break
            rates.append(calls * k / (ms / 1000))
        return rates, ms / calls

    rows = []
    for k in sizes:
        pr, p_ms = windows(run_pairing, k)
        vr, v_ms = windows(run_verify, k)
        ok = d_ok[:k].cpu().numpy()
        assert ok.all(), "a valid proof failed to verify"
        row = {"k": k, "pairings_per_s": [round(r, 1) for r in pr], "pairing_call_ms": round(p_ms, 3),
               "verifications_per_s": [round(r, 1) for r in vr], "verify_call_ms": round(v_ms, 3),
               "fq_mul_per_s_pairing_G": round(max(pr) * ops["pairing"] / 1e9, 3),
               "fq_mul_per_s_verify_G": round(max(vr) * ops["g16_verify_m1"] / 1e9, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps({"op_counts_fq_mul": ops, "rows": len(rows)}))
    pvk.release()
    ctx.close()


if __name__ == "__main__":
    main()
