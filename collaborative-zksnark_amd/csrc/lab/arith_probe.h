// arith_probe.h -- LAB BUILD ONLY: runs one function of fqu.h / fru.h / te.h / fq2pu.h on raw limbs (arith_probe.hip).
//
// Not part of the product ABI (include/czk.h): exported by libczk_hip_lab.so alone, for tests that hold the unsaturated arithmetic
// to a big-integer model at operands a whole MSM or NTT reaches with probability ~2^-26 (tests/test_lazy_arith.py).
//
// Item t of `in` is in_words_per_item u32: the operands' limbs exactly as given (14 per FqU, 9 per FrU, 12 / 8 per packed Fq / Fr;
// no unpacking, no normalisation), in the order of the function's parameters; a point at infinity is a flag word after the point's
// coordinates; an Fq2U is c0 then c1.  Item t of `out` receives the raw result limbs, then a flag word for the functions that return
// bool (1 = true) or maintain an infinity flag.  The words per item must equal what the op expects (CZK_ERR_ARG otherwise).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct czk_ctx czk_ctx;

enum czk_lab_arith_op {
    // fqu.h primitives                      in -> out (u32 words per item)
    CZK_PROBE_FQU_MUL = 0,                // a, b : 28 -> 14
    CZK_PROBE_FQU_SQR = 1,                // a : 14 -> 14
    CZK_PROBE_FQU_MUL_ADD = 2,            // a, b, c, d : 56 -> 14
    CZK_PROBE_FQU_MUL_ADD_HI = 3,         // a, b, c, d, e : 70 -> 14
    CZK_PROBE_FQU_MUL_HI = 4,             // a, b, e : 42 -> 14
    CZK_PROBE_FQU_MUL_ADD4 = 5,           // a .. h : 112 -> 14
    CZK_PROBE_FQU_NORMALIZE = 6,          // 14 -> 14
    CZK_PROBE_FQU_SUB_LAZY_4 = 7,         // a, b : 28 -> 14
    CZK_PROBE_FQU_SUB_LAZY_8 = 8,
    CZK_PROBE_FQU_SUB_LAZY_16 = 9,
    CZK_PROBE_FQU_SUB3_NORM = 10,         // a, b, c : 42 -> 14
    CZK_PROBE_FQU_UNPACK = 11,            // 12 -> 14
    CZK_PROBE_FQU_PACK = 12,              // 14 -> 12
    CZK_PROBE_FQU_NEG5 = 13,              // fqu_neg5<false> : 14 -> 14
    CZK_PROBE_FQU_NEG5_BIG = 14,          // fqu_neg5<true>
    CZK_PROBE_FQU_ADD_LAZY = 15,          // a, b : 28 -> 14
    CZK_PROBE_FQU_SUBN_32 = 16,           // a, b : 28 -> 14
    CZK_PROBE_FQU_SUBN_64 = 17,
    CZK_PROBE_FQU_SUBN_128 = 18,
    // Fq2U products
    CZK_PROBE_FQ2U_MUL = 20,              // a, b : 56 -> 28
    CZK_PROBE_FQ2U_SQR = 21,              // a : 28 -> 28
    CZK_PROBE_FQ2U_MUL_N5 = 22,           // a, b (n5b1 = fqu_neg5<false>(b.c1)) : 56 -> 28
    // G1 / G2 formulas of fqu.h
    CZK_PROBE_FQU_XYZZ_ACC_MIXED = 30,    // ax, ay, azz, azzz, qx, qy : 84 -> 56 + returned bool
    CZK_PROBE_XYZZU_ADD = 31,             // a + inf, b + inf : 114 -> 56 + inf
    CZK_PROBE_XYZZU_DOUBLE = 32,          // a + inf : 57 -> 56 + inf
    CZK_PROBE_XYZZU_TO_SAT = 33,          // a + inf : 57 -> 4 x 12
    CZK_PROBE_XYZZU_FROM_SAT = 34,        // 4 x 12 : 48 -> 56 + inf
    CZK_PROBE_FQ2U_XYZZ_ACC_MIXED = 35,   // ax, ay, azz, azzz, qx, qy (Fq2U each) : 168 -> 112 + returned bool
    // te.h
    CZK_PROBE_TEU_FROM_NIELS = 40,        // ym, yp, k2 : 42 -> 56
    CZK_PROBE_TEU_MADD = 41,              // a, ym, yp, k2 : 98 -> 56
    CZK_PROBE_TEU_ADD = 42,               // a, b : 112 -> 56
    CZK_PROBE_TEU_DOUBLE = 43,            // a : 56 -> 56
    CZK_PROBE_TEU_TO_JAC = 44,            // a : 56 -> 3 x 12
    CZK_PROBE_TE_LOAD_NIELS = 45,         // one 48-word table entry, neg flag, 3 pad words : 52 -> ym, yp, k2 = 42
    // fq2pu.h: item t runs on lanes 2 t (c0 halves) and 2 t + 1 (c1 halves); memory holds whole Fq2 values, c0 then c1
    CZK_PROBE_P2_MUL = 50,                // a, b, BIG flag : 57 -> 28
    CZK_PROBE_XYZZU2_ADD = 51,            // a + inf, b + inf : 226 -> 112 + inf
    CZK_PROBE_XYZZU2_DOUBLE = 52,         // a + inf : 113 -> 112 + inf
    CZK_PROBE_XYZZU2_ACC_MIXED = 53,      // ax, ay, azz, azzz, qx, qy : 168 -> 112 + returned bool
    // fru.h
    CZK_PROBE_FRU_MUL = 60,               // a, b : 18 -> 9
    CZK_PROBE_FRU_NORMALIZE = 62,         // 9 -> 9
    CZK_PROBE_FRU_UNPACK = 63,            // 8 -> 9
    CZK_PROBE_FRU_PACK = 64,              // 9 -> 8
    CZK_PROBE_FRU_REDUCE_2R = 65,         // 9 -> 9
    CZK_PROBE_FRU_CANON = 66,             // 9 -> 8
    CZK_PROBE_FRU_CANON_MULOUT = 67,      // 9 -> 8
    CZK_PROBE_FRU_ADD = 68,               // a, b : 18 -> 9
    // fru_sub<K, U> for every FruC<K, U> of fru_constants.inc (K = 2 .. 256, U = 1, 2): op = BASE + 2 log2(K) + (U - 1); a, b : 18 -> 9
    CZK_PROBE_FRU_SUB_BASE = 100,
};

// mem: CZK_MEM_HOST or CZK_MEM_DEVICE for both buffers.
int czk_lab_arith_probe(czk_ctx* ctx, int op, const uint32_t* in, size_t in_words_per_item, uint32_t* out, size_t out_words_per_item,
                        size_t n, int mem);

#ifdef __cplusplus
}
#endif
