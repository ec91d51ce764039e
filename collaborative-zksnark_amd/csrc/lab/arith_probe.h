// arith_probe.h -- LAB BUILD ONLY: runs one function of fqu.h / fru.h / te.h / fq2pu.h (arith_probe.hip), or of the saturated field.h /
// tower.h / curve.h in either compile form (sat_probe.h), on raw limbs.
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
    // fqu.h: the signed-column (`_s`) forms of the multiplies; operands as above, within the signed-column contract
    CZK_PROBE_FQU_MUL_S = 70,             // a, b : 28 -> 14
    CZK_PROBE_FQU_SQR_S = 71,             // a : 14 -> 14
    CZK_PROBE_FQU_MUL_ADD_S = 72,         // a, b, c, d : 56 -> 14
    CZK_PROBE_FQU_MUL_ADD_HI_S = 73,      // a, b, c, d, e : 70 -> 14
    CZK_PROBE_FQU_MUL_HI_S = 74,          // a, b, e : 42 -> 14
    CZK_PROBE_FQU_MUL_ADD4_S = 75,        // a .. h : 112 -> 14
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
    // the SATURATED arithmetic (field.h, tower.h, curve.h; sat_probe.h): op = BASE + 2 fn + form, fn from czk_lab_sat_fn below,
    // form 0 = compiled with the Montgomery multiply inlined (arith_probe.hip), 1 = with -DCZK_NOINLINE_MUL (sat_probe.hip)
    CZK_PROBE_SAT_BASE = 200,
};

// Words per item: Fr 8, Fq 12, Fq2 24, Fq6 72, Fq12 144, in the reference's nesting; W below = the words of the op's field.
enum czk_lab_sat_fn {
    // Fp<P>: fn = CZK_SAT_FR_BASE / CZK_SAT_FQ_BASE + one of these
    CZK_SAT_FP_ADD = 0,                   // a, b : 2 W -> W
    CZK_SAT_FP_SUB = 1,                   // a, b
    CZK_SAT_FP_DBL = 2,                   // a : W -> W
    CZK_SAT_FP_NEG = 3,
    CZK_SAT_FP_REDUCE = 4,                // any a < 2^(32 N)
    CZK_SAT_FP_MUL = 5,                   // a, b
    CZK_SAT_FP_SQR = 6,
    CZK_SAT_FP_INTO_REPR = 7,
    CZK_SAT_FP_FROM_REPR = 8,
    CZK_SAT_FP_INV = 9,
    CZK_SAT_FR_BASE = 0,
    CZK_SAT_FQ_BASE = 10,
    CZK_SAT_FQ_MUL_BY_NONRESIDUE = 20,
    CZK_SAT_FQ2_ADD = 21,                 // a, b : 48 -> 24
    CZK_SAT_FQ2_SUB = 22,
    CZK_SAT_FQ2_DBL = 23,                 // a : 24 -> 24
    CZK_SAT_FQ2_NEG = 24,
    CZK_SAT_FQ2_MUL = 25,                 // a, b
    CZK_SAT_FQ2_SQR = 26,
    CZK_SAT_FQ2_INV = 27,
    CZK_SAT_FQ2_MUL_BY_U = 28,
    CZK_SAT_FQ2_MUL_FQ = 29,              // a, k (Fq) : 36 -> 24
    CZK_SAT_FQ2_CONJ = 30,
    // curve.h: fn = CZK_SAT_G1_BASE (F = Fq) / CZK_SAT_G2_BASE (F = Fq2) + one of these
    CZK_SAT_JAC_DOUBLE = 0,               // p : 3 W -> 3 W
    CZK_SAT_JAC_ADD_MIXED = 1,            // p, q affine, q_inf : 5 W + 1 -> 3 W
    CZK_SAT_JAC_ADD = 2,                  // p, q : 6 W -> 3 W
    CZK_SAT_JAC_TO_AFFINE = 3,            // p : 3 W -> 2 W + returned bool
    CZK_SAT_XYZZ_DOUBLE_AFFINE = 4,       // q affine : 2 W -> 4 W
    CZK_SAT_XYZZ_DOUBLE = 5,              // p : 4 W -> 4 W
    CZK_SAT_XYZZ_ADD_MIXED = 6,           // p, q affine : 6 W -> 4 W
    CZK_SAT_XYZZ_ACC_MIXED = 7,           // ax, ay, azz, azzz, qx, qy : 6 W -> 4 W
    CZK_SAT_XYZZ_ADD = 8,                 // p, q : 8 W -> 4 W
    CZK_SAT_XYZZ_TO_JAC = 9,              // p : 4 W -> 3 W
    CZK_SAT_G1_BASE = 31,
    CZK_SAT_G2_BASE = 41,
    // tower.h: form 1 only (the tower is never compiled with the multiply inlined)
    CZK_SAT_FQ6_ADD = 51,                 // a, b : 144 -> 72
    CZK_SAT_FQ6_SUB = 52,
    CZK_SAT_FQ6_NEG = 53,                 // a : 72 -> 72
    CZK_SAT_FQ6_MUL_BY_V = 54,
    CZK_SAT_FQ6_MUL = 55,                 // a, b
    CZK_SAT_FQ6_MUL_BY_01 = 56,           // a, c0, c1 (Fq2) : 120 -> 72
    CZK_SAT_FQ6_MUL_BY_1 = 57,            // a, c1 (Fq2) : 96 -> 72
    CZK_SAT_FQ6_INV = 58,
    CZK_SAT_FQ6_FROBENIUS_1 = 59,
    CZK_SAT_FQ6_FROBENIUS_2 = 60,
    CZK_SAT_FQ12_MUL = 61,                // a, b : 288 -> 144
    CZK_SAT_FQ12_SQR = 62,                // a : 144 -> 144
    CZK_SAT_FQ12_CONJ = 63,
    CZK_SAT_FQ12_INV = 64,
    CZK_SAT_FQ12_MUL_BY_034 = 65,         // a, c0, c3, c4 (Fq2) : 216 -> 144
    CZK_SAT_FQ12_FROBENIUS_1 = 66,
    CZK_SAT_FQ12_FROBENIUS_2 = 67,
    CZK_SAT_FQ12_CYCLOTOMIC_SQUARE = 68,
    // the n items of a call as ONE batch: fq12_load_strided from u64 word w of item t at [72 t + w] (_1) or [w n + t] (_N, SoA) to packed
    // items, and fq12_store_strided from packed items to those layouts : 144 -> 144
    CZK_SAT_FQ12_LOAD_STRIDED_1 = 69,
    CZK_SAT_FQ12_STORE_STRIDED_1 = 70,
    CZK_SAT_FQ12_LOAD_STRIDED_N = 71,
    CZK_SAT_FQ12_STORE_STRIDED_N = 72,
    CZK_SAT_FN_COUNT = 73,
};

// mem: CZK_MEM_HOST or CZK_MEM_DEVICE for both buffers.
int czk_lab_arith_probe(czk_ctx* ctx, int op, const uint32_t* in, size_t in_words_per_item, uint32_t* out, size_t out_words_per_item,
                        size_t n, int mem);

#ifdef __cplusplus
}

namespace czk {
// sat_probe.hip: the form-1 ops, reached through czk_lab_arith_probe's switch (which has validated every argument but fn)
int sat_probe_noinline(czk_ctx* ctx, int fn, const uint32_t* in, size_t in_words_per_item, uint32_t* out, size_t out_words_per_item, size_t n, int mem);
}
#endif
