// pairing_steps.h -- the device steps of the BLS12-377 pairing that pairing.hip (products of pairings, Groth16 verification) and pairing_share.hip
// (pairings of shared points) both run: the two line steps of G2Prepared::from, ell, the Miller loop and the final exponentiation, with their constants.
// The register budget and the SoA workspace are described at the head of pairing.hip.  Built with -DCZK_NOINLINE_MUL only (tower.h has no other form).
#pragma once
#include "curve.h"
#include "tower.h"

namespace czk {

constexpr u64 PAIRING_X = 0x8508c00000000001ull;   // mod.rs:16; bit 63 set: BitIteratorBE(X).skip(1) = bits 62..0
constexpr int LINES = 69;                          // 63 doubling steps + 6 addition steps (popcount(X) - 1)
constexpr size_t LINE_WORDS = (size_t)LINES * 36;  // (c0, c1, c2) of Fq2 = 36 u64 per line
constexpr int PAIR_BLOCK = 64;

// ------------------------------------------------------------------------------------------------- G2 preparation
// g2.rs:105-132 doubling_step on homogeneous projective (x, y, z); D-twist coefficients (-h, 3 j, i)
CZK_D void doubling_step(Fq2& rx, Fq2& ry, Fq2& rz, Fq2& l0, Fq2& l1, Fq2& l2) {
    const Fq two_inv = fq_const(PAIRING_TWO_INV);
    Fq2 coeff_b = Fq2::zero();
    coeff_b.c1 = fq_const(PAIRING_G2_B_C1);
    Fq2 a = fq2_mul_fq(f_mul(rx, ry), two_inv);
    Fq2 b = f_sqr(ry);
    Fq2 c = f_sqr(rz);
    Fq2 e = f_mul(coeff_b, f_add(f_dbl(c), c));
    Fq2 f = f_add(f_dbl(e), e);
    Fq2 g = fq2_mul_fq(f_add(b, f), two_inv);
    Fq2 h = f_sub(f_sqr(f_add(ry, rz)), f_add(b, c));
    Fq2 i = f_sub(e, b);
    Fq2 j = f_sqr(rx);
    Fq2 e_square = f_sqr(e);
    rx = f_mul(a, f_sub(b, f));
    ry = f_sub(f_sqr(g), f_add(f_dbl(e_square), e_square));
    rz = f_mul(b, h);
    l0 = f_neg(h);
    l1 = f_add(f_dbl(j), j);
    l2 = i;
}
// g2.rs:134-157 addition_step; D-twist coefficients (lambda, -theta, j)
CZK_D void addition_step(Fq2& rx, Fq2& ry, Fq2& rz, const Fq2& qx, const Fq2& qy, Fq2& l0, Fq2& l1, Fq2& l2) {
    Fq2 theta = f_sub(ry, f_mul(qy, rz));
    Fq2 lambda = f_sub(rx, f_mul(qx, rz));
    Fq2 c = f_sqr(theta);
    Fq2 d = f_sqr(lambda);
    Fq2 e = f_mul(lambda, d);
    Fq2 f = f_mul(rz, c);
    Fq2 g = f_mul(rx, d);
    Fq2 h = f_sub(f_add(e, f), f_dbl(g));
    rx = f_mul(lambda, h);
    ry = f_sub(f_mul(theta, f_sub(g, h)), f_mul(e, ry));
    rz = f_mul(rz, e);
    l0 = lambda;
    l1 = f_neg(theta);
    l2 = f_sub(f_mul(theta, qx), f_mul(lambda, qy));
}

// ------------------------------------------------------------------------------------------------- Miller loop
// mod.rs:54-72 ell, TwistType::D: f *= (c0 p.y, 0, 0) + (c1 p.x, c2, 0) w
CZK_D void ell(Fq12& f, const u64* lines, size_t stride, int j, const G1Affine& p) {
    const u64* c = lines + (size_t)j * 36 * stride;
    const Fq2 c0 = fq2_mul_fq(fq2_load_strided(c, stride), p.y);
    const Fq2 c1 = fq2_mul_fq(fq2_load_strided(c + 12 * stride, stride), p.x);
    const Fq2 c2 = fq2_load_strided(c + 24 * stride, stride);
    f = fq12_mul_by_034(f, c0, c1, c2);
}

// mod.rs:94-126: `each(f, j)` applies line j of every (non-skipped) pair of the product
template <class Each>
CZK_D Fq12 miller_loop(Each each) {
    Fq12 f = Fq12::one();
    int j = 0;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        f = f_sqr(f);
        each(f, j++);
        if ((PAIRING_X >> b) & 1) each(f, j++);
    }
    return f;   // X_IS_NEGATIVE = false: no conjugation
}

// ------------------------------------------------------------------------------------------------- final exponentiation
// exp_by_x (mod.rs:74-80): cyclotomic_exp by X, input read from the workspace slot at p.  Binary square-and-multiply from the top
// bit (63 cyclotomic squarings, 6 products); the reference's NAF chain reaches the same element.
CZK_D Fq12 exp_by_x(const u64* p, size_t s) {
    Fq12 res = fq12_load_strided(p, s);
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        res = fq12_cyclotomic_square(res);
        if ((PAIRING_X >> b) & 1) res = f_mul(res, fq12_load_strided(p, s));
    }
    return res;
}

// mod.rs:128-193, step for step.  ws: three Fq12 slots of this thread (stride s = threads of the launch): S0 = r, S1 = y0, S2 = y1.
CZK_D Fq12 final_exponentiation(const Fq12& f, u64* ws, size_t s) {
    u64 *S0 = ws, *S1 = ws + 72 * s, *S2 = ws + 144 * s;
    {
        Fq12 r = f_mul(fq12_conj(f), f_inv(f));                 // f^(p^6 - 1)
        r = f_mul(fq12_frobenius(r, 2), r);                     // f^((p^6 - 1)(p^2 + 1))
        fq12_store_strided(S0, s, r);
        fq12_store_strided(S1, s, fq12_cyclotomic_square(r));   // y0
    }
    {
        Fq12 y1 = f_mul(exp_by_x(S0, s), fq12_conj(fq12_load_strided(S0, s)));   // y1 = r^x; y2 = conj(r); y1 *= y2
        fq12_store_strided(S2, s, y1);
    }
    {
        Fq12 y2 = exp_by_x(S2, s);                                                 // y2 = y1^x
        fq12_store_strided(S2, s, f_mul(fq12_conj(fq12_load_strided(S2, s)), y2)); // y1 = conj(y1) * y2
    }
    {
        Fq12 y2 = exp_by_x(S2, s);                                                     // y2 = y1^x
        fq12_store_strided(S2, s, f_mul(fq12_frobenius(fq12_load_strided(S2, s), 1), y2));   // y1 = frob(y1, 1) * y2
    }
    fq12_store_strided(S0, s, f_mul(fq12_load_strided(S0, s), fq12_load_strided(S1, s)));   // r *= y0
    fq12_store_strided(S1, s, exp_by_x(S2, s));                                            // y0 = y1^x
    Fq12 y2 = exp_by_x(S1, s);                                                             // y2 = y0^x
    Fq12 y1 = f_mul(fq12_conj(fq12_load_strided(S2, s)), y2);                              // y1 = conj(y1) * y2
    y1 = f_mul(y1, fq12_frobenius(fq12_load_strided(S2, s), 2));                           // y1 *= frob(y1_old, 2)
    return f_mul(fq12_load_strided(S0, s), y1);                                            // r *= y1
}

}  // namespace czk
