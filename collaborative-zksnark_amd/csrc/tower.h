// tower.h -- BLS12-377 Fq6 / Fq12 tower arithmetic on field.h's Montgomery Fq / Fq2, for the pairing (pairing.hip).
//
//   Fq6  = Fq2[v]/(v^3 - u)   (curves/bls12_377/src/fields/fq6.rs:12-14: NONRESIDUE = u)
//   Fq12 = Fq6[w]/(w^2 - v)   (fq12.rs:12: NONRESIDUE = v)
//
// Every operation returns the unique reduced field element the reference's (fp6_3over2.rs, fp12_2over3over2.rs,
// cubic_extension.rs, quadratic_extension.rs) returns; where the reference has a special form (mul_by_034, mul_by_01,
// cyclotomic_square) it is restated line by line.  Memory layout = the reference's nesting: an Fq12 is 72 u64,
// c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1, each Fq 6 Montgomery limbs.
//
// The Frobenius coefficients, 1/2 and the D-twist's COEFF_B come from pairing_constants.inc, which tools/gen_pairing_constants.py
// derives from q.
#pragma once
#include "field.h"
#include "pairing_constants.inc"

namespace czk {

CZK_HD Fq fq_const(const u32 (&m)[12]) {
    Fq r;
#pragma unroll
    for (int i = 0; i < 12; i++) r.l[i] = m[i];
    return r;
}

// ------------------------------------------------------------------------------------------------- Fq2 helpers
// u * a = (beta a1, a0)   (fq6.rs: mul_fp2_by_nonresidue with NONRESIDUE = u)
CZK_HD Fq2 fq2_mul_by_u(const Fq2& a) { return Fq2{fq_mul_by_nonresidue(a.c1), a.c0}; }
// mul_assign_by_fp
CZK_HD Fq2 fq2_mul_fq(const Fq2& a, const Fq& k) { return Fq2{fp_mul(a.c0, k), fp_mul(a.c1, k)}; }
// frobenius_map(odd) on Fq2 = conjugation (FROBENIUS_COEFF_FP2_C1[1] = -1)
CZK_HD Fq2 fq2_conj(const Fq2& a) { return Fq2{a.c0, fp_neg(a.c1)}; }

// ------------------------------------------------------------------------------------------------- Fq6
struct Fq6 {
    Fq2 c0, c1, c2;
    static CZK_HD Fq6 zero() { return Fq6{Fq2::zero(), Fq2::zero(), Fq2::zero()}; }
    static CZK_HD Fq6 one() { return Fq6{Fq2::one(), Fq2::zero(), Fq2::zero()}; }
    CZK_HD bool operator==(const Fq6& b) const { return c0 == b.c0 && c1 == b.c1 && c2 == b.c2; }
};
CZK_HD Fq6 f_add(const Fq6& a, const Fq6& b) { return Fq6{f_add(a.c0, b.c0), f_add(a.c1, b.c1), f_add(a.c2, b.c2)}; }
CZK_HD Fq6 f_sub(const Fq6& a, const Fq6& b) { return Fq6{f_sub(a.c0, b.c0), f_sub(a.c1, b.c1), f_sub(a.c2, b.c2)}; }
CZK_HD Fq6 f_neg(const Fq6& a) { return Fq6{f_neg(a.c0), f_neg(a.c1), f_neg(a.c2)}; }
// v * a = (u a2, a0, a1)   (fp12_2over3over2.rs:24-30 mul_fp6_by_nonresidue)
CZK_HD Fq6 fq6_mul_by_v(const Fq6& a) { return Fq6{fq2_mul_by_u(a.c2), a.c0, a.c1}; }
// cubic_extension.rs Mul (Devegili et al. Karatsuba): 6 Fq2 products
CZK_HD Fq6 f_mul(const Fq6& a, const Fq6& b) {
    Fq2 v0 = f_mul(a.c0, b.c0), v1 = f_mul(a.c1, b.c1), v2 = f_mul(a.c2, b.c2);
    Fq6 r;
    r.c0 = f_add(v0, fq2_mul_by_u(f_sub(f_sub(f_mul(f_add(a.c1, a.c2), f_add(b.c1, b.c2)), v1), v2)));
    r.c1 = f_add(f_sub(f_sub(f_mul(f_add(a.c0, a.c1), f_add(b.c0, b.c1)), v0), v1), fq2_mul_by_u(v2));
    r.c2 = f_add(f_sub(f_sub(f_mul(f_add(a.c0, a.c2), f_add(b.c0, b.c2)), v0), v2), v1);
    return r;
}
// fp6_3over2.rs mul_by_01: a * (c0 + c1 v)
CZK_HD Fq6 fq6_mul_by_01(const Fq6& a, const Fq2& c0, const Fq2& c1) {
    Fq2 a_a = f_mul(a.c0, c0), b_b = f_mul(a.c1, c1);
    Fq2 t1 = f_add(fq2_mul_by_u(f_sub(f_mul(c1, f_add(a.c1, a.c2)), b_b)), a_a);
    Fq2 t3 = f_add(f_sub(f_mul(c0, f_add(a.c0, a.c2)), a_a), b_b);
    Fq2 t2 = f_sub(f_sub(f_mul(f_add(c0, c1), f_add(a.c0, a.c1)), a_a), b_b);
    return Fq6{t1, t2, t3};
}
// fp6_3over2.rs mul_by_1: a * (c1 v)
CZK_HD Fq6 fq6_mul_by_1(const Fq6& a, const Fq2& c1) {
    Fq2 b_b = f_mul(a.c1, c1);
    Fq2 t1 = fq2_mul_by_u(f_sub(f_mul(c1, f_add(a.c1, a.c2)), b_b));
    Fq2 t2 = f_sub(f_mul(c1, f_add(a.c0, a.c1)), b_b);
    return Fq6{t1, t2, b_b};
}
// cubic_extension.rs inverse (Guide to Pairing-based Cryptography, Algorithm 5.23)
CZK_HD Fq6 f_inv(const Fq6& a) {
    Fq2 t0 = f_sub(f_sqr(a.c0), fq2_mul_by_u(f_mul(a.c1, a.c2)));
    Fq2 t1 = f_sub(fq2_mul_by_u(f_sqr(a.c2)), f_mul(a.c0, a.c1));
    Fq2 t2 = f_sub(f_sqr(a.c1), f_mul(a.c0, a.c2));
    Fq2 n = f_add(f_mul(a.c0, t0), fq2_mul_by_u(f_add(f_mul(a.c2, t1), f_mul(a.c1, t2))));
    Fq2 ni = f_inv(n);
    return Fq6{f_mul(t0, ni), f_mul(t1, ni), f_mul(t2, ni)};
}
// cubic_extension.rs frobenius_map for power 1 or 2 (coefficients in Fq)
CZK_HD Fq6 fq6_frobenius(const Fq6& a, int power) {
    if (power == 1) {
        return Fq6{fq2_conj(a.c0), fq2_mul_fq(fq2_conj(a.c1), fq_const(PAIRING_FROB6_C1_1)), fq2_mul_fq(fq2_conj(a.c2), fq_const(PAIRING_FROB6_C2_1))};
    }
    return Fq6{a.c0, fq2_mul_fq(a.c1, fq_const(PAIRING_FROB6_C1_2)), fq2_mul_fq(a.c2, fq_const(PAIRING_FROB6_C2_2))};
}

// ------------------------------------------------------------------------------------------------- Fq12
struct Fq12 {
    Fq6 c0, c1;
    static CZK_HD Fq12 one() { return Fq12{Fq6::one(), Fq6::zero()}; }
    CZK_HD bool operator==(const Fq12& b) const { return c0 == b.c0 && c1 == b.c1; }
    CZK_HD bool is_one() const { return *this == one(); }
};
// quadratic_extension.rs Mul (Karatsuba): 3 Fq6 products
CZK_HD Fq12 f_mul(const Fq12& a, const Fq12& b) {
    Fq6 v0 = f_mul(a.c0, b.c0), v1 = f_mul(a.c1, b.c1);
    Fq6 c1 = f_sub(f_sub(f_mul(f_add(a.c0, a.c1), f_add(b.c0, b.c1)), v0), v1);
    return Fq12{f_add(v0, fq6_mul_by_v(v1)), c1};
}
// quadratic_extension.rs square (complex method): 2 Fq6 products
CZK_HD Fq12 f_sqr(const Fq12& a) {
    Fq6 v0 = f_sub(a.c0, a.c1);
    Fq6 v3 = f_sub(a.c0, fq6_mul_by_v(a.c1));
    Fq6 v2 = f_mul(a.c0, a.c1);
    v0 = f_add(f_mul(v0, v3), v2);
    return Fq12{f_add(v0, fq6_mul_by_v(v2)), f_add(v2, v2)};
}
CZK_HD Fq12 fq12_conj(const Fq12& a) { return Fq12{a.c0, f_neg(a.c1)}; }
// quadratic_extension.rs inverse: (c0 - c1 w) / (c0^2 - v c1^2)
CZK_HD Fq12 f_inv(const Fq12& a) {
    Fq6 n = f_sub(f_mul(a.c0, a.c0), fq6_mul_by_v(f_mul(a.c1, a.c1)));
    Fq6 ni = f_inv(n);
    return Fq12{f_mul(a.c0, ni), f_neg(f_mul(a.c1, ni))};
}
// fp12_2over3over2.rs:92-110 mul_by_034: a * ((c0, 0, 0) + (c3, c4, 0) w)
CZK_HD Fq12 fq12_mul_by_034(const Fq12& f, const Fq2& c0, const Fq2& c3, const Fq2& c4) {
    Fq6 a{f_mul(f.c0.c0, c0), f_mul(f.c0.c1, c0), f_mul(f.c0.c2, c0)};
    Fq6 b = fq6_mul_by_01(f.c1, c3, c4);
    Fq6 e = fq6_mul_by_01(f_add(f.c0, f.c1), f_add(c0, c3), c4);
    return Fq12{f_add(a, fq6_mul_by_v(b)), f_sub(e, f_add(a, b))};
}
// quadratic_extension.rs frobenius_map + mul_base_field_by_frob_coeff, power 1 or 2
CZK_HD Fq12 fq12_frobenius(const Fq12& a, int power) {
    Fq6 c0 = fq6_frobenius(a.c0, power), c1 = fq6_frobenius(a.c1, power);
    const Fq k = power == 1 ? fq_const(PAIRING_FROB12_C1_1) : fq_const(PAIRING_FROB12_C1_2);
    return Fq12{c0, Fq6{fq2_mul_fq(c1.c0, k), fq2_mul_fq(c1.c1, k), fq2_mul_fq(c1.c2, k)}};
}
// fp12_2over3over2.rs:134-216 cyclotomic_square_in_place (Granger-Scott; q^2 = 1 mod 6 for BLS12-377)
CZK_HD Fq12 fq12_cyclotomic_square(const Fq12& a) {
    const Fq2 &r0 = a.c0.c0, &r4 = a.c0.c1, &r3 = a.c0.c2, &r2 = a.c1.c0, &r1 = a.c1.c1, &r5 = a.c1.c2;
    Fq2 tmp = f_mul(r0, r1);
    Fq2 t0 = f_sub(f_sub(f_mul(f_add(r0, r1), f_add(fq2_mul_by_u(r1), r0)), tmp), fq2_mul_by_u(tmp));
    Fq2 t1 = f_dbl(tmp);
    tmp = f_mul(r2, r3);
    Fq2 t2 = f_sub(f_sub(f_mul(f_add(r2, r3), f_add(fq2_mul_by_u(r3), r2)), tmp), fq2_mul_by_u(tmp));
    Fq2 t3 = f_dbl(tmp);
    tmp = f_mul(r4, r5);
    Fq2 t4 = f_sub(f_sub(f_mul(f_add(r4, r5), f_add(fq2_mul_by_u(r5), r4)), tmp), fq2_mul_by_u(tmp));
    Fq2 t5 = f_dbl(tmp);
    Fq12 o;
    o.c0.c0 = f_add(f_dbl(f_sub(t0, r0)), t0);     // z0 = 3 t0 - 2 z0
    o.c1.c1 = f_add(f_dbl(f_add(t1, r1)), t1);     // z1 = 3 t1 + 2 z1
    tmp = fq2_mul_by_u(t5);
    o.c1.c0 = f_add(f_dbl(f_add(r2, tmp)), tmp);   // z2 = 3 (u t5) + 2 z2
    o.c0.c2 = f_add(f_dbl(f_sub(t4, r3)), t4);     // z3 = 3 t4 - 2 z3
    o.c0.c1 = f_add(f_dbl(f_sub(t2, r4)), t2);     // z4 = 3 t2 - 2 z4
    o.c1.c2 = f_add(f_dbl(f_add(r5, t3)), t3);     // z5 = 3 t3 + 2 z5
    return o;
}

// memory <-> registers (72 u64 at p; `stride` u64 between consecutive words: 1 = packed, n = SoA across n threads)
CZK_HD Fq fq_load_strided(const u64* p, size_t stride) {
    Fq r;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        u64 w = p[i * stride];
        r.l[2 * i] = (u32)w;
        r.l[2 * i + 1] = (u32)(w >> 32);
    }
    return r;
}
CZK_HD void fq_store_strided(u64* p, size_t stride, const Fq& a) {
#pragma unroll
    for (int i = 0; i < 6; i++) p[i * stride] = (u64)a.l[2 * i] | ((u64)a.l[2 * i + 1] << 32);
}
CZK_HD Fq2 fq2_load_strided(const u64* p, size_t stride) { return Fq2{fq_load_strided(p, stride), fq_load_strided(p + 6 * stride, stride)}; }
CZK_HD void fq2_store_strided(u64* p, size_t stride, const Fq2& a) {
    fq_store_strided(p, stride, a.c0);
    fq_store_strided(p + 6 * stride, stride, a.c1);
}
CZK_HD Fq6 fq6_load_strided(const u64* p, size_t stride) {
    return Fq6{fq2_load_strided(p, stride), fq2_load_strided(p + 12 * stride, stride), fq2_load_strided(p + 24 * stride, stride)};
}
CZK_HD void fq6_store_strided(u64* p, size_t stride, const Fq6& a) {
    fq2_store_strided(p, stride, a.c0);
    fq2_store_strided(p + 12 * stride, stride, a.c1);
    fq2_store_strided(p + 24 * stride, stride, a.c2);
}
CZK_HD Fq12 fq12_load_strided(const u64* p, size_t stride) { return Fq12{fq6_load_strided(p, stride), fq6_load_strided(p + 36 * stride, stride)}; }
CZK_HD void fq12_store_strided(u64* p, size_t stride, const Fq12& a) {
    fq6_store_strided(p, stride, a.c0);
    fq6_store_strided(p + 36 * stride, stride, a.c1);
}

}  // namespace czk
