"""Plain big-integer restatement of the BLS12-377 pairing (TEST INFRASTRUCTURE ONLY).

Restates, with Python integers and oracle/pyref.py's Fq / Fq2 helpers, the reference's `Bls12::<Parameters>` engine
(paths relative to the reference root):
  * tower Fq6 = Fq2[v]/(v^3 - u), Fq12 = Fq6[w]/(w^2 - v) ... curves/bls12_377/src/fields/{fq6.rs:12-14, fq12.rs:12}
  * Frobenius coefficients ........................... derived here from q (frobenius_coefficients()); compared against the
                                                        reference's text through tests/golden/pairing_constants.json
  * G2Prepared::from, doubling_step, addition_step ... algebra/ec/src/models/bls12/g2.rs:69-157 (TwistType::D)
  * ell, miller_loop, final_exponentiation ........... algebra/ec/src/models/bls12/mod.rs:54-193
  * verify_proof ..................................... groth16/src/verifier.rs:23-58

Products and squares are stated as the schoolbook tower formulas, not the reference's Karatsuba / sparse / cyclotomic forms:
every one of those is the same field element, so this shares no formula with csrc/tower.h beyond the tower itself.
Elements are canonical integers (not Montgomery): Fq2 = (c0, c1), Fq6 = (c0, c1, c2) of Fq2, Fq12 = (c0, c1) of Fq6.
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pyref  # noqa: E402
from pyref import F1, F2, G1_GEN, G2_B, G2_GEN, INF, Q_MOD, R_MOD, ec_add, ec_mul, ec_neg, fq2_add, fq2_inv, fq2_mul, fq2_sub  # noqa: E402,F401

Q = Q_MOD
X = 0x8508C00000000001          # curves/bls12_377/src/curves/mod.rs:16 (X_IS_NEGATIVE = false, TwistType::D)
X_BITS = [(X >> i) & 1 for i in range(X.bit_length() - 2, -1, -1)]   # BitIteratorBE::new(X).skip(1)

FQ2_ZERO, FQ2_ONE = (0, 0), (1, 0)
FQ6_ZERO, FQ6_ONE = (FQ2_ZERO, FQ2_ZERO, FQ2_ZERO), (FQ2_ONE, FQ2_ZERO, FQ2_ZERO)
FQ12_ONE = (FQ6_ONE, FQ6_ZERO)
XI = (0, 1)                     # Fq6 NONRESIDUE = u (fq6.rs:14); Fq12 NONRESIDUE = v (fq12.rs:12)


# ----------------------------------------------------------------------------- Fq2 / Fq6 / Fq12
def fq2_neg(a):
    return ((-a[0]) % Q, (-a[1]) % Q)


def fq2_scale(a, k):
    return (a[0] * k % Q, a[1] * k % Q)


def fq2_pow(a, e):
    r = FQ2_ONE
    while e:
        if e & 1:
            r = fq2_mul(r, a)
        a = fq2_mul(a, a)
        e >>= 1
    return r


def fq2_conj(a):
    return (a[0], (-a[1]) % Q)


def fq6_add(a, b):
    return tuple(fq2_add(x, y) for x, y in zip(a, b))


def fq6_sub(a, b):
    return tuple(fq2_sub(x, y) for x, y in zip(a, b))


def fq6_neg(a):
    return tuple(fq2_neg(x) for x in a)


def fq6_mul(a, b):
    t = [FQ2_ZERO] * 5
    for i in range(3):
        for j in range(3):
            t[i + j] = fq2_add(t[i + j], fq2_mul(a[i], b[j]))
    return (fq2_add(t[0], fq2_mul(XI, t[3])), fq2_add(t[1], fq2_mul(XI, t[4])), t[2])


def fq6_mul_by_v(a):
    return (fq2_mul(XI, a[2]), a[0], a[1])


def fq6_inv(a):
    # a^-1 = conj-product / norm: solve with the adjugate of the multiplication-by-a matrix over Fq2
    a0, a1, a2 = a
    t0 = fq2_sub(fq2_mul(a0, a0), fq2_mul(XI, fq2_mul(a1, a2)))
    t1 = fq2_sub(fq2_mul(XI, fq2_mul(a2, a2)), fq2_mul(a0, a1))
    t2 = fq2_sub(fq2_mul(a1, a1), fq2_mul(a0, a2))
    n = fq2_add(fq2_mul(a0, t0), fq2_mul(XI, fq2_add(fq2_mul(a2, t1), fq2_mul(a1, t2))))
    ni = fq2_inv(n)
    return (fq2_mul(t0, ni), fq2_mul(t1, ni), fq2_mul(t2, ni))


def fq12_mul(a, b):
    return (fq6_add(fq6_mul(a[0], b[0]), fq6_mul_by_v(fq6_mul(a[1], b[1]))),
            fq6_add(fq6_mul(a[0], b[1]), fq6_mul(a[1], b[0])))


def fq12_sqr(a):
    return fq12_mul(a, a)


def fq12_conj(a):
    return (a[0], fq6_neg(a[1]))


def fq12_inv(a):
    # (a0 + a1 w)^-1 = (a0 - a1 w) / (a0^2 - v a1^2)
    n = fq6_sub(fq6_mul(a[0], a[0]), fq6_mul_by_v(fq6_mul(a[1], a[1])))
    ni = fq6_inv(n)
    return (fq6_mul(a[0], ni), fq6_neg(fq6_mul(a[1], ni)))


def fq12_pow(a, e):
    r = FQ12_ONE
    while e:
        if e & 1:
            r = fq12_mul(r, a)
        a = fq12_sqr(a)
        e >>= 1
    return r


def frobenius_coefficients():
    """FROBENIUS_COEFF_FP6_C1[i] = u^((q^i - 1) / 3), _C2[i] = u^((2 q^i - 2) / 3) (i < 6), FROBENIUS_COEFF_FP12_C1[i] = u^((q^i - 1) / 6)
    (i < 12): the values the comments of fq6.rs:17-69 and fq12.rs:15-73 state, derived from q alone.  Every one lies in Fq (c1 == 0)."""
    c6_1 = [fq2_pow(XI, (Q ** i - 1) // 3) for i in range(6)]
    c6_2 = [fq2_pow(XI, (2 * Q ** i - 2) // 3) for i in range(6)]
    c12_1 = [fq2_pow(XI, (Q ** i - 1) // 6) for i in range(12)]
    return {"FROBENIUS_COEFF_FP6_C1": c6_1, "FROBENIUS_COEFF_FP6_C2": c6_2, "FROBENIUS_COEFF_FP12_C1": c12_1}


_FROB = frobenius_coefficients()


def fq6_frob(a, p):
    return (fq2_conj(a[0]) if p & 1 else a[0],
            fq2_mul(fq2_conj(a[1]) if p & 1 else a[1], _FROB["FROBENIUS_COEFF_FP6_C1"][p % 6]),
            fq2_mul(fq2_conj(a[2]) if p & 1 else a[2], _FROB["FROBENIUS_COEFF_FP6_C2"][p % 6]))


def fq12_frob(a, p):
    c = _FROB["FROBENIUS_COEFF_FP12_C1"][p % 12]
    return (fq6_frob(a[0], p), tuple(fq2_mul(x, c) for x in fq6_frob(a[1], p)))


# ----------------------------------------------------------------------------- G2Prepared (g2.rs:69-157)
TWO_INV = pow(2, -1, Q)


def doubling_step(r):
    x, y, z = r
    a = fq2_scale(fq2_mul(x, y), TWO_INV)
    b = fq2_mul(y, y)
    c = fq2_mul(z, z)
    e = fq2_mul(G2_B, fq2_scale(c, 3))
    f = fq2_scale(e, 3)
    g = fq2_scale(fq2_add(b, f), TWO_INV)
    h = fq2_sub(fq2_mul(fq2_add(y, z), fq2_add(y, z)), fq2_add(b, c))
    i = fq2_sub(e, b)
    j = fq2_mul(x, x)
    e2 = fq2_mul(e, e)
    nr = (fq2_mul(a, fq2_sub(b, f)), fq2_sub(fq2_mul(g, g), fq2_scale(e2, 3)), fq2_mul(b, h))
    return nr, (fq2_neg(h), fq2_scale(j, 3), i)           # TwistType::D


def addition_step(r, q):
    x, y, z = r
    theta = fq2_sub(y, fq2_mul(q[1], z))
    lam = fq2_sub(x, fq2_mul(q[0], z))
    c = fq2_mul(theta, theta)
    d = fq2_mul(lam, lam)
    e = fq2_mul(lam, d)
    f = fq2_mul(z, c)
    g = fq2_mul(x, d)
    h = fq2_sub(fq2_add(e, f), fq2_scale(g, 2))
    nr = (fq2_mul(lam, h), fq2_sub(fq2_mul(theta, fq2_sub(g, h)), fq2_mul(e, y)), fq2_mul(z, e))
    j = fq2_sub(fq2_mul(theta, q[0]), fq2_mul(lam, q[1]))
    return nr, (lam, fq2_neg(theta), j)                   # TwistType::D


def g2_prepare(q):
    """G2Prepared::from: [] for infinity, else 69 (c0, c1, c2) triples."""
    if q is INF:
        return []
    coeffs, r = [], (q[0], q[1], FQ2_ONE)
    for bit in X_BITS:
        r, c = doubling_step(r)
        coeffs.append(c)
        if bit:
            r, c = addition_step(r, q)
            coeffs.append(c)
    return coeffs


# ----------------------------------------------------------------------------- Miller loop / final exponentiation (mod.rs:54-193)
def ell(f, coeffs, p):
    c0 = fq2_scale(coeffs[0], p[1])
    c1 = fq2_scale(coeffs[1], p[0])
    # mul_by_034(c0, c3 = c1, c4 = c2): f * ((c0, 0, 0) + (c3, c4, 0) w)
    return fq12_mul(f, ((c0, FQ2_ZERO, FQ2_ZERO), (c1, coeffs[2], FQ2_ZERO)))


def miller_loop(pairs):
    """pairs: [(G1 affine or INF, G2 affine or INF)]; pairs with infinity on either side are skipped."""
    prepared = [(p, g2_prepare(q)) for p, q in pairs if p is not INF and q is not INF]
    f, idx = FQ12_ONE, 0
    for bit in X_BITS:
        f = fq12_sqr(f)
        for p, c in prepared:
            f = ell(f, c[idx], p)
        idx += 1
        if bit:
            for p, c in prepared:
                f = ell(f, c[idx], p)
            idx += 1
    return f


def exp_by_x(f):
    return fq12_pow(f, X)


def final_exponentiation(f):
    f1 = fq12_conj(f)
    f2 = fq12_inv(f)
    r = fq12_mul(f1, f2)
    f2 = r
    r = fq12_frob(r, 2)
    r = fq12_mul(r, f2)
    y0 = fq12_sqr(r)
    y1 = exp_by_x(r)
    y2 = fq12_conj(r)
    y1 = fq12_mul(y1, y2)
    y2 = exp_by_x(y1)
    y1 = fq12_conj(y1)
    y1 = fq12_mul(y1, y2)
    y2 = exp_by_x(y1)
    y1 = fq12_frob(y1, 1)
    y1 = fq12_mul(y1, y2)
    r = fq12_mul(r, y0)
    y0 = exp_by_x(y1)
    y2 = exp_by_x(y0)
    y0 = fq12_frob(y1, 2)
    y1 = fq12_conj(y1)
    y1 = fq12_mul(y1, y2)
    y1 = fq12_mul(y1, y0)
    r = fq12_mul(r, y1)
    return r


def pairing(p, q):
    return final_exponentiation(miller_loop([(p, q)]))


def product_of_pairings(pairs):
    return final_exponentiation(miller_loop(pairs))


def g1_add(p, q):
    return ec_add(F1, p, q)


def g1_mul(k, p=G1_GEN):
    return ec_mul(F1, k % R_MOD, p)


def g2_mul(k, q=G2_GEN):
    return ec_mul(F2, k % R_MOD, q)


def verify_proof(alpha_beta, gamma_g2, delta_g2, gamma_abc, a, b, c, public_inputs):
    """verifier.rs:23-58 (prepare_verifying_key's e(alpha, beta) passed in): e(A, B) e(g_ic, -gamma) e(C, -delta) == e(alpha, beta)."""
    if len(public_inputs) + 1 != len(gamma_abc):
        raise ValueError("MalformedVerifyingKey")
    g_ic = gamma_abc[0]
    for x, base in zip(public_inputs, gamma_abc[1:]):
        g_ic = g1_add(g_ic, g1_mul(x, base))
    qap = product_of_pairings([(a, b), (g_ic, ec_neg(F2, gamma_g2)), (c, ec_neg(F2, delta_g2))])
    return qap == alpha_beta


# ----------------------------------------------------------------------------- limb I/O (czk.h layouts, Montgomery)
def fq12_to_limbs(f):
    """72 u64: c0.c0.c0, c0.c0.c1, c0.c1.c0, ... c1.c2.c1, each Fq as 6 Montgomery limbs."""
    out = []
    for c6 in f:
        for c2 in c6:
            for x in c2:
                out += pyref.int_to_limbs(pyref.fq_to_mont(x), 6)
    return out


def fq12_from_limbs(limbs):
    v = [pyref.fq_from_mont(pyref.limbs_to_int(limbs[6 * i:6 * i + 6])) for i in range(12)]
    f2 = [(v[2 * i], v[2 * i + 1]) for i in range(6)]
    return ((f2[0], f2[1], f2[2]), (f2[3], f2[4], f2[5]))


def g1_to_limbs(p):
    if p is INF:
        return [0] * 6 + pyref.int_to_limbs(pyref.FQ_MONT_R, 6), 1
    return pyref.int_to_limbs(pyref.fq_to_mont(p[0]), 6) + pyref.int_to_limbs(pyref.fq_to_mont(p[1]), 6), 0


def g2_to_limbs(q):
    if q is INF:
        return [0] * 12 + pyref.int_to_limbs(pyref.FQ_MONT_R, 6) + [0] * 6, 1
    return [w for x in (q[0][0], q[0][1], q[1][0], q[1][1]) for w in pyref.int_to_limbs(pyref.fq_to_mont(x), 6)], 0


def g1_from_limbs(limbs, inf):
    if inf:
        return INF
    return (pyref.fq_from_mont(pyref.limbs_to_int(limbs[:6])), pyref.fq_from_mont(pyref.limbs_to_int(limbs[6:12])))


def g2_from_limbs(limbs, inf):
    if inf:
        return INF
    v = [pyref.fq_from_mont(pyref.limbs_to_int(limbs[6 * i:6 * i + 6])) for i in range(4)]
    return ((v[0], v[1]), (v[2], v[3]))
