"""Big-integer model and operand families for the SATURATED arithmetic of csrc/field.h, tower.h and curve.h (TEST INFRASTRUCTURE ONLY).

tests/test_sat_arith.py runs every function of those headers on the device, one item per thread on raw u32 limbs (czk_lab_arith_probe, ops
from 200 up), in both forms build.py compiles field.h in, and holds each result word for word to this file.  tests/test_sat_arith_cpu.py
proves, on this file alone, that the families contain what they claim.

Nothing here restates the code under test: a field result is the unique residue below p (`a b R^-1 mod p` for the Montgomery product),
a tower result is its definition in tests/pairing_ref.py's schoolbook tower, a curve result is oracle/pyref.py's affine group law.

Values travel as RAW integers: what the limbs in memory spell, i.e. Montgomery form x R mod p for everything but fp_reduce / fp_into_repr
/ fp_from_repr, which are defined on raw values.  An extension element is a nested tuple of raw integers in the reference's nesting.
"""
from __future__ import annotations

import random

import pairing_ref as T
import pyref

M32 = 0xFFFFFFFF


class Field:
    def __init__(self, name, p, n):
        self.name, self.p, self.n = name, p, n
        self.radix = 1 << (32 * n)
        self.one = self.radix % p                      # Montgomery one, R
        self.r2 = self.radix * self.radix % p
        self.rinv = pow(self.radix, -1, p)
        self.pinv = pow(p, -1, self.radix)

    def words(self, v):
        assert 0 <= v < self.radix
        return [(v >> (32 * i)) & M32 for i in range(self.n)]

    # ---- the functions of field.h, on raw values
    def add(self, a, b):
        return (a + b) % self.p

    def sub(self, a, b):
        return (a - b) % self.p

    def dbl(self, a):
        return 2 * a % self.p

    def neg(self, a):
        return -a % self.p

    def reduce(self, a):
        return a - self.p if a >= self.p else a

    def mul(self, a, b):
        return a * b * self.rinv % self.p

    def sqr(self, a):
        return self.mul(a, a)

    def into_repr(self, a):
        return a * self.rinv % self.p

    def from_repr(self, a):
        return a * self.radix % self.p

    def inv(self, a):
        """(x R)^-1 R = R^2 / a; the Fermat power a^(p-2) of zero is zero"""
        return self.r2 * pow(a, -1, self.p) % self.p if a else 0

    # ---- Montgomery reduction, observed: quotient digits and the value before the final subtraction
    def quotient(self, a, b):
        return -a * b * self.pinv % self.radix

    def unreduced(self, a, b):
        t, rem = divmod(a * b + self.quotient(a, b) * self.p, self.radix)
        assert rem == 0 and t < 2 * self.p
        return t


FR = Field("fr", pyref.R_MOD, 8)
FQ = Field("fq", pyref.Q_MOD, 12)
P = FQ.p


def carry_ripple(F, a, b):
    """number of consecutive limbs, from limb 0 up, out of which a + b carries"""
    c, run = 0, 0
    for x, y in zip(F.words(a), F.words(b)):
        c = (x + y + c) >> 32
        if not c:
            break
        run += 1
    return run


def borrow_ripple(F, a, b):
    """number of consecutive limbs, from limb 0 up, out of which a - b borrows"""
    c, run = 0, 0
    for x, y in zip(F.words(a), F.words(b)):
        c = 1 if x - y - c < 0 else 0
        if not c:
            break
        run += 1
    return run


# ------------------------------------------------------------------------------------------------------------- operand families
def singles(F):
    """the edge values below p, as a sorted list without repeats"""
    p, n = F.p, F.n
    out = {0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.one, F.one + 1, F.one - 1, F.r2, largest_limbs(F)}
    for k in range(n):
        out |= {1 << (32 * k), (1 << (32 * k)) - 1 if k else 0, p - (1 << (32 * k))}
        out.add(M32 << (32 * k))                                                      # limb k alone at 0xffffffff
        out.add(((p - 1) >> (32 * (k + 1)) << (32 * (k + 1))) | ((1 << (32 * k)) - 1))   # limb k alone at 0, the rest as large as p allows
    return sorted(v for v in out if 0 <= v < p)


def above_p(F):
    """fp_reduce alone takes these: p <= a < 2^(32 N)"""
    p, top = F.p, F.radix - 1
    out = {p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, top, top - 1, top - p, M32 << (32 * (F.n - 1))}
    out |= {p + (1 << (32 * k)) for k in range(F.n)} | {p + (1 << (32 * k)) - 1 for k in range(F.n)} | {top - (M32 << (32 * k)) for k in range(F.n)}
    return sorted(v for v in out if p <= v <= top)


def randoms(F, rng, count):
    return [rng.randrange(F.p) for _ in range(count)]


def addsub_pairs(F, rng):
    p, n, S = F.p, F.n, singles(F)
    out = []
    for i, a in enumerate(S + randoms(F, rng, 24)):
        out += [(a, t - a) for t in (p - 1, p, p + 1) if 0 <= t - a < p]              # a + b in {p - 1, p, p + 1}
        out += [(a, b) for b in (a, a - 1, a + 1) if 0 <= b < p]                      # a - b in {0, 1, -1}
        out += [(a, S[(5 * i + j) % len(S)]) for j in (1, 2, 3)]
    for k in range(1, n):
        # a carry out of limb 0 that ripples through limbs 1 .. k - 1 (each sums to 0xffffffff) and is absorbed in limb k
        mid = [rng.randrange(1 << 32) for _ in range(k - 1)]
        hi = rng.randrange(p >> (32 * k + 2)) << (32 * k)
        a = hi | sum(x << (32 * (j + 1)) for j, x in enumerate(mid)) | M32
        b = hi | sum((x ^ M32) << (32 * (j + 1)) for j, x in enumerate(mid)) | (1 + rng.randrange(M32))
        out += [(a, b), (b, a)]
        out.append(((1 << (32 * k)) - 1, 1))                                          # the low k limbs all 0xffffffff, plus one
        # a borrow out of limb 0 through k - 1 limbs where a and b agree, absorbed in limb k
        same = sum(x << (32 * (j + 1)) for j, x in enumerate(mid))
        hi_a = (1 + rng.randrange((p >> (32 * k + 1)) - 1)) << (32 * k)
        out += [(hi_a | same, hi_a - (1 << (32 * k)) | same | 1), (1 << (32 * k), 1), (hi_a - (1 << (32 * k)) | same | 1, hi_a | same)]
    out += list(zip(randoms(F, rng, 150), randoms(F, rng, 150)))
    return out


def ones_quotient_pairs(F, rng, count):
    """a b == p (mod 2^(32 N)): every Montgomery quotient digit is 0xffffffff"""
    out = []
    while len(out) < count:
        a = rng.randrange(F.p) | 1
        b = F.p * pow(a, -1, F.radix) % F.radix
        if b < F.p:
            out.append((a, b))
    return out


def zero_quotient_pairs(F, rng, count):
    """a = 2^(16 N) x, b = 2^(16 N) y: the low half of a b is zero, so every quotient digit is zero"""
    h = 16 * F.n
    return [(rng.randrange(1, F.p >> h) << h, rng.randrange(1, F.p >> h) << h) for _ in range(count - 1)] + [((F.p >> h) << h, (F.p >> h) << h)]


def largest_limbs(F):
    """every limb as large as a value below p allows: the column maximum of the 96-bit accumulator"""
    return ((F.p >> (32 * (F.n - 1))) << (32 * (F.n - 1))) - 1


def mul_pairs(F, rng):
    S = singles(F)
    big = largest_limbs(F)
    out = [(a, S[(7 * i + j) % len(S)]) for i, a in enumerate(S) for j in (0, 1, 2, 3)]
    out += [(a, a) for a in S] + [(big, big), (big, F.p - 1), (F.p - 1, F.p - 1)]
    out += zero_quotient_pairs(F, rng, 6) + ones_quotient_pairs(F, rng, 6)
    r = randoms(F, rng, 200)
    out += list(zip(r, randoms(F, rng, 200))) + [(a, a) for a in r[:40]]
    return out


# ------------------------------------------------------------------------------------------------------------- the tower
def to_c(x):
    """raw (Montgomery) -> canonical, through any nesting"""
    return tuple(to_c(v) for v in x) if isinstance(x, tuple) else x * FQ.rinv % P


def to_m(x):
    return tuple(to_m(v) for v in x) if isinstance(x, tuple) else x * FQ.radix % P


def flat(x):
    """nested tuple of raw values -> u32 words, 12 per Fq"""
    if isinstance(x, (tuple, list)):
        return [w for v in x for w in flat(v)]
    return FQ.words(x)


def nest(vals, shape):
    """a flat list of Fq values -> the nesting `shape` (2: Fq2, 6: Fq6, 12: Fq12)"""
    if shape == 2:
        return (vals[0], vals[1])
    if shape == 6:
        return tuple(nest(vals[2 * i:2 * i + 2], 2) for i in range(3))
    return (nest(vals[:6], 6), nest(vals[6:12], 6))


def tower_family(deg, rng, n_random):
    """raw elements of Fq2 / Fq6 / Fq12 (deg = 2, 6, 12): every coefficient from the single-value set, 0 and 1, every subfield, one
    non-zero coefficient at each position, random elements"""
    S = singles(FQ)
    out = [[0] * deg, [FQ.one] + [0] * (deg - 1)]
    out += [[s] * deg for s in S]
    out += [[S[(7 * i + 11 * j) % len(S)] for i in range(deg)] for j in range(len(S))]
    sub = [d for d in (1, 2, 6) if d < deg]
    for d in sub:                                       # Fq, Fq2, Fq6 inside: only the first d coefficients non-zero
        out += [randoms(FQ, rng, d) + [0] * (deg - d) for _ in range(4)] + [[P - 1] * d + [0] * (deg - d)]
    for pos in range(deg):
        for v in (FQ.one, P - 1, rng.randrange(1, P)):
            out.append([v if i == pos else 0 for i in range(deg)])
    out += [randoms(FQ, rng, deg) for _ in range(n_random)]
    return [nest(v, deg) for v in out]


def sparse_operands(k, rng, count):
    """k Fq2 line coefficients (raw) per operand: every subset of them zero, edge values, then random ones"""
    S = singles(FQ)
    out = []
    for mask in range(1 << k):
        for _ in range(3):
            out.append(tuple((0, 0) if mask >> j & 1 else tuple(randoms(FQ, rng, 2)) for j in range(k)))
    out += [tuple((S[(3 * i + j) % len(S)], S[(5 * i + 2 * j + 1) % len(S)]) for j in range(k)) for i in range(len(S))]
    out += [tuple((FQ.one if j == i else 0, 0) for j in range(k)) for i in range(k)]
    out += [tuple(tuple(randoms(FQ, rng, 2)) for _ in range(k)) for _ in range(count)]
    return out


def on_c(f):
    """lifts a function on canonical tower elements to raw ones"""
    return lambda *a: to_m(f(*[to_c(x) for x in a]))


def fq2_sqr(a):
    return T.fq2_mul(a, a)


def fq6_expand_01(c0, c1):
    return (c0, c1, T.FQ2_ZERO)


def fq12_expand_034(c0, c3, c4):
    return ((c0, T.FQ2_ZERO, T.FQ2_ZERO), (c3, c4, T.FQ2_ZERO))


FQ6_V = (T.FQ2_ZERO, T.FQ2_ONE, T.FQ2_ZERO)


def fq6_pow(a, e):
    r = T.FQ6_ONE
    while e:
        if e & 1:
            r = T.fq6_mul(r, a)
        a = T.fq6_mul(a, a)
        e >>= 1
    return r


def cyclotomic_element(g):
    """g^((p^6 - 1)(p^2 + 1)) by the power itself"""
    return T.fq12_pow(g, (P ** 6 - 1) * (P ** 2 + 1))


def cyclotomic_element_fast(g):
    """the same element: g^(p^6) is the conjugate, g^(p^2) the Frobenius map"""
    h = T.fq12_mul(T.fq12_conj(g), T.fq12_inv(g))
    return T.fq12_mul(T.fq12_frob(h, 2), h)


def granger_scott_square(a):
    """fp12_2over3over2.rs cyclotomic_square_in_place as the values it computes: with (z0, z4, z3, z2, z1, z5) = (c0.c0, c0.c1, c0.c2, c1.c0,
    c1.c1, c1.c2) and xi = u, the three Fq4 squares (x + y s)^2 = (x^2 + xi y^2) + (2 x y) s, then z' = 3 t -/+ 2 z.  Equal to the
    square on the cyclotomic subgroup only."""
    (z0, z4, z3), (z2, z1, z5) = a
    add, sub, mul, xi = T.fq2_add, T.fq2_sub, T.fq2_mul, lambda x: T.fq2_mul(T.XI, x)
    k = T.fq2_scale

    def fq4_square(x, y):
        return add(mul(x, x), xi(mul(y, y))), k(mul(x, y), 2)
    t0, t1 = fq4_square(z0, z1)
    t2, t3 = fq4_square(z2, z3)
    t4, t5 = fq4_square(z4, z5)
    return ((sub(k(t0, 3), k(z0, 2)), sub(k(t2, 3), k(z4, 2)), sub(k(t4, 3), k(z3, 2))),
            (add(k(xi(t5), 3), k(z2, 2)), add(k(t1, 3), k(z1, 2)), add(k(t3, 3), k(z5, 2))))


# ------------------------------------------------------------------------------------------------------------- curves
def fq_sqrt(a):
    """Tonelli-Shanks in Fq (p - 1 = 2^46 t); None for a non-residue"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 2, P) != 1:
        return None
    t, s = P - 1, 0
    while t % 2 == 0:
        t, s = t // 2, s + 1
    z = next(z for z in range(2, 100) if pow(z, (P - 1) // 2, P) == P - 1)
    m, c, tt, r = s, pow(z, t, P), pow(a, t, P), pow(a, (t + 1) // 2, P)
    while tt != 1:
        i, x = 0, tt
        while x != 1:
            x, i = x * x % P, i + 1
        b = pow(c, 1 << (m - i - 1), P)
        m, c, tt, r = i, b * b % P, tt * b * b % P, r * b % P
    return r


def fq2_sqrt(a):
    """a square root in Fq2 = Fq[u] / (u^2 + 5) through the norm; None for a non-residue"""
    a0, a1 = a
    if a1 == 0:
        r = fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        r = fq_sqrt(a0 * pow(pyref.FQ2_NONRESIDUE, -1, P) % P)
        return None if r is None else (0, r)
    s = fq_sqrt((a0 * a0 - pyref.FQ2_NONRESIDUE * a1 * a1) % P)
    if s is None:
        return None
    for sg in (s, -s):
        x0 = fq_sqrt((a0 + sg) * pow(2, -1, P) % P)
        if x0:
            r = (x0, a1 * pow(2 * x0, -1, P) % P)
            if T.fq2_mul(r, r) == (a0 % P, a1 % P):
                return r
    return None


class Curve:
    """G1 (deg 1) or G2 (deg 2): canonical affine points of pyref, raw coordinates in memory"""

    def __init__(self, deg):
        self.deg = deg
        self.F = pyref.F1 if deg == 1 else pyref.F2
        self.b = pyref.G1_B if deg == 1 else pyref.G2_B
        self.gen = pyref.G1_GEN if deg == 1 else pyref.G2_GEN
        self.name = "g1" if deg == 1 else "g2"
        self.w = 12 * deg
        self.one = FQ.one if deg == 1 else (FQ.one, 0)
        self.zero = 0 if deg == 1 else (0, 0)

    def lift_x(self, x):
        """a point with this canonical x, or None"""
        F = self.F
        rhs = F.add(F.mul(x, F.mul(x, x)), self.b)
        y = fq_sqrt(rhs) if self.deg == 1 else fq2_sqrt(rhs)
        return None if y is None else (x, y)

    def rand_coord(self, rng, nonzero=False):
        lo = 1 if nonzero else 0
        return rng.randrange(lo, P) if self.deg == 1 else (rng.randrange(lo, P), rng.randrange(P))

    def jac(self, pt, z):
        """raw Jacobian (X, Y, Z) of the canonical affine point under the RAW z (non-zero); the point at infinity keeps z == 0"""
        F = self.F
        if pt is pyref.INF:
            return (self.one, self.one, self.zero)
        zc = to_c(z)
        z2 = F.mul(zc, zc)
        return (to_m(F.mul(pt[0], z2)), to_m(F.mul(pt[1], F.mul(z2, zc))), z)

    def xyzz(self, pt, z):
        F = self.F
        if pt is pyref.INF:
            return (self.one, self.one, self.zero, self.zero)
        zc = to_c(z)
        z2 = F.mul(zc, zc)
        z3 = F.mul(z2, zc)
        return (to_m(F.mul(pt[0], z2)), to_m(F.mul(pt[1], z3)), to_m(z2), to_m(z3))

    def aff(self, pt):
        return (to_m(pt[0]), to_m(pt[1]))

    def is_zero(self, v):
        return v == self.zero

    def from_jac(self, j):
        if self.is_zero(j[2]):
            return pyref.INF
        F = self.F
        x, y, z = to_c(j)
        zi = F.inv(z)
        zi2 = F.mul(zi, zi)
        return (F.mul(x, zi2), F.mul(y, F.mul(zi2, zi)))

    def from_xyzz(self, v):
        if self.is_zero(v[2]):
            return pyref.INF
        F = self.F
        x, y, zz, zzz = to_c(v)
        assert F.mul(zz, F.mul(zz, zz)) == F.mul(zzz, zzz), "not an XYZZ point: ZZ^3 != ZZZ^2"
        return (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))

    def add(self, a, b):
        return pyref.ec_add(self.F, a, b)

    def neg(self, a):
        return pyref.ec_neg(self.F, a)

    def on_curve(self, a):
        return pyref.ec_on_curve(self.F, a, self.b)


G1, G2 = Curve(1), Curve(2)
ORDER_TWO_G1 = (P - 1, 0)          # (-1)^3 + 1 == 0: the point of order two of y^2 = x^3 + 1


def curve_points(C, rng):
    """canonical affine points: subgroup points, points outside the subgroup, points whose RAW x is an edge value, and on G1 the point of
    order two.  Returns (points, names)."""
    pts = [C.gen, pyref.ec_mul(C.F, 2, C.gen), pyref.ec_mul(C.F, rng.randrange(1, pyref.R_MOD), C.gen), pyref.ec_mul(C.F, pyref.R_MOD - 1, C.gen)]
    names = ["gen", "2gen", "k.gen", "-gen"]
    found = 0
    while found < 2:                                    # random x: a point of the curve, outside the prime-order subgroup
        pt = C.lift_x(C.rand_coord(rng))
        if pt is not None and pyref.ec_mul(C.F, pyref.R_MOD, pt) is not pyref.INF:
            pts.append(pt)
            names.append("outside")
            found += 1
    S = singles(FQ)
    found = 0
    for i, s in enumerate(S):                           # raw x (or x.c0, x.c1) from the edge set
        x = to_c(s) if C.deg == 1 else (to_c(s), to_c(S[(3 * i + 1) % len(S)]))
        pt = C.lift_x(x)
        if pt is not None and pt[1] != C.F.zero and found < 12:
            pts.append(pt)
            names.append("edge-x")
            found += 1
    if C.deg == 1:
        pts.append(ORDER_TWO_G1)
        names.append("order2")
    return pts, names


def edge_z(C, rng):
    """raw non-zero Z values: one, edge values, random"""
    S = [s for s in singles(FQ) if s]
    zs = [S[i] for i in range(0, len(S), 5)] + [rng.randrange(1, P) for _ in range(3)]
    if C.deg == 1:
        return [FQ.one] + zs
    return [(FQ.one, 0)] + [(z, S[(7 * i) % len(S)] if i % 2 else 0) for i, z in enumerate(zs)] + [(0, zs[0])]


def curve_pairs(C, rng):
    """(P, Q, tag) canonical pairs: P + Q general, P + P, P + (-P), infinity on either or both sides"""
    pts, names = curve_points(C, rng)
    INF = pyref.INF
    out = [(INF, INF, "inf+inf")]
    for i, (p, nm) in enumerate(zip(pts, names)):
        q = pts[(i + 1) % len(pts)]
        out += [(p, q, nm + "+next"), (p, p, nm + "+same"), (p, C.neg(p), nm + "+neg"), (p, INF, nm + "+inf"), (INF, p, "inf+" + nm)]
    return out


# ------------------------------------------------------------------------------------------------------------- built once
_CACHE = {}


def families():
    """every operand family, from fixed seeds, built once per process"""
    if _CACHE:
        return _CACHE
    for F, seed in ((FR, 0x5A7F), (FQ, 0x5A70)):
        rng = random.Random(seed)
        _CACHE[F.name + ".singles"] = singles(F) + randoms(F, rng, 100)
        _CACHE[F.name + ".reduce"] = singles(F) + above_p(F) + [rng.randrange(F.radix) for _ in range(100)] + randoms(F, rng, 50)
        _CACHE[F.name + ".addsub"] = addsub_pairs(F, rng)
        _CACHE[F.name + ".mul"] = mul_pairs(F, rng)
    rng = random.Random(0x5A72)
    _CACHE["fq2"] = tower_family(2, rng, 200)
    _CACHE["fq6"] = tower_family(6, rng, 200)
    _CACHE["fq12"] = tower_family(12, rng, 200)
    _CACHE["sparse1"] = sparse_operands(1, rng, 40)
    _CACHE["sparse2"] = sparse_operands(2, rng, 40)
    _CACHE["sparse3"] = sparse_operands(3, rng, 40)
    gs = [to_c(g) for g in _CACHE["fq12"][-24:]]
    _CACHE["cyclotomic"] = [to_m(cyclotomic_element_fast(g)) for g in gs]
    for C, seed in ((G1, 0x5A73), (G2, 0x5A74)):
        rng = random.Random(seed)
        _CACHE[C.name + ".pairs"] = curve_pairs(C, rng)
        _CACHE[C.name + ".z"] = edge_z(C, rng)
    return _CACHE


# what tests/test_sat_arith_cpu.py establishes and tests/test_sat_arith.py asserts before it feeds a family to the device
FAMILY_SIZES = {
    "fr.singles": 145,
    "fr.reduce": 225,
    "fr.addsub": 808,
    "fr.mul": 480,
    "fq.singles": 165,
    "fq.reduce": 257,
    "fq.addsub": 1012,
    "fq.mul": 580,
    "fq2": 343,
    "fq6": 360,
    "fq12": 383,
    "sparse1": 112,
    "sparse2": 119,
    "sparse3": 132,
    "cyclotomic": 24,
    "g1.pairs": 96,
    "g1.z": 17,
    "g2.pairs": 91,
    "g2.z": 18,
}
