"""What tests/test_sat_arith.py feeds the device, proven on the model alone (tests/sat_model.py): every family stays inside the contract of
the functions it is fed to and contains the inputs it is there for, and the model's own definitions of the special forms agree."""
import pytest

import pairing_ref as T
import pyref
import sat_model as M
from sat_model import FQ, FR, G1, G2, P


@pytest.fixture(scope="module")
def fam():
    return M.families()


def test_family_sizes(fam):
    assert {k: len(v) for k, v in fam.items()} == M.FAMILY_SIZES
    assert all(2 * n <= 4000 for n in M.FAMILY_SIZES.values())


@pytest.mark.parametrize("F", [FR, FQ], ids=["fr", "fq"])
def test_field_families_stay_below_p_and_hold_the_edges(fam, F):
    p, n = F.p, F.n
    S = fam[F.name + ".singles"]
    assert all(0 <= a < p for a in S) and S[0] == 0
    must = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, F.one, F.one - 1, F.one + 1, F.r2, M.largest_limbs(F)]
    must += [v for k in range(n) for v in (1 << (32 * k), p - (1 << (32 * k)))] + [(1 << (32 * k)) - 1 for k in range(1, n)]
    must += [M.M32 << (32 * k) for k in range(n - 1)]
    assert set(must) <= set(S)
    for k in range(n):                                   # limb k alone at zero, every limb above it as in p - 1, every limb below it full
        assert any(F.words(a)[k] == 0 and F.words(a)[k + 1:] == F.words(p - 1)[k + 1:] and all(w == M.M32 for w in F.words(a)[:k]) for a in S)
    red = fam[F.name + ".reduce"]
    assert all(0 <= a < F.radix for a in red) and {0, p - 1, p, p + 1, 2 * p, F.radix - 1} <= set(red)
    assert sum(a >= p for a in red) > 50 and sum(a < p for a in red) > 50
    pairs = fam[F.name + ".addsub"]
    assert all(0 <= a < p and 0 <= b < p for a, b in pairs)
    assert {p - 1, p, p + 1} <= {a + b for a, b in pairs} and {0, 1, -1} <= {a - b for a, b in pairs}
    assert set(range(1, n)) <= {M.carry_ripple(F, a, b) for a, b in pairs}
    assert set(range(1, n)) <= {M.borrow_ripple(F, a, b) for a, b in pairs}
    # a ripple through limbs that are NOT all equal: the carry travels because each limb sum is 0xffffffff
    assert any(M.carry_ripple(F, a, b) == n - 1 and len(set(F.words(a)[1:n - 1])) > 1 for a, b in pairs)
    assert any(a + b >= p for a, b in pairs) and any(a + b < p for a, b in pairs) and any(a < b for a, b in pairs)


@pytest.mark.parametrize("F", [FR, FQ], ids=["fr", "fq"])
def test_mul_family_reaches_both_branches_and_both_quotient_extremes(fam, F):
    p = F.p
    pairs = fam[F.name + ".mul"]
    assert all(0 <= a < p and 0 <= b < p for a, b in pairs)
    t = [F.unreduced(a, b) for a, b in pairs]
    assert sum(x >= p for x in t) >= 4 and sum(x < p for x in t) >= 4          # the final subtraction taken and not taken
    assert all(F.reduce(x) == F.mul(a, b) for x, (a, b) in zip(t, pairs))
    q = [F.quotient(a, b) for a, b in pairs]
    ones = [(a, b) for (a, b), m in zip(pairs, q) if m == F.radix - 1]
    zeros = [(a, b) for (a, b), m in zip(pairs, q) if m == 0 and a and b]
    assert len(ones) >= 4 and all(a * b % F.radix == p for a, b in ones)
    assert sum(a % (1 << (16 * F.n)) == 0 and b % (1 << (16 * F.n)) == 0 for a, b in zeros) >= 4       # a = 2^(16 N) x, b = 2^(16 N) y
    big = M.largest_limbs(F)
    assert (big, big) in pairs and big < p and F.words(big)[:-1] == [M.M32] * (F.n - 1) and F.words(big)[-1] == F.words(p)[-1] - 1
    assert sum(a == b for a, b in pairs) >= 40
    assert F.inv(0) == 0 and all(F.mul(F.inv(a), a) == F.one for a in fam[F.name + ".singles"] if a)
    assert F.into_repr(F.one) == 1 and F.from_repr(1) == F.one and F.mul(F.one, F.one) == F.one


def test_tower_families(fam):
    for key, deg in (("fq2", 2), ("fq6", 6), ("fq12", 12)):
        A = [M.flat(a) for a in fam[key]]
        vals = [[sum(w << (32 * j) for j, w in enumerate(r[12 * i:12 * i + 12])) for i in range(deg)] for r in A]
        assert all(0 <= v < P for r in vals for v in r)
        assert vals[0] == [0] * deg and vals[1] == [FQ.one] + [0] * (deg - 1)
        S = set(M.singles(FQ))
        assert all(any(r[i] == s for r in vals) for s in S for i in (0, deg - 1))         # every edge value, first and last coefficient
        for pos in range(deg):
            assert any(r[pos] and not any(r[:pos] + r[pos + 1:]) for r in vals)             # one non-zero coefficient, at each position
        for d in (1, 2, 6):
            if d < deg:
                assert any(all(r[:d]) and not any(r[d:]) for r in vals)                     # an element of each subfield
        assert sum(all(r) for r in vals) >= 200
    for k in (1, 2, 3):
        ops = fam[f"sparse{k}"]
        assert all(len(s) == k and all(0 <= v < P for c in s for v in c) for s in ops)
        assert {tuple(c == (0, 0) for c in s) for s in ops} >= {tuple(bool(m >> j & 1) for j in range(k)) for m in range(1 << k)}


def test_special_forms_agree_with_their_definitions_in_the_model(fam):
    rng_elems = [M.to_c(a) for a in fam["fq12"][-4:]]
    a = rng_elems[0]
    # sparse operands expanded: mul_by_01 / mul_by_1 / mul_by_034 / mul_by_v are plain products
    c0, c3, c4 = [M.to_c(c) for c in fam["sparse3"][-1]]
    e = M.fq12_expand_034(c0, c3, c4)
    assert e[0][1] == e[0][2] == e[1][2] == T.FQ2_ZERO and T.fq12_mul(a, e) == T.fq12_mul(e, a)
    assert T.fq6_mul(a[0], M.FQ6_V) == T.fq6_mul_by_v(a[0])
    assert T.fq12_mul(a, T.fq12_inv(a)) == T.FQ12_ONE and T.fq6_mul(a[0], T.fq6_inv(a[0])) == T.FQ6_ONE
    # Frobenius maps are the p-th and p^2-th power
    for x in rng_elems[:2]:
        assert T.fq12_frob(x, 1) == T.fq12_pow(x, P) and T.fq12_frob(x, 2) == T.fq12_pow(x, P * P)
        assert T.fq6_frob(x[0], 1) == M.fq6_pow(x[0], P) and T.fq6_frob(x[1], 2) == M.fq6_pow(x[1], P * P)
    # the cyclotomic subgroup, by the power itself, and Granger-Scott's square on it and off it
    g = rng_elems[1]
    h = M.cyclotomic_element(g)
    assert h == M.cyclotomic_element_fast(g) and h != T.FQ12_ONE
    assert T.fq12_mul(T.fq12_frob(T.fq12_frob(h, 2), 2), h) == T.fq12_frob(h, 2)          # h^(p^4 - p^2 + 1) == 1
    assert M.granger_scott_square(h) == T.fq12_sqr(h)
    assert M.granger_scott_square(g) != T.fq12_sqr(g)
    cyc = [M.to_c(x) for x in fam["cyclotomic"]]
    assert len(set(cyc)) == len(cyc) and all(M.granger_scott_square(x) == T.fq12_sqr(x) for x in cyc)
    assert all(T.fq12_mul(x, T.fq12_conj(x)) == T.FQ12_ONE for x in cyc)                     # unitary: the inverse is the conjugate


@pytest.mark.parametrize("C", [G1, G2], ids=["g1", "g2"])
def test_curve_families(fam, C):
    pairs = fam[C.name + ".pairs"]
    INF = pyref.INF
    assert all(C.on_curve(p) and C.on_curve(q) for p, q, _ in pairs)
    tags = [t for *_, t in pairs]
    assert "inf+inf" in tags and any(t.endswith("+same") for t in tags) and any(t.endswith("+neg") for t in tags)
    assert any(p is INF and q is not INF for p, q, _ in pairs) and any(q is INF and p is not INF for p, q, _ in pairs)
    outside = [p for p, _, t in pairs if t.startswith("outside")]
    assert outside and all(pyref.ec_mul(C.F, pyref.R_MOD, p) is not INF for p in outside)
    assert all(pyref.ec_mul(C.F, pyref.R_MOD, p) is INF for p, _, t in pairs if t.startswith(("gen", "k.gen")))
    S = set(M.singles(FQ))
    edge = [p for p, _, t in pairs if t.startswith("edge-x")]
    assert len(edge) >= 5 and all((M.to_m(p[0]) if C.deg == 1 else M.to_m(p[0])[0]) in S for p in edge)
    zs = fam[C.name + ".z"]
    assert len(set(zs)) == len(zs) and all(not C.is_zero(z) for z in zs) and zs[0] == C.one
    # Jacobian and XYZZ lifts are the same point under every Z
    p = pairs[1][0]
    assert all(C.from_jac(C.jac(p, z)) == p and C.from_xyzz(C.xyzz(p, z)) == p for z in zs)
    assert C.from_jac(C.jac(INF, zs[1])) is INF and C.from_xyzz(C.xyzz(INF, zs[1])) is INF


def test_the_point_of_order_two_is_on_g1(fam):
    t = M.ORDER_TWO_G1
    assert t == (P - 1, 0) and G1.on_curve(t) and G1.add(t, t) is pyref.INF and G1.neg(t) == t
    assert any(p == t and q == t for p, q, _ in fam["g1.pairs"])
