"""The saturated Fr / Fq / Fq2 arithmetic of csrc/field.h, the Fq6 / Fq12 tower of tower.h and the group law of curve.h ON THE DEVICE, at
their edges, against tests/sat_model.py.

On the device field.h's add / sub / double / reduce and every column of the Montgomery multiply are inline-assembly carry chains that the
host never executes, so a check compiled for the host proves nothing about them.  czk_lab_arith_probe (ops from 200 up, lab library only)
runs one function per item on raw limbs, in both forms build.py compiles field.h in: `name` with the multiply inlined (the hot kernels'
form), `name@noinline` with -DCZK_NOINLINE_MUL (the form of pairing.hip, point_codec.hip, msm.hip, lanes.hip, net.hip, net_rounds.hip; the only form the
tower has).  Field and tower results are compared word for word with the model; curve results as group elements with oracle/pyref.py's
affine law and, where a host entry point runs the same header (czk_jac_add, czk_jac_add_mixed, czk_jac_to_affine, czk_jac_scalar_mul by
2), bit for bit with the portable host path.  Every family is fed whole; its size is the one tests/test_sat_arith_cpu.py established.
"""
import numpy as np
import pytest

import czk_amd
import pairing_ref as T
import pyref
import sat_model as M
from sat_model import FQ, FR, G1, G2

pytestmark = pytest.mark.gpu
BOTH = ("", "@noinline")
TOWER = ("@noinline",)


@pytest.fixture(scope="module")
def ctx():
    c = czk_amd.Context(0, lab=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fam():
    f = M.families()
    assert {k: len(v) for k, v in f.items()} == M.FAMILY_SIZES
    return f


def run(ctx, op, rows):
    return ctx.lab_arith_probe(op, np.array(rows, dtype=np.uint32)).tolist()


def check_exact(ctx, name, rows, want, forms=BOTH):
    """rows / want: one list of u32 words per item; every item is compared, in every form"""
    assert len(rows) == len(want) and rows
    for form in forms:
        got = run(ctx, name + form, rows)
        bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, f"{name + form}: {len(bad)} of {len(rows)} items differ, first {bad[0]}: in {rows[bad[0]]} got {got[bad[0]]} want {want[bad[0]]}"


def fl(*xs):
    return [w for x in xs for w in M.flat(x)]


# ------------------------------------------------------------------------------------------------------------- Fr, Fq
@pytest.mark.parametrize("F", [FR, FQ], ids=["fr", "fq"])
def test_fp_add_sub_dbl_neg_reduce_at_the_edges(ctx, fam, F):
    pairs, ones, red = fam[F.name + ".addsub"], fam[F.name + ".singles"], fam[F.name + ".reduce"]
    rows = [F.words(a) + F.words(b) for a, b in pairs]
    check_exact(ctx, F.name + "_add", rows, [F.words(F.add(a, b)) for a, b in pairs])
    check_exact(ctx, F.name + "_sub", rows, [F.words(F.sub(a, b)) for a, b in pairs])
    rows = [F.words(a) for a in ones]
    check_exact(ctx, F.name + "_dbl", rows, [F.words(F.dbl(a)) for a in ones])
    check_exact(ctx, F.name + "_neg", rows, [F.words(F.neg(a)) for a in ones])
    check_exact(ctx, F.name + "_reduce", [F.words(a) for a in red], [F.words(F.reduce(a)) for a in red])


@pytest.mark.parametrize("F", [FR, FQ], ids=["fr", "fq"])
def test_fp_mul_family_at_the_edges(ctx, fam, F):
    pairs, ones = fam[F.name + ".mul"], fam[F.name + ".singles"]
    check_exact(ctx, F.name + "_mul", [F.words(a) + F.words(b) for a, b in pairs], [F.words(F.mul(a, b)) for a, b in pairs])
    rows = [F.words(a) for a in ones]
    check_exact(ctx, F.name + "_sqr", rows, [F.words(F.sqr(a)) for a in ones])
    check_exact(ctx, F.name + "_into_repr", rows, [F.words(F.into_repr(a)) for a in ones])
    check_exact(ctx, F.name + "_from_repr", rows, [F.words(F.from_repr(a)) for a in ones])
    assert ones[0] == 0 and F.inv(0) == 0                  # the Fermat inverse of zero is zero
    check_exact(ctx, F.name + "_inv", rows, [F.words(F.inv(a)) for a in ones])
    if F is FQ:
        check_exact(ctx, "fq_mul_by_nonresidue", rows, [F.words(-5 * a % F.p) for a in ones])


# ------------------------------------------------------------------------------------------------------------- Fq2
def test_fq2_at_the_edges(ctx, fam):
    A = fam["fq2"]
    B = [A[(5 * i + 3) % len(A)] for i in range(len(A))]
    ks = fam["fq.singles"]
    pairs = list(zip(A, B)) + [(a, a) for a in A[:60]]
    rows2 = [fl(a, b) for a, b in pairs]
    rows1 = [fl(a) for a in A]
    c = M.on_c
    check_exact(ctx, "fq2_add", rows2, [fl(c(T.fq2_add)(a, b)) for a, b in pairs])
    check_exact(ctx, "fq2_sub", rows2, [fl(c(T.fq2_sub)(a, b)) for a, b in pairs])
    check_exact(ctx, "fq2_mul", rows2, [fl(c(T.fq2_mul)(a, b)) for a, b in pairs])
    check_exact(ctx, "fq2_dbl", rows1, [fl(c(lambda a: T.fq2_add(a, a))(a)) for a in A])
    check_exact(ctx, "fq2_neg", rows1, [fl(c(T.fq2_neg)(a)) for a in A])
    check_exact(ctx, "fq2_sqr", rows1, [fl(c(M.fq2_sqr)(a)) for a in A])
    check_exact(ctx, "fq2_conj", rows1, [fl(c(T.fq2_conj)(a)) for a in A])
    check_exact(ctx, "fq2_mul_by_u", rows1, [fl(c(lambda a: T.fq2_mul(T.XI, a))(a)) for a in A])
    assert A[0] == (0, 0)                                   # f_inv(0) == 0
    check_exact(ctx, "fq2_inv", rows1, [fl(c(T.fq2_inv)(a) if a != (0, 0) else (0, 0)) for a in A])
    rows = [fl(a, ks[(3 * i) % len(ks)]) for i, a in enumerate(A)]
    check_exact(ctx, "fq2_mul_fq", rows, [fl(c(lambda a, k: T.fq2_scale(a, k))(a, ks[(3 * i) % len(ks)])) for i, a in enumerate(A)])


# ------------------------------------------------------------------------------------------------------------- Fq6, Fq12
def test_fq6_at_the_edges(ctx, fam):
    A = fam["fq6"]
    B = [A[(5 * i + 3) % len(A)] for i in range(len(A))]
    pairs = list(zip(A, B)) + [(a, a) for a in A[:40]]
    rows2, rows1 = [fl(a, b) for a, b in pairs], [fl(a) for a in A]
    c = M.on_c
    check_exact(ctx, "fq6_add", rows2, [fl(c(T.fq6_add)(a, b)) for a, b in pairs], TOWER)
    check_exact(ctx, "fq6_sub", rows2, [fl(c(T.fq6_sub)(a, b)) for a, b in pairs], TOWER)
    check_exact(ctx, "fq6_mul", rows2, [fl(c(T.fq6_mul)(a, b)) for a, b in pairs], TOWER)
    check_exact(ctx, "fq6_neg", rows1, [fl(c(T.fq6_neg)(a)) for a in A], TOWER)
    check_exact(ctx, "fq6_mul_by_v", rows1, [fl(c(lambda a: T.fq6_mul(a, M.FQ6_V))(a)) for a in A], TOWER)
    assert A[0] == M.nest([0] * 6, 6)                       # f_inv(0) == 0
    check_exact(ctx, "fq6_inv", rows1, [fl(c(T.fq6_inv)(a) if a != A[0] else a) for a in A], TOWER)
    # the sparse products equal the full product with the sparse operand expanded
    s2, s1 = fam["sparse2"], fam["sparse1"]
    items = [(A[(7 * i) % len(A)], s) for i, s in enumerate(s2)] + [(a, s2[i % len(s2)]) for i, a in enumerate(A)]
    check_exact(ctx, "fq6_mul_by_01", [fl(a, s) for a, s in items], [fl(c(lambda a, s: T.fq6_mul(a, M.fq6_expand_01(*s)))(a, s)) for a, s in items], TOWER)
    items = [(A[(7 * i) % len(A)], s) for i, s in enumerate(s1)] + [(a, s1[i % len(s1)]) for i, a in enumerate(A)]
    check_exact(ctx, "fq6_mul_by_1", [fl(a, s) for a, s in items],
                [fl(c(lambda a, s: T.fq6_mul(a, (T.FQ2_ZERO, s[0], T.FQ2_ZERO)))(a, s)) for a, s in items], TOWER)
    # Frobenius: a handful through the power itself, the rest against pairing_ref.fq6_frob
    few = [M.to_c(a) for a in A[-3:]]
    for power in (1, 2):
        assert [T.fq6_frob(a, power) for a in few] == [M.fq6_pow(a, M.P ** power) for a in few]
        check_exact(ctx, f"fq6_frobenius_{power}", rows1, [fl(c(lambda a: T.fq6_frob(a, power))(a)) for a in A], TOWER)


def test_fq12_at_the_edges(ctx, fam):
    A = fam["fq12"]
    B = [A[(5 * i + 3) % len(A)] for i in range(len(A))]
    pairs = list(zip(A, B)) + [(a, a) for a in A[:40]]
    rows1 = [fl(a) for a in A]
    c = M.on_c
    check_exact(ctx, "fq12_mul", [fl(a, b) for a, b in pairs], [fl(c(T.fq12_mul)(a, b)) for a, b in pairs], TOWER)
    check_exact(ctx, "fq12_sqr", rows1, [fl(c(T.fq12_sqr)(a)) for a in A], TOWER)
    check_exact(ctx, "fq12_conj", rows1, [fl(c(T.fq12_conj)(a)) for a in A], TOWER)
    assert A[0] == M.nest([0] * 12, 12)                     # f_inv(0) == 0
    check_exact(ctx, "fq12_inv", rows1, [fl(c(T.fq12_inv)(a) if a != A[0] else a) for a in A], TOWER)
    s3 = fam["sparse3"]
    items = [(A[(7 * i) % len(A)], s) for i, s in enumerate(s3)] + [(a, s3[i % len(s3)]) for i, a in enumerate(A)]
    check_exact(ctx, "fq12_mul_by_034", [fl(a, s) for a, s in items],
                [fl(c(lambda a, s: T.fq12_mul(a, M.fq12_expand_034(*s)))(a, s)) for a, s in items], TOWER)


def test_fq12_frobenius_and_cyclotomic_square(ctx, fam):
    A, cyc = fam["fq12"], fam["cyclotomic"]
    rows1 = [fl(a) for a in A]
    c = M.on_c
    few = [M.to_c(a) for a in A[-3:]]
    for power in (1, 2):
        assert [T.fq12_frob(a, power) for a in few] == [T.fq12_pow(a, M.P ** power) for a in few]
        check_exact(ctx, f"fq12_frobenius_{power}", rows1, [fl(c(lambda a: T.fq12_frob(a, power))(a)) for a in A], TOWER)
    # on the cyclotomic subgroup the special square IS the square; elsewhere it is the reference's Granger-Scott formula
    want = [c(T.fq12_sqr)(a) for a in cyc]
    assert want == [c(M.granger_scott_square)(a) for a in cyc]
    check_exact(ctx, "fq12_cyclotomic_square", [fl(a) for a in cyc], [fl(w) for w in want], TOWER)
    check_exact(ctx, "fq12_cyclotomic_square", rows1, [fl(c(M.granger_scott_square)(a)) for a in A], TOWER)


@pytest.mark.parametrize("n", [1, 64, 381])
def test_fq12_strided_loads_and_stores(ctx, fam, n):
    """n items as one batch, packed (stride 1) and SoA (u64 word w of item t at [w n + t], the layout of the final exponentiation's
    workspace): fq12_load_strided into registers and out through plain stores, plain loads and out through fq12_store_strided"""
    A = fam["fq12"]
    assert n <= len(A)
    packed = np.array([fl(a) for a in A[:n]], dtype=np.uint32)
    soa = np.ascontiguousarray(packed.view(np.uint64).T).view(np.uint32).reshape(n, 144)     # the same bytes, word-major
    for got, want in ((run(ctx, "fq12_load_strided_1@noinline", packed), packed), (run(ctx, "fq12_store_strided_1@noinline", packed), packed),
                      (run(ctx, "fq12_load_strided_n@noinline", soa), packed), (run(ctx, "fq12_store_strided_n@noinline", packed), soa)):
        assert np.array_equal(np.array(got, dtype=np.uint32), want)


# ------------------------------------------------------------------------------------------------------------- curve.h
def unflat(C, words, k):
    """k coordinates of C's base field from u32 words (raw values)"""
    v = [sum(int(w) << (32 * j) for j, w in enumerate(words[12 * i:12 * i + 12])) for i in range(k * C.deg)]
    return tuple(v) if C.deg == 1 else tuple((v[2 * i], v[2 * i + 1]) for i in range(k))


def u64s(words):
    return np.array(words, dtype=np.uint32).view(np.uint64)


def curve_cases(C, fam):
    """(P, Q, zp, zq, tag): every pair under rotating Z, and P + P / P + (-P) under two different Z as well"""
    zs = fam[C.name + ".z"]
    out = []
    for i, (p, q, tag) in enumerate(fam[C.name + ".pairs"]):
        out.append((p, q, zs[i % len(zs)], zs[(3 * i + 1) % len(zs)], tag))
        out.append((p, q, zs[0], zs[0], tag))
        if tag.endswith(("+same", "+neg")):
            out.append((p, q, zs[(i + 2) % len(zs)], zs[(i + 5) % len(zs)], tag))
    return out


def run_forms(ctx, name, rows):
    return [(form, run(ctx, name + form, rows)) for form in BOTH]


@pytest.mark.parametrize("C", [G1, G2], ids=["g1", "g2"])
def test_jacobian_formulas_on_the_device(ctx, fam, C):
    g, cases = C.deg, curve_cases(C, fam)
    assert any(t.startswith("order2") for *_, t in cases) == (C is G1) and any(t.startswith("outside") for *_, t in cases)
    INF = pyref.INF
    jp = [C.jac(p, zp) for p, _, zp, _, _ in cases]
    jp += [(x, y, C.zero) for x, y, _ in jp[1:6]]                   # infinity with arbitrary X, Y: only Z == 0 says so
    pts = [p for p, *_ in cases] + [INF] * 5
    rows = [fl(j) for j in jp]
    two = np.array([2, 0, 0, 0], dtype=np.uint64)
    host = [list(ctx.jac_scalar_mul(g, u64s(r), two).view(np.uint32)) for r in rows]
    for form, got in run_forms(ctx, C.name + "_jac_double", rows):
        for i, (o, p) in enumerate(zip(got, pts)):
            assert C.from_jac(unflat(C, o, 3)) == C.add(p, p), (form, i)
            assert o == host[i], (form, i, "device and host jac_double differ")
    aff, inf = ctx.jac_to_affine(g, np.array([u64s(r) for r in rows]))
    for form, got in run_forms(ctx, C.name + "_jac_to_affine", rows):
        for i, (o, p) in enumerate(zip(got, pts)):
            assert o[-1] == (p is INF) == inf[i], (form, i)
            assert o[-1] or M.to_c(unflat(C, o, 2)) == p, (form, i)
            assert o[:-1] == list(aff[i].view(np.uint32)), (form, i, "device and host jac_to_affine differ")
    # p + q, both Jacobian
    rows = [fl(C.jac(p, zp), C.jac(q, zq)) for p, q, zp, zq, _ in cases]
    host = [list(ctx.jac_add(g, u64s(r[:3 * C.w]), u64s(r[3 * C.w:])).view(np.uint32)) for r in rows]
    for form, got in run_forms(ctx, C.name + "_jac_add", rows):
        for i, (o, (p, q, *_, tag)) in enumerate(zip(got, cases)):
            assert C.from_jac(unflat(C, o, 3)) == C.add(p, q), (form, i, tag)
            assert o == host[i], (form, i, tag, "device and host jac_add differ")
    # p + q, q affine with its infinity flag
    rows = [fl(C.jac(p, zp), C.aff(q) if q is not INF else (C.zero, C.one)) + [int(q is INF)] for p, q, zp, _, _ in cases]
    host = [list(ctx.jac_add_mixed(g, u64s(r[:3 * C.w]), u64s(r[3 * C.w:5 * C.w]), bool(r[-1])).view(np.uint32)) for r in rows]
    for form, got in run_forms(ctx, C.name + "_jac_add_mixed", rows):
        for i, (o, (p, q, *_, tag)) in enumerate(zip(got, cases)):
            assert C.from_jac(unflat(C, o, 3)) == C.add(p, q), (form, i, tag)
            assert o == host[i], (form, i, tag, "device and host jac_add_mixed differ")


@pytest.mark.parametrize("C", [G1, G2], ids=["g1", "g2"])
def test_xyzz_formulas_on_the_device(ctx, fam, C):
    cases = curve_cases(C, fam)
    INF = pyref.INF
    xp = [C.xyzz(p, zp) for p, _, zp, _, _ in cases]
    xp += [(x, y, C.zero, C.zero) for x, y, _, _ in xp[1:6]]
    pts = [p for p, *_ in cases] + [INF] * 5
    rows = [fl(x) for x in xp]
    for form, got in run_forms(ctx, C.name + "_xyzz_double", rows):
        for i, (o, p) in enumerate(zip(got, pts)):
            assert C.from_xyzz(unflat(C, o, 4)) == C.add(p, p), (form, i)
    for form, got in run_forms(ctx, C.name + "_xyzz_to_jac", rows):
        for i, (o, p) in enumerate(zip(got, pts)):
            assert C.from_jac(unflat(C, o, 3)) == p, (form, i)
    fin = [p for p in dict.fromkeys(pts) if p is not INF]              # xyzz_double_affine: an affine point, never infinity
    for form, got in run_forms(ctx, C.name + "_xyzz_double_affine", [fl(C.aff(p)) for p in fin]):
        for i, (o, p) in enumerate(zip(got, fin)):
            assert C.from_xyzz(unflat(C, o, 4)) == C.add(p, p), (form, i)
    rows = [fl(C.xyzz(p, zp), C.xyzz(q, zq)) for p, q, zp, zq, _ in cases]
    for form, got in run_forms(ctx, C.name + "_xyzz_add", rows):
        for i, (o, (p, q, *_, tag)) in enumerate(zip(got, cases)):
            assert C.from_xyzz(unflat(C, o, 4)) == C.add(p, q), (form, i, tag)
    mixed = [cs for cs in cases if cs[1] is not INF]                     # the mixed forms take an affine q that is not infinity
    assert len(mixed) >= len(cases) // 2
    rows = [fl(C.xyzz(p, zp), C.aff(q)) for p, q, zp, _, _ in mixed]
    for name in ("_xyzz_add_mixed", "_xyzz_acc_mixed"):
        for form, got in run_forms(ctx, C.name + name, rows):
            for i, (o, (p, q, *_, tag)) in enumerate(zip(got, mixed)):
                assert C.from_xyzz(unflat(C, o, 4)) == C.add(p, q), (name, form, i, tag)
