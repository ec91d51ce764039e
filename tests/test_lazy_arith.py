"""The unsaturated Fq / Fr arithmetic ON THE DEVICE against the big-integer model, at the edges of its lazy bounds.

czk_lab_arith_probe (csrc/lab/arith_probe.hip, lab library only) runs one function of fqu.h / fru.h / te.h / fq2pu.h per item on raw
limbs, so a test can force any representative: the largest admissible limb vectors, values k p - 1 / k p / k p + 1, de-normalised
representatives, Montgomery quotient digits all ones / all zeros, single columns at their maximum, P == +-Q at every admissible
multiple of p.  Every comparison is exact integer equality: primitives against tests/lazy_model.py's closed formulas, formulas
against the model's limbs AND, as group elements, against oracle/pyref.py's affine law.  Before any expected value is used the
model's capacity checker has accepted the input (it raises otherwise).
"""
import random

import numpy as np
import pytest

import czk_amd
import lazy_model as M
import pyref
from lazy_model import FQ, FR, P, R

pytestmark = pytest.mark.gpu

CQ, CR = M.Concrete(FQ), M.Concrete(FR)
LAZY, NORM = 1 << 30, 1 << 28


@pytest.fixture(scope="module")
def ctx():
    c = czk_amd.Context(0, lab=True)
    yield c
    c.close()


def flat(*parts):
    out = []
    for p in parts:
        if isinstance(p, (list, tuple)):
            out += flat(*p)
        else:
            out.append(int(p))
    return out


def run(ctx, op, rows):
    return ctx.lab_arith_probe(op, np.array([flat(r) for r in rows], dtype=np.uint32)).tolist()


def check_exact(ctx, op, rows, want):
    got = run(ctx, op, rows)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != flat(w)]
    assert not bad, f"{op}: {len(bad)} of {len(rows)} items differ, first {bad[0]}: in {rows[bad[0]]} got {got[bad[0]]} want {flat(want[bad[0]])}"


@pytest.fixture(scope="module")
def fq_ops():
    """operand families of fqu.h's multiplies: lazy (limbs < 2^30, value < 2^7 p) and normalised (limbs < 2^28)"""
    rng = random.Random(2024)
    lazy = (M.fam_largest(FQ, LAZY, 128) + M.fam_patterns(FQ, LAZY, 128) + M.fam_special(FQ, 128) + M.fam_denormalised(FQ, LAZY, 128, rng, 150)
            + M.fam_random(FQ, LAZY, 128, rng, 150))
    norm = (M.fam_largest(FQ, NORM, 128) + M.fam_patterns(FQ, NORM, 128) + M.fam_special(FQ, 128, 12) + M.fam_random(FQ, NORM, 128, rng, 100))
    return {"rng": rng, "lazy": lazy, "norm": norm}


def subtrahends(S, K, U, limb_cap, rng, count):
    """operands a K mod table (limbs >= U 2^w) absorbs: every limb below limb_cap and at most the table's -- the top limb included, which
    is what "value below K mod" means exactly -- from the largest such vector down"""
    L = S.table(K, U)
    big = [min(limb_cap - 1, x) for x in L[:-1]] + [L[-1]]
    out = [big] + [big[:i] + [big[i] - 1] + big[i + 1:] for i in range(S.n)]
    out += [S.digits(v) for k in range(1, K) for v in (k * S.mod - 1, k * S.mod, k * S.mod + 1)]
    out += [S.digits(rng.randrange((K - 1) * S.mod)) for _ in range(count)]
    return out


def neg5_limit(big):
    """the largest operands of fqu_neg5 under its exact contract: 5 x the top limb at most the table's top limb, the rest normalised"""
    top = FQ.table(512 if big else 16, 5)[-1] // 5
    g = [NORM - 1] * 13 + [top]
    return [g] + [g[:i] + [g[i] - 1] + g[i + 1:] for i in range(14)]


def fq_sqrt(a):
    """Tonelli-Shanks in Fq (p - 1 = 2^46 t); None for a non-residue"""
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


def test_lab_probe_is_refused_on_a_product_context():
    c = czk_amd.Context(0)
    with pytest.raises(RuntimeError):
        c.lab_arith_probe("fqu_mul", np.zeros((1, 28), dtype=np.uint32))
    c.close()


# ------------------------------------------------------------------------------------------------------------- Fq primitives
def test_fqu_mul_and_sqr_at_the_edges(ctx, fq_ops):
    rng, lazy = fq_ops["rng"], fq_ops["lazy"]
    pairs = [(a, lazy[(7 * i + 3) % len(lazy)]) for i, a in enumerate(lazy)] + [(a, a) for a in lazy[:40]]
    pairs += M.quotient_pairs(FQ, 128, rng) + M.column_pairs(FQ, LAZY, LAZY, 128, 128)
    want = [CQ.mul(a, b) for a, b in pairs]
    assert want == [FQ.digits(FQ.mont_exact(FQ.value(a) * FQ.value(b))) for a, b in pairs]
    assert all(max(w[:13]) < NORM and FQ.value(w) * 100 < 101 * P + 128 * 128 * P * P * 100 // FQ.radix for w in want)
    check_exact(ctx, "fqu_mul", pairs, want)
    sq = [CQ.sqr(a) for a in lazy]
    assert sq == [FQ.digits(FQ.mont_exact(FQ.value(a) ** 2)) for a in lazy]
    check_exact(ctx, "fqu_sqr", lazy, sq)


def test_fqu_fused_multiplies_at_the_edges(ctx, fq_ops):
    """fqu_mul_add / _hi / mul_hi / mul_add4: one factor of each product lazy, one normalised (limb products < 2^58); e: limbs < 2^32"""
    rng, lazy, norm = fq_ops["rng"], fq_ops["lazy"], fq_ops["norm"]
    es = M.fam_largest(FQ, 1 << 32, 30000) + M.fam_patterns(FQ, 1 << 32, 30000) + M.fam_random(FQ, 1 << 32, 30000, rng, 40)
    n = lambda i: norm[i % len(norm)]
    rows2 = [(a, n(3 * i), lazy[(5 * i + 1) % len(lazy)], n(3 * i + 1)) for i, a in enumerate(lazy)]
    rows2 += [(a, b, a, b) for a, b in M.column_pairs(FQ, LAZY, NORM, 128, 128)]
    val = FQ.value
    want = [CQ.mul_add(*r) for r in rows2]
    assert want == [FQ.digits(FQ.mont_exact(val(a) * val(b) + val(c) * val(d))) for a, b, c, d in rows2]
    check_exact(ctx, "fqu_mul_add", rows2, want)
    rows_hi = [r + (es[i % len(es)],) for i, r in enumerate(rows2)]
    want = [CQ.mul_add_hi(*r) for r in rows_hi]
    assert want == [FQ.digits(FQ.mont_exact(val(a) * val(b) + val(c) * val(d) + (val(e) << 392))) for a, b, c, d, e in rows_hi]
    check_exact(ctx, "fqu_mul_add_hi", rows_hi, want)
    rows_h = [(a, lazy[(11 * i + 5) % len(lazy)], es[i % len(es)]) for i, a in enumerate(lazy)]
    want = [CQ.mul_hi(*r) for r in rows_h]
    assert want == [FQ.digits(FQ.mont_exact(val(a) * val(b) + (val(e) << 392))) for a, b, e in rows_h]
    check_exact(ctx, "fqu_mul_hi", rows_h, want)
    rows4 = [rows2[i] + rows2[(i + 17) % len(rows2)] for i in range(len(rows2))]
    rows4.append((M.greedy_max(FQ, LAZY, 128), M.greedy_max(FQ, NORM, 128)) * 4)       # all four products at the column maximum
    want = [CQ.mul_add4(*r) for r in rows4]
    assert want == [FQ.digits(FQ.mont_exact(sum(val(r[2 * j]) * val(r[2 * j + 1]) for j in range(4)))) for r in rows4]
    check_exact(ctx, "fqu_mul_add4", rows4, want)


def test_fqu_limbwise_primitives_at_the_edges(ctx, fq_ops):
    rng, lazy, norm = fq_ops["rng"], fq_ops["lazy"], fq_ops["norm"]
    wide = M.fam_largest(FQ, (1 << 32) - 16, 30000) + M.fam_patterns(FQ, (1 << 32) - 16, 30000) + M.fam_random(FQ, (1 << 32) - 16, 30000, rng, 60)
    ins = wide + lazy
    want = [CQ.norm(a) for a in ins]
    assert want == [FQ.digits(FQ.value(a)) for a in ins]
    check_exact(ctx, "fqu_normalize", ins, want)
    for K in (4, 8, 16):            # subtrahend: normalised, value < K p (its top limb stays under the table's)
        subs = subtrahends(FQ, K, 1, NORM, rng, 40)
        rows = [(lazy[(3 * i) % len(lazy)], b) for i, b in enumerate(subs)]
        check_exact(ctx, f"fqu_sub_lazy<{K}>", rows, [M.sub_lazy(CQ, K, a, b) for a, b in rows])
    for K in (32, 64, 128):
        subs = subtrahends(FQ, K, 1, NORM, rng, 40)
        rows = [(norm[(3 * i) % len(norm)], b) for i, b in enumerate(subs)]
        check_exact(ctx, f"fqu_subn_{K}", rows, [CQ.norm(CQ.lin([(1, a)], K, 1, [(1, b)])) for a, b in rows])
    small = M.fam_largest(FQ, NORM, 2) + M.fam_special(FQ, 2) + M.fam_random(FQ, NORM, 2, rng, 60)      # b + 2 c < 8 p
    rows = [(norm[i % len(norm)], small[i], small[(i + 9) % len(small)]) for i in range(len(small))]
    check_exact(ctx, "fqu_sub3_norm", rows, [M.sub3_norm(CQ, *r) for r in rows])
    for big, cap in ((False, 3), (True, 102)):     # whole multiples of p below the exact limit (3.1999 p / 102.4 p), then the limit itself
        a5 = neg5_limit(big) + M.fam_largest(FQ, NORM, cap) + M.fam_special(FQ, cap) + M.fam_random(FQ, NORM, cap, rng, 60)
        assert FQ.value(a5[0]) * 100 > (319 if not big else 10200) * P
        check_exact(ctx, "fqu_neg5<true>" if big else "fqu_neg5<false>", a5, [M.neg5(CQ, a, big) for a in a5])
    rows = [(a, lazy[(i + 1) % len(lazy)]) for i, a in enumerate(lazy)]
    check_exact(ctx, "fqu_add_lazy", rows, [M.add_lazy(CQ, a, b) for a, b in rows])
    vals = [0, 1, P - 1, P, (1 << 384) - 1, FQ.one] + [rng.randrange(1 << 384) for _ in range(100)]
    words = [[(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)] for v in vals]
    check_exact(ctx, "fqu_unpack", words, [M.unpack32(FQ, w) for w in words])
    check_exact(ctx, "fqu_pack", [FQ.digits(v) for v in vals], words)


# --------------------------------------------------------------------------------------------------------------------- Fr
def test_fru_canon_family_on_the_device(ctx):
    cases = [FR.digits(v) for q in range(439) for v in (q * R - 1, q * R, q * R + 1) if 0 <= v < 1 << 261] + [FR.digits((1 << 261) - 1)]
    for t in M.fru_quotient_steps():
        cases += [FR.digits(t << 232), FR.digits(((t + 1) << 232) - 1)]
    check_exact(ctx, "fru_reduce_2r", cases, [M.fru_reduce_2r(a)[1] for a in cases])
    canon = [[(M.fru_canon(a) >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for a in cases]
    assert all(M.fru_canon(a) == FR.value(a) % R for a in cases)
    check_exact(ctx, "fru_canon", cases, canon)
    outs = [a for a in cases if FR.value(a) < 2 * R]
    check_exact(ctx, "fru_canon_mulout", outs, [[(FR.value(a) % R >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for a in outs])


def test_fru_primitives_at_the_edges(ctx):
    rng = random.Random(77)
    cap = int(2 ** 31.4)
    lazy = M.fam_largest(FR, cap, 438) + M.fam_patterns(FR, cap, 438) + M.fam_special(FR, 438) + M.fam_random(FR, cap, 438, rng, 200)
    lazy = [a for a in lazy if FR.value(a) < 1 << 261]
    lazy += [M.denormalise(FR, FR.digits((1 << 261) - 1 - d), cap, rng) for d in range(8)]     # limbs up to 2^31.4, value just below 2^261
    assert max(max(a[:8]) for a in lazy[-8:]) > 1 << 31 and all(FR.value(a) >> 260 for a in lazy[-8:])
    mult = M.fam_largest(FR, 1 << 29, 2) + M.fam_special(FR, 2) + M.fam_random(FR, 1 << 29, 2, rng, 60)
    rows = [(a, mult[i % len(mult)]) for i, a in enumerate(lazy)] + M.quotient_pairs(FR, 2, rng) + M.column_pairs(FR, cap, 1 << 29, 438, 2)
    want = [CR.mul(a, b) for a, b in rows]
    assert want == [FR.digits(FR.mont_exact(FR.value(a) * FR.value(b))) for a, b in rows]
    check_exact(ctx, "fru_mul", rows, want)
    for lg in range(1, 9):
        for U in (1, 2):
            K = 1 << lg
            subs = subtrahends(FR, K, U, U << 29, rng, 20)
            mins = M.fam_largest(FR, 1 << 30, 200) + M.fam_random(FR, 1 << 30, 200, rng, 8)
            rows = [(mins[i % len(mins)], b) for i, b in enumerate(subs)]
            check_exact(ctx, f"fru_sub<{K},{U}>", rows, [M.fru_sub(CR, K, U, a, b) for a, b in rows])
    wide = M.fam_largest(FR, int(3.5 * (1 << 30)), 438) + M.fam_random(FR, int(3.5 * (1 << 30)), 438, rng, 60)      # "limbs stay below 3.5 * 2^30"
    check_exact(ctx, "fru_normalize", wide, [CR.norm(a) for a in wide])
    rows = [(a, lazy[(i + 1) % len(lazy)]) for i, a in enumerate(lazy) if max(a) + max(lazy[(i + 1) % len(lazy)]) < 1 << 32]
    check_exact(ctx, "fru_add", rows, [M.add_lazy(CR, a, b) for a, b in rows])
    vals = [0, 1, R - 1, R, 2 * R - 1, (1 << 256) - 1] + [rng.randrange(1 << 256) for _ in range(60)]
    words = [[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for v in vals]
    check_exact(ctx, "fru_unpack", words, [M.unpack32(FR, w) for w in words])
    check_exact(ctx, "fru_pack", [FR.digits(v) for v in vals], words)


# ------------------------------------------------------------------------------------------------------- points and formulas
def g1(k):
    return pyref.ec_mul(pyref.F1, k, pyref.G1_GEN)


def u(v, j=0):
    """field element -> u-form limbs at the representative residue + j p"""
    return FQ.digits(v % P * FQ.one % P + j * P)


def res(l):
    """u-form limbs -> field element (the R' factor removed)"""
    return FQ.value(l) * pow(FQ.one, -1, P) % P


def xyzz_rep(Pt, z, jx=0):
    x, y = Pt
    return [u(x * z * z, jx), u(y * z ** 3), u(z * z), u(z ** 3)]


def xyzz_affine(c):
    X, Y, ZZ, ZZZ = (res(l) for l in c)
    assert ZZ and ZZZ and pow(ZZ, 3, P) == ZZZ * ZZZ % P
    return X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P


def neg_lazy(y_limbs):
    return CQ.lin([], 4, 1, [(1, y_limbs)])


def rows_of(out, n=14):
    return [out[i:i + n] for i in range(0, len(out) - len(out) % n, n)]


def test_fqu_xyzz_acc_mixed_random_and_forced_cases(ctx):
    rng = random.Random(5)
    pts = [g1(rng.randrange(1, R)) for _ in range(12)]
    rows, want, sums = [], [], []
    for i, A in enumerate(pts):                              # ordinary additions, the accumulator at every multiple of p below 9 p
        Qp = pts[(i + 1) % len(pts)]
        for jx in range(9):
            for neg in (False, True):
                acc = xyzz_rep(A, rng.randrange(1, P), jx)
                acc[1] = FQ.digits(FQ.value(acc[1]) + rng.randrange(5) * P)          # y < 5.5 p
                qx, qy = u(Qp[0]), u(Qp[1])
                r = acc + [qx, neg_lazy(qy) if neg else qy]
                out = M.fqu_xyzz_acc_mixed(CQ, *r)            # the capacity checker accepts the input, and predicts the limbs
                assert out is not None
                rows.append(r), want.append(list(out) + [1]), sums.append(pyref.ec_add(pyref.F1, A, pyref.ec_neg(pyref.F1, Qp) if neg else Qp))
    got = run(ctx, "fqu_xyzz_acc_mixed", rows)
    for g, w, s in zip(got, want, sums):
        assert g == flat(w)
        c = rows_of(g)
        assert max(max(l[:13]) for l in c) < NORM and FQ.value(c[0]) * 2 < 19 * P and all(FQ.value(l) * 100 < 101 * P for l in c[1:])
        assert xyzz_affine(c) == s
    # P == +-Q at every admissible representative of the accumulator's x: the filter must report, the inputs stay untouched
    rows = []
    for A in pts[:4]:
        for jx in range(10):
            for neg in (False, True):
                acc = xyzz_rep(A, rng.randrange(1, P), jx)
                if FQ.value(acc[0]) * 2 >= 19 * P:
                    continue
                rows.append(acc + [u(A[0]), neg_lazy(u(A[1])) if neg else u(A[1])])
                assert M.fqu_xyzz_acc_mixed(CQ, *rows[-1]) is None
    assert len(rows) >= 72
    got = run(ctx, "fqu_xyzz_acc_mixed", rows)
    assert all(g == flat(r[:4]) + [0] for g, r in zip(got, rows))
    # false alarm: the low limb of H inside the window while H != 0 mod p -- `false` is allowed, the inputs stay untouched
    rows = []
    for t in range(6, 19):
        acc = xyzz_rep(pts[0], rng.randrange(1, P), 3)
        qx = u(pts[1][0])
        u2 = CQ.mul(qx, acc[2])
        acc[0][0] = (u2[0] + FQ.table(16, 1)[0] - t) & FQ.mask
        assert (FQ.value(CQ.mul(qx, acc[2])) - FQ.value(acc[0])) % P != 0 and M.fqu_xyzz_acc_mixed(CQ, *acc, qx, u(pts[1][1])) is None
        rows.append(acc + [qx, u(pts[1][1])])
    got = run(ctx, "fqu_xyzz_acc_mixed", rows)
    assert all(g == flat(r[:4]) + [0] for g, r in zip(got, rows))


def test_xyzzu_add_and_double_with_exceptional_cases(ctx):
    rng = random.Random(6)
    F = pyref.F1
    pts = [g1(rng.randrange(1, R)) for _ in range(8)]
    zero = [[0] * 14] * 4
    rows, sums = [], []

    def rep(Pt, jx):
        return xyzz_rep(Pt, rng.randrange(1, P), jx)

    for i, A in enumerate(pts):
        B = pts[(i + 3) % len(pts)]
        for jx in (0, 4, 8):
            rows.append(rep(A, jx) + [0] + rep(B, 8 - jx) + [0]), sums.append(pyref.ec_add(F, A, B))
        for jx in range(9):                                   # P == Q and P == -Q, both operands at every representative up to the largest
            rows.append(rep(A, jx) + [0] + rep(A, 8 - jx) + [0]), sums.append(pyref.ec_add(F, A, A))
            rows.append(rep(A, jx) + [0] + rep(pyref.ec_neg(F, A), 8) + [0]), sums.append(None)
        rows.append(zero + [1] + rep(A, 8) + [0]), sums.append(A)                  # accumulator at infinity
        rows.append(rep(A, 8) + [0] + zero + [1]), sums.append(A)                  # Q at infinity
    rows.append(zero + [1] + zero + [1]), sums.append(None)
    for r in rows:                                            # the capacity checker runs the fast path of every finite pair
        if not r[4] and not r[9]:
            M.xyzzu_add(CQ, r[:4], r[5:9])
    got = run(ctx, "xyzzu_add", rows)
    for g, s, r in zip(got, sums, rows):
        assert (g[56] == 1) == (s is None)
        if s is not None:
            c = rows_of(g[:56])
            assert max(max(l[:13]) for l in c) < NORM and FQ.value(c[0]) * 2 < 19 * P
            if not r[4] and not r[9]:                         # a sum (fast or slow path): y, zz, zzz multiply outputs
                assert all(FQ.value(l) * 100 < 101 * P for l in c[1:])
            assert xyzz_affine(c) == s
    # exact limbs on the fast path
    fast = [r for r in rows if not r[4] and not r[9] and M.xyzzu_add(CQ, r[:4], r[5:9]) is not None]
    check_exact(ctx, "xyzzu_add", fast, [list(M.xyzzu_add(CQ, r[:4], r[5:9])) + [0] for r in fast])
    # a false alarm with real points: b affine (zz = R'), x2 chosen so that U2 - U1 is a non-zero multiple of 2^28 plus -1, 0 or 1
    alarms = []
    A = pts[0]
    a = rep(A, 0)
    lam2 = res(a[2])
    u1 = FQ.value(a[0]) % P
    k = 1
    while len(alarms) < 3:
        k += 1
        for t in (3, 4, 5):
            tgt = (u1 + (k << 28) + t - 4) % P                # integer value of U2: low limb of U2 - U1 + 4 p is t
            x2 = tgt * pow(FQ.one, -1, P) * pow(lam2, -1, P) % P
            y2 = fq_sqrt((x2 ** 3 + 1) % P)
            if y2 is None:
                continue
            alarms.append((a + [0] + [u(x2), u(y2), u(1), u(1)] + [0], pyref.ec_add(F, A, (x2, y2))))
    for r, _ in alarms:
        assert M.xyzzu_add(CQ, r[:4], r[5:9]) is None         # the model takes the slow path too
    got = run(ctx, "xyzzu_add", [r for r, _ in alarms])
    for g, (_, s) in zip(got, alarms):
        assert g[56] == 0 and xyzz_affine(rows_of(g[:56])) == s
    # doubling
    rows = [rep(A, jx) + [0] for A in pts for jx in range(9)]
    want = [list(M.xyzzu_double(CQ, r[:4])) + [0] for r in rows]
    got = run(ctx, "xyzzu_double", rows)
    for g, w, r in zip(got, want, rows):
        assert g == flat(w)
    for g, A in zip(got[::9], pts):
        assert xyzz_affine(rows_of(g[:56])) == pyref.ec_add(F, A, A)
    assert run(ctx, "xyzzu_double", [zero + [1]])[0][56] == 1
    # points of order two, (-1, 0) and (-zeta, 0): Y == 0 at every representative j p the discipline admits (y <= 4 p) gives the neutral element, flag
    # set -- the family serves keys that may hold any curve point (CZK_MEM_ANY_POINTS); and a false alarm, a real point whose Y has a low limb below
    # the filter's bound, still doubles to the right point through the complete formulas
    zeta = next(z for z in (pow(g, (P - 1) // 3, P) for g in range(2, 20)) if z != 1)
    for T in ((P - 1, 0), (-zeta % P, 0)):
        assert pyref.ec_on_curve(pyref.F1, T, 1)
        rows = []
        for j in range(5):
            z = rng.randrange(1, P)
            rows.append([u(T[0] * z * z, j), FQ.digits(j * P), u(z * z), u(z ** 3)] + [0])
        for g in run(ctx, "xyzzu_double", rows):
            assert g[56] == 1
    alarm, n3 = [], (P - 1) // 3                               # 9 does not divide p - 1: a cube c has the cube root c^(1 / 3 mod (p - 1) / 3)
    assert n3 % 3
    while len(alarm) < 3:
        x = rng.randrange(P)
        y = fq_sqrt((x ** 3 + 1) % P)
        if y is None:
            continue
        Yv = (rng.randrange(1, 1 << 340) << 28) + 4 * len(alarm)      # the integer Y = y z^3 R' is to be: not 0 mod p, low limb 0, 4, 8
        c = Yv * pow(y * FQ.one, -1, P) % P
        if pow(c, n3, P) != 1:
            continue                                               # z^3 = c has no solution
        z = pow(c, pow(3, -1, n3), P)
        assert pow(z, 3, P) == c
        row = xyzz_rep((x, y), z)
        assert FQ.value(row[1]) == Yv and row[1][0] <= 8
        alarm.append((row + [0], pyref.ec_add(F, (x, y), (x, y))))
    for g, (_, s) in zip(run(ctx, "xyzzu_double", [r for r, _ in alarm]), alarm):
        assert g[56] == 0 and xyzz_affine(rows_of(g[:56])) == s


def jac_affine(words):
    X, Y, Z = (sum(w << (32 * i) for i, w in enumerate(words[12 * k:12 * k + 12])) for k in range(3))
    if Z == 0:
        return None
    Rm = pow(1 << 384, -1, P)                                  # saturated Montgomery form: each coordinate carries the factor 2^384
    X, Y, Z = X * Rm % P, Y * Rm % P, Z * Rm % P
    zi = pow(Z, -1, P)
    return X * zi * zi % P, Y * zi ** 3 % P


def test_teu_madd_chain_of_64_with_negated_points(ctx):
    """sixty-four consecutive teu_madd steps on one accumulator (first entry through teu_from_niels), positive table points and negated
    ones (the lazy 4 p - k2 of te_load_niels), every intermediate state checked: limbs against the model, the point -- through teu_to_jac
    on the device and through the birational map in Python -- against the affine law"""
    rng = random.Random(8)
    F = pyref.F1
    ks = [rng.randrange(1, R) for _ in range(8)]
    pts = [g1(k) for k in ks]
    niels = [M.te_niels(p) for p in pts]
    entry = [flat([n[0] + [0, 0], n[1] + [0, 0], n[2] + [0, 0]]) for n in niels]
    loaded = {neg: run(ctx, "te_load_niels", [e + [neg, 0, 0, 0] for e in entry]) for neg in (0, 1)}
    for neg in (0, 1):
        for n, g in zip(niels, loaded[neg]):
            assert g == flat(M.te_negate_niels(CQ, *n) if neg else n)
    seq = [(rng.randrange(len(pts)), rng.randrange(2)) for _ in range(65)]
    i0, n0 = seq[0]
    state = run(ctx, "teu_from_niels", [rows_of(loaded[n0][i0])])[0]
    assert state == flat(M.teu_from_niels(CQ, *rows_of(loaded[n0][i0])))
    total = pyref.ec_neg(F, pts[i0]) if n0 else pts[i0]
    states, totals = [state], [total]
    for i, neg in seq[1:]:
        nl = rows_of(loaded[neg][i])
        want = flat(M.teu_madd(CQ, rows_of(state), *nl))     # capacity-checked, limb-exact
        state = run(ctx, "teu_madd", [rows_of(state) + nl])[0]
        assert state == want
        total = pyref.ec_add(F, total, pyref.ec_neg(F, pts[i]) if neg else pts[i])
        states.append(state), totals.append(total)
    jac = run(ctx, "teu_to_jac", states)
    for n, (st, jw, tot) in enumerate(zip(states, jac, totals)):
        c = rows_of(st)
        assert max(max(l[:13]) for l in c) < NORM
        if n:                                                  # after a teu_madd: every coordinate a multiply output
            assert all(FQ.value(l) * 100 < 101 * P for l in c)
        else:                                                  # after teu_from_niels: x < 5 p, y < 2 p, z = 2, t a multiply output
            assert FQ.value(c[0]) < 5 * P and FQ.value(c[1]) < 2 * P and FQ.value(c[2]) == 2 * FQ.one and FQ.value(c[3]) * 100 < 101 * P
        X, Y, Z, T = (res(l) for l in c)
        assert X * Y % P == Z * T % P
        assert M.te_to_sw(X, Y, Z) == tot and jac_affine(jw) == tot
    # the other formulas on two of the states, and P + (-P) = the neutral element through the unified law
    a, b = rows_of(states[5]), rows_of(states[40])
    check_exact(ctx, "teu_add", [a + b, a + a], [M.teu_add(CQ, a, b), M.teu_add(CQ, a, a)])
    check_exact(ctx, "teu_double", [a, rows_of(states[0])], [M.teu_double(CQ, a), M.teu_double(CQ, rows_of(states[0]))])
    s = rows_of(run(ctx, "teu_add", [a + b])[0])
    assert M.te_to_sw(*(res(l) for l in s[:3])) == pyref.ec_add(F, totals[5], totals[40])
    one = rows_of(run(ctx, "teu_from_niels", [rows_of(loaded[0][0])])[0])
    gone = rows_of(run(ctx, "teu_madd", [one + rows_of(loaded[1][0])])[0])
    assert res(gone[0]) == 0 and res(gone[1]) == res(gone[2]) != 0
    assert jac_affine(run(ctx, "teu_to_jac", [gone])[0]) is None


# ---- G2
def g2(k):
    return pyref.ec_mul(pyref.F2, k, pyref.G2_GEN)


def u2f(v, j=(0, 0)):
    return [u(v[0], j[0]), u(v[1], j[1])]


def res2(c):
    return res(c[0]), res(c[1])


def xyzz2_rep(Pt, z, jx=(0, 0), jy=(0, 0)):
    F = pyref.F2
    zz = F.mul(z, z)
    zzz = F.mul(zz, z)
    return [u2f(F.mul(Pt[0], zz), jx), u2f(F.mul(Pt[1], zzz), jy), u2f(zz), u2f(zzz)]


def xyzz2_affine(c):
    F = pyref.F2
    X, Y, ZZ, ZZZ = (res2(x) for x in c)
    assert F.mul(F.mul(ZZ, ZZ), ZZ) == F.mul(ZZZ, ZZZ)
    return F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ))


def pairs_of(out):
    r = rows_of(out)
    return [[r[2 * i], r[2 * i + 1]] for i in range(len(r) // 2)]


def test_fq2u_products(ctx):
    rng = random.Random(9)
    ops = [[a, b] for a, b in zip(M.fam_largest(FQ, NORM, 3) + M.fam_special(FQ, 3) + M.fam_random(FQ, NORM, 3, rng, 60),
                                  M.fam_random(FQ, NORM, 3, rng, 200))]
    rows = [(a, ops[(i + 5) % len(ops)]) for i, a in enumerate(ops)]
    for name, f in (("fq2u_mul", M.fq2u_mul), ("fq2u_mul_n5", lambda B, a, b: M.fq2u_mul_n5(B, a, b, M.neg5(B, b[1], False)))):
        want = [f(CQ, a, b) for a, b in rows]
        for (a, b), w in zip(rows, want):
            assert res2(w) == pyref.fq2_mul(res2(a), res2(b))
        check_exact(ctx, name, rows, want)
    big = [[a, b] for a, b in zip(M.fam_largest(FQ, NORM, 131) + M.fam_random(FQ, NORM, 131, rng, 60), M.fam_random(FQ, NORM, 131, rng, 200))]
    want = [M.fq2u_sqr(CQ, a) for a in big]
    for a, w in zip(big, want):
        assert res2(w) == pyref.fq2_mul(res2(a), res2(a))
    check_exact(ctx, "fq2u_sqr", big, want)


def test_fq2u_xyzz_acc_mixed_chain_of_64_from_the_largest_accumulator(ctx):
    """sixty-four fq2u_xyzz_acc_mixed steps starting from the largest admissible accumulator representative (X just below 85 p,
    Y just below 36 p, both halves), positive and negated table points; every state: limbs against the model, documented bounds, and the
    group element against the affine law.  Then P == +-Q at the largest representatives: the filter reports, the inputs stay."""
    rng = random.Random(10)
    F = pyref.F2
    pts = [g2(rng.randrange(1, R)) for _ in range(6)]
    A = g2(rng.randrange(1, R))
    acc = xyzz2_rep(A, (rng.randrange(1, P), rng.randrange(P)), (84, 84), (35, 35))
    total = A
    for step in range(64):
        i, neg = rng.randrange(len(pts)), rng.randrange(2)
        qx, qy = u2f(pts[i][0]), u2f(pts[i][1])
        if neg:
            qy = [neg_lazy(qy[0]), neg_lazy(qy[1])]
        want = M.fq2u_xyzz_acc_mixed(CQ, *acc, qx, qy)
        assert want is not None
        g = run(ctx, "fq2u_xyzz_acc_mixed", [acc + [qx, qy]])[0]
        assert g == flat(want) + [1], step
        acc = pairs_of(g[:112])
        total = pyref.ec_add(F, total, pyref.ec_neg(F, pts[i]) if neg else pts[i])
        for c, cap in zip(acc, (85, 36, 3, 3)):
            assert max(max(h[:13]) for h in c) < NORM and all(FQ.value(h) < cap * P for h in c)
        assert xyzz2_affine(acc) == total, step
    rows = []
    for jx in ((0, 0), (84, 84), (84, 0), (40, 17)):
        for neg in (False, True):
            a = xyzz2_rep(A, (rng.randrange(1, P), rng.randrange(P)), jx, (35, 35))
            qy = u2f(A[1])
            rows.append(a + [u2f(A[0]), [neg_lazy(qy[0]), neg_lazy(qy[1])] if neg else qy])
            assert M.fq2u_xyzz_acc_mixed(CQ, *rows[-1]) is None
    got = run(ctx, "fq2u_xyzz_acc_mixed", rows)
    assert all(g == flat(r[:4]) + [0] for g, r in zip(got, rows))


def test_lane_pair_forms(ctx):
    """fq2pu.h on adjacent lanes: p2_mul, xyzzu2_add (with P == +-Q and infinities, both operands at their largest representatives),
    xyzzu2_double, xyzzu2_acc_mixed"""
    rng = random.Random(11)
    F = pyref.F2
    pts = [g2(rng.randrange(1, R)) for _ in range(5)]
    zf = lambda: (rng.randrange(1, P), rng.randrange(P))
    ops = [[a, b] for a, b in zip(M.fam_largest(FQ, LAZY, 100) + M.fam_random(FQ, LAZY, 100, rng, 40), M.fam_random(FQ, LAZY, 100, rng, 100))]
    for big, cap in ((0, 3), (1, 102)):
        mult = [[a, b] for a, b in zip(M.fam_largest(FQ, NORM, cap) + M.fam_random(FQ, NORM, cap, rng, 40), M.fam_random(FQ, NORM, cap, rng, 100))]
        mult = [[a, a] for a in neg5_limit(bool(big))] + mult      # the multiplier's c1 half goes through fqu_neg5: its exact limit
        rows = [(a, mult[i % len(mult)], big) for i, a in enumerate(ops)]
        check_exact(ctx, "p2_mul", rows, [M.p2_mul(CQ, a, b, bool(big)) for a, b, _ in rows])
    zero = [[[0] * 14] * 2] * 4
    big_rep = lambda Pt: xyzz2_rep(Pt, zf(), (98, 98), (35, 35))
    rows, sums = [], []
    for i, A in enumerate(pts):
        B = pts[(i + 1) % len(pts)]
        rows.append(big_rep(A) + [0] + big_rep(B) + [0]), sums.append(pyref.ec_add(F, A, B))
        rows.append(xyzz2_rep(A, zf()) + [0] + big_rep(B) + [0]), sums.append(pyref.ec_add(F, A, B))
        rows.append(big_rep(A) + [0] + big_rep(A) + [0]), sums.append(pyref.ec_add(F, A, A))
        rows.append(big_rep(A) + [0] + big_rep(pyref.ec_neg(F, A)) + [0]), sums.append(None)
        rows.append(zero + [1] + big_rep(A) + [0]), sums.append(A)
        rows.append(big_rep(A) + [0] + zero + [1]), sums.append(A)
    fast = []
    for r in rows:
        if not r[4] and not r[9]:
            w = M.xyzzu2_add(CQ, r[:4], r[5:9])
            if w is not None:
                fast.append((r, w))
    got = run(ctx, "xyzzu2_add", rows)
    for g, s in zip(got, sums):
        assert (g[112] == 1) == (s is None)
        if s is not None:
            assert xyzz2_affine(pairs_of(g[:112])) == s
    assert len(fast) >= 10
    check_exact(ctx, "xyzzu2_add", [r for r, _ in fast], [list(w) + [0] for _, w in fast])
    for g in run(ctx, "xyzzu2_add", [r for r, _ in fast]):
        c = pairs_of(g[:112])
        assert all(max(h[:13]) < NORM for x in c for h in x) and all(FQ.value(h) * 5 < 46 * P for h in c[0]) and all(FQ.value(h) * 5 < 6 * P for x in c[1:] for h in x)
    rows = [big_rep(A) + [0] for A in pts] + [xyzz2_rep(A, zf()) + [0] for A in pts]
    want = [list(M.xyzzu2_double(CQ, r[:4])) + [0] for r in rows]
    check_exact(ctx, "xyzzu2_double", rows, want)
    for g, A in zip(run(ctx, "xyzzu2_double", rows), pts + pts):
        assert xyzz2_affine(pairs_of(g[:112])) == pyref.ec_add(F, A, A)
    rows, want, sums = [], [], []
    for i, A in enumerate(pts):
        for neg in (False, True):
            B = pts[(i + 2) % len(pts)]
            acc = xyzz2_rep(A, zf(), (8, 8), (2, 2))
            qy = u2f(B[1])
            rows.append(acc + [u2f(B[0]), [neg_lazy(qy[0]), neg_lazy(qy[1])] if neg else qy])
            want.append(list(M.xyzzu2_acc_mixed(CQ, *rows[-1])) + [1]), sums.append(pyref.ec_add(F, A, pyref.ec_neg(F, B) if neg else B))
            same = acc + [u2f(A[0]), [neg_lazy(u(A[1][0])), neg_lazy(u(A[1][1]))] if neg else u2f(A[1])]
            assert M.xyzzu2_acc_mixed(CQ, *same) is None
            rows.append(same), want.append(acc + [0]), sums.append(None)
    got = run(ctx, "xyzzu2_acc_mixed", rows)
    for g, w, s in zip(got, want, sums):
        assert g == flat(w)
        if s is not None:
            assert xyzz2_affine(pairs_of(g[:112])) == s


# ---- u-form <-> saturated Montgomery form
def sat_words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(12)]


def test_xyzzu_to_sat_and_from_sat(ctx):
    """xyzzu_to_sat multiplies the packed integer by 2^376 under the saturated reduction: value 2^384 / R' = value / 2^8 mod p, canonical;
    xyzzu_from_sat is the inverse map onto canonical u-form limbs.  Finite points at every representative of x, the edge values
    k p - 1 / k p / k p + 1, the point at infinity; the round trip reproduces the residue."""
    rng = random.Random(12)
    inv8, zero = pow(256, -1, P), [[0] * 14] * 4
    pts = [g1(rng.randrange(1, R)) for _ in range(4)]
    rows = [xyzz_rep(A, rng.randrange(1, P), jx) + [0] for A in pts for jx in range(9)]
    edge = [FQ.digits(v) for k in range(10) for v in (k * P - 1, k * P, k * P + 1) if 0 <= v and 2 * v < 19 * P]     # x < 9.5 p
    small = [FQ.digits(v) for v in (1, P - 1, P, P + 1, FQ.one, 101 * P // 100 - 1)]                                  # multiply outputs
    rows += [[x, small[i % len(small)], small[(i + 1) % len(small)], small[(i + 2) % len(small)], 0] for i, x in enumerate(edge)]
    want = [flat([sat_words(FQ.value(l) * inv8 % P) for l in r[:4]]) for r in rows]
    check_exact(ctx, "xyzzu_to_sat", rows, want)
    inf = run(ctx, "xyzzu_to_sat", [rows[0][:4] + [1], zero + [1]])
    for g in inf:                                               # XYZZ<Fq>::zero(): zz == zzz == 0
        assert g[24:48] == [0] * 24
    back = run(ctx, "xyzzu_from_sat", want)
    for g, r in zip(back, rows):
        c = rows_of(g[:56])
        assert g[56] == (1 if FQ.value(r[2]) % P == 0 else 0)
        if not g[56]:
            assert [FQ.value(l) for l in c] == [FQ.value(l) % P for l in r[:4]] and max(max(l[:13]) for l in c) < NORM
    assert sum(g[56] for g in back) == sum(FQ.value(r[2]) % P == 0 for r in rows) > 0       # zz == p: a residue of zero reads as infinity
    sat = [[rng.randrange(P), rng.randrange(P), rng.randrange(1, P), rng.randrange(P)] for _ in range(40)] + [[0, 1, P - 1, P - 1], [P - 1, 0, 1, 1]]
    check_exact(ctx, "xyzzu_from_sat", [[sat_words(v) for v in r] for r in sat], [[FQ.digits(v * 256 % P) for v in r] + [0] for r in sat])
    assert run(ctx, "xyzzu_from_sat", [[sat_words(v) for v in (5, 7, 0, 9)]])[0] == [0] * 56 + [1]
    for g, r in zip(run(ctx, "xyzzu_to_sat", [[FQ.digits(v * 256 % P) for v in r] + [0] for r in sat]), sat):
        assert g == flat([sat_words(v) for v in r])


# ---- Fq2: forced P == +-Q at every representative, and false alarms of the two-half filters
class Spy(M.Concrete):
    """the capacity checker, remembering what each filter compare saw"""

    def __init__(self):
        super().__init__(FQ)
        self.seen = []

    def window(self, a, name, masked):
        self.seen.append(super().window(a, name, masked))
        return self.seen[-1]


def fq2_sqrt(a):
    """square root in Fq2 = Fq[u] / (u^2 + 5) through the norm; None for a non-residue"""
    a0, a1 = a
    s = fq_sqrt((a0 * a0 + 5 * a1 * a1) % P) if (a0 or a1) else 0
    if s is None:
        return None
    for sg in (s, -s):
        x0 = fq_sqrt((a0 + sg) * pow(2, -1, P) % P) if (a0 + sg) % P else None
        if x0:
            r = (x0, a1 * pow(2 * x0, -1, P) % P)
            if pyref.fq2_mul(r, r) == (a0 % P, a1 % P):
                return r
    return None


def g2_with_low_limbs(A, K, targets, rng, accept):
    """a point Q of E'(Fq2) whose u-form x has, in every half c that `targets` names, the low limb of x_c - A.x_c + K p equal to
    targets[c] (p == 1 mod 2^28: shift A's half by a multiple of 2^28 plus targets[c] - K); the other half is free.  The products
    in front of the filter may add a multiple of p, i.e. a small number, to that limb: `accept` has the last word."""
    F, k = pyref.F2, 0
    r1 = pow(FQ.one, -1, P)
    while True:
        k += 1
        x = []
        for c in (0, 1):
            if c in targets:
                v = FQ.value(u(A[0][c])) + (k << 28) + targets[c] - K   # K p contributes K to the low limb
                if v >= P:
                    break
                x.append(v * r1 % P)
            else:
                x.append(rng.randrange(P))
        else:
            x = tuple(x)
            y = fq2_sqrt(F.add(F.mul(x, F.mul(x, x)), pyref.G2_B))
            if y is not None and y != (0, 0) and accept((x, y)):
                return x, y


def affine2(Pt, jx=(0, 0)):
    """(x, y, 1, 1) in u-form: zz = zzz = R', what an accumulator holds after its first point"""
    return [u2f(Pt[0], jx), u2f(Pt[1]), u2f((1, 0)), u2f((1, 0))]


def test_fq2_filters_forced_at_every_representative_and_false_alarms(ctx):
    """fq2u_xyzz_acc_mixed, xyzzu2_acc_mixed, xyzzu2_add.
    Forced: P == Q and P == -Q with one half of the accumulator's x swept over every admissible multiple of p and the other half at its
    extremes -- the filter must report (acc_mixed: false, inputs untouched; add: the slow path returns 2 P or infinity).
    False alarms on real curve points: both halves of H inside the window while H != 0 (acc_mixed: false is allowed, inputs untouched;
    add: the slow path must return the right sum), and ONE half inside, the other outside -- the conjunction must not fire: fast path,
    limbs equal to the model's, the right sum."""
    rng = random.Random(13)
    F = pyref.F2
    A = g2(rng.randrange(1, R))
    zf = lambda: (rng.randrange(1, P), rng.randrange(P))

    def sweep(top):
        return [(j, e) for j in range(top + 1) for e in (0, top)] + [(e, j) for j in range(top + 1) for e in (0, top)]

    def signed(Pt, neg):
        qy = u2f(Pt[1])
        return [u2f(Pt[0]), [neg_lazy(qy[0]), neg_lazy(qy[1])] if neg else qy]

    for op, f, top, jy in (("fq2u_xyzz_acc_mixed", M.fq2u_xyzz_acc_mixed, 84, (35, 35)), ("xyzzu2_acc_mixed", M.xyzzu2_acc_mixed, 8, (2, 2))):
        rows = [xyzz2_rep(A, zf(), jx, jy) + signed(A, neg) for jx in sweep(top) for neg in (False, True)]
        for r in rows:                                         # the capacity checker accepts every row, and sees the filter fire
            assert f(CQ, *r) is None
        got = run(ctx, op, rows)
        bad = [i for i, (g, r) in enumerate(zip(got, rows)) if g != flat(r[:4]) + [0]]
        assert not bad, (op, len(bad), bad[:5])
    rows, sums = [], []
    for jx in sweep(99):
        a = xyzz2_rep(A, zf(), jx, (35, 35))
        rows.append(a + [0] + xyzz2_rep(A, zf(), (99 - jx[0], 99 - jx[1]), (35, 35)) + [0]), sums.append(pyref.ec_add(F, A, A))
        rows.append(a + [0] + xyzz2_rep(pyref.ec_neg(F, A), zf(), (99, 99), (35, 35)) + [0]), sums.append(None)
    for r in rows:
        assert M.xyzzu2_add(CQ, r[:4], r[5:9]) is None
    for g, s in zip(run(ctx, "xyzzu2_add", rows), sums):
        assert (g[112] == 1) == (s is None)
        if s is not None:
            assert xyzz2_affine(pairs_of(g[:112])) == s

    # false alarms: (function, K of H = U2 - X1 + K p, a window value, one just outside)
    def model(op, Qp, neg):
        spy = Spy()
        if op == "xyzzu2_add":
            row = affine2(A) + [0] + affine2(Qp) + [0]
            return row, M.xyzzu2_add(spy, row[:4], row[5:9]), spy.seen[:2]
        row = affine2(A) + signed(Qp, neg)
        return row, (M.fq2u_xyzz_acc_mixed if op == "fq2u_xyzz_acc_mixed" else M.xyzzu2_acc_mixed)(spy, *row), spy.seen[:2]

    for op, K, tin, tout in (("fq2u_xyzz_acc_mixed", 128, 100, 30), ("fq2u_xyzz_acc_mixed", 128, 42, 156), ("xyzzu2_acc_mixed", 16, 12, 2),
                             ("xyzzu2_acc_mixed", 16, 16, 23), ("xyzzu2_add", 4, 4, 0), ("xyzzu2_add", 4, 4, 9)):
        for targets, pattern in (({0: tin, 1: tin}, [True, True]), ({0: tin, 1: tout}, [True, False]), ({0: tout, 1: tin}, [False, True]),
                                 ({0: tin}, [True, False]), ({1: tin}, [False, True])):
            for neg in ((False,) if op == "xyzzu2_add" else (False, True)):
                Qp = g2_with_low_limbs(A, K, targets, rng, lambda Qc: model(op, Qc, neg)[2] == pattern)
                Qs = pyref.ec_neg(F, Qp) if neg else Qp
                row, want, seen = model(op, Qp, neg)
                assert seen == pattern and (want is None) == all(pattern)       # the halves aimed at are inside the window, the others outside
                g = run(ctx, op, [row])[0]
                total = pyref.ec_add(F, A, Qs)
                assert total is not None
                if want is not None:                           # one half outside: the fast path, exactly
                    assert g == flat(want) + [0 if op == "xyzzu2_add" else 1], (op, targets, neg)
                    assert xyzz2_affine(pairs_of(g[:112])) == total
                elif op == "xyzzu2_add":                       # both inside, H != 0: the slow path returns the sum
                    assert g[112] == 0 and xyzz2_affine(pairs_of(g[:112])) == total
                else:                                          # both inside: `false`, inputs untouched
                    assert g == flat(row[:4]) + [0]
