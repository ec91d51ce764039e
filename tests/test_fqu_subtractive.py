"""The signed-column (`_s`) multiplies of csrc/fqu.h on the device, limb for limb against tests/subtractive_model.py and lazy_model.py.

czk_lab_arith_probe runs fqu_mul_s / fqu_sqr_s / the fused `_s` multiplies on the operand sets of the CPU test (edge generators, quotient
digits all ones / all zero / top only / low only, every column at its maximum) plus the pairs that drive a column to the lowest and the
highest value the contract allows; every row is first vetted against the contract (column extremes from the model).  Then the two hot
formulas as 64-step chains, and one MSM per group through the accumulate and reduction kernels against the checker.
"""
import random

import numpy as np
import pytest

import czk_amd
import lazy_model as M
import pyref
import subtractive_model as SM
from lazy_model import FQ, P, R
from util import rand_fr_canonical

pytestmark = pytest.mark.gpu

CQ = M.Concrete(FQ)
NORM = 1 << 28
LIMIT = SM.I63 - (1 << 60)


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


def vetted(pairs, e=None, squares=()):
    """the model's limbs for one row, after checking that the row is inside the signed-column contract"""
    ex = [0, 0]
    r = SM.sub_mul_sum(pairs, e=e, squares=squares, extremes=ex)
    assert -SM.I63 < ex[0] and ex[1] < LIMIT, "test row outside the signed-column contract"
    return r, ex


def test_signed_multiplies_limb_exact(ctx):
    rng = random.Random(22)
    sets = SM.operand_sets()
    pairs = [(a, b) for _, a, b in sets] + SM.extreme_pairs()
    want, lows, highs = [], [], []
    for a, b in pairs:
        w, ex = vetted([(a, b)])
        assert w == CQ.mul(a, b) == FQ.digits(FQ.mont_exact(FQ.value(a) * FQ.value(b)))
        want.append(w), lows.append(ex[0]), highs.append(ex[1])
    assert min(lows) < -(1 << 58) and max(highs) > LIMIT * 95 // 100          # the extreme pairs do reach both ends
    check_exact(ctx, "fqu_mul_s", pairs, want)

    sq = [a for _, a, _ in sets if max(a) < 1 << 29] + [[int(2 ** 29.4)] * 13 + [0]]
    want = [vetted([], squares=[a])[0] for a in sq]
    assert want == [CQ.sqr(a) for a in sq]
    check_exact(ctx, "fqu_sqr_s", sq, want)

    # fused forms: one factor of each product normalised; e: any limbs below 2^32
    nrm = M.fam_largest(FQ, NORM, 9) + M.fam_patterns(FQ, NORM, 9) + M.fam_random(FQ, NORM, 9, rng, 24)
    es = M.fam_largest(FQ, 1 << 32, 30000) + M.fam_patterns(FQ, 1 << 32, 30000) + M.fam_random(FQ, 1 << 32, 30000, rng, 24)
    first = [(a, b) if max(b) < NORM else (b, a) for a, b in pairs if min(max(a), max(b)) < NORM]
    n = lambda i: nrm[i % len(nrm)]
    rows2 = [(a, b, first[(5 * i + 1) % len(first)][0], n(i)) for i, (a, b) in enumerate(first)]
    rows2 += [(a, b, a, b) for a, b in M.column_pairs(FQ, 1 << 30, NORM, 128, 9)]
    z = M.quotient_pairs(FQ, 9, rng)[1]
    rows2 += [(z[0], z[1], [0] * 14, n(1)), (z[0], z[1], z[0], z[1])]                    # quotient zero in a fused product
    want = [vetted([(a, b), (c, d)])[0] for a, b, c, d in rows2]
    assert want == [CQ.mul_add(*r) for r in rows2]
    check_exact(ctx, "fqu_mul_add_s", rows2, want)
    rows_hi = [r + (es[i % len(es)],) for i, r in enumerate(rows2)]
    want = [vetted([(a, b), (c, d)], e=e)[0] for a, b, c, d, e in rows_hi]
    assert want == [CQ.mul_add_hi(*r) for r in rows_hi]
    check_exact(ctx, "fqu_mul_add_hi_s", rows_hi, want)
    rows_h = [(a, b, es[i % len(es)]) for i, (a, b) in enumerate(pairs)]
    want = [vetted([(a, b)], e=e)[0] for a, b, e in rows_h]
    assert want == [CQ.mul_hi(*r) for r in rows_h]
    check_exact(ctx, "fqu_mul_hi_s", rows_h, want)
    # four products: at most limbs of 2^29 against normalised ones (the Y3 sites: 2 x 2^56 + 2 x 2^57 per term)
    small = [r for r in rows2 if max(max(r[0]), max(r[2])) < 1 << 29]
    rows4 = [small[i] + small[(i + 17) % len(small)] for i in range(len(small))]
    rows4.append((M.greedy_max(FQ, 1 << 29, 64), M.greedy_max(FQ, NORM, 9)) * 4)         # all four products at their column maximum
    want = [vetted([(r[0], r[1]), (r[2], r[3]), (r[4], r[5]), (r[6], r[7])])[0] for r in rows4]
    assert want == [CQ.mul_add4(*r) for r in rows4]
    check_exact(ctx, "fqu_mul_add4_s", rows4, want)
    assert 2000 <= len(pairs) + len(sq) + 2 * len(rows2) + len(rows_h) + len(rows4) <= 6000


# ------------------------------------------------------------------------------------------------------------------- chains
def g1(k):
    return pyref.ec_mul(pyref.F1, k, pyref.G1_GEN)


def g2(k):
    return pyref.ec_mul(pyref.F2, k, pyref.G2_GEN)


def u(v, j=0):
    return FQ.digits(v % P * FQ.one % P + j * P)


def res(l):
    return FQ.value(l) * pow(FQ.one, -1, P) % P


def rows_of(out, n=14):
    return [out[i:i + n] for i in range(0, len(out) - len(out) % n, n)]


def test_teu_madd_chain_of_64(ctx):
    """sixty-four teu_madd steps (five of its seven products on signed columns), positive and negated table points: every state limb-exact
    against the additive model, the last one against the affine law"""
    rng = random.Random(23)
    F = pyref.F1
    pts = [g1(rng.randrange(1, R)) for _ in range(6)]
    niels = [M.te_niels(p) for p in pts]
    loaded = {0: niels, 1: [M.te_negate_niels(CQ, *n) for n in niels]}
    i0 = rng.randrange(len(pts))
    state = flat(M.teu_from_niels(CQ, *niels[i0]))
    assert run(ctx, "teu_from_niels", [list(niels[i0])])[0] == state
    total = pts[i0]
    for step in range(64):
        i, neg = rng.randrange(len(pts)), rng.randrange(2)
        nl = list(loaded[neg][i])
        want = flat(M.teu_madd(CQ, rows_of(state), *nl))
        state = run(ctx, "teu_madd", [rows_of(state) + nl])[0]
        assert state == want, step
        total = pyref.ec_add(F, total, pyref.ec_neg(F, pts[i]) if neg else pts[i])
    X, Y, Z, T = (res(l) for l in rows_of(state))
    assert X * Y % P == Z * T % P and M.te_to_sw(X, Y, Z) == total


def test_fq2u_xyzz_acc_mixed_chain_of_64(ctx):
    """sixty-four fq2u_xyzz_acc_mixed steps from the largest accumulator representative (every multiply of the formula on signed columns)"""
    rng = random.Random(24)
    F = pyref.F2
    u2f = lambda v, j=(0, 0): [u(v[0], j[0]), u(v[1], j[1])]
    pts = [g2(rng.randrange(1, R)) for _ in range(4)]
    A = g2(rng.randrange(1, R))
    z = (rng.randrange(1, P), rng.randrange(P))
    zz = F.mul(z, z)
    zzz = F.mul(zz, z)
    acc = [u2f(F.mul(A[0], zz), (84, 84)), u2f(F.mul(A[1], zzz), (35, 35)), u2f(zz), u2f(zzz)]
    total = A
    for step in range(64):
        i, neg = rng.randrange(len(pts)), rng.randrange(2)
        qx, qy = u2f(pts[i][0]), u2f(pts[i][1])
        if neg:
            qy = [CQ.lin([], 4, 1, [(1, qy[0])]), CQ.lin([], 4, 1, [(1, qy[1])])]
        want = M.fq2u_xyzz_acc_mixed(CQ, *acc, qx, qy)
        assert want is not None
        g = run(ctx, "fq2u_xyzz_acc_mixed", [acc + [qx, qy]])[0]
        assert g == flat(want) + [1], step
        r = rows_of(g[:112])
        acc = [[r[2 * k], r[2 * k + 1]] for k in range(4)]
        total = pyref.ec_add(F, total, pyref.ec_neg(F, pts[i]) if neg else pts[i])
    X, Y, ZZ, ZZZ = ((res(c[0]), res(c[1])) for c in acc)
    assert (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ))) == total


# ---------------------------------------------------------------------------------------------------------------------- MSM
@pytest.mark.parametrize("g", [1, 2])
def test_msm_of_4096_points_and_4_lanes_against_the_checker(orc, g):
    """the accumulate and reduction kernels end to end: 2^12 points x 4 lanes per group, a base at infinity and a zero scalar included"""
    n, lanes = 1 << 12, 4
    ctx = czk_amd.Context(0)
    bases = ctx.fixed_base_points(g, rand_fr_canonical(0x5B70 + g, n))
    inf = np.zeros(n, dtype=np.uint8)
    inf[[3, n - 50]] = 1
    sc = rand_fr_canonical(0x5B80 + g, lanes * n).reshape(lanes, n, 4)
    sc[:, 7] = 0
    b = ctx.register_bases(g, bases, inf)
    got = ctx.msm(b, sc, lanes=lanes)
    for ln in range(lanes):
        want_aff, want_inf = orc.jac_to_affine(g, orc.multi_scalar_mul(g, bases, inf, orc.fr_from_repr(sc[ln])))
        have_aff, have_inf = ctx.jac_to_affine(g, got[ln])
        assert bool(have_inf[0]) == want_inf and (want_inf or np.array_equal(have_aff[0], want_aff)), (g, ln)
    b.release()
    ctx.close()
