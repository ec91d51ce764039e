"""The contracts of the unsaturated Fq / Fr arithmetic (csrc/fqu.h, fru.h, te.h, fq2pu.h), checked without a GPU.

The hot kernels are correct only while hand-derived preconditions hold -- operand ranges, 64-bit column capacity, non-negative limbs
under the K p tables, value discipline through whole formulas, the p == 1 mod 2^28 filters, fru_canon's quotient estimate.  Here each
is stated on tests/lazy_model.py (big integers, no product code) and the constants and windows are read from the source TEXT, so a
changed hex digit or a narrowed window fails.  The kernels themselves are held to the same model by tests/test_lazy_arith.py.
"""
import os
import random
import re
from fractions import Fraction as Q

import pytest

import lazy_model as M
from lazy_model import FQ, FR, P, R, Interval, Iv
from ntt_pass_model import NTT_CHAINS

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "collaborative-zksnark_amd", "csrc")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def hexes(body):
    return [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]+)u", body)]


# ------------------------------------------------------------------------------------------------------------------ limb tables
def fq_tables():
    """every `u32 fqu_<K>p[_suffix](int i)` table of fqu.h: name -> (K, U, limbs); U from the comment on its line, else 1"""
    out = {}
    for m in re.finditer(r"u32 (fqu_(\d+)p\w*)\(int i\) \{([^\n]*)\n\s*constexpr u32 m\[14\] = \{([^}]*)\}", src("fqu.h")):
        u = re.search(r">= (\d+) \* 2\^28", m.group(3))
        out[m.group(1)] = (int(m.group(2)), int(u.group(1)) if u else 1, hexes(m.group(4)))
    return out


def fr_tables():
    return {(int(k), int(u)): hexes(body) for k, u, body in
            re.findall(r"struct FruC<(\d+), (\d+)> \{[^\n]*constexpr u32 m\[9\] = \{([^}]*)\}", src("fru_constants.inc"))}


def test_every_fq_limb_table_is_K_p_with_limbs_above_U():
    t = fq_tables()
    assert set(t) == {"fqu_4p", "fqu_8p", "fqu_16p", "fqu_8p_wide", "fqu_8p_u2", "fqu_16p_u5", "fqu_16p_u4", "fqu_256p", "fqu_128p", "fqu_64p",
                      "fqu_64p_u3", "fqu_32p", "fqu_512p_u5"}
    for name, (K, U, l) in t.items():
        assert len(l) == 14 and all(x < 1 << 32 for x in l), name
        assert FQ.value(l) == K * P, f"{name}: sum L_i 2^(28 i) != {K} p"
        assert all(x >= U << 28 for x in l[:13]), f"{name}: a limb below {U} * 2^28"
        assert l == FQ.table(K, U), name
    assert t["fqu_8p_wide"][1] == 3 and t["fqu_16p_u5"][1] == 5 and t["fqu_512p_u5"][1] == 5 and t["fqu_64p_u3"][1] == 3


def test_every_fr_limb_table_is_K_r_with_limbs_above_U():
    t = fr_tables()
    assert set(t) == {(1 << lg, u) for lg in range(1, 9) for u in (1, 2)}
    for (K, U), l in t.items():
        assert len(l) == 9 and all(x < 1 << 32 for x in l), (K, U)
        assert FR.value(l) == K * R, (K, U)
        assert all(x >= U << 29 for x in l[:8]), (K, U)
        assert l[8] == (K * R >> 232) - U and l == FR.table(K, U), (K, U)


def _one_table(text, decl, n):
    m = re.search(re.escape(decl) + r"[^;]*?constexpr u32 m\[%d\] = \{([^}]*)\}" % n, text, re.S)
    assert m, decl
    return hexes(m.group(1))


def test_named_constants_equal_their_definitions():
    fqu, fru, te = src("fqu.h"), src("fru_constants.inc"), src("te_constants.inc")
    assert _one_table(fqu, "u32 fqu_p(int i)", 14) == FQ.digits(P)
    assert _one_table(fqu, "FqU fqu_one()", 14) == FQ.digits((1 << 392) % P)
    k_to_u = _one_table(fqu, "Fq fqu_k_to_u()", 12)
    assert sum(x << (32 * i) for i, x in enumerate(k_to_u)) == (1 << 392) % P
    m = re.search(r"Fq fqu_k_from_u\(\) \{[^}]*r\.l\[(\d+)\] = 0x([0-9a-f]+)u;", fqu, re.S)
    k_from_u = int(m.group(2), 16) << (32 * int(m.group(1)))
    assert k_from_u == 1 << 376 and k_from_u % P == pow(1 << 384, 2, P) * pow(1 << 392, -1, P) % P      # R^2 / R'
    assert _one_table(fru, "u32 fru_r(int i)", 9) == FR.digits(R)
    assert _one_table(fru, "u32 fru_one(int i)", 9) == FR.digits((1 << 261) % R)
    k32 = _one_table(fru, "u32 fru_k32(int i)", 8)
    assert sum(x << (32 * i) for i, x in enumerate(k32)) == (32 << 256) % R
    assert int(re.search(r"FRU_R_TOP = (\d+)u", fru).group(1)) == R >> 232 == M.FRU_R_TOP
    assert P % (1 << 28) == 1 and R % (1 << 29) == 1            # what makes the quotient digit -acc and the filters one compare
    # twisted Edwards constants: the definition chain of te_constants.inc
    assert M.TE_S * M.TE_S % P == 3 and M.TE_F * M.TE_F % P == -(M.TE_A + 2) * M.TE_S ** 3 % P
    assert int(re.search(r"// D = (\d+)", te).group(1)) == M.TE_D and int(re.search(r"// s = (\d+)", te).group(1)) == M.TE_S
    two_d = hexes(re.search(r"#define TE_2D_U \{([^}]*)\}", te).group(1))
    inv_d = hexes(re.search(r"#define TE_INV_D_U \{([^}]*)\}", te).group(1))
    assert two_d == FQ.digits(2 * M.TE_D * FQ.one % P) and inv_d == FQ.digits(pow(M.TE_D, -1, P) * FQ.one % P)
    for name, v in (("TE_S_S", M.TE_S), ("TE_F_S", M.TE_F), ("TE_2D_S", 2 * M.TE_D), ("TE_S_INV_S", pow(M.TE_S, -1, P))):
        ws = hexes(re.search(r"#define %s \{([^}]*)\}" % name, te).group(1))
        assert sum(x << (32 * i) for i, x in enumerate(ws)) == v * (1 << 384) % P, name


# --------------------------------------------------------------------------------------------- the model against itself
def test_column_loop_equals_the_closed_montgomery_formula():
    """two independent statements of the multiply (column sums / one division) agree limb for limb at the edges"""
    rng = random.Random(1)
    C = M.Concrete(FQ)
    ops = M.fam_largest(FQ, 1 << 30, 128) + M.fam_patterns(FQ, 1 << 30, 128) + M.fam_special(FQ, 128, 6) + M.fam_random(FQ, 1 << 30, 128, rng, 24)
    pairs = [(a, rng.choice(ops)) for a in ops] + M.quotient_pairs(FQ, 128, rng) + M.column_pairs(FQ, 1 << 30, 1 << 30, 128, 128)
    for a, b in pairs:
        assert C.mul(a, b) == FQ.digits(FQ.mont_exact(FQ.value(a) * FQ.value(b)))
        assert C.sqr(a) == FQ.digits(FQ.mont_exact(FQ.value(a) ** 2))
    n = M.fam_random(FQ, 1 << 28, 128, rng, 8)                 # normalised factors: limb products < 2^58
    for a, b in pairs[:40]:
        c, d, e = rng.choice(n), rng.choice(n), rng.choice(ops)
        want = FQ.mont_exact(FQ.value(a) * FQ.value(c) + FQ.value(b) * FQ.value(d))
        assert C.mul_add(a, c, b, d) == FQ.digits(want)
        assert C.mul_add_hi(a, c, b, d, e) == FQ.digits(FQ.mont_exact(FQ.value(a) * FQ.value(c) + FQ.value(b) * FQ.value(d) + (FQ.value(e) << 392)))
    CR = M.Concrete(FR)
    lazy = M.fam_largest(FR, int(2 ** 31.4), 437) + M.fam_random(FR, int(2 ** 31.4), 437, rng, 16)
    for a in lazy:
        b = FR.digits(rng.randrange(2 * R))
        assert CR.mul(a, b) == FR.digits(FR.mont_exact(FR.value(a) * FR.value(b)))


def test_capacity_checker_rejects_what_the_headers_exclude():
    C = M.Concrete(FQ)
    big = [(1 << 32) - 1] * 14
    with pytest.raises(M.ContractError):
        C.mul(big, big)                                        # 14 x 2^64 in one column
    with pytest.raises(M.ContractError):
        C.lin([], 16, 5, [(5, FQ.digits(4 * P))])              # fqu_neg5<false> of a value above 3.2 p: the top limb goes negative
    with pytest.raises(M.ContractError):
        C.lin([(1, [0] * 14)], 4, 1, [(1, [1 << 29] * 14)])    # fqu_sub_lazy<4> of a subtrahend limb above 2^28 + digit


# ------------------------------------------------------------------------------------------------------------ interval closure
MULOUT = Q(101, 100)        # "a multiply returns a value < 1.01 p with normalised limbs"


def fq(hi, lo=0):
    return Interval(FQ).normalised(lo, hi)


def lazy_neg(B):
    """the lazy 4 p - y of a negated table point (msm_acc.h): y canonical"""
    return B.lin([], 4, 1, [(1, B.normalised(0, 1))])


def below(iv, hi):
    return iv.hi <= hi and iv.limb <= FQ.mask


@pytest.mark.parametrize("neg", [False, True])
@pytest.mark.parametrize("first", [False, True])
def test_closure_fqu_xyzz_acc_mixed(neg, first):
    """accumulator x < 9.5 p, y < 5.5 p normalised, zz, zzz multiply outputs (first addition: x = qx, y <= 4 p, zz = zzz = R')"""
    B = Interval(FQ)
    acc = (fq(1), fq(4), fq(1), fq(1)) if first else (fq(Q(19, 2)), fq(Q(11, 2)), fq(MULOUT), fq(MULOUT))
    x, y, zz, zzz = M.fqu_xyzz_acc_mixed(B, *acc, fq(1), lazy_neg(B) if neg else fq(1))
    assert below(x, Q(19, 2)) and below(y, MULOUT) and below(zz, MULOUT) and below(zzz, MULOUT)


@pytest.mark.parametrize("ya, yb", [(MULOUT, MULOUT), (4, 4)])
def test_closure_xyzzu_add_and_double(ya, yb):
    """x < 9.5 p normalised; y, zz, zzz multiply outputs -- and y <= 4 p, what k_accumulate_u stores for a bucket that holds one
    negated point (fqu_normalize(4 p - y))"""
    B = Interval(FQ)
    a, b = (fq(Q(19, 2)), fq(ya), fq(MULOUT), fq(MULOUT)), (fq(Q(19, 2)), fq(yb), fq(MULOUT), fq(MULOUT))
    for out in (M.xyzzu_add(B, a, b), M.xyzzu_double(B, a)):
        x, y, zz, zzz = out
        assert below(x, Q(19, 2)) and below(y, MULOUT) and below(zz, MULOUT) and below(zzz, MULOUT)


def te_niels_iv(B, neg):
    ym, yp, k2 = fq(1), fq(1), fq(1)
    return M.te_negate_niels(B, ym, yp, k2) if neg else (ym, yp, k2)


@pytest.mark.parametrize("neg", [False, True])
def test_closure_te_formulas(neg):
    """te.h: TEU coordinates are multiply outputs except after teu_from_niels (x < 5 p, y < 2 p, z = 2); every formula accepts either
    and returns multiply outputs"""
    B = Interval(FQ)
    n = te_niels_iv(B, neg)
    f = M.teu_from_niels(B, *n)
    assert below(f[0], 5) and below(f[1], 2) and below(f[2], 2) and below(f[3], MULOUT)
    m = (fq(MULOUT),) * 4
    for a in (f, m):
        for out in [M.teu_madd(B, a, *n), M.teu_double(B, a)] + [M.teu_add(B, a, b) for b in (f, m)]:
            assert all(below(c, MULOUT) for c in out)


def test_closure_fq2u_products():
    B = Interval(FQ, "g2")
    a = (fq(Q(319, 100)), fq(Q(319, 100)))
    for out in (M.fq2u_mul(B, a, a), M.fq2u_mul_n5(B, a, a, M.neg5(B, a[1], False))):
        assert all(c.limb <= FQ.mask for c in out)
    h = (fq(131), fq(131))                                     # fq2u_sqr's operand in the mixed addition: "H in (43, 131)"
    s = M.fq2u_sqr(B, h)
    assert below(s[1], 3) and s[0].limb <= FQ.mask             # "c1 = 2 v2 < 3 p"
    assert below(M.neg5(B, fq(Q(319, 100)), False), 16) and below(M.neg5(B, fq(102), True), 512)
    with pytest.raises(M.ContractError):
        M.neg5(B, fq(Q(16, 5)), False)                         # K = 16: 5 x the top limb of a value just below 3.2 p exceeds the top limb of 16 p


@pytest.mark.parametrize("neg", [False, True])
@pytest.mark.parametrize("first", [False, True])
def test_closure_fq2u_xyzz_acc_mixed(neg, first):
    """the bounds of fq2u_xyzz_acc_mixed's own comment: X < 85 p, Y < 36 p, multiply outputs < 3 p, H in (43, 131) p, r < 67 p.  (The
    section header of fqu.h quotes Y < 49 p, H < 145 p, r < 81 p: loose upper bounds of the same analysis, said so there.)"""
    B = Interval(FQ, "g2")
    two = lambda hi: (fq(hi), fq(hi))
    acc = (two(1), two(4), two(1), two(1)) if first else (two(85), two(36), two(3), two(3))
    qy = (lazy_neg(B), lazy_neg(B)) if neg else two(1)
    x, y, zz, zzz = M.fq2u_xyzz_acc_mixed(B, *acc, two(1), qy)
    for c in range(2):
        assert below(x[c], 85) and below(y[c], 36) and below(zz[c], 3) and below(zzz[c], 3)
        assert B.trace["pp"][c].hi <= 131 and B.trace["pp"][c].lo >= 43 and B.trace["r"][c].hi <= 67      # "H in (43, 131), r < 67"


def test_closure_lane_pair_reduction():
    """fq2pu.h: inputs x < 100, y < 36, zz, zzz < 3.2 (k_accumulate_u2's buckets); sums x < 9.2, the rest < 1.2"""
    B = Interval(FQ, "g2")
    two = lambda hi: (fq(hi), fq(hi))
    big = (two(100), two(36), two(Q(319, 100)), two(Q(319, 100)))
    small = (two(Q(46, 5)), two(Q(6, 5)), two(Q(6, 5)), two(Q(6, 5)))
    outs = [M.xyzzu2_add(B, a, b) for a in (big, small) for b in (big, small)] + [M.xyzzu2_double(B, a) for a in (big, small)]
    for x, y, zz, zzz in outs:
        for c in range(2):
            assert below(x[c], Q(46, 5)) and below(y[c], Q(6, 5)) and below(zz[c], Q(6, 5)) and below(zzz[c], Q(6, 5))


@pytest.mark.parametrize("neg", [False, True])
def test_closure_xyzzu2_acc_mixed(neg):
    """fq2pu.h: ax < 9.2, ay < 4, azz, azzz < 3.2; qx canonical, qy canonical or the lazy 4 p - y"""
    B = Interval(FQ, "g2")
    two = lambda hi: (fq(hi), fq(hi))
    qy = (lazy_neg(B), lazy_neg(B)) if neg else two(1)
    x, y, zz, zzz = M.xyzzu2_acc_mixed(B, two(Q(46, 5)), two(4), two(Q(319, 100)), two(Q(319, 100)), two(1), qy)
    for c in range(2):
        assert below(x[c], Q(46, 5)) and below(y[c], 4) and below(zz[c], Q(319, 100)) and below(zzz[c], Q(319, 100))


# the steps ntt_pass.hip instantiates: (kind, KB) per pass shape, W = 1 (canonical inputs) and W = 2 (scratch values < 2 r)
# (NTT_CHAINS lives in tests/ntt_pass_model.py, the one table: tests/test_ntt_pass_cpu.py holds it to the kernels' instantiations)


@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("K", [5, 6, 7])
@pytest.mark.parametrize("last", [False, True])
def test_closure_ntt_butterflies(K, W, last):
    """ntt_pass.hip: inputs normalised and <= 1.003 r (W = 1) or < 2 r (W = 2); every fru_sub<K, U> finds its subtrahend's limbs below
    U 2^29 and its value below K r, every fru_mul its lazy operand below 2^261 with limbs < 2^31.4 and a canonical twiddle, and what
    leaves the pass is normalised and below 2^261 = what fru_canon accepts"""
    B = Interval(FR)
    tw = B.normalised(0, 1)
    bound = Q(1003, 1000) if W == 1 else Q(2)
    x = [B.normalised(0, bound) for _ in range(8)]
    chain = NTT_CHAINS[K]
    for step, (kind, kb) in enumerate(chain):
        kb *= W
        assert bound <= Q(kb, 2) + Q(1, 10)                    # "real inputs <= KB / 2 + 0.1"
        final = last and step == len(chain) - 1
        if kind == "radix8":
            (M.radix8_last if final else M.radix8)(B, kb, x, tw)
            bound = 6 * kb + Q(1, 10) if final else 8 * bound  # "x1 = x0 - x1 + 4 KB r < 6 KB + 0.1" / "a step of m stages multiplies the bound by 2^m"
        else:
            f = M.radix4_last if final else M.radix4
            lo, hi = x[:4], x[4:]
            f(B, kb, lo, tw), f(B, kb, hi, tw)
            x = lo + hi
            bound = 3 * kb + Q(2, 10) if final else 4 * bound  # "x1 = s02 - x1 + 2 KB r < 3 KB + 0.2"
        # what the next step (or fru_canon) reads went through LDS as it is: normalised, below 2^261
        assert all(v.limb <= FR.mask and v.hi * R < 1 << 261 for v in x), (step, x)
        assert max(v.hi for v in x) <= bound, (step, x)


# --------------------------------------------------------------------------------------------------- exceptional-case filters
def window_in_source(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return tuple(int(g) for g in m.groups())


def residues_that_vanish(K, minuend, subtrahend):
    """H = minuend - subtrahend + K p with H == 0 mod p: minuend = c + i p, subtrahend = c + j p for one c in [0, p), so H = (K + i - j) p
    for every admissible i, j; p == 1 mod 2^28 makes the low 28 bits of H that multiplier"""
    imax, jmax = int(minuend.hi) if minuend.hi % 1 else int(minuend.hi) - 1, int(subtrahend.hi) if subtrahend.hi % 1 else int(subtrahend.hi) - 1
    hs = {K + i - j for i in range(imax + 1) for j in range(jmax + 1)}
    assert min(hs) > 0
    return {(h * P) & FQ.mask for h in hs}, hs


def test_filter_fqu_xyzz_acc_mixed_has_no_false_negative():
    lo, width = window_in_source(src("fqu.h"), r"\(\(pp\.l\[0\] & FQU_MASK\) - (\d+)u\) <= (\d+)u\) return false;")
    assert (lo, lo + width) == M.WINDOWS["fqu_xyzz_acc_mixed"]
    B = Interval(FQ)
    M.fqu_xyzz_acc_mixed(B, fq(Q(19, 2)), fq(Q(11, 2)), fq(MULOUT), fq(MULOUT), fq(1), fq(1))
    lows, hs = residues_that_vanish(16, B.trace["u2"], B.trace["ax"])
    assert hs == set(range(7, 18)) and all(lo <= v <= lo + width for v in lows)


def test_filter_xyzzu_add_has_no_false_negative():
    lo, width = window_in_source(src("fqu.h"), r"\(\(pp\.l\[0\] & FQU_MASK\) - (\d+)u\) <= (\d+)u\) \{\s*a = xyzzu_add_slow")
    assert (lo, lo + width) == M.WINDOWS["xyzzu_add"]
    B = Interval(FQ)
    a = (fq(Q(19, 2)), fq(4), fq(MULOUT), fq(MULOUT))
    M.xyzzu_add(B, a, a)
    lows, hs = residues_that_vanish(4, B.trace["u2"], B.trace["u1"])
    assert hs == {3, 4, 5} and all(lo <= v <= lo + width for v in lows)


def test_filter_fq2u_xyzz_acc_mixed_has_no_false_negative():
    lo, hi = window_in_source(src("fqu.h"), r"if \(fqu_low_in\(pp\.c0, (\d+), (\d+)\) && fqu_low_in\(pp\.c1, \1, \2\)\) return false;\s*const FqU n5zzz")
    assert (lo, hi) == M.WINDOWS["fq2u_xyzz_acc_mixed"]
    B = Interval(FQ, "g2")
    two = lambda h: (fq(h), fq(h))
    M.fq2u_xyzz_acc_mixed(B, two(85), two(36), two(3), two(3), two(1), two(1))
    for c in range(2):
        lows, hs = residues_that_vanish(128, B.trace["u2"][c], B.trace["ax"][c])
        assert min(hs) >= 44 and max(hs) <= 130 and all(lo <= v <= hi for v in lows)     # "j in (43, 145)"


def test_filters_of_the_lane_pair_forms_have_no_false_negative():
    txt = src("fq2pu.h")
    lo, width = window_in_source(txt, r"pair_all\(\(pp\.l\[0\] - (\d+)u\) <= (\d+)u\)\) \{\s*a = xyzzu2_add_slow")
    assert (lo, lo + width) == M.WINDOWS["xyzzu2_add"]
    B = Interval(FQ, "g2")
    two = lambda h: (fq(h), fq(h))
    big = (two(100), two(36), two(Q(319, 100)), two(Q(319, 100)))
    M.xyzzu2_add(B, big, big)
    for c in range(2):
        lows, hs = residues_that_vanish(4, B.trace["u2"][c], B.trace["u1"][c])
        assert hs == {3, 4, 5} and all(lo <= v <= lo + width for v in lows)
    lo, width = window_in_source(txt, r"pair_all\(\(pp\.l\[0\] - (\d+)u\) <= (\d+)u\)\) return false;")
    assert (lo, lo + width) == M.WINDOWS["xyzzu2_acc_mixed"]
    B = Interval(FQ, "g2")
    M.xyzzu2_acc_mixed(B, two(Q(46, 5)), two(4), two(Q(319, 100)), two(Q(319, 100)), two(1), two(1))
    for c in range(2):
        lows, hs = residues_that_vanish(16, B.trace["u2"][c], B.trace["ax"][c])
        assert hs == set(range(7, 18)) and all(lo <= v <= lo + width for v in lows)
    (ub,) = window_in_source(txt, r"pair_all\(u\.l\[0\] < (\d+)u\)\) \{\s*a = xyzzu2_double_slow")
    assert (0, ub - 1) == M.WINDOWS["xyzzu2_double"] and ub >= 2 * 36      # U = 2 Y1 < 72 p is 0 mod p only as j p, j < 72


# ---------------------------------------------------------------------------------------------------- fru_reduce_2r / fru_canon
def fru_canon_cases():
    """normalised 9-limb values: q r - 1, q r, q r + 1 for q in 0..438, 2^261 - 1, both sides of every step of the quotient estimate"""
    vs = [v for q in range(439) for v in (q * R - 1, q * R, q * R + 1) if 0 <= v < 1 << 261] + [(1 << 261) - 1]
    for t in M.fru_quotient_steps():
        vs += [t << 232, ((t + 1) << 232) - 1]
    return [FR.digits(v) for v in vs]


def test_fru_canon_quotient_estimate_and_result():
    cases = fru_canon_cases()
    assert len(cases) > 3 * 438 and all(max(l) <= FR.mask for l in cases)
    short = 0
    for l in cases:
        q, t = M.fru_reduce_2r(l)                  # raises unless q is floor(a / r) or one less
        short += q == FR.value(l) // R - 1
        assert max(t) <= FR.mask and FR.value(t) < 2 * R
        assert M.fru_canon(l) == FR.value(l) % R
    assert short > 0                               # the conditional subtraction is needed: some case really falls one short
