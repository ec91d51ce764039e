"""The signed-column ("subtractive") Montgomery reduction of csrc/fqu.h, checked without a GPU.

Three things are stated here on big integers (tests/subtractive_model.py, tests/lazy_model.py):

  * the subtractive column loop, run in 64-bit two's complement, returns the SAME limbs as the additive loop -- including the operand
    pairs whose quotient is zero, where the additive form adds no p (a mutation that drops the q != 0 condition fails);
  * every call site that the headers route through an `_s` multiply keeps every column inside the signed range, and below the
    contract's 2^63 - 2^60; the sites left on the additive loop are listed with the bound that excludes them;
  * the headers call the `_s` forms at exactly the sites this table says (read from the source text).

The kernels themselves are held to the same model by tests/test_fqu_subtractive.py.
"""
import os
import random
import re
from fractions import Fraction as Q

import pytest

import lazy_model as M
import subtractive_model as SM
from lazy_model import FQ, P, Interval

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "collaborative-zksnark_amd", "csrc")
MULOUT = Q(101, 100)
LIMIT = SM.I63 - (1 << 60)          # the contract: column sum + carry (+ e) below 2^63 - 2^60


def fq(hi, lo=0):
    return Interval(FQ).normalised(lo, hi)


def two(hi):
    return fq(hi), fq(hi)


def lazy_neg(B):
    return B.lin([], 4, 1, [(1, B.normalised(0, 1))])


# ------------------------------------------------------------------------------------------------------------- limb equality
operand_sets = SM.operand_sets


def test_operand_sets_cover_the_quotient_shapes():
    seen = set()
    for label, a, b in operand_sets():
        q = FQ.value(a) * FQ.value(b) * pow(P, -1, FQ.radix) % FQ.radix
        d = FQ.digits(q) if q >> (28 * 13) < 1 << 28 else None
        assert d is not None
        if q == 0:
            seen.add("zero")
        elif all(x == FQ.mask for x in d):
            seen.add("ones")
        elif all(x == 0 for x in d[:13]):
            seen.add("top")
        elif all(x == 0 for x in d[1:]):
            seen.add("low")
    assert seen == {"zero", "ones", "top", "low"}


def test_subtractive_loop_equals_the_additive_loop_limb_for_limb():
    C = M.Concrete(FQ)
    sets = operand_sets()
    for label, a, b in sets:
        want = C.mul(a, b)
        assert want == FQ.digits(FQ.mont_exact(FQ.value(a) * FQ.value(b)))
        assert SM.sub_mul_sum([(a, b)]) == want, label
        if all(x < 1 << 29 for x in a):
            assert SM.sub_mul_sum([], squares=[a]) == C.sqr(a), label
    rng = random.Random(21)
    nrm = M.fam_largest(FQ, 1 << 28, 9) + M.fam_random(FQ, 1 << 28, 9, rng, 12)
    lazy_e = M.fam_largest(FQ, 1 << 32, 128) + M.fam_random(FQ, 1 << 30, 128, rng, 12)
    for label, a, b in sets[::3]:
        if max(b) > FQ.mask:
            continue                                           # the fused forms want one normalised factor per product
        c, d, e = rng.choice(sets)[1], rng.choice(nrm), rng.choice(lazy_e)
        f, g, h = rng.choice(nrm), rng.choice(nrm), rng.choice(nrm)
        assert SM.sub_mul_sum([(a, b), (c, d)]) == C.mul_add(a, b, c, d), label
        assert SM.sub_mul_sum([(a, b), (c, d)], e=e) == C.mul_add_hi(a, b, c, d, e), label
        assert SM.sub_mul_sum([(a, b)], e=e) == C.mul_hi(a, b, e), label
        if max(a) <= FQ.mask << 1 and max(c) <= FQ.mask << 1:
            assert SM.sub_mul_sum([(a, b), (c, d), (f, g), (c, h)]) == C.mul_add4(a, b, c, d, f, g, c, h), label


def test_dropping_the_quotient_flag_is_caught():
    """the mutation `always_top` (top digit always t_13 - 2^28) returns p too much exactly where the quotient is zero"""
    C = M.Concrete(FQ)
    zeros = [(a, b) for label, a, b in operand_sets() if label == "q-zero"]
    assert len(zeros) >= 4
    for a, b in zeros:
        want = C.mul(a, b)
        assert SM.sub_mul_sum([(a, b)]) == want
        got = SM.sub_mul_sum([(a, b)], always_top=True)
        assert got != want and FQ.value(got) == FQ.value(want) + P
    others = [(a, b) for label, a, b in operand_sets() if label == "q-ones"]
    assert all(SM.sub_mul_sum([x], always_top=True) == C.mul(*x) for x in others)


def test_a_column_outside_the_signed_range_is_what_breaks_the_form():
    """the reason for the contract: with both operands at 2^30 per limb a column passes 2^63 and the arithmetic shift misreads it"""
    a = [(1 << 30) - 1] * 13 + [0]
    assert SM.sub_mul_sum([(a, a)]) != M.Concrete(FQ).mul(a, a)
    lo, hi = SM.signed_columns([(1, (1 << 30) - 1, (1 << 30) - 1)])
    assert hi >= SM.I63 and lo > -SM.I63


# ---------------------------------------------------------------------------------------------------------- call-site proofs
# formula -> the multiplies of its lazy_model statement, in call order: (name in the header, True if the header uses the `_s` form)
SITES = {
    "teu_from_niels": [("t", True)],
    "teu_madd": [("A", True), ("B", True), ("C", True), ("E F", False), ("G H", True), ("F G", False), ("E H", True)],
    "teu_add": [("A", False), ("B", True), ("T1 T2", True), ("C", True), ("Dh", True), ("E F", False), ("G H", True), ("F G", False), ("E H", True)],
    "teu_double": [("A", True), ("B", True), ("Cz", True), ("S", True), ("E F", False), ("G H", True), ("F G", True), ("E H", False)],
    "fqu_xyzz_acc_mixed": [("u2", True), ("s2", True), ("p2", False), ("zz", True), ("p3", True), ("zzz", True), ("qv", True), ("t", False), ("y", True)],
    "xyzzu_add": [(n, True) for n in ("u1", "u2", "s1", "s2", "p2", "p3", "qv", "zz ab", "zz", "zzz ab", "zzz", "t", "y")],
    "xyzzu_double": [("v", True), ("w", True), ("s", True), ("xx", True), ("mm", False), ("y3", True), ("zz", True), ("zzz", True)],
    "fq2u_mul": [("v0", True), ("v1", True), ("m", True)],
    "fq2u_sqr": [("v", True), ("v2", True)],
    "fq2u_mul_n5": [("c0", True), ("c1", True)],
    # pp (2), r (2), p2 = fq2u_sqr (2), zz, p3, zzz, qv = fq2u_mul_n5 (2 each), v2, X3.c0 (mul_hi), Y3 (2 x mul_add4); the two
    # B.mul_add of the model's own trace (u2) come after pp
    "fq2u_xyzz_acc_mixed": [(n, True) for n in ("pp0", "pp1", "u2 trace", "u2 trace", "r0", "r1", "p2 v", "p2 v2", "zz0", "zz1", "p30", "p31", "zzz0", "zzz1", "qv0",
                                                 "qv1", "v2", "x3", "y30", "y31")],
    "xyzzu2_add": [("p2_mul", True)] * 24 + [("y", True)] * 2,
    "xyzzu2_double": [("p2_mul", True)] * 10 + [("y3", True)] * 2 + [("p2_mul", True)] * 4,
    "xyzzu2_acc_mixed": [("p2_mul", True)] * 16 + [("y", True)] * 2,
}


def runs(name):
    """every (discipline, inputs) the closure proofs of tests/test_lazy_arith_cpu.py run the formula on"""
    if name in ("teu_from_niels", "teu_madd", "teu_add", "teu_double"):
        for neg in (False, True):
            B = SM.SiteRecorder(FQ)
            n = (fq(1), fq(1), fq(1))
            n = M.te_negate_niels(B, *n) if neg else n
            f = M.teu_from_niels(B, *n)
            if name == "teu_from_niels":
                yield B
                continue
            m = (fq(MULOUT),) * 4
            for a in (f, m):
                for b in ((f, m) if name == "teu_add" else (None,)):
                    B.sites.clear()
                    {"teu_madd": lambda: M.teu_madd(B, a, *n), "teu_double": lambda: M.teu_double(B, a), "teu_add": lambda: M.teu_add(B, a, b)}[name]()
                    yield B
    elif name == "fqu_xyzz_acc_mixed":
        for neg in (False, True):
            for first in (False, True):
                B = SM.SiteRecorder(FQ)
                acc = (fq(1), fq(4), fq(1), fq(1)) if first else (fq(Q(19, 2)), fq(Q(11, 2)), fq(MULOUT), fq(MULOUT))
                M.fqu_xyzz_acc_mixed(B, *acc, fq(1), lazy_neg(B) if neg else fq(1))
                yield B
    elif name in ("xyzzu_add", "xyzzu_double"):
        for ya, yb in ((MULOUT, MULOUT), (4, 4)):
            B = SM.SiteRecorder(FQ)
            a, b = (fq(Q(19, 2)), fq(ya), fq(MULOUT), fq(MULOUT)), (fq(Q(19, 2)), fq(yb), fq(MULOUT), fq(MULOUT))
            M.xyzzu_add(B, a, b) if name == "xyzzu_add" else M.xyzzu_double(B, a)
            yield B
    elif name in ("fq2u_mul", "fq2u_mul_n5", "fq2u_sqr"):
        B = SM.SiteRecorder(FQ, "g2")
        a = two(Q(319, 100))
        if name == "fq2u_mul":
            M.fq2u_mul(B, a, a)
        elif name == "fq2u_mul_n5":
            M.fq2u_mul_n5(B, a, a, M.neg5(B, a[1], False))
        else:
            M.fq2u_sqr(B, two(131))
        yield B
    elif name == "fq2u_xyzz_acc_mixed":
        for neg in (False, True):
            for first in (False, True):
                B = SM.SiteRecorder(FQ, "g2")
                acc = (two(1), two(4), two(1), two(1)) if first else (two(85), two(36), two(3), two(3))
                M.fq2u_xyzz_acc_mixed(B, *acc, two(1), (lazy_neg(B), lazy_neg(B)) if neg else two(1))
                yield B
    elif name in ("xyzzu2_add", "xyzzu2_double"):
        big = (two(100), two(36), two(Q(319, 100)), two(Q(319, 100)))
        small = (two(Q(46, 5)), two(Q(6, 5)), two(Q(6, 5)), two(Q(6, 5)))
        for a in (big, small):
            for b in ((big, small) if name == "xyzzu2_add" else (None,)):
                B = SM.SiteRecorder(FQ, "g2")
                M.xyzzu2_add(B, a, b) if name == "xyzzu2_add" else M.xyzzu2_double(B, a)
                yield B
    elif name == "xyzzu2_acc_mixed":
        for neg in (False, True):
            B = SM.SiteRecorder(FQ, "g2")
            M.xyzzu2_acc_mixed(B, two(Q(46, 5)), two(4), two(Q(319, 100)), two(Q(319, 100)), two(1), (lazy_neg(B), lazy_neg(B)) if neg else two(1))
            yield B
    else:
        raise KeyError(name)


# the sites left additive, with the highest column the interval model gives them (log2, rounded down to 0.1): all at or above the contract
EXCLUDED = {("teu_madd", "E F"): 63.2, ("teu_madd", "F G"): 63.3, ("teu_add", "A"): 62.8, ("teu_add", "E F"): 63.2, ("teu_add", "F G"): 63.3,
            ("teu_double", "E F"): 63.7, ("teu_double", "E H"): 63.3, ("fqu_xyzz_acc_mixed", "p2"): 62.9, ("fqu_xyzz_acc_mixed", "t"): 62.8,
            ("xyzzu_double", "mm"): 62.9}


@pytest.mark.parametrize("name", sorted(SITES))
def test_every_signed_call_site_keeps_its_columns_in_range(name):
    table = SITES[name]
    count = 0
    for B in runs(name):
        count += 1
        assert len(B.sites) == len(table), (name, len(B.sites))
        for (site, signed), (_, lo, hi) in zip(table, B.sites):
            if signed:
                assert -SM.I63 <= lo and hi < LIMIT, f"{name} / {site}: a column can reach {hi:#x} (contract {LIMIT:#x})"
            else:
                assert hi >= LIMIT, f"{name} / {site}: qualifies for the signed form (highest column {hi:#x}) but is listed additive"
                assert hi >= 2 ** EXCLUDED[(name, site)], (name, site)
    assert count >= 1
    assert {s for n, s in EXCLUDED if n == name} == {s for s, signed in table if not signed}


def test_teu_add_kt_sites():
    """teu_add_kt = teu_add with C = T1 (2 D T2) as ONE product of two normalised values; teu_kt a normalised value times the constant 2 D"""
    for lo, hi in (SM.signed_columns([(1, FQ.mask, FQ.mask)]),):
        assert -SM.I63 <= lo and hi < LIMIT


def test_the_negative_part_of_a_column_is_bounded_as_the_header_says():
    lo, _ = SM.signed_columns([(1, 0, 0)])
    assert -13 * (1 << 56) < lo < 0


# ------------------------------------------------------------------------------------------------------ the source agrees
def body(text, decl):
    i = text.index(decl)
    j = text.index("\n}\n", i)
    return text[i:j]


def calls(text):
    """the multiplies of a function body in source order: True for an `_s` form"""
    return [m.group(2) is not None for m in re.finditer(r"\bfqu_(mul_add4|mul_add_hi|mul_add|mul_hi|mul|sqr)(_s)?\(", text)]


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_headers_use_the_signed_form_at_exactly_the_listed_sites():
    fqu, te, p2 = src("fqu.h"), src("te.h"), src("fq2pu.h")
    fin = calls(body(te, "void teu_finish("))
    assert fin == [False, True, False, True]                                       # E F, G H, F G, E H
    want = lambda name: [s for _, s in SITES[name]]
    assert calls(body(te, "void teu_madd(")) + fin == want("teu_madd")
    add = calls(body(te, "void teu_add("))
    assert [add[0], add[1], add[3], add[2], add[4]] + fin == want("teu_add")     # C = mul(mul(t1, t2), 2 D): the outer call comes first in the text
    assert calls(body(te, "void teu_add_kt(")) == [False, True, True, True]
    assert calls(body(te, "FqU teu_kt(") + "\n") == [True] or "fqu_mul_s(b.t, te_2d_u())" in te
    assert calls(body(te, "void teu_double(")) == want("teu_double")
    assert calls(body(te, "TEU teu_from_niels(")) == want("teu_from_niels")
    assert calls(body(fqu, "bool fqu_xyzz_acc_mixed(")) == want("fqu_xyzz_acc_mixed")
    xa = calls(body(fqu, "void xyzzu_add("))
    assert len(xa) == 13 and all(xa)
    assert calls(body(fqu, "void xyzzu_double(")) == want("xyzzu_double")
    assert calls(body(fqu, "Fq2U fq2u_mul(")) == want("fq2u_mul") and calls(body(fqu, "Fq2U fq2u_sqr(")) == want("fq2u_sqr")
    assert calls(body(fqu, "Fq2U fq2u_mul_n5(")) == want("fq2u_mul_n5")
    g2 = body(fqu, "bool fq2u_xyzz_acc_mixed(")
    default_branch = g2[:g2.index("#else")] + g2[g2.index("#endif"):]
    assert all(calls(default_branch)) and len(calls(default_branch)) == 4 + 1 + 1 + 2
    assert "return fqu_mul_add_s(a.own, b.x, a.oth, b.y)" in p2 and p2.count("fqu_mul_add4_s(") == 3 and "fqu_mul_add4(" not in p2
    # the accessor for p's negated limbs must not look like a K p table to tests/test_lazy_arith_cpu.py
    assert "u32 fqu_neg_p(int i)" in fqu and not re.search(r"u32 fqu_\d+p\w*\(int i\) \{ return 0u", fqu)
