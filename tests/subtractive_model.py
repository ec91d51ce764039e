"""Big-integer model of the SUBTRACTIVE column loop of csrc/fqu.h (the `_s` multiplies) -- TEST INFRASTRUCTURE ONLY.

The additive loop of lazy_model.Concrete.mul_sum adds m p with m = -T / p mod R'; this one subtracts q p with q = T / p mod R' and keeps the
column accumulator in 64-bit two's complement, exactly as the kernel's registers do:

    digit t_k = acc & MASK (p == 1 mod 2^28), columns subtract sum t_i p_(k - i) for the limbs p_1.. of p, acc >>= 28 arithmetically;
    the TOP digit is taken as t_13 - 2^28 when any digit is non-zero (q != 0): that adds p 2^392 to the numerator, i.e. the "+ p" the
    additive form returns for q != 0 -- and nothing when q == 0, where the additive form returns T / R' itself.

`signed_columns` is the interval side: the lowest and highest value any column can hold for operands inside given limb bounds.
"""
import random

from lazy_model import (FQ, P, U32, U64, Interval, column_pairs, fam_largest, fam_patterns, fam_random, fam_special, quotient_pairs)

I63 = 1 << 63


def wrap(v):
    """the value a 64-bit register holds, read as signed"""
    v &= U64 - 1
    return v - U64 if v >= I63 else v


def sub_mul_sum(pairs, e=None, squares=(), always_top=False, S=FQ, extremes=None):
    """result limbs of the subtractive loop; `always_top` is the MUTATION that drops the q != 0 condition.  `extremes`: a two-element list
    that receives the lowest and highest value a column held when it was carried out (as the register read it)"""
    n, w, mask = S.n, S.w, S.mask
    t, r, acc = [0] * n, [0] * n, 0
    if extremes is not None:
        extremes[:] = [0, 0]
    for k in range(2 * n - 1):
        i0 = 0 if k < n else k - n + 1
        i1 = k if k < n else n - 1
        for a, b in pairs:
            acc = wrap(acc + sum(a[i] * b[k - i] for i in range(i0, i1 + 1)))
        for a in squares:
            acc = wrap(acc + sum(a[i] * ((a[k - i] << 1) % U32) for i in range(i0, (k + 1) // 2)) + (a[k // 2] ** 2 if k % 2 == 0 else 0))
        acc = wrap(acc - sum(t[i] * S.modl[k - i] for i in range(i0, (k - 1 if k < n else n - 1) + 1)))
        if k < n:
            t[k] = acc & mask
            if k == n - 1:
                if always_top or any(t):
                    t[k] -= 1 << w                  # v_and_or with ~MASK, read as a negative multiplier
                acc = wrap(acc - t[k])              # the p_0 = 1 product of the top digit: leaves the low 28 bits zero, carries the + 1
        else:
            if e is not None:
                acc = wrap(acc + e[k - n])
            r[k - n] = acc & mask
        if extremes is not None:
            extremes[:] = [min(extremes[0], acc), max(extremes[1], acc)]
        acc >>= w                                   # arithmetic: Python's >> on a negative int floors
    r[n - 1] = acc % U32
    if e is not None:
        r[n - 1] = (r[n - 1] + e[n - 1]) % U32
    return r


def signed_columns(prods, e=None, S=FQ):
    """(lowest, highest) true column value over the whole loop, for prods = [(count, limb bound a, limb bound b)] (bounds inclusive) and an
    addend with limbs <= e.  Lowest: every product zero, every digit 2^w - 1.  Highest: every limb at its bound, every digit zero but the
    top one, which as t_13 - 2^w contributes up to 2^w p_j.  The two extremes are taken independently: a bound, not a tight one."""
    n, w, mask = S.n, S.w, S.mask
    lo_c = hi_c = 0
    lo = hi = 0
    for k in range(2 * n - 1):
        i0 = 0 if k < n else k - n + 1
        cab = (k if k < n else n - 1) - i0 + 1
        red = sum(mask * S.modl[k - i] for i in range(i0, (k - 1 if k < n else n - 1) + 1))
        col_lo = lo_c - red - (mask if k < n else 0)
        col_hi = hi_c + sum(cnt * cab * la * lb for cnt, la, lb in prods)
        if k == n - 1:
            col_hi += 1 << w                        # - (t_13 - 2^w) p_0
        if k >= n:
            col_hi += (1 << w) * S.modl[k - n + 1] + (e if e is not None else 0)
        lo, hi = min(lo, col_lo), max(hi, col_hi)
        lo_c, hi_c = col_lo >> w, col_hi >> w
    return lo, hi


def fits_signed(prods, e=None):
    lo, hi = signed_columns(prods, e)
    return -I63 <= lo and hi < I63


class SiteRecorder(Interval):
    """lazy_model's interval tracker, additionally recording for every multiply of a formula, in call order, the bounds of its columns
    under the signed loop: .sites = [(kind, lowest, highest)]"""

    def __init__(self, S, discipline="g1"):
        super().__init__(S, discipline)
        self.sites = []

    def _mul(self, prods, e=None):
        lo, hi = signed_columns([(c, a.lmax, b.lmax) for c, a, b in prods], e.lmax if e is not None else None)
        self.sites.append((len(prods), lo, hi))
        return super()._mul(prods, e)


# --------------------------------------------------------------------------------------------------------------------------------
# operand sets shared by the CPU and GPU tests
# --------------------------------------------------------------------------------------------------------------------------------
def operand_sets():
    """(label, a, b) for the plain multiply: lazy_model's edge generators at the three limb disciplines a signed site can see, the
    quotient pairs (digits all ones / all zero), only the top / only the low digit non-zero, every single column at its maximum"""
    rng = random.Random(20)
    out = []
    for cap_a, cap_b, va, vb in ((1 << 28, 1 << 28, 9, 9), (1 << 30, 1 << 28, 128, 9), (1 << 29, 1 << 29, 64, 64)):
        A = fam_largest(FQ, cap_a, va) + fam_patterns(FQ, cap_a, va) + fam_special(FQ, va, 4) + fam_random(FQ, cap_a, va, rng, 16)
        Bs = fam_largest(FQ, cap_b, vb) + fam_patterns(FQ, cap_b, vb) + fam_special(FQ, vb, 4) + fam_random(FQ, cap_b, vb, rng, 16)
        out += [("edge", a, rng.choice(Bs)) for a in A] + [("edge", rng.choice(A), b) for b in Bs]
        out += [("column", a, b) for a, b in column_pairs(FQ, cap_a, cap_b, va, vb)]
    ones, zero = quotient_pairs(FQ, 9, rng)
    out += [("q-ones", *ones), ("q-zero", *zero), ("q-zero", zero[1], zero[0]), ("q-zero", [0] * 14, ones[0]), ("q-zero", ones[1], [0] * 14)]
    # lazy_model's "ones" pair has the ADDITIVE digits all ones (a b == p mod R': the subtracted quotient is 1); the subtracted digits
    # are all ones for a b == -p mod R'
    while True:
        a = rng.randrange(1, 9 * P, 2)
        b = (FQ.radix - P) * pow(a, -1, FQ.radix) % FQ.radix
        if b < 128 * P:
            out.append(("q-ones", FQ.digits(a), FQ.digits(b)))
            break
    one = FQ.digits(1)
    for _ in range(6):
        # a * 1 has quotient a p^-1 mod R': choose the quotient, get the operand.  Top digit only / low digit only / one digit each.
        for q in ((rng.randrange(1, 1 << 28)) << (28 * 13), rng.randrange(1, 1 << 28), 1 << (28 * 13), 1, (1 << 28) - 1, ((1 << 28) - 1) << (28 * 13)):
            a = q * P % FQ.radix
            if a < 9 * P:
                out.append(("q-digit", FQ.digits(a), one))
    return out


def extreme_pairs():
    """(a, b) that drive a column of the signed loop as low and as high as the contract allows.
    Lowest: a = R' - p, b = 1 -- the product is R' - p itself, every quotient digit is 2^28 - 1 and no operand product reaches the high
    columns, which then hold only the carry and -sum t_i p_j (the result is 1).
    Highest: fourteen products of a 2^30 - 1 limb with a 2^28 - 1 limb in one column, and thirteen of two limbs of 2^29.54 (a column within 5 % of the contract's 2^63 - 2^60)."""
    low = (FQ.digits(FQ.radix - P), FQ.digits(1))
    cap = 1 << 30
    high = ([cap - 1] * 13 + [0], [FQ.mask] * 13 + [0])
    mid = int(2 ** 29.54)
    return [low, (low[1], low[0]), high, (high[1], high[0]), ([mid - 1] * 13 + [0], [mid - 1] * 13 + [0])]
