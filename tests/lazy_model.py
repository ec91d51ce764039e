"""Big-integer model of the unsaturated ("lazy") Fq / Fr arithmetic of csrc/fqu.h, fru.h, te.h and fq2pu.h (TEST INFRASTRUCTURE ONLY).

Plain Python integers; imports nothing from the product.  Three layers:

  * exact references: the closed Montgomery formula (`mont_exact`), limb <-> integer maps, the K p / K r limb tables regenerated from
    their definition (`table`);
  * a CAPACITY CHECKER (`Concrete`): every primitive on concrete limb vectors, raising ContractError when a 64-bit column or a 32-bit
    limb expression would wrap -- it also returns the limbs the kernel must produce;
  * an INTERVAL TRACKER (`Interval`): the same primitives on (value bound in units of the modulus, limb bound) pairs, each asserting
    its documented precondition and returning its postcondition.

Every formula of the headers is restated ONCE, over an abstract backend, and runs on either: on intervals it proves closure of the
documented invariants, on concrete limbs it vets test inputs (and predicts the raw output limbs).
"""
from __future__ import annotations

from fractions import Fraction as Fr_

P = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
R = 8444461749428370424248824938781546531375899335154063827935233455917409239041
U32, U64 = 1 << 32, 1 << 64


class ContractError(AssertionError):
    pass


def need(cond, msg):
    if not cond:
        raise ContractError(msg)


class Sys:
    """A residue system: n limbs of w bits, Montgomery radix 2^(w n)."""

    def __init__(self, name, mod, w, n):
        self.name, self.mod, self.w, self.n = name, mod, w, n
        self.bits = w * n
        self.mask = (1 << w) - 1
        self.radix = 1 << self.bits
        self.one = self.radix % mod                  # the Montgomery one
        self.ninv = (-pow(mod, -1, self.radix)) % self.radix
        self.top_shift = w * (n - 1)
        self.modl = self.digits(mod)

    def value(self, l):
        assert len(l) == self.n
        return sum(int(x) << (self.w * i) for i, x in enumerate(l))

    def digits(self, v):
        """base-2^w digits, the top limb takes the rest"""
        assert v >= 0
        l = [(v >> (self.w * i)) & self.mask for i in range(self.n - 1)] + [v >> self.top_shift]
        need(l[-1] < U32, "top limb does not fit 32 bits")
        return l

    def mont_exact(self, T):
        """the value a product-scanning Montgomery reduction of T returns: (T + ((-T / mod) mod radix) mod) / radix, exactly"""
        m = (T * self.ninv) % self.radix
        q, rem = divmod(T + m * self.mod, self.radix)
        assert rem == 0
        return q

    def table(self, K, U):
        """K mod in redundant limb form: every limb but the top is the digit + U 2^w, borrowed from the limb above"""
        d = self.digits(K * self.mod)
        l = list(d)
        for i in range(self.n - 1):
            l[i] += U << self.w
            l[i + 1] -= U
        assert self.value(l) == K * self.mod and all(x >= 0 for x in l)
        return l


FQ = Sys("Fq", P, 28, 14)
FR = Sys("Fr", R, 29, 9)
FRU_R_TOP = R >> 232

# twisted Edwards form of G1 (csrc/te_constants.inc states the derivation): s^2 = 3, A = -3 / s, D = -(A - 2) / (A + 2), f^2 = -(A + 2) s^3
TE_S = 30567070899668889872121584789658882274245471728719284894883538395508419196346447682510590835309008936731240225793
TE_F = 202380648630189413781767775132768689582897972803719204311380468168466639537554822918624264483630724598885089179654
TE_A = (-3 * pow(TE_S, -1, P)) % P
TE_D = (-(TE_A - 2) * pow(TE_A + 2, -1, P)) % P

# the windows of the exceptional-case filters as the headers document them: name -> (lo, hi) on the low limb
WINDOWS = {"fqu_xyzz_acc_mixed": (6, 18), "xyzzu_add": (3, 5), "fq2u_xyzz_acc_mixed": (40, 150), "xyzzu2_add": (3, 5),
           "xyzzu2_acc_mixed": (6, 18), "xyzzu2_double": (0, 71)}


# --------------------------------------------------------------------------------------------------------------------------------
# capacity checker: concrete limbs
# --------------------------------------------------------------------------------------------------------------------------------
class Concrete:
    def __init__(self, S, windows=None):
        self.S = S
        self.windows = dict(WINDOWS if windows is None else windows)

    def const(self, limbs):
        return [int(x) for x in limbs]

    def _chk(self, a):
        need(len(a) == self.S.n and all(0 <= x < U32 for x in a), "operand limb outside 32 bits")

    def mul_sum(self, pairs, e=None, squares=()):
        """The column loop of fqu_mul / fqu_sqr / fqu_mul_add / fqu_mul_add4 / fru_mul stated plainly: column k holds the carry plus
        sum a_i b_(k-i) over every pair plus sum m_i mod_(k-i).  `squares`: operands multiplied with themselves through the doubled
        copy (fqu_sqr).  Raises when a column reaches 2^64 or a limb expression leaves 32 bits; returns the result limbs."""
        S, n, w = self.S, self.S.n, self.S.w
        for a, b in pairs:
            self._chk(a), self._chk(b)
        for a in squares:
            self._chk(a)
            need(all((x << 1) < U32 for x in a), "a << 1 wraps")
        if e is not None:
            self._chk(e)
        m, r, carry = [0] * n, [0] * n, 0
        for k in range(2 * n - 1):
            i0 = 0 if k < n else k - n + 1
            i1 = k if k < n else n - 1
            col = carry
            for a, b in pairs:
                col += sum(a[i] * b[k - i] for i in range(i0, i1 + 1))
            for a in squares:
                col += sum(a[i] * (a[k - i] << 1) for i in range(i0, (k + 1) // 2)) + (a[k // 2] ** 2 if k % 2 == 0 else 0)
            col += sum(m[i] * S.modl[k - i] for i in range(i0, (k - 1 if k < n else n - 1) + 1))
            need(col < U64, f"column {k} reaches 2^64")
            if k < n:
                m[k] = (-col) & S.mask
                col += S.mask                      # == adding m[k] * mod[0] as far as the carry goes (mod == 1 mod 2^w)
                need(col < U64, f"column {k} reaches 2^64")
            else:
                if e is not None:
                    col += e[k - n]
                    need(col < U64, f"column {k} reaches 2^64")
                r[k - n] = col & S.mask
            carry = col >> w
        need(carry < U32, "top limb wraps")
        r[n - 1] = carry
        if e is not None:
            r[n - 1] += e[n - 1]
            need(r[n - 1] < U32, "top limb + e wraps")
        return r

    def mul(self, a, b):
        return self.mul_sum([(a, b)])

    def sqr(self, a):
        return self.mul_sum([], squares=[a])

    def mul_add(self, a, b, c, d):
        return self.mul_sum([(a, b), (c, d)])

    def mul_add_hi(self, a, b, c, d, e):
        return self.mul_sum([(a, b), (c, d)], e=e)

    def mul_hi(self, a, b, e):
        return self.mul_sum([(a, b)], e=e)

    def mul_add4(self, a, b, c, d, e, f, g, h):
        return self.mul_sum([(a, b), (c, d), (e, f), (g, h)])

    def lin(self, pos=(), K=None, U=None, neg=()):
        """limb-wise  sum coef x  +  (L_(K, U) - sum coef y): the bracket must not go negative, nothing may leave 32 bits"""
        S = self.S
        L = S.table(K, U) if K is not None else [0] * S.n
        out = []
        for i in range(S.n):
            br = L[i]
            for c, y in neg:
                need(c * y[i] < U32, f"{c}u * x wraps in limb {i}")
                br -= c * y[i]
                need(br >= 0, f"K p table subtraction goes negative in limb {i}")
            t = br
            for c, x in pos:
                need(c * x[i] < U32, f"{c}u * x wraps in limb {i}")
                t += c * x[i]
            need(t < U32, f"limb {i} wraps")
            out.append(t)
        return out

    def norm(self, a):
        S = self.S
        self._chk(a)
        c, r = 0, []
        for i in range(S.n - 1):
            t = a[i] + c
            need(t < U32, "carry add wraps")
            r.append(t & S.mask)
            c = t >> S.w
        need(a[-1] + c < U32, "top limb wraps")
        r.append(a[-1] + c)
        assert r == S.digits(S.value(a))
        return r

    def window(self, a, name, masked):
        lo, hi = self.windows[name]
        l0 = a[0] & self.S.mask if masked else a[0]
        return ((l0 - lo) % U32) <= hi - lo


# --------------------------------------------------------------------------------------------------------------------------------
# interval tracker
# --------------------------------------------------------------------------------------------------------------------------------
class Iv:
    """value in [lo, hi] units of the modulus; every limb but the top <= limb, top limb <= top"""

    def __init__(self, lo, hi, limb, top):
        self.lo, self.hi, self.limb, self.top = Fr_(lo), Fr_(hi), int(limb), int(top)

    @property
    def lmax(self):
        return max(self.limb, self.top)

    def __repr__(self):
        return f"Iv([{float(self.lo):.3f}, {float(self.hi):.3f}], limb < 2^{self.limb.bit_length()}, top {self.top:#x})"


class Interval:
    """Two value disciplines are documented for Fq, and a formula is checked under the one its header states:
         "g1"  fqu.h's opening comment (G1 / twisted Edwards code): every multiply operand below 2^7 p with limbs < 2^30;
         "g2"  the Fq2 section of fqu.h and fq2pu.h: operands normalised or lazy with limbs < 2^30, values tracked through the formula
               (some exceed 2^7 p: d1 = a0 - a1 + 256 p of fq2u_sqr, the K p - 5 b operands up to 512 p) and every multiply OUTPUT
               below 26 p, far under the capacity 2^392 = 38968 p.
       Column capacity, 32-bit limb expressions and the fit of every result are checked under both."""

    def __init__(self, S, discipline="g1"):
        assert discipline in ("g1", "g2")
        self.S, self.discipline = S, discipline
        self.trace = {}

    def topmax(self, hi):
        return int(Fr_(hi) * self.S.mod) >> self.S.top_shift

    def normalised(self, lo, hi):
        return Iv(lo, hi, self.S.mask, self.topmax(hi))

    def const(self, limbs):
        v = Fr_(self.S.value(limbs), self.S.mod)
        return Iv(v, v, max(limbs[:-1]), limbs[-1])

    def _columns(self, prods, e):
        """worst-case run of the column loop: every limb at its bound, every quotient digit at 2^w - 1"""
        S, n = self.S, self.S.n
        carry = 0
        for k in range(2 * n - 1):
            i0 = 0 if k < n else k - n + 1
            cab = (k if k < n else n - 1) - i0 + 1
            col = carry + sum(cnt * cab * a.lmax * b.lmax for cnt, a, b in prods)
            col += sum(S.mask * S.modl[k - i] for i in range(i0, (k - 1 if k < n else n - 1) + 1))
            col += S.mask if k < n else (e.lmax if e is not None else 0)
            need(col < U64, f"column {k} can reach 2^64")
            carry = col >> S.w

    def _mul(self, prods, e=None):
        S = self.S
        self._columns(prods, e)
        k = Fr_(S.mod, S.radix)
        lo = sum(c * a.lo * b.lo for c, a, b in prods) * k
        hi = sum(c * a.hi * b.hi for c, a, b in prods) * k + 1      # (T + (radix - 1) mod) / radix
        if S is FQ and self.discipline == "g2":
            need(hi < 26, f"multiply output can reach {float(hi):.2f} p >= 26 p")
        if e is not None:
            need(e.lmax < U32, "e limb outside 32 bits")
            lo, hi = lo + e.lo, hi + e.hi
        need(hi * S.mod < S.radix, "result does not fit the limb form")
        need(self.topmax(hi) < U32, "top limb wraps")
        return self.normalised(lo, hi)

    def _value(self, a):
        if self.discipline == "g1":
            need(a.hi <= 128, f"multiply operand value > 2^7 p: {a}")

    # Fq preconditions as fqu.h documents them
    def _single(self, a):
        need(a.lmax < 1 << 30, f"multiply operand limb >= 2^30: {a}")
        self._value(a)

    def _pair58(self, a, b):
        need(a.lmax * b.lmax < 1 << 58, f"limb product >= 2^58: {a} x {b}")
        self._value(a), self._value(b)

    def mul(self, a, b):
        if self.S is FR:
            need(a.lmax <= int(2 ** 31.4), f"fru_mul lazy operand limb > 2^31.4: {a}")
            need(a.hi * R < 1 << 261, f"fru_mul lazy operand value >= 2^261: {a}")
            need(b.lmax <= FR.mask and b.hi <= 2, f"fru_mul multiplier not normalised / >= 2 r: {b}")
        else:
            self._single(a), self._single(b)
        return self._mul([(1, a, b)])

    def sqr(self, a):
        self._single(a)
        need(2 * a.lmax < U32, "a << 1 wraps")
        return self._mul([(1, a, a)])      # the doubled-operand form sums the same column values

    def mul_add(self, a, b, c, d):
        self._pair58(a, b), self._pair58(c, d)
        return self._mul([(1, a, b), (1, c, d)])

    def mul_add_hi(self, a, b, c, d, e):
        self._pair58(a, b), self._pair58(c, d)
        return self._mul([(1, a, b), (1, c, d)], e)

    def mul_hi(self, a, b, e):
        self._single(a), self._single(b)
        return self._mul([(1, a, b)], e)

    def mul_add4(self, a, b, c, d, e, f, g, h):
        for x, y in ((a, b), (c, d), (e, f), (g, h)):
            self._pair58(x, y)
        return self._mul([(1, a, b), (1, c, d), (1, e, f), (1, g, h)])

    def lin(self, pos=(), K=None, U=None, neg=()):
        S = self.S
        if K is not None:
            L = S.table(K, U)
            need(sum(c * y.limb for c, y in neg) <= min(L[:-1]), f"subtrahend limbs exceed {U} * 2^{S.w}: " + ", ".join(map(repr, (y for _, y in neg))))
            need(sum(c * y.top for c, y in neg) <= L[-1], "top limb of the table can go negative: " + ", ".join(map(repr, (y for _, y in neg))))
            limb, top, k = max(L[:-1]), L[-1], K
        else:
            assert not neg
            limb = top = k = 0
        for c, x in list(pos) + list(neg):
            need(c * x.lmax < U32, f"{c}u * x wraps")
        limb += sum(c * x.limb for c, x in pos)
        top += sum(c * x.top for c, x in pos)
        need(limb < U32 and top < U32, "limb-wise sum wraps")
        lo = sum(c * x.lo for c, x in pos) + k - sum(c * y.hi for c, y in neg)
        hi = sum(c * x.hi for c, x in pos) + k - sum(c * y.lo for c, y in neg)
        need(lo >= 0, "value can go negative")
        return Iv(lo, hi, limb, top)

    def norm(self, a):
        S = self.S
        c = 0
        for _ in range(S.n - 1):
            need(a.limb + c < U32, "carry add wraps")
            c = (a.limb + c) >> S.w
        need(a.top + c < U32, "top limb wraps")
        need(self.topmax(a.hi) < U32, "top limb wraps")
        return self.normalised(a.lo, a.hi)

    def window(self, a, name, masked):
        self.trace["window:" + name] = a
        return False                       # the fast path is what closure is about; the slow paths are saturated arithmetic


# --------------------------------------------------------------------------------------------------------------------------------
# the formulas, once, over a backend B (fqu.h / te.h / fq2pu.h; comments there)
# --------------------------------------------------------------------------------------------------------------------------------
def sub_lazy(B, K, a, b):
    return B.lin([(1, a)], K, 1, [(1, b)])


def add_lazy(B, a, b):
    return B.lin([(1, a), (1, b)])


def sub3_norm(B, a, b, c):
    return B.norm(B.lin([(1, a)], 8, 3, [(1, b), (2, c)]))


def neg5(B, a, big):
    return B.norm(B.lin([], 512 if big else 16, 5, [(5, a)]))


def fqu_xyzz_acc_mixed(B, ax, ay, azz, azzz, qx, qy):
    """returns None where the header returns false"""
    u2 = B.mul(qx, azz)
    pp = sub_lazy(B, 16, u2, ax)
    if isinstance(B, Interval):
        B.trace.update(u2=u2, ax=ax)
    if B.window(pp, "fqu_xyzz_acc_mixed", True):
        return None
    s2 = B.mul(qy, azzz)
    r = sub_lazy(B, 8, s2, ay)
    p2 = B.sqr(pp)
    zz = B.mul(azz, p2)
    p3 = B.mul(pp, p2)
    zzz = B.mul(azzz, p3)
    qv = B.mul(ax, p2)
    t = B.sqr(r)
    x3 = sub3_norm(B, t, p3, qv)
    d = B.norm(sub_lazy(B, 16, qv, x3))
    nay = B.lin([], 8, 1, [(1, ay)])
    return x3, B.mul_add(r, d, nay, p3), zz, zzz


def xyzzu_add(B, a, b):
    """a, b: (x, y, zz, zzz), both finite; returns None where the header takes xyzzu_add_slow"""
    u1 = B.mul(a[0], b[2])
    u2 = B.mul(b[0], a[2])
    pp = sub_lazy(B, 4, u2, u1)
    if isinstance(B, Interval):
        B.trace.update(u1=u1, u2=u2)
    if B.window(pp, "xyzzu_add", True):
        return None
    s1 = B.mul(a[1], b[3])
    s2 = B.mul(b[1], a[3])
    r = sub_lazy(B, 4, s2, s1)
    p2 = B.sqr(pp)
    p3 = B.mul(pp, p2)
    qv = B.mul(u1, p2)
    zz = B.mul(B.mul(a[2], b[2]), p2)
    zzz = B.mul(B.mul(a[3], b[3]), p3)
    t = B.sqr(r)
    x3 = sub3_norm(B, t, p3, qv)
    d = B.norm(sub_lazy(B, 16, qv, x3))
    ns1 = B.lin([], 8, 1, [(1, s1)])
    return x3, B.mul_add(r, d, ns1, p3), zz, zzz


def xyzzu_double(B, a):
    u = B.lin([(2, a[1])])
    v = B.sqr(u)
    w = B.mul(u, v)
    s = B.mul(a[0], v)
    xx = B.sqr(a[0])
    m = B.lin([(3, xx)])
    mm = B.sqr(m)
    x3 = B.norm(B.lin([(1, mm)], 8, 3, [(2, s)]))
    d = B.norm(sub_lazy(B, 16, s, x3))
    nw = B.lin([], 8, 1, [(1, w)])
    y3 = B.mul_add(m, d, nw, a[1])
    return x3, y3, B.mul(v, a[2]), B.mul(w, a[3])


def te_consts(B):
    S = FQ
    return {"one": B.const(S.digits(S.one)), "inv_d": B.const(S.digits(pow(TE_D, -1, P) * S.one % P)), "two_d": B.const(S.digits(2 * TE_D * S.one % P))}


def te_negate_niels(B, ym, yp, k2):
    """te_load_niels with neg set: the roles of Y - X and Y + X swap, k2 becomes the lazy 4 p - k2"""
    return yp, ym, B.lin([], 4, 1, [(1, k2)])


def teu_from_niels(B, ym, yp, k2):
    c = te_consts(B)
    return (B.norm(sub_lazy(B, 4, yp, ym)), B.norm(add_lazy(B, yp, ym)), B.norm(add_lazy(B, c["one"], c["one"])), B.mul(k2, c["inv_d"]))


def teu_finish(B, E, F, G, H):
    return B.mul(E, F), B.mul(G, H), B.mul(F, G), B.mul(E, H)


def teu_madd(B, a, ym, yp, k2):
    x, y, z, t = a
    A = B.mul(sub_lazy(B, 8, y, x), ym)
    Bq = B.mul(add_lazy(B, y, x), yp)
    C = B.mul(t, k2)
    F = B.lin([(2, z)], 4, 1, [(1, C)])
    G = B.lin([(2, z), (1, C)])
    return teu_finish(B, sub_lazy(B, 4, Bq, A), F, G, add_lazy(B, Bq, A))


def teu_add(B, a, b):
    A = B.mul(sub_lazy(B, 8, a[1], a[0]), sub_lazy(B, 8, b[1], b[0]))
    Bq = B.mul(add_lazy(B, a[1], a[0]), add_lazy(B, b[1], b[0]))
    C = B.mul(B.mul(a[3], b[3]), te_consts(B)["two_d"])
    Dh = B.mul(a[2], b[2])
    F = B.lin([(2, Dh)], 4, 1, [(1, C)])
    G = B.lin([(2, Dh), (1, C)])
    return teu_finish(B, sub_lazy(B, 4, Bq, A), F, G, add_lazy(B, Bq, A))


def teu_double(B, a):
    A, Bq, Cz = B.sqr(a[0]), B.sqr(a[1]), B.sqr(a[2])
    S_ = B.sqr(add_lazy(B, a[0], a[1]))
    G = B.norm(sub_lazy(B, 4, Bq, A))
    E = B.lin([(1, S_)], 8, 2, [(1, A), (1, Bq)])
    F = B.lin([(1, G)], 8, 2, [(2, Cz)])
    H = B.lin([], 8, 2, [(1, A), (1, Bq)])
    return teu_finish(B, E, F, G, H)


# ---- Fq2 = pairs (c0, c1), u^2 = -5
def fq2u_mul(B, a, b):
    v0 = B.mul(a[0], b[0])
    v1 = B.mul(a[1], b[1])
    m = B.mul(add_lazy(B, a[0], a[1]), add_lazy(B, b[0], b[1]))
    c1 = B.lin([(1, m)], 8, 2, [(1, v0), (1, v1)])
    c0 = B.lin([(1, v0)], 16, 5, [(5, v1)])
    return B.norm(c0), B.norm(c1)


def _sqr_parts(B, a):
    d1 = B.lin([(1, a[0])], 256, 1, [(1, a[1])])
    d2 = B.norm(B.lin([(1, a[0]), (5, a[1])]))
    return d1, d2


def fq2u_sqr(B, a):
    d1, d2 = _sqr_parts(B, a)
    v = B.mul(d1, d2)
    v2 = B.mul(a[0], a[1])
    return B.norm(B.lin([(1, v)], 16, 4, [(4, v2)])), B.norm(B.lin([(2, v2)]))


def fq2u_mul_n5(B, a, b, n5b1):
    return B.mul_add(a[0], b[0], a[1], n5b1), B.mul_add(a[0], b[1], a[1], b[0])


def fq2u_xyzz_acc_mixed(B, ax, ay, azz, azzz, qx, qy):
    """default (four-product) branch; returns None where the header returns false"""
    n5zz = neg5(B, azz[1], False)
    e0 = B.lin([], 128, 1, [(1, ax[0])])
    e1 = B.lin([], 128, 1, [(1, ax[1])])
    pp = (B.mul_add_hi(qx[0], azz[0], qx[1], n5zz, e0), B.mul_add_hi(qx[0], azz[1], qx[1], azz[0], e1))
    if isinstance(B, Interval):
        B.trace.update(ax=ax, u2=(B.mul_add(qx[0], azz[0], qx[1], n5zz), B.mul_add(qx[0], azz[1], qx[1], azz[0])))
    w0, w1 = B.window(pp[0], "fq2u_xyzz_acc_mixed", False), B.window(pp[1], "fq2u_xyzz_acc_mixed", False)
    if w0 and w1:
        return None
    n5zzz = neg5(B, azzz[1], False)
    nay0 = B.lin([], 64, 1, [(1, ay[0])])
    nay1 = B.lin([], 64, 1, [(1, ay[1])])
    r = (B.mul_add_hi(qy[0], azzz[0], qy[1], n5zzz, nay0), B.mul_add_hi(qy[0], azzz[1], qy[1], azzz[0], nay1))
    p2 = fq2u_sqr(B, pp)
    n5p2 = neg5(B, p2[1], False)
    zz = fq2u_mul_n5(B, p2, azz, n5zz)
    p3 = fq2u_mul_n5(B, pp, p2, n5p2)
    zzz = fq2u_mul_n5(B, p3, azzz, n5zzz)
    qv = fq2u_mul_n5(B, ax, p2, n5p2)
    d1, d2 = _sqr_parts(B, r)
    v2 = B.mul(r[0], r[1])
    f0 = B.lin([], 64, 3, [(1, p3[0]), (2, qv[0])])
    f1 = B.lin([], 64, 3, [(1, p3[1]), (2, qv[1])])
    e0 = B.lin([(1, B.lin([], 16, 4, [(4, v2)])), (1, f0)])
    e1 = B.lin([(2, v2), (1, f1)])
    x3 = (B.mul_hi(d1, d2, e0), B.norm(e1))
    d = (B.norm(B.lin([(1, qv[0])], 128, 1, [(1, x3[0])])), B.norm(B.lin([(1, qv[1])], 128, 1, [(1, x3[1])])))
    n5r = neg5(B, r[1], True)
    n5p3 = neg5(B, p3[1], False)
    y3 = (B.mul_add4(d[0], r[0], d[1], n5r, nay0, p3[0], nay1, n5p3), B.mul_add4(d[0], r[1], d[1], r[0], nay0, p3[1], nay1, p3[0]))
    if isinstance(B, Interval):
        B.trace.update(pp=pp, r=r)
    return x3, y3, zz, zzz


# ---- fq2pu.h: one Fq2 element over a lane pair; here a pair is (even lane's half, odd lane's half)
def p2_mul(B, a, b, big):
    """P2A of a times P2B<big> of b: even lane a0 b0 + a1 (K p - 5 b1), odd lane a1 b0 + a0 b1"""
    return B.mul_add(a[0], b[0], a[1], neg5(B, b[1], big)), B.mul_add(a[1], b[0], a[0], b[1])


def _p2_y3(B, r, d, ns, p3):
    n5d, n5p3 = neg5(B, d[1], True), neg5(B, p3[1], False)
    return (B.mul_add4(r[0], d[0], r[1], n5d, ns[0], p3[0], ns[1], n5p3), B.mul_add4(r[1], d[0], r[0], d[1], ns[1], p3[0], ns[0], p3[1]))


def _both(f):
    return f(0), f(1)


def xyzzu2_add(B, a, b):
    """a, b: (x, y, zz, zzz) of pairs, both finite; None where the header takes xyzzu2_add_slow"""
    u1 = p2_mul(B, a[0], b[2], False)
    u2 = p2_mul(B, b[0], a[2], False)
    pp = _both(lambda h: B.norm(sub_lazy(B, 4, u2[h], u1[h])))
    if isinstance(B, Interval):
        B.trace.update(u1=u1, u2=u2)
    w0, w1 = B.window(pp[0], "xyzzu2_add", False), B.window(pp[1], "xyzzu2_add", False)
    if w0 and w1:
        return None
    zzab = p2_mul(B, a[2], b[2], False)
    s1 = p2_mul(B, a[1], b[3], False)
    zzzab = p2_mul(B, a[3], b[3], False)
    s2 = p2_mul(B, b[1], a[3], False)
    r = _both(lambda h: B.norm(sub_lazy(B, 4, s2[h], s1[h])))
    p2 = p2_mul(B, pp, pp, True)
    p3 = p2_mul(B, pp, p2, False)
    qv = p2_mul(B, u1, p2, False)
    zz = p2_mul(B, zzab, p2, False)
    zzz = p2_mul(B, zzzab, p3, False)
    t = p2_mul(B, r, r, True)
    x3 = _both(lambda h: sub3_norm(B, t[h], p3[h], qv[h]))
    d = _both(lambda h: B.norm(sub_lazy(B, 16, qv[h], x3[h])))
    ns1 = _both(lambda h: B.lin([], 8, 1, [(1, s1[h])]))
    return x3, _p2_y3(B, r, d, ns1, p3), zz, zzz


def xyzzu2_double(B, a):
    """None where the header takes xyzzu2_double_slow"""
    u = _both(lambda h: B.norm(B.lin([(2, a[1][h])])))
    w0, w1 = B.window(u[0], "xyzzu2_double", False), B.window(u[1], "xyzzu2_double", False)
    if w0 and w1:
        return None
    v = p2_mul(B, u, u, True)
    w = p2_mul(B, u, v, False)
    s = p2_mul(B, a[0], v, False)
    xx = p2_mul(B, a[0], a[0], True)
    m = _both(lambda h: B.norm(B.lin([(3, xx[h])])))
    mm = p2_mul(B, m, m, True)
    x3 = _both(lambda h: B.norm(B.lin([(1, mm[h])], 8, 3, [(2, s[h])])))
    d = _both(lambda h: B.norm(sub_lazy(B, 16, s[h], x3[h])))
    nw = _both(lambda h: B.lin([], 8, 1, [(1, w[h])]))
    n5d, n5y = neg5(B, d[1], True), neg5(B, a[1][1], True)
    y3 = (B.mul_add4(m[0], d[0], m[1], n5d, nw[0], a[1][0], nw[1], n5y), B.mul_add4(m[1], d[0], m[0], d[1], nw[1], a[1][0], nw[0], a[1][1]))
    return x3, y3, p2_mul(B, v, a[2], False), p2_mul(B, w, a[3], False)


def xyzzu2_acc_mixed(B, ax, ay, azz, azzz, qx, qy):
    u2 = p2_mul(B, qx, azz, False)
    pp = _both(lambda h: B.norm(sub_lazy(B, 16, u2[h], ax[h])))
    if isinstance(B, Interval):
        B.trace.update(u2=u2, ax=ax)
    w0, w1 = B.window(pp[0], "xyzzu2_acc_mixed", False), B.window(pp[1], "xyzzu2_acc_mixed", False)
    if w0 and w1:
        return None
    s2 = p2_mul(B, qy, azzz, False)
    r = _both(lambda h: B.norm(sub_lazy(B, 8, s2[h], ay[h])))
    p2 = p2_mul(B, pp, pp, True)
    zz3 = p2_mul(B, azz, p2, False)
    p3 = p2_mul(B, pp, p2, False)
    qv = p2_mul(B, ax, p2, False)
    zzz3 = p2_mul(B, azzz, p3, False)
    t = p2_mul(B, r, r, True)
    x3 = _both(lambda h: sub3_norm(B, t[h], p3[h], qv[h]))
    d = _both(lambda h: B.norm(sub_lazy(B, 16, qv[h], x3[h])))
    nay = _both(lambda h: B.lin([], 8, 1, [(1, ay[h])]))
    return x3, _p2_y3(B, r, d, nay, p3), zz3, zzz3


# --------------------------------------------------------------------------------------------------------------------------------
# Fr: the NTT butterflies of ntt_pass.hip (B over FR)
# --------------------------------------------------------------------------------------------------------------------------------
def fru_sub(B, K, U, a, b):
    return B.lin([(1, a)], K, U, [(1, b)])


def bfly(B, K, U, x, i, j, w):
    d = fru_sub(B, K, U, x[i], x[j])
    x[i] = add_lazy(B, x[i], x[j])
    x[j] = B.mul(d, w)


class Tws(tuple):
    """One twiddle per butterfly, indexed as the kernel's arrays are (ntt_pass.hip): radix8 tw[0..4) first stage, tw[4..6) second, tw[6] third; radix4
    tw[0..2) first stage, tw[2] second; radix8_last tw[1..4) = tw2[1..4) and tw[4] = tw1; radix4_last tw[0] = tw1.  A plain operand instead of a Tws
    is one twiddle for every butterfly (the interval proof: any canonical twiddle)."""


def _tw(tw, i):
    return tw[i] if isinstance(tw, Tws) else tw


def radix8(B, KB, x, tw):
    for k in range(4):
        bfly(B, KB, 1, x, k, k + 4, _tw(tw, k))
    bfly(B, 2 * KB, 2, x, 0, 2, _tw(tw, 4))
    bfly(B, 2 * KB, 2, x, 1, 3, _tw(tw, 5))
    bfly(B, 2, 1, x, 4, 6, _tw(tw, 4))
    bfly(B, 2, 1, x, 5, 7, _tw(tw, 5))
    x[0], x[1] = B.norm(x[0]), B.norm(x[1])
    bfly(B, 4 * KB, 1, x, 0, 1, _tw(tw, 6))
    bfly(B, 2, 1, x, 2, 3, _tw(tw, 6))
    bfly(B, 4, 2, x, 4, 5, _tw(tw, 6))
    bfly(B, 2, 1, x, 6, 7, _tw(tw, 6))
    for k in (0, 2, 4, 6):
        x[k] = B.norm(x[k])


def radix4(B, KB, x, tw):
    bfly(B, KB, 1, x, 0, 2, _tw(tw, 0))
    bfly(B, KB, 1, x, 1, 3, _tw(tw, 1))
    bfly(B, 2 * KB, 2, x, 0, 1, _tw(tw, 2))
    bfly(B, 2, 1, x, 2, 3, _tw(tw, 2))
    x[0], x[2] = B.norm(x[0]), B.norm(x[2])


def radix4_last(B, KB, x, tw):
    d02 = fru_sub(B, KB, 1, x[0], x[2])
    s02 = add_lazy(B, x[0], x[2])
    bfly(B, KB, 1, x, 1, 3, _tw(tw, 0))
    x[0], x[1] = B.norm(add_lazy(B, s02, x[1])), B.norm(fru_sub(B, 2 * KB, 2, s02, x[1]))
    x[2], x[3] = B.norm(add_lazy(B, d02, x[3])), B.norm(fru_sub(B, 2, 1, d02, x[3]))


def radix8_last(B, KB, x, tw):
    d04 = fru_sub(B, KB, 1, x[0], x[4])
    x[0] = add_lazy(B, x[0], x[4])
    for k in range(1, 4):
        bfly(B, KB, 1, x, k, k + 4, _tw(tw, k))
    d = fru_sub(B, 2 * KB, 2, x[0], x[2])
    x[0] = add_lazy(B, x[0], x[2])
    x[2] = d
    bfly(B, 2 * KB, 2, x, 1, 3, _tw(tw, 4))
    e = fru_sub(B, 2, 1, d04, x[6])
    x[4] = add_lazy(B, d04, x[6])
    x[6] = e
    bfly(B, 2, 1, x, 5, 7, _tw(tw, 4))
    x[0], x[1] = B.norm(x[0]), B.norm(x[1])
    for i, (K, U) in ((0, (4 * KB, 1)), (2, (2, 1)), (4, (4, 2)), (6, (2, 1))):
        s = add_lazy(B, x[i], x[i + 1])
        x[i + 1] = B.norm(fru_sub(B, K, U, x[i], x[i + 1]))
        x[i] = B.norm(s)


def fru_reduce_2r(a):
    """limbs normalised, value < 2^261 -> (q, limbs of a - q r); raises unless q is floor(a / r) or one less"""
    need(all(0 <= x <= FR.mask for x in a), "fru_reduce_2r wants normalised limbs")
    v = FR.value(a)
    q = a[8] // (FRU_R_TOP + 1)
    need(v // R - 1 <= q <= v // R, f"quotient estimate {q} for floor(a / r) = {v // R}")
    return q, FR.digits(v - q * R)


def fru_canon(a):
    _, t = fru_reduce_2r(a)
    v = FR.value(t)
    v = v - R if v >= R else v            # fp_reduce: one conditional subtraction
    need(0 <= v < R, "not canonical after one conditional subtraction")
    return v


def fru_quotient_steps():
    """the top-limb values at which the quotient estimate steps, and the one before each"""
    return [t for q in range(1, (1 << 29) // (FRU_R_TOP + 1) + 1) for t in (q * (FRU_R_TOP + 1) - 1, q * (FRU_R_TOP + 1))]


# --------------------------------------------------------------------------------------------------------------------------------
# packing (pure re-slicing) and curve maps
# --------------------------------------------------------------------------------------------------------------------------------
def pack32(S, l, words):
    """normalised limbs -> `words` 32-bit words of the integer (what fqu_pack / fru_pack store)"""
    v = S.value(l)
    need(v < 1 << (32 * words), "value does not fit the packed form")
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(words)]


def unpack32(S, ws):
    return S.digits(sum(int(x) << (32 * i) for i, x in enumerate(ws)))


def sw_to_te(Pt):
    """affine point of E: y^2 = x^3 + 1 -> affine (X, Y) of -X^2 + Y^2 = 1 + D X^2 Y^2"""
    x, y = Pt
    w = (x + 1) * pow(TE_S, -1, P) % P
    return TE_F * w * pow(y, -1, P) % P, (w - 1) * pow(w + 1, -1, P) % P


def te_to_sw(X, Y, Z):
    """projective (X : Y : Z) -> affine point of E, None for the neutral element (0 : 1 : 1)"""
    if X % P == 0:
        return None
    w = (Z + Y) * pow(Z - Y, -1, P) % P
    return (TE_S * w - 1) % P, TE_F * w * Z * pow(X, -1, P) % P


def te_niels(Pt):
    """(Y - X, Y + X, 2 D X Y) x R' mod p, canonical limbs"""
    X, Y = sw_to_te(Pt)
    return tuple(FQ.digits(v % P * FQ.one % P) for v in (Y - X, Y + X, 2 * TE_D * X * Y))


# --------------------------------------------------------------------------------------------------------------------------------
# input families (shared by the CPU and GPU tests): limb vectors of system S with every limb < limb_cap (a power of two or any
# exclusive bound) and value < value_cap * mod
# --------------------------------------------------------------------------------------------------------------------------------
def greedy_max(S, limb_cap, value_cap):
    """the largest admissible vector, chosen from the top limb down"""
    rem, l = value_cap * S.mod - 1, [0] * S.n
    for i in reversed(range(S.n)):
        l[i] = min(limb_cap - 1, rem >> (S.w * i))
        rem -= l[i] << (S.w * i)
    return l


def fam_largest(S, limb_cap, value_cap):
    g = greedy_max(S, limb_cap, value_cap)
    return [g] + [g[:i] + [g[i] - 1] + g[i + 1:] for i in range(S.n) if g[i] > 0]


def fam_patterns(S, limb_cap, value_cap):
    g = greedy_max(S, limb_cap, value_cap)
    hot = [[g[j] if j == i else 0 for j in range(S.n)] for i in range(S.n)]
    alt = [[g[j] if j % 2 == par else 0 for j in range(S.n)] for par in (0, 1)]
    return hot + alt


def fam_special(S, value_cap, kmax=None):
    vs = [0, 1, S.one, S.mod - 1]
    for k in range(1, (kmax or value_cap) + 1):
        vs += [k * S.mod - 1] + ([k * S.mod, k * S.mod + 1] if k < value_cap else [])
    return [S.digits(v) for v in vs]


def denormalise(S, l, limb_cap, rng):
    """the same value with 2^w moved from limb i + 1 into limb i, at random places, up to the limb bound"""
    l = list(l)
    for i in rng.sample(range(S.n - 1), S.n - 1):
        room = (limb_cap - 1 - l[i]) >> S.w
        k = rng.randint(0, min(room, l[i + 1]))
        l[i] += k << S.w
        l[i + 1] -= k
    return l


def fam_denormalised(S, limb_cap, value_cap, rng, count):
    out = []
    for _ in range(count):
        v = rng.randrange(S.mod) + rng.randrange(value_cap) * S.mod
        out.append(denormalise(S, S.digits(v), limb_cap, rng))
    return out


def fam_random(S, limb_cap, value_cap, rng, count):
    out = [S.digits(rng.randrange(S.mod)) for _ in range(count // 2)]
    return out + fam_denormalised(S, limb_cap, value_cap, rng, count - count // 2)


def quotient_pairs(S, value_cap, rng):
    """(a, b) whose Montgomery quotient digits are all 2^w - 1 (a b == mod  mod radix) and all 0 (a b == 0 mod radix)"""
    half = S.bits // 2
    zero = (S.digits(rng.randrange(1, 1 << (S.bits - half - 9)) << half), S.digits(rng.randrange(1, 1 << (S.bits - half - 9)) << half))
    while True:
        a = rng.randrange(1, min(value_cap * S.mod, S.radix), 2)
        b = S.mod * pow(a, -1, S.radix) % S.radix
        if b < value_cap * S.mod:
            assert (a * b * S.ninv) % S.radix == S.radix - 1
            return [(S.digits(a), S.digits(b)), zero]


def column_pairs(S, cap_a, cap_b, value_cap_a, value_cap_b):
    """for every column k, the operand pair whose only non-zero limbs are the ones that meet in column k, at their maxima"""
    ga, gb = greedy_max(S, cap_a, value_cap_a), greedy_max(S, cap_b, value_cap_b)
    out = []
    for k in range(2 * S.n - 1):
        i0, i1 = max(0, k - S.n + 1), min(k, S.n - 1)
        out.append(([ga[i] if i0 <= i <= i1 else 0 for i in range(S.n)], [gb[i] if i0 <= i <= i1 else 0 for i in range(S.n)]))
    return out
