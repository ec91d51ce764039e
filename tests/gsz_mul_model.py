"""Big-integer model of the GSZ (Shamir) products and their product check, party by party: batch_mult (mpc-algebra/src/share/gsz20/mod.rs:559-594),
batch_inv (:325-342), partial_products (:343-366), hadamard_check (:599-614), ip_check (:738-787), ip_compress (:619-733), ip_compute (:789-808), with
king_compute (:468-524), open_degree_vec (:440-459) and coin (:529-531) underneath.  TEST INFRASTRUCTURE ONLY.

A shared vector is a list of `parties` lanes of n Python ints (canonical values mod r): lane j is party j's share p(w^j), w the generator of the
order-`parties` share domain (gsz20/mod.rs:98-105).  Every function does what ONE party does with its own lane, in a loop over the parties; the only
cross-party steps are `Domain.open` (everyone broadcasts) and the king's open inside `king` (everyone sends to the king, the king sends the opened
VALUE back to everyone, :478, :509).  Material is consumed in the reference's order through a `Material` cursor, so the device calls can be replayed
from the same arrays.

One deliberate difference from the reference: its add / sub never update `degree`, so hadamard_check's rzs_sum keeps "degree 0" (:605-610); with its
constant stand-in shares that is harmless, on real shares the last mult(ip, ...) for n = 1 would open a degree-2t polynomial against a bound of 0.
Here degrees are the TRUE ones: every operand of the check is a degree-`deg` share, every king's open bounds at 2 deg and every plain open at deg."""
import random

from share_mul_model import MONT_R_INV, R_MOD, from_limbs, to_limbs  # noqa: F401  (the limb helpers are part of this model's face)

OP_MUL, OP_INV, OP_PARTIAL_PRODUCTS, OP_PRODUCT_CHECK = 0, 1, 2, 3
# LARGE_SUBGROUP_ROOT_OF_UNITY of Fr (algebra/bls12_377 fr.rs:21-28), Montgomery limbs: a root of order 3 * 2^47
_LARGE_ROOT_LIMBS = (0xc790c167, 0x9bfe9d90, 0x39013bff, 0x7175a69e, 0xadabcf93, 0x3fbbb698, 0xd6f0dc97, 0x0c59f8d8)
_LARGE_ROOT = sum(v << (32 * i) for i, v in enumerate(_LARGE_ROOT_LIMBS)) * MONT_R_INV % R_MOD


def ceil_log2(n: int) -> int:
    return (n - 1).bit_length() if n > 1 else 0


def material_counts(op: int, n: int):
    """(double shares, random shares) one call over n elements consumes: what czk_gsz_material_counts reports"""
    if op == OP_MUL:
        return n, 0
    if op == OP_INV:
        return n, n
    if op == OP_PARTIAL_PRODUCTS:          # doubles: batch_inv(m) n + 1, mx, mxm, mms, the inner batch_inv n each; rands: m n + 1, batch_inv(m) n + 1, inner n
        return (5 * n + 1, 3 * n + 2) if n else (0, 0)
    if op == OP_PRODUCT_CHECK:             # doubles: ip_l and ip3 per round, four final mults; rands: hadamard coin, a coin per round, xr, yr
        return (2 * ceil_log2(n) + 4, ceil_log2(n) + 3) if n else (0, 0)
    raise ValueError(op)


def threshold(parties: int) -> int:
    return (parties - 1) // 2              # gsz20/mod.rs:94-96


class Domain:
    """MixedRadixEvaluationDomain::new(parties) as far as the shares need it (mixed_radix.rs:57-107; root rule fields/mod.rs:337-367)"""

    def __init__(self, parties: int):
        q = 1 if parties % 3 == 0 else 0
        two = parties // 3 ** q
        if parties < 1 or two & (two - 1):
            raise ValueError("no share domain of that size")
        w = _LARGE_ROOT if q else pow(_LARGE_ROOT, 3, R_MOD)
        for _ in range(47 - (two.bit_length() - 1)):
            w = w * w % R_MOD
        self.parties, self.w, self.w_inv, self.size_inv = parties, w, pow(w, -1, R_MOD), pow(parties, -1, R_MOD)
        self.points = [pow(w, j, R_MOD) for j in range(parties)]
        self.inv_tab = [[self.size_inv * pow(self.w_inv, j * k, R_MOD) % R_MOD for k in range(parties)] for j in range(parties)]

    def share(self, values, deg: int, rng):
        """a random degree-`deg` sharing of every value: lane j = p(w^j), p(0) = the value"""
        out = [[0] * len(values) for _ in range(self.parties)]
        for i, v in enumerate(values):
            cs = [v % R_MOD] + [rng.randrange(R_MOD) for _ in range(deg)]
            for j, pt in enumerate(self.points):
                acc = 0
                for c in reversed(cs):
                    acc = (acc * pt + c) % R_MOD
                out[j][i] = acc
        return out

    def public(self, values):
        """from_public (:185-187): the value on every party, a degree-0 sharing"""
        return [[v % R_MOD for v in values] for _ in range(self.parties)]

    def coeffs(self, vals):
        return [sum(vals[j] * self.inv_tab[j][k] for j in range(self.parties)) % R_MOD for k in range(self.parties)]

    def open(self, vals, bound: int):
        """open_degree_vec (:440-459) on one element's `parties` values -> (p(0), 1 if the polynomial exceeds the bound)"""
        P = self.parties                   # only p(0) and the coefficients above the bound matter
        high = any(sum(vals[j] * self.inv_tab[j][k] for j in range(P)) % R_MOD for k in range(bound + 1, P))
        return sum(vals) * self.size_inv % R_MOD, int(high)

    def batch_open(self, vec, bound: int):
        vals, bad = [], 0
        for i in range(len(vec[0])):
            v, b = self.open([lane[i] for lane in vec], bound)
            vals.append(v)
            bad += b
        return vals, bad


class Material:
    """Double shares (r of degree deg, r2 of degree 2 deg, one value) and random shares as GSZ vectors, with the cursors the protocols advance."""

    def __init__(self, dr, dr2, rands):
        self.dr, self.dr2, self.rands = dr, dr2, rands
        self.d = self.r = 0

    def doubles(self, k):
        s = slice(self.d, self.d + k)
        self.d += k
        assert self.d <= len(self.dr[0]), "out of double shares"
        return [ln[s] for ln in self.dr], [ln[s] for ln in self.dr2]

    def rand(self, k):
        s = slice(self.r, self.r + k)
        self.r += k
        assert self.r <= len(self.rands[0]), "out of random shares"
        return [ln[s] for ln in self.rands]


def random_material(D: Domain, deg: int, op: int, n: int, seed: int) -> Material:
    """What a trusted dealer hands out for one call (insecure here: one process knows everything).  Random shares are of non-zero values: the
    protocols invert what they mask."""
    rng = random.Random(seed)
    nd, nr = material_counts(op, n)
    vals = [rng.randrange(R_MOD) for _ in range(nd)]
    return Material(D.share(vals, deg, rng), D.share(vals, 2 * deg, rng), D.share([rng.randrange(1, R_MOD) for _ in range(nr)], deg, rng))


def dummy_material(D: Domain, op: int, n: int) -> Material:
    """the reference's stubs (:383-406): one on every party"""
    nd, nr = material_counts(op, n)
    return Material(D.public([1] * nd), D.public([1] * nd), D.public([1] * nr))


def king(D: Domain, deg: int, masked, r, tamper=None):
    """batch_king_compute with f = identity (:494-524) and the subtraction that follows: masked = x y + r2 lanes -> (v - r lanes, violations of 2 deg).
    tamper(masked) may change what the parties send to the king."""
    if tamper:
        tamper(masked)
    vals, bad = D.batch_open(masked, 2 * deg)
    return [[(v - rj) % R_MOD for v, rj in zip(vals, lane)] for lane in r], bad


def batch_mult(D: Domain, deg: int, x, y, src: Material, tamper=None):
    """:559-594 -> (shares, degree violations)"""
    r, r2 = src.doubles(len(x[0]))
    return king(D, deg, [[(a * b + c) % R_MOD for a, b, c in zip(lx, ly, l2)] for lx, ly, l2 in zip(x, y, r2)], r, tamper)


def batch_inv(D: Domain, deg: int, x, src: Material):
    """:325-342 -> (shares, degree violations, zero divisors); a zero divisor is counted and its element's share is zero on every lane"""
    rs = src.rand(len(x[0]))
    prod, bad = batch_mult(D, deg, x, rs, src)
    opened, b = D.batch_open(prod, deg)
    zero = sum(v == 0 for v in opened)
    inv = [pow(v, -1, R_MOD) if v else 0 for v in opened]
    return [[c * k % R_MOD for c, k in zip(lane, inv)] for lane in rs], bad + b, zero


def partial_products(D: Domain, deg: int, x, src: Material):
    """:343-366 -> (shares of x_0 ... x_i, degree violations, zero divisors)"""
    n = len(x[0])
    m = src.rand(n + 1)
    m_inv, bad, zero = batch_inv(D, deg, m, src)
    mx, b = batch_mult(D, deg, [ln[:n] for ln in m], x, src)
    bad += b
    mxm, b = batch_mult(D, deg, mx, [ln[1:] for ln in m_inv], src)
    bad += b
    mxm_pub, b = D.batch_open(mxm, deg)
    bad += b
    for i in range(1, n):
        mxm_pub[i] = mxm_pub[i] * mxm_pub[i - 1] % R_MOD
    mms, b = batch_mult(D, deg, [[ln[0]] * n for ln in m], [ln[1:] for ln in m_inv], src)
    bad += b
    mms_inv, b, z = batch_inv(D, deg, mms, src)
    return [[v * k % R_MOD for v, k in zip(lane, mxm_pub)] for lane in mms_inv], bad + b, zero + z


# ---- the product check: every share below is ONE element per party, a list of `parties` ints ---------------------------------------------------------
def coin(D: Domain, deg: int, src: Material):
    return D.open([ln[0] for ln in src.rand(1)], deg)


def ip_compute(D: Domain, deg: int, xs, ys, src: Material):
    """:789-808 -> (share, violations)"""
    r, r2 = src.doubles(1)
    masked = [[(sum(a * b for a, b in zip(lx, ly)) + l2[0]) % R_MOD] for lx, ly, l2 in zip(xs, ys, r2)]
    out, bad = king(D, deg, masked, r)
    return [ln[0] for ln in out], bad


def mult(D: Domain, deg: int, x, y, src: Material):
    out, bad = batch_mult(D, deg, [[v] for v in x], [[v] for v in y], src)
    return [ln[0] for ln in out], bad


def ip_check(D: Domain, deg: int, xs, ys, ip, src: Material):
    """:738-787 with ip_compress (:619-733) inline -> (x y == z, degree violations)"""
    P, bad = D.parties, 0
    xs, ys = [list(ln) for ln in xs], [list(ln) for ln in ys]
    while len(xs[0]) > 1:
        if len(xs[0]) % 2:
            for ln in xs + ys:
                ln.append(0)                                   # from_public(0): zero on every party
        h = len(xs[0]) // 2
        xl, xr, yl, yr = [ln[:h] for ln in xs], [ln[h:] for ln in xs], [ln[:h] for ln in ys], [ln[h:] for ln in ys]
        ip_l, b = ip_compute(D, deg, xl, yl, src)
        bad += b
        ip_r = [(a - c) % R_MOD for a, c in zip(ip, ip_l)]
        x3 = [[(2 * r - l) % R_MOD for l, r in zip(ll, lr)] for ll, lr in zip(xl, xr)]   # the line through (1, xl), (2, xr) at 3
        y3 = [[(2 * r - l) % R_MOD for l, r in zip(ll, lr)] for ll, lr in zip(yl, yr)]
        ip3, b = ip_compute(D, deg, x3, y3, src)
        bad += b
        c, b = coin(D, deg, src)
        bad += b
        xs = [[((r - l) * c + 2 * l - r) % R_MOD for l, r in zip(ll, lr)] for ll, lr in zip(xl, xr)]
        ys = [[((r - l) * c + 2 * l - r) % R_MOD for l, r in zip(ll, lr)] for ll, lr in zip(yl, yr)]
        inv2 = pow(2, -1, R_MOD)
        f1, f2, f3 = (c - 2) * (c - 3) * inv2 % R_MOD, -(c - 1) * (c - 3) % R_MOD, (c - 1) * (c - 2) * inv2 % R_MOD
        ip = [(f1 * ip_l[j] + f2 * ip_r[j] + f3 * ip3[j]) % R_MOD for j in range(P)]
    xr, yr = [ln[0] for ln in src.rand(1)], [ln[0] for ln in src.rand(1)]
    x, y = [ln[0] for ln in xs], [ln[0] for ln in ys]
    blinds = []
    ipr, b = mult(D, deg, xr, yr, src)
    bad += b
    for u, v in ((x, xr), (y, yr), (ip, ipr)):
        m, b = mult(D, deg, u, v, src)
        bad += b
        blinds.append(m)
    opened = []
    for m in blinds:
        v, b = D.open(m, deg)
        bad += b
        opened.append(v)
    return opened[0] * opened[1] % R_MOD == opened[2], bad


def hadamard_check(D: Domain, deg: int, xs, ys, zs, src: Material):
    """:599-614 -> (the check's verdict, degree violations)"""
    r, bad = coin(D, deg, src)
    n = len(xs[0])
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * r % R_MOD
    xs = [[a * p % R_MOD for a, p in zip(ln, pw)] for ln in xs]
    ip = [sum(a * p for a, p in zip(ln, pw)) % R_MOD for ln in zs]
    ok, b = ip_check(D, deg, xs, ys, ip, src)
    return ok, bad + b
