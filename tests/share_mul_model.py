"""Big-integer model of FieldShare::batch_mul / batch_inv / partial_products (mpc-algebra/src/share/field.rs:97-127, :135-148, :163-182), party by
party, for additive shares (lpp = 1 lane per party) and SPDZ shares (lpp = 2: sh and mac) with any MAC key.  TEST INFRASTRUCTURE ONLY.

A shared vector is a list of L = lpp * parties lanes of n Python ints (canonical values mod r), lane lpp * p = party p's `sh`, lane lpp * p + 1 its
`mac` -- the lane order of the device calls.  Every function below does what ONE party does with its own lanes, in a loop over the parties; the only
cross-party step is `batch_open`.  Material is consumed in the reference's order, through a `Material` cursor, so the device calls can be replayed
from the same arrays."""
import random

import numpy as np

R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041
MONT_R = (1 << 256) % R_MOD
MONT_R_INV = pow(MONT_R, -1, R_MOD)
OP_MUL, OP_INV, OP_PARTIAL_PRODUCTS = 0, 1, 2


def material_counts(op: int, n: int):
    """(triples, inverse pairs) one call of n elements consumes: what czk_share_material_counts reports"""
    if op == OP_MUL:
        return n, 0
    if op == OP_INV:
        return n, n
    if op == OP_PARTIAL_PRODUCTS:
        return 4 * n, (2 * n + 1 if n else 0)       # n + 1 pairs (m, m_inv), n of the inner batch_inv; mx, mxm, mms and the inner product
    raise ValueError(op)


class Scheme:
    def __init__(self, lpp: int, parties: int, mac_shares=None):
        assert lpp in (1, 2) and parties >= 1
        self.lpp, self.parties, self.lanes = lpp, parties, lpp * parties
        self.mac_shares = [m % R_MOD for m in (mac_shares or [0] * parties)]
        assert len(self.mac_shares) == parties
        self.alpha = sum(self.mac_shares) % R_MOD

    # ---- what one party does to its own share (its lpp lanes of one element) ------------------------------------------------------------------
    def add(self, a, b):
        return [(u + v) % R_MOD for u, v in zip(a, b)]

    def sub(self, a, b):
        return [(u - v) % R_MOD for u, v in zip(a, b)]

    def scale(self, a, k):
        return [u * k % R_MOD for u in a]

    def shift(self, p, a, v):
        """add the public v: the king's sh (share/add.rs:141-146); every party's mac += mac_share * v (share/spdz.rs:204-208)"""
        out = list(a)
        if p == 0:
            out[0] = (out[0] + v) % R_MOD
        if self.lpp == 2:
            out[1] = (out[1] + self.mac_shares[p] * v) % R_MOD
        return out

    # ---- sharing and opening ------------------------------------------------------------------------------------------------------------------
    def share(self, values, rng):
        """a random sharing of `values`: additive shares of v and (SPDZ) of alpha * v"""
        n = len(values)
        out = [[0] * n for _ in range(self.lanes)]
        for i, v in enumerate(values):
            for ln, tot in ((0, v % R_MOD), (1, self.alpha * v % R_MOD))[:self.lpp]:
                parts = [rng.randrange(R_MOD) for _ in range(self.parties - 1)]
                parts.append((tot - sum(parts)) % R_MOD)
                for p in range(self.parties):
                    out[self.lpp * p + ln][i] = parts[p]
        return out

    def king_share(self, values):
        """from_add_shared(v on the king, 0 elsewhere): the dummy material's sharing (sh = v, mac = alpha * v on the king's lanes)"""
        n = len(values)
        out = [[0] * n for _ in range(self.lanes)]
        out[0] = [v % R_MOD for v in values]
        if self.lpp == 2:
            out[1] = [self.alpha * v % R_MOD for v in values]
        return out

    def party(self, vec, p, i):
        return [vec[self.lpp * p + ln][i] for ln in range(self.lpp)]

    def batch_open(self, vec):
        """(values, failed MAC checks): the sum of the sh lanes; sum_p (mac_share_p * value - mac_p) must vanish (share/spdz.rs:166-185)"""
        n = len(vec[0])
        vals = [sum(vec[self.lpp * p][i] for p in range(self.parties)) % R_MOD for i in range(n)]
        bad = 0
        if self.lpp == 2:
            for i in range(n):
                dx = sum(self.mac_shares[p] * vals[i] - vec[2 * p + 1][i] for p in range(self.parties)) % R_MOD
                bad += dx != 0
        return vals, bad

    def opened(self, vec):
        return self.batch_open(vec)[0]

    def mac_opened(self, vec):
        n = len(vec[0])
        return [sum(vec[2 * p + 1][i] for p in range(self.parties)) % R_MOD for i in range(n)]


class Material:
    """Triples (x, y, z = x y) and inverse pairs (b, c) as shared vectors of T resp. P elements, with the cursors the protocols advance."""

    def __init__(self, tx, ty, tz, pb, pc):
        self.tx, self.ty, self.tz, self.pb, self.pc = tx, ty, tz, pb, pc
        self.t = self.p = 0

    def triples(self, k):
        s = slice(self.t, self.t + k)
        self.t += k
        assert self.t <= len(self.tx[0]), "out of triples"
        return [ln[s] for ln in self.tx], [ln[s] for ln in self.ty], [ln[s] for ln in self.tz]

    def inv_pairs(self, k):
        s = slice(self.p, self.p + k)
        self.p += k
        assert self.p <= len(self.pb[0]), "out of inverse pairs"
        return [ln[s] for ln in self.pb], [ln[s] for ln in self.pc]


def random_material(S: Scheme, op: int, n: int, seed: int) -> Material:
    """What a trusted dealer hands out for one call of `op` over n elements: random values, randomly split (insecure here: one process knows
    everything).  The relation inside a pair is the one the reference's formula needs in that slot: partial_products multiplies by m and by m_inv, so
    its first n + 1 pairs are (m, 1 / m); batch_inv returns c / open(x b), which is 1 / x for c = b, so its pairs are (b, b).  (The reference's only
    source hands out (1, 1), which is both.)"""
    rng = random.Random(seed)
    triples, pairs = material_counts(op, n)
    inverses = n + 1 if op == OP_PARTIAL_PRODUCTS and n else 0
    x = [rng.randrange(R_MOD) for _ in range(triples)]
    y = [rng.randrange(R_MOD) for _ in range(triples)]
    b = [rng.randrange(1, R_MOD) for _ in range(pairs)]
    c = [pow(v, -1, R_MOD) if i < inverses else v for i, v in enumerate(b)]
    return Material(S.share(x, rng), S.share(y, rng), S.share([u * v % R_MOD for u, v in zip(x, y)], rng), S.share(b, rng), S.share(c, rng))


def dummy_material(S: Scheme, op: int, n: int) -> Material:
    """DummyFieldTripleSource (mpc-algebra/src/wire/field.rs:41-76): one on the king, zero elsewhere"""
    triples, pairs = material_counts(op, n)
    return Material(*[S.king_share([1] * triples) for _ in range(3)], *[S.king_share([1] * pairs) for _ in range(2)])


def batch_mul(S: Scheme, ss, os_, src: Material):
    """field.rs:97-127 -> (shares, failed MAC checks over both opens)"""
    n = len(ss[0])
    xs, ys, zs = src.triples(n)
    sxs, bad1 = S.batch_open([[(a + b) % R_MOD for a, b in zip(l1, l2)] for l1, l2 in zip(ss, xs)])
    oys, bad2 = S.batch_open([[(a + b) % R_MOD for a, b in zip(l1, l2)] for l1, l2 in zip(os_, ys)])
    out = [[0] * n for _ in range(S.lanes)]
    for p in range(S.parties):
        for i in range(n):
            z, y, x = S.party(zs, p, i), S.party(ys, p, i), S.party(xs, p, i)
            r = S.shift(p, S.sub(S.sub(z, S.scale(y, sxs[i])), S.scale(x, oys[i])), sxs[i] * oys[i] % R_MOD)
            for ln in range(S.lpp):
                out[S.lpp * p + ln][i] = r[ln]
    return out, bad1 + bad2


def batch_inv(S: Scheme, xs, src: Material):
    """field.rs:135-148 -> (shares, failed MAC checks, zero divisors).  The reference unwraps the inverse; here a zero divisor is counted and its
    element's share is zero on every lane."""
    n = len(xs[0])
    bs, cs = src.inv_pairs(n)
    prod, bad = batch_mul(S, xs, bs, src)
    opened, bad2 = S.batch_open(prod)
    zero = sum(v == 0 for v in opened)
    inv = [pow(v, -1, R_MOD) if v else 0 for v in opened]
    return [[c * k % R_MOD for c, k in zip(lane, inv)] for lane in cs], bad + bad2, zero


def partial_products(S: Scheme, x, src: Material):
    """field.rs:163-182 -> (shares of x_0 ... x_i, failed MAC checks, zero divisors)"""
    n = len(x[0])
    m, m_inv = src.inv_pairs(n + 1)
    mx, bad = batch_mul(S, [ln[:n] for ln in m], x, src)
    mxm, b = batch_mul(S, mx, [ln[1:] for ln in m_inv], src)
    bad += b
    mxm_pub, b = S.batch_open(mxm)
    bad += b
    for i in range(1, n):
        mxm_pub[i] = mxm_pub[i] * mxm_pub[i - 1] % R_MOD
    mms, b = batch_mul(S, [[ln[0]] * n for ln in m], [ln[1:] for ln in m_inv], src)
    bad += b
    mms_inv, b, zero = batch_inv(S, mms, src)
    bad += b
    return [[v * k % R_MOD for v, k in zip(lane, mxm_pub)] for lane in mms_inv], bad, zero


# ---- Montgomery limbs of the device calls ---------------------------------------------------------------------------------------------------------
def to_limbs(vec) -> np.ndarray:
    """lanes of ints -> (lanes, n, 4) uint64 Montgomery limbs"""
    out = np.zeros((len(vec), len(vec[0]) if vec else 0, 4), dtype=np.uint64)
    for ln, lane in enumerate(vec):
        for i, v in enumerate(lane):
            m = v * MONT_R % R_MOD
            for j in range(4):
                out[ln, i, j] = (m >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def from_limbs(arr):
    arr = np.asarray(arr, dtype=np.uint64)
    return [[sum(int(arr[ln, i, j]) << (64 * j) for j in range(4)) * MONT_R_INV % R_MOD for i in range(arr.shape[1])] for ln in range(arr.shape[0])]
