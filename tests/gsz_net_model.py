"""The GSZ products and product check of tests/gsz_mul_model.py restated for ONE PARTY PER PROCESS, as czk_net_gsz_* (include/czk.h) runs them.
TEST INFRASTRUCTURE ONLY.

A `Party` holds its own lane of every vector and of the material and nothing else.  Its protocols are generators: wherever the party needs the others
it yields one exchange -- ("to_king", values, tag), ("from_king", answers or None, tag) or ("broadcast", values, tag) -- and is resumed with what the
exchange delivers to its rank.  `run` steps the parties in lockstep through a `RecordingNet`, which checks that all of them ask for the same exchange,
performs it and writes it down, so a test can read off how many exchanges a call makes and in which order values and coins travel.

The king (rank 0) alone sees the gathered masked products, so he alone counts violations of the bound 2 deg (`king_bad`, part of his `bad`); plain
opens are broadcasts and every rank counts theirs."""
from gsz_mul_model import R_MOD, ceil_log2

INV2 = pow(2, -1, R_MOD)


def exchange_counts(op: str, n: int):
    """(to_king, from_king, broadcasts) of one call over n > 0 elements, as include/czk.h states them"""
    R = ceil_log2(n)
    return {"mul": (1, 1, 0), "inv": (1, 1, 1), "pp": (5, 5, 3), "check": (R + 2, R + 2, R + 2)}[op]


class RecordingNet:
    """mpc-net's three primitives between P lockstepped parties; log = [(kind, tag, elements per party)]"""

    def __init__(self, parties: int):
        self.P, self.log = parties, []

    def to_king(self, vals, tag):
        self.log.append(("to_king", tag, len(vals[0])))
        return [[list(v) for v in vals]] + [None] * (self.P - 1)

    def from_king(self, vals, tag):
        assert all(v is None for v in vals[1:]), "only the king sends"
        self.log.append(("from_king", tag, len(vals[0][0])))
        return [list(a) for a in vals[0]]

    def broadcast(self, vals, tag):
        self.log.append(("broadcast", tag, len(vals[0])))
        return [[list(v) for v in vals] for _ in range(self.P)]

    def counts(self):
        return tuple(sum(k == kind for k, _, _ in self.log) for kind in ("to_king", "from_king", "broadcast"))


def run(net: RecordingNet, gens):
    """steps one generator per party through `net` until all return; -> their return values"""
    gens, results = list(gens), [None] * net.P
    msgs = [next(g) for g in gens]
    while True:
        kind, tag = msgs[0][0], msgs[0][2]
        assert all(m[0] == kind and m[2] == tag for m in msgs), "the parties disagree on the exchange"
        got = getattr(net, kind)([m[1] for m in msgs], tag)
        msgs, done = [], 0
        for j, g in enumerate(gens):
            try:
                msgs.append(g.send(got[j]))
            except StopIteration as e:
                results[j], done = e.value, done + 1
        if done:
            assert done == net.P, "some parties returned before the others"
            return results


class Party:
    def __init__(self, D, rank: int, deg: int, dr, dr2, rands):
        """dr, dr2, rands: THIS party's lanes of the material (lists of ints)"""
        self.D, self.rank, self.deg, self.dr, self.dr2, self.rands = D, rank, deg, dr, dr2, rands
        self.d = self.r = 0
        self.bad = self.king_bad = self.zero = 0

    def doubles(self, k):
        s = slice(self.d, self.d + k)
        self.d += k
        assert self.d <= len(self.dr), "out of double shares"
        return self.dr[s], self.dr2[s]

    def rand(self, k):
        s = slice(self.r, self.r + k)
        self.r += k
        assert self.r <= len(self.rands), "out of random shares"
        return self.rands[s]

    # ---- the two cross-party steps ----------------------------------------------------------------------------------------------------------------
    def king_trip(self, masked, tag):
        """batch_king_compute with f = identity: one to_king and one from_king -> the opened values"""
        gathered = yield ("to_king", masked, tag)
        ans = None
        if self.rank == 0:
            opened = []
            for i in range(len(masked)):
                v, b = self.D.open([g[i] for g in gathered], 2 * self.deg)
                opened.append(v)
                self.bad += b
                self.king_bad += b
            ans = [opened] * self.D.parties                            # `vec![output; n]`
        return (yield ("from_king", ans, tag))

    def open(self, share, tag):
        """batch_open at the bound deg: one broadcast -> the values"""
        gathered = yield ("broadcast", share, tag)
        vals = []
        for i in range(len(share)):
            v, b = self.D.open([g[i] for g in gathered], self.deg)
            vals.append(v)
            self.bad += b
        return vals

    # ---- the protocols ------------------------------------------------------------------------------------------------------------------------------
    def batch_mul(self, x, y, tag="mul"):
        r, r2 = self.doubles(len(x))
        v = yield from self.king_trip([(a * b + c) % R_MOD for a, b, c in zip(x, y, r2)], tag)
        return [(vi - ri) % R_MOD for vi, ri in zip(v, r)]

    def batch_inv(self, x, tag="inv"):
        rs = self.rand(len(x))
        prod = yield from self.batch_mul(x, rs, tag)
        opened = yield from self.open(prod, tag)
        self.zero += sum(v == 0 for v in opened)
        return [c * (pow(v, -1, R_MOD) if v else 0) % R_MOD for c, v in zip(rs, opened)]

    def partial_products(self, x):
        n = len(x)
        m = self.rand(n + 1)
        m_inv = yield from self.batch_inv(m, "m_inv")
        mx = yield from self.batch_mul(m[:n], x, "mx")
        mxm = yield from self.batch_mul(mx, m_inv[1:], "mxm")
        run_ = yield from self.open(mxm, "mxm")
        for i in range(1, n):
            run_[i] = run_[i] * run_[i - 1] % R_MOD
        mms = yield from self.batch_mul([m[0]] * n, m_inv[1:], "mms")
        mms_inv = yield from self.batch_inv(mms, "mms_inv")
        return [v * k % R_MOD for v, k in zip(mms_inv, run_)]

    def product_check(self, xs, ys, zs):
        """hadamard_check -> ip_check with ip_l and ip3 of a round in one king round trip and the round's coin after it -> verdict"""
        n = len(xs)
        (c,) = yield from self.open(self.rand(1), ("coin", "hadamard"))
        pw = [1] * n
        for i in range(1, n):
            pw[i] = pw[i - 1] * c % R_MOD
        xs, ys = [a * p % R_MOD for a, p in zip(xs, pw)], list(ys)
        ip = sum(a * p for a, p in zip(zs, pw)) % R_MOD
        rnd = 0
        while len(xs) > 1:
            if len(xs) % 2:
                xs.append(0)
                ys.append(0)
            h = len(xs) // 2
            xl, xr, yl, yr = xs[:h], xs[h:], ys[:h], ys[h:]
            r, r2 = self.doubles(2)
            ipl_m = (sum(a * b for a, b in zip(xl, yl)) + r2[0]) % R_MOD
            ip3_m = (sum((2 * b - a) * (2 * d - e) for a, b, e, d in zip(xl, xr, yl, yr)) + r2[1]) % R_MOD
            v = yield from self.king_trip([ipl_m, ip3_m], ("ip", rnd))
            ip_l, ip3 = (v[0] - r[0]) % R_MOD, (v[1] - r[1]) % R_MOD
            (c,) = yield from self.open(self.rand(1), ("coin", rnd))
            ip_r = (ip - ip_l) % R_MOD
            xs = [((b - a) * c + 2 * a - b) % R_MOD for a, b in zip(xl, xr)]
            ys = [((b - a) * c + 2 * a - b) % R_MOD for a, b in zip(yl, yr)]
            f1, f2, f3 = (c - 2) * (c - 3) * INV2 % R_MOD, -(c - 1) * (c - 3) % R_MOD, (c - 1) * (c - 2) * INV2 % R_MOD
            ip = (f1 * ip_l + f2 * ip_r + f3 * ip3) % R_MOD
            rnd += 1
        xr, yr = self.rand(2)
        x, y = xs[0], ys[0]
        r, r2 = self.doubles(4)
        v = yield from self.king_trip([(xr * yr + r2[0]) % R_MOD, (x * xr + r2[1]) % R_MOD, (y * yr + r2[2]) % R_MOD], ("final", 0))
        ipr, xb, yb = [(a - b) % R_MOD for a, b in zip(v, r[:3])]
        (v,) = yield from self.king_trip([(ip * ipr + r2[3]) % R_MOD], ("final", 1))
        o = yield from self.open([xb, yb, (v - r[3]) % R_MOD], ("blind", 0))
        return o[0] * o[1] % R_MOD == o[2]


def parties_of(D, deg: int, src):
    """one Party per lane of a gsz_mul_model.Material"""
    return [Party(D, j, deg, src.dr[j], src.dr2[j], src.rands[j] if src.rands else []) for j in range(D.parties)]
