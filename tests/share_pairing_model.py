"""Big-integer model of the pairing of shared points and of multiplicative target-group shares: MpcPairingEngine::pairing
(mpc-algebra/src/wire/pairing.rs:194-229), MulFieldShare (share/add.rs:407-480) and SpdzMulFieldShare (share/spdz.rs:459-541) in Fq12.
TEST INFRASTRUCTURE ONLY.  Everything is stated twice:

  literally        `pairing_literal`, `open_literal`, `scale_literal`, `vec_literal` do what the reference writes, on curve points and Fq12 elements
                   of tests/pairing_ref.py: separate pairings, fq12_inv, fq12_pow.  A point is an affine tuple or INF, an Fq12 a nested tuple.
  in the exponent  every point is a known multiple of a generator and every target-group element a known power of gt = e(G1, G2), so the protocol
                   is arithmetic mod r on the discrete logs (`pairing_exp`, `open_exp`, `scale_exp`); the expected limbs are gt^e (`gt_lanes`).
                   0 is infinity resp. one.

Lane order: share_mul_model's (lane lpp p = party p's sh, lpp p + 1 its mac).  Target-group shares are MULTIPLICATIVE: the value is the product of
the sh lanes, i.e. the SUM of their exponents.
Deliberate differences from the reference, as the device calls have them (include/czk.h): the mac lane of e(xa, y) is e(xa, mac lane of y), not built
from the process-global stand-in key; SPDZ mul multiplies both lanes.
The count of `pairing`: ELEMENTS where the MAC check of xa or of yb fails."""
import functools

import numpy as np

import group_share_model as GM
import pairing_ref as PR
from share_mul_model import R_MOD, Scheme  # noqa: F401

INF = PR.INF
FQ12_ZERO = (PR.FQ6_ZERO, PR.FQ6_ZERO)


# ---- gt and its powers --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gt_squares():
    g, out = PR.pairing(PR.G1_GEN, PR.G2_GEN), []
    for _ in range(R_MOD.bit_length()):
        out.append(g)
        g = PR.fq12_sqr(g)
    return out


@functools.lru_cache(maxsize=4096)
def gt_pow(e: int):
    """gt^e, gt = e(G1, G2), e mod r"""
    r, e = PR.FQ12_ONE, e % R_MOD
    for i, s in enumerate(_gt_squares()):
        if (e >> i) & 1:
            r = PR.fq12_mul(r, s)
    return r


def gt_limbs(f) -> np.ndarray:
    return np.array(PR.fq12_to_limbs(f), dtype=np.uint64)


def gt_lanes(lanes) -> np.ndarray:
    """lanes of exponents -> (L, n, 72) Montgomery limbs of gt^e: a device target-group vector"""
    return np.array([[PR.fq12_to_limbs(gt_pow(e)) for e in ln] for ln in lanes], dtype=np.uint64)


def fq12_lanes(lanes) -> np.ndarray:
    return np.array([[PR.fq12_to_limbs(f) for f in ln] for ln in lanes], dtype=np.uint64)


def k_of(S: Scheme, lane: int) -> int:
    """what the public factor is raised to on `lane`: 1 on the king's sh, mac_share_j on party j's mac, 0 elsewhere"""
    if S.lpp == 2 and lane & 1:
        return S.mac_shares[lane >> 1]
    return 1 if lane == 0 else 0


# ---- in the exponent ----------------------------------------------------------------------------------------------------------------------------------
def _sh_sum(S, vec, i):
    return sum(vec[S.lpp * p][i] for p in range(S.parties)) % R_MOD


def _mac_fails(S, vec, i, opened):
    return S.lpp == 2 and (S.alpha * opened - sum(vec[2 * p + 1][i] for p in range(S.parties))) % R_MOD != 0


def pairing_exp(S: Scheme, a, b, tx, ty, tz):
    """a, tx: lanes of G1 discrete logs; b, ty: of G2 discrete logs; tz: of gt exponents -> (lanes of gt exponents, elements whose MAC checks fail):
    gt^(tz_l - xa ty_l - tx_l yb + k_l xa yb)"""
    n = len(a[0])
    out, bad = [[0] * n for _ in range(S.lanes)], 0
    for i in range(n):
        masked_a = [[(a[ln][i] + tx[ln][i]) % R_MOD] for ln in range(S.lanes)]
        masked_b = [[(b[ln][i] + ty[ln][i]) % R_MOD] for ln in range(S.lanes)]
        xa, yb = _sh_sum(S, masked_a, 0), _sh_sum(S, masked_b, 0)
        bad += bool(_mac_fails(S, masked_a, 0, xa) or _mac_fails(S, masked_b, 0, yb))
        for ln in range(S.lanes):
            out[ln][i] = (tz[ln][i] - xa * ty[ln][i] - tx[ln][i] * yb + k_of(S, ln) * xa * yb) % R_MOD
    return out, bad


def open_exp(S: Scheme, v):
    """reveal of gt powers -> (exponents of the values, elements whose MAC check fails)"""
    n = len(v[0])
    vals = [_sh_sum(S, v, i) for i in range(n)]
    return vals, sum(bool(_mac_fails(S, v, i, vals[i])) for i in range(n))


def scale_exp(S: Scheme, v, f):
    """scale by the public gt^f_i; v None: from_public"""
    n = len(f)
    v = v or [[0] * n for _ in range(S.lanes)]
    return [[(v[ln][i] + k_of(S, ln) * f[i]) % R_MOD for i in range(n)] for ln in range(S.lanes)]


# ---- literally ----------------------------------------------------------------------------------------------------------------------------------------
def g1(e: int):
    return PR.g1_mul(e) if e % R_MOD else INF


def g2(e: int):
    return PR.g2_mul(e) if e % R_MOD else INF


def _pair(p, q):
    return PR.FQ12_ONE if p is INF or q is INF else PR.pairing(p, q)


def fq12_inv(f):
    """the device's inverse: Fermat's at the bottom of the tower, so zero stays zero"""
    return FQ12_ZERO if f == FQ12_ZERO else PR.fq12_inv(f)


def pairing_literal(S: Scheme, a, b, tx, ty, tz):
    """pairing.rs:204-225 lane by lane: a, tx lanes of G1 points, b, ty of G2 points, tz of Fq12 -> lanes of Fq12: z / e(xa, y) / e(x, yb) * e(xa, yb),
    the last factor scaled in (spdz.rs:500-506)"""
    n = len(a[0])
    out = [[None] * n for _ in range(S.lanes)]
    for i in range(n):
        xa, yb = INF, INF
        for p in range(S.parties):
            xa = PR.ec_add(PR.F1, PR.ec_add(PR.F1, xa, a[S.lpp * p][i]), tx[S.lpp * p][i])
            yb = PR.ec_add(PR.F2, PR.ec_add(PR.F2, yb, b[S.lpp * p][i]), ty[S.lpp * p][i])
        xayb = _pair(xa, yb)
        for ln in range(S.lanes):
            r = PR.fq12_mul(tz[ln][i], PR.fq12_inv(_pair(xa, ty[ln][i])))
            r = PR.fq12_mul(r, PR.fq12_inv(_pair(tx[ln][i], yb)))
            out[ln][i] = PR.fq12_mul(r, PR.fq12_pow(xayb, k_of(S, ln)))
    return out


def open_literal(S: Scheme, v):
    """reveal (add.rs:414-416, spdz.rs:469-478) on lanes of Fq12 -> (values, elements where prod_j x^(mac_share_j) / mac_j is not one)"""
    n, vals, bad = len(v[0]), [], 0
    for i in range(n):
        x = PR.FQ12_ONE
        for p in range(S.parties):
            x = PR.fq12_mul(x, v[S.lpp * p][i])
        vals.append(x)
        if S.lpp == 2:
            prod = PR.FQ12_ONE
            for p in range(S.parties):
                prod = PR.fq12_mul(prod, PR.fq12_mul(PR.fq12_pow(x, S.mac_shares[p]), fq12_inv(v[2 * p + 1][i])))
            bad += prod != PR.FQ12_ONE
    return vals, bad


def open_integer_rule(S: Scheme, v):
    """the device's form of the same verdict: x^A / (the product of the mac lanes), A the INTEGER sum of the canonical mac shares"""
    n, vals, bad, A = len(v[0]), [], 0, sum(S.mac_shares)
    for i in range(n):
        x, m = PR.FQ12_ONE, PR.FQ12_ONE
        for p in range(S.parties):
            x = PR.fq12_mul(x, v[S.lpp * p][i])
            if S.lpp == 2:
                m = PR.fq12_mul(m, v[2 * p + 1][i])
        vals.append(x)
        bad += S.lpp == 2 and PR.fq12_mul(PR.fq12_pow(x, A), fq12_inv(m)) != PR.FQ12_ONE
    return vals, bad


def scale_literal(S: Scheme, v, f):
    """scale (spdz.rs:500-506, add.rs:444-449) by the public f_i; v None: from_public (spdz.rs:479-485)"""
    n = len(f)
    v = v or [[PR.FQ12_ONE] * n for _ in range(S.lanes)]
    return [[PR.fq12_mul(v[ln][i], PR.fq12_pow(f[i], k_of(S, ln))) if k_of(S, ln) else v[ln][i] for i in range(n)] for ln in range(S.lanes)]


def vec_literal(op: str, a, b=None):
    if op == "inv":
        return [fq12_inv(x) for x in a]
    return [PR.fq12_mul(x, fq12_inv(y) if op == "div" else y) for x, y in zip(a, b)]


def outside_subgroup(seed: int):
    """an Fq12 element that is not an r-th root of unity (a random element of the field: its order does not divide r)"""
    import random
    rng = random.Random(seed)
    f = tuple(tuple((rng.randrange(PR.Q), rng.randrange(PR.Q)) for _ in range(3)) for _ in range(2))
    assert PR.fq12_pow(f, R_MOD) != PR.FQ12_ONE
    return f


def integer_consistent_lanes(S: Scheme, x, rng):
    """SPDZ lanes (n = 1) whose sh lanes multiply to x and whose mac lanes multiply to x^A, A the integer sum of the mac shares: party j holds
    x^(mac_share_j) times a blinding factor, the factors multiplying to one"""
    P = S.parties
    sh = [outside_subgroup(rng.randrange(1 << 30)) for _ in range(P - 1)]
    rest = x
    for s in sh:
        rest = PR.fq12_mul(rest, PR.fq12_inv(s))
    sh.append(rest)
    blind = [gt_pow(rng.randrange(R_MOD)) for _ in range(P - 1)]
    last = PR.FQ12_ONE
    for f in blind:
        last = PR.fq12_mul(last, PR.fq12_inv(f))
    blind.append(last)
    lanes = []
    for p in range(P):
        lanes += [[sh[p]], [PR.fq12_mul(PR.fq12_pow(x, S.mac_shares[p]), blind[p])]]
    return lanes


# ---- limbs of points ----------------------------------------------------------------------------------------------------------------------------------
def point_lanes(g: int, lanes):
    """lanes of discrete logs -> ((L, n, 12 | 24) limbs, (L, n) infinity bytes): a device point vector (group_share_model.exp_lanes)"""
    return GM.exp_lanes(g, lanes)


# ---- cases (never modified: tests copy what they change) ----------------------------------------------------------------------------------------------
def honest_case(S: Scheme, n: int, seed: int):
    """-> (values a, values b, dict of lanes in the exponent: a, b, tx, ty, tz), tz a sharing of x y"""
    import random
    rng = random.Random(seed)
    av, bv, xv, yv = ([rng.randrange(1, R_MOD) for _ in range(n)] for _ in range(4))
    return av, bv, dict(a=S.share(av, rng), b=S.share(bv, rng), tx=S.share(xv, rng), ty=S.share(yv, rng),
                        tz=S.share([x * y % R_MOD for x, y in zip(xv, yv)], rng))


EDGE_ROWS = ("a_is_minus_x", "b_is_minus_y", "a_tx_lane_infinite", "a_ty_lane_infinite", "a_infinite", "dummy_triple", "opposite_lane_summands")


def _move(vec, i, src, dst):
    """lane src's element i becomes 0 (infinity / one); lane dst takes it over, so the lanes still open to the same value"""
    vec[dst][i] = (vec[dst][i] + vec[src][i]) % R_MOD
    vec[src][i] = 0


def edge_case(S: Scheme, seed: int):
    """one element per name of EDGE_ROWS, every row an HONEST sharing (no MAC check fails) -> (values a, values b, lanes)"""
    import random
    assert S.parties >= 2
    n, rng = len(EDGE_ROWS), random.Random(seed)
    av, bv, ln = honest_case(S, n, seed)
    av, bv, ln = list(av), list(bv), {k: [list(x) for x in v] for k, v in ln.items()}
    xv, yv = S.opened(ln["tx"]), S.opened(ln["ty"])

    def reshare(name, i, value):
        for lane, s in enumerate(S.share([value], rng)):
            ln[name][lane][i] = s[0]
    av[0] = (-xv[0]) % R_MOD                                           # xa = open(a + x) is infinity
    reshare("a", 0, av[0])
    bv[1] = (-yv[1]) % R_MOD                                           # yb is infinity
    reshare("b", 1, bv[1])
    _move(ln["tx"], 2, S.lpp, 0)                                       # party 1's sh lane of tx is infinity
    _move(ln["ty"], 3, S.lanes - 1, S.lpp - 1)                         # the last lane of ty (SPDZ: a mac lane) is infinity
    av[4] = 0                                                          # a is infinity on every lane
    for lane in range(S.lanes):
        ln["a"][lane][4] = 0
    for name in ("tx", "ty", "tz"):                                    # DummyPairingTripleSource (pairing.rs:44-58): infinity, infinity, one
        for lane in range(S.lanes):
            ln[name][lane][5] = 0
    old = ln["a"][0][6]                                                # lane 0's a and tx cancel: the sum meets P + (-P)
    ln["a"][0][6] = (-ln["tx"][0][6]) % R_MOD
    ln["a"][S.lpp][6] = (ln["a"][S.lpp][6] + old - ln["a"][0][6]) % R_MOD
    return av, bv, ln
