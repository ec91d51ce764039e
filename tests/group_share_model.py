"""Big-integer model of the products of a shared point and a shared scalar: GroupShare::scale (mpc-algebra/src/share/group.rs:70-109, SPDZ forms
share/spdz.rs:385-446), gsz20's group mult (share/gsz20/mod.rs:1112-1130) and its product check for group triples, hadamard_check -> ip_check ->
ip_compress / ip_compute (:1132-1349).  TEST INFRASTRUCTURE ONLY.  Each protocol is stated twice:

  on curve points   `scale_points` / `gsz_mult_points` / `check_points` do what each party does with its own lanes, step by step as the reference
                    writes it, with the checker's curve arithmetic (oracle/orc.py: jac_add, scalar_mul).  A point is a Jacobian limb array.
  in the exponent   for points given as known multiples of the generator the group protocol IS the field protocol on the discrete logs: `scale_exp`
                    is share_mul_model.batch_mul's arithmetic, `gsz_mult_exp` is gsz_mul_model.batch_mult and `check_exp` its hadamard_check, on
                    ints mod r (0 = infinity).  The expected points are [e] G from the checker (`exp_points`), so a case costs one fixed-base
                    multiplication per output.

Lane order: share_mul_model's (lane lpp p = party p's sh, lpp p + 1 its mac) resp. gsz_mul_model's (lane j = the value at w^j).
One deliberate difference from the reference: its group open_degree_vec (:1048-1080) multiplies shares[i] where the transform needs shares[j]; the
model uses the field version's transform (gsz_mul_model.Domain.inv_tab), as the device call does.
The count of scale: ELEMENTS where either MAC check fails (share_mul_model.batch_mul counts the two opens separately)."""
import numpy as np

import gsz_mul_model as G
import orc
from share_mul_model import MONT_R, R_MOD, Scheme  # noqa: F401

OP_MUL, OP_PRODUCT_CHECK = 0, 1
AW = {1: 12, 2: 24}


def material_counts(op: int, n: int):
    """(group doubles, field doubles, random shares): what czk_gsz_group_material_counts reports"""
    if op == OP_MUL:
        return n, 0, 0
    if op == OP_PRODUCT_CHECK:             # group doubles: ip_l and ip3 per round, mult(yr, y), mult(ip_r, ip); field doubles: mult(xr, yr), mult(x, xr)
        return (2 * G.ceil_log2(n) + 2, 2, G.ceil_log2(n) + 3) if n else (0, 0, 0)
    raise ValueError(op)


class CheckMaterial:
    """what one product check consumes, everything in the exponent: group doubles (gr of degree deg, gr2 of 2 deg), field doubles, random shares"""

    def __init__(self, D: G.Domain, deg: int, n: int, seed: int):
        import random
        rng = random.Random(seed)
        gd, fd, nr = material_counts(OP_PRODUCT_CHECK, n)
        gv, fv = [rng.randrange(R_MOD) for _ in range(gd)], [rng.randrange(R_MOD) for _ in range(fd)]
        self.gr, self.gr2 = D.share(gv, deg, rng), D.share(gv, 2 * deg, rng)
        self.fr, self.fr2 = D.share(fv, deg, rng), D.share(fv, 2 * deg, rng)
        self.rands = D.share([rng.randrange(1, R_MOD) for _ in range(nr)], deg, rng)


def check_exp(D: G.Domain, deg: int, xs, ys, zs, mat: CheckMaterial):
    """hadamard_check for group triples (:1334-1349 -> :1280-1329) in the exponent: gsz_mul_model.hadamard_check on the discrete logs, its doubles
    being the group doubles of the rounds, the two field doubles, then the last two group doubles -- the order the four final mults consume them in
    (mult(xr, yr), mult(x, xr) field; mult(yr, y), mult(ip_r, ip) group) -> (verdict, degree violations)"""
    cut = len(mat.gr[0]) - 2
    dr = [g[:cut] + f + g[cut:] for g, f in zip(mat.gr, mat.fr)]
    dr2 = [g[:cut] + f + g[cut:] for g, f in zip(mat.gr2, mat.fr2)]
    src = G.Material(dr, dr2, mat.rands)
    res = G.hadamard_check(D, deg, xs, ys, zs, src)
    assert (src.d, src.r) == (len(dr[0]), len(mat.rands[0]))
    return res


# ---- limbs ------------------------------------------------------------------------------------------------------------------------------------------
def fr_limbs(vals, mont=False) -> np.ndarray:
    return orc.ints_to_limbs([v % R_MOD * (MONT_R if mont else 1) % R_MOD for v in vals], 4)


def one_y(g: int) -> np.ndarray:
    """the y coordinate the library writes for infinity: 1 (Montgomery)"""
    y = np.zeros(AW[g] // 2, np.uint64)
    y[:6] = orc.fq_from_repr(np.array([1, 0, 0, 0, 0, 0], np.uint64))
    return y


def exp_points(g: int, exps):
    """[e] G for every e -> ((n, AW) affine Montgomery limbs, (n,) infinity bytes); infinity is flag 1 with (0, 1)"""
    pts, inf = orc.fixed_base_points(g, fr_limbs(exps))
    pts, inf = np.array(pts), np.array(inf)
    pts[inf != 0] = 0
    pts[inf != 0, AW[g] // 2:] = one_y(g)
    return pts, inf


def exp_lanes(g: int, lanes):
    """lanes of exponents -> ((L, n, AW) limbs, (L, n) flags): a device point vector"""
    n = len(lanes[0])
    pts, inf = exp_points(g, [e for ln in lanes for e in ln])
    return pts.reshape(len(lanes), n, AW[g]), inf.reshape(len(lanes), n)


# ---- in the exponent --------------------------------------------------------------------------------------------------------------------------------
def scale_exp(S: Scheme, s, o, tx, ty, tz):
    """s, tx, tz: lanes of discrete logs; o, ty: lanes of scalars -> (lanes of discrete logs of out, elements whose MAC checks fail)"""
    n, P, lpp = len(s[0]), S.parties, S.lpp
    out, bad = [[0] * n for _ in range(S.lanes)], 0
    for i in range(n):
        sx = sum(s[lpp * p][i] + tx[lpp * p][i] for p in range(P)) % R_MOD
        oy = sum(o[lpp * p][i] + ty[lpp * p][i] for p in range(P)) % R_MOD
        if lpp == 2:
            ms = sum(s[2 * p + 1][i] + tx[2 * p + 1][i] for p in range(P))
            mo = sum(o[2 * p + 1][i] + ty[2 * p + 1][i] for p in range(P))
            bad += (S.alpha * sx - ms) % R_MOD != 0 or (S.alpha * oy - mo) % R_MOD != 0
        for p in range(P):
            z, y, x = S.party(tz, p, i), S.party(ty, p, i), S.party(tx, p, i)
            r = S.shift(p, S.sub(S.sub(z, S.scale(y, sx)), S.scale(x, oy)), sx * oy % R_MOD)
            for ln in range(lpp):
                out[lpp * p + ln][i] = r[ln]
    return out, bad


def gsz_mult_exp(D: G.Domain, deg: int, x, y, gr, gr2):
    """x: lanes of scalars; y, gr, gr2: lanes of discrete logs -> (lanes of discrete logs of out, elements over the king's bound)"""
    return G.batch_mult(D, deg, x, y, G.Material(gr, gr2, [[]]))


# ---- on curve points --------------------------------------------------------------------------------------------------------------------------------
class Curve:
    """the checker's group law on Jacobian limb arrays; public scalars are ints mod r"""

    def __init__(self, g: int):
        self.g, self.aw = g, AW[g]
        self.inf = self.mul(orc.generator_affine(g), False, 0)

    def from_affine(self, aff, is_inf):
        return self.mul(aff, is_inf, 1)

    def mul(self, aff, is_inf, k: int):
        return orc.scalar_mul(self.g, aff, is_inf, fr_limbs([k])[0])

    def scale(self, p, k: int):
        aff, is_inf = orc.jac_to_affine(self.g, p)
        return self.mul(aff, is_inf, k)

    def add(self, a, b):
        return orc.jac_add(self.g, a, b)

    def neg(self, p):
        aff, is_inf = orc.jac_to_affine(self.g, p)
        aff = np.array(aff)
        aff[self.aw // 2:] = orc.fq_neg(aff[self.aw // 2:])
        return self.from_affine(aff, is_inf)

    def sub(self, a, b):
        return self.add(a, self.neg(b))

    def sum(self, ps):
        acc = self.inf
        for p in ps:
            acc = self.add(acc, p)
        return acc

    def is_inf(self, p) -> bool:
        return orc.jac_to_affine(self.g, p)[1]

    def lanes_in(self, pts, inf):
        """(L, n, AW) limbs + (L, n) flags -> lanes of Jacobian points"""
        return [[self.from_affine(pts[ln, i], bool(inf[ln, i])) for i in range(pts.shape[1])] for ln in range(pts.shape[0])]

    def lanes_out(self, lanes):
        """lanes of Jacobian points -> ((L, n, AW), (L, n)) as the library writes them"""
        L, n = len(lanes), len(lanes[0])
        pts, inf = np.zeros((L, n, self.aw), np.uint64), np.zeros((L, n), np.uint8)
        for ln in range(L):
            for i in range(n):
                aff, is_inf = orc.jac_to_affine(self.g, lanes[ln][i])
                pts[ln, i], inf[ln, i] = aff, is_inf
                if is_inf:
                    pts[ln, i] = 0
                    pts[ln, i, self.aw // 2:] = one_y(self.g)
        return pts, inf


def scale_points(C: Curve, S: Scheme, s, o, tx, ty, tz):
    """group.rs:70-109 party by party; s, tx, tz: lanes of Jacobian points, o, ty: lanes of ints -> (lanes of points, elements whose MAC checks fail)"""
    n, P, lpp = len(s[0]), S.parties, S.lpp
    out, bad = [[None] * n for _ in range(S.lanes)], 0
    for i in range(n):
        masked = [C.add(s[ln][i], tx[ln][i]) for ln in range(S.lanes)]                    # t.add(&x)
        sx = C.sum(masked[lpp * p] for p in range(P))                                     # .open(): broadcast, sum (spdz.rs:385-391)
        oy = sum(o[lpp * p][i] + ty[lpp * p][i] for p in range(P)) % R_MOD
        if lpp == 2:
            dx = C.sum(C.sub(C.scale(sx, S.mac_shares[p]), masked[2 * p + 1]) for p in range(P))      # :392-402
            do = sum(S.mac_shares[p] * oy - (o[2 * p + 1][i] + ty[2 * p + 1][i]) for p in range(P)) % R_MOD
            bad += (not C.is_inf(dx)) or do != 0
        shift = C.scale(sx, oy)                                                           # sx *= oy
        for p in range(P):
            for ln in range(lpp):
                at = lpp * p + ln
                r = C.sub(tz[at][i], C.scale(sx, ty[at][i]))                              # out.sub(scale_pub_group(sx, y))
                r = C.sub(r, C.scale(tx[at][i], oy))                                      # out.sub(x.scale_pub_scalar(oy))
                if ln == 0 and p == 0:
                    r = C.add(r, shift)                                                   # the king's sh
                if ln == 1:
                    r = C.add(r, C.scale(shift, S.mac_shares[p]))                         # mac += mac_share * other (:430-438)
                out[at][i] = r
    return out, bad


def gsz_mult_points(C: Curve, D: G.Domain, deg: int, x, y, gr, gr2):
    """:1112-1130 with the king's open in the exponent; x: lanes of ints; y, gr, gr2: lanes of Jacobian points -> (lanes of points, elements over the bound)"""
    n, P = len(x[0]), D.parties
    out, bad = [[None] * n for _ in range(P)], 0
    for i in range(n):
        d = [C.add(C.scale(y[j][i], x[j][i]), gr2[j][i]) for j in range(P)]               # y_cp.val *= x.val; += r2.val
        coeff = [C.sum(C.scale(d[j], D.inv_tab[j][k]) for j in range(P)) for k in range(P)]
        bad += any(not C.is_inf(coeff[k]) for k in range(2 * deg + 1, P))
        for j in range(P):
            out[j][i] = C.sub(coeff[0], gr[j][i])                                         # shift_res.val -= r.val
    return out, bad


def check_points(C: Curve, D: G.Domain, deg: int, xs, ys, zs, gr, gr2, fr, fr2, rands):
    """hadamard_check (:1334-1349) -> ip_check (:1280-1329) with ip_compress (:1160-1275) and ip_compute (:1132-1155) inline, on curve points: xs, fr,
    fr2, rands lanes of ints; ys, zs, gr, gr2 lanes of Jacobian points -> (verdict, degree violations).  The field steps are gsz_mul_model's."""
    P, fsrc, gk = D.parties, G.Material(fr, fr2, rands), [0]

    def open_pts(vals, bound):
        coeff = [C.sum(C.scale(vals[j], D.inv_tab[j][k]) for j in range(P)) for k in range(P)]
        return coeff[0], int(any(not C.is_inf(coeff[k]) for k in range(bound + 1, P)))

    def king(sent):                                                    # += r2, king_compute at 2 deg, -= r (:1145-1153, :1117-1124)
        k = gk[0]
        gk[0] += 1
        v, b = open_pts([C.add(s, ln[k]) for s, ln in zip(sent, gr2)], 2 * deg)
        return [C.sub(v, ln[k]) for ln in gr], b

    def ip_compute(xl, yl):
        return king([C.sum(C.scale(p, a) for a, p in zip(lx, ly)) for lx, ly in zip(xl, yl)])

    rho, bad = G.coin(D, deg, fsrc)
    n = len(xs[0])
    pw = [pow(rho, i, R_MOD) for i in range(n)]
    xs = [[a * p % R_MOD for a, p in zip(ln, pw)] for ln in xs]
    ip = [C.sum(C.scale(z, p) for z, p in zip(ln, pw)) for ln in zs]
    ys = [list(ln) for ln in ys]
    while len(xs[0]) > 1:
        if len(xs[0]) % 2:
            for lx, ly in zip(xs, ys):
                lx.append(0)
                ly.append(C.inf)
        h = len(xs[0]) // 2
        xl, xr, yl, yr = [ln[:h] for ln in xs], [ln[h:] for ln in xs], [ln[:h] for ln in ys], [ln[h:] for ln in ys]
        ip_l, b = ip_compute(xl, yl)
        bad += b
        ip_r = [C.sub(a, c) for a, c in zip(ip, ip_l)]
        x3 = [[(2 * r - l) % R_MOD for l, r in zip(ll, lr)] for ll, lr in zip(xl, xr)]
        y3 = [[C.sub(C.add(r, r), l) for l, r in zip(ll, lr)] for ll, lr in zip(yl, yr)]
        ip3, b = ip_compute(x3, y3)
        bad += b
        c, b = G.coin(D, deg, fsrc)
        bad += b
        xs = [[((r - l) * c + 2 * l - r) % R_MOD for l, r in zip(ll, lr)] for ll, lr in zip(xl, xr)]
        ys = [[C.add(C.scale(C.sub(r, l), c), C.sub(C.add(l, l), r)) for l, r in zip(ll, lr)] for ll, lr in zip(yl, yr)]
        inv2 = pow(2, -1, R_MOD)
        f1, f2, f3 = (c - 2) * (c - 3) * inv2 % R_MOD, -(c - 1) * (c - 3) % R_MOD, (c - 1) * (c - 2) * inv2 % R_MOD
        ip = [C.sum([C.scale(ip_l[j], f1), C.scale(ip_r[j], f2), C.scale(ip3[j], f3)]) for j in range(P)]
    xr, yr = [ln[0] for ln in fsrc.rand(1)], [ln[0] for ln in fsrc.rand(1)]
    x, y = [ln[0] for ln in xs], [ln[0] for ln in ys]
    ipr, b = G.mult(D, deg, xr, yr, fsrc)
    bad += b
    xb, b = G.mult(D, deg, x, xr, fsrc)
    bad += b
    yb, b = king([C.scale(y[j], yr[j]) for j in range(P)])
    bad += b
    zb, b = king([C.scale(ip[j], ipr[j]) for j in range(P)])
    bad += b
    xo, b = D.open(xb, deg)
    bad += b
    yo, b = open_pts(yb, deg)
    bad += b
    zo, b = open_pts(zb, deg)
    return C.is_inf(C.sub(C.scale(yo, xo), zo)), bad + b
