"""Big-integer model of the reference's point serialization (TEST INFRASTRUCTURE ONLY): square roots in Fq and Fq2, the `Ord` rules,
GroupAffine's CanonicalSerialize / CanonicalDeserialize, `Vec`s and the three Groth16 structs.  Constants come from oracle/pyref.py.

Anchors (relative to the reference root):
  * Tonelli-Shanks as written ........ algebra/ff/src/fields/arithmetic.rs:259-320
  * complex-method Fq2 root .......... algebra/ff/src/fields/models/quadratic_extension.rs:360-399
  * Ord of Fq2 (c1, then c0) ......... quadratic_extension.rs:412-418
  * SWFlags .......................... algebra/serialize/src/flags.rs:110-135
  * point encode / decode ............ algebra/ec/src/models/short_weierstrass_jacobian.rs:108-118, 792-895
  * Vec ............................. algebra/serialize/src/lib.rs:220-229
  * Groth16 structs .................. groth16/src/data_structures.rs:11-18, 43-54, 132-149

Values are canonical Python integers (Fq) or pairs (Fq2); a point is (x, y) or pyref.INF.  The library's root rule (the root y with y <= -y) is
`smaller_root`; `fq_sqrt_reference` / `fq2_sqrt_reference` return whichever root the reference's algorithm lands on.
"""
import numpy as np

from pyref import (F1, F2, FQ_GENERATOR_LIMBS, FQ_MONT_R, FQ_T, FQ_TWO_ADIC_ROOT_LIMBS, FQ_TWO_ADICITY, FQ2_NONRESIDUE, G1_B, G1_GEN, G2_B, G2_GEN, INF, Q_MOD,
                   R_MOD, ec_mul, ec_on_curve, fq2_mul, fq_from_mont, limbs_to_int)

Q = Q_MOD
FQ_TWO_ADIC_ROOT = fq_from_mont(limbs_to_int(FQ_TWO_ADIC_ROOT_LIMBS))
FQ_GENERATOR = fq_from_mont(limbs_to_int(FQ_GENERATOR_LIMBS))
OK, BAD_FLAGS, NOT_CANONICAL, NO_POINT, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(6)
BAD = "bad"   # a failing point in a decoded list (pyref.INF, the point at infinity, is None)
FIELD = {1: F1, 2: F2}
CURVE_B = {1: G1_B, 2: G2_B}
GEN = {1: G1_GEN, 2: G2_GEN}


# ----------------------------------------------------------------------------- square roots
def fq_sqrt_reference(a):
    """sqrt_impl!: Tonelli-Shanks with the reference's loops; None when a is a non-residue"""
    a %= Q
    if a == 0:
        return 0
    z = FQ_TWO_ADIC_ROOT
    w = pow(a, (FQ_T - 1) // 2, Q)
    x = w * a % Q
    b = x * w % Q
    v = FQ_TWO_ADICITY
    while b != 1:
        k, b2k = 0, b
        while b2k != 1:
            b2k = b2k * b2k % Q
            k += 1
        if k == FQ_TWO_ADICITY:
            return None
        w = z
        for _ in range(1, v - k):
            w = w * w % Q
        z = w * w % Q
        b = b * z % Q
        x = x * w % Q
        v = k
    return x if x * x % Q == a else None


def fq2_sqrt_reference(a):
    """QuadExtField::sqrt, the complex method.  Where c1 = 0 and c0 is a non-residue of Fq the reference answers None although the element is a
    square in Fq2 (every element of Fq is): this model returns the root (0, sqrt(c0 / beta)) there, as the library does."""
    c0, c1 = a[0] % Q, a[1] % Q
    if c1 == 0:
        r = fq_sqrt_reference(c0)
        if r is not None:
            return (r, 0)
        r = fq_sqrt_reference(c0 * pow(FQ2_NONRESIDUE, -1, Q) % Q)
        return None if r is None else (0, r)
    alpha = fq_sqrt_reference((c0 * c0 - FQ2_NONRESIDUE * c1 * c1) % Q)   # sqrt(norm)
    if alpha is None:
        return None
    two_inv = pow(2, -1, Q)
    delta = (alpha + c0) * two_inv % Q
    if pow(delta, (Q - 1) // 2, Q) == Q - 1:   # legendre().is_qnr()
        delta = (delta - alpha) % Q
    x0 = fq_sqrt_reference(delta)
    if x0 is None or x0 == 0:
        return None
    cand = (x0, c1 * two_inv * pow(x0, -1, Q) % Q)
    return cand if fq2_mul(cand, cand) == (c0, c1) else None


def f_neg(ext, a):
    return (-a) % Q if ext == 1 else ((-a[0]) % Q, (-a[1]) % Q)


def f_gt(ext, a, b):
    """a > b in the reference's Ord: Fq by value, Fq2 by c1 and then c0"""
    return a > b if ext == 1 else (a[1], a[0]) > (b[1], b[0])


def smaller_root(ext, y):
    """the library's rule: of y and -y the one with y <= -y"""
    return f_neg(ext, y) if f_gt(ext, y, f_neg(ext, y)) else y


def f_sqrt(ext, a):
    """(exists, root by the library's rule or zero)"""
    r = fq_sqrt_reference(a) if ext == 1 else fq2_sqrt_reference(a)
    zero = 0 if ext == 1 else (0, 0)
    return (False, zero) if r is None else (True, smaller_root(ext, r))


# ----------------------------------------------------------------------------- limbs
def fq_mont_limbs(v):
    v = v * FQ_MONT_R % Q
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]


def f_mont_limbs(ext, a):
    return fq_mont_limbs(a) if ext == 1 else fq_mont_limbs(a[0]) + fq_mont_limbs(a[1])


def f_from_limbs(ext, limbs):
    vals = [fq_from_mont(limbs_to_int(limbs[6 * i:6 * i + 6])) for i in range(ext)]
    return vals[0] if ext == 1 else tuple(vals)


def points_to_arrays(group, pts):
    """[(x, y) | INF | BAD (a failing point: zero coordinates, flag 0)] -> ((n, 12|24) uint64 Montgomery limbs, (n,) uint8 infinity flags); infinity
    is written (0, 1), as every array of the library holds it"""
    F = FIELD[group]
    arr = np.zeros((len(pts), 12 * group), dtype=np.uint64)
    inf = np.zeros(len(pts), dtype=np.uint8)
    for i, P in enumerate(pts):
        if P == BAD:
            continue
        x, y = (F.zero, F.one) if P is INF else P
        inf[i] = 1 if P is INF else 0
        arr[i] = f_mont_limbs(group, x) + f_mont_limbs(group, y)
    return arr, inf


# ----------------------------------------------------------------------------- points
def _fq_bytes(v, flags=0):
    assert 0 <= v < Q
    return (v | flags << 376).to_bytes(48, "little")


def _f_bytes(ext, a, flags=0):
    return _fq_bytes(a, flags) if ext == 1 else _fq_bytes(a[0]) + _fq_bytes(a[1], flags)


def point_size(group, compressed=True):
    return 48 * group * (1 if compressed else 2)


def encode_point(group, P, compressed=True):
    """GroupAffine::serialize / serialize_uncompressed; P = (x, y), or INF (written as zero() = (0, 1, infinity))"""
    F = FIELD[group]
    if P is INF:
        return _f_bytes(group, F.zero, 0x40) if compressed else _f_bytes(group, F.zero) + _f_bytes(group, F.one, 0x40)
    x, y = P
    if compressed:
        return _f_bytes(group, x, 0x80 if f_gt(group, y, f_neg(group, y)) else 0)
    return _f_bytes(group, x) + _f_bytes(group, y)


def _f_read(ext, data, flagged):
    """(value or None when a limb group is >= q, flag bits of the last byte); only the last Fq of a flagged element has its bits removed"""
    vals = []
    flags = data[-1] & 0xC0 if flagged else 0
    for i in range(ext):
        v = int.from_bytes(data[48 * i:48 * i + 48], "little")
        if flagged and i == ext - 1:
            v &= (1 << 382) - 1
        vals.append(v)
    if any(v >= Q for v in vals):
        return None, flags
    return (vals[0] if ext == 1 else tuple(vals)), flags


def decode_point(group, data, compressed=True, checked=True):
    """(status, point): the point is (x, y), INF, or BAD for a failing one -- the library's statuses in the library's order
    (include/czk.h czk_points_deserialize)"""
    F, b = FIELD[group], CURVE_B[group]
    fs = 48 * group
    assert len(data) == point_size(group, compressed)
    if data[-1] & 0xC0 == 0xC0:
        return BAD_FLAGS, BAD
    x, flags = _f_read(group, data[:fs], compressed)
    y = None
    if not compressed:
        y, flags = _f_read(group, data[fs:], True)
        if y is None:
            return NOT_CANONICAL, BAD
    if x is None:
        return NOT_CANONICAL, BAD
    if flags & 0x40:
        return OK, INF
    if compressed:
        exists, y = f_sqrt(group, F.add(F.mul(x, F.mul(x, x)), b))
        if not exists:
            return NO_POINT, BAD
        if flags & 0x80:
            y = f_neg(group, y)
    elif checked and not ec_on_curve(F, (x, y), b):
        return NOT_ON_CURVE, BAD
    if checked and ec_mul(F, R_MOD, (x, y)) is not INF:
        return NOT_IN_SUBGROUP, BAD
    return OK, (x, y)


def encode_points(group, pts, compressed=True):
    return b"".join(encode_point(group, P, compressed) for P in pts)


def decode_points(group, data, compressed=True, checked=True):
    """([status], [point], number bad, first bad index or n)"""
    size = point_size(group, compressed)
    res = [decode_point(group, data[i:i + size], compressed, checked) for i in range(0, len(data), size)]
    st = [r[0] for r in res]
    bad = [i for i, s in enumerate(st) if s != OK]
    return st, [r[1] for r in res], len(bad), (bad[0] if bad else len(st))


# ----------------------------------------------------------------------------- Vec and the Groth16 structs
def encode_vec(group, pts, compressed=True):
    return len(pts).to_bytes(8, "little") + encode_points(group, pts, compressed)


VK_FIELDS = (("alpha_g1", 1, False), ("beta_g2", 2, False), ("gamma_g2", 2, False), ("delta_g2", 2, False), ("gamma_abc_g1", 1, True))
PK_FIELDS = VK_FIELDS + (("beta_g1", 1, False), ("delta_g1", 1, False), ("a_query", 1, True), ("b_g1_query", 1, True), ("b_g2_query", 2, True),
                         ("h_query", 1, True), ("l_query", 1, True))
PROOF_FIELDS = (("a", 1, False), ("b", 2, False), ("c", 1, False))


def encode_struct(fields, obj, compressed=True):
    """obj: {field: point | [points]} in model form"""
    return b"".join(encode_vec(g, obj[name], compressed) if is_vec else encode_point(g, obj[name], compressed) for name, g, is_vec in fields)


def arrays_to_points(group, arr, inf=None):
    """the inverse of points_to_arrays for valid points"""
    arr = np.asarray(arr, dtype=np.uint64).reshape(-1, 12 * group)
    out = []
    for i in range(arr.shape[0]):
        if inf is not None and inf[i]:
            out.append(INF)
            continue
        row = [int(v) for v in arr[i]]
        out.append((f_from_limbs(group, row[:6 * group]), f_from_limbs(group, row[6 * group:])))
    return out


def key_to_model(fields, key):
    """a groth16_setup style dict (numpy arrays) -> the model form encode_struct takes"""
    out = {}
    for name, g, is_vec in fields:
        out[name] = arrays_to_points(g, *key[name]) if is_vec else arrays_to_points(g, key[name])[0]
    return out
