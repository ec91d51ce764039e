"""The host-side contract of the point, fixed-base, codec, pairing and KZG entry points (csrc/point_ops.hip, fixed_base.hip, point_codec.hip,
pairing.hip, kzg.hip), through the C ABI itself: what each call answers when exactly one argument is wrong (code AND message), that an empty call
touches nothing, and that every kind of caller gets the same values -- host or device memory, optional output flags taken or not, optional
input flags given or null -- at n = 1 and at one item more than the unit's block (129; 65 for the pairing kernels), the segmented calls with
three segments of which the middle one is empty.  Expected values come from the affine big-integer group law and the pairing of
tests/pairing_ref.py, the codec of tests/point_codec_ref.py and, for the KZG verdicts, the known-beta identity over the openings' discrete
logarithms (tests/test_kzg.py); never from the library.
The matrix is run whole: tests/test_point_ops.py, test_fixed_base.py, test_point_codec.py, test_pairing.py and test_kzg.py cover the cell "host
memory, every optional array given" at sizes that cross a block too, but not at exactly these, and the cell costs milliseconds here.  fq_sqrt,
whose outputs are all required, is run in device memory only (host memory: tests/test_point_codec.py, n up to 257).
The last section does the same for the pointwise Fr calls (csrc/fr_vec.hip: values from Python integers, n = 1 and 257) and pins the rejections and
empty calls of the radix-2 transforms (csrc/ntt.hip) and of the Groth16 witness map (csrc/witness_map.hip)."""
import ctypes as C

import numpy as np
import pytest

import pairing_ref as P
import point_codec_ref as R
from util import R_MOD, ints_to_limbs

pytestmark = pytest.mark.gpu
HOST, DEV, ERR_ARG = 0, 1, 3
FLD = {1: P.F1, 2: P.F2}
GEN = {1: P.G1_GEN, 2: P.G2_GEN}
N_ROWS = 130                                   # rows [1, 1 + n) are used: row 1 carries a flag on either side, so n = 1 sees the flags
SIZES = {"points": (1, 129), "pairing": (1, 65)}
BIG = (1 << 252) + 0x1234567                   # a 253-bit scalar below r
SCALARS = (0, 1, R_MOD - 1, BIG)
GROUP_MSG, MEM_MSG = "group must be CZK_G1 or CZK_G2", "mem must be CZK_MEM_HOST or CZK_MEM_DEVICE"

# name -> (argument names after the context, kinds: i int, u unsigned, z size_t, p pointer)
ABI = {
    "czk_points_add": ("group a a_inf b b_inf n negate_b out out_inf mem", "ippppzippi"),
    "czk_points_mul": ("group pts inf pts_stride scalars n scalar_form out out_inf mem", "ippzpzippi"),
    "czk_points_sum": ("group pts inf offsets k out out_inf mem", "ipppzppi"),
    "czk_fixed_base_create": ("group base window n_hint out", "ipuzp"),
    "czk_fixed_base_msm": ("fb scalars n scalar_form out out_inf mem", "ppzippi"),
    "czk_fq_sqrt": ("ext a n out out_exists mem", "ipzppi"),
    "czk_points_serialize": ("group pts inf n compressed out mem", "ippzipi"),
    "czk_points_deserialize": ("group bytes n flags out_pts out_inf out_status out_bad out_first_bad mem", "ipzipppppi"),
    "czk_pairing": ("g1 g1_inf g2 g2_inf n out mem", "ppppzpi"),
    "czk_pairing_product": ("g1 g1_inf g2 g2_inf offsets k out out_is_one mem", "pppppzppi"),
    "czk_groth16_pvk_create": ("alpha beta gamma delta gamma_abc gamma_abc_inf n_gamma_abc out", "ppppppzp"),
    "czk_groth16_verify": ("pvk a b c inf public_inputs m k out_ok mem", "ppppppzzpi"),
    "czk_kzg10_vk_create": ("g gamma_g h beta_h out", "ppppp"),
    "czk_kzg10_check": ("vk comm comm_inf points values w w_inf random_v k out_ok mem", "ppppppppzpi"),
    "czk_kzg10_batch_check": ("vk comm comm_inf points values w w_inf random_v randomizers offsets b out_ok mem", "ppppppppppzpi"),
    # the pointwise Fr calls (fr_vec.hip), the radix-2 transforms (ntt.hip) and the Groth16 witness map (witness_map.hip)
    "czk_fr_vec_op": ("op a b out n mem", "ipppzi"),
    "czk_fr_vec_scale": ("a k out n mem", "pppzi"),
    "czk_fr_beaver_combine": ("x y z sx oy add_open out n mem", "pppppipzi"),
    "czk_fr_spdz_open": ("shares parties n out_value out_bad", "pzzpp"),
    "czk_fr_into_repr": ("a out n mem", "ppzi"),
    "czk_fr_from_repr": ("a out n mem", "ppzi"),
    "czk_spdz_open_combine": ("a b tx ty tz parties king_mask sx oy chk_a chk_b ab n", "pppppzqpppppz"),
    "czk_ntt_fr": ("data log_d lanes kind in_len mem", "puzizi"),
    "czk_ntt_fr_to": ("src src_stride dst log_d lanes kind in_len mem", "pzpuzizi"),
    "czk_witness_map_pre": ("a a_len b b_len log_d lanes", "pzpzuz"),
    "czk_witness_map_pre_masked": ("a a_len b b_len mask_a mask_b log_d lanes", "pzpzppuz"),
    "czk_witness_map_post": ("ab c c_len log_d lanes", "ppzuz"),
    "czk_witness_map_post_h": ("ab c c_len log_d lanes", "ppzuz"),
}
_CT = {"i": C.c_int, "u": C.c_uint, "z": C.c_size_t, "q": C.c_uint64}


def _ptr(x):
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data_as(C.c_void_p)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return x if isinstance(x, (C.c_void_p, type(C.byref(C.c_void_p())))) else C.c_void_p(int(x))


def call(ctx, name, **kw):
    """(return code, the context's message) of one call of the C ABI; every argument by name"""
    names, kinds = ABI[name][0].split(), ABI[name][1]
    assert sorted(kw) == sorted(names), (name, sorted(set(kw) ^ set(names)))
    args = [_ptr(kw[n]) if k == "p" else _CT[k](kw[n]) for n, k in zip(names, kinds)]
    rc = getattr(ctx._L, name)(ctx._h, *args)
    return rc, (ctx._L.czk_last_error(ctx._h) or b"").decode()


def ok(ctx, name, **kw):
    rc, msg = call(ctx, name, **kw)
    assert rc == 0, (name, rc, msg)


class Mem:
    """buffers of one kind of caller: numpy arrays (host) or torch tensors on the context's GPU (device)"""

    def __init__(self, ctx, mem):
        self.ctx, self.mem = ctx, mem

    def put(self, a):
        if a is None or self.mem == HOST:
            return None if a is None else np.ascontiguousarray(a)
        import torch
        a = np.array(a)                        # (a writable copy: frombuffer arrays are not)
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", self.ctx.device))

    def out(self, shape, dtype=np.uint64):
        return self.put(np.full(shape, 0xA5, dtype=np.uint8).view(dtype) if dtype == np.uint8 else np.full(shape, 0xA5A5A5A5A5A5A5A5, dtype=dtype))

    def get(self, x):
        if self.mem == HOST:
            return x
        self.ctx.sync()
        a = x.cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a


def limbs(group, points):
    """(points (n, 12|24), flags (n,)); infinity is written (0, 1)"""
    f = P.g1_to_limbs if group == 1 else P.g2_to_limbs
    rows = [f(p) for p in points]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(-1, 12 * group), np.array([r[1] for r in rows], dtype=np.uint8)


def mont(vals):
    return ints_to_limbs([v % R_MOD * (1 << 256) % R_MOD for v in vals], 4)


def offsets(vals):
    return np.array(vals, dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    """Everything the expected values are made of, computed once: per group five points, the rows' flags, and the memoised group law"""
    d = {"pts": {g: [P.ec_mul(FLD[g], k, GEN[g]) for k in (1, 2, 3, 5, 7)] for g in (1, 2)}, "mul": {}}
    d["fa"] = np.array([i % 4 == 1 for i in range(N_ROWS)], dtype=np.uint8)   # flags of the first / only point array
    d["fb"] = np.array([i % 6 == 1 for i in range(N_ROWS)], dtype=np.uint8)   # flags of the second one
    return d


def rows(data, group, step, shift):
    return [data["pts"][group][(step * i + shift) % 5] for i in range(N_ROWS)]


def eff(points, flags, given):
    """the points a call sees: a flagged row is infinity whatever its limbs, a null flag array means none is"""
    return [P.INF if given and f else p for p, f in zip(points, flags)]


def mul(data, group, k, p):
    key = (group, k, p)
    if key not in data["mul"]:
        data["mul"][key] = P.ec_mul(FLD[group], k, p)
    return data["mul"][key]


def fold(group, points):
    acc = P.INF
    for p in points:
        acc = P.ec_add(FLD[group], acc, p)
    return acc


def check_points(group, m, out, out_inf, want):
    w_pts, w_inf = limbs(group, want)
    assert np.array_equal(m.get(out).reshape(-1, 12 * group), w_pts)
    if out_inf is not None:
        assert np.array_equal(m.get(out_inf), w_inf)


OPTIONAL_CELLS = [(o, i) for o in (True, False) for i in (True, False)]   # (take the optional output, give the optional inputs)


# ------------------------------------------------------------------------------------------------- the memory matrix: point_ops.hip
@pytest.mark.parametrize("n", SIZES["points"])
@pytest.mark.parametrize("mem", [HOST, DEV])
@pytest.mark.parametrize("group", [1, 2])
def test_matrix_points_add_mul(ctx, data, group, mem, n):
    m, F, sl = Mem(ctx, mem), FLD[group], slice(1, 1 + n)
    a, b = rows(data, group, 1, 0), rows(data, group, 2, 1)
    ks = [SCALARS[i % 4] for i in range(N_ROWS)]
    la, lb, lk = limbs(group, a)[0][sl], limbs(group, b)[0][sl], ints_to_limbs(ks, 4)[sl]
    for take, given in OPTIONAL_CELLS:
        fa, fb = (data["fa"][sl], data["fb"][sl]) if given else (None, None)
        ea, eb = eff(a, data["fa"], given)[sl], eff(b, data["fb"], given)[sl]
        out, oi = m.out((n, 12 * group)), m.out(n, np.uint8) if take else None
        ok(ctx, "czk_points_add", group=group, a=m.put(la), a_inf=m.put(fa), b=m.put(lb), b_inf=m.put(fb), n=n, negate_b=1, out=out, out_inf=oi, mem=mem)
        check_points(group, m, out, oi, [P.ec_add(F, x, P.ec_neg(F, y)) for x, y in zip(ea, eb)])
        for stride in (1, 0):
            out, oi = m.out((n, 12 * group)), m.out(n, np.uint8) if take else None
            np_ = n if stride else 1
            ok(ctx, "czk_points_mul", group=group, pts=m.put(la[:np_]), inf=m.put(fa[:np_] if given else None), pts_stride=stride, scalars=m.put(lk), n=n,
               scalar_form=0, out=out, out_inf=oi, mem=mem)
            check_points(group, m, out, oi, [mul(data, group, k, ea[i if stride else 0]) for i, k in enumerate(ks[sl])])


@pytest.mark.parametrize("offs", [[0, 1], [0, 65, 65, 129]], ids=["k1", "k3_empty_middle"])
@pytest.mark.parametrize("mem", [HOST, DEV])
@pytest.mark.parametrize("group", [1, 2])
def test_matrix_points_sum(ctx, data, group, mem, offs):
    m, n, k = Mem(ctx, mem), offs[-1], len(offs) - 1
    a = rows(data, group, 1, 0)
    la = limbs(group, a)[0][1:1 + n]
    for take, given in OPTIONAL_CELLS:
        ea = eff(a, data["fa"], given)[1:1 + n]
        out, oi = m.out((k, 12 * group)), m.out(k, np.uint8) if take else None
        ok(ctx, "czk_points_sum", group=group, pts=m.put(la), inf=m.put(data["fa"][1:1 + n] if given else None), offsets=offsets(offs), k=k, out=out, out_inf=oi,
           mem=mem)
        check_points(group, m, out, oi, [fold(group, ea[offs[j]:offs[j + 1]]) for j in range(k)])


# ------------------------------------------------------------------------------------------------- fixed_base.hip
@pytest.fixture(scope="module")
def fixed_bases(ctx, data):
    """czk_fixed_base_create: a table of window 3 over [2] G per group"""
    hs = {}
    for group in (1, 2):
        h = C.c_void_p(0)
        ok(ctx, "czk_fixed_base_create", group=group, base=limbs(group, [data["pts"][group][1]])[0], window=3, n_hint=0, out=C.byref(h))
        hs[group] = h
    yield hs
    for h in hs.values():
        ctx._L.czk_fixed_base_release(h)


@pytest.mark.parametrize("n", SIZES["points"])
@pytest.mark.parametrize("mem", [HOST, DEV])
@pytest.mark.parametrize("group", [1, 2])
def test_matrix_fixed_base_msm(ctx, data, fixed_bases, group, mem, n):
    m = Mem(ctx, mem)
    ks = [SCALARS[i % 4] for i in range(1, 1 + n)]
    for take in (True, False):
        out, oi = m.out((n, 12 * group)), m.out(n, np.uint8) if take else None
        ok(ctx, "czk_fixed_base_msm", fb=fixed_bases[group], scalars=m.put(ints_to_limbs(ks, 4)), n=n, scalar_form=0, out=out, out_inf=oi, mem=mem)
        check_points(group, m, out, oi, [mul(data, group, k, data["pts"][group][1]) for k in ks])


# ------------------------------------------------------------------------------------------------- point_codec.hip
@pytest.mark.parametrize("n", SIZES["points"])
@pytest.mark.parametrize("ext", [1, 2])
def test_matrix_fq_sqrt(ctx, ext, n):
    """device memory (host memory: tests/test_point_codec.py at n up to 257); both outputs are required"""
    m = Mem(ctx, DEV)
    vals = [0, 4, 5, 7, 11, 13] if ext == 1 else [(0, 0), (4, 0), (3, 5), (1, 1), (0, 2), (7, 0)]
    want = [R.f_sqrt(ext, v) for v in vals]
    assert {w[0] for w in want} == {True, False}
    idx = [i % len(vals) for i in range(1, 1 + n)]
    a = np.array([R.f_mont_limbs(ext, vals[i]) for i in idx], dtype=np.uint64)
    out, ex = m.out((n, 6 * ext)), m.out(n, np.uint8)
    ok(ctx, "czk_fq_sqrt", ext=ext, a=m.put(a), n=n, out=out, out_exists=ex, mem=DEV)
    assert np.array_equal(m.get(out), np.array([R.f_mont_limbs(ext, want[i][1]) for i in idx], dtype=np.uint64))
    assert list(m.get(ex)) == [int(want[i][0]) for i in idx]


@pytest.mark.parametrize("n", SIZES["points"])
@pytest.mark.parametrize("mem", [HOST, DEV])
@pytest.mark.parametrize("group", [1, 2])
def test_matrix_points_serialize(ctx, data, group, mem, n):
    m, a, sl = Mem(ctx, mem), rows(data, group, 1, 0), slice(1, 1 + n)
    la = limbs(group, a)[0][sl]
    for given in (True, False):
        for compressed in (1, 0):
            out = m.out(n * R.point_size(group, bool(compressed)), np.uint8)
            ok(ctx, "czk_points_serialize", group=group, pts=m.put(la), inf=m.put(data["fa"][sl] if given else None), n=n, compressed=compressed, out=out, mem=mem)
            assert m.get(out).tobytes() == R.encode_points(group, eff(a, data["fa"], given)[sl], bool(compressed))


@pytest.fixture(scope="module")
def encoded(data):
    """per (group, compressed): the rows' bytes with row 2 spoilt (both flag bits set), and what point_codec_ref decodes from them (unchecked; checked
    where it costs one [r] P per distinct row)"""
    out, memo = {}, {}
    for group in (1, 2):
        pts = eff(rows(data, group, 1, 0), data["fa"], True)
        for compressed in (True, False):
            size = R.point_size(group, compressed)
            raw = bytearray(R.encode_points(group, pts, compressed))
            raw[3 * size - 1] |= 0xC0
            for checked in (True, False):
                res = []
                for i in range(N_ROWS):
                    key = (group, compressed, checked, bytes(raw[i * size:(i + 1) * size]))
                    if key not in memo:
                        memo[key] = R.decode_point(group, key[3], compressed, checked)
                    res.append(memo[key])
                out[(group, compressed, checked)] = (np.frombuffer(bytes(raw), dtype=np.uint8).reshape(N_ROWS, size), res)
    return out


@pytest.mark.parametrize("n", SIZES["points"])
@pytest.mark.parametrize("mem", [HOST, DEV])
@pytest.mark.parametrize("group", [1, 2])
def test_matrix_points_deserialize(ctx, encoded, group, mem, n):
    m, sl = Mem(ctx, mem), slice(1, 1 + n)
    for (compressed, checked) in ((True, True), (False, False)):
        raw, res = encoded[(group, compressed, checked)]
        res = res[sl]
        w_pts, w_inf = R.points_to_arrays(group, [r[1] for r in res])
        bad = [i for i, r in enumerate(res) if r[0] != R.OK]
        assert len(bad) == (1 if n > 1 else 0)
        for status, count in OPTIONAL_CELLS:
            out, oi, st = m.out((n, 12 * group)), m.out(n, np.uint8), m.out(n, np.uint8) if status else None
            n_bad, first = C.c_size_t(77), C.c_size_t(77)
            ok(ctx, "czk_points_deserialize", group=group, bytes=m.put(raw[sl].reshape(-1)), n=n, flags=(1 if compressed else 0) | (2 if checked else 0), out_pts=out,
               out_inf=oi, out_status=st, out_bad=C.byref(n_bad) if count else None, out_first_bad=C.byref(first) if count else None, mem=mem)
            assert np.array_equal(m.get(out), w_pts) and np.array_equal(m.get(oi), w_inf)
            if status:
                assert list(m.get(st)) == [r[0] for r in res]
            if count:
                assert (n_bad.value, first.value) == (len(bad), bad[0] if bad else n)


# ------------------------------------------------------------------------------------------------- pairing.hip
@pytest.fixture(scope="module")
def pairs(data):
    """130 rows over three pairs (P_i, Q_i) and their pairings from pairing_ref"""
    p1, p2 = data["pts"][1][:3], data["pts"][2][2:5]
    return {"g1": [p1[i % 3] for i in range(N_ROWS)], "g2": [p2[i % 3] for i in range(N_ROWS)], "e": [P.pairing(x, y) for x, y in zip(p1, p2)]}


def pair_values(data, pairs, given):
    return [P.FQ12_ONE if given and (data["fa"][i] or data["fb"][i]) else pairs["e"][i % 3] for i in range(N_ROWS)]


def fq12_rows(vals):
    return np.array([P.fq12_to_limbs(v) for v in vals], dtype=np.uint64)


@pytest.mark.parametrize("n", SIZES["pairing"])
@pytest.mark.parametrize("mem", [HOST, DEV])
def test_matrix_pairing(ctx, data, pairs, mem, n):
    m, sl = Mem(ctx, mem), slice(1, 1 + n)
    g1, g2 = limbs(1, pairs["g1"])[0][sl], limbs(2, pairs["g2"])[0][sl]
    for given in (True, False):
        out = m.out((n, 72))
        ok(ctx, "czk_pairing", g1=m.put(g1), g1_inf=m.put(data["fa"][sl] if given else None), g2=m.put(g2), g2_inf=m.put(data["fb"][sl] if given else None), n=n,
           out=out, mem=mem)
        assert np.array_equal(m.get(out), fq12_rows(pair_values(data, pairs, given)[sl]))


@pytest.mark.parametrize("sizes", [[1], [2, 0, 1], [j % 3 for j in range(65)]], ids=["k1", "k3_empty_middle", "k65"])
@pytest.mark.parametrize("mem", [HOST, DEV])
def test_matrix_pairing_product(ctx, data, pairs, mem, sizes):
    m, k = Mem(ctx, mem), len(sizes)
    offs = [0] + list(np.cumsum(sizes))
    n = int(offs[-1])
    sl = slice(1, 1 + n)
    g1, g2 = limbs(1, pairs["g1"])[0][sl], limbs(2, pairs["g2"])[0][sl]
    for given in (True, False):
        vals = pair_values(data, pairs, given)[sl]
        want = []
        for j in range(k):
            acc = P.FQ12_ONE
            for v in vals[offs[j]:offs[j + 1]]:
                acc = P.fq12_mul(acc, v)
            want.append(acc)
        for take_out, take_one in ((True, True), (True, False), (False, True)):
            out, one = m.out((k, 72)) if take_out else None, m.out(k, np.uint8) if take_one else None
            ok(ctx, "czk_pairing_product", g1=m.put(g1), g1_inf=m.put(data["fa"][sl] if given else None), g2=m.put(g2),
               g2_inf=m.put(data["fb"][sl] if given else None), offsets=offsets(offs), k=k, out=out, out_is_one=one, mem=mem)
            if take_out:
                assert np.array_equal(m.get(out), fq12_rows(want))
            if take_one:
                assert list(m.get(one)) == [int(w == P.FQ12_ONE) for w in want]


@pytest.fixture(scope="module")
def groth16(ctx):
    """A key from known scalars, a proof that satisfies e(A, B) = e(alpha, beta) e(g_ic, gamma) e(C, delta) by construction and one with C moved;
    the verdicts of pairing_ref.verify_proof, with and without C flagged as infinity"""
    alpha, beta, gamma, delta, g0, g1, x, a, b = 11, 13, 17, 19, 23, 29, 31, 37, 41
    c = (a * b - alpha * beta - (g0 + x * g1) * gamma) * pow(delta, -1, R_MOD) % R_MOD
    pt = {"alpha": P.g1_mul(alpha), "beta": P.g2_mul(beta), "gamma": P.g2_mul(gamma), "delta": P.g2_mul(delta), "abc": [P.g1_mul(g0), P.g1_mul(g1)],
          "a": P.g1_mul(a), "b": P.g2_mul(b), "c": [P.g1_mul(c), P.g1_mul(c + 1)]}
    ab = P.pairing(pt["alpha"], pt["beta"])
    verdict = {(v, f): P.verify_proof(ab, pt["gamma"], pt["delta"], pt["abc"], pt["a"], pt["b"], P.INF if f else pt["c"][v], [x])
               for v in (0, 1) for f in (0, 1)}
    assert verdict[(0, 0)] and not verdict[(1, 0)] and not verdict[(0, 1)]
    h = C.c_void_p(0)
    ok(ctx, "czk_groth16_pvk_create", alpha=limbs(1, [pt["alpha"]])[0], beta=limbs(2, [pt["beta"]])[0], gamma=limbs(2, [pt["gamma"]])[0],
       delta=limbs(2, [pt["delta"]])[0], gamma_abc=limbs(1, pt["abc"])[0], gamma_abc_inf=None, n_gamma_abc=2, out=C.byref(h))
    yield {"pvk": h, "pt": pt, "x": x, "verdict": verdict}
    ctx._L.czk_groth16_pvk_release(h)


@pytest.mark.parametrize("k", SIZES["pairing"])
@pytest.mark.parametrize("mem", [HOST, DEV])
def test_matrix_groth16_verify(ctx, groth16, mem, k):
    m, pt = Mem(ctx, mem), groth16["pt"]
    variant = [int(i % 3 == 2) for i in range(1, 1 + k)]                 # 1: the proof with C moved
    c_flag = [int(i % 4 == 1) for i in range(1, 1 + k)]                  # row 1, the only row of k = 1, is the valid proof with C flagged
    a, b = np.repeat(limbs(1, [pt["a"]])[0], k, axis=0), np.repeat(limbs(2, [pt["b"]])[0], k, axis=0)
    c = limbs(1, [pt["c"][v] for v in variant])[0]
    inf = np.array([[0, 0, f] for f in c_flag], dtype=np.uint8)
    for given in (True, False):                                           # (test_pairing.py's proofs never carry flags: no cell is left out)
        out = m.out(k, np.uint8)
        ok(ctx, "czk_groth16_verify", pvk=groth16["pvk"], a=m.put(a), b=m.put(b), c=m.put(c), inf=m.put(inf if given else None),
           public_inputs=m.put(np.repeat(mont([groth16["x"]]), k, axis=0)), m=1, k=k, out_ok=out, mem=mem)
        assert list(m.get(out)) == [int(groth16["verdict"][(v, f if given else 0)]) for v, f in zip(variant, c_flag)]


# ------------------------------------------------------------------------------------------------- kzg.hip
BETA, GAMMA = 0x6B10_0001, 0x6B11_0003


@pytest.fixture(scope="module")
def kzg(ctx, data):
    """The verifier key of known beta, gamma and 130 openings over six templates (c, z, v, rv, w = (c - v - gamma rv) / (beta - z)): commitments
    [c] g and proofs [w] g.  Rows 70 and up with i % 3 == 1 claim v + 1.  An opening passes iff c - v - gamma rv + w (z - beta) == 0 for the
    values the call sees (0 for a point flagged infinite, rv = 0 without random_v); a batch iff the randomised sum of those residuals is 0."""
    tpl = []
    for t in range(6):
        c, z, v, rv = 1000 + 37 * t, 2000 + 41 * t, 3000 + 43 * t, (0 if t % 2 == 0 else 4000 + 47 * t)
        tpl.append({"c": c, "z": z, "v": v, "rv": rv, "w": (c - v - GAMMA * rv) * pow(BETA - z, -1, R_MOD) % R_MOD})
    pts = [(P.g1_mul(t["c"]), P.g1_mul(t["w"])) for t in tpl]
    o = [dict(tpl[i % 6], v=tpl[i % 6]["v"] + int(i >= 70 and i % 3 == 1)) for i in range(N_ROWS)]
    h = C.c_void_p(0)
    ok(ctx, "czk_kzg10_vk_create", g=limbs(1, [P.G1_GEN])[0], gamma_g=limbs(1, [P.g1_mul(GAMMA)])[0], h=limbs(2, [P.G2_GEN])[0],
       beta_h=limbs(2, [P.g2_mul(BETA)])[0], out=C.byref(h))
    # the identity itself, once against pairing_ref: an honest opening and the same with v + 1
    t = tpl[1]
    for dv, want in ((0, True), (1, False)):
        inner = P.g1_add(pts[1][0], P.ec_neg(P.F1, P.g1_add(P.g1_mul(t["v"] + dv), P.g1_mul(GAMMA * t["rv"]))))
        q = P.ec_add(P.F2, P.g2_mul(t["z"]), P.ec_neg(P.F2, P.g2_mul(BETA)))
        assert (P.product_of_pairings([(inner, P.G2_GEN), (pts[1][1], q)]) == P.FQ12_ONE) == want
    yield {"vk": h, "rows": o, "comm": limbs(1, [pts[i % 6][0] for i in range(N_ROWS)])[0], "w": limbs(1, [pts[i % 6][1] for i in range(N_ROWS)])[0],
           "r": [(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 128) for i in range(N_ROWS)]}
    ctx._L.czk_kzg10_vk_release(h)


def residual(data, o, i, flags, hiding):
    c = 0 if flags and data["fa"][i] else o["c"]
    w = 0 if flags and data["fb"][i] else o["w"]
    return (c - o["v"] - GAMMA * (o["rv"] if hiding else 0) + w * (o["z"] - BETA)) % R_MOD


def kzg_args(m, data, kzg, sl, flags, hiding):
    o = kzg["rows"][sl]
    return dict(vk=kzg["vk"], comm=m.put(kzg["comm"][sl]), comm_inf=m.put(data["fa"][sl] if flags else None), points=m.put(mont([r["z"] for r in o])),
                values=m.put(mont([r["v"] for r in o])), w=m.put(kzg["w"][sl]), w_inf=m.put(data["fb"][sl] if flags else None),
                random_v=m.put(mont([r["rv"] for r in o]) if hiding else None), mem=m.mem)


@pytest.mark.parametrize("k", SIZES["points"])
@pytest.mark.parametrize("mem", [HOST, DEV])
def test_matrix_kzg10_check(ctx, data, kzg, mem, k):
    m, sl = Mem(ctx, mem), slice(1, 1 + k)
    seen = set()
    for flags, hiding in OPTIONAL_CELLS:
        out = m.out(k, np.uint8)
        ok(ctx, "czk_kzg10_check", k=k, out_ok=out, **kzg_args(m, data, kzg, sl, flags, hiding))
        want = [int(residual(data, kzg["rows"][i], i, flags, hiding) == 0) for i in range(1, 1 + k)]
        assert list(m.get(out)) == want
        seen |= set(want)
    assert seen == {0, 1}


@pytest.mark.parametrize("offs", [[0, 1], [0, 65, 65, 129]], ids=["b1", "b3_empty_middle"])
@pytest.mark.parametrize("mem", [HOST, DEV])
def test_matrix_kzg10_batch_check(ctx, data, kzg, mem, offs):
    m, k, b = Mem(ctx, mem), offs[-1], len(offs) - 1
    sl = slice(1, 1 + k)
    seen = set()
    for flags, hiding in OPTIONAL_CELLS:
        out = m.out(b, np.uint8)
        ok(ctx, "czk_kzg10_batch_check", randomizers=m.put(ints_to_limbs(kzg["r"][sl], 4)), offsets=offsets(offs), b=b, out_ok=out,
           **kzg_args(m, data, kzg, sl, flags, hiding))
        want = [int(sum(kzg["r"][i] * residual(data, kzg["rows"][i], i, flags, hiding) for i in range(1 + offs[j], 1 + offs[j + 1])) % R_MOD == 0)
                for j in range(b)]
        assert list(m.get(out)) == want
        seen |= set(want)
    assert b == 1 or seen == {0, 1}


# ------------------------------------------------------------------------------------------------- empty calls and argument errors
@pytest.fixture(scope="module")
def good(ctx, data, fixed_bases, groth16, kzg):
    """per call: arguments of a valid call over ONE item (one segment / batch of one item) of G1 in host memory, and the same in device memory"""
    def make(m):
        g1, g2 = m.put(limbs(1, [P.G1_GEN])[0]), m.put(limbs(2, [P.G2_GEN])[0])
        fr, f0 = m.put(mont([5])), m.put(np.zeros(3, dtype=np.uint8))
        o12, o24, o72, o1 = (lambda: m.out((1, 12))), (lambda: m.out((1, 24))), (lambda: m.out((1, 72))), (lambda: m.out(8, np.uint8))
        o01, mem = offsets([0, 1]), m.mem
        pt = groth16["pt"]
        return {
            "czk_points_add": dict(group=1, a=g1, a_inf=f0, b=g1, b_inf=f0, n=1, negate_b=0, out=o12(), out_inf=o1(), mem=mem),
            "czk_points_mul": dict(group=1, pts=g1, inf=f0, pts_stride=1, scalars=fr, n=1, scalar_form=1, out=o12(), out_inf=o1(), mem=mem),
            "czk_points_sum": dict(group=1, pts=g1, inf=f0, offsets=o01, k=1, out=o12(), out_inf=o1(), mem=mem),
            "czk_fixed_base_msm": dict(fb=fixed_bases[1], scalars=fr, n=1, scalar_form=1, out=o12(), out_inf=o1(), mem=mem),
            "czk_fq_sqrt": dict(ext=1, a=m.put(np.array([R.f_mont_limbs(1, 4)], dtype=np.uint64)), n=1, out=m.out((1, 6)), out_exists=o1(), mem=mem),
            "czk_points_serialize": dict(group=1, pts=g1, inf=f0, n=1, compressed=1, out=m.out(48, np.uint8), mem=mem),
            "czk_points_deserialize": dict(group=1, bytes=m.put(np.frombuffer(R.encode_points(1, [P.G1_GEN]), dtype=np.uint8)), n=1, flags=3, out_pts=o12(),
                                           out_inf=o1(), out_status=o1(), out_bad=None, out_first_bad=None, mem=mem),
            "czk_pairing": dict(g1=g1, g1_inf=f0, g2=g2, g2_inf=f0, n=1, out=o72(), mem=mem),
            "czk_pairing_product": dict(g1=g1, g1_inf=f0, g2=g2, g2_inf=f0, offsets=o01, k=1, out=o72(), out_is_one=o1(), mem=mem),
            "czk_groth16_verify": dict(pvk=groth16["pvk"], a=m.put(limbs(1, [pt["a"]])[0]), b=m.put(limbs(2, [pt["b"]])[0]), c=m.put(limbs(1, pt["c"][:1])[0]),
                                       inf=f0, public_inputs=m.put(mont([groth16["x"]])), m=1, k=1, out_ok=o1(), mem=mem),
            "czk_kzg10_check": dict(k=1, out_ok=o1(), **kzg_args(m, data, kzg, slice(0, 1), True, True)),
            "czk_kzg10_batch_check": dict(randomizers=m.put(ints_to_limbs([7], 4)), offsets=o01, b=1, out_ok=o1(), **kzg_args(m, data, kzg, slice(0, 1), True, True)),
        }
    h = {HOST: make(Mem(ctx, HOST)), DEV: make(Mem(ctx, DEV))}
    g1, g2 = limbs(1, [P.G1_GEN])[0], limbs(2, [P.G2_GEN])[0]
    for mem in h:   # the three calls that make a handle take host memory only
        h[mem]["czk_fixed_base_create"] = dict(group=1, base=g1, window=3, n_hint=0, out=C.byref(C.c_void_p(0)))
        h[mem]["czk_groth16_pvk_create"] = dict(alpha=g1, beta=g2, gamma=g2, delta=g2, gamma_abc=g1, gamma_abc_inf=None, n_gamma_abc=1, out=C.byref(C.c_void_p(0)))
        h[mem]["czk_kzg10_vk_create"] = dict(g=g1, gamma_g=g1, h=g2, beta_h=g2, out=C.byref(C.c_void_p(0)))
    return h


COUNT = {"czk_points_add": "n", "czk_points_mul": "n", "czk_points_sum": "k", "czk_fixed_base_msm": "n", "czk_fq_sqrt": "n", "czk_points_serialize": "n",
         "czk_points_deserialize": "n", "czk_pairing": "n", "czk_pairing_product": "k", "czk_groth16_verify": "k", "czk_kzg10_check": "k",
         "czk_kzg10_batch_check": "b"}


@pytest.mark.parametrize("mem", [HOST, DEV])
@pytest.mark.parametrize("name", sorted(COUNT))
def test_empty_call_returns_ok_and_touches_no_output(ctx, good, name, mem):
    """(the three create calls have no count)"""
    m = Mem(ctx, mem)
    kw = dict(good[mem][name])
    kw[COUNT[name]] = 0
    before = {a: m.get(v).copy() for a, v in kw.items() if a.startswith("out") and v is not None}   # (still as Mem.out filled them: no call wrote to them)
    assert before and all((v.view(np.uint8) == 0xA5).all() for v in before.values())
    if name == "czk_points_deserialize":       # the two counters are written first, whatever follows: 0 failures, first failure = n = 0
        n_bad, first = C.c_size_t(77), C.c_size_t(77)
        kw.update(out_bad=C.byref(n_bad), out_first_bad=C.byref(first))
    ok(ctx, name, **kw)
    for a, was in before.items():
        assert np.array_equal(m.get(kw[a]), was), a
    if name == "czk_points_deserialize":
        assert (n_bad.value, first.value) == (0, 0)


NULL_MSG = {"czk_points_add": "null points_add buffer", "czk_points_mul": "null points_mul buffer", "czk_points_sum": "null points_sum buffer",
            "czk_fixed_base_msm": "null fixed_base_msm buffer", "czk_fq_sqrt": "null fq_sqrt buffer", "czk_points_serialize": "null points_serialize buffer",
            "czk_points_deserialize": "null points_deserialize buffer", "czk_pairing": "null pairing argument", "czk_groth16_verify": "null proof argument",
            "czk_kzg10_check": "null opening argument", "czk_groth16_pvk_create": "null verifying key argument (gamma_abc_g1 needs at least one point)",
            "czk_kzg10_vk_create": "null verifier key point"}
REQUIRED = {"czk_points_add": "a b out", "czk_points_mul": "pts scalars out", "czk_points_sum": "offsets out", "czk_fixed_base_msm": "scalars out",
            "czk_fq_sqrt": "a out out_exists", "czk_points_serialize": "pts out", "czk_points_deserialize": "bytes out_pts out_inf", "czk_pairing": "g1 g2 out",
            "czk_groth16_verify": "a b c out_ok public_inputs", "czk_kzg10_check": "comm points values w out_ok",
            "czk_groth16_pvk_create": "alpha beta gamma delta gamma_abc", "czk_kzg10_vk_create": "g gamma_g h beta_h"}
# (call, the one argument that is wrong, the message): every argument check of every call, texts as the library has always had them
ERRORS = [(name, {"mem": 2}, MEM_MSG) for name in sorted(COUNT)]
ERRORS += [(name, {"group": 3}, GROUP_MSG) for name in ("czk_points_add", "czk_points_mul", "czk_points_sum", "czk_fixed_base_create", "czk_points_serialize",
                                                        "czk_points_deserialize")]
ERRORS += [(name, {"group": 0}, GROUP_MSG) for name in ("czk_points_add", "czk_fixed_base_create")]
ERRORS += [(name, {arg: None}, NULL_MSG[name]) for name in sorted(REQUIRED) for arg in REQUIRED[name].split()]
ERRORS += [
    ("czk_points_mul", {"pts_stride": 2}, "pts_stride must be 1, or 0 for one point"),
    ("czk_points_mul", {"scalar_form": 2}, "bad scalar_form"),
    ("czk_points_mul", {"scalar_form": -1}, "bad scalar_form"),
    ("czk_fixed_base_msm", {"scalar_form": 2}, "bad scalar_form"),
    ("czk_points_sum", {"offsets": offsets([1, 1])}, "offsets[0] must be 0"),
    ("czk_points_sum", {"offsets": offsets([0, 2, 1]), "k": 2}, "offsets must be non-decreasing"),
    ("czk_points_sum", {"pts": None}, "null points"),
    ("czk_pairing_product", {"offsets": None}, "null pairing_product argument"),
    ("czk_pairing_product", {"offsets": offsets([1, 1])}, "offsets[0] must be 0"),
    ("czk_pairing_product", {"offsets": offsets([0, 2, 1]), "k": 2}, "offsets must be non-decreasing"),
    ("czk_pairing_product", {"g1": None}, "null points"),
    ("czk_pairing_product", {"g2": None}, "null points"),
    ("czk_kzg10_batch_check", {"offsets": None}, "null batch argument"),
    ("czk_kzg10_batch_check", {"out_ok": None}, "null batch argument"),
    ("czk_kzg10_batch_check", {"offsets": offsets([1, 1])}, "offsets[0] must be 0"),
    ("czk_kzg10_batch_check", {"offsets": offsets([0, 2, 1]), "b": 2}, "offsets must be non-decreasing"),
    ("czk_kzg10_batch_check", {"randomizers": None}, "null opening argument"),
    ("czk_kzg10_batch_check", {"comm": None}, "null opening argument"),
    ("czk_kzg10_check", {"vk": None}, "null verifier key"),
    ("czk_kzg10_batch_check", {"vk": None}, "null verifier key"),
    ("czk_groth16_verify", {"pvk": None}, "null verifying key"),
    ("czk_groth16_verify", {"m": 2}, "MalformedVerifyingKey"),
    ("czk_groth16_verify", {"m": 0}, "MalformedVerifyingKey"),
    ("czk_groth16_pvk_create", {"n_gamma_abc": 0}, "null verifying key argument (gamma_abc_g1 needs at least one point)"),
    ("czk_fixed_base_msm", {"fb": None}, "null fixed_base_msm argument"),
    ("czk_fixed_base_create", {"out": None}, "null fixed_base_create argument"),
    ("czk_fixed_base_create", {"base": None}, "null base"),
    ("czk_fixed_base_create", {"window": 21}, "window must be 0 (chosen by the library) or 1..20"),
    ("czk_fixed_base_create", {"base": limbs(1, [P.INF])[0]}, "the base is the point at infinity"),
    ("czk_fq_sqrt", {"ext": 3}, "ext must be 1 (Fq) or 2 (Fq2)"),
    ("czk_points_deserialize", {"flags": 4}, "flags: CZK_POINTS_COMPRESSED | CZK_POINTS_CHECKED"),
]


@pytest.mark.parametrize("name,wrong,msg", ERRORS, ids=[f"{i}-{n[4:]}-{'+'.join(w)}" for i, (n, w, _) in enumerate(ERRORS)])
def test_one_wrong_argument(ctx, good, name, wrong, msg):
    """CZK_ERR_ARG and the message, with every other argument valid (host memory; a decreasing offset needs a second segment, hence k = 2)"""
    kw = dict(good[HOST][name], **wrong)
    assert call(ctx, name, **kw) == (ERR_ARG, msg)


@pytest.mark.parametrize("name,arg", [("czk_points_serialize", "out"), ("czk_points_deserialize", "bytes")])
def test_unaligned_device_byte_buffer(ctx, good, name, arg):
    """every pointer of the call is device memory; the byte buffer starts one byte into an allocation"""
    kw, room = dict(good[DEV][name]), Mem(ctx, DEV).out(64, np.uint8)
    kw[arg] = room.data_ptr() + 1
    assert call(ctx, name, **kw) == (ERR_ARG, "device byte buffers must be 8-byte aligned")


# ------------------------------------------------------------------------------------------------- fr_vec.hip, ntt.hip, witness_map.hip
# The pointwise Fr calls, the radix-2 transforms and the Groth16 witness map.  Values of the transforms and of the witness map are covered by
# tests/test_gpu_parity.py and tests/test_witness_map_short.py; here: the pointwise values for every kind of caller, and every rejection.
# (A null context: tests/test_fr_ntt_calls_cpu.py.)
ERR_SIZE, SCALAR_HOST = 1, 256
FR_SIZES = (1, 257)                            # one element; one past the 256-thread block
FR_ROWS = 258                                  # rows [1, 1 + n) are used
LOG_D, D = 3, 8                                # the domain of the transform and witness-map rejections
SCALE_MEM_MSG = "mem must be CZK_MEM_HOST, CZK_MEM_DEVICE or CZK_MEM_DEVICE | CZK_MEM_SCALAR_HOST"
ADICITY_MSG = "domain larger than 2^TWO_ADICITY (radix2/mod.rs:61-63)"
WM_NULL_MSG, WM_SIZE_MSG = "null witness_map argument", "witness_map: more evaluations than the domain holds"


@pytest.fixture(scope="module")
def fr_rows():
    """five columns of FR_ROWS residues: 0, 1 and r - 1 meet each other and random elements in every column pair (periods 4, 5, 7, 9, 11)"""
    from util import limbs_to_ints, rand_fr_canonical
    rnd = limbs_to_ints(rand_fr_canonical(0xC0DE, 5 * FR_ROWS))
    edge = (0, None, 1, R_MOD - 1)             # row 1, the only row of n = 1, is random in every column
    cols = []
    for c, period in enumerate((4, 5, 7, 9, 11)):
        cols.append([rnd[c * FR_ROWS + i] if i % period >= 4 or edge[i % period] is None else edge[i % period] for i in range(FR_ROWS)])
    assert all({0, 1, R_MOD - 1} <= set(col) for col in cols)
    return cols


def fr_check(m, out, want):
    assert np.array_equal(m.get(out), mont(want))


@pytest.mark.parametrize("n", FR_SIZES)
@pytest.mark.parametrize("mem", [HOST, DEV])
def test_matrix_fr_vec_op(ctx, fr_rows, mem, n):
    m, sl = Mem(ctx, mem), slice(1, 1 + n)
    a, b = fr_rows[0][sl], fr_rows[1][sl]
    for op, f in ((0, lambda x, y: x + y), (1, lambda x, y: x - y), (2, lambda x, y: x * y)):
        out = m.out((n, 4))
        ok(ctx, "czk_fr_vec_op", op=op, a=m.put(mont(a)), b=m.put(mont(b)), out=out, n=n, mem=mem)
        fr_check(m, out, [f(x, y) for x, y in zip(a, b)])


@pytest.mark.parametrize("n", FR_SIZES)
@pytest.mark.parametrize("mode", ["host", "device", "device_scalar_host"])
def test_matrix_fr_vec_scale(ctx, fr_rows, mode, n):
    """the three modes: everything host memory, everything device memory, device vectors with the scalar in host memory"""
    m = Mem(ctx, HOST if mode == "host" else DEV)
    mem = {"host": HOST, "device": DEV, "device_scalar_host": DEV | SCALAR_HOST}[mode]
    a = fr_rows[0][1:1 + n]
    for k in (0, 1, R_MOD - 1, fr_rows[1][1]):
        out, kk = m.out((n, 4)), mont([k])
        ok(ctx, "czk_fr_vec_scale", a=m.put(mont(a)), k=kk if mode == "device_scalar_host" else m.put(kk), out=out, n=n, mem=mem)
        fr_check(m, out, [x * k for x in a])


@pytest.mark.parametrize("n", FR_SIZES)
@pytest.mark.parametrize("mem", [HOST, DEV])
def test_matrix_fr_beaver_combine(ctx, fr_rows, mem, n):
    m = Mem(ctx, mem)
    x, y, z, sx, oy = (c[1:1 + n] for c in fr_rows)
    for add_open in (0, 1):
        out = m.out((n, 4))
        ok(ctx, "czk_fr_beaver_combine", x=m.put(mont(x)), y=m.put(mont(y)), z=m.put(mont(z)), sx=m.put(mont(sx)), oy=m.put(mont(oy)), add_open=add_open,
           out=out, n=n, mem=mem)
        fr_check(m, out, [zz - yy * s - xx * o + add_open * s * o for xx, yy, zz, s, o in zip(x, y, z, sx, oy)])


@pytest.mark.parametrize("n", FR_SIZES)
@pytest.mark.parametrize("mem", [HOST, DEV])
def test_matrix_fr_repr(ctx, fr_rows, mem, n):
    """into_repr: Montgomery words -> the residue's own words; from_repr: the way back"""
    m, a = Mem(ctx, mem), fr_rows[0][1:1 + n]
    out = m.out((n, 4))
    ok(ctx, "czk_fr_into_repr", a=m.put(mont(a)), out=out, n=n, mem=mem)
    assert np.array_equal(m.get(out), ints_to_limbs(a, 4))
    out = m.out((n, 4))
    ok(ctx, "czk_fr_from_repr", a=m.put(ints_to_limbs(a, 4)), out=out, n=n, mem=mem)
    fr_check(m, out, a)


@pytest.fixture(scope="module")
def fr_good(ctx, fr_rows):
    """per call: arguments of a valid call (three elements; the transforms: two lanes of a 2^3 domain), in host memory where the call takes it and in
    device memory.  czk_fr_spdz_open's counter is host memory in either case."""
    def make(m):
        mem = m.mem
        vec = lambda lanes=1, n=3: m.put(mont(fr_rows[0][1:1 + lanes * n]))
        o = lambda lanes=1, n=3: m.out((lanes * n, 4))
        g = {
            "czk_fr_vec_op": dict(op=0, a=vec(), b=vec(), out=o(), n=3, mem=mem),
            "czk_fr_vec_scale": dict(a=vec(), k=vec(1, 1), out=o(), n=3, mem=mem),
            "czk_fr_beaver_combine": dict(x=vec(), y=vec(), z=vec(), sx=vec(), oy=vec(), add_open=1, out=o(), n=3, mem=mem),
            "czk_fr_into_repr": dict(a=vec(), out=o(), n=3, mem=mem),
            "czk_fr_from_repr": dict(a=vec(), out=o(), n=3, mem=mem),
            "czk_ntt_fr": dict(data=o(2, D), log_d=LOG_D, lanes=2, kind=0, in_len=D, mem=mem),
        }
        if mem == DEV:
            g.update({
                "czk_fr_spdz_open": dict(shares=vec(4), parties=2, n=3, out_value=o(), out_bad=C.byref(C.c_uint64(77))),
                "czk_spdz_open_combine": dict(a=vec(2), b=vec(2), tx=vec(2), ty=vec(2), tz=vec(2), parties=1, king_mask=1, sx=o(), oy=o(), chk_a=o(), chk_b=o(),
                                              ab=o(2), n=3),
                "czk_ntt_fr_to": dict(src=vec(2, D), src_stride=D, dst=o(2, D), log_d=LOG_D, lanes=2, kind=0, in_len=D, mem=DEV),
                "czk_witness_map_pre": dict(a=o(2, D), a_len=D, b=o(2, D), b_len=D, log_d=LOG_D, lanes=2),
                "czk_witness_map_pre_masked": dict(a=o(2, D), a_len=D, b=o(2, D), b_len=D, mask_a=vec(2, D), mask_b=vec(2, D), log_d=LOG_D, lanes=2),
                "czk_witness_map_post": dict(ab=o(2, D), c=o(2, D), c_len=D, log_d=LOG_D, lanes=2),
                "czk_witness_map_post_h": dict(ab=o(2, D), c=o(2, D), c_len=D, log_d=LOG_D, lanes=2),
            })
        return g
    return {HOST: make(Mem(ctx, HOST)), DEV: make(Mem(ctx, DEV))}


# call -> (the count that makes it empty, the buffers it writes)
FR_EMPTY = {
    "czk_fr_vec_op": ("n", "out"), "czk_fr_vec_scale": ("n", "out"), "czk_fr_beaver_combine": ("n", "out"), "czk_fr_into_repr": ("n", "out"),
    "czk_fr_from_repr": ("n", "out"), "czk_fr_spdz_open": ("n", "out_value"), "czk_spdz_open_combine": ("n", "sx oy chk_a chk_b ab"),
    "czk_ntt_fr": ("lanes", "data"), "czk_ntt_fr_to": ("lanes", "dst"), "czk_witness_map_pre": ("lanes", "a b"),
    "czk_witness_map_pre_masked": ("lanes", "a b"), "czk_witness_map_post": ("lanes", "ab c"), "czk_witness_map_post_h": ("lanes", "ab c"),
}
FR_HOST_CALLS = ("czk_fr_vec_op", "czk_fr_vec_scale", "czk_fr_beaver_combine", "czk_fr_into_repr", "czk_fr_from_repr", "czk_ntt_fr")


@pytest.mark.parametrize("name,mem", [(n, DEV) for n in sorted(FR_EMPTY)] + [(n, HOST) for n in FR_HOST_CALLS])
def test_empty_fr_call_returns_ok_and_touches_no_output(ctx, fr_good, name, mem):
    m, (count, outs) = Mem(ctx, mem), FR_EMPTY[name]
    kw = dict(fr_good[mem][name])
    kw[count] = 0
    before = {a: m.get(kw[a]).copy() for a in outs.split()}                  # (still as Mem.out filled them: no call wrote to them)
    assert all((v.view(np.uint8) == 0xA5).all() for v in before.values())
    if name == "czk_fr_spdz_open":                                           # the counter is zeroed before the call looks at n
        bad = C.c_uint64(77)
        kw["out_bad"] = C.byref(bad)
    ok(ctx, name, **kw)
    for a, was in before.items():
        assert np.array_equal(m.get(kw[a]), was), a
    if name == "czk_fr_spdz_open":
        assert bad.value == 0


def _each_null(name, args, msg, mem=HOST):
    return [(name, mem, {a: None}, ERR_ARG, msg) for a in args.split()]


# (call, the memory of the valid arguments, the one argument that is wrong, the code, the message)
FR_ERRORS = _each_null("czk_fr_vec_op", "a b out", "bad vec_op argument") + _each_null("czk_fr_vec_op", "a b out", "bad vec_op argument", DEV)
FR_ERRORS += [
    ("czk_fr_vec_op", HOST, {"op": -1}, ERR_ARG, "bad vec_op argument"),
    ("czk_fr_vec_op", HOST, {"op": 3}, ERR_ARG, "bad vec_op argument"),
    ("czk_fr_vec_op", HOST, {"op": 3, "n": 0}, ERR_ARG, "bad vec_op argument"),          # a bad op is rejected even by an empty call
    ("czk_fr_vec_op", HOST, {"op": -1, "n": 0}, ERR_ARG, "bad vec_op argument"),
    ("czk_fr_vec_op", HOST, {"mem": 2}, ERR_ARG, MEM_MSG),
    ("czk_fr_vec_scale", HOST, {"k": None}, ERR_ARG, "bad vec_scale argument"),
    ("czk_fr_vec_scale", HOST, {"k": None, "n": 0}, ERR_ARG, "bad vec_scale argument"),  # ... and a null scalar
    ("czk_fr_vec_scale", DEV, {"k": None, "n": 0}, ERR_ARG, "bad vec_scale argument"),
    ("czk_fr_vec_scale", HOST, {"a": None}, ERR_ARG, "bad vec_scale argument"),
    ("czk_fr_vec_scale", HOST, {"out": None}, ERR_ARG, "bad vec_scale argument"),
    ("czk_fr_vec_scale", HOST, {"mem": 2}, ERR_ARG, SCALE_MEM_MSG),
    ("czk_fr_vec_scale", HOST, {"mem": SCALAR_HOST}, ERR_ARG, SCALE_MEM_MSG),             # the scalar flag goes with device vectors only
    ("czk_fr_vec_scale", HOST, {"mem": 2, "n": 0}, ERR_ARG, SCALE_MEM_MSG),
]
FR_ERRORS += _each_null("czk_fr_beaver_combine", "x y z sx oy out", "null beaver argument")
FR_ERRORS += [("czk_fr_beaver_combine", HOST, {"mem": 2}, ERR_ARG, MEM_MSG)]
FR_ERRORS += _each_null("czk_fr_spdz_open", "out_bad shares out_value", "bad spdz_open argument", DEV)
FR_ERRORS += [("czk_fr_spdz_open", DEV, {"parties": 0}, ERR_ARG, "bad spdz_open argument")]
for _name in ("czk_fr_into_repr", "czk_fr_from_repr"):
    FR_ERRORS += _each_null(_name, "a out", "null repr argument") + [(_name, HOST, {"mem": 2}, ERR_ARG, MEM_MSG)]
FR_ERRORS += [("czk_spdz_open_combine", DEV, {"parties": p}, ERR_ARG, "spdz_open_combine: 1 to 32 parties (the king mask has one bit per lane)") for p in (0, 33)]
FR_ERRORS += _each_null("czk_spdz_open_combine", "a b tx ty tz sx oy chk_a chk_b ab", "null spdz_open_combine argument", DEV)
FR_ERRORS += [
    ("czk_ntt_fr", HOST, {"data": None}, ERR_ARG, "null data"),
    ("czk_ntt_fr", DEV, {"data": None}, ERR_ARG, "null data"),
    ("czk_ntt_fr", HOST, {"log_d": 48}, ERR_SIZE, ADICITY_MSG),
    ("czk_ntt_fr", HOST, {"mem": 2}, ERR_ARG, MEM_MSG),
    ("czk_ntt_fr", HOST, {"kind": -1}, ERR_ARG, "bad ntt kind"),
    ("czk_ntt_fr", HOST, {"kind": 4}, ERR_ARG, "bad ntt kind"),
    ("czk_ntt_fr", DEV, {"kind": 4}, ERR_ARG, "bad ntt kind"),
    ("czk_ntt_fr", HOST, {"in_len": D + 1}, ERR_SIZE, "coeffs.len() > domain size (radix2/mod.rs:100)"),
    ("czk_ntt_fr", DEV, {"in_len": D + 1}, ERR_SIZE, "coeffs.len() > domain size (radix2/mod.rs:100)"),
    ("czk_ntt_fr_to", DEV, {"dst": None}, ERR_ARG, "null ntt argument"),
    ("czk_ntt_fr_to", DEV, {"src": None}, ERR_ARG, "null ntt argument"),
    ("czk_ntt_fr_to", DEV, {"mem": HOST}, ERR_ARG, "czk_ntt_fr_to takes device memory (host callers copy and use czk_ntt_fr)"),
    ("czk_ntt_fr_to", DEV, {"log_d": 48}, ERR_SIZE, "domain too large: log2 D exceeds TWO_ADICITY = 47 (radix2/mod.rs:61-63)"),
    ("czk_ntt_fr_to", DEV, {"src_stride": D - 1}, ERR_ARG, "in_len exceeds the source lane stride"),
    ("czk_ntt_fr_to", DEV, {"kind": 4}, ERR_ARG, "bad ntt kind"),
]
for _name, _ptrs, _lens in (("czk_witness_map_pre", "a b", "a_len b_len"), ("czk_witness_map_pre_masked", "a b mask_a mask_b", "a_len b_len"),
                            ("czk_witness_map_post", "ab c", "c_len"), ("czk_witness_map_post_h", "ab c", "c_len")):
    FR_ERRORS += _each_null(_name, _ptrs, WM_NULL_MSG, DEV) + [(_name, DEV, {a: D + 1}, ERR_SIZE, WM_SIZE_MSG) for a in _lens.split()]
FR_ERRORS += [("czk_witness_map_pre_masked", DEV, {"log_d": 48}, ERR_SIZE, ADICITY_MSG)]


@pytest.mark.parametrize("name,mem,wrong,code,msg", FR_ERRORS, ids=[f"{i}-{n[4:]}-{'dev' if m else 'host'}-{'+'.join(w)}" for i, (n, m, w, _, _) in enumerate(FR_ERRORS)])
def test_one_wrong_fr_argument(ctx, fr_good, name, mem, wrong, code, msg):
    """the code and the message, every other argument valid; the buffers the call would have written still hold their sentinel"""
    kw = dict(fr_good[mem][name], **wrong)
    assert call(ctx, name, **kw) == (code, msg)
    m = Mem(ctx, mem)
    for a in FR_EMPTY[name][1].split():
        if kw[a] is not None:
            assert (m.get(kw[a]).view(np.uint8) == 0xA5).all(), a
