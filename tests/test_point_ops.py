"""Elementwise group arithmetic on device arrays (czk_points_add, czk_points_mul, czk_points_sum) against the affine big-integer group law
of tests/pairing_ref.py (oracle/pyref.py's ec_add / ec_mul): every comparison is exact -- affine Montgomery limbs are canonical -- and covers
every exceptional case of the reference's add_assign_mixed / add_assign, points of small order and points outside the prime-order subgroup."""
import numpy as np
import pytest

import pairing_ref as P
from util import R_MOD, ints_to_limbs, rand_fr_canonical, limbs_to_ints

pytestmark = pytest.mark.gpu
Q = P.Q
FLD = {1: P.F1, 2: P.F2}
SIZES = (1, 127, 128, 129)                     # one thread, and either side of a block of 128
ORDER2 = (Q - 1, 0)                            # (-1, 0): y = 0, so 2 P = infinity
ORDER3 = (0, 1)                                # (0, 1) on y^2 = x^3 + 1: 2 P = -P; NOT the infinity encoding (its flag is 0)
EDGE_SCALARS = (0, 1, 2, R_MOD - 1, R_MOD, R_MOD + 1, 1 << 253, (1 << 256) - 1)


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def to_limbs(group, points):
    f = P.g1_to_limbs if group == 1 else P.g2_to_limbs
    rows = [f(p) for p in points]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(-1, 12 * group), np.array([r[1] for r in rows], dtype=np.uint8)


def from_limbs(group, pts, inf):
    f = P.g1_from_limbs if group == 1 else P.g2_from_limbs
    return [f([int(v) for v in pts[i]], int(inf[i])) for i in range(len(inf))]


def assert_points(group, got, want):
    """exact: flags equal, finite coordinates equal limb for limb, infinity written as (0, 1)"""
    w_pts, w_inf = to_limbs(group, want)
    assert np.array_equal(got[1], w_inf), np.nonzero(got[1] != w_inf)[0][:8]
    assert np.array_equal(got[0], w_pts), np.nonzero((got[0] != w_pts).any(axis=1))[0][:8]


def _off_subgroup(ctx, group, count):
    """On-curve points OUTSIDE the prime-order subgroup: small x decoded by czk_points_deserialize(compressed, unchecked), which solves for y and
    makes no subgroup test; kept when [r] P is not infinity."""
    import czk_amd
    size = 48 * group
    cands = np.zeros((64, size), dtype=np.uint8)
    for i in range(64):
        cands[i, 0] = i + 2                    # x = i + 2 (G2: x = (i + 2, 0)); flags clear: the smaller root
    pts, inf, status, _, _ = ctx.points_deserialize(group, cands.reshape(-1), compressed=True, checked=False)
    out = []
    for i in np.nonzero(status == czk_amd.binding.CZK_POINT_OK)[0]:
        p = from_limbs(group, pts[i:i + 1], inf[i:i + 1])[0]
        b = 1 if group == 1 else P.G2_B
        assert P.pyref.ec_on_curve(FLD[group], p, b)
        if P.ec_mul(FLD[group], R_MOD, p) is not P.INF:
            out.append(p)
        if len(out) == count:
            return out
    raise AssertionError("not enough off-subgroup points")


@pytest.fixture(scope="module")
def pool(ctx):
    """per group: subgroup points, off-subgroup points, (G1) the points of order 2 and 3"""
    out = {}
    for group in (1, 2):
        ks = limbs_to_ints(rand_fr_canonical(0x9010 + group, 3))
        gen = P.G1_GEN if group == 1 else P.G2_GEN
        sub = [P.ec_mul(FLD[group], k, gen) for k in ks]
        off = _off_subgroup(ctx, group, 2)
        small = [ORDER2, ORDER3] if group == 1 else []
        out[group] = {"sub": sub, "off": off, "small": small, "all": sub + off + small}
    return out


def _add_rows(group, pool):
    """(a, b) rows: every exceptional case first, then pairs of distinct points"""
    F, pts = FLD[group], pool[group]["all"]
    p, q = pool[group]["sub"][0], pool[group]["off"][0]
    rows = [(p, p), (p, P.ec_neg(F, p)), (P.INF, p), (p, P.INF), (P.INF, P.INF), (q, q), (q, P.ec_neg(F, q))]
    if group == 1:
        assert P.pyref.ec_on_curve(F, ORDER2, 1) and P.pyref.ec_on_curve(F, ORDER3, 1)
        rows += [(ORDER2, ORDER2), (ORDER3, ORDER3), (ORDER3, P.ec_neg(F, ORDER3)), (ORDER3, p), (p, ORDER3), (ORDER2, ORDER3)]
    for i in range(129):
        a, b = pts[i % len(pts)], pts[(3 * i + 1) % len(pts)]
        rows.append((a, b if a != b else pts[(3 * i + 2) % len(pts)]))
    return rows


@pytest.fixture(scope="module")
def add_cases(pool):
    """per group: the rows as limbs and the sums / differences from the affine law, computed once"""
    out = {}
    for group in (1, 2):
        F, rows = FLD[group], _add_rows(group, pool)
        out[group] = {"rows": rows, "a": to_limbs(group, [r[0] for r in rows]), "b": to_limbs(group, [r[1] for r in rows]),
                      "sum": [P.ec_add(F, a, b) for a, b in rows], "diff": [P.ec_add(F, a, P.ec_neg(F, b)) for a, b in rows]}
    return out


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_points_add(ctx, add_cases, group, n):
    c = add_cases[group]
    total = len(c["rows"])
    # n = 1: every exceptional row as a call of its own; larger n: the first n rows (all exceptional rows + distinct pairs)
    windows = [(i, i + 1) for i in range(total - 129 + 2)] if n == 1 else [(0, n)]
    for lo, hi in windows:
        for negate, want in ((False, c["sum"]), (True, c["diff"])):
            got = ctx.points_add(group, c["a"][0][lo:hi], c["b"][0][lo:hi], a_inf=c["a"][1][lo:hi], b_inf=c["b"][1][lo:hi], negate_b=negate)
            assert_points(group, got, want[lo:hi])


def test_points_add_small_order_points_are_not_infinity(ctx):
    """(0, 1) with flag 0 is the order-3 point -- 2 P = -P -- although infinity is WRITTEN as (0, 1) with flag 1; (-1, 0) doubles to infinity."""
    a, a_inf = to_limbs(1, [ORDER3, ORDER2, P.INF])
    assert np.array_equal(a[0], a[2]) and list(a_inf) == [0, 0, 1]
    pts, inf = ctx.points_add(1, a, a, a_inf=a_inf, b_inf=a_inf)
    assert list(inf) == [0, 1, 1]
    assert from_limbs(1, pts, inf)[0] == (0, Q - 1)
    assert_points(1, (pts, inf), [(0, Q - 1), P.INF, P.INF])
    pts, inf = ctx.points_add(1, a, a)         # no flags given: row 2 is the order-3 point as well
    assert list(inf) == [0, 1, 0] and np.array_equal(pts[2], pts[0])


@pytest.fixture(scope="module")
def mul_cases(pool):
    """per group: (point, scalar) -> [k] P from the affine law over the whole 256-bit scalar (no reduction: the point's order need not be r)"""
    rnd = limbs_to_ints(rand_fr_canonical(0x9020, 1)) + [int.from_bytes(bytes(range(7, 39)), "little")]   # the last one is above r
    scalars = list(EDGE_SCALARS) + rnd
    out = {}
    for group in (1, 2):
        pts = pool[group]["all"] + [P.INF]
        memo = {}
        for i, p in enumerate(pts):
            for k in set(scalars) | {k % R_MOD for k in scalars}:
                memo[(i, k)] = P.ec_mul(FLD[group], k, p)
        out[group] = {"points": pts, "scalars": scalars, "memo": memo, "off": len(pool[group]["sub"])}
    return out


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("montgomery", [False, True])
def test_points_mul_stride_1(ctx, mul_cases, group, montgomery):
    import czk_amd
    c = mul_cases[group]
    idx = [(i, k) for i in range(len(c["points"])) for k in c["scalars"]]
    idx = idx * (1 + 129 // len(idx))          # every (point, scalar) pair, repeated to more than one block
    pts, inf = to_limbs(group, [c["points"][i] for i, _ in idx])
    if montgomery:                             # an Fr: the scalar is k mod r, handed over as k R mod r and decoded on the device
        ks = ints_to_limbs([(k % R_MOD) * (1 << 256) % R_MOD for _, k in idx], 4)
        want = [c["memo"][(i, k % R_MOD)] for i, k in idx]
    else:
        ks = ints_to_limbs([k for _, k in idx], 4)
        want = [c["memo"][(i, k)] for i, k in idx]
    form = czk_amd.CZK_SCALAR_MONTGOMERY if montgomery else czk_amd.CZK_SCALAR_CANONICAL
    assert len(idx) > 128
    assert_points(group, ctx.points_mul(group, pts, ks, inf=inf, scalar_form=form), want)
    for n in (1, 127):
        assert_points(group, ctx.points_mul(group, pts[:n], ks[:n], inf=inf[:n], scalar_form=form), want[:n])


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("montgomery", [False, True])
def test_points_mul_stride_0(ctx, mul_cases, group, montgomery):
    import czk_amd
    c = mul_cases[group]
    form = czk_amd.CZK_SCALAR_MONTGOMERY if montgomery else czk_amd.CZK_SCALAR_CANONICAL
    for i in (0, c["off"], len(c["points"]) - 1):     # a subgroup point, an off-subgroup point, infinity
        red = (lambda k: k % R_MOD) if montgomery else (lambda k: k)
        scalars = c["scalars"] * 13            # 130 scalars: two blocks
        ks = ints_to_limbs([red(k) * (1 << 256) % R_MOD if montgomery else k for k in scalars], 4)
        pts, inf = to_limbs(group, [c["points"][i]])
        got = ctx.points_mul(group, pts, ks, inf=inf, stride=0, scalar_form=form)
        assert_points(group, got, [c["memo"][(i, red(k))] for k in scalars])


def test_points_mul_agrees_with_the_host_scalar_mul(ctx, mul_cases):
    """the existing host call czk_jac_scalar_mul, point by point"""
    import czk_amd
    for group in (1, 2):
        c = mul_cases[group]
        pts, inf = to_limbs(group, c["points"][:4])
        ks = ints_to_limbs([R_MOD - 1, (1 << 256) - 1, 2, c["scalars"][-2]], 4)
        assert c["scalars"][-2] < R_MOD
        got = ctx.points_mul(group, pts, ks, inf=inf)
        one = np.array(P.pyref.int_to_limbs(P.pyref.FQ_MONT_R, 6) + ([0] * 6 if group == 2 else []), dtype=np.uint64)
        for i in range(4):
            jac = ctx.jac_scalar_mul(group, np.concatenate([pts[i], one]), ks[i])
            aff, ainf = ctx.jac_to_affine(group, jac)
            assert int(ainf[0]) == int(got[1][i]) and np.array_equal(aff[0], got[0][i]), (group, i)


@pytest.mark.parametrize("group", [1, 2])
def test_points_sum(ctx, pool, group):
    F, pts = FLD[group], pool[group]["all"]
    p = pts[1]
    segs = []
    for j, length in enumerate((0, 1, 2, 63, 64, 65, 129, 1000)):
        # every 7th entry infinity; consecutive entries differ, equal and opposite points meet inside the lanes' strides
        segs.append([P.INF if (i + j) % 7 == 3 else (pts[(5 * i + j) % len(pts)] if i % 11 else P.ec_neg(F, pts[(i + j) % len(pts)]))
                     for i in range(length)])
    segs.append([p, P.ec_neg(F, p), p, p])                 # opposite partial sums, then equal ones
    segs.append([p] * 64)                                  # one point per lane: every step of the tree is a doubling
    segs.append([P.INF] * 5)
    segs.append([])                                        # a trailing empty segment
    flat = [x for s in segs for x in s]
    offs = np.cumsum([0] + [len(s) for s in segs])
    want = []
    for s in segs:
        acc = P.INF
        for x in s:
            acc = P.ec_add(F, acc, x)
        want.append(acc)
    assert want[8] == P.ec_add(F, p, p) and want[9] == P.ec_mul(F, 64, p) and want[10] is P.INF and want[0] is P.INF
    lp, li = to_limbs(group, flat)
    assert_points(group, ctx.points_sum(group, lp, offs, inf=li), want)
    # a single segment, and an odd number of segments (the second wave of the last block has none)
    assert_points(group, ctx.points_sum(group, lp[:offs[7]], offs[:8], inf=li[:offs[7]]), want[:7])
    assert_points(group, ctx.points_sum(group, lp[:1000], [0, 1000], inf=li[:1000]), [_sum(F, flat[:1000])])


def _sum(F, xs):
    acc = P.INF
    for x in xs:
        acc = P.ec_add(F, acc, x)
    return acc


def test_empty_calls_and_argument_errors(ctx):
    import czk_amd
    for group in (1, 2):
        e = np.zeros((0, 12 * group), dtype=np.uint64)
        assert ctx.points_add(group, e, e)[0].shape == (0, 12 * group)
        assert ctx.points_mul(group, e, np.zeros((0, 4), dtype=np.uint64))[0].shape == (0, 12 * group)
        assert ctx.points_sum(group, e, [0])[0].shape == (0, 12 * group)
        pts, inf = ctx.points_sum(group, e, [0, 0, 0])
        assert list(inf) == [1, 1]
    one = to_limbs(1, [P.G1_GEN])[0]
    with pytest.raises(czk_amd.CzkError):
        ctx.points_sum(1, one, [1, 1])                     # offsets[0] != 0
    with pytest.raises(czk_amd.CzkError):
        ctx.points_mul(1, one, np.zeros((1, 4), dtype=np.uint64), stride=2)
    with pytest.raises(czk_amd.CzkError):
        ctx.points_add(3, np.zeros((1, 24), dtype=np.uint64), np.zeros((1, 24), dtype=np.uint64))


def test_device_memory_calls_only_enqueue_and_may_work_in_place(ctx, add_cases, mul_cases):
    """CZK_MEM_DEVICE: the same results from device pointers, with out aliasing an input"""
    import czk_amd
    import torch
    dev = torch.device("cuda", ctx.device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).to(dev)
    M = czk_amd.CZK_MEM_DEVICE
    for group in (1, 2):
        c = add_cases[group]
        n = 129
        a, ai, b, bi = up(c["a"][0][:n]), up(c["a"][1][:n]), up(c["b"][0][:n]), up(c["b"][1][:n])
        ctx.points_add(group, a.data_ptr(), b.data_ptr(), a_inf=ai.data_ptr(), b_inf=bi.data_ptr(), negate_b=True, n=n, out=a.data_ptr(),
                       out_inf=ai.data_ptr(), mem=M)
        ks = up(ints_to_limbs([3] * n, 4))
        out, oi = torch.zeros_like(a), torch.zeros_like(ai)
        ctx.points_mul(group, a.data_ptr(), ks.data_ptr(), inf=ai.data_ptr(), n=n, out=out.data_ptr(), out_inf=oi.data_ptr(), mem=M)
        s, si = torch.zeros((2, 12 * group), dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.uint8, device=dev)
        ctx.points_sum(group, out.data_ptr(), [0, 100, n], inf=oi.data_ptr(), out=s.data_ptr(), out_inf=si.data_ptr(), mem=M)
        ctx.sync()
        F = FLD[group]
        diff = c["diff"][:n]
        assert_points(group, (a.cpu().numpy().view(np.uint64), ai.cpu().numpy()), diff)
        tripled = [P.ec_mul(F, 3, x) for x in diff]
        assert_points(group, (out.cpu().numpy().view(np.uint64), oi.cpu().numpy()), tripled)
        assert_points(group, (s.cpu().numpy().view(np.uint64), si.cpu().numpy()), [_sum(F, tripled[:100]), _sum(F, tripled[100:])])
