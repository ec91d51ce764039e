"""The MSM's bucket accumulation and bucket reduction on the device, stage by stage, against the integer model of tests/msm_buckets_model.py.

czk_lab_msm_buckets (csrc/lab/msm_bucket_probe.hip, lab library only) runs the launches of the accumulate and reduce stages (msm.hip
msm_accumulate_enqueue / msm_fixup_enqueue / msm_reduce_enqueue, the functions msm_stage_accumulate and msm_stage_reduce call) on entry lists
written here, over the tables of a registered key, and returns every bucket as a Jacobian triple, the counters of the rare paths (raw exc_count,
dirty buckets, work items, over-full buckets, the overflow flag) and the reduction's result per lane.  Every case checks ALL of them: buckets in
affine against [exponent] G from the checker's fixed-base MSM (empty buckets must read as infinity), lane results against sum (b + 1) bucket_b,
counters against the model's control flow.  The entry lists come from the named builders of the model, which tests/test_msm_buckets_cpu.py
proves to contain what their names say.

Families: G1 twisted Edwards (k_accumulate_te), G1 u-form XYZZ (CZK_MEM_ANY_POINTS: k_accumulate_u, XyzzOps), G2 (k_accumulate_u2, Xyzz2Ops), and
one table-free key (CZK_MEM_NO_TABLES) per group.  The twisted Edwards family has no exception list: its exception and dirty counts are 0.

Exception counts are asserted EQUAL to the model's.  The filters of fqu_xyzz_acc_mixed / fq2u_xyzz_acc_mixed admit false positives at about
2^-24 per addition; the probe's order is deterministic, so a seeded case either meets one always or never, and none of the seeds here does.

Points of even order: E(Fq) has the three points of order two (-1, 0), (-zeta, 0), (-zeta^2, 0), and the u-form G1 family serves keys that may
hold them; the cases at the end place them alone, twice and beside an odd-order point, at B = 128 (the tail's Horner doublings meet them) and
B = 2 048 (the level kernel's doublings too).  G2 has no such case: the twist y^2 = x^3 + b' has a point (x, 0) only if -b' is a cube in Fq2,
and (-b')^((q^2 - 1) / 3) != 1 (test_twist_has_no_point_of_order_two computes it), so xyzzu2_double's Y == 0 route is unreachable from curve points.

The last section runs the same edges through the product library (czk_msm_g1, registered CZK_MEM_ANY_POINTS keys).

Measured on one MI355X: the 231 cases of this file in 21 s; the slowest case (the exception list over 3 x 2 048 G2 buckets) 0.7 s."""
import random

import numpy as np
import pytest

import msm_buckets_model as M
import msm_digits_model as D
import pairing_ref as PR
from util import ints_to_limbs

pytestmark = pytest.mark.gpu

FAMILIES = ("g1_te", "g1_u", "g2", "g1_split", "g2_split")
TABLED = ("g1_te", "g1_u", "g2")


@pytest.fixture(scope="module")
def czk():
    import czk_amd
    return czk_amd


@pytest.fixture(scope="module")
def lab(czk):
    c = czk.Context(0, lab=True)
    yield c
    c.close()


class Fam:
    def __init__(self, name, g, handle, key, family):
        self.name, self.g, self.handle, self.key, self.family = name, g, handle, key, family


@pytest.fixture(scope="module")
def fams(czk, lab, orc):
    """One 512-base key per family, bases [k_i] G from the checker's fixed-base MSM; the model's table from the dimensions the probe reports."""
    ks = M.key_exponents(0xB0C)
    pts = {g: orc.fixed_base_points(g, ints_to_limbs(ks, 4))[0] for g in (1, 2)}
    flags = {"g1_te": (1, 0), "g1_u": (1, czk.CZK_MEM_ANY_POINTS), "g2": (2, 0), "g1_split": (1, czk.CZK_MEM_NO_TABLES), "g2_split": (2, czk.CZK_MEM_NO_TABLES)}
    out = {}
    for name, (g, mem) in flags.items():
        h = lab.register_bases(g, pts[g], None, mem=czk.CZK_MEM_HOST | mem)
        d = lab.lab_msm_buckets(h, 128, np.zeros((1, 1), np.uint32), *[np.zeros((1, 128), np.uint32)] * 3, dims_only=True)
        assert d["nb"] == M.N_BASES and (d["heavy_chunk"], d["heavy_sub"]) == (M.HEAVY_CHUNK, M.HEAVY_SUB)
        assert d["exc_cap"] == (0 if d["family"] == M.FAM_TE else M.EXC_CAP)
        assert (d["c"] == 0 and d["W"] == 1) if "split" in name else (d["c"], d["W"]) == h.layout()
        out[name] = Fam(name, g, h, M.Key(M.ExpGroup, M.table_exponents(ks, d["c"], d["W"]), d["nb"], d["W"]), d["family"])
    assert out["g1_te"].family == M.FAM_TE and out["g1_u"].family == out["g2"].family == out["g2_split"].family == M.FAM_U
    yield out
    for f in out.values():
        f.handle.release()


def _expected_points(orc, fam, values):
    """values: group elements of the family's key, in order -> (affine limbs, infinity flags)"""
    if fam.key.G is M.ExpGroup:
        aff, inf = orc.fixed_base_points(fam.g, ints_to_limbs([v % M.R_MOD for v in values] or [0], 4))
        return aff[:len(values)], inf[:len(values)]
    rows = [PR.g1_to_limbs(v) for v in values]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(len(values), 12), np.array([r[1] for r in rows], dtype=np.uint8)


def run_case(lab, orc, fam, case, tag, seed=1):
    """Runs the probe on a case and holds every bucket, every lane result and every counter to the model.  Returns the probe's output."""
    exp = M.expect(fam.key.G, fam.key.vals, case, fam.family)
    B, n_lanes = case["B"], len(case["lanes"])
    out = lab.lab_msm_buckets(fam.handle, B, *M.layout(case, seed))
    print("probe case %-40s %-8s B=%5d lanes=%d exc=%5d dirty=%4d items=%4d heavy=%d" % (tag, fam.name, B, n_lanes, out["exc_count"], out["dirty"], out["items"], out["heavy"]))
    # ---- counters
    assert out["overflow"] == 0 and out["items"] == exp["items"] and out["heavy"] == exp["heavy"], (tag, fam.name, "work items")
    if exp["exact"]:
        assert (out["exc_count"], out["dirty"]) == (exp["exc_count"], exp["dirty"]), (tag, fam.name, "exceptions", exp["exc_count"], exp["dirty"])
    else:
        assert out["exc_count"] >= exp["exc_count"] and out["dirty"] >= exp["dirty"], (tag, fam.name, "exceptions (lower bounds)")
    # ---- buckets, all of them
    aw = 12 if fam.g == 1 else 24
    got_aff, got_inf = lab.jac_to_affine(fam.g, out["buckets"].reshape(n_lanes * B, -1))
    where = [(ln, b) for ln in range(n_lanes) for b in sorted(exp["buckets"][ln])]
    want_aff, want_flag = _expected_points(orc, fam, [exp["buckets"][ln][b] for ln, b in where])
    want_inf = np.ones(n_lanes * B, dtype=np.uint8)
    full = np.zeros((n_lanes * B, aw), dtype=np.uint64)
    for k, (ln, b) in enumerate(where):
        want_inf[ln * B + b] = want_flag[k]
        full[ln * B + b] = want_aff[k]
    bad = np.flatnonzero(got_inf != want_inf)
    assert bad.size == 0, (tag, fam.name, "bucket infinity flags (lane * B + bucket)", bad[:8].tolist())
    fin = want_inf == 0
    bad = np.flatnonzero((got_aff[fin] != full[fin]).any(axis=1))
    assert bad.size == 0, (tag, fam.name, "buckets (index among the finite ones)", bad[:8].tolist())
    # ---- lane results (the checker's own conversion)
    res_aff, res_inf = _expected_points(orc, fam, exp["results"])
    for ln in range(n_lanes):
        aff, inf = orc.jac_to_affine(fam.g, out["result"][ln])
        assert inf == bool(res_inf[ln]) and (inf or np.array_equal(aff, res_aff[ln])), (tag, fam.name, "result of lane", ln)
    return out


# ---------------------------------------------------------------------------------------------------- accumulation
@pytest.mark.parametrize("name", FAMILIES)
def test_first_entry_and_short_chains(lab, orc, fams, name):
    """One entry, plain and negated; P, P; P, -P; P, P, P; P, -P, Q; Q1, Q2, -(Q1 + Q2) in three orders; higher-window entries."""
    run_case(lab, orc, fams[name], M.short_chains(fams[name].key), "short chains")


@pytest.mark.parametrize("cnt", M.EDGE_COUNTS)
@pytest.mark.parametrize("name", FAMILIES)
def test_chunk_edges(lab, orc, fams, name, cnt):
    """Entry counts either side of HEAVY_CHUNK and of a work item's edge; 1 024 + 128 * 256 and one more drive k_heavy_combine's strided loop."""
    out = run_case(lab, orc, fams[name], M.chunk_edge(fams[name].key, cnt), "chunk edge %d" % cnt)
    assert out["items"] == max(0, -(-(cnt - M.HEAVY_CHUNK) // M.HEAVY_SUB)) and out["exc_count"] == 0


@pytest.mark.parametrize("pos", [2, 1024, 1025])
@pytest.mark.parametrize("name", FAMILIES)
def test_exceptional_addition_at_a_chosen_place(lab, orc, fams, name, pos):
    f = fams[name]
    out = run_case(lab, orc, f, M.exceptional_at(f.key, pos), "accumulator's value as entry %d" % pos)
    assert out["exc_count"] == (0 if f.family == M.FAM_TE or pos == 1025 else 1)


@pytest.mark.parametrize("name", FAMILIES)
def test_equal_and_opposite_partials(lab, orc, fams, name):
    out = run_case(lab, orc, fams[name], M.equal_opposite_partials(fams[name].key), "equal / opposite partial sums")
    assert out["heavy"] == 4 and out["items"] == 2 + 3 + 4 + 4


@pytest.mark.parametrize("n", M.CAP_COUNTS)
@pytest.mark.parametrize("name", FAMILIES)
def test_exception_list_cap(lab, orc, fams, name, n):
    """n buckets (P_b, P_b) over 3 lanes of 2 048: exc_count = n, dirty = max(0, n - cap), every bucket 2 P_b."""
    f = fams[name]
    out = run_case(lab, orc, f, M.exception_cap(f.key, n), "exception list %d" % n)
    if f.family != M.FAM_TE:
        assert out["exc_count"] == n and out["dirty"] == max(0, n - M.EXC_CAP)


@pytest.mark.parametrize("name", FAMILIES)
def test_overfull_and_dirty(lab, orc, fams, name):
    """Five buckets of 1 024 + 300 copies of one point: 5 x 1 023 exceptional additions, more than the cap, so at least one over-full bucket is dirty
    whatever the schedule: k_heavy_combine skips it and the fix-up recomputes it from all of its entries."""
    f = fams[name]
    out = run_case(lab, orc, f, M.overfull_same_point(f.key, 5), "over-full and dirty")
    assert out["heavy"] == 5
    if f.family != M.FAM_TE:
        assert out["dirty"] >= 1 and out["exc_count"] > M.EXC_CAP


@pytest.mark.parametrize("name", FAMILIES)
def test_overfull_with_deferred_points(lab, orc, fams, name):
    f = fams[name]
    out = run_case(lab, orc, f, M.overfull_same_point(f.key, 1), "over-full with deferred points")
    if f.family != M.FAM_TE:
        assert (out["exc_count"], out["dirty"]) == (M.HEAVY_CHUNK - 1, 0)


@pytest.mark.parametrize("interleave", [1, 2, 4])
@pytest.mark.parametrize("lanes", [1, 3, 4, 5])
@pytest.mark.parametrize("name", TABLED)
def test_lanes_and_interleave(lab, orc, fams, name, lanes, interleave):
    """Different content and a different perm in every lane; with 5 lanes and groups of 4 the last group is a single lane."""
    lab.set_option("msm_lane_interleave", interleave)
    try:
        run_case(lab, orc, fams[name], M.lanes_random(fams[name].key, lanes), "lanes %d interleave %d" % (lanes, interleave), seed=lanes)
    finally:
        lab.set_option("msm_lane_interleave", 0)


# ---------------------------------------------------------------------------------------------------- reduction
@pytest.mark.parametrize("aimed", list(M.AIMED))
@pytest.mark.parametrize("name", TABLED)
def test_reduce_aimed_buckets(lab, orc, fams, name, aimed):
    run_case(lab, orc, fams[name], M.singles(fams[name].key, M.AIMED[aimed], 2048), aimed)


@pytest.mark.parametrize("B", [128, 1024, 2048, 16384])
@pytest.mark.parametrize("name", FAMILIES)
def test_reduce_shapes(lab, orc, fams, name, B):
    """Tail only; the tail at its limit; one level; two levels, the second reading E_in."""
    run_case(lab, orc, fams[name], M.reduce_shapes(fams[name].key, B), "reduce B = %d" % B)


@pytest.mark.parametrize("B", [128, 2048, 16384])
@pytest.mark.parametrize("opposite", [False, True])
@pytest.mark.parametrize("name", TABLED)
def test_reduce_neighbours_equal_or_opposite(lab, orc, fams, name, opposite, B):
    run_case(lab, orc, fams[name], M.neighbours(fams[name].key, B, opposite), "neighbours %s" % ("opposite" if opposite else "equal"))


@pytest.mark.parametrize("B", [128, 2048])
@pytest.mark.parametrize("name", TABLED)
def test_reduce_all_buckets_the_same_point(lab, orc, fams, name, B):
    run_case(lab, orc, fams[name], M.all_same(fams[name].key, B), "all the same point")


@pytest.mark.parametrize("name", TABLED)
def test_reduce_chunk_whose_A_and_E_cancel(lab, orc, fams, name):
    run_case(lab, orc, fams[name], M.level_cancel(fams[name].key), "A and E cancel")


@pytest.mark.parametrize("B", [128, 2048, 16384])
@pytest.mark.parametrize("name", TABLED)
def test_reduce_everything_neutral(lab, orc, fams, name, B):
    out = run_case(lab, orc, fams[name], M.neutral(B), "everything neutral")
    assert lab.jac_to_affine(fams[name].g, out["result"])[1].all()


# ---------------------------------------------------------------------------------------------------- the probe refuses what it could not read safely
def test_probe_rejects_bad_lists(czk, lab, fams):
    f = fams["g1_u"]
    B, good = 128, M.layout(M.short_chains(f.key))
    table = f.key.nb * f.key.W

    def bad(k, fn):
        arrs = [np.array(a, dtype=np.uint32) for a in good]
        fn(arrs[k])
        with pytest.raises(czk.CzkError):
            lab.lab_msm_buckets(f.handle, B, *arrs)
    off0 = good[1][0][0]                                  # bucket 0 holds one entry

    def outside(a):
        a[0, off0] = table                                # an entry index one past the table

    def outside_neg(a):
        a[0, off0] = table | M.NEG

    def seg(a):
        a[0, 0] = 2 ** 32 - 1                             # offsets: a segment that starts far outside `sorted`

    def seg_len(a):
        a[0, 0] = len(good[0][0]) + 1                     # counts: a segment longer than `sorted`

    def perm_dup(a):
        a[0, 0] = a[0, 1]

    def perm_big(a):
        a[0, 5] = B
    for k, fn in ((0, outside), (0, outside_neg), (1, seg), (2, seg_len), (3, perm_dup), (3, perm_big)):
        bad(k, fn)
    lab.lab_msm_buckets(f.handle, B, *good)               # and the unmodified lists pass


# ---------------------------------------------------------------------------------------------------- points of even order
def _order_two_points():
    q = PR.Q
    zeta = next(z for z in (pow(g, (q - 1) // 3, q) for g in range(2, 20)) if z != 1)
    return (q - 1, 0), (-zeta % q, 0)


def _limbs_of(points):
    return np.array([PR.g1_to_limbs(p)[0] for p in points], dtype=np.uint64)


@pytest.fixture(scope="module")
def tkey(czk, lab):
    """Bases 0, 1: the points of order two (-1, 0) and (-zeta, 0); bases 2 .. 5: [3] G, [5] G, [7] G, [11] G.  CZK_MEM_ANY_POINTS."""
    pts = list(_order_two_points()) + [PR.g1_mul(k) for k in (3, 5, 7, 11)]
    h = lab.register_bases(1, _limbs_of(pts), None, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_ANY_POINTS)
    d = lab.lab_msm_buckets(h, 128, np.zeros((1, 1), np.uint32), *[np.zeros((1, 128), np.uint32)] * 3, dims_only=True)
    assert d["family"] == M.FAM_U and d["nb"] == len(pts)
    yield Fam("g1_u_T", 1, h, M.Key(M.PointGroup, pts, len(pts), 1), M.FAM_U)
    h.release()


def test_twist_has_no_point_of_order_two():
    """-b' is not a cube in Fq2: no (x, 0) on the twist, so G2 needs no even-order case."""
    minus_b = PR.fq2_neg(PR.G2_B)
    assert (PR.Q * PR.Q - 1) % 3 == 0 and PR.fq2_pow(minus_b, (PR.Q * PR.Q - 1) // 3) != (1, 0)


@pytest.mark.parametrize("B", [128, 2048])
@pytest.mark.parametrize("arrangement", ["alone", "twice", "beside"])
def test_points_of_order_two(lab, orc, tkey, arrangement, B):
    """T alone in bucket j >= 2 is doubled by the reduction (Horner doublings of the tail at B = 128, the level kernel's scaling at B = 2 048): the
    doubling of a point with Y == 0 must give the neutral element, flag set, or the later additions run the general formula on zz == 0."""
    run_case(lab, orc, tkey, M.torsion(arrangement, B), "order two, %s" % arrangement)


# ---------------------------------------------------------------------------------------------------- the same edges through the product library
@pytest.fixture(scope="module")
def ctx(czk):
    c = czk.Context(0)
    yield c
    c.close()


def _affine(ctx, orc, jac):
    aff, inf = orc.jac_to_affine(1, jac)
    aff2, inf2 = ctx.jac_to_affine(1, jac)
    assert inf == bool(inf2[0]) and (inf or np.array_equal(aff, aff2[0]))
    return PR.INF if inf else PR.g1_from_limbs([int(x) for x in aff], 0)


@pytest.mark.parametrize("s", [3, 65])
@pytest.mark.parametrize("which", [0, 1])
def test_product_single_point_of_order_two(czk, ctx, orc, which, s):
    """[3] T = [65] T = T through czk_msm_g1 (table-free, complete on every curve point) and through a registered CZK_MEM_ANY_POINTS key."""
    T = _order_two_points()[which]
    base, sc = _limbs_of([T]), ints_to_limbs([s], 4)
    assert _affine(ctx, orc, ctx.msm_oneshot(1, base, None, sc)[0]) == T
    b = ctx.register_bases(1, base, None, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_ANY_POINTS)
    assert b.arith() == 1
    assert _affine(ctx, orc, ctx.msm(b, sc)[0]) == T
    b.release()


def test_product_order_two_alone_in_its_bucket(czk, ctx, orc):
    """T among 300 subgroup points, its scalar a single odd digit d that no digit of the other scalars equals in absolute value: bucket d - 1 holds T alone."""
    rng = random.Random(0x70)
    n, T = 300, _order_two_points()[0]
    ks = [rng.randrange(1, M.R_MOD) for _ in range(n)]
    bases = np.concatenate([orc.fixed_base_points(1, ints_to_limbs(ks, 4))[0], _limbs_of([T])])
    b = ctx.register_bases(1, bases, None, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_ANY_POINTS)
    c = b.layout_for(n + 1)[0]
    W, d = D.num_windows(c), 37
    assert d <= D.half(c, 0)
    sc = []
    for _ in range(n):
        digits = [rng.choice([x for x in range(-D.half(c, w) + 1, D.half(c, w) + 1) if abs(x) != d]) for w in range(W - 2)] + [rng.randrange(1, 30), 0]
        sc.append(D.compose(digits, c))
        assert all(abs(x) != d for x in D.recode(sc[-1], c))
    want = PR.ec_add(PR.F1, PR.g1_mul(sum(k * s for k, s in zip(ks, sc)) % M.R_MOD), T)
    assert _affine(ctx, orc, ctx.msm(b, ints_to_limbs(sc + [d], 4))[0]) == want
    b.release()


def test_product_overfull_bucket_any_points_key(czk, ctx, orc):
    """3 000 scalars equal to 1 on a CZK_MEM_ANY_POINTS key: one bucket of 3 000 entries (k_accumulate_u, eight work items, k_heavy_combine on u-form
    bucket storage), against [sum k_i] G."""
    rng = random.Random(0x71)
    ks = [rng.randrange(1, M.R_MOD) for _ in range(3000)]
    b = ctx.register_bases(1, orc.fixed_base_points(1, ints_to_limbs(ks, 4))[0], None, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_ANY_POINTS)
    assert b.arith() == 1
    want, _ = orc.fixed_base_points(1, ints_to_limbs([sum(ks) % M.R_MOD], 4))
    got = ctx.msm(b, ints_to_limbs([1] * 3000, 4))
    assert _affine(ctx, orc, got[0]) == PR.g1_from_limbs([int(x) for x in want[0]], 0)
    b.release()
