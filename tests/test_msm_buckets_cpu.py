"""The integer model of the bucket accumulation and reduction (tests/msm_buckets_model.py) against the checker, and its case builders against
their names: the counts at the named thresholds, the number of exceptional additions, partial sums equal or opposite where claimed.  The constants
the model mirrors are read from the source text.  No GPU."""
import os
import random
import re

import numpy as np
import pytest

import msm_buckets_model as M
import msm_digits_model as D
import pairing_ref as PR
from util import ints_to_limbs

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "collaborative-zksnark_amd", "csrc")
G = M.ExpGroup


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def test_constants_are_the_sources():
    acc = _src("msm_acc.h")
    assert _const(acc, "HEAVY_CHUNK") == M.HEAVY_CHUNK and _const(acc, "HEAVY_SUB") == M.HEAVY_SUB and _const(acc, "TAIL_MAX") == M.TAIL_MAX
    assert _const(_src("czk_internal.h"), "MSM_L") == M.MSM_L and _const(_src("czk_internal.h"), "MSM_LOG_L") == M.MSM_L.bit_length() - 1
    assert _const(_src("msm_acc_g1.hip"), "G1_EXC_CAP") == M.EXC_CAP and _const(_src("msm_acc_g2.hip"), "G2_EXC_CAP") == M.EXC_CAP
    assert re.search(r"for \(u32 j = tid; j < extra; j \+= %d\)" % M.COMBINE_THREADS, acc)          # k_heavy_combine's strided loop
    assert "n_in > %d" % M.TAIL_MAX in _src("msm.hip")                                                # the level loop's threshold
    probe = _src(os.path.join("lab", "msm_bucket_probe.hip"))                                         # the probe reports what the kernels use
    assert (_const(probe, "PROBE_HEAVY_CHUNK"), _const(probe, "PROBE_HEAVY_SUB"), _const(probe, "PROBE_EXC_CAP")) == (M.HEAVY_CHUNK, M.HEAVY_SUB, M.EXC_CAP)


@pytest.fixture(scope="module")
def key():
    ks = M.key_exponents(0xB0C)
    c = 9
    W = D.num_windows(c)
    return M.Key(G, M.table_exponents(ks, c, W), M.N_BASES, W), ks, c


def _affine_of_exponents(orc, g, exps):
    pts, inf = orc.fixed_base_points(g, ints_to_limbs([e % M.R_MOD for e in exps], 4))
    return pts, inf


@pytest.mark.parametrize("g", [1, 2])
@pytest.mark.parametrize("c,n", [(8, 40), (9, 200), (5, 64)])
def test_model_result_is_the_checkers_msm(orc, g, c, n):
    """Scalars -> signed digits -> sorted entry lists (tests/msm_digits_model.py) -> the model's buckets and lane result, as an exponent, against
    the checker's Pippenger over the same bases and scalars, in affine."""
    rng = random.Random(1000 * c + n + g)
    ks = [rng.randrange(1, M.R_MOD) for _ in range(n)]
    sc = [rng.randrange(M.R_MOD) for _ in range(n)]
    sc[3], sc[5] = 0, M.R_MOD - 1
    W, B = D.num_windows(c), 1 << (c - 1)
    digits = [D.recode(s, c) for s in sc]
    buckets, _ = D.sort_model([[digits[i][w] for i in range(n)] for w in range(W)], W, n, B)
    vals = M.table_exponents(ks, c, W)
    exp = M.expect(G, vals, M.case(B, buckets), M.FAM_U)
    assert exp["results"][0] == sum(k * s for k, s in zip(ks, sc)) % M.R_MOD
    bases, inf = _affine_of_exponents(orc, g, ks)
    want, want_inf = orc.jac_to_affine(g, orc.msm(g, bases, inf, ints_to_limbs(sc, 4)))
    have, have_inf = _affine_of_exponents(orc, g, [exp["results"][0]])
    assert not want_inf and not have_inf[0] and np.array_equal(have[0], want)


def test_point_group_agrees_with_exponents(orc):
    """The affine group law used for the even-order cases gives, on subgroup points, what the exponents give."""
    ks = [5, 11, M.R_MOD - 3]
    pts = [PR.g1_mul(k) for k in ks]
    lane = {0: [0, 1], 3: [0, 0, 2 | M.NEG], 6: [1, 1 | M.NEG]}
    a = M.expect(M.PointGroup, pts, M.case(128, lane), M.FAM_U)
    b = M.expect(G, ks, M.case(128, lane), M.FAM_U)
    assert a["exc_count"] == b["exc_count"] == 2 and a["buckets"][0][6] is PR.INF and b["buckets"][0][6] == 0
    assert a["results"][0] == PR.g1_mul(b["results"][0]) and a["buckets"][0][3] == PR.g1_mul(b["buckets"][0][3])


def test_layout_is_what_the_probe_accepts(key):
    k, _, _ = key
    cs = M.lanes_random(k, 3)
    srt, off, cnt, perm = M.layout(cs, seed=5)
    total = len(srt[0])
    for ln, lane in enumerate(cs["lanes"]):
        assert sorted(perm[ln]) == list(range(128)) and perm[ln] != perm[(ln + 1) % 3]
        assert all(cnt[ln][perm[ln][i]] >= cnt[ln][perm[ln][i + 1]] for i in range(127))
        used = []
        for b in range(128):
            assert 0 <= off[ln][b] and off[ln][b] + cnt[ln][b] <= total
            assert srt[ln][off[ln][b]:off[ln][b] + cnt[ln][b]] == lane.get(b, [])
            used += range(off[ln][b], off[ln][b] + cnt[ln][b])
        assert len(set(used)) == len(used)
        assert lane != cs["lanes"][(ln + 1) % 3]


# ---------------------------------------------------------------------------------------------------- the builders do what their names say
def test_short_chains(key):
    k, _, _ = key
    cs = M.short_chains(k)
    lane = cs["lanes"][0]
    for b, want in M.CHAINS.items():
        t = M.bucket_trace(G, k.vals, lane[b % cs["B"]])
        assert t["exc"] == want, b
    for b in M.CHAINS_NEUTRAL:
        assert M.bucket_trace(G, k.vals, lane[b])["value"] == 0
    assert lane[1][0] & M.NEG and not lane[0][0] & M.NEG                    # a negated and a plain first entry
    assert M.expect(G, k.vals, cs, M.FAM_U)["exc_count"] == sum(M.CHAINS.values())
    assert M.expect(G, k.vals, cs, M.FAM_TE)["exc_count"] == 0


@pytest.mark.parametrize("cnt", M.EDGE_COUNTS)
def test_chunk_edges(key, cnt):
    k, _, _ = key
    cs = M.chunk_edge(k, cnt)
    t = M.bucket_trace(G, k.vals, cs["lanes"][0][37])
    assert len(cs["lanes"][0][37]) == cnt and t["exc"] == 0 and t["items"] == max(0, -(-(cnt - M.HEAVY_CHUNK) // M.HEAVY_SUB))
    assert t["tree_equal"] == t["tree_opposite"] == 0 and t["last"] == "" and t["value"] != 0
    exp = M.expect(G, k.vals, cs, M.FAM_U)
    assert exp["exc_count"] == 0 and exp["items"] == t["items"] and exp["heavy"] == (cnt > M.HEAVY_CHUNK)


def test_chunk_edges_reach_the_strided_loop():
    assert M.EDGE_COUNTS[-2] == 33792 and M.EDGE_COUNTS[-1] == 33793
    assert -(-(M.EDGE_COUNTS[-2] - M.HEAVY_CHUNK) // M.HEAVY_SUB) == M.COMBINE_THREADS           # 128 items: every thread one
    assert -(-(M.EDGE_COUNTS[-1] - M.HEAVY_CHUNK) // M.HEAVY_SUB) == M.COMBINE_THREADS + 1       # 129: thread 0 takes a second one


@pytest.mark.parametrize("pos,exc,last", [(2, 1, ""), (1024, 1, ""), (1025, 0, "equal")])
def test_exceptional_at(key, pos, exc, last):
    """Entry `pos` is the accumulator's own value: deferred in the main kernel (entries 2 and 1 024), a doubling in k_heavy_combine's last addition
    (entry 1 025, a work item of its own)."""
    k, _, _ = key
    cs = M.exceptional_at(k, pos)
    codes = cs["lanes"][0][5]
    t = M.bucket_trace(G, k.vals, codes)
    X = M.value(G, k.vals, codes[0])
    acc = 0
    for c in codes[:pos - 1]:
        acc = G.add(acc, M.value(G, k.vals, c))
    assert len(codes) == pos and acc == X == M.value(G, k.vals, codes[pos - 1])
    assert t["exc"] == exc and t["last"] == last and t["value"] == 2 * X % M.R_MOD and t["items"] == (pos > M.HEAVY_CHUNK)


def test_equal_opposite_partials(key):
    k, _, _ = key
    lane = M.equal_opposite_partials(k)["lanes"][0]
    t = {b: M.bucket_trace(G, k.vals, lane[b]) for b in (10, 11, 12, 13)}
    assert all(t[b]["exc"] == 0 for b in t)
    p = t[10]["partials"]
    assert len(p) == 2 and p[0] == p[1] != 0 and (t[10]["tree_equal"], t[10]["tree_opposite"]) == (1, 0)
    p = t[11]["partials"]
    assert len(p) == 3 and p[0] == p[1] == G.neg(p[2]) and (t[11]["tree_equal"], t[11]["tree_opposite"]) == (0, 1)
    p = t[12]["partials"]
    assert len(p) == 4 and p[0] == p[2] and p[1] == p[3] and p[0] not in (p[1], G.neg(p[1])) and (t[12]["tree_equal"], t[12]["tree_opposite"]) == (2, 0)
    assert t[13]["items"] == 4 and t[13]["last"] == "opposite" and t[13]["value"] == 0 and t[13]["main"] != 0


@pytest.mark.parametrize("n", M.CAP_COUNTS)
def test_exception_cap(key, n):
    k, _, _ = key
    cs = M.exception_cap(k, n)
    assert cs["B"] == 2048 and len(cs["lanes"]) == 3 and sum(len(l) for l in cs["lanes"]) == n
    assert all(len(c) == 2 and c[0] == c[1] for l in cs["lanes"] for c in l.values())
    exp = M.expect(G, k.vals, cs, M.FAM_U)
    assert exp["exact"] and exp["exc_count"] == n and exp["dirty"] == max(0, n - M.EXC_CAP) and exp["items"] == 0
    assert all(v == 2 * M.value(G, k.vals, cs["lanes"][ln][b][0]) % M.R_MOD for ln in range(3) for b, v in exp["buckets"][ln].items())


def test_overfull_same_point(key):
    k, _, _ = key
    five = M.expect(G, k.vals, M.overfull_same_point(k, 5), M.FAM_U)
    assert not five["exact"] and five["dirty"] == 1 and five["heavy"] == 5 and five["items"] == 10      # 5 x 1 023 > the cap: lower bounds
    assert 5 * (M.HEAVY_CHUNK - 1) > M.EXC_CAP
    cs = M.overfull_same_point(k, 1)
    one = M.expect(G, k.vals, cs, M.FAM_U)
    assert one["exact"] and one["exc_count"] == M.HEAVY_CHUNK - 1 and one["dirty"] == 0 and one["heavy"] == 1 and one["items"] == 2
    assert one["buckets"][0][3] == 1324 * M.value(G, k.vals, cs["lanes"][0][3][0]) % M.R_MOD


def test_reduction_builders(key):
    k, ks, c = key
    for name, bk in M.AIMED.items():
        cs = M.singles(k, bk, 2048)
        assert sorted(cs["lanes"][0]) == sorted(bk) and all(G.add(cs_v, M.expect(G, k.vals, cs, M.FAM_U)["buckets"][1][b]) == 0
                                                            for b, cs_v in M.expect(G, k.vals, cs, M.FAM_U)["buckets"][0].items()), name
    for opp in (False, True):
        e = M.expect(G, k.vals, M.neighbours(k, 2048, opp), M.FAM_U)["buckets"][0]
        assert all(e[b + 1] == (G.neg(e[b]) if opp else e[b]) for b in (0, 3, 6, 15, 1025, 2046))
    e = M.expect(G, k.vals, M.all_same(k, 128), M.FAM_U)
    assert len(set(e["buckets"][0].values())) == 1 and len(e["buckets"][0]) == 128 and e["results"][0] == (128 * 129 // 2) * e["buckets"][0][0] % M.R_MOD
    # level_cancel: second-level chunk 37 = buckets 2368 .. 2431; A (scaled by 2^3) and the sum of its E entries are opposite and not neutral
    cs = M.level_cancel(k)
    e = M.expect(G, k.vals, cs, M.FAM_U)["buckets"][0]
    start = 64 * 37
    run = [sum(e.get(start + 8 * m + t, 0) for t in range(8)) % M.R_MOD for m in range(8)]
    E0 = [sum(t * e.get(start + 8 * m + t, 0) for t in range(8)) % M.R_MOD for m in range(8)]
    A = 8 * sum(m * run[m] for m in range(8)) % M.R_MOD
    assert A != 0 and (A + sum(E0)) % M.R_MOD == 0 and [x != 0 for x in E0] == [True] + [False] * 7
    assert M.neutral(128)["lanes"] == [{}, {}]


def test_torsion_builders():
    """T0 = (-1, 0) and T1 = (-zeta, 0) have order two; the builders place them alone, twice and beside an odd-order point."""
    q = PR.Q
    zeta = next(z for z in (pow(g, (q - 1) // 3, q) for g in range(2, 20)) if z != 1)
    T0, T1 = (q - 1, 0), (-zeta % q, 0)
    for T in (T0, T1):
        assert PR.pyref.ec_on_curve(PR.F1, T, 1) and PR.ec_add(PR.F1, T, T) is PR.INF
    pts = [T0, T1] + [PR.g1_mul(k) for k in (3, 5, 7)]
    PG = M.PointGroup
    for B in (128, 2048):
        e = M.expect(PG, pts, M.torsion("alone", B), M.FAM_U)
        assert e["buckets"][0] == {2: T0, 64: T1, B - 1: T0} and e["exc_count"] == 0
        assert e["results"][0] == PG.add(PG.mul(3, T0), PG.add(PG.mul(65, T1), PG.mul(B, T0))) and e["results"][0] == PG.add(T0, T1)
        e = M.expect(PG, pts, M.torsion("twice", B), M.FAM_U)
        assert e["exc_count"] == 3 and all(e["buckets"][0][b] is PR.INF for b in (2, 64, B - 1))
        e = M.expect(PG, pts, M.torsion("beside", B), M.FAM_U)
        assert e["exc_count"] == 0 and e["buckets"][0][2] == PG.add(T0, pts[2]) and e["buckets"][0][70] == PG.add(T0, T1) and e["buckets"][0][70][1] == 0
