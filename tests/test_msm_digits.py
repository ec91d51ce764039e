"""The MSM's digit recoding and bucket sort (csrc/msm_sort.hip) on the device, against the big-integer model of tests/msm_digits_model.py.

czk_lab_msm_sort (csrc/lab/msm_sort_probe.hip, lab library only) runs the sort of one MSM call on its own -- dimensions, workspace layout and
msm_sort_enqueue are the product's -- and returns its arrays.  Every probe case compares, limb for limb: `digits` with code(recode(...)) for
every lane, window and scalar; per bucket the population, the segment of `sorted` (pairwise disjoint, together exactly [0, non-zero digits),
the multiset of entries equal to the model's, the sentinel untouched behind them); `perm` as a permutation of the buckets in non-increasing
order of min(population, CNT_BINS - 1).  The scalars are the families of the model, which tests/test_msm_digits_cpu.py proves to contain the
edges they are named after.  The end-to-end cases run the same scalars through ctx.msm against the checker's Pippenger, in affine.

Scalars are canonical (below r) throughout: the interface requires it, and values at or above r are not tested.
numpy only carries and compares the arrays here; every expected value is computed by the model on Python integers."""
import numpy as np
import pytest

import msm_digits_model as M
from test_gpu_parity import _bases, _same_point
from util import ints_to_limbs, limbs_to_ints, rand_fr_canonical, R_MOD

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def czk():
    import czk_amd
    return czk_amd


@pytest.fixture(scope="module")
def lab(czk):
    c = czk.Context(0, lab=True)
    yield c
    c.close()


def _rand_ints(seed, n):
    return limbs_to_ints(rand_fr_canonical(seed, n))


def _montgomery(vals):
    return [v * (1 << 256) % R_MOD for v in vals]


def run_probe(lab, case, c, lanes_scalars, size=None, split=False, one_pass=False, montgomery=False, inf=None, nb=None):
    """Runs the probe on `lanes_scalars` (one list of integers per lane) and holds every array to the model.  Returns the probe's output with
    the model's populations per bucket set added ("model_pop")."""
    import czk_amd
    n_scalars = len(lanes_scalars[0])
    assert all(len(l) == n_scalars for l in lanes_scalars)
    size = n_scalars if size is None else size
    nb = size if nb is None else nb
    arr = np.stack([ints_to_limbs(_montgomery(l) if montgomery else l, 4) for l in lanes_scalars])
    out = lab.lab_msm_sort(c, arr, size=size, split=split, one_pass=one_pass, inf=inf, nb=nb,
                           scalar_form=czk_amd.CZK_SCALAR_MONTGOMERY if montgomery else czk_amd.CZK_SCALAR_CANONICAL)
    c, Wd, W, B, total = out["c"], out["Wd"], out["W"], out["B"], out["total"]
    real = len(lanes_scalars)
    assert Wd == M.num_windows(c) and B == 1 << (c - 1) and W == (1 if split else Wd) and out["lanes"] == (real * Wd if split else real)
    assert total == W * size and out["n_parts"] == 1 << out["part_shift"]
    # ---- digits
    flags = None if inf is None else np.asarray(inf, dtype=np.uint8)

    def base_flags(i):
        if flags is None:
            return None
        return [int(flags[i])] * Wd if split else [int(flags[w, i]) for w in range(Wd)]
    model = [[M.recode(s, c, base_flags(i)) for i, s in enumerate(l[:size])] for l in lanes_scalars]      # [lane][i][w]
    want = np.array([[[M.code(model[l][i][w]) for i in range(size)] for w in range(Wd)] for l in range(real)], dtype=np.uint32).reshape(real, Wd, size)
    got = out["digits"].reshape(real, Wd, size)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (case, "digit (lane, window, scalar)", bad[:5].tolist(), [hex(int(got[tuple(b)])) for b in bad[:5]], [hex(int(want[tuple(b)])) for b in bad[:5]])
    # ---- buckets, per bucket set
    sets = [(l, w) for l in range(real) for w in range(Wd)] if split else [(l, None) for l in range(real)]
    placements, pops = set(), []
    for v, (l, w) in enumerate(sets):
        dg = [[model[l][i][w] for i in range(size)]] if split else [[model[l][i][x] for i in range(size)] for x in range(Wd)]
        buckets, pop = M.sort_model(dg, W, nb, B)
        pops.append(pop)
        nnz = sum(pop)
        counts, offsets, srt, perm = (out[k][v].astype(np.int64) for k in ("counts", "offsets", "sorted", "perm"))
        assert np.array_equal(counts, np.array(pop, dtype=np.int64)), (case, v, "counts")
        order = np.array(sorted(buckets, key=lambda b: int(offsets[b])), dtype=np.int64)       # the non-empty buckets by offset: each starts where the last ends
        ends = np.cumsum(counts[order])
        assert np.array_equal(offsets[order], ends - counts[order]) and (nnz == 0 or int(ends[-1]) == nnz), (case, v, "segments")
        for b, want_entries in buckets.items():
            seg = srt[offsets[b]:offsets[b] + counts[b]]
            assert np.array_equal(np.sort(seg), np.array(want_entries, dtype=np.int64)), (case, v, "bucket", b)
        assert np.all(srt[nnz:] == SENTINEL) and not np.any(srt[:nnz] == SENTINEL), (case, v, "sentinel")
        assert np.array_equal(np.sort(perm), np.arange(B)), (case, v, "perm is a permutation")
        key = np.minimum(counts[perm], M.CNT_BINS - 1)
        assert np.all(key[1:] <= key[:-1]), (case, v, "perm order")
        if not one_pass and out["n_parts"]:
            part = np.bincount(np.arange(B) & (out["n_parts"] - 1), weights=counts, minlength=out["n_parts"]).astype(np.int64)
            placements |= {"staged" if n <= out["cap"] else "direct" for n in part.tolist() if n}
    out["model_pop"] = pops
    out["placements"] = placements
    print("probe case %-26s c=%2d lanes=%3d n_parts=%4d cap=%6d %-8s %s" % (case, c, out["lanes"], out["n_parts"], out["cap"], "one-pass" if one_pass else ("split" if split else "table"),
                                                                              "/".join(sorted(placements)) or "-"))   # (pytest -rP: the branches a session reached)
    return out


def two_lanes(c, one=False):
    s = M.edge_scalars(c)
    return [s] if one else [s, s[::-1]]


@pytest.mark.parametrize("c", [8, 13, 14, 16, 19, 20, 21, 22])
def test_sort_widths_table_form(lab, c):
    """window_edges + carry_chains + field_edges, two lanes with different scalars (one at c = 22): the option's lower bound, the mixed widths
    (W_hi = 14, 7, 2), the two-bit top window, and 4 / 512 / 1024 / 2048 partitions (c = 13, 20, 21, 22): each k_part_scatter launch."""
    out = run_probe(lab, f"widths c={c}", c, two_lanes(c, one=c == 22))
    assert out["c"] == c and out["n_parts"] == max(1, (1 << (c - 1)) >> 10)
    if c in (13, 14, 19):
        assert M.full_windows(c) == {13: 14, 14: 7, 19: 2}[c]


def test_sort_montgomery_scalars(lab):
    run_probe(lab, "montgomery c=13", 13, two_lanes(13), montgomery=True)
    run_probe(lab, "montgomery split", 0, two_lanes(13), split=True, montgomery=True)


def _first(c, size, seed):
    """`size` scalars for a table-free call at width c, the hardest first"""
    ch, fe = M.carry_chains(c), M.field_edges(c)
    s = M._below_r(ch[-7:] + fe[3:] + M.window_edges(c) + ch + fe + _rand_ints(seed, max(0, size - 600)))
    return s[:size] if len(s) >= size else s + _rand_ints(seed + 1, size - len(s))


def test_sort_table_free_split_form(lab):
    """the widths choose_c_split gives for 1, 7, 300 and 5000 pairs: per window one bucket set, Wd * n_parts histograms"""
    widths = []
    for size in (1, 7, 300, 5000):
        c = lab.lab_msm_sort(0, np.zeros((2, size, 4), dtype=np.uint64), split=True, dims_only=True)["c"]
        a = _first(c, size, 900 + size)
        out = run_probe(lab, f"split size={size}", 0, [a, a[::-1]], split=True)
        assert out["c"] == c and out["W"] == 1 and out["lanes"] == 2 * M.num_windows(c)
        widths.append(c)
    assert any(c in M.MIXED_WIDTHS for c in widths), widths
    assert len(set(widths)) >= 3, widths


@pytest.mark.parametrize("c", [13, 20])
def test_sort_one_pass(lab, c):
    """the sort of "msm_sort_onepass": 2 scan tiles of 2048 buckets at c = 13, 256 at c = 20"""
    out = run_probe(lab, f"one-pass c={c}", c, two_lanes(c), one_pass=True)
    assert (out["B"] + 2047) // 2048 == {13: 2, 20: 256}[c]


def test_sort_partition_shapes(lab):
    """k_part_sort at c = 13: a partition of exactly `cap` entries is staged in LDS, one of cap + 1 is placed directly; partitions of 1, 1023,
    1024, 1025, 4095, 4096 and 4097 entries sit on either side of the loops' four-entries-per-thread tails."""
    c, n = 13, M.PARTITION_SCALARS
    d = lab.lab_msm_sort(c, np.zeros((1, n, 4), dtype=np.uint64), dims_only=True)
    assert (d["n_parts"], d["part_shift"], d["B"], d["total"]) == (4, 2, 4096, 20 * n) and 4097 < d["cap"] < 19 * n
    lanes = M.partition_shapes(c, d["n_parts"], d["part_shift"], d["cap"], n)
    out = run_probe(lab, "partition_shapes c=13", c, lanes)
    assert out["cap"] == d["cap"]
    sizes = sorted(sum(pop[b] for b in range(p, out["B"], 4)) for pop in out["model_pop"] for p in range(4))
    assert [s for s in sizes if s] == sorted((d["cap"], d["cap"] + 1) + M.PARTITION_SIZES)
    assert out["placements"] == {"staged", "direct"}
    hit = {b for pop in out["model_pop"] for b, k in enumerate(pop) if k}
    assert {0, out["B"] - 1} <= hit and any(b >> 2 == 1023 for b in hit)


def _population_checks(out, c, v_sets):
    bk = M.population_buckets(c)
    for v, targets in v_sets.items():
        counts, perm = out["counts"][v], out["perm"][v]
        for b, t in targets.items():
            assert counts[b] == t
        big = [b for b, t in targets.items() if t >= M.CNT_BINS - 1]
        assert set(perm[:len(big)].tolist()) == set(big)                       # CNT_BINS - 1 and CNT_BINS share the last bin, in either order
        rest = sorted((b for b in targets if b not in big), key=lambda b: -targets[b])
        assert perm[len(big):len(big) + len(rest)].tolist() == rest          # then 2046, 2, 1 (distinct populations: the order is fixed)
    return bk


def test_sort_populations_at_the_clamp(lab):
    """Buckets of exactly CNT_BINS - 2, CNT_BINS - 1 and CNT_BINS entries (and 2, 1, 0): the clamp of the population order."""
    c = 13
    bk, tg = M.population_buckets(c), M.POPULATION_TARGETS
    out = run_probe(lab, "populations c=13", c, [M.populations(c, M.num_windows(c))])
    assert sorted(k for k in out["model_pop"][0] if k) == [1, 2, 2046, 2047, 2048]
    _population_checks(out, c, {0: dict(zip(bk, tg))})
    size = M.POPULATION_SPLIT_SCALARS
    c = lab.lab_msm_sort(0, np.zeros((1, size, 4), dtype=np.uint64), split=True, dims_only=True)["c"]
    bk = M.population_buckets(c)
    assert len(bk) == 5
    out = run_probe(lab, "populations split", 0, [M.populations(c, 1)], split=True)
    _population_checks(out, c, {0: {bk[0]: tg[0], bk[3]: tg[3], bk[4]: tg[4]}, 1: {bk[0]: tg[1]}, 2: {bk[0]: tg[2]}})


def test_sort_one_bucket(lab):
    """Every entry of a lane in one bucket (d = 1, a middle one, the largest that fits every window, 2^(c-1)): one partition, one segment,
    more than CNT_BINS entries."""
    c = 13
    ds = M.one_bucket_digits(c)
    lanes = [(M.one_bucket_scalars(c, d) * 130)[:130] for d in ds]
    out = run_probe(lab, "one_bucket c=13", c, lanes)
    for v, d in enumerate(ds):
        assert [b for b, k in enumerate(out["model_pop"][v]) if k] == [d - 1] and out["perm"][v][0] == d - 1
    assert max(max(p) for p in out["model_pop"]) > M.CNT_BINS
    one = (M.one_bucket_scalars(c, ds[1]) * 700)[:2100]
    out = run_probe(lab, "one_bucket split", c, [one], split=True)
    assert all(sum(1 for k in pop if k) <= 1 for pop in out["model_pop"]) and max(max(p) for p in out["model_pop"]) == 2100


def test_sort_long_call_at_a_narrow_width(lab):
    """70 000 scalars at c = 8: the long-call rule raises the partitions to the bucket count (128 partitions of one bucket each)."""
    out = run_probe(lab, "long call c=8", 8, [_rand_ints(0x70000, 70000)])
    assert out["B"] == 128 and out["n_parts"] == 128 and out["part_shift"] == 7


@pytest.mark.parametrize("split", [False, True], ids=["table", "split"])
def test_sort_size_below_scalars_and_bases_with_flagged_bases(lab, split):
    """size < n_scalars (more scalars than bases) and size < nb (fewer scalars than bases); base 3 is at infinity, base 7 in window 2 only
    (table form: a table entry can be at infinity on its own), Montgomery scalars in the second run."""
    c = 13
    Wd = M.num_windows(c)
    s = M.edge_scalars(c)

    def flags(nb):
        f = np.zeros(nb if split else (Wd, nb), dtype=np.uint8)
        if split:
            f[[3, 7]] = 1
        else:
            f[:, 3] = 1
            f[2, 7] = 1
        return f
    out = run_probe(lab, "more scalars than bases", c, [s[:40], s[40:80]], size=25, nb=25, split=split, inf=flags(25))
    assert not out["digits"].reshape(2, Wd, 25)[:, :, 3].any() and out["digits"].reshape(2, Wd, 25)[:, :, 4].any()
    out = run_probe(lab, "fewer scalars than bases", c, [s[100:125], s[130:155]], size=25, nb=40, split=split, inf=flags(40), montgomery=True)
    assert not out["digits"].reshape(2, Wd, 25)[:, 2, 7].any()


def test_lab_msm_sort_needs_the_lab_library(czk):
    c = czk.Context(0)
    with pytest.raises(RuntimeError):
        c.lab_msm_sort(13, np.zeros((1, 1, 4), dtype=np.uint64))
    c.close()


# ---- end to end: the same scalars through ctx.msm, against the checker's Pippenger
def _key(ctx, orc, g, n, seed):
    """n random bases with one at infinity, one equal pair and one opposite pair (as test_msm_matches_reference_pippenger arranges them)"""
    _, bases = _bases(ctx, g, n, seed)
    inf = np.zeros(n, dtype=np.uint8)
    bases[3] = bases[2]
    aw = bases.shape[1] // 2
    neg = bases[4].copy()
    neg[aw:] = orc.fq_neg(bases[4][aw:]) if g == 1 else np.concatenate([orc.fq_neg(bases[4][aw:aw + 6]), orc.fq_neg(bases[4][aw + 6:])])
    bases[5] = neg
    inf[7] = 1
    return bases, inf


def _end_to_end(ctx, czk, orc, g, scalars, flags=0, want_c=None):
    n = len(scalars)
    bases, inf = _key(ctx, orc, g, n, 7000 + n)
    sc = ints_to_limbs(scalars, 4)
    b = ctx.register_bases(g, bases, inf, mem=czk.CZK_MEM_HOST | flags)
    if want_c is not None:
        assert b.layout_for(n)[0] == want_c
    want = orc.msm(g, bases, inf, sc)
    ok = _same_point(ctx, orc, g, ctx.msm(b, sc)[0], want)
    ok_m = _same_point(ctx, orc, g, ctx.msm(b, orc.fr_from_repr(sc), scalar_form=czk.CZK_SCALAR_MONTGOMERY)[0], want)
    b.release()
    assert ok and ok_m, (g, n, ok, ok_m)


@pytest.mark.parametrize("c", [8, 13, 16, 19, 21, 22])
def test_msm_edge_scalars_g1_tables(czk, orc, c):
    ctx = czk.Context(0, options={"msm_slots": 1, "msm_window_g1": c, "msm_fixed_c": 1})
    _end_to_end(ctx, czk, orc, 1, M.edge_scalars(c), want_c=c)
    ctx.close()


@pytest.mark.parametrize("c", [13, 19])
def test_msm_edge_scalars_g1_xyzz_kernels(czk, orc, c):
    ctx = czk.Context(0, lab=True, options={"msm_slots": 1, "msm_window_g1": c, "msm_fixed_c": 1, "msm_no_te": 1})
    _end_to_end(ctx, czk, orc, 1, M.edge_scalars(c), want_c=c)
    ctx.close()


@pytest.mark.parametrize("c", [8, 13, 19])
def test_msm_edge_scalars_g2_tables(czk, orc, c):
    ctx = czk.Context(0, options={"msm_slots": 1, "msm_window_g2": c, "msm_fixed_c": 1})
    _end_to_end(ctx, czk, orc, 2, M.edge_scalars(c), want_c=c)
    ctx.close()


@pytest.mark.parametrize("g", [1, 2])
def test_msm_edge_scalars_table_free(czk, orc, lab, g):
    """A table-free key picks its width from the call's size: 300 pairs, the whole family of the width such a call gets and random scalars behind it."""
    n = 300
    c = lab.lab_msm_sort(0, np.zeros((1, n, 4), dtype=np.uint64), split=True, dims_only=True)["c"]
    sc = M.edge_scalars(c)
    assert len(sc) <= n
    sc = sc + _rand_ints(78, n - len(sc))
    ctx = czk.Context(0, options={"msm_slots": 1})
    _end_to_end(ctx, czk, orc, g, sc, flags=czk.CZK_MEM_NO_TABLES, want_c=c)
    ctx.close()


@pytest.mark.parametrize("g", [1, 2])
def test_msm_one_bucket(czk, orc, g):
    """a single bucket receives every window multiple of every base, with both signs"""
    c = 13
    ctx = czk.Context(0, options={"msm_slots": 1, "msm_window_g1": c, "msm_window_g2": c, "msm_fixed_c": 1})
    _end_to_end(ctx, czk, orc, g, (M.one_bucket_scalars(c, M.one_bucket_digits(c)[1]) * 40)[:100], want_c=c)
    ctx.close()
