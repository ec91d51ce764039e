"""What tests/test_msm_digits.py feeds the device, proven on the model alone (tests/msm_digits_model.py; no GPU, no library): the window
geometry of every width, the invariants of the recoding on every family member, and that each family contains what it is there for."""
import pytest

import msm_digits_model as M

R = M.R_MOD


@pytest.fixture(scope="module")
def fam():
    return {c: M.families(c) for c in M.WIDTHS}


def test_family_sizes_are_fixed_and_small(fam):
    assert {c: {k: len(v) for k, v in f.items()} for c, f in fam.items()} == M.FAMILY_SIZES
    assert all(n <= 600 for f in M.FAMILY_SIZES.values() for n in f.values())
    # what a width case of the GPU tests runs (the product's table widths start at 7)
    assert all(len(M.edge_scalars(c)) <= 600 for c in M.WIDTHS if c >= 7)
    assert all(len(lane) == M.PARTITION_SCALARS <= 600 for lane in M.partition_shapes(13, 4, 2, 7024))


@pytest.mark.parametrize("c", M.WIDTHS)
def test_windows_tile_the_scalar(c):
    W, hi = M.num_windows(c), M.full_windows(c)
    assert M.win_bit(c, 0) == 0
    for w in range(1, W):
        assert M.win_bit(c, w) == M.win_bit(c, w - 1) + M.win_width(c, w - 1), (c, w)     # starts where the one below ends
    end = M.win_bit(c, W - 1) + M.win_width(c, W - 1)
    assert end >= M.SCALAR_BITS                       # every bit of a scalar and the carry's is in a window
    assert end <= 273 and M.win_bit(c, W - 1) <= 252       # the top window starts inside a scalar's 253 bits; what it spans above bit 255 reads as 0
    # the windows end at bit 254 exactly at the mixed widths -- and at c = 2, which divides 254 and needs no narrower window
    assert (end == M.SCALAR_BITS) == (c in M.MIXED_WIDTHS or c == 2)
    assert (hi < W) == (c in M.MIXED_WIDTHS)
    assert all(M.win_width(c, w) == (c if w < hi else c - 1) for w in range(W))
    if c == 13:
        assert (W, hi, M.win_bit(c, 14), M.win_bit(c, 19)) == (20, 14, 182, 242)
    if c == 19:
        assert (W, hi, M.win_bit(c, 2), M.win_bit(c, 13)) == (14, 2, 38, 236)
    if c == 21:
        assert (W, M.win_bit(c, 12), end) == (13, 252, 273)


@pytest.mark.parametrize("c", M.WIDTHS)
def test_recoding_invariants_on_every_family_member(fam, c):
    members = [s for v in fam[c].values() for s in v] + M.populations(c, 1)
    if c == 13:
        members += [s for lane in M.partition_shapes(13, 4, 2, 7024) for s in lane]
    assert members
    for s in members:
        assert 0 <= s < R
        d, carry = M.recode_carry(s, c)
        assert carry == 0, (c, s)                                                          # no carry leaves the top window
        assert sum(x << M.win_bit(c, w) for w, x in enumerate(d)) == s                     # reconstruction
        assert all(-M.half(c, w) < x <= M.half(c, w) for w, x in enumerate(d))            # range, half-open
        assert M.compose(d, c) == s and M.recode(s, c) == d
        flags = [w % 3 == 1 for w in range(len(d))]
        assert M.recode(s, c, flags) == [0 if f else x for f, x in zip(flags, d)]          # a flagged window's digit is dropped, the carry still runs
    assert M.code(0) == 0 and M.code(5) == 5 and M.code(-5) == 5 | 1 << 31


@pytest.mark.parametrize("c", M.WIDTHS)
def test_window_edges_hold_the_edges_in_every_window(fam, c):
    """Every window w below the top has a scalar with digit +half (the last bucket, no carry), one with -(half - 1) (the first negative digit),
    one whose all-ones window became 0 under a carry that goes on, and one with +half made by a carry.  The top window cannot: a scalar below r
    has a top-window value below half at every width (asserted), so its digit there is never +half nor negative."""
    W = M.num_windows(c)
    digs = [M.recode(s, c) for s in fam[c]["window_edges"]]
    raw = [[(s >> M.win_bit(c, w)) & ((1 << M.win_width(c, w)) - 1) for w in range(W)] for s in fam[c]["window_edges"]]
    top_max = (R - 1) >> M.win_bit(c, W - 1)
    assert top_max + 1 <= M.half(c, W - 1)
    for w in range(W - 1):
        h = M.half(c, w)
        assert sum(1 for d, v in zip(digs, raw) if d[w] == h and v[w] == h) >= 1, (c, w)
        if w:
            assert sum(1 for d, v in zip(digs, raw) if d[w] == h and v[w] == h - 1) >= 1, (c, w)      # half reached by the carry
        assert sum(1 for d in digs if d[w] == -(h - 1) and d[w + 1] >= 1) >= 1, (c, w)
        assert sum(1 for d, v in zip(digs, raw) if v[w] == 2 * h - 1 and d[w] == 0 and w > 0 and d[w + 1] == 1) >= (1 if w else 0), (c, w)
    # the top window: its largest values, with and without a carry from below
    assert any(d[W - 1] == 1 for d in digs) and any(v[W - 1] == 0 and d[W - 1] == 1 for d, v in zip(digs, raw))


@pytest.mark.parametrize("c", M.WIDTHS)
def test_carry_chains_and_field_edges(fam, c):
    W = M.num_windows(c)
    ch = fam[c]["carry_chains"]
    digs = [M.recode(s, c) for s in ch]
    for w in range(1, W):
        k = M.win_bit(c, w)
        if (1 << k) + 1 < R:
            assert {(1 << k) - 1, 1 << k, (1 << k) + 1} <= set(ch)
    # every digit negative except the highest, which is the carry alone: the chain runs through every window below it
    chains = [d for d in digs if d[-1] >= 0 and max(i for i, x in enumerate(d) if x) >= W - 2 and all(x < 0 for x in d[:max(i for i, x in enumerate(d) if x)])]
    assert len(chains) >= (2 if c > 2 else 1) and all(d[max(i for i, x in enumerate(d) if x)] == 1 for d in chains)
    if c == 2:   # half + 1 is all ones: under the carry the window becomes 0 and the carry goes on, through every window
        assert sum(1 for d in digs if d[0] == -1 and not any(d[1:W - 2]) and d[W - 2:].count(1) == 1) >= 1
    # every entry in the last bucket of its window's width, no carry
    assert sum(1 for d in digs if all(x == M.half(c, w) for w, x in enumerate(d[:W - 2]))) >= 1
    # the two alternations of these values: the carry turns the windows of `half` negative as well
    vals = [[(s >> M.win_bit(c, w)) & ((1 << M.win_width(c, w)) - 1) for w in range(W - 2)] for s in ch]
    for ph in (0, 1):
        assert sum(1 for v in vals if all(x == M.half(c, w) + (w % 2 == ph) for w, x in enumerate(v))) >= 1
    # digits that alternate in sign, in both phases
    assert sum(1 for d in digs if all((x < 0) == (w % 2 == 0) for w, x in enumerate(d[:W - 2]))) >= 1
    assert sum(1 for d in digs if all((x < 0) == (w % 2 == 1) for w, x in enumerate(d[:W - 2]))) >= 1
    fe = fam[c]["field_edges"]
    assert {0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, 1 << 252} <= set(fe)
    t = M.top_ones(c)
    bit = M.win_bit(c, W - 1)
    assert t in fe and t < R and t + (1 << bit) >= R and (t + 1) % (1 << bit) == 0


@pytest.mark.parametrize("c", M.WIDTHS)
def test_one_bucket_members_fill_a_single_bucket(fam, c):
    W, B = M.num_windows(c), 1 << (c - 1)
    ds = M.one_bucket_digits(c)
    assert 1 in ds and B in ds and len(ds) >= (3 if c > 3 else 2)
    for d in ds:
        sc = M.one_bucket_scalars(c, d)
        assert sc and set(sc) <= set(fam[c]["one_bucket"])
        digs = [M.recode(s, c) for s in sc]
        bks, pop = M.sort_model([[dg[w] for dg in digs] for w in range(W)], W, len(sc), B)
        assert list(bks) == [d - 1] and sum(pop) == pop[d - 1] == len(bks[d - 1])
        fits = sum(1 for w in range(W - 1) if d <= M.half(c, w))
        assert pop[d - 1] >= len(sc) * (fits - 2) and fits >= 2            # nearly every window that can hold d does
        if d < min(M.half(c, w) for w in range(W)):
            assert any(x < 0 for dg in digs for x in dg) and len(sc) == 3  # both signs land in the bucket


@pytest.mark.parametrize("c", M.WIDTHS)
def test_populations_are_exact(fam, c):
    W, B = M.num_windows(c), 1 << (c - 1)
    bk = M.population_buckets(c)
    tg = M.POPULATION_TARGETS[:len(bk)]
    assert tg[:2] == (M.CNT_BINS - 1, M.CNT_BINS) and (c < 5 or tg == (2047, 2048, 2046, 1, 2))
    # table form: one bucket set
    sc = fam[c]["populations"]
    digs = [M.recode(s, c) for s in sc]
    bks, pop = M.sort_model([[d[w] for d in digs] for w in range(W)], W, len(sc), B)
    assert {b: len(v) for b, v in bks.items()} == dict(zip(bk, tg)) and sum(pop) == sum(tg) and all(pop[b] == t for b, t in zip(bk, tg))
    assert B == len(bk) or 0 in pop
    assert any(x < 0 for d in digs for x in d)
    # table-free form: one bucket set per window
    sc = M.populations(c, 1)
    assert len(sc) == M.POPULATION_SPLIT_SCALARS
    digs = [M.recode(s, c) for s in sc]
    pops = [{b: len(v) for b, v in M.sort_model([[d[w] for d in digs]], 1, len(sc), B)[0].items()} for w in range(W)]
    assert pops[0] == {bk[0]: tg[0], **dict(zip(bk[3:], tg[3:]))}
    assert pops[1] == {bk[0]: tg[1]}
    assert pops[2] == ({bk[0]: tg[2]} if len(tg) > 2 else {})
    assert all(p == {} for p in pops[3:])


def test_partition_shapes_at_width_13():
    """c = 13 on gfx950 with 600 scalars: 4 partitions (part_shift 2) and a staging area of cap = 2 * (20 * 600 / 4) + 1024 = 7024 entries."""
    c, n_parts, shift, cap = 13, 4, 2, 7024
    W, B = 20, 4096
    lanes = M.partition_shapes(c, n_parts, shift, cap)
    plan = M.partition_plan(c, n_parts, cap)
    assert len(lanes) == len(plan) == 4
    sizes = []
    hit = set()
    for sc, want in zip(lanes, plan):
        digs = [M.recode(s, c) for s in sc]
        _, pop = M.sort_model([[d[w] for d in digs] for w in range(W)], W, len(sc), B)
        part = [sum(pop[b] for b in range(p, B, n_parts)) for p in range(n_parts)]
        assert part == [want.get(p, 0) for p in range(n_parts)]
        sizes += [n for n in part if n]
        hit |= {b for b, n in enumerate(pop) if n}
        assert any(x < 0 for d in digs for x in d)
    assert sorted(sizes) == sorted((cap, cap + 1) + M.PARTITION_SIZES) == [1, 1023, 1024, 1025, 4095, 4096, 4097, 7024, 7025]
    assert {0, B - 1} <= hit                                                   # the first and the last bucket
    assert {b & 3 for b in hit} == {0, 1, 2, 3} and any(b >> shift == 1023 for b in hit) and any(b >> shift == 0 and b & 3 == 3 for b in hit)
