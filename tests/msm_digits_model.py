"""Big-integer model of the MSM's signed-digit recoding and bucket sort (csrc/msm_sort.hip), and scalar families that sit on their edges
(TEST INFRASTRUCTURE ONLY).

tests/test_msm_digits.py runs the sort of one MSM call on the device (czk_lab_msm_sort, lab library) and holds every digit, every bucket and the
population order to this file.  tests/test_msm_digits_cpu.py proves, on this file alone, that the families contain what they claim.

The window geometry restates the definitions of csrc/czk_internal.h (msm_num_windows, msm_full_windows, msm_win_bit, msm_win_width).  The
recoding is defined by its invariants -- the signed sum of d_w 2^bit(w) is the scalar, -2^(cw-1) < d_w <= 2^(cw-1), no carry leaves the top
window -- which fix every digit: the digits of a window form a complete residue system modulo 2^cw.  The tie at half = 2^(cw-1) (positive, no
carry) is the product's current rule; a change of that rule changes `recode` in the same commit.

Families are built digits first: choose a digit vector, then `compose` the scalar that has it.  All arithmetic is on Python integers.
"""
from __future__ import annotations

import functools
import random

R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041
SCALAR_BITS = 254            # 253-bit scalars + the carry
CNT_BINS = 2048              # czk_internal.h: populations of CNT_BINS - 1 and more share the last bin of the population order
PSORT_THREADS = 1024         # k_part_sort: threads per partition, four entries per thread and iteration
WIDTHS = tuple(range(2, 23))
MIXED_WIDTHS = tuple(range(3, 15)) + (19,)   # the upper windows are one bit narrower


# ---- window geometry
def num_windows(c):
    return (SCALAR_BITS + c - 1) // c


def full_windows(c):
    """W_hi: windows [0, W_hi) are c bits wide, windows [W_hi, W) are c - 1 bits wide"""
    W = num_windows(c)
    top, slack = SCALAR_BITS - (W - 1) * c, W * c - SCALAR_BITS
    return W - slack if top < 10 and slack <= W else W


def win_bit(c, w):
    hi = full_windows(c)
    return w * c - (w - hi if w > hi else 0)


def win_width(c, w):
    return c if w < full_windows(c) else c - 1


@functools.lru_cache(maxsize=None)
def _layout(c):
    """(first bit, width) of every window"""
    return tuple((win_bit(c, w), win_width(c, w)) for w in range(num_windows(c)))


def half(c, w):
    return 1 << (_layout(c)[w][1] - 1)


# ---- recoding
def recode_carry(s, c):
    """(signed digits of s, the carry that leaves the top window)"""
    assert 0 <= s < (1 << 256)
    carry, out = 0, []
    for bit, cw in _layout(c):
        v = ((s >> bit) & ((1 << cw) - 1)) + carry
        if v > (1 << (cw - 1)):
            out.append(v - (1 << cw))
            carry = 1
        else:
            out.append(v)
            carry = 0
    return out, carry


def recode(s, c, inf_flags=None):
    """signed digits of the canonical scalar s, 0 where the base's flag for that window is set"""
    d, _ = recode_carry(s, c)
    return [0 if inf_flags is not None and inf_flags[w] else x for w, x in enumerate(d)]


def code(d):
    """the product's u32 encoding of a digit"""
    return 0 if d == 0 else abs(d) | ((1 << 31) if d < 0 else 0)


def compose(digits, c):
    """the scalar that has the digit vector `digits`"""
    assert len(digits) == num_windows(c)
    for w, d in enumerate(digits):
        assert -half(c, w) < d <= half(c, w), (c, w, d)
    s = sum(d << _layout(c)[w][0] for w, d in enumerate(digits))
    assert 0 <= s < R_MOD, (c, digits)
    return s


def sort_model(digits, W, nb, B):
    """digits[w][i]: the digits of one bucket set (W windows, nb points per window) -> ({bucket: the sorted list of its entries
    (w nb + i) | sign << 31} for the buckets that have any, the populations of all B buckets)"""
    buckets = {}
    assert len(digits) == W
    for w in range(W):
        for i, d in enumerate(digits[w]):
            if d:
                assert abs(d) <= B
                buckets.setdefault(abs(d) - 1, []).append((w * nb + i) | ((1 << 31) if d < 0 else 0))
    pop = [0] * B
    for b, v in buckets.items():
        v.sort()
        pop[b] = len(v)
    return buckets, pop


# ---- families
def _below_r(vals):
    seen, out = set(), []
    for v in vals:
        if 0 <= v < R_MOD and v not in seen:
            seen.add(v)
            out.append(v)
    return out


def _cut(c, vals):
    """the scalar with value vals[w] in window w, its top windows cleared until it is below r"""
    W = num_windows(c)
    vals = list(vals)
    top = W
    while True:
        s = sum(v << win_bit(c, w) for w, v in enumerate(vals))
        if s < R_MOD:
            return s
        top -= 1
        vals[top] = 0


def edge_values(c, w, reduced=False):
    cw = win_width(c, w)
    h, full = 1 << (cw - 1), (1 << cw) - 1
    return ([h, h + 1], [h - 1, full]) if reduced else ([0, 1, h - 1, h, h + 1, full - 1, full],) * 2


def window_edges(c):
    """every window with an edge value and zeros elsewhere; the same with all ones in every lower window, so that a carry arrives.  Widths with
    more than 40 windows (c < 7) keep two values per window and kind, to stay within the size limit."""
    W = num_windows(c)
    out = []
    for w in range(W):
        plain, carried = edge_values(c, w, reduced=W > 40)
        bit = win_bit(c, w)
        out += [v << bit for v in plain]
        out += [(v << bit) | ((1 << bit) - 1) for v in carried]
    return _below_r(out)


def carry_chains(c):
    W = num_windows(c)
    out = []
    for w in range(1, W):
        k = win_bit(c, w)
        out += [(1 << k) - 1, 1 << k, (1 << k) + 1]
    neg = [half(c, w) + 1 for w in range(W)]   # every digit negative, a carry through every window
    pos = [half(c, w) for w in range(W)]       # no carry, every entry in the last bucket of its width
    out.append(_cut(c, neg))
    out.append(_cut(c, neg[:1] + pos[1:]))     # the same with `half` above window 0: negative by the carry alone (at c = 2 the line above gives zeros under the carry)
    out.append(_cut(c, pos))
    out.append(_cut(c, [neg[w] if w % 2 == 0 else pos[w] for w in range(W)]))
    out.append(_cut(c, [pos[w] if w % 2 == 0 else neg[w] for w in range(W)]))
    # (a window of `half` that receives a carry turns negative.)  Digits that alternate in sign: half + 1, then half - 1 under its carry
    out.append(_cut(c, [neg[w] if w % 2 == 0 else pos[w] - 1 for w in range(W)]))
    out.append(_cut(c, [neg[w] if w % 2 == 1 else (pos[w] - 1 if w else pos[w]) for w in range(W)]))
    return _below_r(out)


def top_ones(c):
    """the largest scalar below r with all ones under the top window"""
    bit = win_bit(c, num_windows(c) - 1)
    t = R_MOD >> bit
    assert t >= 1
    s = (t << bit) | ((1 << bit) - 1)
    return s if s < R_MOD else s - (1 << bit)


def field_edges(c):
    return _below_r([0, 1, 2, R_MOD - 1, R_MOD - 2, (R_MOD - 1) // 2, (R_MOD + 1) // 2, 1 << 252, top_ones(c)])


def _all_digit(c, d, signs):
    """every window that can hold d holds +-d (signs: "+", "-" = negative under a positive highest digit, "+-" = alternating); the top
    windows are cleared until the scalar is below r"""
    W = num_windows(c)
    mags = [d if d <= half(c, w) else 0 for w in range(W)]
    for top in range(W, 0, -1):
        hi = max(w for w in range(top) if mags[w])
        dig = [0] * W
        for w in range(top):
            neg = w != hi and (signs == "-" or (signs == "+-" and w % 2 == 1)) and mags[w] < half(c, w)
            dig[w] = -mags[w] if neg else mags[w]
        if sum(x << win_bit(c, w) for w, x in enumerate(dig)) < R_MOD:
            return compose(dig, c)
    raise AssertionError((c, d))


def one_bucket_digits(c):
    """d = 1, one in the middle, the largest that fits every window, and 2^(c-1) (the last bucket: the full-width windows only)"""
    narrow = 1 << (min(win_width(c, w) for w in range(num_windows(c))) - 1)
    return sorted({1, max(1, narrow // 2 + narrow // 8), narrow, 1 << (c - 1)})


def one_bucket_scalars(c, d):
    return _below_r([_all_digit(c, d, sg) for sg in ("+", "-", "+-")])


def one_bucket(c):
    return [s for d in one_bucket_digits(c) for s in one_bucket_scalars(c, d)]


POPULATION_TARGETS = (CNT_BINS - 1, CNT_BINS, CNT_BINS - 2, 1, 2)   # (widths 2 and 3 have two buckets that fit every window: the first two)
POPULATION_SPLIT_SCALARS = CNT_BINS + 52


def _fill(c, n, plan):
    """plan: {window: [digit magnitudes, one per scalar from scalar 0 up]} -> n scalars.  Signs alternate, except that a scalar's highest
    digit is positive (and a magnitude equal to half stays positive)."""
    W = num_windows(c)
    out = []
    k = 0
    for i in range(n):
        dig = [0] * W
        seen_top = False
        for w in range(W - 1, -1, -1):
            m = plan.get(w, ())
            d = m[i] if i < len(m) else 0
            if d:
                k += 1
                dig[w] = -d if seen_top and k % 2 and d < half(c, w) else d
                seen_top = True
        out.append(compose(dig, c))
    return out


def population_buckets(c):
    """the buckets whose populations are fixed, in the order of POPULATION_TARGETS: digits that fit every window.  Widths below 5 have
    fewer than five such buckets and keep the first targets only."""
    narrow = 1 << (min(win_width(c, w) for w in range(num_windows(c))) - 1)
    want = [narrow - 1, 0, narrow // 2, 1, 2]
    out = []
    for b in want:
        if 0 <= b < narrow and b not in out:
            out.append(b)
    return out


def populations(c, W_table):
    """W_table windows share a bucket set (table form: all of them; table-free form: 1).  In the table form the buckets of
    population_buckets(c) hold exactly POPULATION_TARGETS entries of the one bucket set; in the table-free form the three large populations
    sit in the bucket sets of windows 0, 1 and 2 (a set holds one entry per scalar), the small ones in window 0's.  The top window stays empty."""
    W = num_windows(c)
    bk = population_buckets(c)
    tg = POPULATION_TARGETS[:len(bk)]
    if W_table > 1:
        usable = W - 1
        flat = [b + 1 for b, t in zip(bk, tg) for _ in range(t)]
        n = (len(flat) + usable - 1) // usable
        plan = {w: [] for w in range(usable)}
        for j, d in enumerate(flat):          # scalar j // usable, from its highest usable window down
            plan[usable - 1 - j % usable].append(d)
        return _fill(c, n, plan)
    n = POPULATION_SPLIT_SCALARS
    big = bk[0] + 1
    plan = {2: [big] * tg[2] if len(tg) > 2 else [], 1: [big] * tg[1], 0: [big] * tg[0]}
    for b, t in zip(bk[3:], tg[3:]):
        plan[0] = plan[0] + [b + 1] * t
    return _fill(c, n, plan)


PARTITION_SIZES = (1, PSORT_THREADS - 1, PSORT_THREADS, PSORT_THREADS + 1, 4 * PSORT_THREADS - 1, 4 * PSORT_THREADS, 4 * PSORT_THREADS + 1)
PARTITION_SCALARS = 600


def partition_plan(c, n_parts, cap, n=PARTITION_SCALARS):
    """lanes of {partition: entries}: one partition of cap and one of cap + 1 entries, and PARTITION_SIZES, packed into as few lanes of n scalars
    as hold them (the top window stays empty)"""
    budget = (num_windows(c) - 1) * n
    lanes = []
    for size in (cap, cap + 1) + PARTITION_SIZES:
        assert size <= budget, (size, budget)
        for ln in lanes:
            if len(ln) < n_parts and sum(ln.values()) + size <= budget:
                ln[len(ln)] = size
                break
        else:
            lanes.append({0: size})
    return lanes


def partition_shapes(c, n_parts, part_shift, cap, n=PARTITION_SCALARS):
    """One list of n scalars per lane of partition_plan.  Partition p is the set of buckets (idx << part_shift) | p; its entries cycle through
    the indices 0, the last one (1023 at c >= 11), the last that fits the narrower windows, and seeded random ones, so that bucket 0 and bucket
    B - 1 are hit in partitions 0 and n_parts - 1."""
    assert n_parts == 1 << part_shift
    W, B = num_windows(c), 1 << (c - 1)
    per = B // n_parts
    rng = random.Random(0x5047 + c)
    out = []
    for sizes in partition_plan(c, n_parts, cap, n):
        slots = [(w, i) for i in range(n) for w in range(W - 2, -1, -1)]   # a scalar's slots from its highest usable window down
        plan = {w: [0] * n for w in range(W - 1)}
        at = 0
        for p, size in sizes.items():
            for k in range(size):
                w, i = slots[at]
                at += 1
                lim = min(per, (half(c, w) - p + n_parts - 1) // n_parts)   # indices whose digit fits this window
                idx = (0, per - 1, lim - 1, rng.randrange(per), rng.randrange(per))[k % 5] % lim
                plan[w][i] = ((idx << part_shift) | p) + 1
        out.append(_fill(c, n, plan))
    return out


def families(c, W_table=None):
    """name -> scalars.  (partition_shapes is built from the layout the product reports: see above.)"""
    W_table = num_windows(c) if W_table is None else W_table
    return {"window_edges": window_edges(c), "carry_chains": carry_chains(c), "field_edges": field_edges(c), "one_bucket": one_bucket(c),
            "populations": populations(c, W_table)}


def edge_scalars(c):
    """what the width cases of the GPU tests feed the device"""
    return _below_r(window_edges(c) + carry_chains(c) + field_edges(c))


# width -> family -> size (populations: the table form; the table-free form has POPULATION_SPLIT_SCALARS)
FAMILY_SIZES = {
    2: {"window_edges": 503, "carry_chains": 384, "field_edges": 9, "one_bucket": 4, "populations": 33},
    3: {"window_edges": 336, "carry_chains": 259, "field_edges": 9, "one_bucket": 7, "populations": 49},
    4: {"window_edges": 252, "carry_chains": 196, "field_edges": 9, "one_bucket": 10, "populations": 98},
    5: {"window_edges": 200, "carry_chains": 157, "field_edges": 9, "one_bucket": 10, "populations": 123},
    6: {"window_edges": 168, "carry_chains": 133, "field_edges": 9, "one_bucket": 10, "populations": 147},
    7: {"window_edges": 429, "carry_chains": 115, "field_edges": 9, "one_bucket": 10, "populations": 171},
    8: {"window_edges": 369, "carry_chains": 100, "field_edges": 9, "one_bucket": 10, "populations": 199},
    9: {"window_edges": 333, "carry_chains": 91, "field_edges": 9, "one_bucket": 10, "populations": 220},
    10: {"window_edges": 297, "carry_chains": 82, "field_edges": 9, "one_bucket": 10, "populations": 246},
    11: {"window_edges": 273, "carry_chains": 76, "field_edges": 9, "one_bucket": 10, "populations": 268},
    12: {"window_edges": 249, "carry_chains": 70, "field_edges": 9, "one_bucket": 10, "populations": 293},
    13: {"window_edges": 225, "carry_chains": 64, "field_edges": 9, "one_bucket": 10, "populations": 324},
    14: {"window_edges": 213, "carry_chains": 61, "field_edges": 9, "one_bucket": 10, "populations": 342},
    15: {"window_edges": 189, "carry_chains": 55, "field_edges": 9, "one_bucket": 7, "populations": 384},
    16: {"window_edges": 177, "carry_chains": 52, "field_edges": 9, "one_bucket": 7, "populations": 410},
    17: {"window_edges": 165, "carry_chains": 49, "field_edges": 9, "one_bucket": 7, "populations": 439},
    18: {"window_edges": 164, "carry_chains": 49, "field_edges": 9, "one_bucket": 7, "populations": 439},
    19: {"window_edges": 153, "carry_chains": 46, "field_edges": 9, "one_bucket": 10, "populations": 473},
    20: {"window_edges": 141, "carry_chains": 43, "field_edges": 9, "one_bucket": 7, "populations": 512},
    21: {"window_edges": 140, "carry_chains": 43, "field_edges": 9, "one_bucket": 7, "populations": 512},
    22: {"window_edges": 129, "carry_chains": 40, "field_edges": 9, "one_bucket": 7, "populations": 559},
}
