"""Integer model of the MSM's bucket accumulation and bucket reduction (csrc/msm_acc.h, the second half of csrc/msm.hip), and the builders of
the entry lists tests/test_msm_buckets.py feeds to czk_lab_msm_buckets.  TEST INFRASTRUCTURE ONLY: Python integers throughout.

Model of values.  A key's bases are k_i G with known k_i, so a table entry (window w, base i) is the exponent k_i 2^bit(w) mod r, a bucket the
sum of its entries' exponents, and a lane result sum_b (b + 1) bucket_b (ExpGroup).  Keys that hold points of even order have no exponent: their
entries are affine points under the group law of tests/pairing_ref.py (PointGroup).

Model of the control flow, in entry order (k_accumulate_u / k_accumulate_u2): the first entry is taken over; an entry equal to +- the
accumulator is an exceptional addition and is deferred (the accumulator stays); past EXC_CAP deferred points in all a bucket goes dirty and
stops; only the first HEAVY_CHUNK entries are folded there, the rest in work items of HEAVY_SUB entries (complete formulas: nothing deferred),
whose partial sums k_heavy_combine adds in a strided loop and a tree (combine_trace).  The twisted Edwards kernels add with unified formulas:
no exceptional additions, no flags.

Entry codes are (w * nb + i) | sign << 31, as the sort writes them."""
import random

import msm_digits_model as D
import pairing_ref as PR

R_MOD = D.R_MOD
HEAVY_CHUNK, HEAVY_SUB = 1024, 256     # msm_acc.h
EXC_CAP = 4096                         # msm_acc_g1.hip G1_EXC_CAP, msm_acc_g2.hip G2_EXC_CAP
TAIL_MAX, MSM_L = 1024, 8              # msm_acc.h, czk_internal.h
COMBINE_THREADS = 128                  # k_heavy_combine: one block per over-full bucket
NEG = 1 << 31
FAM_TE, FAM_U = 0, 1                   # the probe's `family`


class ExpGroup:
    """Elements of the prime-order subgroup as exponents of the generator."""
    zero = 0

    @staticmethod
    def add(a, b):
        return (a + b) % R_MOD

    @staticmethod
    def neg(a):
        return (-a) % R_MOD

    @staticmethod
    def mul(k, a):
        return k * a % R_MOD


class PointGroup:
    """Affine points of E(Fq) (any order), None = infinity."""
    zero = PR.INF

    @staticmethod
    def add(a, b):
        return PR.ec_add(PR.F1, a, b)

    @staticmethod
    def neg(a):
        return PR.ec_neg(PR.F1, a)

    @staticmethod
    def mul(k, a):
        return PR.ec_mul(PR.F1, k, a)


def table_exponents(ks, c, W):
    """Exponents of the window table of a key with bases k_i G: entry w * nb + i = k_i 2^bit(w) (c = 0: a table-free key, window 0 only)."""
    if c == 0:
        assert W == 1
        return [k % R_MOD for k in ks]
    assert W == D.num_windows(c)
    return [(k << D.win_bit(c, w)) % R_MOD for w in range(W) for k in ks]


def value(G, vals, code):
    v = vals[code & (NEG - 1)]
    return G.neg(v) if code & NEG else v


def combine_trace(G, partials):
    """k_heavy_combine on the partial sums of one bucket's work items: (sum, additions of equal operands, additions of opposite operands)."""
    n, dbl, opp = len(partials), 0, 0

    def add(a, b):
        nonlocal dbl, opp
        if a != G.zero and b != G.zero:
            dbl += a == b
            opp += a == G.neg(b)
        return G.add(a, b)
    v = [G.zero] * COMBINE_THREADS
    for tid in range(min(COMBINE_THREADS, n)):
        for j in range(tid, n, COMBINE_THREADS):
            v[tid] = add(v[tid], partials[j])
    live, stride = min(n, COMBINE_THREADS), COMBINE_THREADS // 2
    while stride:
        for tid in range(stride):
            if tid + stride < live:
                v[tid] = add(v[tid], v[tid + stride])
        stride //= 2
    return v[0], dbl, opp


def bucket_trace(G, vals, codes):
    """One bucket in entry order: its value, the exceptional additions of the main kernel (first HEAVY_CHUNK entries), the work items, the partial
    sums' tree statistics and the equal / opposite additions of the final bucket + partials step."""
    acc, started, exc = G.zero, False, 0
    for code in codes[:HEAVY_CHUNK]:
        q = value(G, vals, code)
        if not started:
            acc, started = q, True
        elif q == acc or q == G.neg(acc):
            exc += 1
        else:
            acc = G.add(acc, q)
    partials = []
    for first in range(HEAVY_CHUNK, len(codes), HEAVY_SUB):
        p = G.zero
        for code in codes[first:first + HEAVY_SUB]:
            p = G.add(p, value(G, vals, code))
        partials.append(p)
    total = G.zero
    for code in codes:
        total = G.add(total, value(G, vals, code))
    tree, dbl, opp = combine_trace(G, partials) if partials else (G.zero, 0, 0)
    main = G.zero
    for code in codes[:HEAVY_CHUNK]:
        main = G.add(main, value(G, vals, code))
    assert G.add(main, tree) == total
    last = ("equal" if main == tree else "opposite" if main == G.neg(tree) else "") if partials and main != G.zero and tree != G.zero else ""
    return {"value": total, "exc": exc, "items": len(partials), "partials": partials, "tree_equal": dbl, "tree_opposite": opp, "last": last, "main": main}


def expect(G, vals, case, family):
    """What the probe must return for `case` (a list of {bucket: [codes]} per lane; case B): bucket values, lane results, counters.  exc_count and
    dirty are exact when the exception list does not overflow or when no bucket has more than one exceptional addition (which bucket meets the
    full list is the schedule's choice otherwise: `exact` False, and the figures are lower bounds)."""
    B, lanes = case["B"], case["lanes"]
    buckets, results, exc, items, heavy, most = [], [], 0, 0, 0, 0
    for lane in lanes:
        vb, res = {}, G.zero
        for b, codes in lane.items():
            assert 0 <= b < B and codes
            t = bucket_trace(G, vals, codes)
            vb[b] = t["value"]
            res = G.add(res, G.mul(b + 1, t["value"]))
            exc += t["exc"]
            most = max(most, t["exc"])
            items += t["items"]
            heavy += t["items"] > 0
        buckets.append(vb)
        results.append(res)
    out = {"buckets": buckets, "results": results, "items": items, "heavy": heavy}
    if family == FAM_TE:
        out.update(exc_count=0, dirty=0, exact=True)
    elif exc <= EXC_CAP or most <= 1:
        out.update(exc_count=exc, dirty=max(0, exc - EXC_CAP), exact=True)
    else:
        out.update(exc_count=EXC_CAP + 1, dirty=1, exact=False)
    return out


def layout(case, seed=1):
    """The probe's arrays for a case: (sorted (lanes x total), offsets, counts, perm (lanes x B)) as lists.  Segments lie in a shuffled bucket order; perm is a descending-population order whose ties are broken differently in every lane."""
    rng = random.Random(seed)
    B, lanes = case["B"], case["lanes"]
    total = max(1, max(sum(len(c) for c in lane.values()) for lane in lanes))
    srt, offs, cnts, perms = [], [], [], []
    for lane in lanes:
        s, off, cnt = [0] * total, [0] * B, [0] * B
        order = list(lane)
        rng.shuffle(order)
        pos = 0
        for b in order:
            off[b], cnt[b] = pos, len(lane[b])
            s[pos:pos + cnt[b]] = lane[b]
            pos += cnt[b]
        for b in range(B):
            if not cnt[b]:
                off[b] = rng.randrange(total)     # an empty bucket's offset is never read through: any value in range
        perm = list(range(B))
        rng.shuffle(perm)
        perm.sort(key=lambda b: -cnt[b])
        srt.append(s), offs.append(off), cnts.append(cnt), perms.append(perm)
    return srt, offs, cnts, perms


# ------------------------------------------------------------------------------------------------ keys
N_BASES = 512
REL_SUM = (500, 0, 1)      # ks[500] = ks[0] + ks[1]
REL_SUM2 = (501, 2, 3)     # ks[501] = ks[2] + ks[3]
REL_8X = (502, 4)          # ks[502] = 8 ks[4]


def key_exponents(seed):
    """The k_i of a 512-base key: random, with the three relations the builders use."""
    rng = random.Random(seed)
    ks = [rng.randrange(1, R_MOD) for _ in range(N_BASES)]
    ks[500] = (ks[0] + ks[1]) % R_MOD
    ks[501] = (ks[2] + ks[3]) % R_MOD
    ks[502] = 8 * ks[4] % R_MOD
    return ks


class Key:
    """What the builders know of a key: nb points per window, W windows, and the table's values (exponents or points)."""

    def __init__(self, G, vals, nb, W):
        self.G, self.vals, self.nb, self.W = G, vals, nb, W

    def code(self, i, w=0, neg=False):
        assert 0 <= i < self.nb and 0 <= w < self.W
        return (w * self.nb + i) | (NEG if neg else 0)


def case(B, *lanes):
    return {"B": B, "lanes": [dict(l) for l in lanes]}


def distinct_run(key, rng, n, start=None, avoid=()):
    """n entries drawn from the table so that no addition of the run is exceptional (no entry equals +- the sum so far, and no partial sum is
    the neutral element); with `start` the run continues an accumulator of that value.  Index range: the whole table except `avoid`."""
    G, out, acc = key.G, [], start
    while len(out) < n:
        idx = rng.randrange(key.nb * key.W)
        if idx % key.nb in avoid:
            continue
        code = idx | (NEG if rng.getrandbits(1) else 0)
        q = value(G, key.vals, code)
        if acc is None:
            acc = q
        elif q == acc or q == G.neg(acc) or G.add(acc, q) == G.zero:
            continue
        else:
            acc = G.add(acc, q)
        out.append(code)
    return out


def filler(key, rng, B, skip, n_buckets=20, longest=6):
    """A few short ordinary buckets around the aimed one, so that a case never runs on an otherwise empty bucket set."""
    out = {}
    for b in rng.sample([b for b in range(B) if b not in skip], n_buckets):
        out[b] = distinct_run(key, rng, rng.randrange(1, longest + 1))
    return out


# ------------------------------------------------------------------------------------------------ case builders
def short_chains(key, B=128):
    """First entry and short chains.  Bucket -> (entries, exceptional additions): see CHAINS."""
    P, Q, w1 = 7, 9, min(1, key.W - 1)
    s, a, b = REL_SUM
    c = key.code
    lane = {
        0: [c(P)], 1: [c(P, neg=True)], 2: [c(P), c(P)], 3: [c(P), c(P, neg=True)], 4: [c(P), c(P), c(P)], 5: [c(P), c(P, neg=True), c(Q)],
        6: [c(a), c(b), c(s, neg=True)], 7: [c(b), c(s, neg=True), c(a)], 8: [c(s, neg=True), c(a), c(b)],
        B - 1: [c(P, w1, neg=True), c(P, w1, neg=True)], 64: [c(Q, w1, neg=True)], 65: [c(P, neg=True), c(P)],
    }
    return case(B, lane)


CHAINS = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 1, 6: 1, 7: 1, 8: 1, -1: 1, 64: 0, 65: 1}   # bucket (-1: B - 1) -> exceptional additions
CHAINS_NEUTRAL = (3, 6, 7, 8, 65)                                                        # buckets of short_chains whose sum is the neutral element
EDGE_COUNTS = (1023, 1024, 1025, 1279, 1280, 1281, HEAVY_CHUNK + COMBINE_THREADS * HEAVY_SUB, HEAVY_CHUNK + COMBINE_THREADS * HEAVY_SUB + 1)


def chunk_edge(key, cnt, B=128, bucket=37, seed=11):
    """One bucket of `cnt` entries with distinct sums (no exceptional addition anywhere in entry order), a few ordinary buckets around it."""
    rng = random.Random(seed * 100003 + cnt)
    lane = filler(key, rng, B, {bucket})
    lane[bucket] = distinct_run(key, rng, cnt)
    return case(B, lane)


def zero_blocks(key, rng, n):
    """n entries that sum to the neutral element and, behind an accumulator X that is none of their partial sums, cause no exceptional addition:
    pairs (Y, -Y), and one triple (P2, P3, -(P2 + P3)) when n is odd."""
    out = []
    if n % 2:
        s, a, b = REL_SUM2
        out += [key.code(a), key.code(b), key.code(s, neg=True)]
    while len(out) < n:
        i = rng.randrange(10, 400)
        w = rng.randrange(key.W)
        out += [key.code(i, w), key.code(i, w, neg=True)]
    return out


def exceptional_at(key, pos, B=128, bucket=5, seed=12):
    """The accumulator's own value X as entry `pos` (1-based): X, then pos - 2 entries that sum to zero, then X again."""
    rng = random.Random(seed * 7919 + pos)
    X = key.code(450)
    lane = filler(key, rng, B, {bucket})
    lane[bucket] = [X] + zero_blocks(key, rng, pos - 2) + [X]
    assert len(lane[bucket]) == pos
    return case(B, lane)


def equal_opposite_partials(key, B=128, seed=13):
    """Over-full buckets whose work items repeat or negate one another: bucket 10: items (L, L), the tree doubles; 11: (L, L, -L), the tree cancels
    items 0 and 2 and adds item 1 to the neutral element; 12: (L, M, L, M), two doublings and an addition; 13: main chunk S, items -S: the bucket
    cancels to the neutral element in the last addition."""
    rng = random.Random(seed)
    L = distinct_run(key, rng, HEAVY_SUB)
    M = distinct_run(key, rng, HEAVY_SUB)
    neg = [c ^ NEG for c in L]
    S = distinct_run(key, rng, HEAVY_CHUNK)
    lane = filler(key, rng, B, {10, 11, 12, 13})
    lane[10] = distinct_run(key, rng, HEAVY_CHUNK) + L + L
    lane[11] = distinct_run(key, rng, HEAVY_CHUNK) + L + L + neg
    lane[12] = distinct_run(key, rng, HEAVY_CHUNK) + L + M + L + M
    lane[13] = S + [c ^ NEG for c in S]
    return case(B, lane)


CAP_COUNTS = (EXC_CAP - 1, EXC_CAP, EXC_CAP + 1, 6000)


def exception_cap(key, n_buckets, B=2048, lanes=3):
    """n_buckets buckets over 3 lanes of 2 048 hold (P_b, P_b): one exceptional addition each."""
    assert n_buckets <= B * lanes
    out = [{} for _ in range(lanes)]
    for k in range(n_buckets):
        code = key.code(k % 400, (k // 400) % key.W, neg=bool(k & 1))
        out[k % lanes][(k // lanes * 5 + 3) % B] = [code, code]      # (5 is odd: a permutation of the buckets)
    return case(B, *out)


def overfull_same_point(key, n_buckets, copies=HEAVY_CHUNK + 300, B=128):
    """n_buckets buckets of `copies` copies of one point each: HEAVY_CHUNK - 1 exceptional additions per bucket, then work items of copies."""
    return case(B, {3 + 17 * k: [key.code(20 + k, neg=bool(k & 1))] * copies for k in range(n_buckets)})


def lanes_random(key, lanes, B=128, seed=14):
    """Different ordinary content in every lane: about half of the buckets, up to 40 entries, and one bucket of 300."""
    rng = random.Random(seed * 31 + lanes)
    out = []
    for ln in range(lanes):
        lane = {b: distinct_run(key, rng, rng.randrange(1, 41)) for b in rng.sample(range(B), B // 2)}
        lane[(ln * 29 + 1) % B] = distinct_run(key, rng, 300)
        out.append(lane)
    return case(B, *out)


# the aimed buckets of tests/test_msm_reduce_lean.py (B = 2 048: 256 chunks of 8)
AIMED = {
    "first entry of a chunk (no A addition)": [800],
    "last entry of a chunk (running starts here)": [807],
    "bucket 0": [0],
    "bucket B - 1": [2047],
    "only the last entry of a chunk": [1039],
    "only the first entry of a chunk": [1032],
    "first and last entry of one chunk": [1200, 1207],
    "a full chunk and its neighbours' edges": list(range(1599, 1609)),
    "the last chunk": list(range(2040, 2048)),
    "the first chunk": list(range(0, 8)),
}


def singles(key, buckets, B, lanes=2, neg_lane=True):
    """One entry per named bucket: lane 0 positive, lane 1 the negated entries."""
    return case(B, *[{b: [key.code(30 + j % 300, neg=bool(ln) and neg_lane)] for j, b in enumerate(buckets)} for ln in range(lanes)])


def reduce_shapes(key, B, seed=15):
    """Ordinary buckets for the reduction at B = 128 (tail only), 1 024 (the tail at its limit), 2 048 (one level), 16 384 (two levels, E_in): lane 0
    every fifth bucket and the ends, lane 1 sparse."""
    rng = random.Random(seed + B)
    dense = {b: distinct_run(key, rng, rng.randrange(1, 4)) for b in set(range(0, B, 5)) | {0, 1, B - 2, B - 1}}
    sparse = {b: distinct_run(key, rng, 1) for b in rng.sample(range(B), 9)}
    return case(B, dense, sparse)


def neighbours(key, B, opposite):
    """Pairs of neighbouring buckets that hold the same point, or a point and its negative (a running sum then passes through the neutral element
    inside a chunk), at the start, the middle and the end of chunks, across a chunk edge and at both ends of the bucket set."""
    lane = {}
    for j, b in enumerate((0, 3, 6, 15, B // 2 + 1, B - 2)):
        lane[b] = [key.code(40 + j)]
        lane[b + 1] = [key.code(40 + j, neg=opposite)]
    return case(B, lane)


def all_same(key, B):
    """Every bucket the same point: every addition of a tree level meets equal operands."""
    return case(B, {b: [key.code(60)] for b in range(B)}, {b: [key.code(61, neg=True)] for b in range(B)})


def level_cancel(key, B=16384, M=37):
    """A chunk of the SECOND level whose A and E cancel (B = 16 384; chunk M covers buckets 64 M .. 64 M + 63): P = k_4 G alone in the first bucket of
    the chunk's second level-0 chunk contributes 8 P to A; -8 P = -(k_502 G) in the second bucket of its first level-0 chunk contributes -8 P to
    E and nothing to A."""
    i8, i1 = REL_8X
    return case(B, {64 * M + 8: [key.code(i1)], 64 * M + 1: [key.code(i8, neg=True)], 5: [key.code(70)], B - 9: [key.code(71)]})


def neutral(B, lanes=2):
    return case(B, *[{} for _ in range(lanes)])


def torsion(arrangement, B):
    """Even-order points (a key whose bases 0 and 1 are the points of order two T0, T1 and whose bases 2.. have odd order): T alone in buckets
    2, 64 and B - 1; T twice; T beside one odd-order point.  Codes are window 0 only (the higher windows of T are the neutral element)."""
    if arrangement == "alone":
        return case(B, {2: [0], 64: [1 | NEG], B - 1: [0]}, {2: [1], B - 1: [1]})
    if arrangement == "twice":
        return case(B, {2: [0, 0], 64: [1, 1 | NEG], B - 1: [0, 0], 9: [2]})
    assert arrangement == "beside"
    return case(B, {2: [0, 2], 64: [3, 1], B - 1: [0, 4 | NEG], 70: [0, 1]}, {5: [2, 0, 3]})
