"""The integer model of the NTT passes (tests/ntt_pass_model.py) held to the checkers, and the extreme input families of tests/test_ntt_pass.py vetted
limb for limb, without a GPU.

  * model vs oracle: the model composed over pass_plan(n) equals the C checker's transforms at 2^11 .. 2^14 (ragged in_len included) and the O(D^2)
    definition at 2^11; its post modes 3 and 4 equal what the witness-map calls compute from separate checker calls;
  * the families hold what their names say;
  * limb-exact capacity: the steps of a whole tile run on tests/lazy_model.py's Concrete backend (which raises where a 64-bit column, a 32-bit limb,
    a K r table or a quotient estimate would be outside its contract) on the extreme families, for canonical (W = 1) and scratch (W = 2) inputs --
    so the inputs the GPU test sends are inside the contracts by the reference alone, and the all-top family reaches exactly 256 r - 128;
  * the (B0, RB, KB) table the model runs is the one ntt_pass.hip instantiates, read from the source text.
"""
import os
import random
import re

import numpy as np
import pytest

import lazy_model as L
import ntt_pass_model as M
from lazy_model import FR, Concrete
from util import ints_to_limbs, limbs_to_ints

R = M.R
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "collaborative-zksnark_amd", "csrc")
KINDS = {"fft": 0, "ifft": 1, "coset_fft": 2, "coset_ifft": 3}


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------------------ model vs oracle
def test_constants_are_the_checkers(orc):
    import pyref
    assert M.R == pyref.R_MOD and M.GENERATOR == pyref.FR_GENERATOR and M.TWO_ADICITY == pyref.FR_TWO_ADICITY
    for n in (0, 1, 11, 14, 47):
        assert M.root_of_unity(n) == pyref.fr_root_of_unity(n)
        assert M.root_of_unity(n) * M.MONT % R == limbs_to_ints(orc.domain_constants(n)["group_gen"].reshape(1, 4))[0]


def test_pass_plan_definition():
    for n in range(48):
        plan = M.pass_plan(n)
        assert len(plan) == max(1, -(-n // 7)) and sum(k for k, _ in plan) == n and plan[-1][1] == 0
        ks = [k for k, _ in plan]
        assert max(ks) - min(ks) <= 1 and ks == sorted(ks, reverse=True) and max(ks) <= 7
        assert all(s == sum(ks[p + 1:]) for p, (_, s) in enumerate(plan))
    assert M.pass_plan(11) == [(6, 5), (5, 0)] and M.pass_plan(14) == [(7, 7), (7, 0)] and M.pass_plan(21) == [(7, 14), (7, 7), (7, 0)]
    assert [n for n in range(11, 22) if M.equal_groups(n)] == [12, 14, 15, 18, 21]


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", [11, 12, 13, 14])
def test_model_composed_over_the_plan_is_the_oracles_transform(orc, n, kind):
    D = 1 << n
    rng = random.Random(n * 16 + KINDS[kind])
    x = [rng.randrange(R) for _ in range(D)]
    for in_len in (D, D - 3) if n > 11 else (D, D - 3, D // 2 + 1, 1, 0):
        want = limbs_to_ints(orc.ntt_fr(ints_to_limbs(x, 4), n, KINDS[kind], in_len=in_len))
        tail = x[:in_len] + [M.DEADBEEF] * (D - in_len)          # what lies behind in_len is not read
        assert M.transform(tail, n, KINDS[kind], in_len=in_len) == want, in_len


@pytest.mark.parametrize("kind", list(KINDS))
def test_model_is_the_definition_at_2_11(kind):
    import pyref
    rng = random.Random(KINDS[kind])
    x = [rng.randrange(R) for _ in range(1 << 11)]
    assert M.transform(x, 11, KINDS[kind]) == pyref.dft(x, 11, inverse=kind in ("ifft", "coset_ifft"), coset=kind.startswith("coset"))


def test_fused_pass_is_the_two_passes_of_the_pair(orc):
    """ifft then coset_fft at 2^12 = 6 + 6: first inverse pass, the fused pass, last forward pass"""
    n, C = 12, 6
    rng = random.Random(12)
    x = [rng.randrange(R) for _ in range(1 << n)]
    v = M.run_pass(x, n, 6, 6, M.omega(n, True), first=True)
    v = M.run_fused(v, n, C)
    v = M.run_pass(v, n, 0, 6, M.omega(n), last=True)
    lim = ints_to_limbs(x, 4)
    assert v == limbs_to_ints(orc.ntt_fr(orc.ntt_fr(lim, n, 1), n, 2))


@pytest.mark.parametrize("n", [11, 12])
def test_post_modes_3_and_4_are_the_witness_map_forms(orc, n):
    """mode 3: witness_map_post_h's h = (coset_ifft(ab) - ifft(c)) / Z(g) -- the checker's witness_map_post computes it as coset_ifft((ab - coset_fft(ifft(c))) / Z(g));
    mode 4: witness_map_pre_masked's coset_fft(ifft(a)) + mask"""
    D = 1 << n
    rng = random.Random(n)
    ab, c, mask = ([rng.randrange(R) for _ in range(D)] for _ in range(3))
    (K0, s0), (K1, s1) = M.pass_plan(n)
    zinv = limbs_to_ints(orc.domain_constants(n)["vanishing_inv"].reshape(1, 4))[0] * pow(M.MONT, -1, R) % R   # the plain field element
    assert zinv * (pow(M.GENERATOR, D, R) - 1) % R == 1
    ifft_c = M.transform(c, n, 1)
    v = M.run_pass(ab, n, s0, K0, M.omega(n, True), first=True)
    h = M.run_pass(v, n, s1, K1, M.omega(n, True), last=True, post_mode=3, addend=ifft_c, c2=zinv)
    assert h == limbs_to_ints(orc.witness_map_post(ints_to_limbs(ab, 4), ints_to_limbs(c, 4), n))
    # mode 4
    ea, _ = orc.witness_map_pre(ints_to_limbs(ab, 4), ints_to_limbs(c, 4), n)
    want = limbs_to_ints(orc.fr_add(ea, ints_to_limbs(mask, 4)))
    v = M.run_pass(M.transform(ab, n, 1), n, s0, K0, M.omega(n), first=True, prescale=True)
    assert M.run_pass(v, n, s1, K1, M.omega(n), last=True, post_mode=4, addend=mask) == want


# ------------------------------------------------------------------------------------------------------------------------ codecs
def test_codecs_round_trip_and_refuse_what_a_format_excludes():
    rng = random.Random(3)
    vals = [0, 1, R - 1, R, 2 * R - 1] + [rng.randrange(2 * R) for _ in range(20)]
    for fmt in (1, 2):
        rows = M.encode(vals, fmt)
        assert rows.shape == (len(vals), M.words_per_elem(fmt)) and M.decode(rows, fmt) == vals and M.in_range(rows, vals, fmt)
    canon = [v for v in vals if v < R]
    assert M.decode(M.encode(canon, 0), 0) == canon
    with pytest.raises(AssertionError):
        M.encode([R], 0)
    with pytest.raises(AssertionError):
        M.encode([2 * R], 2)
    # format 1 is the 29-bit re-slicing of the same integer (lazy_model's digits)
    assert M.encode(vals, 1).tolist() == [FR.digits(v) for v in vals]
    # a row nobody wrote is outside every format
    for fmt in (0, 1, 2):
        s = np.full((1, M.words_per_elem(fmt)), M.SENTINEL_WORD, dtype=np.uint32)
        assert not M.in_range(s, M.decode(s, fmt), fmt)
    assert M.DEADBEEF >= R and M.decode(M.encode([M.DEADBEEF], 0, check=False), 0) == [M.DEADBEEF]


# ------------------------------------------------------------------------------------------------------------------------ families
@pytest.mark.parametrize("scratch", [False, True])
@pytest.mark.parametrize("K,s_lo,n", [(5, 4, 11), (6, 5, 11), (7, 4, 12), (7, 0, 11)])
def test_families_hold_what_their_names_say(K, s_lo, n, scratch):
    D, top = 1 << n, M.top_of(scratch)
    assert top == (2 * R - 1 if scratch else R - 1)
    fams = M.families(K, scratch)
    want = {"all_top", "all_0", "all_1", "random"} | {"impulse_" + w for w in ("0", "1", "half", "last")} | {"stage%d_%s" % (q, h) for q in range(K) for h in ("low", "high")}
    assert set(fams) == want | ({"all_r"} if scratch else set())
    built = {name: f(n, s_lo, K, 7, top) for name, f in fams.items()}
    for name, v in built.items():
        assert len(v) == D and all(0 <= x <= top for x in v), name
    assert set(built["all_top"]) == {top} and set(built["all_0"]) == {0} and set(built["all_1"]) == {1}
    if scratch:
        assert set(built["all_r"]) == {R}                                     # congruent to 0, stored as r
    for where, at in (("0", 0), ("1", 1), ("half", D // 2), ("last", D - 1)):
        v = built["impulse_" + where]
        assert v[at] == top and sum(1 for x in v if x) == 1
    for q in range(K):
        lo, hi = built["stage%d_low" % q], built["stage%d_high" % q]
        bit = 1 << (s_lo + q)
        for i in range(D):
            if not i & bit:                                                    # the pair that meets at stage s_lo + q of the transform: (i, i | bit)
                assert (lo[i], lo[i | bit]) == (top, 0) and (hi[i], hi[i | bit]) == (0, top)
        for q2 in range(K):                                                    # at every other stage of the pass a pair holds two equal values: its difference is 0 mod r
            if q2 != q:
                b2 = 1 << (s_lo + q2)
                assert all(lo[i] == lo[i | b2] for i in range(D) if not i & b2)
    assert built["random"] == fams["random"](n, s_lo, K, 7, top) != fams["random"](n, s_lo, K, 8, top)
    assert max(built["random"]) > top - (top >> 8) and (not scratch or any(x >= R for x in built["random"]))
    a, a2 = M.alias_pair(n, 5)
    assert all(x < R and y in (x, x + R) for x, y in zip(a, a2)) and D // 4 < sum(1 for x, y in zip(a, a2) if x != y) < 3 * D // 4
    assert M.prefix_lengths(n) == [0, 1, D // 2 + 1, D - 3, D]
    for in_len in M.prefix_lengths(n):
        v = M.prefix_input(n, in_len, D + 5, 9)
        assert len(v) == D + 5 and all(x < R for x in v[:in_len]) and set(v[in_len:]) == {M.DEADBEEF}


# ------------------------------------------------------------------------------------------------------------------------ the kernels' constants
def _instantiations(text, kernel):
    """[(K, B0, RB, KB expression)] of the step calls in the body of `kernel`, in order, grouped by K"""
    m = re.search(r"void " + kernel + r"\(.*?\n\}\n", text, flags=re.S)
    assert m, kernel
    return re.findall(r"(strided_step|final_step|final_step_keep)<(\d), (?:(\d), )?(\d), ([^,>]+)[,>]", m.group(0))


def test_the_models_step_table_is_what_the_kernels_instantiate():
    text = src("ntt_pass.hip")
    assert re.search(r"constexpr unsigned NTT2_LOGT = 4, NTT2_T = 16;", text)
    assert re.search(r"constexpr unsigned PROBE_NTT2_T = 16;", src(os.path.join("lab", "ntt_pass_probe.hip")))
    assert re.search(r"constexpr int W = LAZY_IN \? 2 : 1;", text) and len(re.findall(r"constexpr int W = NTT2_SCRATCH_2R \? 2 : 1;", text)) == 2
    want = {K: [(b0, rb, "%d * W" % kb) for b0, rb, kb in steps] for K, steps in M.STEPS.items()}
    for kernel, step in (("k_ntt2_strided", "strided_step"), ("k_ntt2_final", "final_step")):
        got = {}
        for fn, K, b0, rb, kb in _instantiations(text, kernel):
            assert fn == step
            got.setdefault(int(K), []).append((int(b0), int(rb), kb.strip()))
        assert got == want, kernel
    # the fused pass: the inverse half as k_ntt2_final (its last step keeps the outputs: final_step_keep<C, RB, KB>, B0 = 0), the forward half as
    # k_ntt2_strided on canonical inputs (W = 1, written out)
    inv, fwd = {}, {}
    for fn, K, b0, rb, kb in _instantiations(text, "k_ntt2_final_first"):
        if fn == "strided_step":
            fwd.setdefault(int(K), []).append((int(b0), int(rb), kb.strip()))
        else:
            inv.setdefault(int(K), []).append((int(b0) if fn == "final_step" else 0, int(rb), kb.strip()))
    assert inv == want and fwd == {K: [(b0, rb, str(kb)) for b0, rb, kb in steps] for K, steps in M.STEPS.items()}
    # and it is the table of the interval proof (tests/test_lazy_arith_cpu.py imports it from the model)
    import test_lazy_arith_cpu
    assert test_lazy_arith_cpu.NTT_CHAINS is M.NTT_CHAINS
    assert M.NTT_CHAINS == {7: [("radix8", 2), ("radix4", 16), ("radix4", 64)], 6: [("radix8", 2), ("radix8", 16)], 5: [("radix8", 2), ("radix4", 16)]}
    for K, steps in M.STEPS.items():                    # the steps tile the K row bits from the top down
        assert steps[0][0] + steps[0][1] == K and steps[-1][0] == 0 and all(a[0] == b[0] + b[1] for a, b in zip(steps, steps[1:]))


# ------------------------------------------------------------------------------------------------------------------------ limb-exact capacity
T = 16


def tw_u(w):
    """a twiddle as the tables hold it: w 2^261 mod r, nine normalised limbs"""
    return FR.digits(w * (1 << 261) % R)


class Tile:
    """One tile of a pass on the Concrete backend, at the smallest domain that is one tile: n = K + 4 (a strided pass with s_lo = 4: rows are the K
    stage bits, 16 columns; a last pass: 16 chunks of 2^K).  Group membership and twiddle indices follow strided_step / final_step."""

    def __init__(self, K, W, last, inverse=False):
        self.K, self.W, self.last, self.n = K, W, last, K + 4
        self.D = 1 << self.n
        self.s_lo = 0 if last else 4
        w = M.omega(self.n, inverse)
        self.w = w
        self.pw = {}
        self.max_out = 0

    def tw(self, s, j):
        """w_s^j, w_s = omega^(D >> (s + 1)), in table form"""
        key = (self.D >> (s + 1)) * j % self.D
        if key not in self.pw:
            self.pw[key] = tw_u(pow(self.w, key, R))
        return self.pw[key]

    def index(self, row, t):
        """global element index of (row or in-chunk index, column or chunk)"""
        if not self.last:
            return (row << self.s_lo) | t
        return (M.bitrev(t, 4) << self.K) | row          # chunk t of the only block: h = brev(chunk, hb), hb = n - C = 4

    def run(self, values, cols=range(T)):
        """values: 2^n integers.  Returns {output index: limbs} for the chosen columns (chunks)"""
        B, K = Concrete(FR), self.K
        out = {}
        for t in cols:
            x = {row: FR.digits(values[self.index(row, t)]) for row in range(1 << K)}
            for step, (b0, rb, kb) in enumerate(M.STEPS[K]):
                final = self.last and b0 == 0
                for ro in range(1 << (K - rb)):
                    below, above = ro & ((1 << b0) - 1), ro >> b0
                    r0 = (above << (b0 + rb)) | below
                    rows = [r0 | (k << b0) for k in range(1 << rb)]
                    g = [x[r] for r in rows]
                    col = 0 if self.last else t              # last pass: twiddle index = in-chunk index below the stage bit
                    idx = lambda k: ((below | (k << b0)) << self.s_lo) | col   # noqa: E731
                    s = self.s_lo + b0
                    if final and rb == 3:
                        L.radix8_last(B, kb * self.W, g, L.Tws([None] + [self.tw(2, k) for k in (1, 2, 3)] + [self.tw(1, 1)]))
                    elif final:
                        L.radix4_last(B, kb * self.W, g, L.Tws([self.tw(1, 1)]))
                    elif rb == 3:
                        L.radix8(B, kb * self.W, g, L.Tws([self.tw(s + 2, idx(k)) for k in range(4)] + [self.tw(s + 1, idx(k)) for k in range(2)] + [self.tw(s, idx(0))]))
                    else:
                        L.radix4(B, kb * self.W, g, L.Tws([self.tw(s + 1, idx(k)) for k in range(2)] + [self.tw(s, idx(0))]))
                    for r, v in zip(rows, g):
                        x[r] = v
                # what goes through LDS to the next step is normalised
                assert all(max(v) <= FR.mask for v in x.values()), (step, t)
            for row, v in x.items():
                i = self.index(row, t)
                out[M.bitrev(i, self.n) if self.last else i] = v
        return out


def extreme_families(K, W):
    fams = M.families(K, scratch=W == 2)
    names = ["all_top", "random"] + ["stage%d_%s" % (q, h) for q in range(K) for h in ("low", "high")] + (["all_r"] if W == 2 else [])
    return {nm: fams[nm] for nm in names}


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("W", [1, 2])
@pytest.mark.parametrize("K", [5, 6, 7])
def test_extreme_families_stay_inside_every_limb_contract(K, W, last):
    """No ContractError anywhere in the tile (columns, limbs, K r tables, fru_mul's operand, the quotient estimate of fru_reduce_2r / fru_canon), and
    fru_canon of every tile output is the value model's.  The all-top family runs the whole tile; the others two columns of it (columns differ in
    their twiddles alone).  A last pass with W = 1 is scratch format 0."""
    tile = Tile(K, W, last)
    n, top = tile.n, M.top_of(W == 2)
    size_inv = tw_u(pow(tile.D, -1, R))
    B = Concrete(FR)
    for name, f in extreme_families(K, W).items():
        values = f(n, tile.s_lo, K, 11, top)
        cols = range(T) if name == "all_top" else (0, 13)
        out = tile.run(values, cols)
        want = M.run_pass(values, n, tile.s_lo, K, tile.w, last=last)
        assert len(out) == len(cols) << K
        for i, limbs in out.items():
            assert L.fru_canon(limbs) == want[i], (name, i)            # also runs fru_reduce_2r's quotient check
            if last:                                                     # post modes 1 .. 3 multiply the lazy value instead
                assert FR.value(B.mul(limbs, size_inv)) < 2 * R
        biggest = max(FR.value(v) for v in out.values())
        if name == "all_top" and not last:
            # 2^K sums of top: what store_output hands fru_reduce_2r
            assert biggest == (1 << K) * top and FR.value(out[0]) == biggest
            if (K, W) == (7, 2):
                assert biggest == 256 * R - 128
        assert biggest < 1 << 261


def test_the_families_reach_the_last_pass_bound():
    """radix4_last at KB = 128 (K = 7, scratch inputs < 2 r) documents x1 = s02 - x1 + 2 KB r < 384.2 r.  stage0_low puts 2 r - 1 on the minuend's side of
    every stage-0 pair and 0 on the other, so s02 is 128 (2 r - 1) and the concrete run stands at 384 r: the families reach the edge the comment budgets,
    and nothing exceeds it"""
    tile = Tile(7, 2, True)
    top = M.top_of(True)
    worst = {}
    for name, f in M.families(7, True).items():
        out = tile.run(f(tile.n, 0, 7, 1, top), cols=(0,))
        worst[name] = max(FR.value(v) for v in out.values())
    assert 384 * R - 256 <= worst["stage0_low"] < 384 * R + R // 5
    assert max(worst.values()) == worst["stage0_low"]
