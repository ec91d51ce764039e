"""The NTT on the device, ONE PASS at a time, against the integer model of tests/ntt_pass_model.py.

czk_lab_ntt_pass (csrc/lab/ntt_pass_probe.hip, lab library only) launches exactly one launch_ntt2_pass -- or the fused launch_ntt2_final_first -- on a
buffer written here, with the domain's own tables, at any legal (log_d, s_lo, K), and returns the whole output buffer: every lane, pre-filled with a
sentinel, and a guard tail behind the last lane.  Every case compares EVERY element of every lane with the model, and the guard with the sentinel:

  * scratch outputs are decoded with the codec of the format the probe reports; they must lie in the format's range (< 2 r for formats 1 and 2, < r
    for format 0 -- a sentinel row lies outside both) and be congruent mod r to the model.  The raw scratch words are NOT pinned: they are internal;
  * canonical outputs (last passes) equal the model word for word.

What a product run cannot reach and these inputs do: scratch lanes that hold 2 r - 1 everywhere (the bound analysis' edge: 2 -> 16 -> 64 -> 256 r),
r where the residue is 0, alternations that make every difference of a stage an exact multiple of r, aliases a / a + r of one vector, outputs that
are 0 by construction (post modes 3 and 4 with the addend that cancels the transform), and the instantiations that first appear at 2^17 and 2^20
(k_ntt2_strided<6, true>, <7, true>) at 2^11.  tests/test_ntt_pass_cpu.py proves on the limb-exact model that these inputs are inside every contract.

The last section runs structured inputs through the product library (czk_ntt_fr, czk_ntt_fr_mixed, the witness-map calls) against the checker.

Last passes run at log_d = 11 (the smallest domain with second-generation tables; for C = 7 that is C + 4, one block) and at C + 6 (C + 8 for C = 5,
where C + 6 = 11 again).

Measured on one MI355X: the 101 cases of this file in about 25 s; the slowest (czk_ntt_fr on structured inputs at 2^14, then the last passes with C = 7
at 2^13) 0.4 s -- nearly all of it the Python model."""
import ctypes as C
import random

import numpy as np
import pytest

import ntt_pass_model as M
from util import ints_to_limbs

pytestmark = pytest.mark.gpu

R = M.R
LANES = 3


@pytest.fixture(scope="module")
def czk():
    import czk_amd
    return czk_amd


@pytest.fixture(scope="module")
def lab(czk):
    c = czk.Context(0, lab=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fmt(lab):
    d = lab.lab_ntt_pass(11, dims_only=True)
    assert d["format"] in (0, 1, 2) and d["elem_bytes"] == 4 * M.words_per_elem(d["format"]) and d["min_log"] == 11 and d["T"] == 16 and d["guard"] >= 16
    return d["format"]


# ------------------------------------------------------------------------------------------------------------------------ comparison
def check_guard(out, n_rows, tag):
    guard = out[n_rows:]
    assert guard.shape[0] >= 16 and (guard == M.SENTINEL_WORD).all(), (tag, "guard tail written", np.flatnonzero((guard != M.SENTINEL_WORD).any(axis=1))[:8].tolist())


def check_scratch(out, fmt, want_lanes, tag):
    """out: the probe's whole buffer; want_lanes: the model's integers per lane.  Returns the decoded integers per lane."""
    D = len(want_lanes[0])
    n_rows = len(want_lanes) * D
    rows = out[:n_rows]
    unwritten = np.flatnonzero((rows == M.SENTINEL_WORD).all(axis=1))
    assert unwritten.size == 0, (tag, "elements never written (lane * D + index)", unwritten[:8].tolist())
    got = M.decode(rows, fmt)
    bound = R if fmt == 0 else 2 * R
    bad = [i for i, v in enumerate(got) if v >= bound]
    assert not bad and M.in_range(rows, got, fmt), (tag, "outside the scratch format's range", bad[:8])
    lanes = [got[ln * D:(ln + 1) * D] for ln in range(len(want_lanes))]
    for ln, (g, w) in enumerate(zip(lanes, want_lanes)):
        bad = [i for i in range(D) if (g[i] - w[i]) % R]
        assert not bad, (tag, "lane", ln, "elements not congruent to the model", bad[:8], len(bad))
    check_guard(out, n_rows, tag)
    return lanes


def check_canonical(out, want_lanes, tag):
    D = len(want_lanes[0])
    n_rows = len(want_lanes) * D
    want = M.encode([v for lane in want_lanes for v in lane], 0)
    bad = np.flatnonzero((out[:n_rows] != want).any(axis=1))
    assert bad.size == 0, (tag, "canonical outputs differ from the model (lane * D + index)", bad[:8].tolist(), int(bad.size))
    check_guard(out, n_rows, tag)


def lane_groups(names, size=LANES):
    """the family names in groups of `size`, the last one filled up with its own first"""
    gs = [names[i:i + size] for i in range(0, len(names), size)]
    gs[-1] = gs[-1] + gs[-1][:1] * (size - len(gs[-1]))
    return gs


def scratch_inputs(n, s_lo, K, seed):
    """[(tag, [lane values])] over every scratch family, three lanes a launch; the alias pair rides with a random lane"""
    fams, top = M.families(K, True), M.top_of(True)
    out = [("+".join(g), [fams[nm](n, s_lo, K, seed + i, top) for i, nm in enumerate(g)]) for g in lane_groups(list(fams))]
    a, a2 = M.alias_pair(n, seed)
    out.append(("alias", [a, a2, fams["random"](n, s_lo, K, seed + 9, top)]))
    return out


def stack(lanes, fmt, check=True):
    return np.concatenate([M.encode(v, fmt, check=check) for v in lanes])


# ------------------------------------------------------------------------------------------------------------------------ plans
def test_pass_plans_are_the_models(lab):
    for n in range(48):
        d = lab.lab_ntt_pass(n, dims_only=True)
        assert list(zip(d["K"], d["s_lo"])) == M.pass_plan(n) and d["m"] == len(M.pass_plan(n)) and d["equal_groups"] == M.equal_groups(n), n


# ------------------------------------------------------------------------------------------------------------------------ first passes
# per K: the domain that is one tile row (s_lo + K = log_d = 11) and one with several (s_lo + K < log_d)
FIRST_SHAPES = [(K, n, s_lo) for K in (5, 6, 7) for n, s_lo in ((11, 11 - K), (12, 4))]


@pytest.mark.parametrize("prescale", [False, True])
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K,n,s_lo", FIRST_SHAPES)
def test_first_pass(lab, fmt, K, n, s_lo, inverse, prescale):
    """k_ntt2_strided<K, false>: canonical lanes at a stride that is not D, every canonical family, every prefix length with a tail that must not be read"""
    D, top, w = 1 << n, M.top_of(False), M.omega(n, inverse)
    fams = M.families(K, False)
    run = lambda data, in_len, stride: lab.lab_ntt_pass(n, K, s_lo, data, inverse=inverse, first=True, lanes=LANES, in_len=in_len,  # noqa: E731
                                                         in_lane_stride=stride, prescale=prescale)["out"]
    stride = D + 5
    for g in lane_groups(list(fams)):
        lanes = [fams[nm](n, s_lo, K, 3 + i, top) for i, nm in enumerate(g)]
        out = run(stack([v + [M.DEADBEEF] * (stride - D) for v in lanes], 0, check=False), D, stride)
        check_scratch(out, fmt, [M.run_pass(v, n, s_lo, K, w, first=True, prescale=prescale) for v in lanes], ("first", K, n, s_lo, inverse, prescale, g))
    for in_len in M.prefix_lengths(n):
        stride = in_len + (5 if in_len + 3 == D else 3)
        lanes = [M.prefix_input(n, in_len, stride, 20 + ln) for ln in range(LANES)]
        out = run(stack(lanes, 0, check=False), in_len, stride)
        want = [M.run_pass(v, n, s_lo, K, w, first=True, in_len=in_len, prescale=prescale) for v in lanes]
        assert in_len or not any(any(x) for x in want)
        check_scratch(out, fmt, want, ("first, prefix", K, n, s_lo, inverse, prescale, in_len))


# ------------------------------------------------------------------------------------------------------------------------ middle passes
MIDDLE_SHAPES = [(K, n, s_lo) for K in (5, 6, 7) for n, s_lo in ((11, 4), (12, 12 - K), (13, 5))]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("K,n,s_lo", MIDDLE_SHAPES)
def test_middle_pass(lab, fmt, K, n, s_lo, inverse):
    """k_ntt2_strided<K, true> (scratch formats 1 and 2; <K, false> under format 0): scratch in, scratch out, on every scratch family.  <6, true> and
    <7, true> first appear in a plan at 2^17 and 2^20."""
    w = M.omega(n, inverse)
    for tag, lanes in scratch_inputs(n, s_lo, K, 31):
        if fmt == 0:
            lanes = [[x % R for x in v] for v in lanes]
        out = lab.lab_ntt_pass(n, K, s_lo, stack(lanes, fmt), inverse=inverse, lanes=LANES)["out"]
        got = check_scratch(out, fmt, [M.run_pass(v, n, s_lo, K, w) for v in lanes], ("middle", K, n, s_lo, inverse, tag))
        if tag == "alias":
            bad = [i for i in range(1 << n) if (got[0][i] - got[1][i]) % R]
            assert not bad, ("middle", K, n, s_lo, "a and a + r disagree", bad[:8])


# ------------------------------------------------------------------------------------------------------------------------ last passes
LAST_SHAPES = [(5, 11), (5, 13), (6, 11), (6, 12), (7, 11), (7, 13)]


def _scratch(lanes, fmt):
    return [[x % R for x in v] for v in lanes] if fmt == 0 else lanes


@pytest.mark.parametrize("post_mode", [0, 1, 2])
@pytest.mark.parametrize("C,n", LAST_SHAPES)
def test_last_pass(lab, fmt, C, n, post_mode):
    """k_ntt2_final<C, 0>: bit-reversed canonical store, plain (forward tables), * 1 / D and * g^-k / D (inverse tables)"""
    inverse = post_mode != 0
    w = M.omega(n, inverse)
    for tag, lanes in scratch_inputs(n, 0, C, 41):
        lanes = _scratch(lanes, fmt)
        out = lab.lab_ntt_pass(n, C, 0, stack(lanes, fmt), inverse=inverse, last=True, lanes=LANES, posttab=post_mode == 2, post_mode=post_mode)["out"]
        want = [M.run_pass(v, n, 0, C, w, last=True, post_mode=post_mode) for v in lanes]
        check_canonical(out, want, ("last", C, n, post_mode, tag))
        if tag == "alias":
            assert want[0] == want[1]


def addend_inputs(n, C, fmt):
    fams, top = M.families(C, True), M.top_of(True)
    a, a2 = M.alias_pair(n, 51)
    return _scratch([fams["all_top"](n, 0, C, 0, top), a2, fams["stage%d_high" % (C - 1)](n, 0, C, 0, top)], fmt)


@pytest.mark.parametrize("C,n", LAST_SHAPES)
def test_last_pass_plus_addend(lab, fmt, C, n):
    """k_ntt2_final<C, 4>: canonical v + addend_k; with the addend -v every output word is exactly zero"""
    D, w = 1 << n, M.omega(n)
    lanes = addend_inputs(n, C, fmt)
    plain = [M.run_pass(v, n, 0, C, w, last=True) for v in lanes]
    for name, addend in (("0", [[0] * D] * LANES), ("r-1", [[R - 1] * D] * LANES), ("-v", [[(-x) % R for x in v] for v in plain])):
        out = lab.lab_ntt_pass(n, C, 0, stack(lanes, fmt), last=True, lanes=LANES, post_mode=4, addend=stack(addend, 0))["out"]
        want = [M.run_pass(v, n, 0, C, w, last=True, post_mode=4, addend=ad) for v, ad in zip(lanes, addend)]
        check_canonical(out, want, ("last + addend", C, n, name))
        if name == "-v":
            assert not out[:LANES * D].any(), ("last + addend", C, n, "a sum that cancels is not stored as zero")
    assert any(any(v) for v in plain)


@pytest.mark.parametrize("C,n", LAST_SHAPES)
def test_last_pass_minus_addend_times_constant(lab, fmt, C, n):
    """k_ntt2_final<C, 3>: (v g^-k / D - addend_k) c2; with the addend v g^-k / D every output word is exactly zero"""
    D, w = 1 << n, M.omega(n, True)
    c2 = random.Random(n * 8 + C).randrange(1, R)
    c2_word = M.encode([c2 * M.MONT % R], 0)[0]
    lanes = addend_inputs(n, C, fmt)
    scaled = [M.run_pass(v, n, 0, C, w, last=True, post_mode=2) for v in lanes]
    for name, addend in (("v", scaled), ("0", [[0] * D] * LANES), ("r-1", [[R - 1] * D] * LANES)):
        out = lab.lab_ntt_pass(n, C, 0, stack(lanes, fmt), inverse=True, last=True, lanes=LANES, posttab=True, post_mode=3, addend=stack(addend, 0),
                               postconst2=c2_word)["out"]
        want = [M.run_pass(v, n, 0, C, w, last=True, post_mode=3, addend=ad, c2=c2) for v, ad in zip(lanes, addend)]
        check_canonical(out, want, ("last - addend", C, n, name))
        if name == "v":
            assert not out[:LANES * D].any(), ("last - addend", C, n, "a difference that cancels is not stored as zero")
    assert any(any(v) for v in scaled)


# ------------------------------------------------------------------------------------------------------------------------ fused pass
@pytest.mark.parametrize("C,n", [(5, 11), (6, 11), (6, 12), (7, 11), (7, 14)])
def test_fused_pass(lab, fmt, C, n):
    """k_ntt2_final_first<C>: the model of "last pass with 1 / D, then first pass with g^i" (forward half: s_lo = n - C).  2^12 = 6 + 6 and 2^14 = 7 + 7
    are the plans that fuse; 2^14 runs the extreme and the alias lanes only."""
    cases = scratch_inputs(n, 0, C, 61)
    if n == 14:
        cases = [c for c in cases if c[0].startswith("all_top") or c[0] == "alias"]
    for tag, lanes in cases:
        lanes = _scratch(lanes, fmt)
        out = lab.lab_ntt_pass(n, C, 0, stack(lanes, fmt), fused=True, lanes=LANES)["out"]
        got = check_scratch(out, fmt, [M.run_fused(v, n, C) for v in lanes], ("fused", C, n, tag))
        if tag == "alias":
            assert not [i for i in range(1 << n) if (got[0][i] - got[1][i]) % R]


# ------------------------------------------------------------------------------------------------------------------------ argument errors
def test_probe_rejects_what_it_could_not_run_safely(czk, lab, fmt):
    D, words = 1 << 11, M.words_per_elem(fmt)
    good = np.zeros((D, words), dtype=np.uint32)

    def refused(*a, **k):
        with pytest.raises(czk.CzkError) as e:
            lab.lab_ntt_pass(*a, **k)
        assert e.value.code == 3, e.value                                # CZK_ERR_ARG
    lab.lab_ntt_pass(11, 5, 4, good)                                     # (the base case itself runs)
    refused(11, 5, 3, good)                                              # s_lo < 4
    refused(11, 5, 7, good)                                              # s_lo + K > log_d
    refused(11, 4, 4, good)                                              # K = 4
    refused(11, 8, 0, good, last=True)                                   # K = 8
    refused(15, 5, 4, np.zeros((1 << 15, words), dtype=np.uint32))       # log_d = 15
    refused(10, 5, 4, np.zeros((1 << 10, words), dtype=np.uint32))       # below the second generation's tables
    refused(11, 5, 4, good, last=True)                                   # a last pass has s_lo = 0
    refused(11, 5, 0, good, last=True, post_mode=5)
    refused(11, 5, 0, good, last=True, post_mode=2)                      # mode 2 without its table
    refused(11, 5, 0, good, last=True, post_mode=4)                      # mode 4 without an addend
    refused(11, 5, 4, good, post_mode=1)                                 # a post mode on a strided pass
    refused(11, 5, 4, good, prescale=True)                               # a pre-scale on a pass that is not first
    refused(11, 5, 4, good[:-1])                                         # a buffer one element short
    refused(11, 5, 4, good, lanes=2)
    refused(11, 5, 4, good, lanes=0)
    refused(11, 5, 4, np.zeros((D, 8), dtype=np.uint32), first=True, in_len=D + 1, in_lane_stride=D)
    refused(11, 5, 4, np.zeros((D, 8), dtype=np.uint32), first=True, in_len=D, in_lane_stride=D - 1)
    refused(12, 7, 0, np.zeros((1 << 12, words), dtype=np.uint32), fused=True, inverse=True)
    refused(10, 7, 0, np.zeros((1 << 10, words), dtype=np.uint32), fused=True)   # 4 + C > log_d
    # null data with sizes: the raw call
    desc = czk.binding.LabNttPassDesc(mode=0, log_d=11, K=5, s_lo=4, lanes=1)
    dims = np.zeros(21, dtype=np.uint64)
    null, dp = C.c_void_p(0), dims.ctypes.data_as(C.c_void_p)
    L = czk.binding.lab_lib()
    assert L.czk_lab_ntt_pass(lab._h, C.byref(desc), null, C.c_size_t(good.nbytes), null, null, dp, null, C.c_size_t(0)) == 3
    assert L.czk_lab_ntt_pass(lab._h, C.byref(desc), null, C.c_size_t(0), null, null, dp, null, C.c_size_t(64)) == 3
    assert L.czk_lab_ntt_pass(lab._h, C.byref(desc), good.ctypes.data_as(C.c_void_p), C.c_size_t(good.nbytes), null, null, dp, null, C.c_size_t(0)) == 3
    assert L.czk_lab_ntt_pass(lab._h, C.byref(desc), null, C.c_size_t(0), null, null, dp, null, C.c_size_t(0)) == 0


def test_probe_needs_the_lab_library(czk):
    ctx = czk.Context(0)
    with pytest.raises(RuntimeError):
        ctx.lab_ntt_pass(11, dims_only=True)
    assert not hasattr(czk.lib(), "czk_lab_ntt_pass")
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------------ product library, no probe
@pytest.fixture(scope="module")
def ctx(czk):
    c = czk.Context(0)
    yield c
    c.close()


def structured_lanes(D):
    """constant 1 and constant r - 1 (stored words), zero, impulses at 0, 1, D / 2, D - 1: (7, D, 4) u64"""
    lanes = [[1] * D, [R - 1] * D, [0] * D]
    for at in (0, 1 % D, D // 2, D - 1):
        v = [0] * D
        v[at] = R - 1
        lanes.append(v)
    return np.stack([ints_to_limbs(v, 4) for v in lanes])


def prefix_cases(D):
    tail = ints_to_limbs([M.DEADBEEF], 4)[0]
    out = []
    for in_len in sorted({x for x in (0, 1, D // 2 + 1, D - 3, D) if 0 <= x <= D}):
        rng = random.Random(D + in_len)
        v = ints_to_limbs([rng.randrange(R) for _ in range(D)], 4)
        v[in_len:] = tail
        out.append((in_len, v))
    return out


def run_structured(ctx, orc, transform, oracle, size_arg, D, tag):
    lanes = structured_lanes(D)
    for kind in range(4):
        got = lanes.copy()
        transform(got, size_arg, kind, lanes=lanes.shape[0])
        for ln in range(lanes.shape[0]):
            assert np.array_equal(got[ln], oracle(lanes[ln], size_arg, kind)), (tag, kind, "lane", ln)
        for in_len, v in prefix_cases(D):
            got = v.copy()
            transform(got, size_arg, kind, in_len=in_len)
            assert np.array_equal(got, oracle(v, size_arg, kind, in_len=in_len)), (tag, kind, "in_len", in_len)


@pytest.mark.parametrize("log_d", range(1, 15))
def test_product_ntt_on_structured_inputs(ctx, orc, log_d):
    """czk_ntt_fr: the first-generation kernels below 2^11, the second generation from there on; almost every output is 0 or a repeated value"""
    run_structured(ctx, orc, ctx.ntt_fr, orc.ntt_fr, log_d, 1 << log_d, ("ntt_fr", log_d))


@pytest.mark.parametrize("log_d", [11, 12])
def test_product_ntt_first_generation_on_structured_inputs(czk, orc, log_d):
    c = czk.Context(0, options={"ntt_gen1": 1})
    run_structured(c, orc, c.ntt_fr, orc.ntt_fr, log_d, 1 << log_d, ("ntt_fr, ntt_gen1", log_d))
    c.close()


@pytest.mark.parametrize("k", [1, 5, 9])
def test_product_mixed_radix_ntt_on_structured_inputs(ctx, orc, k):
    size = 3 << k
    run_structured(ctx, orc, ctx.ntt_fr_mixed, orc.ntt_fr_mixed, size, size, ("ntt_fr_mixed", size))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("log_d", [11, 12])
def test_product_witness_map_outputs_that_vanish(czk, orc, log_d):
    """czk_witness_map_pre_masked with masks equal to the negated transform, czk_witness_map_post_h with ab = coset_fft(ifft(c)): post modes 4 and 3 store
    all-zero vectors through the product path ("witness_map_short" = 7), and the longer kernel sequences (= 0) agree bit for bit"""
    import torch
    d, lanes = 1 << log_d, 2
    rng = random.Random(log_d)
    a, b, c = (np.stack([ints_to_limbs([rng.randrange(R) for _ in range(d)], 4) for _ in range(lanes)]) for _ in range(3))
    a[1, d // 2:] = 0
    b[0] = ints_to_limbs([R - 1], 4)[0]                                                       # a constant lane: its ifft is an impulse
    pre = [orc.witness_map_pre(a[ln], b[ln], log_d) for ln in range(lanes)]
    ma, mb = np.stack([orc.fr_neg(p[0]) for p in pre]), np.stack([orc.fr_neg(p[1]) for p in pre])
    ab = np.stack([orc.ntt_fr(orc.ntt_fr(c[ln], log_d, 1), log_d, 2) for ln in range(lanes)])
    assert not any(orc.witness_map_post(ab[ln], c[ln], log_d).any() for ln in range(lanes))     # the checker's h is zero
    results = {}
    for opt in (7, 0):
        cx = czk.Context(0, options={"witness_map_short": opt})
        ta, tb, tma, tmb, tab, tc = (_dev(x) for x in (a, b, ma, mb, ab, c))
        torch.cuda.synchronize()
        cx.witness_map_pre_masked(ta.data_ptr(), tb.data_ptr(), tma.data_ptr(), tmb.data_ptr(), log_d, lanes)
        cx.witness_map_post_h(tab.data_ptr(), tc.data_ptr(), log_d, lanes)
        cx.sync()
        results[opt] = [_host(t).copy() for t in (ta, tb, tab)]
        cx.close()
        for name, got in zip(("a + mask_a", "b + mask_b", "h"), results[opt]):
            assert not got.any(), (opt, name, "not all zero", np.flatnonzero(got.reshape(-1, 4).any(axis=1))[:8].tolist())
    assert all(np.array_equal(x, y) for x, y in zip(results[7], results[0]))
    # and with masks / a product that do NOT cancel, against the checker
    ma2 = ma.copy()
    ma2[:, ::3] = ints_to_limbs([R - 1], 4)[0]
    ab2 = ab.copy()
    ab2[:, 1::2] = 0
    for opt in (7, 0):
        cx = czk.Context(0, options={"witness_map_short": opt})
        ta, tb, tma, tmb, tab, tc = (_dev(x) for x in (a, b, ma2, mb, ab2, c))
        torch.cuda.synchronize()
        cx.witness_map_pre_masked(ta.data_ptr(), tb.data_ptr(), tma.data_ptr(), tmb.data_ptr(), log_d, lanes)
        cx.witness_map_post_h(tab.data_ptr(), tc.data_ptr(), log_d, lanes)
        cx.sync()
        ga, gh = _host(ta), _host(tab)
        cx.close()
        for ln in range(lanes):
            assert np.array_equal(ga[ln], orc.fr_add(pre[ln][0], ma2[ln])), (opt, "a + mask_a", ln)
            assert np.array_equal(gh[ln], orc.witness_map_post(ab2[ln], c[ln], log_d)), (opt, "h", ln)
