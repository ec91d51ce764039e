"""czk_fr_random, czk_gsz_dn_generate and czk_gsz_dn_check (csrc/gsz_dn.hip, include/czk.h) against tests/gsz_dn_model.py: the keyed generator element
for element, the generated lanes limb for limb at every instantiation and on the generic path, where the kernels write and how their grid-stride
loops end, the generated material at work in gsz20's product and product check, the consistency check on honest and perturbed lanes, and the
argument rules."""
import functools
import os
import random
import re

import numpy as np
import pytest
import torch

import gsz_dn_model as DN
import gsz_mul_model as M
import guarded
from guarded import Guards
from gsz_mul_model import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = bytes(range(32))
NONCE = bytes.fromhex("000000090000004a00000000")
ERR_SIZE, ERR_ARG = 1, 3


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _domain(parties):
    return M.Domain(parties)


def _keys(parties, seed):
    rng = random.Random(seed)
    return [bytes(rng.randrange(256) for _ in range(32)) for _ in range(parties)]


def _nonce(kind, seq):
    return kind.to_bytes(4, "little") + seq.to_bytes(8, "little")


def _limbs(lane):
    return M.to_limbs([lane])[0]


def _guards_ready():
    """the guard bands are filled by torch kernels on torch's stream, the calls under test run on the context's own: the fill must have ended before them"""
    torch.cuda.synchronize()


def _per_cu_blocks():
    """blocks per CU that cap the grids of gsz_dn.hip, on blocks of 256 threads"""
    src = open(os.path.join(ROOT, "collaborative-zksnark_amd", "csrc", "gsz_dn.hip")).read()
    m = re.search(r"constexpr size_t GSZ_DN_BLOCKS_PER_CU = (\d+);", src)
    assert m and "const size_t cap = GSZ_DN_BLOCKS_PER_CU * (size_t)ctx->num_cu;" in src and "size_t blocks = (n + 255) / 256;" in src
    assert "const unsigned g = dn_grid(ctx, a.outputs);" in src and "const dim3 grid(g), b(256);" in src
    for k in ("(k_gsz_dn<LN, true>)", "(k_gsz_dn<LN, false>)", "(k_gsz_dn<0, true>)", "(k_gsz_dn<0, false>)"):
        assert f"hipLaunchKernelGGL({k}, grid, b," in src, k
    assert "hipLaunchKernelGGL(k_fr_random, dim3(dn_grid(ctx, n)), dim3(256)," in src
    return int(m.group(1))


# ---- the keyed generator ------------------------------------------------------------------------------------------------------------------------------
FR_RANDOM_CALLS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 257), (123456789, 65), ((1 << 32) - 257, 257)]     # the last one ends at 2^32 exactly


@pytest.mark.gpu
def test_fr_random_is_the_models_stream(ctx):
    for first, n in FR_RANDOM_CALLS:
        want = _limbs(DN.sample(KEY, NONCE, first, n))
        assert np.array_equal(ctx.fr_random(KEY, NONCE, first, n), want), (first, n)
    # another key, another nonce: other elements, still the model's
    k2, n2 = bytes(reversed(KEY)), bytes(range(100, 112))
    got = ctx.fr_random(k2, n2, 7, 65)
    assert np.array_equal(got, _limbs(DN.sample(k2, n2, 7, 65))) and not np.array_equal(got, ctx.fr_random(KEY, n2, 7, 65))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["host", "device"])
def test_fr_random_writes_n_elements_and_nothing_else(ctx, where):
    import czk_amd
    mem = czk_amd.CZK_MEM_HOST if where == "host" else czk_amd.CZK_MEM_DEVICE
    for first, n in FR_RANDOM_CALLS:
        G = Guards("cpu" if where == "host" else "cuda")
        out = G.out(1, n)
        _guards_ready()
        ctx.fr_random(KEY, NONCE, first, n, out=out.ptr, mem=mem)
        ctx.sync()
        assert np.array_equal(G.check()[0][0], _limbs(DN.sample(KEY, NONCE, first, n))), (first, n)
    G = Guards("cuda")
    out = G.out(1, 4)
    _guards_ready()
    ctx.fr_random(KEY, NONCE, 5, 0, out=out.ptr, mem=czk_amd.CZK_MEM_DEVICE)
    ctx.sync()
    assert out.untouched()


@pytest.mark.gpu
def test_fr_random_second_trip_of_the_grid(ctx):
    import czk_amd
    T = guarded.grid_threads(_per_cu_blocks())
    n = T + 3
    G = Guards("cuda")
    out = G.out(1, n)
    _guards_ready()
    ctx.fr_random(KEY, NONCE, 11, n, out=out.ptr, mem=czk_amd.CZK_MEM_DEVICE)
    ctx.sync()
    got = G.check()[0][0]
    for lo, hi in ((0, 64), (T - 64, n)):
        assert np.array_equal(got[lo:hi], _limbs(DN.sample(KEY, NONCE, 11 + lo, hi - lo))), (lo, hi)
    assert len(np.unique(got, axis=0)) == n and bool((got[:, 3] < (0x12ab655e9a2ca556 + 1)).all())      # distinct and below r's top limb bound


# ---- generation ---------------------------------------------------------------------------------------------------------------------------------------
def _generate(ctx, kind, parties, d, keys, nonce, deal):
    """-> (r, r2) as (parties, outputs, 4) uint64, written into guard bands"""
    outputs = deal * (parties - d)
    G = Guards("cuda")
    r = G.out(parties, outputs, name="out_r")
    r2 = G.out(parties, outputs, name="out_r2") if kind == DN.KIND_DOUBLES else None
    _guards_ready()
    ctx.gsz_dn_generate(kind, parties, d, keys, nonce, deal, r.ptr, None if r2 is None else r2.ptr)
    ctx.sync()
    foot = G.check()
    return foot[0], (foot[1] if r2 is not None else None)


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [3, 4, 6, 8, 12, 1, 2])              # the four instantiations, the generic path, and the worlds without a polynomial
def test_generated_lanes_are_the_models(ctx, parties):
    D, d = _domain(parties), M.threshold(parties)
    keys = _keys(parties, 100 + parties)
    for kind in (DN.KIND_DOUBLES, DN.KIND_RANDS):
        for deal in (1, 2, 65, 257):
            nonce = _nonce(kind, deal)
            assert ctx.gsz_dn_counts(kind, parties, d, deal * (parties - d)) == (deal, deal * (parties - d))
            got, got2 = _generate(ctx, kind, parties, d, keys, nonce, deal)
            want, want2 = DN.generate(D, kind, d, keys, nonce, deal)
            assert np.array_equal(got, M.to_limbs(want)), (kind, deal)
            if kind == DN.KIND_DOUBLES:
                assert np.array_equal(got2, M.to_limbs(want2)), (kind, deal)


@pytest.mark.gpu
def test_random_shares_of_any_degree_below_the_parties(ctx):
    """CZK_GSZ_DN_RANDS takes every d < parties (the registers of the instantiations are sized for it); doubles every 2 d < parties"""
    for parties, d, kind in ((4, 3, DN.KIND_RANDS), (8, 7, DN.KIND_RANDS), (8, 0, DN.KIND_RANDS), (6, 1, DN.KIND_DOUBLES), (8, 2, DN.KIND_DOUBLES), (12, 11, DN.KIND_RANDS)):
        keys, nonce, deal = _keys(parties, d), _nonce(kind, 77), 3
        got, got2 = _generate(ctx, kind, parties, d, keys, nonce, deal)
        want, want2 = DN.generate(_domain(parties), kind, d, keys, nonce, deal)
        assert np.array_equal(got, M.to_limbs(want)) and (want2 is None or np.array_equal(got2, M.to_limbs(want2))), (parties, d)


@pytest.mark.gpu
@pytest.mark.parametrize("parties,side", [(4, 0), (4, 1), (12, 1)])
def test_generation_either_side_of_the_second_trip(ctx, parties, side):
    """outputs just below / just above T (4 parties) resp. just over T (12 parties, whose parked coefficients are indexed by the grid's thread count): the items around the
    trip boundary and at both ends against the model, the guard bands, and every remaining output through czk_fr_gsz_open -- calls this file does not touch"""
    T = guarded.grid_threads(_per_cu_blocks())
    D, d, kind = _domain(parties), M.threshold(parties), DN.KIND_DOUBLES
    per = parties - d
    deal = T // per + side
    outputs = deal * per
    assert (T - per < outputs <= T) if side == 0 else (T < outputs < T + per + 1)
    keys, nonce = _keys(parties, 5), _nonce(kind, 9)
    G = Guards("cuda")
    r, r2 = G.out(parties, outputs, name="out_r"), G.out(parties, outputs, name="out_r2")
    _guards_ready()
    ctx.gsz_dn_generate(kind, parties, d, keys, nonce, deal, r.ptr, r2.ptr)
    ctx.sync()
    got, got2 = G.check()
    near = [t for t in list(range(64)) + list(range(max(T - 64, 0), min(T + 64, outputs))) + list(range(outputs - 64, outputs))]
    items = sorted({t % deal for t in near})
    want, want2 = DN.generate(D, kind, d, keys, nonce, deal, items=items)
    idx = DN.output_indices(D, d, deal, items)
    assert set(near) <= set(idx)
    assert np.array_equal(got[:, idx], M.to_limbs(want)) and np.array_equal(got2[:, idx], M.to_limbs(want2))
    # the rest: both halves are sharings within their bounds of the same values
    v1 = torch.empty((outputs, 4), dtype=torch.int64, device="cuda")
    v2 = torch.empty_like(v1)
    assert ctx.fr_gsz_open(r.ptr, parties, outputs, v1.data_ptr(), degree=d) == 0
    assert ctx.fr_gsz_open(r2.ptr, parties, outputs, v2.data_ptr(), degree=2 * d) == 0
    assert torch.equal(v1, v2) and len(torch.unique(v1, dim=0)) == outputs
    if d:                                                           # ... and not of a lower degree: the degree-d half exceeds d - 1 everywhere
        assert ctx.fr_gsz_open(r.ptr, parties, outputs, v2.data_ptr(), degree=d - 1) == outputs


# ---- the material at work -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("parties", [3, 4])
def test_generated_material_multiplies_and_passes_the_product_check(ctx, parties):
    D, d, n = _domain(parties), M.threshold(parties), 33
    rng = random.Random(parties)
    xv, yv = [rng.randrange(R_MOD) for _ in range(n)], [rng.randrange(R_MOD) for _ in range(n)]
    keys = _keys(parties, 8)

    def material(kind, want, seq):
        deal, outputs = ctx.gsz_dn_counts(kind, parties, d, want + 2)
        r = torch.empty((parties, outputs, 4), dtype=torch.int64, device="cuda")
        r2 = torch.empty_like(r) if kind == DN.KIND_DOUBLES else None
        ctx.gsz_dn_generate(kind, parties, d, keys, _nonce(kind, seq), deal, r.data_ptr(), None if r2 is None else r2.data_ptr())
        assert ctx.gsz_dn_check(kind, parties, d, r.data_ptr(), None if r2 is None else r2.data_ptr(), outputs) == (True, 0)
        out = r[:, :want].contiguous(), (None if r2 is None else r2[:, :want].contiguous())
        _guards_ready()                                             # (torch copied on its own stream)
        return out

    up = lambda lanes: torch.from_numpy(M.to_limbs(lanes).view(np.int64)).cuda()       # noqa: E731
    x, y = up(D.share(xv, d, rng)), up(D.share(yv, d, rng))
    dr, dr2 = material(DN.KIND_DOUBLES, n, 1)
    z = torch.empty_like(x)
    assert ctx.gsz_share_batch_mul(parties, d, x.data_ptr(), y.data_ptr(), dr.data_ptr(), dr2.data_ptr(), z.data_ptr(), n) == (0, 0)
    ctx.sync()
    assert D.batch_open(M.from_limbs(z.cpu().numpy().view(np.uint64)), d) == ([a * b % R_MOD for a, b in zip(xv, yv)], 0)
    nd, nr = ctx.gsz_material_counts(3, n)
    cr, cr2 = material(DN.KIND_DOUBLES, nd, 2)
    rands, _ = material(DN.KIND_RANDS, nr, 3)
    assert ctx.gsz_product_check(parties, d, x.data_ptr(), y.data_ptr(), z.data_ptr(), n, cr.data_ptr(), cr2.data_ptr(), rands.data_ptr()) == (True, 0)


# ---- the consistency check ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _check_case(parties, kind, deal):
    """generated lanes from the model, shared and never modified -> (r, r2) lists of lanes"""
    D, d = _domain(parties), M.threshold(parties)
    return DN.generate(D, kind, d, _keys(parties, 50 + parties), _nonce(kind, 1000 + deal), deal)


def _run_check(ctx, kind, parties, d, r, r2):
    G = Guards("cuda")
    fr = G.freeze(M.to_limbs(r).reshape(-1, 4), "r")
    fr2 = G.freeze(M.to_limbs(r2).reshape(-1, 4), "r2") if r2 is not None else None
    res = ctx.gsz_dn_check(kind, parties, d, fr.ptr, None if fr2 is None else fr2.ptr, len(r[0]))
    G.check()                                                       # the check does not modify its inputs
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [3, 4, 6, 8, 12])
def test_the_check_accepts_what_was_generated(ctx, parties):
    D, d = _domain(parties), M.threshold(parties)
    for kind in (DN.KIND_DOUBLES, DN.KIND_RANDS):
        for deal in (2, 5, 300):                                   # 300 items: more than one block of the fold, a ragged last one
            r, r2 = _check_case(parties, kind, deal)
            assert DN.check(D, kind, d, r, r2) == (1, 0, True)
            assert _run_check(ctx, kind, parties, d, r, r2) == (True, 0), (kind, deal)


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [3, 4, 8])
def test_one_wrong_element_is_caught_the_way_the_model_says(ctx, parties):
    D, d = _domain(parties), M.threshold(parties)
    for kind in (DN.KIND_DOUBLES, DN.KIND_RANDS):
        for deal, lane, at in ((5, 1, 0), (300, parties - 1, 257), (300, 0, 300 * (parties - d) - 1), (300, 1, 300 * (parties - d) - 2)):
            r, r2 = _check_case(parties, kind, deal)
            r = [ln[:] for ln in r]
            r[lane][at] = (r[lane][at] + 1) % R_MOD
            ok, bad, equal = DN.check(D, kind, d, r, r2)
            assert ok == 0 and bad > 0                              # a single lane off by one is no polynomial of degree d
            assert _run_check(ctx, kind, parties, d, r, r2) == (False, bad), (kind, deal, lane, at)


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [3, 4, 8])
def test_a_second_half_of_another_value_fails_on_the_equality_alone(ctx, parties):
    D, d = _domain(parties), M.threshold(parties)
    r, r2 = _check_case(parties, DN.KIND_DOUBLES, 5)
    for only in (None, 3):                                          # every output's second half shifted by a constant on every lane; then output 3's alone
        s2 = [[(v + 12345) % R_MOD if only in (None, i) else v for i, v in enumerate(ln)] for ln in r2]
        assert DN.check(D, DN.KIND_DOUBLES, d, r, s2) == (0, 0, False)
        assert _run_check(ctx, DN.KIND_DOUBLES, parties, d, r, s2) == (False, 0), only
    assert _run_check(ctx, DN.KIND_RANDS, parties, d, r, None) == (True, 0)                   # the first half alone is still consistent


# ---- argument rules -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_rules(ctx):
    import czk_amd

    def code(fn, *a, **k):
        try:
            fn(*a, **k)
        except czk_amd.binding.CzkError as e:
            return e.code
        return 0
    G = Guards("cuda")
    r, r2 = G.out(8, 64, name="out_r"), G.out(8, 64, name="out_r2")
    _guards_ready()
    gen = ctx.gsz_dn_generate
    keys = _keys(8, 1)
    # fr_random
    assert code(ctx.fr_random, KEY, NONCE, (1 << 32) - 1, 2, out=r.ptr, mem=czk_amd.CZK_MEM_DEVICE) == ERR_SIZE
    assert code(ctx.fr_random, KEY, NONCE, 1, 1 << 32, out=r.ptr, mem=czk_amd.CZK_MEM_DEVICE) == ERR_SIZE
    assert code(ctx.fr_random, KEY, NONCE, 0, 4, out=None, mem=czk_amd.CZK_MEM_DEVICE) == ERR_ARG
    assert code(ctx.fr_random, KEY, NONCE, 0, 4, out=r.ptr, mem=77) == ERR_ARG
    with pytest.raises(ValueError):
        ctx.fr_random(KEY[:31], NONCE, 0, 4)
    # generate: the degree rules, the sizes, nothing to do, null pointers
    assert code(gen, DN.KIND_DOUBLES, 4, 2, keys[:4], NONCE, 4, r.ptr, r2.ptr) == ERR_ARG           # 2 d >= P
    assert code(gen, DN.KIND_DOUBLES, 3, 2, keys[:3], NONCE, 4, r.ptr, r2.ptr) == ERR_ARG
    assert code(gen, DN.KIND_RANDS, 4, 4, keys[:4], NONCE, 4, r.ptr) == ERR_ARG                     # d >= P
    assert code(gen, 2, 4, 1, keys[:4], NONCE, 4, r.ptr, r2.ptr) == ERR_ARG                         # no such kind
    assert code(gen, DN.KIND_RANDS, 5, 1, keys[:5], NONCE, 4, r.ptr) == ERR_SIZE                    # no share domain
    assert code(gen, DN.KIND_RANDS, 0, 0, b"", NONCE, 4, r.ptr) == ERR_SIZE
    assert code(gen, DN.KIND_RANDS, 128, 1, _keys(128, 2), NONCE, 4, r.ptr) == ERR_SIZE             # more than 96 parties
    assert code(gen, DN.KIND_DOUBLES, 4, 1, keys[:4], NONCE, (1 << 32) // 4 + 1, r.ptr, r2.ptr) == ERR_SIZE    # deal draws > 2^32
    assert code(gen, DN.KIND_RANDS, 4, 1, keys[:4], NONCE, (1 << 31) + 1, r.ptr) == ERR_SIZE
    assert code(gen, DN.KIND_DOUBLES, 4, 1, keys[:4], NONCE, 0, r.ptr, r2.ptr) == 0                 # deal = 0: nothing touched
    assert code(gen, DN.KIND_DOUBLES, 4, 1, keys[:4], NONCE, 0, None, None) == 0
    assert code(gen, DN.KIND_DOUBLES, 4, 1, keys[:4], NONCE, 4, r.ptr, None) == ERR_ARG
    assert code(gen, DN.KIND_RANDS, 4, 1, keys[:4], NONCE, 4, None) == ERR_ARG
    # check
    chk = ctx.gsz_dn_check
    assert code(chk, DN.KIND_DOUBLES, 4, 1, r.ptr, r2.ptr, 2) == ERR_ARG                            # two outputs are sacrificed: nothing left to check
    assert code(chk, DN.KIND_DOUBLES, 4, 1, r.ptr, None, 12) == ERR_ARG
    assert code(chk, DN.KIND_DOUBLES, 4, 2, r.ptr, r2.ptr, 12) == ERR_ARG
    assert code(chk, DN.KIND_RANDS, 5, 1, r.ptr, None, 12) == ERR_SIZE
    assert code(chk, DN.KIND_RANDS, 4, 1, r.ptr, None, 1 << 32) == ERR_SIZE
    ctx.sync()
    assert r.untouched() and r2.untouched()
