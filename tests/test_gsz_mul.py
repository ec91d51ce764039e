"""czk_gsz_share_batch_mul / _batch_inv / _partial_products and czk_gsz_product_check (csrc/gsz_mul.hip, include/czk.h) against the big-integer model of
gsz20's protocols (tests/gsz_mul_model.py): every output lane limb for limb, the verdict and the counts, tampered contributions at 3 and 4 parties,
zero divisors, where the kernels write and how their grid-stride loops and block partials end, and the argument rules."""
import functools
import os
import random
import re

import numpy as np
import pytest

import gsz_mul_model as M
from gsz_mul_model import R_MOD
from util import rand_fr_canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"mul": M.OP_MUL, "inv": M.OP_INV, "pp": M.OP_PARTIAL_PRODUCTS}
PARTIES = [3, 4, 6, 8, 12]                                           # the four register-resident instantiations and the generic path


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _domain(parties):
    return M.Domain(parties)


@functools.lru_cache(maxsize=None)
def _case(parties, op, n, zero_at=None):
    """One product call's inputs and the model's outputs, computed once and shared (never modified: tests copy what they change).
    -> dict of (parties, k, 4) uint64 limb arrays x, y, dr, dr2, rands, want + bad, zero, opened"""
    D, t = _domain(parties), M.threshold(parties)
    rng = random.Random(7 * n + op + 100 * parties)
    xv = [rng.randrange(1, R_MOD) for _ in range(n)]
    if zero_at is not None:
        xv[zero_at] = 0
    x, y = D.share(xv, t, rng), D.share([rng.randrange(R_MOD) for _ in range(n)], t, rng)
    src = M.random_material(D, t, op, n, seed=n + 17 * op)
    if op == M.OP_MUL:
        want, bad = M.batch_mult(D, t, x, y, src)
        zero = 0
    elif op == M.OP_INV:
        want, bad, zero = M.batch_inv(D, t, x, src)
    else:
        want, bad, zero = M.partial_products(D, t, x, src)
    assert (src.d, src.r) == M.material_counts(op, n)
    c = {k: M.to_limbs(v) for k, v in (("x", x), ("y", y), ("dr", src.dr), ("dr2", src.dr2), ("want", want))}
    c["rands"] = M.to_limbs(src.rands) if src.rands[0] else np.zeros((parties, 1, 4), np.uint64)
    c.update(bad=bad, zero=zero, opened=D.batch_open(want, t)[0], xv=xv)
    return c


@functools.lru_cache(maxsize=None)
def _check_case(parties, n, wrong_z=False, bad_material=False):
    """n triples from a batch_mult, the check's material and the model's verdict -> limb arrays xs, ys, zs, dr, dr2, rands + ok, bad"""
    D, t = _domain(parties), M.threshold(parties)
    rng = random.Random(31 * n + parties)
    x, y = D.share([rng.randrange(R_MOD) for _ in range(n)], t, rng), D.share([rng.randrange(R_MOD) for _ in range(n)], t, rng)
    z, _ = M.batch_mult(D, t, x, y, M.random_material(D, t, M.OP_MUL, n, seed=n))
    if wrong_z:                                                      # a consistent sharing of 1 added to the last product: no degree test sees it
        one = D.share([1], t, rng)
        z = [ln[:-1] + [(ln[-1] + o[0]) % R_MOD] for ln, o in zip(z, one)]
    src = M.random_material(D, t, M.OP_PRODUCT_CHECK, n, seed=5 * n + 1)
    if bad_material:                                                 # party 1's share of the LAST double's r2 and of the first coin are off by one
        src.dr2[1][-1] = (src.dr2[1][-1] + 1) % R_MOD
        src.rands[1][0] = (src.rands[1][0] + 1) % R_MOD
    keep = {k: M.to_limbs(v) for k, v in (("xs", x), ("ys", y), ("zs", z), ("dr", src.dr), ("dr2", src.dr2), ("rands", src.rands))}
    ok, bad = M.hadamard_check(D, t, x, y, z, src)
    assert (src.d, src.r) == M.material_counts(M.OP_PRODUCT_CHECK, n)
    keep.update(ok=ok, bad=bad)
    return keep


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _run(ctx, parties, op, n, c, d=None):
    """one lanes-form product call on device copies of the case's arrays (d: already uploaded / tampered ones) -> (limbs, bad, zero)"""
    import torch
    d = dict(d or {})
    for k in ("x", "y", "dr", "dr2", "rands"):
        if k not in d:
            d[k] = _dev(c[k])
    out = torch.empty((parties, n, 4), dtype=torch.int64, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items()}
    t = M.threshold(parties)
    if op == M.OP_MUL:
        bad, zero = ctx.gsz_share_batch_mul(parties, t, p["x"], p["y"], p["dr"], p["dr2"], out.data_ptr(), n)
    else:
        fn = ctx.gsz_share_batch_inv if op == M.OP_INV else ctx.gsz_share_partial_products
        bad, zero = fn(parties, t, p["x"], p["dr"], p["dr2"], p["rands"], out.data_ptr(), n)
    return out.cpu().numpy().view(np.uint64), bad, zero


def _run_check(ctx, parties, n, c, d=None):
    d = dict(d or {})
    for k in ("xs", "ys", "zs", "dr", "dr2", "rands"):
        if k not in d:
            d[k] = _dev(c[k])
    p = {k: v.data_ptr() for k, v in d.items()}
    return ctx.gsz_product_check(parties, M.threshold(parties), p["xs"], p["ys"], p["zs"], n, p["dr"], p["dr2"], p["rands"])


# ---- bit-exact -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 1025])            # either side of the scan's 32-element segment and of a block
@pytest.mark.parametrize("parties", PARTIES)
def test_products_equal_the_model_limb_for_limb(ctx, parties, n):
    for name, op in OPS.items():
        c = _case(parties, op, n)
        assert ctx.gsz_material_counts(op, n) == M.material_counts(op, n)
        got, bad, zero = _run(ctx, parties, op, n, c)
        assert (bad, zero) == (c["bad"], c["zero"]) == (0, 0), name
        assert np.array_equal(got, c["want"]), (name, "first differing lane", int(np.argwhere((got != c["want"]).any(axis=(1, 2)))[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 33, 1025])           # odd lengths at every level of the halving; 1025: several blocks of partials
@pytest.mark.parametrize("parties", PARTIES)
def test_product_check_gives_the_models_verdict_and_count(ctx, parties, n):
    assert ctx.gsz_material_counts(M.OP_PRODUCT_CHECK, n) == M.material_counts(M.OP_PRODUCT_CHECK, n)
    for kw, want in (({}, (True, 0)), ({"wrong_z": True}, (False, 0)), ({"bad_material": True}, None)):
        c = _check_case(parties, n, **kw)
        if want is not None:
            assert (c["ok"], c["bad"]) == want, kw
        elif 2 * M.threshold(parties) < parties - 1:
            assert c["bad"] == 2, kw                                 # the king's bound sees the double, the open's bound the coin
        else:
            assert c["bad"] == 1, kw                                 # 3 parties: the king's bound is vacuous
        assert _run_check(ctx, parties, n, c) == (c["ok"], c["bad"]), kw


@pytest.mark.gpu
def test_stand_in_shares_and_dummy_material_pass_the_check(ctx):
    """the reference's own case: every party holds the value, every random share is one (gsz20/mod.rs:383-406)"""
    D, n = _domain(3), 5
    x, y = D.public([5, 7, 11, 13, 17]), D.public([2, 3, 4, 5, 6])
    src = M.dummy_material(D, M.OP_MUL, n)
    c = {k: M.to_limbs(v) for k, v in (("x", x), ("y", y), ("dr", src.dr), ("dr2", src.dr2))}
    c["rands"] = np.zeros((3, 1, 4), np.uint64)
    got, bad, zero = _run(ctx, 3, M.OP_MUL, n, c)
    assert (bad, zero) == (0, 0) and np.array_equal(got, M.to_limbs(D.public([10, 21, 44, 65, 102])))
    src = M.dummy_material(D, M.OP_PRODUCT_CHECK, n)
    cc = {"xs": c["x"], "ys": c["y"], "zs": got, "dr": M.to_limbs(src.dr), "dr2": M.to_limbs(src.dr2), "rands": M.to_limbs(src.rands)}
    assert _run_check(ctx, 3, n, cc) == (True, 0)


# ---- tampering -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_wrong_contribution_is_caught_by_the_kings_bound_at_4_parties_and_only_by_the_check_at_3(ctx):
    import torch
    n = 33
    for parties in (4, 3):
        t = M.threshold(parties)
        c = _case(parties, M.OP_MUL, n)
        r2 = _dev(c["dr2"])
        r2[1, 5, 2] ^= 1 << 7                                        # party 1's x y + r2 for element 5
        got, bad, zero = _run(ctx, parties, M.OP_MUL, n, c, {"dr2": r2})
        if parties == 4:
            assert bad == 1 and zero == 0
            continue
        assert (bad, zero) == (0, 0) and not np.array_equal(got[:, 5], c["want"][:, 5])
        assert np.array_equal(np.delete(got, 5, axis=1), np.delete(c["want"], 5, axis=1))
        z = _dev(got)
        opened = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        assert ctx.fr_gsz_open(z.data_ptr(), 3, n, opened.data_ptr(), degree=t) == 0      # still a consistent degree-t sharing, of a wrong product
        src = M.random_material(_domain(3), t, M.OP_PRODUCT_CHECK, n, seed=77)
        cc = {"xs": c["x"], "ys": c["y"], "zs": got, "dr": M.to_limbs(src.dr), "dr2": M.to_limbs(src.dr2), "rands": M.to_limbs(src.rands)}
        assert _run_check(ctx, 3, n, cc) == (False, 0)
        cc["zs"] = c["want"]
        assert _run_check(ctx, 3, n, cc) == (True, 0)
        # a flipped limb in one party's z is no consistent sharing any more: the open's degree bound sees it
        z = _dev(c["want"])
        z[1, 5, 2] ^= 1 << 7
        assert ctx.fr_gsz_open(z.data_ptr(), 3, n, opened.data_ptr(), degree=t) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [3, 8])
def test_zero_divisors_are_counted_and_their_outputs_are_zero(ctx, parties):
    n = 33
    c = _case(parties, M.OP_INV, n, zero_at=20)
    got, bad, zero = _run(ctx, parties, M.OP_INV, n, c)
    assert (bad, zero) == (0, 1) == (c["bad"], c["zero"]) and np.array_equal(got, c["want"])
    assert not got[:, 20].any() and got[:, 19].any()
    c = _case(parties, M.OP_PARTIAL_PRODUCTS, n, zero_at=20)
    got, bad, zero = _run(ctx, parties, M.OP_PARTIAL_PRODUCTS, n, c)
    assert (bad, zero) == (0, 0) and np.array_equal(got, c["want"])
    assert all(c["opened"][:20]) and c["opened"][20:] == [0] * (n - 20)   # later running products open to zero: no error


# ---- tails and footprints ----------------------------------------------------------------------------------------------------------------------------
def _per_cu_blocks():
    """blocks per CU that cap the grids of gsz_mul.hip, on blocks of 256 threads"""
    src = open(os.path.join(ROOT, "collaborative-zksnark_amd", "csrc", "gsz_mul.hip")).read()
    m = re.search(r"constexpr size_t GSZ_MUL_BLOCKS_PER_CU = (\d+);", src)
    assert m and "const size_t cap = GSZ_MUL_BLOCKS_PER_CU * (size_t)ctx->num_cu;" in src and "size_t blocks = (n + 255) / 256;" in src
    for k in ("k_gsz_mul<LN>", "k_gsz_mul<0>"):
        assert re.search(rf"hipLaunchKernelGGL\({re.escape(k)}, g, b,", src), k
    assert "CZK_GSZ_SWEEP(k_gsz_hadamard, P, dim3(g0), b," in src and "const unsigned P = (unsigned)parties, R = ceil_log2(n), g0 = gsz_mul_grid(ctx, n);" in src
    assert "const unsigned g = gsz_mul_grid(ctx, h);" in src and src.count("(k_gsz_ip<") == src.count("hipLaunchKernelGGL(k_gsz_ip<") == src.count("k_gsz_ip<3>, dim3(g), b,") + src.count("k_gsz_ip<4>, dim3(g), b,") == 2 and "hipLaunchKernelGGL(k_gsz_fold, dim3(g), b," in src
    return int(m.group(1))


def test_grid_cap_is_where_the_test_reads_it():
    assert _per_cu_blocks() == 8


def _rand_lanes(seed, lanes, n, orc):
    return orc.fr_from_repr(rand_fr_canonical(seed, lanes * n)).reshape(lanes, n, 4)


def _lane_consts(D, orc):
    """w^j as one Montgomery element per party"""
    return M.to_limbs([[p] for p in D.points])


def _sharing(orc, D, secret, slope):
    """lane j = secret + slope w^j: a degree-1 sharing of every element of `secret` ((n, 4) Montgomery limbs) by the checker's vector ops"""
    n = secret.shape[0]
    return np.stack([orc.fr_add(secret, orc.fr_mul(slope, np.tile(w, (n, 1)))) for w in _lane_consts(D, orc)])


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_tails_and_footprints_of_the_product_kernels(ctx, orc, which):
    """k_gsz_mul (through batch_mul, and its opening form through batch_inv, whose last step is k_share_scale) at the sizes around the second trip of
    the grid-stride loop, inside guard bands: pads intact, inputs unchanged, values by the checker's vector ops.  Random lanes are no sharings of
    anything: with 4 parties every element violates the king's bound and the open's."""
    import guarded
    from guarded import Guards
    T = guarded.grid_threads(_per_cu_blocks())
    parties, t, n = 4, 1, [T - 1, T + 3][which]
    G = Guards("cuda")
    v = {k: _rand_lanes(11 + j, parties, n, orc) for j, k in enumerate(("x", "y", "dr", "dr2"))}
    f = {k: G.freeze(a.reshape(parties * n, 4), k) for k, a in v.items()}
    out = G.out(parties, n)
    bad, zero = ctx.gsz_share_batch_mul(parties, t, f["x"].ptr, f["y"].ptr, f["dr"].ptr, f["dr2"].ptr, out.ptr, n)
    val, vbad = orc.gsz_open(np.stack([orc.fr_add(orc.fr_mul(v["x"][j], v["y"][j]), v["dr2"][j]) for j in range(parties)]), degree=2 * t)
    want = np.stack([orc.fr_sub(val, v["dr"][j]) for j in range(parties)])
    assert np.array_equal(G.check()[0], want) and (bad, zero) == (vbad, 0) == (n, 0)
    # batch_inv: out_j * open(x rs) = rs_j on every lane (y plays rs)
    G2 = Guards("cuda")
    f = {k: G2.freeze(a.reshape(parties * n, 4), k) for k, a in v.items()}
    out = G2.out(parties, n)
    bad, zero = ctx.gsz_share_batch_inv(parties, t, f["x"].ptr, f["dr"].ptr, f["dr2"].ptr, f["y"].ptr, out.ptr, n)
    got = G2.check()[0]
    opened, obad = orc.gsz_open(want, degree=t)
    assert (bad, zero) == (vbad + obad, 0) == (2 * n, 0)
    for j in range(parties):
        assert np.array_equal(orc.fr_mul(got[j], opened), v["y"][j]), j


@pytest.mark.gpu
@pytest.mark.parametrize("n", [512, 513, 514, "T-1", "T+3", "2T+5"])
def test_tails_of_the_check_kernels(ctx, orc, n):
    """The check's kernels either side of one block's worth of k_gsz_ip partials (half lengths 256 and 257), of the second trip of k_gsz_hadamard's loop
    (T - 1, T + 3) and of k_gsz_ip's and k_gsz_fold's (half length T + 3): honest degree-1 sharings at 3 parties built with the checker's vector ops
    pass, a wrong product in the LAST triple -- the element a short loop would drop -- or in the first of the second trip fails; inputs unchanged."""
    import guarded
    from guarded import Guards
    T = guarded.grid_threads(_per_cu_blocks())
    n = {"T-1": T - 1, "T+3": T + 3, "2T+5": 2 * T + 5}.get(n, n)
    D, t = _domain(3), 1
    sec = {k: _rand_lanes(51 + j, 1, n, orc)[0] for j, k in enumerate(("x", "y", "sx", "sy", "sz"))}
    x, y = _sharing(orc, D, sec["x"], sec["sx"]), _sharing(orc, D, sec["y"], sec["sy"])
    z = _sharing(orc, D, orc.fr_mul(sec["x"], sec["y"]), sec["sz"])
    src = M.random_material(D, t, M.OP_PRODUCT_CHECK, n, seed=n)
    G = Guards("cuda")
    f = {k: G.freeze(a.reshape(-1, 4), k) for k, a in (("xs", x), ("ys", y), ("zs", z), ("dr", M.to_limbs(src.dr)), ("dr2", M.to_limbs(src.dr2)),
                                                         ("rands", M.to_limbs(src.rands)))}
    d = {k: v.t for k, v in f.items()}
    assert _run_check(ctx, 3, n, None, d) == (True, 0)
    G.check()
    one = M.to_limbs(D.share([1], t, random.Random(3)))             # a consistent sharing of 1
    for at in sorted({n - 1, min(T, n - 1)}):
        zt = _dev(z)
        zt[:, at] = _dev(np.stack([orc.fr_add(z[j, at], one[j, 0]) for j in range(3)]))
        assert _run_check(ctx, 3, n, None, dict(d, zs=zt)) == (False, 0), at


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_rules(ctx):
    import torch
    import czk_amd
    from guarded import Guards
    G = Guards("cuda")
    out = G.out(4, 8)
    buf = torch.zeros((4 * 64, 4), dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    calls = {"mul": lambda parties, q, o, n: ctx.gsz_share_batch_mul(parties, 1, q, q, q, q, o, n),
             "inv": lambda parties, q, o, n: ctx.gsz_share_batch_inv(parties, 1, q, q, q, q, o, n),
             "pp": lambda parties, q, o, n: ctx.gsz_share_partial_products(parties, 1, q, q, q, q, o, n)}
    for name, call in calls.items():
        assert call(4, p, out.ptr, 0) == (0, 0) and call(4, None, None, 0) == (0, 0)                    # nothing to do: CZK_OK whatever the pointers
        assert out.untouched(), name
        for args in ((4, None, out.ptr, 8), (4, p, None, 8)):                                           # null vector / output with work to do
            with pytest.raises(czk_amd.CzkError) as e:
                call(*args)
            assert e.value.code == 3, (name, args)
        for args in ((5, p, out.ptr, 8), (7, p, out.ptr, 0), (0, p, out.ptr, 8), (97, p, out.ptr, 8), (128, p, out.ptr, 8),   # no share domain; above 96
                     (4, p, out.ptr, 1 << 60)):                                                         # lanes x n x 32 bytes overflows
            with pytest.raises(czk_amd.CzkError) as e:
                call(*args)
            assert e.value.code == 1, (name, args)
        assert out.untouched(), name
    assert ctx.gsz_product_check(4, 1, None, None, None, 0, None, None, None) == (True, 0)              # no triples: nothing to refute
    for parties, q, n, code in ((4, None, 8, 3), (5, p, 8, 1), (97, p, 8, 1), (4, p, 1 << 60, 1)):
        with pytest.raises(czk_amd.CzkError) as e:
            ctx.gsz_product_check(parties, 1, q, q, q, n, q, q, q)
        assert e.value.code == code, (parties, n)
    for op in (0, 1, 2, 3):
        with pytest.raises(czk_amd.CzkError) as e:
            ctx.gsz_material_counts(op, 1 << 60)
        assert e.value.code == 1
    with pytest.raises(czk_amd.CzkError) as e:
        ctx.gsz_material_counts(4, 8)
    assert e.value.code == 3
    assert ctx.gsz_material_counts(M.OP_PRODUCT_CHECK, 0) == (0, 0) and ctx.gsz_material_counts(M.OP_PARTIAL_PRODUCTS, 0) == (0, 0)
