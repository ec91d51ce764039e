"""czk_share_batch_mul / batch_inv / partial_products and their czk_net_share_* twins (csrc/share_mul.hip, include/czk.h) against the big-integer
model of the reference's formulas (tests/share_mul_model.py): every output lane limb for limb, the two counts, where the kernels write and how their
grid-stride loops end, tampered MACs, the one-party-per-process form over CZK_NET_SHM, and the argument rules."""
import functools
import os
import random
import re
import sys

import numpy as np
import pytest

import share_mul_model as M
from share_mul_model import R_MOD, Scheme
from util import rand_fr_canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = {"mul": M.OP_MUL, "inv": M.OP_INV, "pp": M.OP_PARTIAL_PRODUCTS}
CONFIGS = [(lpp, parties) for lpp in (1, 2) for parties in (1, 2, 3)]


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def _scheme(lpp, parties):
    rng = random.Random(1000 * lpp + parties)
    return Scheme(lpp, parties, [rng.randrange(R_MOD) for _ in range(parties)] if lpp == 2 else None)   # a random MAC key, split across the parties


@functools.lru_cache(maxsize=None)
def _case(lpp, parties, op, n, zero_at=None):
    """One call's inputs and the model's outputs, computed once and shared (never modified: tests copy what they change).
    -> dict of (lanes, k, 4) uint64 limb arrays x, y, pb, pc, tx, ty, tz, want + mac (parties, 4) + bad, zero"""
    S = _scheme(lpp, parties)
    rng = random.Random(7 * n + op)
    xv = [rng.randrange(1, R_MOD) for _ in range(n)]
    if zero_at is not None:
        xv[zero_at] = 0
    x, y = S.share(xv, rng), S.share([rng.randrange(R_MOD) for _ in range(n)], rng)
    src = M.random_material(S, op, n, seed=n + 17 * op)
    if op == M.OP_MUL:
        want, bad = M.batch_mul(S, x, y, src)
        zero = 0
    elif op == M.OP_INV:
        want, bad, zero = M.batch_inv(S, x, src)
    else:
        want, bad, zero = M.partial_products(S, x, src)
    assert (src.t, src.p) == M.material_counts(op, n)
    c = {k: M.to_limbs(v) for k, v in (("x", x), ("y", y), ("pb", src.pb), ("pc", src.pc), ("tx", src.tx), ("ty", src.ty), ("tz", src.tz), ("want", want))}
    c.update(mac=M.to_limbs([S.mac_shares])[0], bad=bad, zero=zero, opened=S.opened(want))
    return c


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _run_lanes(ctx, lpp, parties, op, n, c, d=None, out=None):
    """one lanes-form call on device copies of the case's arrays (d: already uploaded / tampered ones) -> (limbs, bad, zero)"""
    import torch
    d = dict(d or {})
    for k in ("x", "y", "pb", "pc", "tx", "ty", "tz"):
        if k not in d:
            d[k] = _dev(c[k])
    if out is None:
        out = torch.empty((lpp * parties, n, 4), dtype=torch.int64, device="cuda")
    mac = c["mac"] if lpp == 2 else None
    p = {k: v.data_ptr() for k, v in d.items()}
    if op == M.OP_MUL:
        bad, zero = ctx.share_batch_mul(lpp, parties, mac, p["x"], p["y"], p["tx"], p["ty"], p["tz"], out.data_ptr(), n)
    else:
        fn = ctx.share_batch_inv if op == M.OP_INV else ctx.share_partial_products
        bad, zero = fn(lpp, parties, mac, p["x"], p["pb"], p["pc"], p["tx"], p["ty"], p["tz"], out.data_ptr(), n)
    return out.cpu().numpy().view(np.uint64), bad, zero


# ---- lanes form, bit-exact ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 1025])            # either side of the scan's 32-element segment and of a block
@pytest.mark.parametrize("lpp,parties", CONFIGS)
def test_lanes_form_equals_the_model_limb_for_limb(ctx, lpp, parties, n):
    for name, op in OPS.items():
        c = _case(lpp, parties, op, n)
        assert ctx.share_material_counts(op, n) == M.material_counts(op, n)
        got, bad, zero = _run_lanes(ctx, lpp, parties, op, n, c)
        assert (bad, zero) == (c["bad"], c["zero"]) == (0, 0), name
        assert np.array_equal(got, c["want"]), (name, "first differing lane", int(np.argwhere((got != c["want"]).any(axis=(1, 2)))[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("lpp,parties", [(1, 3), (2, 2)])
def test_zero_divisors_are_counted_and_a_zero_factor_is_not_one(ctx, lpp, parties):
    n = 33
    c = _case(lpp, parties, M.OP_INV, n, zero_at=20)
    got, bad, zero = _run_lanes(ctx, lpp, parties, M.OP_INV, n, c)
    assert (bad, zero) == (0, 1) == (c["bad"], c["zero"]) and np.array_equal(got, c["want"])
    assert not got[:, 20].any() and got[:, 19].any()               # the element's share is zero on every lane
    c = _case(lpp, parties, M.OP_PARTIAL_PRODUCTS, n, zero_at=20)
    got, bad, zero = _run_lanes(ctx, lpp, parties, M.OP_PARTIAL_PRODUCTS, n, c)
    assert (bad, zero) == (0, 0) and np.array_equal(got, c["want"])
    assert all(c["opened"][:20]) and c["opened"][20:] == [0] * (n - 20)   # later running products open to zero: no error


# ---- tail and footprint ------------------------------------------------------------------------------------------------------------------------
def _per_cu_blocks():
    """blocks per CU that cap the grids of share_mul.hip, on blocks of 256 threads (tests/test_guarded_cpu.py reads the other files' caps the same way)"""
    src = open(os.path.join(ROOT, "collaborative-zksnark_amd", "csrc", "share_mul.hip")).read()
    m = re.search(r"constexpr size_t SHARE_MUL_BLOCKS_PER_CU = (\d+);", src)
    assert m and "const size_t cap = SHARE_MUL_BLOCKS_PER_CU * (size_t)ctx->num_cu;" in src and "size_t blocks = (n + 255) / 256;" in src
    for k in ("k_share_mul<LN>", "k_share_mul<0>", "k_share_mask", "k_share_combine", "k_share_scale"):
        assert re.search(rf"hipLaunchKernelGGL\({re.escape(k)}, (g, b|dim3\(share_mul_grid\(ctx, n\)\), dim3\(256\))", src), k
    return int(m.group(1))


def test_grid_cap_is_where_the_test_reads_it():
    assert _per_cu_blocks() == 8


def _tail_sizes():
    import guarded
    t = guarded.grid_threads(_per_cu_blocks())
    return [t - 1, t + 3]                                           # the last size of one trip, and three elements into the second


def _rand_lanes(seed, lanes, n, orc):
    return orc.fr_from_repr(rand_fr_canonical(seed, lanes * n)).reshape(lanes, n, 4)


def _orc_batch_mul(orc, lpp, parties, mac, x, y, tx, ty, tz):
    """the reference's batch_mul on (lanes, n, 4) Montgomery limb arrays with the checker's vector ops -> (shares, opened product)"""
    n = x.shape[1]
    sh = range(0, lpp * parties, lpp)
    sx, oy = np.zeros((n, 4), np.uint64), np.zeros((n, 4), np.uint64)
    for ln in sh:
        sx = orc.fr_add(sx, orc.fr_add(x[ln], tx[ln]))
        oy = orc.fr_add(oy, orc.fr_add(y[ln], ty[ln]))
    open_ = orc.fr_mul(sx, oy)
    out = np.empty_like(tz)
    for ln in range(lpp * parties):
        r = orc.fr_sub(orc.fr_sub(tz[ln], orc.fr_mul(ty[ln], sx)), orc.fr_mul(tx[ln], oy))
        if ln == 0:
            r = orc.fr_add(r, open_)
        if lpp == 2 and ln & 1:
            r = orc.fr_add(r, orc.fr_mul(np.tile(mac[ln >> 1], (n, 1)), open_))
        out[ln] = r
    val = np.zeros((n, 4), np.uint64)
    for ln in sh:
        val = orc.fr_add(val, out[ln])
    return out, val


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_tails_and_footprints_of_the_lanes_form_kernels(ctx, orc, which):
    """k_share_mul (through batch_mul) and k_share_scale (through batch_inv) at the sizes around the second trip of their grid-stride loops, inside
    guard bands: pads intact, inputs unchanged, values by the checker's vector ops.  Random lanes are no valid MACs: every opened element is counted."""
    from guarded import Guards
    lpp, parties, n = 2, 2, _tail_sizes()[which]
    L = lpp * parties
    mac = orc.fr_from_repr(rand_fr_canonical(5, parties))
    G = Guards("cuda")
    v = {k: _rand_lanes(11 + j, L, n, orc) for j, k in enumerate(("x", "y", "tx", "ty", "tz"))}
    f = {k: G.freeze(a.reshape(L * n, 4), k) for k, a in v.items()}
    out = G.out(L, n)
    bad, zero = ctx.share_batch_mul(lpp, parties, mac, f["x"].ptr, f["y"].ptr, f["tx"].ptr, f["ty"].ptr, f["tz"].ptr, out.ptr, n)
    want, val = _orc_batch_mul(orc, lpp, parties, mac, v["x"], v["y"], v["tx"], v["ty"], v["tz"])
    assert np.array_equal(G.check()[0], want) and (bad, zero) == (2 * n, 0)
    # batch_inv: out_l * open(x b) = c_l on every lane (y plays b; c is one more random vector)
    G2 = Guards("cuda")
    c = _rand_lanes(31, L, n, orc)
    f = {k: G2.freeze(a.reshape(L * n, 4), k) for k, a in list(v.items()) + [("c", c)]}
    out = G2.out(L, n)
    bad, zero = ctx.share_batch_inv(lpp, parties, mac, f["x"].ptr, f["y"].ptr, f["c"].ptr, f["tx"].ptr, f["ty"].ptr, f["tz"].ptr, out.ptr, n)
    got = G2.check()[0]
    assert (bad, zero) == (3 * n, 0)
    for ln in range(L):
        assert np.array_equal(orc.fr_mul(got[ln], val), c[ln]), ln


@pytest.mark.gpu
def test_tails_and_footprints_of_the_net_form_kernels(orc):
    """k_share_mask and k_share_combine, which only the one-party-per-communicator form launches, three elements into the second trip: a world of one
    over CZK_NET_SHM (every exchange is a local copy) must give the lanes form's values for one party."""
    import czk_amd
    from guarded import Guards
    c = czk_amd.Context(0)
    net = czk_amd.Net(c, czk_amd.CZK_NET_SHM, 0, 1, os.urandom(16), options={"timeout_ms": 60000})
    try:
        for n in _tail_sizes():
            mac = orc.fr_from_repr(rand_fr_canonical(6, 1))
            G = Guards("cuda")
            v = {k: _rand_lanes(41 + j, 2, n, orc) for j, k in enumerate(("x", "y", "tx", "ty", "tz"))}
            f = {k: G.freeze(a.reshape(2 * n, 4), k) for k, a in v.items()}
            out = G.out(2, n)
            bad, zero = net.share_batch_mul(2, mac[0], f["x"].ptr, f["y"].ptr, f["tx"].ptr, f["ty"].ptr, f["tz"].ptr, out.ptr, n, commit=False)
            want, _ = _orc_batch_mul(orc, 2, 1, mac, v["x"], v["y"], v["tx"], v["ty"], v["tz"])
            assert np.array_equal(G.check()[0], want) and (bad, zero) == (2 * n, 0)
    finally:
        net.close()
        c.close()


# ---- tampering -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", ["mul", "inv", "pp"])
def test_a_flipped_limb_is_caught_under_spdz_and_not_under_additive_shares(ctx, op):
    n, parties = 33, 2
    for lpp in (2, 1):
        c = _case(lpp, parties, OPS[op], n)
        operand = "x"
        triple = "ty"
        flips = [(operand, lpp * 1 + lpp - 1), (triple, lpp * 1 + lpp - 1), (operand, lpp * 1), (triple, lpp * 1)]   # party 1: mac lanes, then sh lanes
        for name, lane in flips:
            t = _dev(c[name])
            t[lane, 5, 2] ^= 1 << 7
            got, bad, zero = _run_lanes(ctx, lpp, parties, OPS[op], n, c, {name: t})
            if lpp == 2:
                assert bad >= 1, (op, name, lane)
            else:
                # additive shares carry no MAC: the flip is NOT caught, the call just computes with the changed share
                assert bad == 0 and not np.array_equal(got, c["want"]), (op, name, lane)


# ---- one party per process -------------------------------------------------------------------------------------------------------------------------
def _net_worker(rank, world, q, idb, lpp, commit, tamper):
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import czk_amd
    torch.cuda.set_device(0)
    c = czk_amd.Context(0)
    net = czk_amd.Net(c, czk_amd.CZK_NET_SHM, rank, world, idb, options={"timeout_ms": 60000})
    n, fails, bads = 33, [], []
    mine = slice(lpp * rank, lpp * rank + lpp)
    for name, op in OPS.items():
        case = _case(lpp, world, op, n)
        d = {k: _dev(case[k][mine]) for k in ("x", "y", "pb", "pc", "tx", "ty", "tz")}
        if tamper and rank == world - 1 and lpp == 2:
            d["x"][1, 7, 0] ^= 1                                    # this party's mac lane of the operand
        out = torch.empty((lpp, n, 4), dtype=torch.int64, device="cuda")
        p = {k: v.data_ptr() for k, v in d.items()}
        mac = case["mac"][rank] if lpp == 2 else None
        net.stats_reset()
        if op == M.OP_MUL:
            bad, zero = net.share_batch_mul(lpp, mac, p["x"], p["y"], p["tx"], p["ty"], p["tz"], out.data_ptr(), n, commit=commit)
            # ONE open of 2 n elements: one broadcast (additive) or two (SPDZ: sh, then dx), half of what the reference's two opens count
            if commit is False and net.stats()["broadcasts"] != (1 if lpp == 1 else 2):
                fails.append((name, "broadcasts", net.stats()))
        else:
            fn = net.share_batch_inv if op == M.OP_INV else net.share_partial_products
            bad, zero = fn(lpp, mac, p["x"], p["pb"], p["pc"], p["tx"], p["ty"], p["tz"], out.data_ptr(), n, commit=commit)
        bads.append(bad)
        if not tamper and ((bad, zero) != (0, 0) or not np.array_equal(out.cpu().numpy().view(np.uint64), case["want"][mine])):
            fails.append((name, bad, zero))
    net.barrier()
    net.close()
    c.close()
    q.put((rank, fails, bads))


@pytest.mark.gpu
@pytest.mark.parametrize("world,lpp,commit", [(2, 2, False), (3, 2, "tree"), (3, 1, False), (2, 2, True)])
def test_net_form_gives_every_party_the_models_lanes(ctx, world, lpp, commit):
    """2 and 3 processes on one GPU over CZK_NET_SHM, n = 33: each party's output lanes are the model's for that party -- which the lanes form
    equals too (checked here on the same case) -- with the plain, the SHA-256 and the tree commit round"""
    from test_net import _spawn
    for op in OPS.values():
        c = _case(lpp, world, op, 33)
        assert np.array_equal(_run_lanes(ctx, lpp, world, op, 33, c)[0], c["want"])
    res = _spawn(_net_worker, world, os.urandom(16), lpp, commit, False, timeout=120)
    assert res == [(r, [], [0, 0, 0]) for r in range(world)]


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_net_form_every_rank_sees_a_tampered_mac(world):
    from test_net import _spawn
    res = _spawn(_net_worker, world, os.urandom(16), 2, False, True, timeout=120)
    assert [r for r, _, _ in res] == list(range(world))
    for _, fails, bads in res:
        assert fails == [] and all(b >= 1 for b in bads), res


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_rules(ctx):
    import torch
    import czk_amd
    from guarded import Guards
    G = Guards("cuda")
    out = G.out(4, 8)
    buf = torch.zeros((4 * 40, 4), dtype=torch.int64, device="cuda")
    p, mac = buf.data_ptr(), np.zeros((2, 4), np.uint64)
    calls = {"mul": lambda lpp, parties, m, q, o, n: ctx.share_batch_mul(lpp, parties, m, q, q, q, q, q, o, n),
             "inv": lambda lpp, parties, m, q, o, n: ctx.share_batch_inv(lpp, parties, m, q, q, q, q, q, q, o, n),
             "pp": lambda lpp, parties, m, q, o, n: ctx.share_partial_products(lpp, parties, m, q, q, q, q, q, q, o, n)}
    for name, call in calls.items():
        assert call(2, 2, mac, p, out.ptr, 0) == (0, 0) and call(2, 0, mac, p, out.ptr, 8) == (0, 0)      # nothing to do: CZK_OK ...
        assert call(2, 2, None, None, None, 0) == (0, 0)                                                   # ... whatever the pointers
        assert out.untouched(), name                                                                       # ... and nothing touched
        for args in ((2, 2, mac, None, out.ptr, 8), (2, 2, mac, p, None, 8), (2, 2, None, p, out.ptr, 8),  # null vector / output / MAC key with work to do
                     (3, 2, mac, p, out.ptr, 8), (0, 2, mac, p, out.ptr, 8), (1, 33, None, p, out.ptr, 8)):  # lpp not 1 or 2; more than 32 parties
            with pytest.raises(czk_amd.CzkError) as e:
                call(*args)
            assert e.value.code == 3, (name, args)
        with pytest.raises(czk_amd.CzkError) as e:
            call(2, 2, mac, p, out.ptr, 1 << 60)                                                           # lanes x n x 32 bytes overflows
        assert e.value.code == 1, name
        assert out.untouched(), name
    out2 = torch.empty((2, 8, 4), dtype=torch.int64, device="cuda")
    assert calls["mul"](1, 2, None, p, out2.data_ptr(), 8) == (0, 0)                                       # additive shares need no key
    for op in OPS.values():
        with pytest.raises(czk_amd.CzkError) as e:
            ctx.share_material_counts(op, 1 << 60)
        assert e.value.code == 1
    with pytest.raises(czk_amd.CzkError) as e:
        ctx.share_material_counts(3, 8)
    assert e.value.code == 3
    # the net form: same rules, on a world of one
    net = czk_amd.Net(ctx, czk_amd.CZK_NET_SHM, 0, 1, os.urandom(16))
    try:
        m1 = np.zeros(4, np.uint64)
        assert net.share_batch_mul(2, m1, None, None, None, None, None, None, 0, commit=False) == (0, 0)
        for lpp, m, q, o, n, code in ((2, m1, None, out.ptr, 8, 3), (2, m1, p, None, 8, 3), (2, None, p, out.ptr, 8, 3), (3, m1, p, out.ptr, 8, 3),
                                      (2, m1, p, out.ptr, 1 << 60, 1)):
            for call in (lambda: net.share_batch_mul(lpp, m, q, q, q, q, q, o, n, commit=False),
                         lambda: net.share_batch_inv(lpp, m, q, q, q, q, q, q, o, n, commit=False),
                         lambda: net.share_partial_products(lpp, m, q, q, q, q, q, q, o, n, commit=False)):
                with pytest.raises(czk_amd.CzkError) as e:
                    call()
                assert e.value.code == code
        assert out.untouched()
    finally:
        net.close()
