"""czk_net_gsz_share_batch_mul / _batch_inv / _partial_products and czk_net_gsz_product_check (csrc/net_rounds.hip, kernels in csrc/gsz_mul.hip): the GSZ
products and their product check with ONE PARTY PER PROCESS, 3 and 4 processes sharing the GPU over CZK_NET_SHM.  Every rank's output is its lane of
the big-integer model (tests/gsz_mul_model.py), which the lanes form equals on the same case; the verdict is the same on every rank; the exchanges are
the ones include/czk.h counts; a cheating party is seen by the king's bound at 4 parties and only by the check at 3; tails and write footprints on a
world of one; the argument rules.  Sizes are looped over INSIDE a spawn: starting the processes is what takes the time."""
import os
import sys

import numpy as np
import pytest

import gsz_mul_model as M
from gsz_mul_model import R_MOD
from test_gsz_mul import OPS, _case, _check_case, _dev, _domain, _per_cu_blocks, _rand_lanes, _run, _run_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_SIZES = (1, 2, 33)
CHECK_SIZES = (1, 2, 3, 5, 33, 1025)                                 # odd lengths at every halving level; 1025: several blocks of partials
EXCHANGES = {"mul": (1, 1, 0), "inv": (1, 1, 1), "pp": (5, 5, 3)}    # (to_king, from_king, broadcasts), include/czk.h


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def _exchanges(net):
    s = net.stats()
    return s["to_king"], s["from_king"], s["broadcasts"]


def _mine(c, rank, keys):
    """this rank's lane of the case's arrays, on the device"""
    return {k: _dev(c[k][rank]) for k in keys}


def _product(net, op, t, d, n):
    """one net-form product call on this party's lanes `d` -> (limbs, bad, zero)"""
    import torch
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items()}
    if op == M.OP_MUL:
        bad, zero = net.gsz_share_batch_mul(t, p["x"], p["y"], p["dr"], p["dr2"], out.data_ptr(), n)
    else:
        fn = net.gsz_share_batch_inv if op == M.OP_INV else net.gsz_share_partial_products
        bad, zero = fn(t, p["x"], p["dr"], p["dr2"], p["rands"], out.data_ptr(), n)
    return out.cpu().numpy().view(np.uint64), bad, zero


def _check(net, t, d, n):
    p = {k: v.data_ptr() for k, v in d.items()}
    return net.gsz_product_check(t, p["xs"], p["ys"], p["zs"], n, p["dr"], p["dr2"], p["rands"])


# ---- what the parties do, one function per test (run in every spawned process) -----------------------------------------------------------------------
def _s_products(net, rank, world, fails):
    t = M.threshold(world)
    for name, op in OPS.items():
        for n in PRODUCT_SIZES:
            c = _case(world, op, n)
            net.stats_reset()
            got, bad, zero = _product(net, op, t, _mine(c, rank, ("x", "y", "dr", "dr2", "rands")), n)
            if (bad, zero) != (0, 0) or not np.array_equal(got, c["want"][rank]):
                fails.append((name, n, bad, zero))
            if _exchanges(net) != EXCHANGES[name]:
                fails.append((name, n, net.stats()))


def _s_check(net, rank, world, fails):
    import torch
    t = M.threshold(world)
    for n in CHECK_SIZES:
        R = M.ceil_log2(n)
        for wrong in (False, True):
            d = _mine(_check_case(world, n, wrong_z=wrong), rank, ("xs", "ys", "zs", "dr", "dr2", "rands"))
            keep = {k: d[k].clone() for k in ("xs", "ys", "zs")}
            net.stats_reset()
            ok, bad = _check(net, t, d, n)
            if (ok, bad) != (not wrong, 0):
                fails.append((n, wrong, ok, bad))
            if _exchanges(net) != (R + 2, R + 2, R + 2):
                fails.append((n, wrong, net.stats()))
            if not all(torch.equal(d[k], keep[k]) for k in keep):
                fails.append((n, wrong, "inputs modified"))


def _s_cheat(net, rank, world, fails):
    """rank 1 adds 1 to element 5 of its x share before batch_mul -> (bad, outputs differ from the model's, the check's (ok, bad) at world 3)"""
    n, t = 33, M.threshold(world)
    c = _case(world, M.OP_MUL, n)
    d = _mine(c, rank, ("x", "y", "dr", "dr2", "rands"))
    honest_x = d["x"].clone()
    if rank == 1:
        x = M.from_limbs(c["x"][rank:rank + 1])
        x[0][5] = (x[0][5] + 1) % R_MOD
        d["x"] = _dev(M.to_limbs(x)[0])
    got, bad, zero = _product(net, M.OP_MUL, t, d, n)
    info = [bad, zero, bool(np.array_equal(got, c["want"][rank])), bool(np.array_equal(np.delete(got, 5, axis=0), np.delete(c["want"][rank], 5, axis=0)))]
    if world == 3:
        src = M.random_material(_domain(3), t, M.OP_PRODUCT_CHECK, n, seed=77)
        cc = {"xs": honest_x, "ys": d["y"], "zs": _dev(got)}
        cc.update({k: _dev(M.to_limbs([v[rank]])[0]) for k, v in (("dr", src.dr), ("dr2", src.dr2), ("rands", src.rands))})
        info.append(_check(net, t, cc, n))
        cc["zs"] = _dev(c["want"][rank])                             # the honest product passes on the same material
        info.append(_check(net, t, cc, n))
    return info


def _s_zero(net, rank, world, fails):
    n = 33
    c = _case(world, M.OP_INV, n, zero_at=20)
    got, bad, zero = _product(net, M.OP_INV, M.threshold(world), _mine(c, rank, ("x", "y", "dr", "dr2", "rands")), n)
    return [bad, zero, bool(got[20].any()), bool(got[19].any()), bool(np.array_equal(got, c["want"][rank]))]


SCENARIOS = {f.__name__: f for f in (_s_products, _s_check, _s_cheat, _s_zero)}


def _party(rank, world, q, idb, scenario):
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import czk_amd
    torch.cuda.set_device(0)
    c = czk_amd.Context(0)
    net = czk_amd.Net(c, czk_amd.CZK_NET_SHM, rank, world, idb, options={"timeout_ms": 60000})
    fails = []
    info = SCENARIOS[scenario](net, rank, world, fails)
    net.barrier()
    net.close()
    c.close()
    q.put((rank, fails, info))


def _parties(world, scenario):
    from test_net import _spawn
    res = _spawn(_party, world, os.urandom(16), scenario.__name__, timeout=120)
    assert [r for r, _, _ in res] == list(range(world))
    return res


# ---- 1: every party gets its lane ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world", [3, 4])
def test_every_party_gets_its_lane_of_the_model(ctx, world):
    """n = 1, 2, 33 for the three products: rank j's output is the model's lane j with no violation and no zero divisor, after the exchanges czk.h counts;
    the lanes form -- existing code -- equals the model on the same cases (checked here first)"""
    for op in OPS.values():
        for n in PRODUCT_SIZES:
            c = _case(world, op, n)
            got, bad, zero = _run(ctx, world, op, n, c)
            assert (bad, zero) == (0, 0) and np.array_equal(got, c["want"]), (op, n)
    for rank, fails, _ in _parties(world, _s_products):
        assert fails == [], (rank, fails)


# ---- 2: the check ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world", [3, 4])
def test_the_check_gives_every_rank_the_verdict_in_the_documented_exchanges(world):
    """honest triples: (ok, bad) = (1, 0) on every rank; a wrong last z: ok = 0 on every rank; R + 2 broadcasts, to_king and from_king each; xs, ys, zs
    unchanged"""
    for n in CHECK_SIZES:
        assert _check_case(world, n)["ok"] is True and _check_case(world, n, wrong_z=True)["ok"] is False      # what the model says of the same cases
    for rank, fails, _ in _parties(world, _s_check):
        assert fails == [], (rank, fails)


# ---- 3: a cheating party ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_king_sees_a_cheating_party_at_4_parties():
    res = _parties(4, _s_cheat)
    assert res[0][2][0] >= 1, res                                    # the king's bound 2 t = 2 < n - 1 = 3
    assert all(info[1] == 0 for _, _, info in res)


@pytest.mark.gpu
def test_only_the_check_sees_a_cheating_party_at_3_parties():
    """2 t = n - 1: every contribution passes the king's bound, the product comes out wrong at element 5 alone, and the product check over the honest
    (x, y) and that z fails on every rank (the honest z passes on the same material)"""
    for rank, _, (bad, zero, equal, equal_elsewhere, cheated, honest) in _parties(3, _s_cheat):
        assert (bad, zero) == (0, 0) and not equal and equal_elsewhere, rank
        assert cheated == (False, 0) and honest == (True, 0), rank


# ---- 4: zero divisor -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_zero_divisor_is_counted_on_every_rank_and_its_output_is_zero():
    c = _case(3, M.OP_INV, 33, zero_at=20)
    assert (c["bad"], c["zero"]) == (0, 1)
    for rank, _, info in _parties(3, _s_zero):
        assert info == [0, 1, False, True, True], (rank, info)


# ---- 5: tails and write footprint, one process, a world of one -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net1(ctx):
    import czk_amd
    net = czk_amd.Net(ctx, czk_amd.CZK_NET_SHM, 0, 1, os.urandom(16))
    yield net
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_tails_and_footprints_of_the_party_kernels(ctx, net1, orc, which):
    """k_gsz_net_mask / k_gsz_net_unmask (and k_gsz_open, k_share_scale behind batch_inv) either side of the second trip of their grid-stride loops, inside
    guard bands, on a world of one -- every exchange is a local copy there, and every kernel of the party and of the king runs as in a larger world (the
    chunked staging of larger worlds is tests/test_net.py's): pads intact, inputs unchanged, values those of the lanes form with parties = 1 on the same
    buffers and, for batch_mul, of the checker's vector ops"""
    import guarded
    from guarded import Guards
    T = guarded.grid_threads(_per_cu_blocks())
    n = [T - 1, T + 3][which]
    G = Guards("cuda")
    v = {k: _rand_lanes(21 + j, 1, n, orc)[0] for j, k in enumerate(("x", "y", "dr", "dr2"))}
    f = {k: G.freeze(a, k) for k, a in v.items()}
    out, ref = G.out(1, n, name="net"), G.out(1, n, name="lanes")
    assert net1.gsz_share_batch_mul(0, f["x"].ptr, f["y"].ptr, f["dr"].ptr, f["dr2"].ptr, out.ptr, n) == (0, 0)
    assert ctx.gsz_share_batch_mul(1, 0, f["x"].ptr, f["y"].ptr, f["dr"].ptr, f["dr2"].ptr, ref.ptr, n) == (0, 0)
    got, want = G.check()
    assert np.array_equal(got, want) and np.array_equal(got[0], orc.fr_sub(orc.fr_add(orc.fr_mul(v["x"], v["y"]), v["dr2"]), v["dr"]))
    G2 = Guards("cuda")
    f = {k: G2.freeze(a, k) for k, a in v.items()}
    out, ref = G2.out(1, n, name="net"), G2.out(1, n, name="lanes")
    assert net1.gsz_share_batch_inv(0, f["x"].ptr, f["dr"].ptr, f["dr2"].ptr, f["y"].ptr, out.ptr, n) == (0, 0)           # y plays rs
    assert ctx.gsz_share_batch_inv(1, 0, f["x"].ptr, f["dr"].ptr, f["dr2"].ptr, f["y"].ptr, ref.ptr, n) == (0, 0)
    got, want = G2.check()
    assert np.array_equal(got, want) and got[0, -1].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [513, "T+3", "2T+5"])
def test_tails_of_the_check_on_one_lane(ctx, net1, orc, n):
    """The one-lane instantiations of k_gsz_hadamard, k_gsz_ip and k_gsz_fold and the single-block party kernels around one block of partials (half
    length 257) and the second trip of the loops (T + 3; half length T + 3), on a world of one: honest triples pass, a wrong product in the LAST triple
    or in the first of the second trip fails, as in the lanes form with parties = 1 on the same buffers; inputs unchanged"""
    import guarded
    from guarded import Guards
    T = guarded.grid_threads(_per_cu_blocks())
    n = {"T+3": T + 3, "2T+5": 2 * T + 5}.get(n, n)
    x, y = _rand_lanes(61, 1, n, orc)[0], _rand_lanes(62, 1, n, orc)[0]
    z = orc.fr_mul(x, y)                                             # one party, degree 0: a share is the value
    src = M.random_material(_domain(1), 0, M.OP_PRODUCT_CHECK, n, seed=n)
    G = Guards("cuda")
    f = {k: G.freeze(a, k) for k, a in (("xs", x), ("ys", y), ("zs", z), ("dr", M.to_limbs(src.dr)[0]), ("dr2", M.to_limbs(src.dr2)[0]),
                                        ("rands", M.to_limbs(src.rands)[0]))}
    d = {k: v.t for k, v in f.items()}
    assert _check(net1, 0, d, n) == (True, 0) == _run_check(ctx, 1, n, None, d)
    G.check()
    one = M.to_limbs([[1]])[0, 0]
    for at in sorted({n - 1, min(T, n - 1)}):
        zt = _dev(z)
        zt[at] = _dev(orc.fr_add(z[at:at + 1], one[None])[0])
        assert _check(net1, 0, dict(d, zs=zt), n) == (False, 0) == _run_check(ctx, 1, n, None, dict(d, zs=zt)), at


# ---- 6: arguments ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_rules(ctx, net1):
    import torch
    import czk_amd
    from guarded import Guards
    G = Guards("cuda")
    out = G.out(1, 8)
    p = torch.zeros((64, 4), dtype=torch.int64, device="cuda").data_ptr()
    calls = {"mul": lambda net, q, o, n: net.gsz_share_batch_mul(0, q, q, q, q, o, n), "inv": lambda net, q, o, n: net.gsz_share_batch_inv(0, q, q, q, q, o, n),
             "pp": lambda net, q, o, n: net.gsz_share_partial_products(0, q, q, q, q, o, n)}
    for name, call in calls.items():
        assert call(net1, p, out.ptr, 0) == (0, 0) and call(net1, None, None, 0) == (0, 0)              # nothing to do: CZK_OK whatever the pointers
        for args, code in (((None, out.ptr, 8), 3), ((p, None, 8), 3), ((p, out.ptr, 1 << 60), 1)):     # null vector / output; a byte count that overflows
            with pytest.raises(czk_amd.CzkError) as e:
                call(net1, *args)
            assert e.value.code == code, (name, args)
        assert out.untouched(), name
    assert net1.gsz_product_check(0, None, None, None, 0, None, None, None) == (True, 0)                # no triples: nothing to refute
    for q, n, code in ((None, 8, 3), (p, 1 << 32, 1), (p, 1 << 60, 1)):
        with pytest.raises(czk_amd.CzkError) as e:
            net1.gsz_product_check(0, q, q, q, n, q, q, q)
        assert e.value.code == code, n
    bare = czk_amd.Net(None, czk_amd.CZK_NET_SHM, 0, 1, os.urandom(16))                                 # a communicator without a context
    try:
        for call in list(calls.values()) + [lambda net, q, o, n: net.gsz_product_check(0, q, q, q, n, q, q, q)]:
            with pytest.raises(czk_amd.CzkError) as e:
                call(bare, p, out.ptr, 8)
            assert e.value.code == 3
    finally:
        bare.close()
    assert out.untouched()


@pytest.mark.gpu
def test_a_world_without_a_share_domain_is_a_size_error(ctx):
    """5 parties have no share domain.  The five ranks are threads of this process on one context (creating a communicator is collective); the calls
    fail on their arguments, before any exchange, so they are made one after the other: CZK_ERR_SIZE, n = 0 included, nothing written"""
    import threading
    import torch
    import czk_amd
    from guarded import Guards
    idb, nets = os.urandom(16), [None] * 5

    def make(r):
        nets[r] = czk_amd.Net(ctx, czk_amd.CZK_NET_SHM, r, 5, idb, options={"timeout_ms": 20000})
    threads = [threading.Thread(target=make, args=(r,)) for r in range(5)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert all(nets)
    G = Guards("cuda")
    out = G.out(1, 8)
    p = torch.zeros((64, 4), dtype=torch.int64, device="cuda").data_ptr()
    try:
        for net in (nets[0], nets[4]):
            for call in (lambda k: net.gsz_share_batch_mul(1, p, p, p, p, out.ptr, k), lambda k: net.gsz_share_batch_inv(1, p, p, p, p, out.ptr, k),
                         lambda k: net.gsz_share_partial_products(1, p, p, p, p, out.ptr, k), lambda k: net.gsz_product_check(1, p, p, p, k, p, p, p)):
                for k in (8, 0):
                    with pytest.raises(czk_amd.CzkError) as e:
                        call(k)
                    assert e.value.code == 1, (net.rank, k)
        assert out.untouched()
    finally:
        for net in nets:
            net.close()


# ---- the torch layer -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_parallel_wrappers_return_the_models_lane_and_raise_on_a_failed_check(ctx, net1):
    """parallel.gsz_* over the communicator set with use_net (a world of one: the party's lane is the value): tensors in, the model's lane out;
    a wrong z and a zero divisor raise MpcCheckError"""
    from czk_amd import parallel
    n = 5
    parallel.use_net(net1)
    try:
        for name, op in OPS.items():
            c = _case(1, op, n)
            d = {k: _dev(c[k][0]) for k in ("x", "y", "dr", "dr2", "rands")}
            if op == M.OP_MUL:
                got = parallel.gsz_share_batch_mul(ctx, 0, d["x"], d["y"], d["dr"], d["dr2"])
            else:
                fn = parallel.gsz_share_batch_inv if op == M.OP_INV else parallel.gsz_share_partial_products
                got = fn(ctx, 0, d["x"], d["dr"], d["dr2"], d["rands"])
            ctx.sync()
            assert np.array_equal(got.cpu().numpy().view(np.uint64), c["want"][0]), name
        for wrong in (False, True):
            c = _check_case(1, n, wrong_z=wrong)
            d = [_dev(c[k][0]) for k in ("xs", "ys", "zs", "dr", "dr2", "rands")]
            if wrong:
                with pytest.raises(parallel.MpcCheckError):
                    parallel.gsz_product_check(ctx, 0, *d)
            else:
                parallel.gsz_product_check(ctx, 0, *d)
        c = _case(1, M.OP_INV, n, zero_at=2)
        with pytest.raises(parallel.MpcCheckError):
            parallel.gsz_share_batch_inv(ctx, 0, *[_dev(c[k][0]) for k in ("x", "dr", "dr2", "rands")])
    finally:
        parallel.use_net(None)
