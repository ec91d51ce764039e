"""The Plonk and Marlin provers on REAL additive / SPDZ shares (polyvm.Sharing): the assignment enters as random shares, every product, inverse and
running product of shared vectors runs the reference's protocol (czk_share_*), and the opened proof (polyvm.open_shared_proof) is accepted by the
verifier and equals, commitment for commitment and evaluation for evaluation, the proof the one-lane plain prover makes from the opened assignment.
The same shares through the default lane-wise products (`sharing=None`) do not give an accepted proof, and the default path on plain values is still
the checker-backed machine's."""
import random

import numpy as np
import pytest

import share_mul_model as M
from share_mul_model import R_MOD, Scheme


@pytest.fixture(scope="module")
def gpu():
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    yield czk_amd, ctx
    ctx.close()


def _same(got, want, at="proof"):
    """every commitment, opening proof, evaluation and point of two proofs of the one-lane shape"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), at
        for k in want:
            _same(got[k], want[k], at + "." + k)
    elif isinstance(want, tuple) and len(want) == 2 and isinstance(want[0], np.ndarray) and want[0].ndim == 2 and want[0].shape[1] == 12:
        assert np.array_equal(np.asarray(got[1]) != 0, np.asarray(want[1]) != 0), at
        keep = np.asarray(want[1]) == 0
        assert np.array_equal(np.asarray(got[0])[keep], want[0][keep]), at
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), at
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{at}[{i}]")
    elif isinstance(want, np.ndarray):
        assert np.array_equal(np.asarray(got).reshape(want.shape), want), at
    else:
        assert got == want, at


def _shares(B, S, values, seed):
    """a random sharing of the integers `values` under the 0 / 1 MAC key as a (lanes, n, 4) device array"""
    return B.upload(M.to_limbs(S.share(values, random.Random(seed))))


def _scheme(lpp, parties):
    return Scheme(lpp, parties, [1] + [0] * (parties - 1) if lpp == 2 else None)


def _plonk_circuit(n_gates, seed):
    """n_gates random sum / product gates over two secret inputs and the public wire "x"; the last gate's output is public too"""
    from czk_amd import plonk
    rng = random.Random(seed)
    c = plonk.Circuit()
    have = [c.new_var(), c.new_var(), c.new_pub_var("x")]
    for _ in range(n_gates - 1):
        a, b = rng.choice(have[-8:]), rng.choice(have)
        have.append(c.new_prod(a, b) if rng.random() < 0.5 else c.new_sum(a, b))
    c.publicize_var(c.new_prod(have[-1], have[0]), "result")
    assert c.n_gates() == n_gates
    vals = c.evaluate([rng.randrange(1, R_MOD) for _ in range(c.n_vars - n_gates)])
    return c, vals, {nm: vals[v] for v, nm in c.pub_vars.items()}


_PLONK = {}


def _plonk_case(gpu, n_gates):
    """circuit, layout, key and the plain one-lane prover's proof: made once per size, shared, never modified"""
    if n_gates not in _PLONK:
        czk, ctx = gpu
        from czk_amd import plonk, polyvm
        c, vals, public = _plonk_circuit(n_gates, 0x51 + n_gates)
        B1 = polyvm.GpuBackend(czk, ctx, 1, polyvm.plonk_max_degree(n_gates))
        lay = plonk.layout(B1, c)
        plain = polyvm.plonk_prove(B1, plonk.prover_inputs(B1, lay, vals))
        vk = plonk.verifier_key(lay)
        assert plonk.verify(B1, vk, public, plain, rng=random.Random(1)) is True
        _PLONK[n_gates] = dict(vals=vals, public=public, B1=B1, lay=lay, vk=vk, plain=plain)
    return _PLONK[n_gates]


@pytest.mark.gpu
@pytest.mark.parametrize("n_gates,lpp,parties,source", [(8, 2, 2, "dealer"), (8, 1, 3, "dealer"), (8, 2, 2, "dummy"), (1 << 10, 2, 2, "dealer"),
                                                        (1 << 10, 1, 3, "dealer")])
def test_plonk_on_real_shares_opens_to_the_plain_provers_proof(gpu, n_gates, lpp, parties, source):
    czk, ctx = gpu
    from czk_amd import plonk, polyvm
    case = _plonk_case(gpu, n_gates)
    S = _scheme(lpp, parties)
    src = polyvm.SeededDealer(7) if source == "dealer" else polyvm.DummySource()
    B = polyvm.GpuBackend(czk, ctx, S.lanes, polyvm.plonk_max_degree(n_gates), sharing=polyvm.Sharing(lpp, parties, src), share_srs=case["B1"])
    shares = _shares(B, S, case["vals"], 3)
    out = polyvm.plonk_prove(B, plonk.prover_inputs(B, case["lay"], shares))
    assert np.asarray(out["p_cmt"][0]).shape[0] == S.lanes                          # the proof is on share lanes ...
    opened = polyvm.open_shared_proof(B, out)
    assert plonk.verify(B, case["vk"], case["public"], opened, rng=random.Random(2)) is True
    _same(opened, case["plain"])                                                    # ... and opens to the plain prover's, entry for entry
    if (n_gates, lpp, source) == (8, 2, "dealer"):
        # what the feature fixes: the same shares through the lane-wise products are no proof -- refused at the MAC check or rejected
        B0 = polyvm.GpuBackend(czk, ctx, S.lanes, polyvm.plonk_max_degree(n_gates), lift=B.lift, share_srs=case["B1"])
        out0 = polyvm.plonk_prove(B0, plonk.prover_inputs(B0, case["lay"], shares))
        assert plonk.verify(B0, case["vk"], case["public"], out0, rng=random.Random(3)) is False
        try:
            accepted = plonk.verify(B, case["vk"], case["public"], polyvm.open_shared_proof(B, out0), rng=random.Random(4))
        except polyvm.SharingError:
            accepted = False
        assert accepted is False
        # a tampered share is refused: one limb of party 1's mac lane of the assignment
        bad = shares.clone()
        bad[3, 1, 0] ^= 1
        with pytest.raises(polyvm.SharingError):
            polyvm.open_shared_proof(B, polyvm.plonk_prove(B, plonk.prover_inputs(B, case["lay"], bad)))


@pytest.mark.gpu
@pytest.mark.parametrize("H", [4, 1 << 10])
def test_marlin_on_real_spdz_shares_opens_to_the_plain_provers_proof(gpu, H):
    """index -> prover_inputs (witness as share lanes) -> marlin_prove -> open_shared_proof -> marlin.verify on the squaring chain of
    tests/test_marlin_index.py: |H| = 4 is the smallest chain (two witness variables), 2^10 the large one; SPDZ, 2 parties"""
    czk, ctx = gpu
    from czk_amd import marlin, polyvm
    from test_marlin_index import chain_circuit
    mats, instance, witness = chain_circuit(H, 0x3A21 + H)
    md = polyvm.marlin_max_degree(H)
    B1 = polyvm.GpuBackend(czk, ctx, 1, md)
    idx = marlin.index(B1, mats["a"], mats["b"], mats["c"], 2, H - 2)
    plain = polyvm.marlin_prove(B1, marlin.prover_inputs(B1, idx, instance, witness))
    assert marlin.verify(B1, idx, instance, plain, rng=random.Random(1)) is True
    S = _scheme(2, 2)
    B = polyvm.GpuBackend(czk, ctx, 4, md, sharing=polyvm.Sharing(2, 2, polyvm.SeededDealer(9)), share_srs=B1)
    shares = _shares(B, S, witness, 5)
    out = polyvm.marlin_prove(B, marlin.prover_inputs(B, idx, instance, shares))
    opened = polyvm.open_shared_proof(B, out)
    assert marlin.verify(B, idx, instance, opened, rng=random.Random(2)) is True
    _same({k: v for k, v in opened.items() if k not in ("lcs", "lc_consts")}, {k: v for k, v in plain.items() if k not in ("lcs", "lc_consts")})
    if H == 4:
        B0 = polyvm.GpuBackend(czk, ctx, 4, md, lift=B.lift, share_srs=B1)
        out0 = polyvm.marlin_prove(B0, marlin.prover_inputs(B0, idx, instance, shares))
        assert marlin.verify(B0, idx, instance, out0, rng=random.Random(3)) is False
        try:
            accepted = marlin.verify(B, idx, instance, polyvm.open_shared_proof(B, out0), rng=random.Random(4))
        except polyvm.SharingError:
            accepted = False
        assert accepted is False


@pytest.mark.gpu
def test_default_path_has_not_drifted(gpu, orc):
    """sharing=None on plain values: the Plonk proof of tests/test_pipelines.py's 8-gate, 3-lane case is still the checker-backed machine's, entry for
    entry -- the option changes nothing unless it is given"""
    czk, ctx = gpu
    from czk_amd import polyvm
    from oracle_backend import make_backend
    from test_pipelines import _compare
    md = polyvm.plonk_max_degree(8)
    B = polyvm.GpuBackend(czk, ctx, 3, md)
    assert B.sharing is None and B.lift == (1, 1, 1)
    cpu = make_backend(orc, polyvm, 3, md, bases=B.bases_host(), bases_gamma=B.bases_gamma_host())
    _compare(polyvm.plonk_prove(B, polyvm.plonk_inputs(B, 8)), polyvm.plonk_prove(cpu, polyvm.plonk_inputs(cpu, 8)))


def _party_worker(rank, world, q, idb, lpp):
    import os
    import sys
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        sys.path.insert(0, p)
    import czk_amd
    from czk_amd import parallel, polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    net = czk_amd.Net(ctx, czk_amd.CZK_NET_SHM, rank, world, idb, options={"timeout_ms": 60000})
    parallel.use_net(net)
    B = polyvm.GpuBackend(czk_amd, ctx, lpp, 8, sharing=polyvm.Sharing(lpp, world, polyvm.SeededDealer(7), rank=rank))
    B.commit_opens = "tree"
    S = _scheme(lpp, world)
    a, b = (B.sharing.own(_shares(B, S, v, seed)) for v, seed in ((_PARTY_A, 1), (_PARTY_B, 2)))
    res = [B.download(r).copy() for r in (B.mul(a, b), B.inverse(a), B.prefix_product(a), B.mul(a, B.const(3, len(_PARTY_A))))]
    net.barrier()
    parallel.use_net(None)
    net.close()
    ctx.close()
    q.put((rank, res))


_PARTY_A = [random.Random(11).randrange(1, R_MOD) for _ in range(33)]
_PARTY_B = [random.Random(12).randrange(1, R_MOD) for _ in range(33)]


@pytest.mark.gpu
@pytest.mark.parametrize("world,lpp", [(2, 2), (3, 2)])
def test_one_process_per_party_behind_the_same_sharing_object(world, lpp):
    """GpuBackend with Sharing(rank=...) over parallel.use_net on CZK_NET_SHM: every party's mul / inverse / prefix_product results, put together,
    are valid sharings (MACs included) of the product, the inverses and the running products; a public factor still just scales the lanes"""
    import os
    from test_net import _spawn
    res = _spawn(_party_worker, world, os.urandom(16), lpp, timeout=120)
    assert [r for r, _ in res] == list(range(world))
    S = _scheme(lpp, world)
    run, pp = 1, []
    for v in _PARTY_A:
        run = run * v % R_MOD
        pp.append(run)
    want = ([x * y % R_MOD for x, y in zip(_PARTY_A, _PARTY_B)], [pow(x, -1, R_MOD) for x in _PARTY_A], pp, [3 * x % R_MOD for x in _PARTY_A])
    for k, w in enumerate(want):
        vals, bad = S.batch_open(M.from_limbs(np.concatenate([lanes[k] for _, lanes in res])))
        assert bad == 0 and vals == w, k


def test_sharing_arguments():
    from czk_amd import polyvm
    for lpp, parties in ((0, 2), (3, 2), (1, 0), (2, 33)):
        with pytest.raises(ValueError):
            polyvm.Sharing(lpp, parties, polyvm.DummySource())
    s = polyvm.Sharing(2, 3, polyvm.DummySource())
    assert s.lanes == 6 and s.lift == (1, 1, 0, 0, 0, 0) and [polyvm.unmont(m) for m in s.mac_shares] == [1, 0, 0]
    assert polyvm.Sharing(1, 3, polyvm.DummySource()).lift == (1, 0, 0)
    king, other = polyvm.Sharing(2, 3, polyvm.DummySource(), rank=0), polyvm.Sharing(2, 3, polyvm.DummySource(), rank=2)
    assert (king.backend_lanes, king.lift, other.lift) == (2, (1, 1), (0, 0)) and s.backend_lanes == 6
    for lpp, rank in ((2, 3), (1, 0)):                                             # no such party; one additive lane looks like public data
        with pytest.raises(ValueError):
            polyvm.Sharing(lpp, 3, polyvm.DummySource(), rank=rank)
