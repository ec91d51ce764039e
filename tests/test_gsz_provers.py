"""The Plonk and Marlin provers on REAL GSZ (Shamir) shares (polyvm.Sharing(..., scheme="gsz")): the assignment enters as random degree-t sharings,
every product, inverse and running product of shared vectors runs gsz20's protocol (czk_gsz_share_*), every product's triple goes through gsz20's
product check (czk_gsz_product_check) before anything is opened, and the opened proof (polyvm.open_shared_proof) is accepted by the verifier and
equals, entry for entry, the proof the one-lane plain prover makes.  The same shares through the default lane-wise products (`sharing=None`) give no
accepted proof; a triple corrupted in the queue is refused at the next transcript point; the reference's stand-in case is unchanged."""
import random

import numpy as np
import pytest

import gsz_mul_model as M
from test_shared_provers import _plonk_circuit, _same

_PLONK = {}


def _plonk_case(gpu, n_gates):
    """circuit, layout, key and the plain one-lane prover's proof on this module's context: made once per size, shared, never modified"""
    if n_gates not in _PLONK:
        czk, ctx = gpu
        from czk_amd import plonk, polyvm
        c, vals, public = _plonk_circuit(n_gates, 0x51 + n_gates)
        B1 = polyvm.GpuBackend(czk, ctx, 1, polyvm.plonk_max_degree(n_gates))
        lay = plonk.layout(B1, c)
        plain = polyvm.plonk_prove(B1, plonk.prover_inputs(B1, lay, vals))
        _PLONK[n_gates] = dict(vals=vals, public=public, B1=B1, lay=lay, vk=plonk.verifier_key(lay), plain=plain)
    return _PLONK[n_gates]


@pytest.fixture(scope="module")
def gpu():
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    yield czk_amd, ctx
    ctx.close()


def _shares(B, parties, values, seed):
    """a random degree-t Shamir sharing of the integers `values` as a (parties, n, 4) device array"""
    return B.upload(M.to_limbs(M.Domain(parties).share(values, M.threshold(parties), random.Random(seed))))


def _backend(gpu, parties, max_degree, source, share_srs):
    czk, ctx = gpu
    from czk_amd import polyvm
    return polyvm.GpuBackend(czk, ctx, parties, max_degree, sharing=polyvm.Sharing(1, parties, source, scheme="gsz"), share_srs=share_srs)


@pytest.mark.gpu
@pytest.mark.parametrize("n_gates,parties", [(8, 3), (8, 4), (1 << 10, 3), (1 << 10, 4)])
def test_plonk_on_real_gsz_shares_opens_to_the_plain_provers_proof(gpu, n_gates, parties):
    czk, ctx = gpu
    from czk_amd import plonk, polyvm
    case = _plonk_case(gpu, n_gates)
    md = polyvm.plonk_max_degree(n_gates)
    B = _backend(gpu, parties, md, polyvm.SeededDealer(7), case["B1"])
    shares = _shares(B, parties, case["vals"], 3)
    out = polyvm.plonk_prove(B, plonk.prover_inputs(B, case["lay"], shares))
    assert np.asarray(out["p_cmt"][0]).shape[0] == parties and B.gsz_checks >= 1 and B.gsz_queue_peak > 0
    opened = polyvm.open_shared_proof(B, out)
    assert plonk.verify(B, case["vk"], case["public"], opened, rng=random.Random(2)) is True
    _same(opened, case["plain"])
    if n_gates == 8:
        # what the feature fixes: the same shares through the lane-wise products are no proof -- refused at a degree bound or rejected
        B0 = polyvm.GpuBackend(czk, ctx, parties, md, lift=B.lift, share_srs=case["B1"])
        out0 = polyvm.plonk_prove(B0, plonk.prover_inputs(B0, case["lay"], shares))
        assert plonk.verify(B0, case["vk"], case["public"], out0, rng=random.Random(3)) is False
        try:
            accepted = plonk.verify(B, case["vk"], case["public"], polyvm.open_shared_proof(B, out0), rng=random.Random(4))
        except polyvm.SharingError:
            accepted = False
        assert accepted is False


@pytest.mark.gpu
@pytest.mark.parametrize("H,parties", [(4, 3), (4, 4), (1 << 10, 3), (1 << 10, 4)])
def test_marlin_on_real_gsz_shares_opens_to_the_plain_provers_proof(gpu, H, parties):
    czk, ctx = gpu
    from czk_amd import marlin, polyvm
    from test_marlin_index import chain_circuit
    mats, instance, witness = chain_circuit(H, 0x3A21 + H)
    md = polyvm.marlin_max_degree(H)
    B1 = polyvm.GpuBackend(czk, ctx, 1, md)
    idx = marlin.index(B1, mats["a"], mats["b"], mats["c"], 2, H - 2)
    plain = polyvm.marlin_prove(B1, marlin.prover_inputs(B1, idx, instance, witness))
    B = _backend(gpu, parties, md, polyvm.SeededDealer(9), B1)
    shares = _shares(B, parties, witness, 5)
    out = polyvm.marlin_prove(B, marlin.prover_inputs(B, idx, instance, shares))
    opened = polyvm.open_shared_proof(B, out)
    assert marlin.verify(B, idx, instance, opened, rng=random.Random(2)) is True
    _same({k: v for k, v in opened.items() if k not in ("lcs", "lc_consts")}, {k: v for k, v in plain.items() if k not in ("lcs", "lc_consts")})
    if H == 4:
        B0 = polyvm.GpuBackend(czk, ctx, parties, md, lift=B.lift, share_srs=B1)
        out0 = polyvm.marlin_prove(B0, marlin.prover_inputs(B0, idx, instance, shares))
        assert marlin.verify(B0, idx, instance, out0, rng=random.Random(3)) is False


@pytest.mark.gpu
def test_a_triple_corrupted_in_the_queue_is_refused_at_the_next_transcript_point(gpu):
    from czk_amd import polyvm
    parties, n = 3, 33
    B = _backend(gpu, parties, 64, polyvm.SeededDealer(11), None)
    rng = random.Random(4)
    a, b = (_shares(B, parties, [rng.randrange(M.R_MOD) for _ in range(n)], s) for s in (1, 2))
    z = B.mul(a, b)
    D = M.Domain(parties)
    want = [x * y % M.R_MOD for x, y in zip(D.batch_open(M.from_limbs(B.download(a)), 1)[0], D.batch_open(M.from_limbs(B.download(b)), 1)[0])]
    assert D.batch_open(M.from_limbs(B.download(z)), 1) == (want, 0)
    B.transcript_point()                                            # honest: the check passes and empties the queue
    assert B.gsz_checks == 1 and B.gsz_queue_peak == n and not B._gsz_queue
    z = B.mul(a, b)
    one = B.upload(M.to_limbs(D.share([1] * n, 1, rng)))            # a consistent sharing of one on every element: no degree bound sees it
    x, y, _ = B._gsz_queue[0]
    B._gsz_queue[0] = (x, y, B.add(z, one))
    with pytest.raises(polyvm.SharingError):
        B.transcript_point()
    assert not B._gsz_queue


@pytest.mark.gpu
def test_dummy_source_is_the_stand_in_case(gpu):
    """every party holds the value itself, every double and random share is one: under the new sharing the proof's lanes are, entry for entry, the ones
    today's `sharing=None` GSZ run makes (where a product is the lane-wise product), and the product check passes on them"""
    czk, ctx = gpu
    from czk_amd import polyvm
    from test_pipelines import _compare
    md = polyvm.plonk_max_degree(8)
    B0 = polyvm.GpuBackend(czk, ctx, 3, md)
    B = _backend(gpu, 3, md, polyvm.DummySource(), B0)
    assert B.lift == B0.lift == (1, 1, 1)
    _compare(polyvm.plonk_prove(B, polyvm.plonk_inputs(B, 8)), polyvm.plonk_prove(B0, polyvm.plonk_inputs(B0, 8)))
    assert B.gsz_checks >= 1


def test_gsz_sharing_arguments():
    from czk_amd import polyvm
    s = polyvm.Sharing(1, 3, polyvm.DummySource(), scheme="gsz")
    assert (s.lanes, s.backend_lanes, s.lift, s.degree, s.scheme) == (3, 3, (1, 1, 1), 1, "gsz")
    assert [polyvm.Sharing(1, p, polyvm.DummySource(), scheme="gsz").degree for p in (4, 6, 8, 12)] == [1, 2, 3, 5]
    for lpp, parties in ((2, 3), (1, 5), (1, 0), (1, 97), (1, 9)):
        with pytest.raises(ValueError):
            polyvm.Sharing(lpp, parties, polyvm.DummySource(), scheme="gsz")
    with pytest.raises(ValueError, match="not built"):
        polyvm.Sharing(1, 3, polyvm.DummySource(), rank=0, scheme="gsz")
    with pytest.raises(ValueError):
        polyvm.Sharing(1, 3, polyvm.DummySource(), scheme="spdz")
    assert polyvm.Sharing(2, 2, polyvm.DummySource()).scheme == "spdz" and polyvm.Sharing(1, 2, polyvm.DummySource()).scheme == "additive"
