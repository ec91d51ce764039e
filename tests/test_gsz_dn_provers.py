"""The Plonk and Marlin provers on real GSZ shares whose double and random shares are GENERATED on the device (polyvm.DnSource: czk_gsz_dn_generate and
its consistency check) instead of dealt by SeededDealer: the opened proof verifies and equals the plain prover's entry for entry, whatever the keys;
and a source whose check fails stops the prover before any product is taken."""
import random

import numpy as np
import pytest

import gsz_mul_model as M
from test_gsz_provers import _backend, _shares
from test_shared_provers import _plonk_circuit, _same

_PLONK = {}


def _plonk_case(gpu, n_gates):
    """circuit, layout, key and the plain one-lane prover's proof on THIS module's context: made once, shared, never modified"""
    if n_gates not in _PLONK:
        czk, ctx = gpu
        from czk_amd import plonk, polyvm
        c, vals, public = _plonk_circuit(n_gates, 0x51 + n_gates)
        B1 = polyvm.GpuBackend(czk, ctx, 1, polyvm.plonk_max_degree(n_gates))
        lay = plonk.layout(B1, c)
        _PLONK[n_gates] = dict(vals=vals, public=public, B1=B1, lay=lay, vk=plonk.verifier_key(lay), plain=polyvm.plonk_prove(B1, plonk.prover_inputs(B1, lay, vals)))
    return _PLONK[n_gates]


@pytest.fixture(scope="module")
def gpu():
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    yield czk_amd, ctx
    ctx.close()


def _keys(parties, seed):
    rng = random.Random(seed)
    return [bytes(rng.randrange(256) for _ in range(32)) for _ in range(parties)]


def _plonk_opened(gpu, parties, source, n_gates=8):
    from czk_amd import plonk, polyvm
    case = _plonk_case(gpu, n_gates)
    B = _backend(gpu, parties, polyvm.plonk_max_degree(n_gates), source, case["B1"])
    shares = _shares(B, parties, case["vals"], 3)
    out = polyvm.plonk_prove(B, plonk.prover_inputs(B, case["lay"], shares))
    assert B.gsz_checks >= 1 and B.gsz_queue_peak > 0
    return B, case, polyvm.open_shared_proof(B, out)


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [3, 4])
def test_plonk_with_generated_material_opens_to_the_plain_provers_proof(gpu, parties):
    from czk_amd import plonk, polyvm
    src = polyvm.DnSource(keys=_keys(parties, 1))
    B, case, opened = _plonk_opened(gpu, parties, src)
    assert src.sequence > 2                                        # one nonce per call: doubles and random shares were both drawn, more than once
    assert plonk.verify(B, case["vk"], case["public"], opened, rng=random.Random(2)) is True
    _same(opened, case["plain"])
    # other keys, other material, the same opened proof
    _, _, opened2 = _plonk_opened(gpu, parties, polyvm.DnSource(keys=_keys(parties, 2)))
    _same(opened2, opened)


@pytest.mark.gpu
@pytest.mark.parametrize("parties", [3, 4])
def test_marlin_with_generated_material_opens_to_the_plain_provers_proof(gpu, parties):
    czk, ctx = gpu
    from czk_amd import marlin, polyvm
    from test_marlin_index import chain_circuit
    H = 4
    mats, instance, witness = chain_circuit(H, 0x3A21 + H)
    md = polyvm.marlin_max_degree(H)
    B1 = polyvm.GpuBackend(czk, ctx, 1, md)
    idx = marlin.index(B1, mats["a"], mats["b"], mats["c"], 2, H - 2)
    plain = polyvm.marlin_prove(B1, marlin.prover_inputs(B1, idx, instance, witness))
    opened = []
    for seed in (5, 6):
        B = _backend(gpu, parties, md, polyvm.DnSource(keys=_keys(parties, seed)), B1)
        out = polyvm.marlin_prove(B, marlin.prover_inputs(B, idx, instance, _shares(B, parties, witness, 5)))
        opened.append(polyvm.open_shared_proof(B, out))
        assert marlin.verify(B, idx, instance, opened[-1], rng=random.Random(2)) is True
    skip = ("lcs", "lc_consts")
    _same({k: v for k, v in opened[0].items() if k not in skip}, {k: v for k, v in plain.items() if k not in skip})
    _same({k: v for k, v in opened[1].items() if k not in skip}, {k: v for k, v in opened[0].items() if k not in skip})


@pytest.mark.gpu
def test_keys_come_from_the_os_when_none_are_given(gpu):
    from czk_amd import polyvm
    parties, n = 3, 5
    src = polyvm.DnSource()
    B = _backend(gpu, parties, 64, src, None)
    dr, dr2 = src.doubles(B, n)
    assert len(src.keys) == parties and all(len(k) == 32 for k in src.keys) and len(set(src.keys)) == parties
    assert dr.shape == dr2.shape == (parties, n, 4) and src.rands(B, n).shape == (parties, n, 4) and src.sequence == 2
    D = M.Domain(parties)
    v1, b1 = D.batch_open(M.from_limbs(B.download(dr)), 1)
    v2, b2 = D.batch_open(M.from_limbs(B.download(dr2)), 2)
    assert (b1, b2) == (0, 0) and v1 == v2 and len(set(v1)) == n
    with pytest.raises(ValueError):
        polyvm.DnSource(keys=[b"short"] * 3)
    with pytest.raises(ValueError):
        polyvm.DnSource(keys=_keys(4, 1)).doubles(B, n)


@pytest.mark.gpu
def test_a_failed_check_stops_the_prover_before_any_product(gpu):
    """a dealer's lane perturbed after generation: the source raises where the material is asked for, before the C call that would consume it"""
    czk, ctx = gpu
    from czk_amd import polyvm

    class Cheat(polyvm.DnSource):
        def _generated(self, B, kind, r, r2):
            r = r.clone()
            r[1, 0, 0] += 1                                        # party 1's share of output 0 is off by one
            return r, r2

    parties, n = 3, 33
    src = Cheat(keys=_keys(parties, 3))
    B = _backend(gpu, parties, 64, src, None)
    rng = random.Random(4)
    a, b = (_shares(B, parties, [rng.randrange(M.R_MOD) for _ in range(n)], s) for s in (1, 2))
    with pytest.raises(polyvm.SharingError, match="consistency check"):
        B.mul(a, b)
    assert not B._gsz_queue and src.sequence == 1                  # nothing was multiplied, nothing queued
    # the same keys without the perturbation multiply
    B2 = _backend(gpu, parties, 64, polyvm.DnSource(keys=_keys(parties, 3)), None)
    z = B2.mul(a, b)
    D = M.Domain(parties)
    want = [x * y % M.R_MOD for x, y in zip(D.batch_open(M.from_limbs(B2.download(a)), 1)[0], D.batch_open(M.from_limbs(B2.download(b)), 1)[0])]
    assert D.batch_open(M.from_limbs(B2.download(z)), 1) == (want, 0)
    B2.transcript_point()
    assert B2.gsz_checks == 1
    assert np.asarray(B2.download(z)).shape == (parties, n, 4)
