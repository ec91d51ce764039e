"""Groth16Local.create_proof_shared: create_proof (mpc-snarks/src/groth/prover.rs:110-178) with r and s SHARED -- the three products of a shared
point and a shared scalar run as one czk_share_group_batch_scale / czk_gsz_group_batch_mul call, under GSZ guarded by czk_gsz_group_product_check --
under a real key (tests/groth16_real_key.py): the opened proof is [a] G1, [b] G2, [c] G1 of the expected exponents, verifies, equals what create_proof
gives for the same public r, s, and does not depend on how r and s were shared; an altered product share is refused under GSZ."""
import random

import numpy as np
import pytest

from groth16_real_key import R_INV, expected_exponents, key_scalars, real_key
from util import R_MOD, dot_mod_r, ints_to_limbs, limbs_to_ints, rand_fr_canonical

pytestmark = pytest.mark.gpu


def _open(ctx, p, proof):
    """the parties' sh lanes added up (GSZ: times 1 / n, p(0) of a polynomial given on the n-th roots of unity) -> {k: (affine, infinity)}"""
    ninv = ints_to_limbs([pow(p.P, -1, R_MOD)], 4)[0]
    opened = {}
    for k, g in (("a", 1), ("b", 2), ("c", 1)):
        acc = proof[k][0]
        for j in range(1, p.P):
            acc = ctx.jac_add(g, acc, proof[k][p.lpp * j])
        if p.scheme == "gsz":
            acc = ctx.jac_scalar_mul(g, acc, ninv)
        aff, inf = ctx.jac_to_affine(g, acc)
        opened[k] = (np.ravel(aff[0]).copy(), bool(inf[0]))
    return opened


def _same(a, b):
    return all(a[k][1] == b[k][1] and np.array_equal(a[k][0], b[k][0]) for k in ("a", "b", "c"))


@pytest.mark.parametrize("n_constraints,parties,scheme", [(10, 2, "spdz"), (10, 2, "hbc"), (10, 3, "gsz")])
def test_create_proof_with_shared_r_and_s(orc, n_constraints, parties, scheme):
    import torch
    import czk_amd as czk
    from czk_amd.polyvm import SharingError
    from czk_amd.provers import DnGroupSource, DummyGroupSource, Groth16Local, SeededGroupDealer, to_mont_limbs
    N = n_constraints
    key = real_key(N, limbs_to_ints(rand_fr_canonical(0x7A11 + N, 5)))
    D, ks = key["D"], key_scalars(key)
    rs = rand_fr_canonical(0xC0FFEE + 99 + N, 2)
    r, s = limbs_to_ints(rs)
    ninv = pow(parties, -1, R_MOD) if scheme == "gsz" else 1
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        ctx = czk.Context(0, ts.cuda_stream)
        p = Groth16Local(czk, ctx, N, parties, scheme=scheme, key_scalars=ks)
        p.step()
        torch.cuda.synchronize()
        res = {k: v.copy() for k, v in p.results.items()}
        sources = (DnGroupSource([bytes([7 + j] * 32) for j in range(parties)]), SeededGroupDealer(2)) if scheme == "gsz" else (SeededGroupDealer(1), DummyGroupSource())
        opened = []
        for seed, source in zip((11, 12), sources):                   # two different random sharings of the same r, s
            rng = random.Random(seed)
            r_lanes, s_lanes = p.share_scalar(r, rng), p.share_scalar(s, rng)
            plain = to_mont_limbs([r, s])
            assert not any(np.array_equal(ln, plain[0]) for ln in r_lanes) and not any(np.array_equal(ln, plain[1]) for ln in s_lanes)   # no lane holds the value
            opened.append(_open(ctx, p, p.create_proof_shared({k: v.copy() for k, v in res.items()}, r_lanes, s_lanes, source)))
            shared = (r_lanes, s_lanes)
        assert not np.array_equal(shared[0], p.share_scalar(r, random.Random(11)))
        public = _open(ctx, p, p.create_proof({k: v.copy() for k, v in res.items()}, rs[0], rs[1]))
        if scheme == "gsz":                                            # one product share altered before the check: refused
            def cheat(pts, inf):
                pts = pts.clone()
                pts[1, 2] = pts[0, 0]                                  # party 1's share of g1_b * r replaced by another point
                return pts, inf
            p._products = cheat
            with pytest.raises(SharingError):
                p.create_proof_shared({k: v.copy() for k, v in res.items()}, shared[0], shared[1], SeededGroupDealer(3))
            del p._products
        h_lanes = p.ab.cpu().numpy().view(np.uint64)
        lpp = p.lpp
        del p
        ctx.close()
    sh_lanes = [h_lanes[lpp * j] for j in range(parties)]
    h_acc = sum(dot_mod_r(ln[:D - 1], ks["h"]) for ln in sh_lanes) * R_INV % R_MOD * ninv % R_MOD
    w0 = limbs_to_ints(rand_fr_canonical(0xC0FFEE, 1))[0]
    a_exp, b_exp, c_exp, verifies, qap = expected_exponents(key, w0, r, s, h_acc)
    for k, g, e in (("a", 1, a_exp), ("b", 2, b_exp), ("c", 1, c_exp)):
        want, winf = orc.jac_to_affine(g, orc.scalar_mul(g, orc.generator_affine(g), 0, ints_to_limbs([e], 4)[0]))
        got, ginf = opened[0][k]
        assert not ginf and not winf and np.array_equal(got, np.ravel(want)), (k, scheme)
    assert verifies and qap                                            # the verification equation, and the QAP identity behind it
    assert _same(opened[0], public)                                    # what create_proof gives for the same public r, s
    assert _same(opened[0], opened[1])                                 # a second, different sharing of the same r, s
