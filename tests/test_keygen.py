"""Groth16 key generation on the GPU (czk_amd.keygen.groth16_setup) against the big-integer key of the squaring circuit
(tests/groth16_real_key.py): every query point and infinity flag equals czk_fixed_base_points of the key's discrete logs, and a key
generated here verifies a proof through czk_groth16_verify."""
import numpy as np
import pytest

from groth16_real_key import expected_exponents, real_key
from util import R_MOD, ints_to_limbs, limbs_to_ints, rand_fr_canonical

pytestmark = pytest.mark.gpu
ONE_MONT = ints_to_limbs([(1 << 256) % R_MOD], 4)[0]


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def _csr(rows):
    """rows: one list of variable indices per constraint, every coefficient one"""
    ptr = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    idx = np.array([v for r in rows for v in r], dtype=np.uint32)
    return ptr, idx, np.tile(ONE_MONT, (idx.size, 1))


def squaring_r1cs(N):
    """mpc-snarks/src/proof.rs:304-344 with variables [1, out | w_0 .. w_{N-1}]: A_i = B_i = var 2 + i; C_i = var 3 + i, the last row's is var 1 (out)"""
    ab = [[2 + i] for i in range(N)]
    c = [[3 + i] for i in range(N - 1)] + [[1]]
    return _csr(ab), _csr(ab), _csr(c)


def _toxic(N):
    return limbs_to_ints(rand_fr_canonical(0x6E17 + N, 5))


def _points(ctx, group, logs):
    """([k] G affine limbs, infinity flags) of discrete logs by czk_fixed_base_points; log 0 compares as infinity"""
    logs = [v % R_MOD for v in logs]
    return ctx.fixed_base_points(group, ints_to_limbs(logs, 4)), np.array([v == 0 for v in logs], dtype=np.uint8)


def _check_key(ctx, got, key, s1=1, s2=1):
    ni = 2
    want = {"a_query": (1, key["a"], s1), "b_g1_query": (1, key["b"], s1), "b_g2_query": (2, key["b"], s2), "h_query": (1, key["h"], s1),
            "l_query": (1, key["l"][ni:], s1), "gamma_abc_g1": (1, key["gamma_abc"], s1)}
    for name, (group, logs, s) in want.items():
        pts, inf = got[name]
        wpts, winf = _points(ctx, group, [v * s for v in logs])
        assert pts.shape == wpts.shape and np.array_equal(inf, winf), name
        assert np.array_equal(pts, wpts), name
    for name, group, log, s in (("alpha_g1", 1, "alpha", s1), ("beta_g1", 1, "beta", s1), ("delta_g1", 1, "delta", s1), ("beta_g2", 2, "beta", s2),
                                ("gamma_g2", 2, "gamma", s2), ("delta_g2", 2, "delta", s2)):
        assert np.array_equal(got[name], _points(ctx, group, [key[log] * s])[0][0]), name
    assert any(got["b_g1_query"][1]) and got["b_g1_query"][1][0] == 1 and got["b_g2_query"][1][1] == 1   # variables without a B term


@pytest.mark.parametrize("N", (6, 30))
def test_key_equals_the_known_real_key(ctx, N):
    """D = 8 with no padding row to spare (N = 6) and D = 32 (N = 30)"""
    from czk_amd.keygen import groth16_setup
    toxic = _toxic(N)
    key = real_key(N, toxic)
    assert key["D"] == (8 if N == 6 else 32)
    A, B, C = squaring_r1cs(N)
    got = groth16_setup(ctx, A, B, C, 2, N, [key[k] for k in ("tau", "alpha", "beta", "gamma", "delta")])
    _check_key(ctx, got, key)


@pytest.mark.parametrize("N", (6, 30))
def test_key_from_random_bases(ctx, N):
    from czk_amd.keygen import groth16_setup
    key = real_key(N, _toxic(N))
    s1, s2 = limbs_to_ints(rand_fr_canonical(0xBA5E + N, 2))
    g1 = ctx.fixed_base_points(1, ints_to_limbs([s1], 4))[0]
    g2 = ctx.fixed_base_points(2, ints_to_limbs([s2], 4))[0]
    A, B, C = squaring_r1cs(N)
    got = groth16_setup(ctx, A, B, C, 2, N, [key[k] for k in ("tau", "alpha", "beta", "gamma", "delta")], g1_base=g1, g2_base=g2)
    _check_key(ctx, got, key, s1, s2)


def test_end_to_end_proof_verifies_under_the_generated_key(ctx):
    from czk_amd.keygen import groth16_setup
    N = 30
    key = real_key(N, _toxic(N))
    A, B, C = squaring_r1cs(N)
    got = groth16_setup(ctx, A, B, C, 2, N, [key[k] for k in ("tau", "alpha", "beta", "gamma", "delta")])
    # a proof in the exponent (groth16/src/prover.rs:110-178): h_acc from the QAP identity A(tau) B(tau) - C(tau) = h(tau) Z(tau)
    w0, r, s = limbs_to_ints(rand_fr_canonical(0xE2E, 3))
    w = [w0]
    for _ in range(N):
        w.append(w[-1] * w[-1] % R_MOD)
    z = [1, w[N]] + w[:N]
    dot = lambda q: sum(zi * qi for zi, qi in zip(z, q)) % R_MOD   # noqa: E731
    h_acc = (dot(key["a"]) * dot(key["b"]) - dot(key["c"])) * pow(key["delta"], -1, R_MOD) % R_MOD
    a_exp, b_exp, c_exp, verifies, qap = expected_exponents(key, w0, r, s, h_acc)
    assert verifies and qap
    pa, pc = ctx.fixed_base_points(1, ints_to_limbs([a_exp, c_exp], 4))
    pb = ctx.fixed_base_points(2, ints_to_limbs([b_exp], 4))[0]
    pvk = ctx.groth16_pvk(**got["vk"])
    mont = lambda v: ints_to_limbs([v * (1 << 256) % R_MOD], 4).reshape(1, 1, 4)   # noqa: E731
    assert list(ctx.groth16_verify(pvk, pa.reshape(1, 12), pb.reshape(1, 24), pc.reshape(1, 12), mont(w[N]))) == [True]
    assert list(ctx.groth16_verify(pvk, pa.reshape(1, 12), pb.reshape(1, 24), pc.reshape(1, 12), mont(w[N] + 1))) == [False]
    pvk.release()


def test_setup_errors_follow_the_reference(ctx):
    from czk_amd.keygen import groth16_setup
    from groth16_real_key import omega_for
    A, B, C = squaring_r1cs(6)
    with pytest.raises(ValueError):   # tau in the domain: Z(tau) = 0
        groth16_setup(ctx, A, B, C, 2, 6, [pow(omega_for(3), 5, R_MOD), 2, 3, 4, 5])
    with pytest.raises(ValueError):   # delta = 0 (UnexpectedIdentity)
        groth16_setup(ctx, A, B, C, 2, 6, [7, 2, 3, 4, 0])
