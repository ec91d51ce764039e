"""The pairing and batched Groth16 verification on the GPU (czk_pairing, czk_pairing_product, czk_groth16_pvk_create / czk_groth16_verify),
held bit for bit against the big-integer restatement of the reference's engine (tests/pairing_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import pairing_ref as P
from groth16_real_key import key_scalars, real_key
from util import R_MOD, ints_to_limbs, limbs_to_ints, rand_fr_canonical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_LIMBS = np.array(P.fq12_to_limbs(P.FQ12_ONE), dtype=np.uint64)


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def _g1(points):
    rows = [P.g1_to_limbs(p) for p in points]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(-1, 12), np.array([r[1] for r in rows], dtype=np.uint8)


def _g2(points):
    rows = [P.g2_to_limbs(q) for q in points]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(-1, 24), np.array([r[1] for r in rows], dtype=np.uint8)


def _fixed(ctx, group, ks):
    import czk_amd
    return ctx.fixed_base_points(czk_amd.CZK_G1 if group == 1 else czk_amd.CZK_G2, ints_to_limbs([k % R_MOD for k in ks], 4))


def test_pairing_is_bit_exact_against_the_restatement(ctx):
    a, b = 0x5EED_1234_ABCD, 2 ** 250 + 77
    p, q = P.g1_mul(a), P.g2_mul(b)
    pairs = [(P.G1_GEN, P.G2_GEN), (p, P.G2_GEN), (P.G1_GEN, q), (p, q), (P.ec_neg(P.F1, p), q), (P.INF, q), (p, P.INF), (P.INF, P.INF),
             (P.g1_mul(3), P.g2_mul(R_MOD - 1))]
    g1, i1 = _g1([x for x, _ in pairs])
    g2, i2 = _g2([y for _, y in pairs])
    got = ctx.pairing(g1, g2, i1, i2)
    for j, (x, y) in enumerate(pairs):
        want = np.array(P.fq12_to_limbs(P.pairing(x, y)), dtype=np.uint64)
        assert np.array_equal(got[j], want), j
    assert np.array_equal(got[5], ONE_LIMBS) and np.array_equal(got[6], ONE_LIMBS) and np.array_equal(got[7], ONE_LIMBS)


def test_bilinearity_on_a_batch_of_4096(ctx):
    n = 4096
    a = limbs_to_ints(rand_fr_canonical(0xB111, n))
    b = limbs_to_ints(rand_fr_canonical(0xB112, n))
    ab = [x * y % R_MOD for x, y in zip(a, b)]
    g1_gen, g2_gen = _fixed(ctx, 1, [1] * n), _fixed(ctx, 2, [1] * n)
    e1 = ctx.pairing(_fixed(ctx, 1, a), _fixed(ctx, 2, b))
    e2 = ctx.pairing(_fixed(ctx, 1, ab), g2_gen)
    e3 = ctx.pairing(g1_gen, _fixed(ctx, 2, ab))
    assert np.array_equal(e1, e2) and np.array_equal(e2, e3)
    assert len({e1[i].tobytes() for i in range(0, n, 97)}) == len(range(0, n, 97))   # distinct values: not a degenerate constant
    want = np.array(P.fq12_to_limbs(P.pairing(P.g1_mul(ab[7]), P.G2_GEN)), dtype=np.uint64)
    assert np.array_equal(e1[7], want)


def test_products_of_pairings(ctx):
    ks = [(i * 7919 + 3, i * 104729 + 11) for i in range(17)]
    pts1 = [P.g1_mul(x) for x, _ in ks]
    pts2 = [P.g2_mul(y) for _, y in ks]
    single = ctx.pairing(*_g1(pts1)[:1], *_g2(pts2)[:1])
    sizes = [0, 1, 2, 3, 17]
    offs, g1, g2 = [0], [], []
    for s in sizes:
        g1 += pts1[:s]
        g2 += pts2[:s]
        offs.append(offs[-1] + s)
    a1, i1 = _g1(g1)
    a2, i2 = _g2(g2)
    got, one = ctx.pairing_product(a1, a2, offs, i1, i2)
    for j, s in enumerate(sizes):
        acc = P.FQ12_ONE
        for t in range(s):
            acc = P.fq12_mul(acc, P.fq12_from_limbs(single[t]))
        assert np.array_equal(got[j], np.array(P.fq12_to_limbs(acc), dtype=np.uint64)), s
    assert list(one) == [1, 0, 0, 0, 0]
    # e(P, Q) e(-P, Q) is one
    p, q = P.g1_mul(12345), P.g2_mul(678)
    a1, i1 = _g1([p, P.ec_neg(P.F1, p)])
    a2, i2 = _g2([q, q])
    got, one = ctx.pairing_product(a1, a2, [0, 2], i1, i2)
    assert one[0] == 1 and np.array_equal(got[0], ONE_LIMBS)


@pytest.fixture(scope="module")
def pair_pool(ctx):
    """eight pairs (P_i, Q_i), the last four the first four with P negated, and the GPU's single pairings of them: values the first test
    pins to the model"""
    pts1 = [P.g1_mul(i * 7919 + 5) for i in range(4)]
    pts2 = [P.g2_mul(i * 104729 + 13) for i in range(4)]
    pts1 += [P.ec_neg(P.F1, p) for p in pts1]
    pts2 += pts2
    single = ctx.pairing(_g1(pts1)[0], _g2(pts2)[0])
    return pts1, pts2, [P.fq12_from_limbs(row) for row in single]


@pytest.mark.parametrize("k", [63, 64, 65, 130])
def test_products_of_pairings_across_the_wave_boundary(ctx, pair_pool, k):
    """The final exponentiation parks three Fq12 per thread in a workspace laid out SoA with stride k: k just below, at and above one
    wave, and above two.  Products of 0 to 3 pairs, infinity flags scattered on either side, every value and every is-one flag exact."""
    pts1, pts2, single = pair_pool
    offs, g1, g2, i1, i2, want = [0], [], [], [], [], []
    for j in range(k):
        size = (j + j // 4) % 4
        idx = [(3 * j + 4 * t) % 8 for t in range(size)]          # t and t + 1 pick (i, i + 4): e(P, Q) e(-P, Q) == 1
        acc = P.FQ12_ONE
        for t, i in enumerate(idx):
            inf1, inf2 = (5 * j + t) % 7 == 0, (3 * j + 2 * t) % 11 == 0
            g1.append(P.INF if (5 * j + t) % 14 == 0 else pts1[i])   # an infinity flag with and without the point's limbs beside it
            g2.append(P.INF if (3 * j + 2 * t) % 22 == 0 else pts2[i])
            i1.append(int(inf1))
            i2.append(int(inf2))
            if not (inf1 or inf2):
                acc = P.fq12_mul(acc, single[i])
        offs.append(len(g1))
        want.append(acc)
    a1, a2 = _g1(g1)[0], _g2(g2)[0]
    got, one = ctx.pairing_product(a1, a2, offs, np.array(i1, dtype=np.uint8), np.array(i2, dtype=np.uint8))
    sizes = np.diff(offs)
    assert set(sizes) == {0, 1, 2, 3} and 0 < sum(i1) < len(i1) and 0 < sum(i2) < len(i2)
    ones = [w == P.FQ12_ONE for w in want]
    assert any(o and s == 2 and not (i1[a] or i2[a] or i1[a + 1] or i2[a + 1]) for o, s, a in zip(ones, sizes, offs)), "no e(P, Q) e(-P, Q) product"
    assert any(not o for o in ones)
    for j in range(k):
        assert np.array_equal(got[j], np.array(P.fq12_to_limbs(want[j]), dtype=np.uint64)), (k, j)
    assert list(one) == [int(o) for o in ones]


# ------------------------------------------------------------------------------------------------------------------- Groth16
def _proof(N, parties, scheme):
    """A Groth16 proof of the squaring circuit under a real key (as tests/test_verify.py builds it), opened: returns (key, A, B, C affine limbs, out)."""
    import torch
    import czk_amd as czk
    from czk_amd.provers import Groth16Local
    key = real_key(N, limbs_to_ints(rand_fr_canonical(0x7A11 + N, 5)))
    ks = key_scalars(key)
    rs = rand_fr_canonical(0xC0FFEE + 77 + N, 2)
    ninv = pow(parties, -1, R_MOD) if scheme == "gsz" else 1
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        c = czk.Context(0, ts.cuda_stream)
        p = Groth16Local(czk, c, N, parties, scheme=scheme, key_scalars=ks)
        p.step()
        torch.cuda.synchronize()
        proof = p.create_proof({k: v.copy() for k, v in p.results.items()}, rs[0], rs[1])
        opened = {}
        for k, g in (("a", 1), ("b", 2), ("c", 1)):
            acc = proof[k][0]
            for j in range(1, parties):
                acc = c.jac_add(g, acc, proof[k][p.lpp * j])
            if scheme == "gsz":
                acc = c.jac_scalar_mul(g, acc, ints_to_limbs([ninv], 4)[0])
            aff, inf = c.jac_to_affine(g, acc)
            assert not inf[0]
            opened[k] = np.ravel(aff[0])
        del p
        c.close()
    w = limbs_to_ints(rand_fr_canonical(0xC0FFEE, 1))[0]
    for _ in range(N):
        w = w * w % R_MOD
    return key, opened, w


def _pvk(ctx, key):
    """The verifying key's points built from the toxic waste by czk_fixed_base_points; the toxic waste goes no further."""
    alpha = _fixed(ctx, 1, [key["alpha"]])[0]
    beta, gamma, delta = _fixed(ctx, 2, [key["beta"], key["gamma"], key["delta"]])
    abc = _fixed(ctx, 1, key["gamma_abc"])
    return ctx.groth16_pvk(alpha, beta, gamma, delta, abc), alpha, abc


def _mont(v):
    return ints_to_limbs([v * (1 << 256) % R_MOD], 4)


@pytest.mark.parametrize("n_constraints,parties,scheme", [(10, 2, "spdz"), (1000, 3, "gsz"), (333, 1, "hbc")])
def test_groth16_proofs_verify_by_pairing(ctx, n_constraints, parties, scheme):
    import czk_amd
    from groth16_real_key import expected_exponents  # noqa: F401  (the exponent check of tests/test_verify.py gives the same verdict)
    key, pr, out = _proof(n_constraints, parties, scheme)
    pvk, alpha, abc = _pvk(ctx, key)
    x = _mont(out).reshape(1, 1, 4)
    a, b, c = pr["a"].reshape(1, 12), pr["b"].reshape(1, 24), pr["c"].reshape(1, 12)
    assert list(ctx.groth16_verify(pvk, a, b, c, x)) == [True]
    # the same decision as the reference's three pairings: e(A, B) == e(alpha, beta) e(g_ic, gamma) e(C, delta)
    # tampered proofs
    g1 = _fixed(ctx, 1, [1])[0]
    a_plus = ctx.jac_to_affine(czk_amd.CZK_G1, ctx.jac_add_mixed(czk_amd.CZK_G1, np.concatenate([a[0], np.array(P.pyref.int_to_limbs(P.pyref.FQ_MONT_R, 6), np.uint64)]), g1))[0]
    neg_b = np.array(P.g2_to_limbs(P.ec_neg(P.F2, P.g2_from_limbs(list(b[0]), 0)))[0], dtype=np.uint64).reshape(1, 24)
    other = _proof(10, 1, "hbc")[1] if n_constraints != 10 else _proof(11, 1, "hbc")[1]
    bad_x = _mont(out + 1).reshape(1, 1, 4)
    assert list(ctx.groth16_verify(pvk, a_plus, b, c, x)) == [False]
    assert list(ctx.groth16_verify(pvk, a, neg_b, c, x)) == [False]
    assert list(ctx.groth16_verify(pvk, a, b, other["c"].reshape(1, 12), x)) == [False]
    assert list(ctx.groth16_verify(pvk, a, b, c, bad_x)) == [False]
    with pytest.raises(czk_amd.CzkError) as ei:
        ctx.groth16_verify(pvk, a, b, c, np.concatenate([x, x], axis=1))
    assert ei.value.code == 3 and "MalformedVerifyingKey" in str(ei.value)
    if n_constraints == 10:
        # a batch of 1024: valid and tampered proofs at random positions, every flag exact
        k = 1024
        rng = np.random.default_rng(1)
        kind = rng.integers(0, 4, k)
        A = np.repeat(a, k, axis=0)
        B = np.repeat(b, k, axis=0)
        Cc = np.repeat(c, k, axis=0)
        X = np.repeat(x, k, axis=0)
        A[kind == 1] = a_plus[0]
        B[kind == 2] = neg_b[0]
        X[kind == 3] = bad_x[0]
        ok = ctx.groth16_verify(pvk, A, B, Cc, X)
        assert np.array_equal(ok, kind == 0)
    pvk.release()


def test_groth16_full_size_proof_verifies_by_pairing(ctx):
    """BASELINE configs[1]: 2^20 constraints, SPDZ, two parties -- the proof verifies by pairing."""
    key, pr, out = _proof(1 << 20, 2, "spdz")
    pvk, _, _ = _pvk(ctx, key)
    assert list(ctx.groth16_verify(pvk, pr["a"].reshape(1, 12), pr["b"].reshape(1, 24), pr["c"].reshape(1, 12), _mont(out).reshape(1, 1, 4))) == [True]
    pvk.release()


def test_kzg_opening_checks_by_pairing_product(ctx):
    """KZG10 (poly-commit/src/kzg10/mod.rs): commit to p under powers of tau, open at z with czk_poly_div_linear and an MSM, then
    e(C - [v] G, H) e(-W, [tau] H - [z] H) == 1 through czk_pairing_product alone; a wrong v is not one."""
    import czk_amd
    n = 64
    tau = limbs_to_ints(rand_fr_canonical(0x7A0, 1))[0]
    powers = _fixed(ctx, 1, [pow(tau, i, R_MOD) for i in range(n)])
    coeffs = rand_fr_canonical(0x7A1, n)
    z = limbs_to_ints(rand_fr_canonical(0x7A2, 1))[0]
    coeffs_m = _mont_vec(limbs_to_ints(coeffs))
    q, v = ctx.poly_div_linear(coeffs_m, _mont(z)[0])
    v_int = limbs_to_ints(v.reshape(1, 4))[0] * pow(1 << 256, -1, R_MOD) % R_MOD
    assert v_int == sum(c * pow(z, i, R_MOD) for i, c in enumerate(limbs_to_ints(coeffs))) % R_MOD
    C = ctx.jac_to_affine(czk_amd.CZK_G1, ctx.msm_oneshot(czk_amd.CZK_G1, powers, None, coeffs_m, scalar_form=czk_amd.CZK_SCALAR_MONTGOMERY))
    W = ctx.jac_to_affine(czk_amd.CZK_G1, ctx.msm_oneshot(czk_amd.CZK_G1, powers[:n - 1], None, q.reshape(-1, 4), scalar_form=czk_amd.CZK_SCALAR_MONTGOMERY))
    Cp, Wp = P.g1_from_limbs(list(C[0][0]), C[1][0]), P.g1_from_limbs(list(W[0][0]), W[1][0])
    H = P.G2_GEN
    tz_h = P.ec_add(P.F2, P.g2_mul(tau), P.ec_neg(P.F2, P.g2_mul(z)))
    rows = []
    for vv in (v_int, v_int + 1):
        lhs = P.g1_add(Cp, P.ec_neg(P.F1, P.g1_mul(vv)))
        rows += [(lhs, H), (P.ec_neg(P.F1, Wp), tz_h)]
    g1, i1 = _g1([r[0] for r in rows])
    g2, i2 = _g2([r[1] for r in rows])
    got, one = ctx.pairing_product(g1, g2, [0, 2, 4], i1, i2)
    assert list(one) == [1, 0]


def _mont_vec(vals):
    return ints_to_limbs([v * (1 << 256) % R_MOD for v in vals], 4)


def test_cpp_mirror_matches_python(ctx):
    """tools/pairing_demo.cpp on include/czk.hpp's Bls12_377::pairing and verify_proof: e(G1, G2) and one verification, compared with Python."""
    pkg = os.path.join(ROOT, "collaborative-zksnark_amd")
    out = os.path.join(ROOT, "tools", "pairing_demo.bin")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "pairing_demo.cpp"),
                           "-L" + pkg, "-lczk_hip", "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib", "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    want = P.fq12_to_limbs(P.pairing(P.G1_GEN, P.G2_GEN))
    assert [int(t, 16) for t in lines[0].split()] == want
    assert lines[1:] == ["verify 1", "verify 0"]
