"""KZG10 setup, check and batch_check on the GPU (czk_amd.kzg, csrc/kzg.hip) against the affine big-integer group law and product_of_pairings of
tests/pairing_ref.py and the known-beta identity; the openings are made as in tests/test_pairing.py's KZG test -- czk_poly_div_linear for the
witness polynomial, MSMs over the powers for commitments and proofs -- with polynomials of degree <= 63."""
import random

import numpy as np
import pytest

import pairing_ref as P
import point_codec_ref as R
from util import R_MOD, ints_to_limbs, limbs_to_ints, rand_fr_canonical

pytestmark = pytest.mark.gpu
BETA = limbs_to_ints(rand_fr_canonical(0x6B10, 1))[0]
GAMMA = limbs_to_ints(rand_fr_canonical(0x6B11, 1))[0]
D = 63
K = 65
R_INV = pow(1 << 256, -1, R_MOD)


def mont(vals):
    return ints_to_limbs([v % R_MOD * (1 << 256) % R_MOD for v in vals], 4)


def unmont(limbs):
    return [v * R_INV % R_MOD for v in limbs_to_ints(np.asarray(limbs).reshape(-1, 4))]


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pp(ctx):
    from czk_amd import kzg
    return kzg.setup(ctx, D, BETA, GAMMA, produce_g2_powers=True)


@pytest.fixture(scope="module")
def vk(ctx, pp):
    from czk_amd import kzg
    return ctx.kzg10_vk(**kzg.trim(pp, D)[1])


def _g1(pts, inf):
    return [P.g1_from_limbs([int(v) for v in pts[i]], int(inf[i])) for i in range(len(inf))]


def _g1_limbs(points):
    rows = [P.g1_to_limbs(p) for p in points]
    return np.array([r[0] for r in rows], dtype=np.uint64).reshape(-1, 12), np.array([r[1] for r in rows], dtype=np.uint8)


def _commit(ctx, bases, polys):
    """one MSM per polynomial (a lane each) over the first len(poly) powers: (points, flags)"""
    import czk_amd
    n = max(len(p) for p in polys)
    sc = np.concatenate([mont(list(p) + [0] * (n - len(p))) for p in polys])
    jac = ctx.msm(bases, sc, n_scalars=n, lanes=len(polys), scalar_form=czk_amd.CZK_SCALAR_MONTGOMERY)
    return ctx.jac_to_affine(czk_amd.CZK_G1, jac)


@pytest.fixture(scope="module")
def openings(ctx, pp):
    """K honest openings of polynomials of degree <= 63, not hiding and hiding (blinding polynomial of degree 2 over powers_of_gamma_g, as
    KZG10::commit / open with a hiding bound of 1), plus the special ones: the zero polynomial, a constant, and z = beta."""
    import czk_amd
    bg = ctx.register_bases(czk_amd.CZK_G1, pp["powers_of_g"][0], pp["powers_of_g"][1])
    bgam = ctx.register_bases(czk_amd.CZK_G1, pp["powers_of_gamma_g"][0][:8], pp["powers_of_gamma_g"][1][:8])
    rng = random.Random(0x6B20)
    degs = [D, 1, 2, 62] + [rng.randrange(1, D + 1) for _ in range(K - 4)]
    polys = [[rng.randrange(R_MOD) for _ in range(d + 1)] for d in degs]
    blinds = [[rng.randrange(R_MOD) for _ in range(3)] for _ in range(K)]
    zs = [rng.randrange(R_MOD) for _ in range(K)]
    zs[5] = BETA                                                        # z = beta: beta_h - [z] h is infinity
    quots, vals, bquots, bvals = [], [], [], []
    for p, b, z in zip(polys, blinds, zs):
        q, v = ctx.poly_div_linear(mont(p), mont([z])[0])
        quots.append(unmont(q))
        vals.append(unmont(v)[0])
        q, v = ctx.poly_div_linear(mont(b), mont([z])[0])
        bquots.append(unmont(q))
        bvals.append(unmont(v)[0])
    assert vals[0] == sum(c * pow(zs[0], i, R_MOD) for i, c in enumerate(polys[0])) % R_MOD
    C, W = _g1(*_commit(ctx, bg, polys)), _g1(*_commit(ctx, bg, quots))
    Cb, Wb = _g1(*_commit(ctx, bgam, blinds)), _g1(*_commit(ctx, bgam, bquots))
    assert C[0] == P.g1_mul(sum(c * pow(BETA, i, R_MOD) for i, c in enumerate(polys[0])))      # the known-beta identity
    plain = {"comm": C, "w": W, "z": zs, "v": vals}
    hiding = {"comm": [P.g1_add(a, b) for a, b in zip(C, Cb)], "w": [P.g1_add(a, b) for a, b in zip(W, Wb)], "z": zs, "v": vals, "rv": bvals}
    const = rng.randrange(1, R_MOD)
    special = {"comm": [P.INF, P.g1_mul(const), C[5]], "w": [P.INF, P.INF, W[5]], "z": [zs[1], zs[2], BETA], "v": [0, const, vals[5]]}
    bg.release()
    bgam.release()
    return {"plain": plain, "hiding": hiding, "special": special}


def _arrays(o, idx=None):
    idx = range(len(o["z"])) if idx is None else idx
    comm, comm_inf = _g1_limbs([o["comm"][i] for i in idx])
    w, w_inf = _g1_limbs([o["w"][i] for i in idx])
    kw = {"comm_inf": comm_inf, "w_inf": w_inf}
    if "rv" in o:
        kw["random_v"] = mont([o["rv"][i] for i in idx])
    return (comm, mont([o["z"][i] for i in idx]), mont([o["v"][i] for i in idx]), w), kw


def _altered(o, field, i, rng):
    o = {k: list(v) for k, v in o.items()}
    if field in ("comm", "w"):
        o[field][i] = P.g1_add(o[field][i], P.g1_mul(rng.randrange(1, R_MOD)))
    else:
        o[field][i] = (o[field][i] + rng.randrange(1, R_MOD)) % R_MOD
    return o


# ------------------------------------------------------------------------------------------------- setup, trim, bytes
@pytest.mark.parametrize("max_degree", [1, 2, 63])
def test_setup_against_the_affine_group_law(ctx, pp, max_degree):
    from czk_amd import kzg
    s = pp if max_degree == D else kzg.setup(ctx, max_degree, BETA, GAMMA, produce_g2_powers=True)
    n = max_degree + 1
    assert s["powers_of_g"][0].shape == (n, 12) and s["powers_of_gamma_g"][0].shape == (n + 1, 12) and s["neg_powers_of_h"][0].shape == (n, 24)
    got_g, got_gg = _g1(*s["powers_of_g"]), _g1(*s["powers_of_gamma_g"])
    gamma_g = P.g1_mul(GAMMA)
    for i in sorted({0, 1, n - 1}):
        assert got_g[i] == P.g1_mul(pow(BETA, i, R_MOD)), i
    for i in sorted({0, 1, n - 1, n}):
        assert got_gg[i] == P.g1_mul(pow(BETA, i, R_MOD), gamma_g), i
    assert P.g2_from_limbs([int(v) for v in s["h"]], 0) == P.G2_GEN
    assert P.g2_from_limbs([int(v) for v in s["beta_h"]], 0) == P.g2_mul(BETA)
    inv = pow(BETA, -1, R_MOD)
    for i in sorted({0, 1, n - 1}):
        assert P.g2_from_limbs([int(v) for v in s["neg_powers_of_h"][0][i]], int(s["neg_powers_of_h"][1][i])) == P.g2_mul(pow(inv, i, R_MOD)), i
    # consecutive powers differ by beta everywhere: [beta] powers_of_g[i] == powers_of_g[i + 1], on the GPU and exactly
    nxt = ctx.points_mul(1, s["powers_of_g"][0][:-1], mont([BETA] * (n - 1)), scalar_form=1)
    assert np.array_equal(nxt[0], s["powers_of_g"][0][1:]) and not nxt[1].any()


def test_setup_with_given_bases_and_on_the_device(ctx, pp):
    from czk_amd import kzg
    g, h = P.g1_to_limbs(P.g1_mul(0xA11CE))[0], P.g2_to_limbs(P.g2_mul(0xB0B))[0]
    s = kzg.setup(ctx, 5, BETA, 0, g=g, gamma_g=P.g1_to_limbs(P.g1_mul(7))[0], h=h, to_host=False)
    assert s["neg_powers_of_h"] is None and s["powers_of_g"][0].is_cuda
    assert _g1(s["powers_of_g"][0].cpu().numpy().view(np.uint64), s["powers_of_g"][1].cpu().numpy())[5] == P.g1_mul(0xA11CE * pow(BETA, 5, R_MOD))
    assert _g1(s["powers_of_gamma_g"][0].cpu().numpy().view(np.uint64), s["powers_of_gamma_g"][1].cpu().numpy())[6] == P.g1_mul(7 * pow(BETA, 6, R_MOD))
    assert P.g2_from_limbs([int(v) for v in s["beta_h"]], 0) == P.g2_mul(0xB0B * BETA)
    powers, vk = kzg.trim(s, 5)
    assert np.array_equal(vk["g"], np.array(g, dtype=np.uint64)) and np.array_equal(vk["h"], np.array(h, dtype=np.uint64))


def test_trim_against_setup(pp):
    from czk_amd import kzg
    for d, keep in ((1, 3), (2, 3), (17, 18), (D, D + 1)):              # a supported degree of 1 is raised to 2 (mod.rs:456-458)
        powers, vk = kzg.trim(pp, d)
        assert np.array_equal(powers["powers_of_g"][0], pp["powers_of_g"][0][:keep]) and powers["powers_of_g"][1].shape == (keep,)
        assert np.array_equal(powers["powers_of_gamma_g"][0], pp["powers_of_gamma_g"][0][:keep])
        assert np.array_equal(vk["g"], pp["powers_of_g"][0][0]) and np.array_equal(vk["gamma_g"], pp["powers_of_gamma_g"][0][0])
        assert np.array_equal(vk["h"], pp["h"]) and np.array_equal(vk["beta_h"], pp["beta_h"])


@pytest.mark.parametrize("compressed,checked", [(True, True), (False, True), (False, False)])
def test_vk_byte_round_trip(ctx, vk, compressed, checked):
    from czk_amd import keyio
    data = keyio.kzg10_vk_to_bytes(ctx, vk, compressed)
    assert len(data) == (288 if compressed else 576)
    model = {"g": P.g1_mul(1), "gamma_g": P.g1_mul(GAMMA), "h": P.G2_GEN, "beta_h": P.g2_mul(BETA)}
    assert data == R.encode_struct((("g", 1, False), ("gamma_g", 1, False), ("h", 2, False), ("beta_h", 2, False)), model, compressed)
    back = keyio.kzg10_vk_from_bytes(ctx, data, compressed=compressed, checked=checked)
    for name in ("g", "gamma_g", "h", "beta_h"):
        assert np.array_equal(getattr(back, name), getattr(vk, name)), name
    back.release()
    if checked:                                                         # a point outside the subgroup is refused by the checked forms
        bad = bytearray(data)
        bad[0:48 if compressed else 96] = R.encode_point(1, (0, 1), compressed)      # the order-3 point
        with pytest.raises(ValueError, match="g is not a valid G1 point"):
            keyio.kzg10_vk_from_bytes(ctx, bytes(bad), compressed=compressed, checked=True)


# ------------------------------------------------------------------------------------------------- check
@pytest.mark.parametrize("kind", ["plain", "hiding"])
@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_honest_openings_verify(ctx, vk, openings, kind, k):
    from czk_amd import kzg
    args, kw = _arrays(openings[kind], range(k))
    ok = kzg.check(ctx, vk, *args, **kw)
    assert ok.shape == (k,) and ok.all()


@pytest.mark.parametrize("field", ["v", "z", "w", "comm", "rv"])
def test_a_wrong_field_flips_only_its_own_verdict(ctx, vk, openings, field):
    from czk_amd import kzg
    rng = random.Random(sum(map(ord, field)))
    for k, i in ((8, 3), (65, 64)):
        args, kw = _arrays(_altered(openings["hiding"], field, i, rng), range(k))
        want = np.ones(k, dtype=bool)
        want[i] = False
        assert np.array_equal(kzg.check(ctx, vk, *args, **kw), want), (field, k)


def test_zero_constant_and_z_equal_beta_verify(ctx, vk, openings):
    from czk_amd import kzg
    args, kw = _arrays(openings["special"])
    assert list(kw["comm_inf"]) == [1, 0, 0] and list(kw["w_inf"]) == [1, 1, 0]
    assert kzg.check(ctx, vk, *args, **kw).all()
    assert kzg.check(ctx, vk, *args, random_v=mont([0, 0, 0]), **kw).all()      # rv = 0 decides as None
    bad = _altered(openings["special"], "v", 1, random.Random(3))               # a constant polynomial with the wrong constant
    args, kw = _arrays(bad)
    assert list(kzg.check(ctx, vk, *args, **kw)) == [True, False, True]
    assert kzg.check(ctx, vk, *[a[:0] for a in args]).shape == (0,)


def test_four_verdicts_recomputed_by_the_pairing_restatement(ctx, vk, openings):
    """e(C - [v] g - [rv] gamma_g, h) e(-W, beta_h - [z] h) through tests/pairing_ref.py for an honest and an altered opening of each kind"""
    from czk_amd import kzg
    rng = random.Random(11)
    hid = openings["hiding"]
    cases = [(openings["plain"], 1), (_altered(openings["plain"], "v", 1, rng), 1), (hid, 2), (_altered(hid, "rv", 2, rng), 2)]
    got, want = [], []
    gamma_g, beta_h = P.g1_mul(GAMMA), P.g2_mul(BETA)
    for o, i in cases:
        args, kw = _arrays(o, [i])
        got.append(bool(kzg.check(ctx, vk, *args, **kw)[0]))
        inner = P.g1_add(o["comm"][i], P.ec_neg(P.F1, P.g1_mul(o["v"][i])))
        if "rv" in o:
            inner = P.g1_add(inner, P.ec_neg(P.F1, P.g1_mul(o["rv"][i], gamma_g)))
        q = P.ec_add(P.F2, beta_h, P.ec_neg(P.F2, P.g2_mul(o["z"][i])))
        want.append(P.product_of_pairings([(inner, P.G2_GEN), (P.ec_neg(P.F1, o["w"][i]), q)]) == P.FQ12_ONE)
    assert got == want == [True, False, True, False]


# ------------------------------------------------------------------------------------------------- batch_check
BATCHES = ([], [0], [1, 2], list(range(K)))                             # sizes 0, 1, 2 and 65 in one call


def _batched(o, batches=BATCHES):
    idx = [i for b in batches for i in b]
    args, kw = _arrays(o, idx)
    return args, kw, list(np.cumsum([0] + [len(b) for b in batches])), idx


@pytest.mark.parametrize("kind", ["plain", "hiding"])
def test_batches_of_honest_openings_verify(ctx, vk, openings, kind):
    from czk_amd import kzg
    args, kw, offs, _ = _batched(openings[kind])
    ok = kzg.batch_check(ctx, vk, *args, offsets=offs, rng=random.Random(5), **kw)
    assert list(ok) == [True] * 4
    assert kzg.batch_check(ctx, vk, *args, **kw).shape == (1,)          # offsets None: one batch of everything
    assert list(kzg.batch_check(ctx, vk, *[a[:0] for a in args], offsets=[0, 0])) == [True]


@pytest.mark.parametrize("field,batch,pos", [("v", 1, 0), ("w", 2, 1), ("rv", 3, 64), ("comm", 3, 0), ("z", 3, 33)])
def test_one_bad_opening_fails_only_its_batch(ctx, vk, openings, field, batch, pos):
    from czk_amd import kzg
    i = BATCHES[batch][pos]
    honest = openings["hiding"]
    o = _altered(honest, field, i, random.Random(pos))
    # every batch gathers its own openings: only the chosen batch reads the altered one (opening i is also a member of other batches, honest there)
    mixed = {k: [(o if bi == batch else honest)[k][j] for bi, b in enumerate(BATCHES) for j in b] for k in o}
    args, kw = _arrays(mixed)
    offs = list(np.cumsum([0] + [len(b) for b in BATCHES]))
    ok = kzg.batch_check(ctx, vk, *args, offsets=offs, rng=random.Random(7), **kw)
    assert list(ok) == [bi != batch for bi in range(4)]


def test_the_formula_is_the_references(ctx, vk, openings):
    """v_0 + d and v_1 - d cancel in sum r_i v_i under the randomizers (1, 1) and not under (1, 2): the multiplier of g is sum r_i v_i"""
    from czk_amd import kzg
    o = {k: list(v) for k, v in openings["hiding"].items()}
    d = 0x1234567
    o["v"][0], o["v"][1] = (o["v"][0] + d) % R_MOD, (o["v"][1] - d) % R_MOD
    args, kw = _arrays(o, [0, 1])
    assert list(kzg.check(ctx, vk, *args, **kw)) == [False, False]
    r = lambda *ks: ints_to_limbs(list(ks), 4)
    assert list(kzg.batch_check(ctx, vk, *args, randomizers=r(1, 1), **kw)) == [True]
    assert list(kzg.batch_check(ctx, vk, *args, randomizers=r(1, 2), **kw)) == [False]
    assert list(kzg.batch_check(ctx, vk, *args, randomizers=r(0, 0), **kw)) == [True]       # all-zero randomizers accept anything
    honest, hkw = _arrays(openings["hiding"], [0, 1])
    assert list(kzg.batch_check(ctx, vk, *honest, randomizers=r(1, (1 << 128) - 1), **hkw)) == [True]
    assert list(kzg.batch_check(ctx, vk, *honest, randomizers=r(R_MOD - 1, 2), **hkw)) == [True]


# ------------------------------------------------------------------------------------------------- the provers' openings
def _prove(workload):
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    if workload == "plonk":
        B = polyvm.GpuBackend(czk_amd, ctx, 3, polyvm.plonk_max_degree(64))
        out = polyvm.plonk_prove(B, polyvm.plonk_inputs(B, 64))
    else:
        B = polyvm.GpuBackend(czk_amd, ctx, 4, polyvm.marlin_max_degree(64), lift=(1, 1, 0, 0))
        out = polyvm.marlin_prove(B, polyvm.marlin_inputs(B, 64))
    return ctx, B, out


@pytest.mark.parametrize("workload", ["plonk", "marlin"])
def test_check_openings_accepts_a_proof_and_rejects_an_altered_evaluation(workload):
    from czk_amd import kzg
    ctx, B, out = _prove(workload)
    try:
        vk = B.verifier_key()
        assert P.g1_from_limbs([int(v) for v in vk[0]], 0) == P.G1_GEN and P.g2_from_limbs([int(v) for v in vk[3]], 0) == P.g2_mul(B.tau)
        verdicts = kzg.check_openings(B, out, rng=random.Random(1), details=True)
        labels = [k for k, o in out.items() if isinstance(o, dict) and (o.get("of") or k in ("open_beta", "open_gamma"))]
        assert sorted(verdicts) == sorted(labels) and len(labels) >= 2 and all(verdicts.values())
        if workload == "marlin":
            assert {"open_beta", "open_gamma"} <= set(labels) and any("random_v" in out[k] for k in labels)
        assert kzg.check_openings(B, out) is True
        victim = labels[-1]
        bad = dict(out)
        bad[victim] = dict(out[victim])
        value = np.array(out[victim]["value"], dtype=np.uint64, copy=True)
        value[0] = mont([unmont(value[0])[0] + 1])[0]
        bad[victim]["value"] = value
        verdicts = kzg.check_openings(B, bad, rng=random.Random(2), details=True)
        assert verdicts == {k: k != victim for k in labels}
        assert kzg.check_openings(B, bad) is False
    finally:
        ctx.close()
