"""CPU checks of the pairing restatement (tests/pairing_ref.py) and of the constants the kernels use (csrc/pairing_constants.inc).

The GPU tests (tests/test_pairing.py) hold the kernels to pairing_ref bit for bit, so pairing_ref itself is pinned here on the pairing's
defining properties, and the Frobenius coefficients it and tools/gen_pairing_constants.py derive from q are compared with the reference's
text through tests/golden/pairing_constants.json (written by tests/golden/make_pairing_constants.py), and with the tree itself where it
is readable."""
import importlib.util
import json
import os
import subprocess
import sys

import pairing_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_pairing_constants", os.path.join(GOLDEN, "make_pairing_constants.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)


def test_pairing_is_non_degenerate_and_of_order_r():
    e = P.pairing(P.G1_GEN, P.G2_GEN)
    assert e != P.FQ12_ONE
    assert P.fq12_pow(e, P.R_MOD) == P.FQ12_ONE
    # the reference's chain (eprint 2020/875) is the cube of the plain final exponentiation: pins every step of it
    f = P.miller_loop([(P.G1_GEN, P.G2_GEN)])
    assert P.fq12_pow(f, 3 * ((P.Q ** 12 - 1) // P.R_MOD)) == e


def test_bilinearity():
    e = P.pairing(P.G1_GEN, P.G2_GEN)
    for a, b in ((0x1234567, 0x89ABCDEF), (P.R_MOD - 3, 2 ** 200 + 12345)):
        ab = a * b % P.R_MOD
        want = P.fq12_pow(e, ab)
        assert P.pairing(P.g1_mul(a), P.g2_mul(b)) == want
        assert P.pairing(P.g1_mul(ab), P.G2_GEN) == want
        assert P.pairing(P.G1_GEN, P.g2_mul(ab)) == want
    # products: e(P, Q) e(-P, Q) = 1
    p = P.g1_mul(99)
    assert P.product_of_pairings([(p, P.G2_GEN), (P.ec_neg(P.F1, p), P.G2_GEN)]) == P.FQ12_ONE


def test_infinity_on_either_side_gives_one():
    assert P.pairing(P.INF, P.G2_GEN) == P.FQ12_ONE
    assert P.pairing(P.G1_GEN, P.INF) == P.FQ12_ONE
    assert P.product_of_pairings([]) == P.FQ12_ONE
    assert P.product_of_pairings([(P.INF, P.G2_GEN), (P.G1_GEN, P.G2_GEN)]) == P.pairing(P.G1_GEN, P.G2_GEN)


def test_g2_prepared_has_69_lines():
    assert len(P.X_BITS) == 63 and sum(P.X_BITS) == 6
    assert len(P.g2_prepare(P.G2_GEN)) == 69 and P.g2_prepare(P.INF) == []


def test_limb_layout_round_trips():
    e = P.pairing(P.g1_mul(5), P.G2_GEN)
    limbs = P.fq12_to_limbs(e)
    assert len(limbs) == 72 and P.fq12_from_limbs(limbs) == e
    assert P.fq12_to_limbs(P.FQ12_ONE)[:6] == [int(x) for x in P.pyref.FQ_R_LIMBS]


def test_verify_proof_restatement():
    """verify_proof with points whose discrete logs satisfy a b = alpha beta + x_gamma gamma + c delta, and a tampered proof."""
    al, be, ga, de, c, x = 11, 13, 17, 19, 23, 29
    abc = [31, 37]
    pub = (abc[0] + x * abc[1]) % P.R_MOD
    rhs = (al * be + pub * ga + c * de) % P.R_MOD
    a = 41
    b = rhs * pow(a, -1, P.R_MOD) % P.R_MOD
    ab = P.pairing(P.g1_mul(al), P.g2_mul(be))
    args = (ab, P.g2_mul(ga), P.g2_mul(de), [P.g1_mul(v) for v in abc])
    assert P.verify_proof(*args, P.g1_mul(a), P.g2_mul(b), P.g1_mul(c), [x])
    assert not P.verify_proof(*args, P.g1_mul(a + 1), P.g2_mul(b), P.g1_mul(c), [x])
    try:
        P.verify_proof(*args, P.g1_mul(a), P.g2_mul(b), P.g1_mul(c), [x, x])
        raise AssertionError("wrong input count accepted")
    except ValueError as exc:
        assert "MalformedVerifyingKey" in str(exc)


def _fixture():
    fx = json.load(open(os.path.join(GOLDEN, "pairing_constants.json")))
    return {k: ([[int(a), int(b)] for a, b in v] if not k.startswith("_") else v) for k, v in fx.items()}


def _render_rust(name, coeffs):
    """The fixture's values in the reference's constant forms (FQ_ONE / FQ_ZERO / field_new! with a decimal string, "-1"), each entry
    preceded by a comment carrying a wrong value: the parser must read them back."""
    def fq(v):
        if v == 0:
            return "FQ_ZERO"
        if v == 1:
            return "FQ_ONE"
        if v == P.Q - 1:
            return 'field_new!(Fq, "-1")'
        return f'field_new!(Fq, "{v}")'
    body = "".join(f'        // field_new!(Fq, "7")\n        field_new!(Fq2,\n            {fq(a)},\n            {fq(b)},\n        ),\n' for a, b in coeffs)
    return f"    const {name}: &'static [Fq2] = &[\n{body}    ];\n"


def test_frobenius_coefficients_equal_the_reference_text():
    fx = _fixture()
    derived = P.frobenius_coefficients()
    assert set(derived) == {k for k in fx if not k.startswith("_")}
    assert [len(fx[k]) for k in sorted(derived)] == [12, 6, 6]
    for name, vals in derived.items():
        assert [list(v) for v in vals] == fx[name], name
        assert mk.parse_coefficients(_render_rust(name, fx[name]), name) == fx[name], name
    assert set(fx["_sha256"]) == set(mk.FILES.values())
    if all(os.access(os.path.join("/root/reference", rel), os.R_OK) for rel in mk.FILES.values()):
        now = mk.read_reference("/root/reference")
        assert {k: v for k, v in now.items()} == fx


def test_pairing_constants_inc_is_generated_and_current():
    """csrc/pairing_constants.inc is what tools/gen_pairing_constants.py writes (its derivation agrees with pairing_ref's)."""
    gen = os.path.join(ROOT, "tools", "gen_pairing_constants.py")
    assert subprocess.run([sys.executable, gen, "--check"]).returncode == 0
    spec = importlib.util.spec_from_file_location("gen_pairing_constants", gen)
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    c, two_inv, b2 = g.derive()
    assert c == P.frobenius_coefficients() and two_inv == P.TWO_INV and b2 == tuple(P.G2_B)
