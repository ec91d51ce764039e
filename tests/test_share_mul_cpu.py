"""The big-integer model of the shared-value protocols (tests/share_mul_model.py): with a dealer's random material and with the reference's dummy
material the outputs open to the product, the inverse and the running product of the opened inputs, the MAC lanes to alpha times the same, and the
material consumed is what czk_share_material_counts reports.  No GPU."""
import os
import random
import re

import pytest

import share_mul_model as M
from share_mul_model import R_MOD, Scheme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(lpp, parties) for lpp in (1, 2) for parties in (1, 2, 3)]
SIZES = (1, 2, 33)


def _scheme(lpp, parties, seed):
    rng = random.Random(seed)
    return Scheme(lpp, parties, [rng.randrange(R_MOD) for _ in range(parties)] if lpp == 2 else None), rng


def _material(S, kind, op, n, seed):
    return M.random_material(S, op, n, seed) if kind == "random" else M.dummy_material(S, op, n)


def _check_opens_to(S, out, want):
    vals, bad = S.batch_open(out)
    assert bad == 0 and vals == [w % R_MOD for w in want]
    if S.lpp == 2:
        assert S.mac_opened(out) == [S.alpha * w % R_MOD for w in want]


@pytest.mark.parametrize("kind", ["random", "dummy"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lpp,parties", CONFIGS)
def test_batch_mul_opens_to_the_product(lpp, parties, n, kind):
    S, rng = _scheme(lpp, parties, 100 + n)
    x = [rng.randrange(R_MOD) for _ in range(n)]
    y = [rng.randrange(R_MOD) for _ in range(n)]
    src = _material(S, kind, M.OP_MUL, n, 7)
    out, bad = M.batch_mul(S, S.share(x, rng), S.share(y, rng), src)
    assert bad == 0 and (src.t, src.p) == M.material_counts(M.OP_MUL, n)
    _check_opens_to(S, out, [a * b for a, b in zip(x, y)])


def test_batch_mul_with_random_triples_tells_the_operands_apart():
    """the dummy triples are symmetric in x and y; a random triple used with its shares swapped opens to something else"""
    S, rng = _scheme(2, 2, 5)
    x, y = [rng.randrange(R_MOD) for _ in range(4)], [rng.randrange(R_MOD) for _ in range(4)]
    xs, ys = S.share(x, rng), S.share(y, rng)
    src = M.random_material(S, M.OP_MUL, 4, 9)
    swapped = M.Material(src.ty, src.tx, src.tz, src.pb, src.pc)
    good, _ = M.batch_mul(S, xs, ys, src)
    also_good, _ = M.batch_mul(S, xs, ys, swapped)             # (y, x, z) is a triple too: same opened product, other shares
    assert S.opened(good) == S.opened(also_good) == [a * b % R_MOD for a, b in zip(x, y)] and good != also_good
    wrong = M.Material(src.tx, src.tz, src.ty, src.pb, src.pc)  # z in y's place is no triple
    assert S.opened(M.batch_mul(S, xs, ys, wrong)[0]) != S.opened(good)


@pytest.mark.parametrize("kind", ["random", "dummy"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lpp,parties", CONFIGS)
def test_batch_inv_opens_to_the_inverse(lpp, parties, n, kind):
    S, rng = _scheme(lpp, parties, 200 + n)
    x = [rng.randrange(1, R_MOD) for _ in range(n)]
    src = _material(S, kind, M.OP_INV, n, 8)
    out, bad, zero = M.batch_inv(S, S.share(x, rng), src)
    assert (bad, zero) == (0, 0) and (src.t, src.p) == M.material_counts(M.OP_INV, n)
    _check_opens_to(S, out, [pow(v, -1, R_MOD) for v in x])


@pytest.mark.parametrize("lpp,parties", CONFIGS)
def test_batch_inv_counts_a_zero_divisor(lpp, parties):
    S, rng = _scheme(lpp, parties, 31)
    x = [rng.randrange(1, R_MOD) for _ in range(5)]
    x[1] = x[4] = 0
    out, bad, zero = M.batch_inv(S, S.share(x, rng), _material(S, "random", M.OP_INV, 5, 3))
    assert (bad, zero) == (0, 2)
    assert all(lane[1] == 0 and lane[4] == 0 for lane in out)                      # zero on every lane, not just in the sum
    assert S.opened(out) == [pow(v, -1, R_MOD) if v else 0 for v in x]


@pytest.mark.parametrize("kind", ["random", "dummy"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("lpp,parties", CONFIGS)
def test_partial_products_open_to_the_running_product(lpp, parties, n, kind):
    S, rng = _scheme(lpp, parties, 300 + n)
    x = [rng.randrange(1, R_MOD) for _ in range(n)]
    src = _material(S, kind, M.OP_PARTIAL_PRODUCTS, n, 11)
    out, bad, zero = M.partial_products(S, S.share(x, rng), src)
    assert (bad, zero) == (0, 0) and (src.t, src.p) == M.material_counts(M.OP_PARTIAL_PRODUCTS, n)
    want, run = [], 1
    for v in x:
        run = run * v % R_MOD
        want.append(run)
    _check_opens_to(S, out, want)


@pytest.mark.parametrize("lpp,parties", CONFIGS)
def test_partial_products_with_a_zero_input_open_to_zero_from_there_on(lpp, parties):
    S, rng = _scheme(lpp, parties, 41)
    n = 33
    x = [rng.randrange(1, R_MOD) for _ in range(n)]
    x[17] = 0
    out, bad, zero = M.partial_products(S, S.share(x, rng), _material(S, "random", M.OP_PARTIAL_PRODUCTS, n, 13))
    assert (bad, zero) == (0, 0)                                                   # the divisors are m_0 / m_{i+1}: never zero
    got = S.opened(out)
    assert all(got[:17]) and got[17:] == [0] * (n - 17)


def test_a_broken_mac_is_counted_under_spdz_only():
    for lpp in (1, 2):
        S, rng = _scheme(lpp, 2, 51)
        x, y = S.share([3, 4, 5], rng), S.share([6, 7, 8], rng)
        x[lpp * 1 + lpp - 1][2] ^= 1                                               # party 1's last lane: its mac (SPDZ) or its only share (additive)
        out, bad = M.batch_mul(S, x, y, M.random_material(S, M.OP_MUL, 3, 1))
        assert bad == (1 if lpp == 2 else 0)


def test_material_counts_are_the_formulas_of_the_c_call():
    """czk_share_material_counts in csrc/share_mul.hip: T = n / n / 4 n, P = 0 / n / 2 n + 1"""
    src = open(os.path.join(ROOT, "collaborative-zksnark_amd", "csrc", "share_mul.hip")).read()
    body = src[src.index('extern "C" int czk_share_material_counts'):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"case CZK_SHARE_OP_MUL: \*triples = n; return", body)
    assert re.search(r"case CZK_SHARE_OP_INV: \*triples = n, \*pairs = n; return", body)
    assert re.search(r"case CZK_SHARE_OP_PARTIAL_PRODUCTS: \*triples = 4 \* n, \*pairs = n \? 2 \* n \+ 1 : 0; return", body)
    hdr = open(os.path.join(ROOT, "include", "czk.h")).read()
    for name, val in (("MUL", M.OP_MUL), ("INV", M.OP_INV), ("PARTIAL_PRODUCTS", M.OP_PARTIAL_PRODUCTS)):
        assert re.search(rf"#define CZK_SHARE_OP_{name} {val}\b", hdr)
    for n in (0, 1, 2, 33):
        assert M.material_counts(M.OP_MUL, n) == (n, 0) and M.material_counts(M.OP_INV, n) == (n, n)
        assert M.material_counts(M.OP_PARTIAL_PRODUCTS, n) == (4 * n, 2 * n + 1 if n else 0)


def test_limb_round_trip():
    v = [[0, 1, R_MOD - 1, 12345678901234567890123]]
    assert M.from_limbs(M.to_limbs(v)) == v
    assert [int(w) for w in M.to_limbs([[1]])[0, 0]] == [(M.MONT_R >> (64 * j)) & (2**64 - 1) for j in range(4)]
