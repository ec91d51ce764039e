"""The big-integer model of the GSZ products and their product check (tests/gsz_mul_model.py) against plain arithmetic, on random degree-t
sharings: products open to products, inverses to inverses, running products to running products; the check accepts honest triples and rejects a
wrong z; the consumed material is what material_counts says; and the king's degree bound catches a wrong contribution exactly when it is not
vacuous (2t < parties - 1), which is why 3 parties need the product check.  No GPU."""
import random

import pytest

import gsz_mul_model as M
from gsz_mul_model import R_MOD

PARTIES = [3, 4, 6, 8]
SIZES = [1, 2, 3, 5, 8, 33]


def _setup(parties, n, seed=0):
    D = M.Domain(parties)
    t = M.threshold(parties)
    rng = random.Random(1000 * parties + n + seed)
    xv = [rng.randrange(1, R_MOD) for _ in range(n)]
    yv = [rng.randrange(R_MOD) for _ in range(n)]
    return D, t, rng, xv, yv


def test_share_domain_is_a_subgroup_of_that_order():
    for parties in PARTIES + [1, 2, 12, 96]:
        D = M.Domain(parties)
        assert pow(D.w, parties, R_MOD) == 1 and all(pow(D.w, parties // q, R_MOD) != 1 for q in (2, 3) if parties % q == 0)
    for parties in (5, 7, 9, 18):
        with pytest.raises(ValueError):
            M.Domain(parties)


@pytest.mark.parametrize("parties", PARTIES)
def test_products_inverses_and_running_products_open_to_the_plain_ones(parties):
    for n in SIZES:
        D, t, rng, xv, yv = _setup(parties, n)
        x, y = D.share(xv, t, rng), D.share(yv, t, rng)
        src = M.random_material(D, t, M.OP_MUL, n, seed=n)
        z, bad = M.batch_mult(D, t, x, y, src)
        assert bad == 0 and D.batch_open(z, t) == ([a * b % R_MOD for a, b in zip(xv, yv)], 0)
        assert (src.d, src.r) == M.material_counts(M.OP_MUL, n)
        src = M.random_material(D, t, M.OP_INV, n, seed=n)
        inv, bad, zero = M.batch_inv(D, t, x, src)
        assert (bad, zero) == (0, 0) and D.batch_open(inv, t) == ([pow(a, -1, R_MOD) for a in xv], 0)
        assert (src.d, src.r) == M.material_counts(M.OP_INV, n)
        src = M.random_material(D, t, M.OP_PARTIAL_PRODUCTS, n, seed=n)
        pp, bad, zero = M.partial_products(D, t, x, src)
        run, want = 1, []
        for a in xv:
            run = run * a % R_MOD
            want.append(run)
        assert (bad, zero) == (0, 0) and D.batch_open(pp, t) == (want, 0)
        assert (src.d, src.r) == M.material_counts(M.OP_PARTIAL_PRODUCTS, n)


@pytest.mark.parametrize("parties", PARTIES)
def test_the_check_accepts_honest_triples_and_rejects_a_wrong_product(parties):
    for n in SIZES:
        D, t, rng, xv, yv = _setup(parties, n, seed=5)
        x, y = D.share(xv, t, rng), D.share(yv, t, rng)
        z, _ = M.batch_mult(D, t, x, y, M.random_material(D, t, M.OP_MUL, n, seed=n))
        src = M.random_material(D, t, M.OP_PRODUCT_CHECK, n, seed=3 * n)
        assert M.hadamard_check(D, t, x, y, z, src) == (True, 0)
        assert (src.d, src.r) == M.material_counts(M.OP_PRODUCT_CHECK, n)
        one = D.share([1], t, rng)                                   # a consistent sharing of 1 added to one z: every degree test still passes
        at = n // 2
        z2 = [list(ln) for ln in z]
        for j in range(parties):
            z2[j][at] = (z2[j][at] + one[j][0]) % R_MOD
        src = M.random_material(D, t, M.OP_PRODUCT_CHECK, n, seed=3 * n)
        assert M.hadamard_check(D, t, x, y, z2, src) == (False, 0)
        assert (src.d, src.r) == M.material_counts(M.OP_PRODUCT_CHECK, n)


@pytest.mark.parametrize("parties", PARTIES)
def test_a_wrong_king_input_is_caught_by_the_degree_bound_exactly_when_it_is_not_vacuous(parties):
    n = 5
    D, t, rng, xv, yv = _setup(parties, n, seed=9)
    x, y = D.share(xv, t, rng), D.share(yv, t, rng)

    def plus_one(masked):
        masked[1][2] = (masked[1][2] + 1) % R_MOD                    # party 1's x y + r2 for element 2

    z, bad = M.batch_mult(D, t, x, y, M.random_material(D, t, M.OP_MUL, n, seed=1), tamper=plus_one)
    assert (bad == 1) == (2 * t < parties - 1) and (bad == 0) == (parties == 3)
    if parties == 3:
        # not caught: the products are still consistent degree-t shares, of a wrong value -- only the product check sees it
        vals, b = D.batch_open(z, t)
        assert b == 0 and vals[2] != xv[2] * yv[2] % R_MOD and vals[:2] == [a * c % R_MOD for a, c in zip(xv[:2], yv[:2])]
        assert M.hadamard_check(D, t, x, y, z, M.random_material(D, t, M.OP_PRODUCT_CHECK, n, seed=2)) == (False, 0)


def test_dummy_material_and_public_shares_are_the_stand_in_case():
    """the reference's stubs: every party holds the value itself, every random share is one -- the products are the lane-wise products"""
    D = M.Domain(3)
    x, y = D.public([5, 7, 11]), D.public([2, 3, 4])
    z, bad = M.batch_mult(D, 1, x, y, M.dummy_material(D, M.OP_MUL, 3))
    assert bad == 0 and z == D.public([10, 21, 44])
    assert M.hadamard_check(D, 1, x, y, z, M.dummy_material(D, M.OP_PRODUCT_CHECK, 3)) == (True, 0)


def test_material_counts_follow_the_source():
    assert [M.material_counts(M.OP_PRODUCT_CHECK, n) for n in (0, 1, 2, 3, 5, 8, 33, 1025)] == [(0, 0), (4, 3), (6, 4), (8, 5), (10, 6), (10, 6), (16, 9), (26, 14)]
    assert M.material_counts(M.OP_PARTIAL_PRODUCTS, 7) == (36, 23) and M.material_counts(M.OP_INV, 7) == (7, 7) and M.material_counts(M.OP_MUL, 7) == (7, 0)


def test_the_library_reports_the_models_material_counts():
    """czk_gsz_material_counts needs no GPU: every op at the sizes of the halving's corner cases, the unknown op and the overflow"""
    import ctypes as C

    import czk_amd
    L = czk_amd.lib()

    def counts(op, n):
        d, r = C.c_size_t(7), C.c_size_t(7)
        return L.czk_gsz_material_counts(C.c_int(op), C.c_size_t(n), C.byref(d), C.byref(r)), (d.value, r.value)
    for op in (M.OP_MUL, M.OP_INV, M.OP_PARTIAL_PRODUCTS, M.OP_PRODUCT_CHECK):
        for n in (0, 1, 2, 3, 4, 5, 8, 9, 33, 1024, 1025, 3 << 18):
            assert counts(op, n) == (0, M.material_counts(op, n)), (op, n)
        assert counts(op, 1 << 60) == (1, (0, 0))                    # CZK_ERR_SIZE
    assert counts(4, 8) == (3, (0, 0))                               # CZK_ERR_ARG
    assert L.czk_gsz_material_counts(C.c_int(0), C.c_size_t(8), None, None) == 3
