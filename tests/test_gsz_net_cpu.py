"""The per-party restatement of the GSZ products and product check (tests/gsz_net_model.py: one Party per lane, exchanges only through a recording
net) against the lanes model (tests/gsz_mul_model.py): the same lanes, counts and verdict, the exchange counts include/czk.h states for czk_net_gsz_*,
and the order in which committed values and coins travel.  No GPU."""
import functools
import os
import random
import re

import pytest

import gsz_mul_model as M
import gsz_net_model as N
from gsz_mul_model import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTIES = [3, 4, 8]
SIZES = [1, 2, 3, 5, 33]


@functools.lru_cache(maxsize=None)
def _domain(parties):
    return M.Domain(parties)


def _inputs(parties, n, seed):
    D, t = _domain(parties), M.threshold(parties)
    rng = random.Random(seed)
    return D, t, D.share([rng.randrange(1, R_MOD) for _ in range(n)], t, rng), D.share([rng.randrange(R_MOD) for _ in range(n)], t, rng), rng


def _run(D, t, src, call):
    """call(party, rank) -> that party's generator; -> (results per rank, parties, net)"""
    ps = N.parties_of(D, t, src)
    net = N.RecordingNet(D.parties)
    return N.run(net, [call(p, j) for j, p in enumerate(ps)]), ps, net


def _counts_agree(ps, bad, zero):
    """the model's counts, split the way the ranks see them: the king's bound on rank 0 only, plain opens and zero divisors everywhere"""
    assert ps[0].bad == bad and all(p.zero == zero for p in ps)
    assert all(p.king_bad == 0 and p.bad == bad - ps[0].king_bad for p in ps[1:])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("parties", PARTIES)
def test_products_per_party_equal_the_lanes_model(parties, n):
    D, t, x, y, _ = _inputs(parties, n, 9 * n + parties)
    for op, code in (("mul", M.OP_MUL), ("inv", M.OP_INV), ("pp", M.OP_PARTIAL_PRODUCTS)):
        if op == "mul":
            want, bad = M.batch_mult(D, t, x, y, M.random_material(D, t, code, n, seed=n))
            zero = 0
        else:
            want, bad, zero = (M.batch_inv if op == "inv" else M.partial_products)(D, t, x, M.random_material(D, t, code, n, seed=n))
        src = M.random_material(D, t, code, n, seed=n)
        got, ps, net = _run(D, t, src, lambda p, j: p.batch_mul(x[j], y[j]) if op == "mul" else (p.batch_inv if op == "inv" else p.partial_products)(x[j]))
        assert got == want, op
        assert (bad, zero) == (0, 0)
        _counts_agree(ps, bad, zero)
        assert all((p.d, p.r) == M.material_counts(code, n) for p in ps), op
        assert net.counts() == N.exchange_counts(op, n), op


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("parties", PARTIES)
def test_check_per_party_gives_the_lanes_verdict_counts_and_exchange_order(parties, n):
    D, t, x, y, rng = _inputs(parties, n, 31 * n + parties)
    z, _ = M.batch_mult(D, t, x, y, M.random_material(D, t, M.OP_MUL, n, seed=n))
    one = D.share([1], t, rng)
    wrong = [ln[:-1] + [(ln[-1] + o[0]) % R_MOD] for ln, o in zip(z, one)]       # a consistent sharing of a wrong last product
    for zs, tamper, verdict in ((z, False, True), (wrong, False, False), (z, True, None)):
        def material():
            src = M.random_material(D, t, M.OP_PRODUCT_CHECK, n, seed=5 * n + 1)
            if tamper:                                                           # party 1's share of the last double's r2 and of the first coin
                src.dr2[1][-1] = (src.dr2[1][-1] + 1) % R_MOD
                src.rands[1][0] = (src.rands[1][0] + 1) % R_MOD
            return src
        ok, bad = M.hadamard_check(D, t, x, y, zs, material())
        got, ps, net = _run(D, t, material(), lambda p, j: p.product_check(list(x[j]), list(y[j]), list(zs[j])))
        assert got == [ok] * parties and (verdict is None or ok == verdict)      # the verdict, the same on every party
        _counts_agree(ps, bad, 0)
        if tamper:
            assert bad == (2 if 2 * t < parties - 1 else 1) and ps[0].king_bad == bad - 1
        assert all((p.d, p.r) == M.material_counts(M.OP_PRODUCT_CHECK, n) for p in ps)
        R = M.ceil_log2(n)
        assert net.counts() == N.exchange_counts("check", n) == (R + 2, R + 2, R + 2)
        # what travels, per party: 2 R + 4 elements to the king, R + 4 broadcast
        assert sum(k for kind, _, k in net.log if kind == "to_king") == 2 * R + 4 and sum(k for kind, _, k in net.log if kind == "broadcast") == R + 4
        # a round's coin leaves only after the king round trip that carries ip_l and ip3 of that round has come back
        tags = [(kind, tag) for kind, tag, _ in net.log]
        assert tags[0] == ("broadcast", ("coin", "hadamard"))
        for r in range(R):
            committed = tags.index(("from_king", ("ip", r)))
            assert tags.index(("to_king", ("ip", r))) < committed < tags.index(("broadcast", ("coin", r)))
            assert [k for _, tag, k in net.log if tag == ("ip", r)] == [2, 2]    # both inner products in ONE round trip
            if r:
                assert tags.index(("broadcast", ("coin", r - 1))) < tags.index(("to_king", ("ip", r)))
        assert tags[-5:] == [("to_king", ("final", 0)), ("from_king", ("final", 0)), ("to_king", ("final", 1)), ("from_king", ("final", 1)),
                             ("broadcast", ("blind", 0))]


def test_a_wrong_contribution_to_the_king_is_seen_by_rank_0_alone_at_4_parties_and_by_nobody_at_3():
    n = 8
    for parties in (4, 3):
        D, t, x, y, _ = _inputs(parties, n, 77)
        x2 = [list(ln) for ln in x]
        x2[1][5] = (x2[1][5] + 1) % R_MOD
        want, _ = M.batch_mult(D, t, x, y, M.random_material(D, t, M.OP_MUL, n, seed=3))
        got, ps, _ = _run(D, t, M.random_material(D, t, M.OP_MUL, n, seed=3), lambda p, j: p.batch_mul(x2[j], y[j]))
        if parties == 4:
            assert ps[0].bad == ps[0].king_bad == 1 and all(p.bad == 0 for p in ps[1:])
            continue
        assert all(p.bad == 0 for p in ps) and got != want
        z = got
        ok, ps, _ = _run(D, t, M.random_material(D, t, M.OP_PRODUCT_CHECK, n, seed=4), lambda p, j: p.product_check(list(x[j]), list(y[j]), list(z[j])))
        assert ok == [False] * 3 and all(p.bad == 0 for p in ps)


def test_the_header_states_the_exchange_counts_the_model_makes():
    h = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(ROOT, "include", "czk.h")).read())
    for text in ("batch_mul 1 king round trip", "batch_inv 1 king round trip, then 1 broadcast", "partial_products 5 king round trips, 3 broadcasts",
                 "product_check R + 2 king round trips, R + 2 broadcasts"):
        assert text in re.sub(r" +", " ", h), text
    for name in ("czk_net_gsz_share_batch_mul", "czk_net_gsz_share_batch_inv", "czk_net_gsz_share_partial_products", "czk_net_gsz_product_check"):
        assert re.search(rf"\bint {name}\(czk_net\* net, unsigned degree,", h), name
