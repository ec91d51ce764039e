"""tests/share_pairing_model.py against itself, no GPU: the reference's literal formula for the pairing of shared points (separate pairings, inversions,
powers; tests/pairing_ref.py) equals the exponent form the GPU tests compare against; the lanes open to e(open a, open b); the case builders produce
the edge rows they claim; open's integer-sum exponent gives the per-party verdict outside the subgroup too; the new entry points are declared and
exported."""
import random

import pytest

import pairing_ref as PR
import share_pairing_model as M
from share_mul_model import R_MOD, Scheme

SCHEMES = {"add2": (1, 2), "add3": (1, 3), "spdz2": (2, 2), "spdz3": (2, 3)}


def _scheme(name):
    lpp, parties = SCHEMES[name]
    rng = random.Random(len(name) + parties)
    return Scheme(lpp, parties, [rng.randrange(R_MOD) for _ in range(parties)] if lpp == 2 else None)


def _literal_inputs(ln):
    pts = {k: [[(M.g1 if k in ("a", "tx") else M.g2)(e) for e in lane] for lane in ln[k]] for k in ("a", "b", "tx", "ty")}
    return pts["a"], pts["b"], pts["tx"], pts["ty"], [[M.gt_pow(e) for e in lane] for lane in ln["tz"]]


@pytest.mark.parametrize("name", list(SCHEMES))
def test_the_literal_formula_equals_the_exponent_form_and_opens_to_the_pairing(name):
    S = _scheme(name)
    av, bv, ln = M.honest_case(S, 1, seed=7)
    want, bad = M.pairing_exp(S, ln["a"], ln["b"], ln["tx"], ln["ty"], ln["tz"])
    assert bad == 0
    got = M.pairing_literal(S, *_literal_inputs(ln))
    assert got == [[M.gt_pow(e) for e in lane] for lane in want]
    assert M.open_exp(S, want) == ([av[0] * bv[0] % R_MOD], 0)
    vals, bad = M.open_literal(S, got)
    assert bad == 0 and vals == [PR.pairing(M.g1(av[0]), M.g2(bv[0]))] and M.open_integer_rule(S, got) == (vals, 0)


def test_the_edge_rows_are_what_they_claim_and_the_two_forms_agree_on_them():
    S = _scheme("spdz2")
    av, bv, ln = M.edge_case(S, seed=11)
    row = {name: i for i, name in enumerate(M.EDGE_ROWS)}
    opened = {k: S.batch_open(ln[k]) for k in ("a", "b", "tx", "ty")}
    assert all(b == 0 for _, b in opened.values())                     # every row is an honest sharing
    assert (opened["a"][0], opened["b"][0]) == (av, bv)
    xa = [(a + x) % R_MOD for a, x in zip(opened["a"][0], opened["tx"][0])]
    yb = [(b + y) % R_MOD for b, y in zip(opened["b"][0], opened["ty"][0])]
    assert [i for i, v in enumerate(xa) if v == 0] == [row["a_is_minus_x"]] and [i for i, v in enumerate(yb) if v == 0] == [row["b_is_minus_y"]]
    assert ln["tx"][2][row["a_tx_lane_infinite"]] == 0 and opened["tx"][0][row["a_tx_lane_infinite"]] != 0
    assert ln["ty"][3][row["a_ty_lane_infinite"]] == 0 and opened["ty"][0][row["a_ty_lane_infinite"]] != 0
    assert all(ln["a"][lane][row["a_infinite"]] == 0 for lane in range(4)) and av[row["a_infinite"]] == 0
    assert all(ln[k][lane][row["dummy_triple"]] == 0 for k in ("tx", "ty", "tz") for lane in range(4))
    i = row["opposite_lane_summands"]
    assert (ln["a"][0][i] + ln["tx"][0][i]) % R_MOD == 0 and ln["a"][0][i] != 0 and xa[i] != 0
    want, bad = M.pairing_exp(S, ln["a"], ln["b"], ln["tx"], ln["ty"], ln["tz"])
    assert bad == 0 and M.open_exp(S, want) == ([a * b % R_MOD for a, b in zip(av, bv)], 0)
    assert M.open_exp(S, want)[0][row["a_infinite"]] == 0               # e(infinity, b) is one
    assert M.pairing_literal(S, *_literal_inputs(ln)) == [[M.gt_pow(e) for e in lane] for lane in want]


def test_tampering_in_the_exponent_model():
    S = _scheme("spdz2")
    _, _, honest = M.honest_case(S, 3, seed=3)
    for name, lane in (("a", 3), ("b", 1), ("tx", 1), ("ty", 3)):      # a changed mac lane of an opened point: that element, once
        ln = {k: [list(x) for x in v] for k, v in honest.items()}
        ln[name][lane][1] = (ln[name][lane][1] + 1) % R_MOD
        assert M.pairing_exp(S, ln["a"], ln["b"], ln["tx"], ln["ty"], ln["tz"])[1] == 1
    ln = {k: [list(x) for x in v] for k, v in honest.items()}
    ln["a"][3][1] += 1
    ln["b"][3][1] += 1                                                 # both checks of one element: still one element
    assert M.pairing_exp(S, ln["a"], ln["b"], ln["tx"], ln["ty"], ln["tz"])[1] == 1
    ln = {k: [list(x) for x in v] for k, v in honest.items()}
    ln["tz"][1][2] = (ln["tz"][1][2] + 1) % R_MOD                      # a changed mac lane of tz: not seen by the pairing, counted by the open
    out, bad = M.pairing_exp(S, ln["a"], ln["b"], ln["tx"], ln["ty"], ln["tz"])
    assert bad == 0 and M.open_exp(S, out)[1] == 1
    A = Scheme(1, 3)
    av, bv, ln = M.honest_case(A, 3, seed=4)
    ln = {k: [list(x) for x in v] for k, v in ln.items()}
    ln["a"][2][1] = (ln["a"][2][1] + 1) % R_MOD                        # additive shares carry nothing that could catch it
    out, bad = M.pairing_exp(A, ln["a"], ln["b"], ln["tx"], ln["ty"], ln["tz"])
    assert bad == 0 and M.open_exp(A, out)[0][1] == (av[1] + 1) * bv[1] % R_MOD


def test_the_integer_sum_exponent_gives_the_per_party_verdict_outside_the_subgroup():
    """x^(sum of the canonical shares) over the mac product, against prod_j x^(mac_share_j) / mac_j: equal for any x.  Reducing the sum mod r would
    not be: x^r is not one outside the subgroup."""
    S, rng = _scheme("spdz3"), random.Random(9)
    assert sum(S.mac_shares) >= R_MOD                                  # the integer sum differs from the key mod r
    x = M.outside_subgroup(5)
    lanes = M.integer_consistent_lanes(S, x, rng)
    assert M.open_literal(S, lanes) == ([x], 0) and M.open_integer_rule(S, lanes) == ([x], 0)
    m = PR.FQ12_ONE
    for p in range(S.parties):
        m = PR.fq12_mul(m, lanes[2 * p + 1][0])
    assert PR.fq12_pow(x, sum(S.mac_shares) % R_MOD) != m               # the rule mod r would reject these honest lanes
    lanes[3][0] = PR.fq12_mul(lanes[3][0], M.gt_pow(1))                 # a changed mac lane: both forms count it
    assert M.open_literal(S, lanes)[1] == 1 and M.open_integer_rule(S, lanes)[1] == 1


def test_scale_open_and_the_vector_operations_in_both_forms():
    S, rng = _scheme("spdz2"), random.Random(2)
    v = S.share([rng.randrange(R_MOD) for _ in range(2)], rng)
    f = [rng.randrange(R_MOD), 0]
    want = M.scale_exp(S, v, f)
    assert M.scale_literal(S, [[M.gt_pow(e) for e in lane] for lane in v], [M.gt_pow(e) for e in f]) == [[M.gt_pow(e) for e in lane] for lane in want]
    assert M.open_exp(S, want) == ([(a + b) % R_MOD for a, b in zip(S.opened(v), f)], 0)
    pub = M.scale_exp(S, None, f)                                      # from_public: f on the king's sh, f^(mac_share_j) on the mac lanes, one elsewhere
    assert pub[0] == f and pub[2] == [0, 0] and M.open_exp(S, pub) == (f, 0)
    assert M.scale_literal(S, None, [M.gt_pow(e) for e in f]) == [[M.gt_pow(e) for e in lane] for lane in pub]
    a, b = [M.gt_pow(3), M.outside_subgroup(1), M.gt_pow(5)], [M.gt_pow(4), M.gt_pow(2), M.FQ12_ZERO]
    assert M.vec_literal("mul", a, b)[0] == M.gt_pow(7) and M.vec_literal("div", a, b)[0] == M.gt_pow(R_MOD - 1)
    assert M.vec_literal("div", a, b)[2] == M.FQ12_ZERO and M.vec_literal("inv", b)[2] == M.FQ12_ZERO   # a zero divisor yields zero
    assert PR.fq12_mul(M.vec_literal("inv", a)[1], a[1]) == PR.FQ12_ONE


def test_the_entry_points_are_declared_exported_and_bound():
    import czk_amd
    new = {"czk_share_pairing", "czk_gt_share_open", "czk_gt_share_scale", "czk_fq12_vec_op"}
    assert new <= set(czk_amd.header_symbols()) and new <= set(czk_amd.exported_symbols())
    for m in ("share_pairing", "gt_share_open", "gt_share_scale", "fq12_vec_op"):
        assert callable(getattr(czk_amd.Context, m))
