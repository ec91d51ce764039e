"""The big-integer model of the group-share products (tests/group_share_model.py) against plain arithmetic and against itself: the product of a
shared point and a shared scalar opens to [o] S for SPDZ, additive and GSZ shares; the model on curve points and the model in the exponent agree;
the king's degree bound catches a tampered contribution exactly when it is not vacuous; the library's material counts; the header.  No GPU; curve
arithmetic runs at n <= 3."""
import ctypes as C
import random

import numpy as np
import pytest

import group_share_model as M
import gsz_mul_model as G
from share_mul_model import R_MOD, Scheme


def _scale_case(lpp, parties, n, seed):
    rng = random.Random(seed)
    S = Scheme(lpp, parties, [rng.randrange(R_MOD) for _ in range(parties)] if lpp == 2 else None)
    sv, ov = [rng.randrange(R_MOD) for _ in range(n)], [rng.randrange(R_MOD) for _ in range(n)]
    xv, yv = [rng.randrange(R_MOD) for _ in range(n)], [rng.randrange(R_MOD) for _ in range(n)]
    lanes = dict(s=S.share(sv, rng), o=S.share(ov, rng), tx=S.share(xv, rng), ty=S.share(yv, rng), tz=S.share([a * b % R_MOD for a, b in zip(xv, yv)], rng))
    return S, sv, ov, lanes


def _gsz_case(parties, n, seed):
    rng = random.Random(seed)
    D, t = G.Domain(parties), G.threshold(parties)
    xv, yv, rv = ([rng.randrange(R_MOD) for _ in range(n)] for _ in range(3))
    lanes = dict(x=D.share(xv, t, rng), y=D.share(yv, t, rng), gr=D.share(rv, t, rng), gr2=D.share(rv, 2 * t, rng))
    return D, t, xv, yv, lanes


@pytest.mark.parametrize("lpp,parties", [(2, 2), (1, 3)])
def test_scale_opens_to_the_scaled_point_in_both_models(lpp, parties):
    for g, n in ((1, 3), (2, 1)):
        S, sv, ov, ln = _scale_case(lpp, parties, n, seed=11 * g + parties)
        want = [a * b % R_MOD for a, b in zip(sv, ov)]
        out, bad = M.scale_exp(S, ln["s"], ln["o"], ln["tx"], ln["ty"], ln["tz"])
        assert bad == 0 and S.batch_open(out) == (want, 0)             # [o] S in the exponent, MAC lanes included
        Cv = M.Curve(g)
        pts = {k: Cv.lanes_in(*M.exp_lanes(g, ln[k])) for k in ("s", "tx", "tz")}
        got, bad = M.scale_points(Cv, S, pts["s"], ln["o"], pts["tx"], ln["ty"], pts["tz"])
        assert bad == 0
        gp, gi = Cv.lanes_out(got)
        wp, wi = M.exp_lanes(g, out)                                   # lane for lane: the two models agree
        assert np.array_equal(gp, wp) and np.array_equal(gi, wi)
        opened = Cv.lanes_out([[Cv.sum(got[lpp * p][i] for p in range(parties)) for i in range(n)]])
        wo = M.exp_points(g, want)
        assert np.array_equal(opened[0][0], wo[0]) and np.array_equal(opened[1][0], wo[1])


@pytest.mark.parametrize("parties", [3, 4])
def test_gsz_mult_opens_to_the_scaled_point_in_both_models(parties):
    for g, n in ((1, 3), (2, 1)):
        D, t, xv, yv, ln = _gsz_case(parties, n, seed=7 * g + parties)
        out, bad = M.gsz_mult_exp(D, t, ln["x"], ln["y"], ln["gr"], ln["gr2"])
        assert bad == 0 and D.batch_open(out, t) == ([a * b % R_MOD for a, b in zip(xv, yv)], 0)
        Cv = M.Curve(g)
        pts = {k: Cv.lanes_in(*M.exp_lanes(g, ln[k])) for k in ("y", "gr", "gr2")}
        got, bad = M.gsz_mult_points(Cv, D, t, ln["x"], pts["y"], pts["gr"], pts["gr2"])
        assert bad == 0
        gp, gi = Cv.lanes_out(got)
        wp, wi = M.exp_lanes(g, out)
        assert np.array_equal(gp, wp) and np.array_equal(gi, wi)


def test_a_flipped_mac_lane_is_counted_and_a_flipped_additive_share_is_not():
    S, sv, ov, ln = _scale_case(2, 2, 3, seed=3)
    s = [list(v) for v in ln["s"]]
    s[3][1] = (s[3][1] + 1) % R_MOD                                    # party 1's mac lane of element 1
    assert M.scale_exp(S, s, ln["o"], ln["tx"], ln["ty"], ln["tz"])[1] == 1
    S, sv, ov, ln = _scale_case(1, 3, 3, seed=4)
    s = [list(v) for v in ln["s"]]
    s[2][1] = (s[2][1] + 1) % R_MOD
    out, bad = M.scale_exp(S, s, ln["o"], ln["tx"], ln["ty"], ln["tz"])
    assert bad == 0 and S.opened(out)[1] == (sv[1] + 1) * ov[1] % R_MOD   # not caught: additive shares carry no check


def test_the_degree_bound_is_vacuous_at_3_parties_and_counts_at_4():
    """at 3 parties a consistent sharing of G added to one product passes mult's degree test (only a product check would reject it); at 4 parties a
    tampered contribution to the king is counted"""
    D, t, xv, yv, ln = _gsz_case(3, 3, seed=21)
    out, bad = M.gsz_mult_exp(D, t, ln["x"], ln["y"], ln["gr"], ln["gr2"])
    one = D.share([1], t, random.Random(1))
    out2 = [list(v) for v in out]
    for j in range(3):
        out2[j][1] = (out2[j][1] + one[j][0]) % R_MOD
    vals, b = D.batch_open(out2, t)
    assert bad == 0 and b == 0 and vals[1] == (xv[1] * yv[1] + 1) % R_MOD
    for parties, caught in ((3, 0), (4, 1)):
        D, t, xv, yv, ln = _gsz_case(parties, 3, seed=22)
        gr2 = [list(v) for v in ln["gr2"]]
        gr2[1][2] = (gr2[1][2] + 1) % R_MOD                            # party 1's D_j for element 2 is off by G
        assert M.gsz_mult_exp(D, t, ln["x"], ln["y"], ln["gr"], gr2)[1] == caught


@pytest.mark.parametrize("parties", [3, 4])
def test_the_check_accepts_honest_triples_and_rejects_a_wrong_product_in_both_models(parties):
    """n = 3: two rounds, an odd length at the first; the curve-point model and the exponent model give the same verdict and count"""
    g, n = 1, 3
    D, t, xv, yv, ln = _gsz_case(parties, n, seed=40 + parties)
    z, bad = M.gsz_mult_exp(D, t, ln["x"], ln["y"], ln["gr"], ln["gr2"])
    one = D.share([1], t, random.Random(2))
    z_wrong = [v[:-1] + [(v[-1] + o[0]) % R_MOD] for v, o in zip(z, one)]      # a consistent sharing of G added: mult's degree test passes
    assert bad == 0 and D.batch_open(z_wrong, t)[1] == 0
    Cv = M.Curve(g)
    for zs, verdict in ((z, True), (z_wrong, False)):
        mat = M.CheckMaterial(D, t, n, seed=8)
        assert M.check_exp(D, t, ln["x"], ln["y"], zs, mat) == (verdict, 0)
        pts = {k: Cv.lanes_in(*M.exp_lanes(g, v)) for k, v in (("y", ln["y"]), ("z", zs), ("gr", mat.gr), ("gr2", mat.gr2))}
        assert M.check_points(Cv, D, t, ln["x"], pts["y"], pts["z"], pts["gr"], pts["gr2"], mat.fr, mat.fr2, mat.rands) == (verdict, 0)
    mat = M.CheckMaterial(D, t, n, seed=8)                             # off-by-one material: both models count the same opens
    mat.gr2[1][-1] = (mat.gr2[1][-1] + 1) % R_MOD
    mat.rands[1][0] = (mat.rands[1][0] + 1) % R_MOD
    pts = {k: Cv.lanes_in(*M.exp_lanes(g, v)) for k, v in (("y", ln["y"]), ("z", z), ("gr", mat.gr), ("gr2", mat.gr2))}
    want = M.check_exp(D, t, ln["x"], ln["y"], z, mat)
    assert want[1] >= 1 and M.check_points(Cv, D, t, ln["x"], pts["y"], pts["z"], pts["gr"], pts["gr2"], mat.fr, mat.fr2, mat.rands) == want


def test_the_library_reports_the_models_material_counts():
    import czk_amd
    L = czk_amd.lib()

    def counts(op, n):
        a, b, c = C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
        return L.czk_gsz_group_material_counts(C.c_int(op), C.c_size_t(n), C.byref(a), C.byref(b), C.byref(c)), (a.value, b.value, c.value)
    for n in (0, 1, 3, 48, 1 << 16):
        assert counts(M.OP_MUL, n) == (0, M.material_counts(M.OP_MUL, n)) == (0, (n, 0, 0))
    assert [counts(M.OP_PRODUCT_CHECK, n)[1] for n in (0, 1, 2, 3, 5, 8, 48, 1025)] == [(0, 0, 0), (2, 2, 3), (4, 2, 4), (6, 2, 5), (8, 2, 6), (8, 2, 6), (14, 2, 9), (24, 2, 14)]
    for n in (0, 1, 2, 3, 4, 5, 8, 9, 33, 1 << 16):
        assert counts(M.OP_PRODUCT_CHECK, n) == (0, M.material_counts(M.OP_PRODUCT_CHECK, n))
    assert counts(M.OP_MUL, 1 << 60) == (1, (0, 0, 0))                 # CZK_ERR_SIZE
    assert counts(9, 8) == (3, (0, 0, 0))                              # CZK_ERR_ARG
    assert L.czk_gsz_group_material_counts(C.c_int(0), C.c_size_t(8), None, None, None) == 3


def test_the_header_declares_and_the_library_exports_the_group_share_calls():
    import czk_amd
    new = {"czk_share_group_batch_scale", "czk_gsz_group_batch_mul", "czk_gsz_group_product_check", "czk_gsz_group_material_counts"}
    assert new <= set(czk_amd.header_symbols()) and new <= set(czk_amd.exported_symbols())
