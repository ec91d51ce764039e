"""czk_share_group_batch_scale, czk_gsz_group_batch_mul and czk_gsz_group_product_check (csrc/group_share.hip, include/czk.h) against the big-integer
model (tests/group_share_model.py, in the exponent: every point is a known multiple of the generator and the expected points are the checker's
[e] G): every output lane's affine limbs and infinity flags, the counts and the verdict; the edge rows of the joint double-and-add chain; tampered
shares; where the calls write; the argument rules."""
import functools
import random

import numpy as np
import pytest

import group_share_model as M
import gsz_mul_model as G
from guarded import Guards
from share_mul_model import R_MOD, Scheme, to_limbs

SCHEMES = {"spdz2": (2, 2), "spdz3": (2, 3), "add3": (1, 3)}
GROUPS = [1, 2]


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _copy(lanes):
    return [list(ln) for ln in lanes]


# ---- GroupShare::scale ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scheme(name):
    lpp, parties = SCHEMES[name]
    rng = random.Random(len(name) + parties)
    return Scheme(lpp, parties, [rng.randrange(R_MOD) for _ in range(parties)] if lpp == 2 else None)   # a random MAC key split over the parties


@functools.lru_cache(maxsize=None)
def _scale_lanes(name, n):
    """an honest case in the exponent (never modified: tests copy what they change) -> (values s, values o, dict of lanes)"""
    S, rng = _scheme(name), random.Random(1000 * n + len(name))
    sv, ov, xv, yv = ([rng.randrange(R_MOD) for _ in range(n)] for _ in range(4))
    return sv, ov, dict(s=S.share(sv, rng), o=S.share(ov, rng), tx=S.share(xv, rng), ty=S.share(yv, rng),
                        tz=S.share([a * b % R_MOD for a, b in zip(xv, yv)], rng))


def _run_scale(ctx, g, S, ln, guards=None):
    """the device call on the exponent lanes `ln` -> (limbs (L, n, AW), flags (L, n), bad)"""
    import torch
    n, L = len(ln["s"][0]), S.lanes
    d = {}
    for k in ("s", "tx", "tz"):
        pts, inf = M.exp_lanes(g, ln[k])
        d[k], d[k + "_inf"] = (pts, inf) if guards else (_dev(pts), _dev(inf))
    for k in ("o", "ty"):
        d[k] = to_limbs(ln[k]) if guards else _dev(to_limbs(ln[k]))
    if guards:
        d = {k: guards.freeze(v, k) for k, v in d.items()}
        out, out_inf = guards.out(L, n, words=M.AW[g], name="out"), guards.out(L, n, words=1, dtype=torch.uint8, name="out_inf")
        p = {k: v.ptr for k, v in d.items()}
        bad = ctx.share_group_batch_scale(g, S.lpp, S.parties, to_limbs([S.mac_shares])[0] if S.lpp == 2 else None, p["s"], p["s_inf"], p["o"], p["tx"], p["tx_inf"],
                                          p["ty"], p["tz"], p["tz_inf"], out.ptr, out_inf.ptr, n)
        o, oi = guards.check()
        return o, oi.reshape(L, n), bad
    out = torch.empty((L, n, M.AW[g]), dtype=torch.int64, device="cuda")
    out_inf = torch.full((L, n), 7, dtype=torch.uint8, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items()}
    bad = ctx.share_group_batch_scale(g, S.lpp, S.parties, to_limbs([S.mac_shares])[0] if S.lpp == 2 else None, p["s"], p["s_inf"], p["o"], p["tx"], p["tx_inf"], p["ty"],
                                      p["tz"], p["tz_inf"], out.data_ptr(), out_inf.data_ptr(), n)
    return out.cpu().numpy().view(np.uint64), out_inf.cpu().numpy(), bad


def _assert_scale(ctx, g, S, ln, guards=None):
    want, wbad = M.scale_exp(S, ln["s"], ln["o"], ln["tx"], ln["ty"], ln["tz"])
    wp, wi = M.exp_lanes(g, want)
    gp, gi, bad = _run_scale(ctx, g, S, ln, guards)
    assert np.array_equal(gi, wi), (gi, wi)
    assert np.array_equal(gp, wp), np.argwhere((gp != wp).any(axis=2))[:4]
    assert bad == wbad
    return want, bad


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("name", list(SCHEMES))
@pytest.mark.parametrize("g", GROUPS)
def test_scale_equals_the_model_on_every_lane(ctx, g, name, n):
    S = _scheme(name)
    sv, ov, ln = _scale_lanes(name, n)
    want, bad = _assert_scale(ctx, g, S, ln)
    assert bad == 0 and S.batch_open(want) == ([a * b % R_MOD for a, b in zip(sv, ov)], 0)


@pytest.mark.gpu
def test_scale_with_one_live_thread_in_a_second_block(ctx):
    """additive, one party: one lane, so n = 129 outputs are 129 threads: a second block of 128 with one live thread"""
    S, n, rng = Scheme(1, 1), 129, random.Random(5)
    sv, ov, xv, yv = ([rng.randrange(R_MOD) for _ in range(n)] for _ in range(4))
    ln = dict(s=S.share(sv, rng), o=S.share(ov, rng), tx=S.share(xv, rng), ty=S.share(yv, rng), tz=S.share([a * b % R_MOD for a, b in zip(xv, yv)], rng))
    want, _ = _assert_scale(ctx, 1, S, ln)
    assert want[0] == [a * b % R_MOD for a, b in zip(sv, ov)]
    S = _scheme("spdz2")                                               # and SPDZ: 4 lanes x 129 outputs + 129 check threads, blocks that straddle lanes
    _assert_scale(ctx, 1, S, _scale_lanes("spdz2", n)[2])


def _sh_sum(S, ln, a, b, i, skip=None):
    return sum(ln[a][S.lpp * p][i] + ln[b][S.lpp * p][i] for p in range(S.parties) if S.lpp * p != skip) % R_MOD


def _edge(name, S, ln):
    """the named edge rows on element 1 of an honest n = 3 case (the other elements stay honest): the lanes are changed, not re-shared -- the
    model says what comes out, MAC counts included"""
    i = 1
    if name == "infinity_flags":                                       # infinity among s, tx and tz
        ln["s"][0][i] = ln["tx"][1][i] = ln["tz"][2][i] = 0
        ln["s"][3][0] = ln["tz"][0][2] = 0
    elif name == "s_plus_x_opens_to_infinity":
        ln["tx"][0][i] = (ln["tx"][0][i] - _sh_sum(S, ln, "s", "tx", i)) % R_MOD
    elif name == "o_plus_y_opens_to_zero":
        ln["ty"][0][i] = (ln["ty"][0][i] - _sh_sum(S, ln, "o", "ty", i)) % R_MOD
    elif name == "second_scalar_zero":                                 # k_l oy - y_l = 0: y_l = 0 on a lane with k_l = 0, y_0 = oy on the king's
        ln["ty"][2][i] = 0
        ln["o"][0][0] = (-_sh_sum(S, ln, "o", "ty", 0, skip=0)) % R_MOD          # element 0: oy = y_0 + (o_0 + the rest) with o_0 = -(the rest)
    elif name == "x_equals_sx":                                        # the table entry x_l + sx is a doubling: on a mac lane, and on the king's sh lane
        ln["tx"][1][i] = _sh_sum(S, ln, "s", "tx", i)
        ln["s"][0][2] = (-_sh_sum(S, ln, "s", "tx", 2, skip=0)) % R_MOD          # element 2: sx = x_0 + (s_0 + the rest) = x_0
    elif name == "x_equals_minus_sx":                                  # ... and infinity
        ln["tx"][3][i] = (-_sh_sum(S, ln, "s", "tx", i)) % R_MOD
    elif name == "output_at_infinity":
        want, _ = M.scale_exp(S, ln["s"], ln["o"], ln["tx"], ln["ty"], ln["tz"])
        for lane in (0, 3):
            ln["tz"][lane][i] = (ln["tz"][lane][i] - want[lane][i]) % R_MOD
    elif name == "scalars_one_and_r_minus_one":                        # oy = 1: the chain's scalars are r - 1 and k_l - y_l; oy = r - 1: 1 and ...
        ln["ty"][2][i] = R_MOD - 1                                     # lane 2 (k = 0): the second scalar is 1
        ln["o"][0][i] = (ln["o"][0][i] + 1 - _sh_sum(S, ln, "o", "ty", i)) % R_MOD
        ln["o"][0][2] = (ln["o"][0][2] - 1 - _sh_sum(S, ln, "o", "ty", 2)) % R_MOD
    else:
        raise KeyError(name)


SCALE_EDGES = ["infinity_flags", "s_plus_x_opens_to_infinity", "o_plus_y_opens_to_zero", "second_scalar_zero", "x_equals_sx", "x_equals_minus_sx",
               "output_at_infinity", "scalars_one_and_r_minus_one"]


@pytest.mark.gpu
@pytest.mark.parametrize("edge", SCALE_EDGES)
@pytest.mark.parametrize("g", GROUPS)
def test_scale_edge_rows(ctx, g, edge):
    S = _scheme("spdz2")
    ln = {k: _copy(v) for k, v in _scale_lanes("spdz2", 3)[2].items()}
    _edge(edge, S, ln)
    want, _ = _assert_scale(ctx, g, S, ln)
    if edge == "output_at_infinity":
        assert want[0][1] == 0 and want[3][1] == 0
    if edge == "s_plus_x_opens_to_infinity":
        assert _sh_sum(S, ln, "s", "tx", 1) == 0
    if edge == "scalars_one_and_r_minus_one":
        assert _sh_sum(S, ln, "o", "ty", 1) == 1 and _sh_sum(S, ln, "o", "ty", 2) == R_MOD - 1


@pytest.mark.gpu
def test_a_flipped_mac_lane_is_counted_for_that_element_and_an_additive_share_is_not(ctx):
    S = _scheme("spdz2")
    sv, ov, honest = _scale_lanes("spdz2", 3)
    ln = {k: _copy(v) for k, v in honest.items()}
    ln["s"][3][1] = (ln["s"][3][1] + 1) % R_MOD                        # party 1's mac lane of s, element 1
    want, bad = _assert_scale(ctx, 1, S, ln)
    assert bad == 1
    ln["o"][1][1] = (ln["o"][1][1] + 1) % R_MOD                        # both checks of the SAME element fail: still one element
    ln["s"][1][2] = (ln["s"][1][2] + 1) % R_MOD                        # and a second element
    assert _assert_scale(ctx, 1, S, ln)[1] == 2
    S = _scheme("add3")                                                # additive shares: not caught, the product of the changed value comes out
    sv, ov, honest = _scale_lanes("add3", 3)
    ln = {k: _copy(v) for k, v in honest.items()}
    ln["s"][2][1] = (ln["s"][2][1] + 1) % R_MOD
    want, bad = _assert_scale(ctx, 1, S, ln)
    assert bad == 0 and S.opened(want)[1] == (sv[1] + 1) * ov[1] % R_MOD


# ---- gsz20's group mult ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gsz_lanes(parties, n):
    D, t, rng = G.Domain(parties), G.threshold(parties), random.Random(77 * parties + n)
    xv, yv, rv = ([rng.randrange(R_MOD) for _ in range(n)] for _ in range(3))
    return D, t, xv, yv, dict(x=D.share(xv, t, rng), y=D.share(yv, t, rng), gr=D.share(rv, t, rng), gr2=D.share(rv, 2 * t, rng))


def _run_gsz(ctx, g, parties, t, ln):
    import torch
    n = len(ln["x"][0])
    d = {"x": _dev(to_limbs(ln["x"]))}
    for k in ("y", "gr", "gr2"):
        pts, inf = M.exp_lanes(g, ln[k])
        d[k], d[k + "_inf"] = _dev(pts), _dev(inf)
    out = torch.empty((parties, n, M.AW[g]), dtype=torch.int64, device="cuda")
    out_inf = torch.full((parties, n), 7, dtype=torch.uint8, device="cuda")
    p = {k: v.data_ptr() for k, v in d.items()}
    bad = ctx.gsz_group_batch_mul(g, parties, t, p["x"], p["y"], p["y_inf"], p["gr"], p["gr_inf"], p["gr2"], p["gr2_inf"], out.data_ptr(), out_inf.data_ptr(), n)
    return out.cpu().numpy().view(np.uint64), out_inf.cpu().numpy(), bad


def _assert_gsz(ctx, g, D, t, ln):
    want, wbad = M.gsz_mult_exp(D, t, ln["x"], ln["y"], ln["gr"], ln["gr2"])
    wp, wi = M.exp_lanes(g, want)
    gp, gi, bad = _run_gsz(ctx, g, D.parties, t, ln)
    assert np.array_equal(gi, wi), (gi, wi)
    assert np.array_equal(gp, wp), np.argwhere((gp != wp).any(axis=2))[:4]
    assert bad == wbad
    return want, bad


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("parties", [3, 4, 6])                      # (the kernels have no per-count instantiations: 6 is one more count, not another path)
@pytest.mark.parametrize("g", GROUPS)
def test_gsz_mult_equals_the_model_on_every_lane(ctx, g, parties, n):
    D, t, xv, yv, ln = _gsz_lanes(parties, n)
    assert ctx.gsz_group_material_counts(M.OP_MUL, n) == M.material_counts(M.OP_MUL, n)
    want, bad = _assert_gsz(ctx, g, D, t, ln)
    assert bad == 0 and D.batch_open(want, t) == ([a * b % R_MOD for a, b in zip(xv, yv)], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_gsz_mult_edge_rows(ctx, g):
    D, t, xv, yv, honest = _gsz_lanes(4, 3)
    ln = {k: _copy(v) for k, v in honest.items()}
    ln["gr2"][2][1] = (-ln["x"][2][1] * ln["y"][2][1]) % R_MOD         # a D_j at infinity (an inconsistent r2: the bound counts it at 4 parties)
    ln["y"][0][0] = ln["gr"][1][0] = 0                                 # infinity flags among the inputs
    assert _assert_gsz(ctx, g, D, t, ln)[1] >= 1
    # a degree-0 sharing: all lanes equal (the reference's from_public)
    ln = dict(x=D.public([5, R_MOD - 1, 1]), y=D.public([7, 11, 0]), gr=D.public([3, 4, 5]), gr2=D.public([3, 4, 5]))
    want, bad = _assert_gsz(ctx, g, D, t, ln)
    assert bad == 0 and D.batch_open(want, t)[0] == [35, (R_MOD - 11) % R_MOD, 0]


@pytest.mark.gpu
def test_gsz_tampering_is_counted_at_4_parties_and_passes_the_degree_test_at_3(ctx):
    for parties, caught in ((3, 0), (4, 1)):
        D, t, xv, yv, honest = _gsz_lanes(parties, 3)
        ln = {k: _copy(v) for k, v in honest.items()}
        ln["gr2"][1][2] = (ln["gr2"][1][2] + 1) % R_MOD                # party 1's contribution to the king is off by G for element 2
        want, bad = _assert_gsz(ctx, 1, D, t, ln)
        assert bad == caught
        if not caught:                                                 # consistent degree-t shares of a WRONG value: only the product check sees it
            vals, b = D.batch_open(want, t)
            assert b == 0 and vals[2] != xv[2] * yv[2] % R_MOD and vals[:2] == [a * c % R_MOD for a, c in zip(xv[:2], yv[:2])]


# ---- the product check ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _check_case(parties, n, wrong_z=False, bad_material=False):
    D, t, rng = G.Domain(parties), G.threshold(parties), random.Random(31 * n + parties)
    xv, yv = [rng.randrange(R_MOD) for _ in range(n)], [rng.randrange(R_MOD) for _ in range(n)]
    x, y = D.share(xv, t, rng), D.share(yv, t, rng)
    z, _ = G.batch_mult(D, t, x, y, G.random_material(D, t, G.OP_MUL, n, seed=n))
    if wrong_z:                                                        # a consistent sharing of G added to the last product: no degree test sees it
        one = D.share([1], t, rng)
        z = [ln[:-1] + [(ln[-1] + o[0]) % R_MOD] for ln, o in zip(z, one)]
    mat = M.CheckMaterial(D, t, n, seed=5 * n + 1)
    if bad_material:                                                   # party 1's share of the LAST group double's r2 and of the first coin are off by one
        mat.gr2[1][-1] = (mat.gr2[1][-1] + 1) % R_MOD
        mat.rands[1][0] = (mat.rands[1][0] + 1) % R_MOD
    ok, bad = M.check_exp(D, t, x, y, z, mat)
    return D, t, x, y, z, mat, ok, bad


def _run_check(ctx, g, parties, t, x, y, z, mat):
    n = len(x[0])
    d = {"x": _dev(to_limbs(x)), "fr": _dev(to_limbs(mat.fr)), "fr2": _dev(to_limbs(mat.fr2)), "rands": _dev(to_limbs(mat.rands))}
    for k, v in (("y", y), ("z", z), ("gr", mat.gr), ("gr2", mat.gr2)):
        pts, inf = M.exp_lanes(g, v)
        d[k], d[k + "_inf"] = _dev(pts), _dev(inf)
    keep = {k: v.clone() for k, v in d.items()}
    p = {k: v.data_ptr() for k, v in d.items()}
    res = ctx.gsz_group_product_check(g, parties, t, p["x"], p["y"], p["y_inf"], p["z"], p["z_inf"], n, p["gr"], p["gr_inf"], p["gr2"], p["gr2_inf"], p["fr"], p["fr2"],
                                      p["rands"])
    import torch
    assert all(torch.equal(d[k], keep[k]) for k in d), "the check modified an input"
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])                      # no round; odd lengths at two levels
@pytest.mark.parametrize("parties", [3, 4])
@pytest.mark.parametrize("g", GROUPS)
def test_the_check_gives_the_models_verdict_and_count(ctx, g, parties, n):
    assert ctx.gsz_group_material_counts(M.OP_PRODUCT_CHECK, n) == M.material_counts(M.OP_PRODUCT_CHECK, n)
    for kw, want in (({}, (True, 0)), ({"wrong_z": True}, (False, 0)), ({"bad_material": True}, None)):
        D, t, x, y, z, mat, ok, bad = _check_case(parties, n, **kw)
        assert want is None or (ok, bad) == want
        if want is None:
            assert bad >= 1                                            # the coin's share is off: its open exceeds the bound at either party count
        assert _run_check(ctx, g, parties, t, x, y, z, mat) == (ok, bad), kw


@pytest.mark.gpu
def test_the_check_sums_partials_across_blocks(ctx):
    """n = 130: two blocks of 128 in the hadamard pass, 65 in the first round; verdict and counts only"""
    for kw in ({}, {"wrong_z": True}):
        D, t, x, y, z, mat, ok, bad = _check_case(3, 130, **kw)
        assert (ok, bad) == (not kw, 0)
        assert _run_check(ctx, 1, 3, t, x, y, z, mat) == (ok, bad)


# ---- where the calls write, and the argument rules ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_scale_writes_only_its_outputs_and_leaves_the_inputs(ctx, g):
    S = _scheme("spdz2")
    _assert_scale(ctx, g, S, _scale_lanes("spdz2", 3)[2], guards=Guards("cuda"))


@pytest.mark.gpu
@pytest.mark.parametrize("g", GROUPS)
def test_gsz_mult_writes_only_its_outputs_and_leaves_the_inputs(ctx, g):
    import torch
    D, t, xv, yv, ln = _gsz_lanes(3, 3)
    gd = Guards("cuda")
    d = {"x": gd.freeze(to_limbs(ln["x"]), "x")}
    for k in ("y", "gr", "gr2"):
        pts, inf = M.exp_lanes(g, ln[k])
        d[k], d[k + "_inf"] = gd.freeze(pts, k), gd.freeze(inf, k + "_inf")
    out, out_inf = gd.out(3, 3, words=M.AW[g], name="out"), gd.out(3, 3, words=1, dtype=torch.uint8, name="out_inf")
    p = {k: v.ptr for k, v in d.items()}
    bad = ctx.gsz_group_batch_mul(g, 3, t, p["x"], p["y"], p["y_inf"], p["gr"], p["gr_inf"], p["gr2"], p["gr2_inf"], out.ptr, out_inf.ptr, 3)
    o, oi = gd.check()
    wp, wi = M.exp_lanes(g, M.gsz_mult_exp(D, t, ln["x"], ln["y"], ln["gr"], ln["gr2"])[0])
    assert bad == 0 and np.array_equal(o, wp) and np.array_equal(oi.reshape(3, 3), wi)


@pytest.mark.gpu
def test_argument_rules_and_the_empty_calls(ctx):
    import czk_amd
    import torch
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    keep = buf.clone()
    p = buf.data_ptr()
    ms = np.zeros((33, 4), np.uint64)
    scale = lambda g, lpp, parties, n, s=p, out=p, mac=ms: ctx.share_group_batch_scale(g, lpp, parties, mac, s, None, p, p, None, p, p, None, out, out, n)  # noqa: E731
    mul = lambda g, parties, n, x=p, out=p: ctx.gsz_group_batch_mul(g, parties, 1, x, p, None, p, None, p, None, out, out, n)                              # noqa: E731
    chk = lambda g, parties, n, x=p: ctx.gsz_group_product_check(g, parties, 1, x, p, None, p, None, n, p, None, p, None, p, p, p)                         # noqa: E731
    assert scale(1, 2, 2, 0) == 0 and scale(2, 1, 0, 5) == 0 and mul(1, 3, 0) == 0 and chk(2, 3, 0) == (True, 0)     # empty: nothing touched
    assert scale(1, 2, 2, 0, s=None, out=None) == 0 and mul(1, 3, 0, x=None, out=None) == 0
    assert torch.equal(buf, keep)
    for call in (lambda: scale(3, 2, 2, 1), lambda: scale(1, 3, 2, 1), lambda: scale(1, 2, 33, 1), lambda: scale(1, 2, 2, 1, s=None), lambda: scale(1, 2, 2, 1, out=None),
                 lambda: scale(1, 2, 2, 1, mac=None), lambda: mul(0, 3, 1), lambda: mul(1, 3, 1, x=None), lambda: mul(1, 3, 1, out=None), lambda: chk(5, 3, 1),
                 lambda: chk(1, 3, 1, x=None)):
        with pytest.raises(czk_amd.CzkError) as e:
            call()
        assert e.value.code == 3, e.value                              # CZK_ERR_ARG
    for call in (lambda: mul(1, 5, 1), lambda: mul(1, 0, 1), lambda: mul(1, 97, 1), lambda: chk(1, 5, 1), lambda: chk(1, 5, 0), lambda: mul(2, 7, 0)):
        with pytest.raises(czk_amd.CzkError) as e:
            call()
        assert e.value.code == 1, e.value                              # CZK_ERR_SIZE: no share domain of that size
    assert torch.equal(buf, keep)
    gen, _ = M.exp_points(1, [1, 2, 3])                                # additive shares need no key
    pts, o = _dev(gen), _dev(to_limbs([[1], [2], [3]]))
    out, oi = torch.empty((3, 12), dtype=torch.int64, device="cuda"), torch.empty(3, dtype=torch.uint8, device="cuda")
    assert ctx.share_group_batch_scale(1, 1, 3, None, pts.data_ptr(), None, o.data_ptr(), pts.data_ptr(), None, o.data_ptr(), pts.data_ptr(), None, out.data_ptr(),
                                       oi.data_ptr(), 1) == 0
