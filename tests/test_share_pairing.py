"""czk_share_pairing, czk_gt_share_open, czk_gt_share_scale and czk_fq12_vec_op (csrc/pairing_share.hip, include/czk.h) and the client computations of
collaborative-zksnark_amd/pairing_share.py against the big-integer model (tests/share_pairing_model.py): every output limb of every lane, the counts,
the edge rows of the pair list, a second block with one live thread, tampered shares, where the calls write, the argument rules."""
import functools
import random

import numpy as np
import pytest

import group_share_model as GM
import pairing_ref as PR
import share_pairing_model as M
from guarded import Guards
from share_mul_model import R_MOD, Scheme, to_limbs

SCHEMES = {"add2": (1, 2), "add3": (1, 3), "spdz2": (2, 2), "spdz3": (2, 3)}


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


def _copy(ln):
    return {k: [list(x) for x in v] for k, v in ln.items()}


@functools.lru_cache(maxsize=None)
def _scheme(name):
    lpp, parties = SCHEMES[name]
    rng = random.Random(len(name) + parties)
    return Scheme(lpp, parties, [rng.randrange(R_MOD) for _ in range(parties)] if lpp == 2 else None)   # a random MAC key split over the parties


def _mac(S):
    return to_limbs([S.mac_shares])[0] if S.lpp == 2 else None


@functools.lru_cache(maxsize=None)
def _case(name, n):
    return M.honest_case(_scheme(name), n, seed=100 * n + len(name))


def _inputs(ln):
    """the exponent lanes as host arrays, in the argument order of the call"""
    d = {}
    for k, g in (("a", 1), ("b", 2), ("tx", 1), ("ty", 2)):
        d[k], d[k + "_inf"] = M.point_lanes(g, ln[k])
    d["tz"] = M.gt_lanes(ln["tz"])
    return d


def _run(ctx, S, ln, guards=None):
    """the device call on the exponent lanes -> (limbs (L, n, 72), bad)"""
    import torch
    n, d = len(ln["a"][0]), _inputs(ln)
    if guards:
        d = {k: guards.freeze(v, k) for k, v in d.items()}
        out = guards.out(S.lanes, n, words=72, name="out")
        p, po = {k: v.ptr for k, v in d.items()}, out.ptr
    else:
        d = {k: _dev(v) for k, v in d.items()}
        out = torch.empty((S.lanes, n, 72), dtype=torch.int64, device="cuda")
        p, po = {k: v.data_ptr() for k, v in d.items()}, out.data_ptr()
    bad = ctx.share_pairing(S.lpp, S.parties, _mac(S), p["a"], p["a_inf"], p["b"], p["b_inf"], p["tx"], p["tx_inf"], p["ty"], p["ty_inf"], p["tz"], po, n)
    return (guards.check()[0] if guards else out.cpu().numpy().view(np.uint64)), bad


def _assert_pairing(ctx, S, ln, guards=None):
    want, wbad = M.pairing_exp(S, ln["a"], ln["b"], ln["tx"], ln["ty"], ln["tz"])
    got, bad = _run(ctx, S, ln, guards)
    wl = M.gt_lanes(want)
    assert np.array_equal(got, wl), np.argwhere((got != wl).any(axis=2))[:4]
    assert bad == wbad
    return want, got, bad


def _open(ctx, S, lanes):
    """czk_gt_share_open on (L, n, 72) host limbs -> ((n, 72) limbs, bad)"""
    import torch
    v, n = _dev(lanes), lanes.shape[1]
    out = torch.empty((n, 72), dtype=torch.int64, device="cuda")
    bad = ctx.gt_share_open(S.lpp, S.parties, _mac(S), v.data_ptr(), n, out.data_ptr())
    return out.cpu().numpy().view(np.uint64), bad


# ---- the lanes against the model ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("name", list(SCHEMES))
def test_share_pairing_equals_the_model_on_every_lane_and_opens_to_the_pairing(ctx, name, n):
    S = _scheme(name)
    av, bv, ln = _case(name, n)
    want, got, bad = _assert_pairing(ctx, S, ln)
    assert bad == 0 and M.open_exp(S, want) == ([a * b % R_MOD for a, b in zip(av, bv)], 0)
    opened, obad = _open(ctx, S, got)
    p1, i1 = GM.exp_points(1, av)                                      # the anchor that owes nothing to the model: Context.pairing of the opened points
    p2, i2 = GM.exp_points(2, bv)
    assert obad == 0 and np.array_equal(opened, ctx.pairing(p1, p2, i1, i2))


@pytest.mark.gpu
def test_share_pairing_equals_the_literal_formula(ctx):
    """model (i): the reference's z / e(xa, y) / e(x, yb) * e(xa, yb) with separate pairings, inversions and powers, at one case"""
    S = _scheme("spdz2")
    _, _, ln = _case("spdz2", 1)
    pts = {k: [[(M.g1 if k in ("a", "tx") else M.g2)(e) for e in lane] for lane in ln[k]] for k in ("a", "b", "tx", "ty")}
    lit = M.pairing_literal(S, pts["a"], pts["b"], pts["tx"], pts["ty"], [[M.gt_pow(e) for e in lane] for lane in ln["tz"]])
    got, bad = _run(ctx, S, ln)
    assert bad == 0 and np.array_equal(got, M.fq12_lanes(lit))


@pytest.mark.gpu
def test_edge_rows_in_one_call(ctx):
    """xa infinite, yb infinite, one lane's tx / ty infinite, a infinite, the dummy triple, lane summands that cancel: one element each"""
    S = _scheme("spdz2")
    av, bv, ln = M.edge_case(S, seed=11)
    want, got, bad = _assert_pairing(ctx, S, ln)
    assert bad == 0
    opened, obad = _open(ctx, S, got)
    assert obad == 0 and np.array_equal(opened, M.gt_lanes([[a * b % R_MOD for a, b in zip(av, bv)]])[0])
    assert np.array_equal(opened[M.EDGE_ROWS.index("a_infinite")], M.gt_limbs(PR.FQ12_ONE))


@pytest.mark.gpu
def test_one_live_thread_in_a_second_block(ctx):
    """additive, 5 parties, n = 13: L n = 65 threads of the pairing kernel, one of them alone in a second block of 64; 63 and 64 sit beside it"""
    S, n = Scheme(1, 5), 13
    assert S.lanes * n == 65
    av, bv, ln = M.honest_case(S, n, seed=65)
    want, _, bad = _assert_pairing(ctx, S, ln)
    assert bad == 0 and M.open_exp(S, want)[0] == [a * b % R_MOD for a, b in zip(av, bv)]


# ---- tampering --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_changed_mac_lane_is_counted_for_that_element_and_an_additive_share_is_not(ctx):
    S = _scheme("spdz2")
    _, _, honest = _case("spdz2", 3)
    ln = _copy(honest)
    ln["a"][3][1] = (ln["a"][3][1] + 1) % R_MOD                        # party 1's mac lane of a, element 1
    assert _assert_pairing(ctx, S, ln)[2] == 1
    ln = _copy(honest)
    ln["b"][1][2] = (ln["b"][1][2] + 1) % R_MOD                        # party 0's mac lane of b, element 2
    assert _assert_pairing(ctx, S, ln)[2] == 1
    ln["a"][1][2] = (ln["a"][1][2] + 1) % R_MOD                        # both checks of the SAME element fail: still one element
    ln["ty"][3][0] = (ln["ty"][3][0] + 1) % R_MOD                      # and a second element
    assert _assert_pairing(ctx, S, ln)[2] == 2
    A = _scheme("add3")                                                # additive shares: NOT caught, the pairing of the changed value comes out
    av, bv, honest = _case("add3", 3)
    ln = _copy(honest)
    ln["a"][2][1] = (ln["a"][2][1] + 1) % R_MOD
    want, _, bad = _assert_pairing(ctx, A, ln)
    assert bad == 0 and M.open_exp(A, want)[0][1] == (av[1] + 1) * bv[1] % R_MOD


@pytest.mark.gpu
def test_a_changed_mac_lane_of_tz_passes_the_pairing_and_is_counted_by_the_open(ctx):
    S = _scheme("spdz2")
    _, _, honest = _case("spdz2", 3)
    ln = _copy(honest)
    ln["tz"][1][2] = (ln["tz"][1][2] + 1) % R_MOD
    want, got, bad = _assert_pairing(ctx, S, ln)
    assert bad == 0 and M.open_exp(S, want)[1] == 1
    assert _open(ctx, S, got)[1] == 1


# ---- share arithmetic -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCHEMES))
def test_open_of_honest_and_changed_lanes(ctx, name):
    S, rng = _scheme(name), random.Random(21)
    vals = [rng.randrange(R_MOD), 0, 1]
    v = S.share(vals, rng)
    got, bad = _open(ctx, S, M.gt_lanes(v))
    assert bad == 0 and np.array_equal(got, M.gt_lanes([vals])[0])
    v[S.lanes - 1][2] = (v[S.lanes - 1][2] + 1) % R_MOD                # the last lane: a mac lane (counted) or an additive share (another value)
    wv, wbad = M.open_exp(S, v)
    got, bad = _open(ctx, S, M.gt_lanes(v))
    assert bad == wbad == (1 if S.lpp == 2 else 0) and np.array_equal(got, M.gt_lanes([wv])[0])


@pytest.mark.gpu
def test_open_outside_the_subgroup_follows_the_integer_exponent(ctx):
    """lanes whose product is no r-th root of unity, macs consistent under the INTEGER sum of the mac shares (which exceeds r here): honest, so not counted"""
    S, rng = _scheme("spdz3"), random.Random(9)
    assert sum(S.mac_shares) >= R_MOD
    x = M.outside_subgroup(5)
    lanes = M.integer_consistent_lanes(S, x, rng)
    assert M.open_literal(S, lanes) == ([x], 0)
    got, bad = _open(ctx, S, M.fq12_lanes(lanes))
    assert bad == 0 and np.array_equal(got[0], M.gt_limbs(x))
    lanes[3][0] = PR.fq12_mul(lanes[3][0], M.gt_pow(1))
    assert M.open_literal(S, lanes)[1] == 1 and _open(ctx, S, M.fq12_lanes(lanes))[1] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["add3", "spdz2", "spdz3"])
def test_scale_and_from_public(ctx, name):
    import torch
    S, rng = _scheme(name), random.Random(22)
    v = S.share([rng.randrange(R_MOD) for _ in range(3)], rng)
    f = [rng.randrange(R_MOD), 0, 1]
    fd = _dev(M.gt_lanes([f])[0])
    for lanes in (v, None):
        vd = None if lanes is None else _dev(M.gt_lanes(lanes))
        out = torch.empty((S.lanes, 3, 72), dtype=torch.int64, device="cuda")
        ctx.gt_share_scale(S.lpp, S.parties, _mac(S), None if vd is None else vd.data_ptr(), fd.data_ptr(), out.data_ptr(), 3)
        ctx.sync()
        want = M.scale_exp(S, lanes, f)
        got = out.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, M.gt_lanes(want))
        assert _open(ctx, S, got)[1] == 0 and M.open_exp(S, want) == ([(a + b) % R_MOD for a, b in zip(S.opened(lanes) if lanes else [0] * 3, f)], 0)


@pytest.mark.gpu
def test_fq12_vector_operations_and_the_zero_divisor(ctx):
    import czk_amd
    import torch
    B = czk_amd.binding
    a = [M.gt_pow(3), M.outside_subgroup(1), M.gt_pow(5), M.FQ12_ZERO]
    b = [M.gt_pow(4), M.outside_subgroup(2), M.FQ12_ZERO, M.gt_pow(6)]
    al, bl = M.fq12_lanes([a])[0], M.fq12_lanes([b])[0]
    for op, name in ((B.CZK_FQ12_OP_MUL, "mul"), (B.CZK_FQ12_OP_DIV, "div"), (B.CZK_FQ12_OP_INV, "inv")):
        want = M.fq12_lanes([M.vec_literal(name, a, b)])[0]
        assert np.array_equal(ctx.fq12_vec_op(op, al, None if name == "inv" else bl), want), name          # host memory
        ad, bd = _dev(al), _dev(bl)
        out = torch.empty((4, 72), dtype=torch.int64, device="cuda")
        ctx.fq12_vec_op(op, ad.data_ptr(), None if name == "inv" else bd.data_ptr(), n=4, out=out.data_ptr(), mem=czk_amd.CZK_MEM_DEVICE)
        ctx.sync()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want), name
    zero = np.zeros(72, np.uint64)
    assert np.array_equal(ctx.fq12_vec_op(B.CZK_FQ12_OP_DIV, al, bl)[2], zero) and np.array_equal(ctx.fq12_vec_op(B.CZK_FQ12_OP_INV, al)[3], zero)


# ---- the client computations ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCHEMES))
def test_pairing_dh_prod_and_div(ctx, name):
    """client.rs:503-581 on shared scalars with a seeded dealer's triples: the two opened sides are equal (the reference's assert_eq) and equal gt to the
    expected exponent"""
    from czk_amd import pairing_share as PS
    from czk_amd.provers import SeededGroupDealer
    S, rng = _scheme(name), random.Random(31)
    sp = PS.SharedPairing(ctx, S.lpp, S.parties, S.mac_shares if S.lpp == 2 else None, SeededGroupDealer(7))
    a, b, c, d = (rng.randrange(1, R_MOD) for _ in range(4))
    sh = lambda v: sp.share_scalars([v], rng)                          # noqa: E731
    left, right = PS.pairing_dh(sp, sh(a), sh(b), sh(a * b % R_MOD))
    assert np.array_equal(left, right) and np.array_equal(left[0], M.gt_limbs(M.gt_pow(a * b)))
    left, right = PS.pairing_prod(sp, sh(a), sh(b), sh(c), sh(d))
    assert np.array_equal(left, right) and np.array_equal(left[0], M.gt_limbs(M.gt_pow((a + b) * (c + d))))
    left, right = PS.pairing_div(sp, sh(a), sh(b), sh(c), sh(d))
    assert np.array_equal(left, right) and np.array_equal(left[0], M.gt_limbs(M.gt_pow((a - b) * (c - d))))


@pytest.mark.gpu
def test_the_dummy_source_and_a_failed_check_in_the_python_layer(ctx):
    from czk_amd import pairing_share as PS
    from czk_amd.polyvm import SharingError
    from czk_amd.provers import DummyGroupSource
    S, rng = _scheme("spdz2"), random.Random(32)
    sp = PS.SharedPairing(ctx, 2, 2, S.mac_shares, DummyGroupSource())
    a, b = rng.randrange(1, R_MOD), rng.randrange(1, R_MOD)
    g1a, g2b = sp.lift_lanes(1, sp.share_scalars([a], rng)), sp.lift_lanes(2, sp.share_scalars([b], rng))
    assert np.array_equal(sp.open(sp.pairing(*g1a, *g2b))[0], M.gt_limbs(M.gt_pow(a * b)))   # the stub triple: the operands are opened as they are
    bad = sp.share_scalars([a], rng)
    bad[1, 0, 0] += 1                                                  # party 0's mac lane
    with pytest.raises(SharingError):
        sp.pairing(*sp.lift_lanes(1, bad), *g2b)


# ---- where the calls write, and the argument rules --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_calls_write_only_their_outputs_and_leave_the_inputs(ctx):
    import czk_amd
    S = _scheme("spdz2")
    _, _, ln = _case("spdz2", 3)
    want, got, _ = _assert_pairing(ctx, S, ln, guards=Guards("cuda"))
    gd = Guards("cuda")
    v, out = gd.freeze(got, "v"), gd.out(1, 3, words=72, name="opened")
    assert ctx.gt_share_open(2, 2, _mac(S), v.ptr, 3, out.ptr) == 0
    assert np.array_equal(gd.check()[0][0], M.gt_lanes([M.open_exp(S, want)[0]])[0])
    gd = Guards("cuda")
    f = [5, 0, R_MOD - 1]
    v, fd, out = gd.freeze(got, "v"), gd.freeze(M.gt_lanes([f])[0], "f"), gd.out(4, 3, words=72, name="scaled")
    ctx.gt_share_scale(2, 2, _mac(S), v.ptr, fd.ptr, out.ptr, 3)
    ctx.sync()
    assert np.array_equal(gd.check()[0], M.gt_lanes(M.scale_exp(S, want, f)))
    gd = Guards("cuda")
    x, y, out = gd.freeze(got, "a"), gd.freeze(got[::-1].copy(), "b"), gd.out(1, 12, words=72, name="product")
    ctx.fq12_vec_op(czk_amd.binding.CZK_FQ12_OP_MUL, x.ptr, y.ptr, n=12, out=out.ptr, mem=czk_amd.CZK_MEM_DEVICE)
    ctx.sync()
    assert np.array_equal(gd.check()[0][0], M.gt_lanes([[(p + q) % R_MOD for p, q in zip(u, w)] for u, w in zip(want, want[::-1])]).reshape(12, 72))


@pytest.mark.gpu
def test_argument_rules_and_the_empty_calls(ctx):
    import czk_amd
    import torch
    B = czk_amd.binding
    buf = torch.zeros(8192, dtype=torch.int64, device="cuda")
    keep = buf.clone()
    p = buf.data_ptr()
    ms = np.zeros((33, 4), np.uint64)
    pair = lambda lpp, parties, n, a=p, out=p, mac=ms: ctx.share_pairing(lpp, parties, mac, a, None, p, None, p, None, p, None, p, out, n)   # noqa: E731
    opn = lambda lpp, parties, n, v=p, out=p, mac=ms: ctx.gt_share_open(lpp, parties, mac, v, n, out)                                       # noqa: E731
    scl = lambda lpp, parties, n, f=p, out=p, mac=ms: ctx.gt_share_scale(lpp, parties, mac, p, f, out, n)                                   # noqa: E731
    vec = lambda op, n, a=p, b=p, out=p, mem=1: ctx.fq12_vec_op(op, a, b, n=n, out=out, mem=mem)                                             # noqa: E731
    assert pair(2, 2, 0) == 0 and pair(1, 0, 5) == 0 and opn(2, 2, 0) == 0 and opn(2, 0, 3) == 0            # empty: nothing touched
    assert pair(2, 2, 0, a=None, out=None, mac=None) == 0 and opn(1, 3, 0, v=None, out=None) == 0
    scl(2, 2, 0, f=None, out=None)
    scl(1, 0, 4)
    vec(B.CZK_FQ12_OP_MUL, 0, a=None, b=None, out=None)
    ctx.sync()
    assert torch.equal(buf, keep)
    for call in (lambda: pair(3, 2, 1), lambda: pair(0, 2, 1), lambda: pair(2, 33, 1), lambda: pair(2, 2, 1, a=None), lambda: pair(2, 2, 1, out=None),
                 lambda: pair(2, 2, 1, mac=None), lambda: opn(3, 2, 1), lambda: opn(2, 33, 1), lambda: opn(2, 2, 1, v=None), lambda: opn(2, 2, 1, out=None),
                 lambda: opn(2, 2, 1, mac=None), lambda: scl(5, 2, 1), lambda: scl(1, 33, 1), lambda: scl(2, 2, 1, f=None), lambda: scl(2, 2, 1, out=None),
                 lambda: scl(2, 2, 1, mac=None), lambda: vec(3, 1), lambda: vec(B.CZK_FQ12_OP_MUL, 1, b=None), lambda: vec(B.CZK_FQ12_OP_INV, 1, a=None),
                 lambda: vec(B.CZK_FQ12_OP_DIV, 1, out=None), lambda: vec(B.CZK_FQ12_OP_MUL, 1, mem=7)):
        with pytest.raises(czk_amd.CzkError) as e:
            call()
        assert e.value.code == 3, e.value                              # CZK_ERR_ARG
    ctx.sync()
    assert torch.equal(buf, keep)
    L = czk_amd.lib()                                                  # a null context or count pointer is rejected, not crashed
    import ctypes as C
    sz = C.c_size_t
    assert L.czk_share_pairing(None, sz(1), sz(1), None, None, None, None, None, None, None, None, None, None, None, sz(1), None) == 3
    assert L.czk_gt_share_open(ctx._h, sz(1), sz(1), None, None, sz(1), None, None) == 3
    one = _dev(M.gt_lanes([[0]]))                                      # additive shares need no key
    out = torch.empty((1, 72), dtype=torch.int64, device="cuda")
    assert ctx.gt_share_open(1, 1, None, one.data_ptr(), 1, out.data_ptr()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint64)[0], M.gt_limbs(PR.FQ12_ONE))
