"""Windowed fixed-base MSM on the GPU (czk_fixed_base_create / _layout / _msm) and czk_fr_lagrange_coefficients.

The expected points come from the checker's restatement of FixedBaseMSM for any base (oracle/ec_tmpl.h fixed_base_msm, called directly through
orc.lib() with the same base); for the generator also from czk_fixed_base_points, the double-and-add every other test rests on.  Every
comparison is bit for bit in affine limbs and infinity flags.  The checker runs once per (group, base) on the longest scalar vector; the
affine result of a scalar does not depend on its neighbours, so shorter calls compare with a prefix."""
import ctypes as C

import numpy as np
import pytest

from groth16_real_key import omega_for
from util import R_MOD, ints_to_limbs, limbs_to_ints, rand_fr_canonical

pytestmark = pytest.mark.gpu
WIDTHS = (1, 3, 8, 11, 13, 0)
SIZES = (0, 1, 33, 129, 1000)
N_MAX = max(SIZES)
K0 = limbs_to_ints(rand_fr_canonical(0xF1B0, 1))[0]


def _half_digits(w):
    """every w-bit digit below bit 252 is 2^(w-1) (so the value stays below r)"""
    return sum(1 << (w * j + w - 1) for j in range(253) if w * j + w - 1 < 252)


def _edge_scalars():
    e = [0, 1, 2, R_MOD - 1, R_MOD - 2, (1 << 252) - 1, 1 << 252]
    for j in (1, 2, 11, 22):
        e += [1 << (11 * j), (1 << (11 * j)) - 1]
    e += [_half_digits(w) for w in (1, 3, 8, 11, 13, 7, 16, 20)]
    assert all(0 <= v < R_MOD for v in e) and len(e) <= 33
    return e


EDGE = _edge_scalars()
SCALARS = np.vstack([ints_to_limbs(EDGE, 4), rand_fr_canonical(0xF1B1, N_MAX - len(EDGE))])
SCALARS_MONT = ints_to_limbs([v * (1 << 256) % R_MOD for v in limbs_to_ints(SCALARS)], 4)


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def _oracle(orc, group, base, k):
    k = np.ascontiguousarray(k, np.uint64).reshape(-1, 4)
    base = np.ascontiguousarray(base, np.uint64)
    out = np.zeros((k.shape[0], 12 * group), dtype=np.uint64)
    inf = np.zeros(k.shape[0], dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    getattr(orc.lib(), f"orc_g{group}_fixed_base_msm")(p(base), p(k), C.c_size_t(k.shape[0]), p(out), p(inf), C.c_int(0))
    return out, inf


@pytest.fixture(scope="module")
def bases(ctx, orc):
    """{(group, name): (base limbs, expected points, expected flags)} for the generator and [k0] G, computed once"""
    out = {}
    for group in (1, 2):
        gen = orc.generator_affine(group)
        other = ctx.fixed_base_points(group, ints_to_limbs([K0], 4))[0]
        assert np.array_equal(other, _oracle(orc, group, gen, ints_to_limbs([K0], 4))[0][0])
        for name, base in (("generator", gen), ("k0", other)):
            want, winf = _oracle(orc, group, base, SCALARS)
            want.setflags(write=False)
            winf.setflags(write=False)
            out[group, name] = (np.ascontiguousarray(base, np.uint64), want, winf)
    return out


def _device_msm(ctx, fb, k, n, form, aw):
    import torch
    import czk_amd
    kd = torch.from_numpy(np.ascontiguousarray(k[:n]).view(np.int64).copy()).to("cuda:0")
    pts = torch.empty((n, aw), dtype=torch.int64, device="cuda:0")
    inf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    ctx.fixed_base_msm(fb, kd.data_ptr(), out=pts.data_ptr(), n=n, scalar_form=form, mem=czk_amd.CZK_MEM_DEVICE, out_inf=inf.data_ptr())
    ctx.sync()
    return pts.cpu().numpy().view(np.uint64), inf.cpu().numpy()


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("group", (1, 2))
def test_parity_with_the_checker(ctx, bases, group, w):
    import czk_amd
    aw = 12 * group
    for name in ("generator", "k0"):
        base, want, winf = bases[group, name]
        fb = ctx.fixed_base(group, base, window=w, n_hint=N_MAX)
        lw, lwin, lbytes = fb.layout()
        assert (lw == w or w == 0) and 1 <= lw <= 20 and lbytes > 0
        for n in SIZES:
            combos = [(czk_amd.CZK_SCALAR_CANONICAL, "host"), (czk_amd.CZK_SCALAR_MONTGOMERY, "device")]
            if n == N_MAX:
                combos += [(czk_amd.CZK_SCALAR_MONTGOMERY, "host"), (czk_amd.CZK_SCALAR_CANONICAL, "device")]
            for form, mem in combos:
                k = SCALARS if form == czk_amd.CZK_SCALAR_CANONICAL else SCALARS_MONT
                if mem == "host":
                    got, ginf = ctx.fixed_base_msm(fb, k[:n], scalar_form=form)
                elif n:
                    got, ginf = _device_msm(ctx, fb, k, n, form, aw)
                else:   # n = 0 with null device pointers: CZK_OK, nothing written
                    ctx.fixed_base_msm(fb, 0, out=0, n=0, scalar_form=form, mem=czk_amd.CZK_MEM_DEVICE, out_inf=0)
                    continue
                assert got.shape == (n, aw) and ginf.shape == (n,)
                assert np.array_equal(ginf, winf[:n]), (name, n, form, mem, np.nonzero(ginf != winf[:n])[0][:8])
                bad = np.nonzero((got != want[:n]).any(axis=1))[0]
                assert bad.size == 0, (name, n, form, mem, bad[:8])
        if name == "generator":   # the existing anchor: czk_fixed_base_points writes (0, 1) for infinity, without a flag
            anchor = ctx.fixed_base_points(group, SCALARS)
            got, ginf = ctx.fixed_base_msm(fb, SCALARS)
            assert np.array_equal(got, anchor) and ginf[0] == 1 and ginf.sum() == 1
        fb.release()


def _fq_one():
    import pyref as P
    return P.FQ_MONT_R


def _sqrt_mod_q(a, q):
    """Tonelli-Shanks"""
    if pow(a, (q - 1) // 2, q) != 1:
        return None
    s, t = 0, q - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (q - 1) // 2, q) != q - 1:
        z += 1
    m, c, u, r = s, pow(z, t, q), pow(a, t, q), pow(a, (t + 1) // 2, q)
    while u != 1:
        i, v = 0, u
        while v != 1:
            v, i = v * v % q, i + 1
        b = pow(c, 1 << (m - i - 1), q)
        m, c, u, r = i, b * b % q, u * b * b % q, r * b % q
    return r


def test_base_outside_the_subgroup(ctx, orc):
    """G1 point of smallest x >= 1 on y^2 = x^3 + 1: not annihilated by r, so the multiples meet the complete addition's special cases"""
    import czk_amd
    import pyref as P
    x = 1
    while (y := _sqrt_mod_q((x ** 3 + 1) % P.Q_MOD, P.Q_MOD)) is None:
        x += 1
    assert y * y % P.Q_MOD == (x ** 3 + 1) % P.Q_MOD
    assert P.ec_mul(P.F1, P.R_MOD, (x, y)) is not P.INF
    base = orc.ints_to_limbs([P.fq_to_mont(x), P.fq_to_mont(y)], 6).reshape(-1)
    reg = ctx.register_bases(czk_amd.CZK_G1, base.reshape(1, 12), None, mem=czk_amd.CZK_MEM_HOST | czk_amd.CZK_MEM_ANY_POINTS)
    assert reg.check_subgroup() == 1
    reg.release()
    k = np.vstack([ints_to_limbs(list(range(41)), 4), rand_fr_canonical(0xF1B2, 216)])
    want, winf = _oracle(orc, 1, base, k)
    for w in (3, 8):
        fb = ctx.fixed_base(czk_amd.CZK_G1, base, window=w)
        got, ginf = ctx.fixed_base_msm(fb, k)
        assert np.array_equal(ginf, winf) and np.array_equal(got, want), w
        fb.release()


def test_handle_behaviour(ctx, orc):
    import czk_amd
    gen = orc.generator_affine(1)
    for w in (1, 3, 8, 11, 13, 20):
        fb = ctx.fixed_base(czk_amd.CZK_G1, gen, window=w)
        lw, lwin, lbytes = fb.layout()
        assert lw == w and lwin == -(-253 // w) + (1 if 253 % w == 0 else 0)
        assert lbytes >= lwin * (1 << (w - 1)) * 96
        if w == 8:
            a = ctx.fixed_base_msm(fb, SCALARS[:129])
            b = ctx.fixed_base_msm(fb, SCALARS[:129])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        fb.release()
        fb.release()   # idempotent on the Python handle
    fb = ctx.fixed_base(czk_amd.CZK_G1, gen, window=8)   # release, then create again
    assert np.array_equal(ctx.fixed_base_msm(fb, SCALARS[:33])[0], ctx.fixed_base_points(czk_amd.CZK_G1, SCALARS[:33]))
    fb.release()
    inf01 = np.concatenate([np.zeros(6, np.uint64), orc.ints_to_limbs([_fq_one()], 6).reshape(-1)])
    inf2 = np.concatenate([np.zeros(12, np.uint64), orc.ints_to_limbs([_fq_one()], 6).reshape(-1), np.zeros(6, np.uint64)])
    for group, base, w in ((1, gen, 21), (1, None, 0), (1, inf01, 0), (1, np.zeros(12, np.uint64), 0), (2, inf2, 0)):
        with pytest.raises(czk_amd.CzkError) as ei:
            ctx.fixed_base(group, base, window=w)
        assert ei.value.code == 3, (group, w)
    fb = ctx.fixed_base(czk_amd.CZK_G1, gen, window=4)
    with pytest.raises(czk_amd.CzkError) as ei:
        ctx.fixed_base_msm(fb, SCALARS[:4], scalar_form=7)
    assert ei.value.code == 3
    with pytest.raises(czk_amd.CzkError) as ei:
        ctx.fixed_base_msm(fb, None, out=None, n=4, mem=czk_amd.CZK_MEM_DEVICE)
    assert ei.value.code == 3
    fb.release()


def _lagrange_ref(log_d, tau, n_out):
    D = 1 << log_d
    omega = omega_for(log_d)
    z = (pow(tau, D, R_MOD) - 1) % R_MOD
    out, wj = [], 1
    for _ in range(n_out):
        if z:
            out.append(z * wj % R_MOD * pow(D * (tau - wj) % R_MOD, -1, R_MOD) % R_MOD)   # L_j(tau) = Z(tau) w^j / (D (tau - w^j))
        else:
            out.append(1 if wj == tau else 0)
        wj = wj * omega % R_MOD
    return out


@pytest.mark.parametrize("log_d", (0, 1, 2, 3, 4, 5, 6, 10))
def test_lagrange_coefficients(ctx, log_d):
    import torch
    import czk_amd
    D = 1 << log_d
    taus = [limbs_to_ints(rand_fr_canonical(0x1A6 + log_d, 1))[0]]
    if log_d >= 2:
        taus.append(pow(omega_for(log_d), 3, R_MOD))   # tau in the domain: one coefficient is 1, the rest 0
    for tau in taus:
        tau_m = ints_to_limbs([tau * (1 << 256) % R_MOD], 4)[0]
        for n_out in sorted({D, max(D - 3, 0)}):
            want = ints_to_limbs([v * (1 << 256) % R_MOD for v in _lagrange_ref(log_d, tau, n_out)], 4)
            got = ctx.fr_lagrange_coefficients(log_d, tau_m, n_out=n_out)
            assert got.shape == (n_out, 4) and np.array_equal(got, want), (log_d, n_out, tau == taus[-1])
            if n_out:
                dev = torch.empty((n_out, 4), dtype=torch.int64, device="cuda:0")
                ctx.fr_lagrange_coefficients(log_d, tau_m, n_out=n_out, out=dev.data_ptr(), mem=czk_amd.CZK_MEM_DEVICE)
                ctx.sync()
                assert np.array_equal(dev.cpu().numpy().view(np.uint64), want)
        if tau == taus[-1] and log_d >= 2:
            assert sum(_lagrange_ref(log_d, tau, D)) == 1 and _lagrange_ref(log_d, tau, D)[3] == 1
    with pytest.raises(czk_amd.CzkError) as ei:
        ctx.fr_lagrange_coefficients(log_d, ints_to_limbs([5], 4)[0], n_out=D + 1)
    assert ei.value.code == 3
