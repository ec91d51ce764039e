"""Parity tests proper: the HIP path (through the C ABI, libczk_hip.so) against the CPU checker (oracle/) on the
same seeded inputs -- bit-exact limbs for field/NTT results, affine equality for group results.  Run on a real
MI355X with `-m gpu`."""
import numpy as np
import pytest

from util import dot_mod_r, ints_to_limbs, limbs_to_ints, rand_fr_canonical, R_MOD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def czk():
    import czk_amd
    return czk_amd


def test_field_vector_ops_bit_exact(ctx, czk, orc):
    n = 5000
    a = rand_fr_canonical(11, n)
    b = rand_fr_canonical(12, n)
    edge = ints_to_limbs([0, 1, R_MOD - 1, R_MOD - 2, 2, 1 << 252], 4)
    a[:6], b[:6] = edge, edge[::-1]
    from czk_amd.binding import CZK_OP_ADD, CZK_OP_MUL, CZK_OP_SUB
    assert np.array_equal(ctx.fr_vec_op(CZK_OP_MUL, a, b), orc.fr_mul(a, b))
    assert np.array_equal(ctx.fr_vec_op(CZK_OP_ADD, a, b), orc.fr_add(a, b))
    assert np.array_equal(ctx.fr_vec_op(CZK_OP_SUB, a, b), orc.fr_sub(a, b))
    assert np.array_equal(ctx.fr_into_repr(a), orc.fr_into_repr(a))
    assert np.array_equal(ctx.fr_from_repr(a), orc.fr_from_repr(a))
    k = a[7].copy()
    assert np.array_equal(ctx.fr_vec_scale(a, k), orc.fr_mul(a, np.tile(k, (n, 1))))
    # local half of Beaver multiplication (share/field.rs:116-126): z - y*sx - x*oy (+ sx*oy for the king)
    x, y, z = rand_fr_canonical(13, n), rand_fr_canonical(14, n), rand_fr_canonical(15, n)
    sx, oy = a, b
    base = orc.fr_sub(orc.fr_sub(z, orc.fr_mul(y, sx)), orc.fr_mul(x, oy))
    assert np.array_equal(ctx.fr_beaver_combine(x, y, z, sx, oy, False), base)
    assert np.array_equal(ctx.fr_beaver_combine(x, y, z, sx, oy, True), orc.fr_add(base, orc.fr_mul(sx, oy)))
    # empty input
    assert ctx.fr_vec_op(CZK_OP_MUL, a[:0], b[:0]).size == 0


def test_domain_constants_match_reference_rule(ctx, orc):
    for log_d in (0, 1, 5, 16, 21, 23, 47):
        got, want = ctx.domain_constants(log_d), orc.domain_constants(log_d)
        for k in want:
            assert np.array_equal(got[k], want[k]), (log_d, k)
    import czk_amd
    with pytest.raises(czk_amd.CzkError) as e:     # D::new -> None above 2^47 (radix2/mod.rs:61-63)
        ctx.domain_constants(48)
    assert e.value.code == 1


@pytest.mark.parametrize("log_d", [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16])
def test_ntt_all_kinds_bit_exact(ctx, czk, orc, log_d):
    d = 1 << log_d
    for in_len in sorted({d, max(1, d - 3), (d + 1) // 2}):
        lanes = 2
        x = orc.fr_from_repr(rand_fr_canonical(100 + log_d, lanes * in_len)).reshape(lanes, in_len, 4)
        for kind in (czk.CZK_FFT, czk.CZK_IFFT, czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT):
            buf = np.full((lanes, d, 4), 0xDEADBEEFDEADBEEF, dtype=np.uint64)   # garbage tail must be ignored
            buf[:, :in_len] = x
            ctx.ntt_fr(buf, log_d, kind, lanes=lanes, in_len=in_len)
            for ln in range(lanes):
                want = orc.ntt_fr(x[ln], log_d, kind, in_len)
                assert np.array_equal(buf[ln], want), (log_d, in_len, kind, ln)


@pytest.mark.parametrize("log_d", [17, 18, 19, 20, 21])
def test_ntt_large_sizes_bit_exact_four_lanes(ctx, czk, orc, log_d):
    """Every output limb of all four transform kinds against the checker's io/oi restatement (radix2/fft.rs:140-260) at
    2^17 .. 2^21 (the three-pass decompositions, incl. the 2^21 BASELINE domain), 4 share lanes in device memory; the
    inverse kinds run on a ragged prefix with a garbage tail (resize(size, zero), radix2/mod.rs:100-101).  The checker's
    answers are the committed digests of tests/golden/fullsize_digests.json (tests/fullsize.py; one case per session is
    also recomputed live)."""
    import torch
    import fullsize
    d, lanes = 1 << log_d, 4
    x = fullsize.ntt_input(orc, log_d, lanes)
    for kind in (czk.CZK_FFT, czk.CZK_IFFT, czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT):
        in_len = fullsize.ntt_in_len(kind, d)
        buf = x.copy()
        buf[:, in_len:] = 0xDEADBEEFDEADBEEF
        t = torch.from_numpy(buf.view(np.int64)).cuda()
        ctx.ntt_fr(t.data_ptr(), log_d, kind, lanes=lanes, in_len=in_len, mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        got = t.cpu().numpy().view(np.uint64)
        fullsize.expect(f"ntt_2e{log_d}_{fullsize.KINDS[kind]}", {f"lane{ln}": got[ln].tobytes() for ln in range(lanes)}, orc)


def test_ntt_size_errors(ctx, czk):
    buf = np.zeros((8, 4), dtype=np.uint64)
    with pytest.raises(czk.CzkError) as e:      # assert!(coeffs.len() <= self.size()) radix2/mod.rs:100
        ctx.ntt_fr(buf, 3, czk.CZK_FFT, in_len=9)
    assert e.value.code == 1
    with pytest.raises(czk.CzkError) as e:
        ctx.ntt_fr(buf, 48, czk.CZK_FFT, in_len=1)
    assert e.value.code == 1


def _fr_pow(orc, base, e):
    acc = orc.fr_from_repr(ints_to_limbs([1], 4))[0]
    base = base.copy()
    while e:
        if e & 1:
            acc = orc.fr_mul(acc, base)
        base = orc.fr_mul(base, base)
        e >>= 1
    return acc


@pytest.mark.parametrize("log_d,lanes", [(21, 2), (22, 2), (23, 2)])
def test_ntt_device_memory_and_full_size_properties(ctx, czk, orc, log_d, lanes):
    """BASELINE sizes D = 2^21 (configs[1]; three 7-stage passes), 2^22 and 2^23 (configs[4]; four passes), device-resident,
    2 lanes: round trips restore the input exactly; forward transforms agree with Horner evaluation at w^i / 22 w^i
    (radix2/mod.rs:320-360) at sampled points."""
    import torch
    d = 1 << log_d
    x = orc.fr_from_repr(rand_fr_canonical(777, lanes * d)).reshape(lanes, d, 4)
    t = torch.from_numpy(x.view(np.int64)).cuda()
    k = orc.domain_constants(log_d)
    w, g = k["group_gen"], k["generator"]
    for fwd, inv in ((czk.CZK_FFT, czk.CZK_IFFT), (czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT)):
        ctx.ntt_fr(t.data_ptr(), log_d, fwd, lanes=lanes, mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        ev = t.cpu().numpy().view(np.uint64)
        for i in (0, 1, 2, 12345, d // 2, d - 1):
            pt = _fr_pow(orc, w, i)
            if fwd == czk.CZK_COSET_FFT:
                pt = orc.fr_mul(pt, g)
            for ln in range(lanes):
                assert np.array_equal(ev[ln, i], orc.fr_horner(x[ln], pt)), (fwd, i, ln)
        ctx.ntt_fr(t.data_ptr(), log_d, inv, lanes=lanes, mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        assert np.array_equal(t.cpu().numpy().view(np.uint64), x)
    # linearity on the device buffer: NTT(a + b) == NTT(a) + NTT(b)
    s = orc.fr_add(x[0], x[1])
    ts = torch.from_numpy(s.view(np.int64)).cuda()
    ctx.ntt_fr(ts.data_ptr(), log_d, czk.CZK_FFT, lanes=1, mem=czk.CZK_MEM_DEVICE)
    ctx.ntt_fr(t.data_ptr(), log_d, czk.CZK_FFT, lanes=2, mem=czk.CZK_MEM_DEVICE)
    ctx.sync()
    tt = t.cpu().numpy().view(np.uint64)
    assert np.array_equal(ts.cpu().numpy().view(np.uint64), orc.fr_add(tt[0], tt[1]))


def _bases(ctx, g, n, seed):
    k = rand_fr_canonical(seed, n)
    return k, ctx.fixed_base_points(g, k)


def _same_point(ctx, orc, g, have_jac, want_jac):
    want_aff, want_inf = orc.jac_to_affine(g, want_jac)
    have_aff, have_inf = ctx.jac_to_affine(g, have_jac)
    chk_aff, chk_inf = orc.jac_to_affine(g, have_jac)     # product's own to-affine agrees with the checker's
    assert chk_inf == bool(have_inf[0]) and (chk_inf or np.array_equal(chk_aff, have_aff[0]))
    return bool(have_inf[0]) == want_inf and (want_inf or np.array_equal(have_aff[0], want_aff))


@pytest.mark.parametrize("g", [1, 2])
def test_fixed_base_points_match_scalar_mul(ctx, czk, orc, g):
    n = 40
    k = rand_fr_canonical(21 + g, n)
    k[0] = ints_to_limbs([1], 4)[0]
    k[1] = ints_to_limbs([2], 4)[0]
    k[2] = ints_to_limbs([R_MOD - 1], 4)[0]
    pts = ctx.fixed_base_points(g, k)
    gen = pts[0]                                  # k = 1 -> the generator itself
    for i in range(n):
        want, inf = orc.jac_to_affine(g, orc.scalar_mul(g, gen, False, k[i]))
        assert not inf and np.array_equal(pts[i], want), (g, i)
    if g == 1:
        assert all(orc.g1_on_curve(p) for p in pts)


@pytest.mark.parametrize("g,n", [(1, 1), (1, 2), (1, 10), (1, 31), (1, 33), (1, 300), (1, 4096), (2, 1), (2, 10), (2, 33), (2, 700)])
def test_msm_matches_reference_pippenger(ctx, czk, orc, g, n):
    """Pippenger parity in affine (test-templates/src/msm.rs:16-33), with the reference's special cases: zero
    scalars (variable_base.rs:19), unit scalars (:44-48), infinity bases, equal and opposite bases."""
    _, bases = _bases(ctx, g, n, 300 + n)
    inf = np.zeros(n, dtype=np.uint8)
    sc = rand_fr_canonical(400 + n, 2 * n).reshape(2, n, 4)
    if n >= 10:
        bases[3] = bases[2]                                            # equal points
        aw = bases.shape[1] // 2
        neg = bases[4].copy()
        if g == 1:
            neg[aw:] = orc.fq_neg(bases[4][aw:])
        else:
            neg[aw:] = np.concatenate([orc.fq_neg(bases[4][aw:aw + 6]), orc.fq_neg(bases[4][aw + 6:])])
        bases[5] = neg                                                 # opposite points
        inf[7] = 1
        sc[:, 0] = 0
        sc[:, 1] = ints_to_limbs([1], 4)[0]
        sc[:, 2] = sc[:, 3] = ints_to_limbs([5], 4)[0]
        sc[:, 4] = sc[:, 5] = ints_to_limbs([R_MOD - 3], 4)[0]
    b = ctx.register_bases(g, bases, inf)
    assert len(b) == n
    got = ctx.msm(b, sc, lanes=2)
    for ln in range(2):
        assert _same_point(ctx, orc, g, got[ln], orc.msm(g, bases, inf, sc[ln])), (g, n, ln)
    # AffineCurve::multi_scalar_mul: Montgomery scalars, one more scalar than bases (h vs h_query, lib.rs:304)
    scm = orc.fr_from_repr(np.vstack([sc[0], ints_to_limbs([77], 4)]))
    got_m = ctx.msm(b, scm, lanes=1, scalar_form=czk.CZK_SCALAR_MONTGOMERY)
    assert _same_point(ctx, orc, g, got_m[0], orc.multi_scalar_mul(g, bases, inf, scm))
    # fewer scalars than bases: size = min(len) (variable_base.rs:16)
    if n > 2:
        got_s = ctx.msm(b, sc[0, : n - 1], lanes=1)
        assert _same_point(ctx, orc, g, got_s[0], orc.msm(g, bases[: n - 1], inf[: n - 1], sc[0, : n - 1]))
    b.release()
    # one-shot entry point with the reference's argument order
    one = ctx.msm_oneshot(g, bases, inf, sc[0])
    assert _same_point(ctx, orc, g, one[0], orc.msm(g, bases, inf, sc[0]))


def test_msm_empty_and_all_zero(ctx, czk, orc):
    _, bases = _bases(ctx, 1, 8, 5)
    b = ctx.register_bases(1, bases, None)
    out = ctx.msm(b, np.zeros((8, 4), dtype=np.uint64))
    assert ctx.jac_to_affine(1, out[0])[1][0] == 1          # all-zero scalars -> infinity
    out = ctx.msm(b, np.zeros((0, 4), dtype=np.uint64), n_scalars=0)
    assert ctx.jac_to_affine(1, out[0])[1][0] == 1          # empty -> zero()
    b.release()
    b0 = ctx.register_bases(1, np.zeros((0, 12), dtype=np.uint64), None)
    out = ctx.msm(b0, rand_fr_canonical(1, 4))
    assert ctx.jac_to_affine(1, out[0])[1][0] == 1
    b0.release()


@pytest.mark.parametrize("g,n", [(1, (1 << 20) + 1), (1, (1 << 21) - 1), (2, (1 << 17) + 1), (2, (1 << 20) + 1), (1, 1 << 18), (1, 3 * (1 << 20) + 7), (1, (1 << 22) + 1),
                                 (2, (1 << 22) + 1), (1, (1 << 23) - 1)])
def test_msm_full_size_known_discrete_logs(ctx, czk, orc, g, n):
    """Size-independent check at BASELINE scale, 4 share lanes: bases P_i = [k_i] G, so MSM(P, s) must equal
    [sum k_i s_i mod r] G; plus linearity between lanes.  Sizes: the Groth16 a/b queries and the h query at 2^20
    constraints (configs[1]), G2 queries, the a/b (G1 and G2) and h queries at 2^22 constraints (configs[4]: 2^22+1, 2^23-1), a KZG
    commit of a 2^18-coefficient polynomial (Plonk, configs[2]) and a non-power-of-two ~3N commit as Marlin's largest polynomials
    at 2^20 (configs[3]; poly-commit/src/kzg10/mod.rs:159-162)."""
    import torch
    lanes = 4
    k = rand_fr_canonical(0xBA5E5, n)
    aw = 12 if g == 1 else 24
    kd = torch.from_numpy(k.view(np.int64)).cuda()
    pts = torch.empty((n, aw), dtype=torch.int64, device="cuda")
    ctx.fixed_base_points(g, kd.data_ptr(), out=pts.data_ptr(), n=n, mem=czk.CZK_MEM_DEVICE)
    b = ctx.register_bases(g, pts.data_ptr(), None, n=n, mem=czk.CZK_MEM_DEVICE)
    del pts
    s = rand_fr_canonical(0xC0FFEE, lanes * n).reshape(lanes, n, 4)
    sd = torch.from_numpy(s.view(np.int64)).cuda()
    out = ctx.msm(b, sd.data_ptr(), n_scalars=n, lanes=lanes, mem=czk.CZK_MEM_DEVICE)
    gen = ctx.fixed_base_points(g, ints_to_limbs([1], 4))[0]
    for ln in range(lanes):
        e = dot_mod_r(k, s[ln])
        assert _same_point(ctx, orc, g, out[ln], orc.scalar_mul(g, gen, False, ints_to_limbs([e], 4)[0])), (g, ln)
    # linearity: MSM(s0) + MSM(s1) == MSM(s0 + s1)
    ssum = orc.fr_into_repr(orc.fr_add(orc.fr_from_repr(s[0]), orc.fr_from_repr(s[1])))
    out_sum = ctx.msm(b, ssum, lanes=1)
    assert _same_point(ctx, orc, g, out_sum[0], orc.jac_add(g, out[0], out[1]))
    b.release()


@pytest.mark.parametrize("g,n,oracle_lanes", [(1, (1 << 20) + 1, (0, 3)), (2, (1 << 20) + 1, (1,))])
def test_msm_full_size_matches_reference_pippenger(ctx, czk, orc, g, n, oracle_lanes):
    """The a/b-query MSM of BASELINE configs[1] (2^20 + 1 points, 4 share lanes, one infinity base like the real key)
    against the checker's Pippenger itself (variable_base.rs:12-106: c = 16, 16 windows of 65 535 buckets) -- not only via
    discrete logs -- compared in affine.  Lanes the checker does not recompute are covered by the discrete-log identity.
    The checker's answers -- and its FixedBaseMSM answer for the 2^20 + 1 bases czk_fixed_base_points generates -- are the committed
    digests of tests/golden/fullsize_digests.json (tests/fullsize.py; one case per session is also recomputed live)."""
    import torch
    import fullsize
    lanes = 4
    assert n == fullsize.FULL_N
    k = rand_fr_canonical(0xBA5E5 + 3, n)
    aw = 12 if g == 1 else 24
    kd = torch.from_numpy(k.view(np.int64)).cuda()
    pts = torch.empty((n, aw), dtype=torch.int64, device="cuda")
    ctx.fixed_base_points(g, kd.data_ptr(), out=pts.data_ptr(), n=n, mem=czk.CZK_MEM_DEVICE)
    inf = np.zeros(n, dtype=np.uint8)
    inf[0] = 1
    infd = torch.from_numpy(inf).cuda()
    b = ctx.register_bases(g, pts.data_ptr(), infd.data_ptr(), n=n, mem=czk.CZK_MEM_DEVICE)
    bases_host = pts.cpu().numpy().view(np.uint64)
    fullsize.expect(f"bases_g{g}_seed3_2e20p1", {"points": bases_host.tobytes()}, orc)      # the GPU's synthetic key = the reference generator's algorithm
    s = fullsize.msm_scalars(orc, n, lanes)                                                  # Montgomery scalars, as the MPC wrappers pass them; a unit and a zero on lane 2
    sd = torch.from_numpy(s.view(np.int64)).cuda()
    out = ctx.msm(b, sd.data_ptr(), n_scalars=n, lanes=lanes, scalar_form=czk.CZK_SCALAR_MONTGOMERY, mem=czk.CZK_MEM_DEVICE)
    aff, ainf = ctx.jac_to_affine(g, out)
    for ln in oracle_lanes:
        fullsize.expect(f"msm_g{g}_2e20p1_lane{ln}", {"affine": fullsize.affine_bytes(aff[ln], ainf[ln])}, orc)
    gen = ctx.fixed_base_points(g, ints_to_limbs([1], 4))[0]
    k[0] = 0
    for ln in set(range(lanes)) - set(oracle_lanes):
        e = dot_mod_r(k, orc.fr_into_repr(s[ln]))
        assert _same_point(ctx, orc, g, out[ln], orc.scalar_mul(g, gen, False, ints_to_limbs([e], 4)[0])), (g, ln)
    b.release()


def test_witness_map_matches_reference_sequence(ctx, czk, orc):
    """R1CStoQAP::witness_map (r1cs_to_qap.rs:47-113) for a single prover on device buffers, squaring circuit
    of N = 1000 constraints (proof.rs:304-344): a_i = b_i = w_i, c_i = w_{i+1}, a[N] = 1, a[N+1] = out."""
    import torch
    from czk_amd.binding import CZK_OP_MUL
    n_c, log_d = 1000, 10
    d = 1 << log_d
    one = orc.fr_from_repr(ints_to_limbs([1], 4))
    w = [orc.fr_from_repr(rand_fr_canonical(9, 1))]
    for _ in range(n_c):
        w.append(orc.fr_sqr(w[-1]))
    w = np.vstack(w)                       # w_0 .. w_N (w_N = public output)
    a = np.zeros((d, 4), dtype=np.uint64)
    a[:n_c] = w[:n_c]
    a[n_c], a[n_c + 1] = one[0], w[n_c]    # instance assignment copy (r1cs_to_qap.rs:79-83)
    bq = np.zeros((d, 4), dtype=np.uint64)
    bq[:n_c] = w[:n_c]
    c = np.zeros((d, 4), dtype=np.uint64)
    c[:n_c] = w[1:n_c + 1]
    want = orc.witness_map_plain(a, bq, c, log_d)
    ta, tb, tc = (torch.from_numpy(v.view(np.int64).copy()).cuda() for v in (a, bq, c))
    ctx.witness_map_pre(ta.data_ptr(), tb.data_ptr(), log_d, 1)
    ctx.fr_vec_op(CZK_OP_MUL, ta.data_ptr(), tb.data_ptr(), out=ta.data_ptr(), n=d, mem=czk.CZK_MEM_DEVICE)
    ctx.witness_map_post(ta.data_ptr(), tc.data_ptr(), log_d, 1)
    ctx.sync()
    h = ta.cpu().numpy().view(np.uint64)
    assert np.array_equal(h, want)
    # the quotient is exact: deg h <= D - 2, so the top coefficient is zero
    assert not h[d - 1].any()


@pytest.mark.parametrize("n_constraints", [10, 1024, 8])
def test_groth16_local_pipeline_config0_matches_reference(ctx, czk, orc, n_constraints):
    """BASELINE configs[0] (`bench.zsh groth16 spdz 10 2`: exactly 10 constraints, domain 16, 2 SPDZ parties; also 2^10
    constraints, domain 2^11): the complete per-party local compute of bench.py's step -- witness map with the Beaver
    local half and device-local opens, then the five MSMs on every share lane -- against the checker: per lane the same
    NTT / pointwise sequence (r1cs_to_qap.rs:47-113, share/field.rs:97-127) and Pippenger (variable_base.rs) on the
    same inputs."""
    import torch
    from czk_amd.provers import Groth16Local
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        c2 = czk.Context(0, ts.cuda_stream)
        p = Groth16Local(czk, c2, n_constraints, 2)
        assert p.N == n_constraints and p.D == {10: 16, 8: 16, 1024: 2048}[n_constraints] and p.lanes == 4
        a0, b0, c0 = (t.cpu().numpy().view(np.uint64).copy() for t in (p.a0, p.b0, p.c0))
        tx, ty, tz = (t.cpu().numpy().view(np.uint64).copy() for t in (p.tx, p.ty, p.tz))
        wit, asg = p.wit.cpu().numpy().view(np.uint64).copy(), p.asg.cpu().numpy().view(np.uint64).copy()
        p.step()
        torch.cuda.synchronize()
        h_gpu = p.ab.cpu().numpy().view(np.uint64)
        assert not bool(p.chk.any().item())
    L, D, ld = 4, p.D, p.log_d
    # checker: lane-wise witness map with the Beaver local half
    A = [orc.witness_map_pre(a0[ln], b0[ln], ld) for ln in range(L)]
    sa = [orc.fr_add(A[ln][0], tx[ln]) for ln in range(L)]
    sb = [orc.fr_add(A[ln][1], ty[ln]) for ln in range(L)]
    sx, oy = orc.fr_add(sa[0], sa[2]), orc.fr_add(sb[0], sb[2])            # open = sum of the parties' sh lanes
    for ln in range(L):
        ab = orc.fr_sub(orc.fr_sub(tz[ln], orc.fr_mul(ty[ln], sx)), orc.fr_mul(tx[ln], oy))
        if ln < 2:
            ab = orc.fr_add(ab, orc.fr_mul(sx, oy))                        # king applies the shift (both lanes)
        h = orc.witness_map_post(ab, c0[ln], ld)
        assert np.array_equal(h_gpu[ln], h), ln
    # the reconstructed h is the single prover's h (shares are additive; MAC key = 1 makes mac lane == sh lane)
    h_sum = orc.fr_add(h_gpu[0], h_gpu[2])
    a_sum, b_sum, c_sum = (orc.fr_add(v[0], v[2]) for v in (a0, b0, c0))
    assert np.array_equal(h_sum, orc.witness_map_plain(a_sum, b_sum, c_sum, ld))
    # MSM results per lane vs the checker's Pippenger on the same (bases, scalars); bases are read back from the
    # registered handles' inputs by regenerating them with the same seeds
    from util import rand_fr_canonical
    N = p.N
    for name, g, n, sd, inf_first, scal in (("h", 1, D - 1, 1, False, h_gpu), ("l", 1, N, 2, False, wit), ("a", 1, N + 1, 3, False, asg),
                                             ("b_g1", 1, N + 1, 4, True, asg), ("b_g2", 2, N + 1, 5, True, asg)):
        bases = ctx.fixed_base_points(g, rand_fr_canonical(0xBA5E5 + sd, n))
        inf = np.zeros(n, dtype=np.uint8)
        inf[0] = 1 if inf_first else 0
        for ln in range(L):
            want = orc.multi_scalar_mul(g, bases, inf, scal[ln].reshape(-1, 4))
            assert _same_point(ctx, orc, g, p.results[name][ln], want), (name, ln)
    c2.close()


@pytest.mark.parametrize("g,opt", [(1, "msm_sat"), (2, "msm_sat_g2")])
def test_msm_saturated_kernel_still_matches(czk, orc, g, opt):
    """LAB library (libczk_hip_lab.so): the options "msm_sat" / "msm_sat_g2" select the saturated accumulate kernels (k_accumulate<Fq>,
    k_accumulate<Fq2>) at registration; keep them covered."""
    c2 = czk.Context(0, lab=True, options={opt: 1})
    _, bases = _bases(c2, g, 500, 41)
    sc = rand_fr_canonical(42, 500)
    inf = np.zeros(500, dtype=np.uint8)
    b = c2.register_bases(g, bases, inf)
    assert _same_point(c2, orc, g, c2.msm(b, sc)[0], orc.msm(g, bases, inf, sc))
    b.release()
    c2.close()


@pytest.mark.parametrize("g,envs", [(1, ("msm_no_te",)), (1, ("msm_no_te", "msm_reduce_sat")), (2, ("msm_reduce_sat_g2",)), (2, ()),
                                    (2, ("msm_g2_mode=1",)), (2, ("msm_g2_mode=2",))])
def test_msm_fallback_reductions_still_match(czk, orc, g, envs):
    """The bucket reduction has three forms per group: u-form buckets (G1 twisted Edwards / G1 XYZZ for CZK_MEM_ANY_POINTS handles /
    G2 on unsaturated lane pairs, the defaults) and, in the LAB library only, the saturated kernels behind the options "msm_reduce_sat" /
    "msm_reduce_sat_g2"; "msm_g2_mode" = 1 / 2 selects the lane-pair G2 ACCUMULATE kernels (faster alone, slower per proof).  n = 20000 gives
    a bucket set of more than 1024 buckets, so the chunked level kernel runs as well as the tail kernels; lanes = 3 leaves a lane pair
    of the G2 kernels with an idle neighbour block.  Equal and opposite bases put P + P and P - P into the reduction itself."""
    c2 = czk.Context(0, lab=True, options={e.split("=")[0]: int(e.split("=")[1]) if "=" in e else 1 for e in envs})
    n = 20000
    _, bases = _bases(c2, g, n, 141)
    half = bases.shape[1] // 2
    bases[1] = bases[0]                                   # the same point twice
    bases[3] = bases[2]                                   # ... and a point with its inverse
    bases[3][half:] = orc.fq_neg(bases[2][half:]) if g == 1 else np.concatenate([orc.fq_neg(bases[2][half:half + 6]), orc.fq_neg(bases[2][half + 6:])])
    sc = rand_fr_canonical(142, 3 * n).reshape(3, n, 4)
    sc[:, :4] = 0
    sc[0, 0, 0], sc[0, 1, 0] = 5, 9                       # lane 0: buckets 5 and 9 of window 0 hold the same point -- the running sum doubles
    sc[0, 2, 0], sc[0, 3, 0] = 6, 8                       #         buckets 6 and 8 hold P and -P
    sc[1, 0, 0], sc[1, 1, 0] = 7, 7                       # lane 1: the accumulate kernel meets P + P
    sc[2, 2, 0], sc[2, 3, 0] = 3, 3                       # lane 2: ... and P - P
    inf = np.zeros(n, dtype=np.uint8)
    inf[[11, 500]] = 1
    b = c2.register_bases(g, bases, inf)
    got = c2.msm(b, sc, lanes=3)
    for ln in range(3):
        assert _same_point(c2, orc, g, got[ln], orc.msm(g, bases, inf, sc[ln])), (envs, ln)
    # the first four scalars alone (a short call: the c = 13 table set, 4096 buckets, so the level kernel runs): bucket 9 = P, 8 = -Q,
    # 6 = Q, 5 = P and nothing else -- the level kernel's running sum meets Q - Q and P + P
    head = np.ascontiguousarray(sc[:, :4])
    got = c2.msm(b, head, n_scalars=4, lanes=3)
    for ln in range(3):
        assert _same_point(c2, orc, g, got[ln], orc.msm(g, bases[:4], inf[:4], head[ln])), (envs, "head", ln)
    b.release()
    c2.close()


def test_msm_one_pass_sort_still_matches(czk, orc):
    """The option "msm_sort_onepass" selects the single-pass counting sort (one global atomic + one random store per entry), which
    nothing else reaches (a call never has more than 2048 partitions); keep it covered (product library)."""
    c2 = czk.Context(0, options={"msm_sort_onepass": 1})
    n = 5000
    _, bases = _bases(c2, 1, n, 43)
    sc = rand_fr_canonical(44, 2 * n).reshape(2, n, 4)
    inf = np.zeros(n, dtype=np.uint8)
    inf[[0, 17]] = 1
    b = c2.register_bases(1, bases, inf)
    got = c2.msm(b, sc, lanes=2)
    for ln in range(2):
        assert _same_point(c2, orc, 1, got[ln], orc.msm(1, bases, inf, sc[ln]))
    b.release()
    c2.close()


@pytest.mark.parametrize("c,lanes", [(13, 2), (20, 2), (21, 2), (22, 1)])
def test_msm_partition_scatter_widths(czk, orc, c, lanes):
    """Sorts with 4 / 512 / 1024 / 2048 partitions of 1024 buckets (c = 13 / 20 / 21 / 22) give the right result: the partition counts at which
    the scatter is launched with 256, 512, 512 and 1024 threads, which otherwise only calls of 2^20 points and more reach.  (Any thread count
    sorts correctly, so this covers each launch, not the choice between them.)  The key keeps its own width for this short call ("msm_fixed_c"), and one workspace slot (one lane at
    c = 22) keeps the bucket workspace near 0.6 GB."""
    c2 = czk.Context(0, options={"msm_slots": 1, "msm_window_g1": c, "msm_fixed_c": 1})
    n = 300
    _, bases = _bases(c2, 1, n, 45)
    sc = rand_fr_canonical(46, lanes * n).reshape(lanes, n, 4)
    inf = np.zeros(n, dtype=np.uint8)
    inf[[3, 250]] = 1
    b = c2.register_bases(1, bases, inf)
    assert b.layout_for(n)[0] == c
    got = c2.msm(b, sc, lanes=lanes)
    for ln in range(lanes):
        assert _same_point(c2, orc, 1, got[ln], orc.msm(1, bases, inf, sc[ln])), (c, ln)
    b.release()
    c2.close()


@pytest.mark.parametrize("g", [1, 2])
def test_msm_adversarial_equal_and_opposite_bases(ctx, czk, orc, g):
    """Worst case for the unsaturated accumulate kernels' exceptional-case hand-off: every base is +-P and the
    scalars collide, so almost every bucket addition is P + P or P + (-P) -- thousands of deferred points, the
    exception list overflows and whole buckets go to the saturated fix-up pass.  The result must still be the exact
    group element (the reference's add_assign_mixed handles these cases inline: short_weierstrass_jacobian.rs:587-597)."""
    n = 3000 if g == 1 else 1200
    _, one = _bases(ctx, g, 1, 99)
    neg = one[0].copy()
    half = one.shape[1] // 2
    if g == 1:
        neg[half:] = orc.fq_neg(one[0][half:])
    else:
        neg[half:] = np.concatenate([orc.fq_neg(one[0][half:half + 6]), orc.fq_neg(one[0][half + 6:])])
    bases = np.tile(one[0], (n, 1))
    bases[1::3] = neg
    sc = rand_fr_canonical(77, 8)
    scal = sc[np.arange(n) % 8].copy()          # only 8 distinct scalars -> heavy bucket collisions
    inf = np.zeros(n, dtype=np.uint8)
    b = ctx.register_bases(g, bases, inf)
    got = ctx.msm(b, scal, lanes=1)
    assert _same_point(ctx, orc, g, got[0], orc.msm(g, bases, inf, scal))
    b.release()


def test_spdz_open_with_mac_check(ctx, czk, orc):
    """czk_fr_spdz_open: the local arithmetic of SpdzFieldShare::batch_open (share/spdz.rs:166-185) with all parties'
    shares on the GPU; a corrupted MAC share must be counted."""
    import torch
    n, parties = 5000, 3
    secret = orc.fr_from_repr(rand_fr_canonical(61, n))
    sh = [orc.fr_from_repr(rand_fr_canonical(62 + p, n)) for p in range(parties - 1)]
    last = secret.copy()
    for s_ in sh:
        last = orc.fr_sub(last, s_)
    sh.append(last)
    lanes = np.stack([np.stack([s_, s_]) for s_ in sh])          # mac share = sh * mac(), mac() = 1 (spdz.rs:41-47)
    t = torch.from_numpy(lanes.view(np.int64).copy()).cuda()
    out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                                       # torch's stream is not the context's
    assert ctx.fr_spdz_open(t.data_ptr(), parties, n, out.data_ptr()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint64), secret)
    t[1, 1, 17, 0] += 1                                           # party 1 tampers with one MAC share
    torch.cuda.synchronize()
    assert ctx.fr_spdz_open(t.data_ptr(), parties, n, out.data_ptr()) == 1


def test_kzg10_commit_matches_reference_composition(ctx, czk, orc):
    """KZG10::commit (poly-commit/src/kzg10/mod.rs:141-193): MSM over powers_of_g, hiding MSM over powers_of_gamma_g,
    into_affine + add_assign_mixed -- composed from the C ABI exactly as include/czk.hpp's KZG10::commit does."""
    deg, hid = 700, 3
    _, pg = _bases(ctx, 1, deg + 1, 71)
    _, pgg = _bases(ctx, 1, hid + 2, 72)
    coeffs = orc.fr_from_repr(rand_fr_canonical(73, deg + 1))
    blind = orc.fr_from_repr(rand_fr_canonical(74, hid + 2))
    bg, bgg = ctx.register_bases(1, pg, None), ctx.register_bases(1, pgg, None)
    c = ctx.msm(bg, coeffs, scalar_form=czk.CZK_SCALAR_MONTGOMERY)[0]
    rc = ctx.msm(bgg, blind, scalar_form=czk.CZK_SCALAR_MONTGOMERY)[0]
    rc_aff, rc_inf = ctx.jac_to_affine(1, rc)
    got = ctx.jac_add_mixed(1, c, rc_aff[0], bool(rc_inf[0]))
    z = np.zeros(deg + 1, dtype=np.uint8)
    want_c = orc.multi_scalar_mul(1, pg, z, coeffs)
    want_r, want_rinf = orc.jac_to_affine(1, orc.multi_scalar_mul(1, pgg, z[: hid + 2], blind))
    want = orc.jac_add_mixed(1, want_c, want_r, want_rinf)
    assert _same_point(ctx, orc, 1, got, want)
    bg.release()
    bgg.release()


# ---- "next" rows: constraint evaluation and division by (X - z) -----------------------------------------------
def _random_csr_limbs(orc, seed, m, n_vars, max_terms=6):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, max_terms + 1, size=m)
    counts[3::7] = 0                                              # empty constraints
    row_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    nnz = int(row_ptr[-1])
    col = rng.integers(0, n_vars, size=nnz).astype(np.uint32)
    coeff = orc.fr_from_repr(rand_fr_canonical(seed + 1, nnz))
    one = orc.fr_from_repr(np.array([[1, 0, 0, 0]], dtype=np.uint64))[0]
    coeff[rng.random(nnz) < 0.5] = one                            # is_one() fast path (r1cs_to_qap.rs:28-32)
    return row_ptr, col, coeff


@pytest.mark.parametrize("m,n_vars,lanes", [(1, 1, 1), (1000, 300, 2), (70001, 50000, 4)])
def test_r1cs_matvec_matches_oracle(ctx, czk, orc, m, n_vars, lanes):
    row_ptr, col, coeff = _random_csr_limbs(orc, 90 + m, m, n_vars)
    z = orc.fr_from_repr(rand_fr_canonical(91 + m, lanes * n_vars)).reshape(lanes, n_vars, 4)
    mat = ctx.r1cs_matrix_register(row_ptr, col, coeff, n_vars)
    got = ctx.r1cs_matvec(mat, z, lanes=lanes)
    for ln in range(lanes):
        assert np.array_equal(got[ln], orc.r1cs_matvec(row_ptr, col, coeff, z[ln])), ln
    mat.release()


def test_r1cs_squaring_circuit_feeds_witness_map(ctx, czk, orc):
    """The matrices of the reference's benchmark circuit (proof.rs:304-344: w_{i+1} = w_i^2) evaluated on device lanes
    with padding stride D, then the device witness map; compared with the oracle run on the oracle's own matvec."""
    import torch
    log_d, N = 10, 1000
    D, n_vars = 1 << log_d, N + 2                                  # assignment = [1, out | w_0 .. w_{N-1}]
    one = orc.fr_from_repr(np.array([[1, 0, 0, 0]], dtype=np.uint64))
    w = [orc.fr_from_repr(rand_fr_canonical(5, 1))]
    for _ in range(N):
        w.append(orc.fr_mul(w[-1], w[-1]))
    z = np.concatenate([one, w[N]] + w[:N]).astype(np.uint64)     # instance (1, out) then witness
    ident = lambda cols: (np.arange(len(cols) + 1, dtype=np.uint64), np.array(cols, dtype=np.uint32), np.tile(one, (len(cols), 1)))
    A = ident([2 + i for i in range(N)] + [0, 1])                  # a_i = w_i, then the instance copy rows (:79-83)
    Bm = ident([2 + i for i in range(N)])
    Cm = ident([2 + i + 1 for i in range(N - 1)] + [1])            # c_i = w_{i+1}, last = out
    dev = {}
    zt = torch.from_numpy(z.view(np.int64).copy()).cuda()
    for name, (rp, col, cf) in (("a", A), ("b", Bm), ("c", Cm)):
        mat = ctx.r1cs_matrix_register(rp, col, cf, n_vars)
        out = torch.zeros((D, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()                                   # torch's stream is not the context's
        ctx.r1cs_matvec(mat, zt.data_ptr(), lanes=1, out=out.data_ptr(), z_stride=n_vars, out_stride=D, mem=czk.CZK_MEM_DEVICE)
        dev[name] = out
        ctx.sync()
        want = np.zeros((D, 4), dtype=np.uint64)
        want[: len(rp) - 1] = orc.r1cs_matvec(rp, col, cf, z)
        assert np.array_equal(out.cpu().numpy().view(np.uint64), want), name
        mat.release()
    a, b, c = (dev[k].cpu().numpy().view(np.uint64).copy() for k in "abc")
    ctx.witness_map_pre(dev["a"].data_ptr(), dev["b"].data_ptr(), log_d, 1)
    ctx.fr_vec_op(2, dev["a"].data_ptr(), dev["b"].data_ptr(), out=dev["a"].data_ptr(), n=D, mem=czk.CZK_MEM_DEVICE)
    ctx.witness_map_post(dev["a"].data_ptr(), dev["c"].data_ptr(), log_d, 1)
    ctx.sync()
    assert np.array_equal(dev["a"].cpu().numpy().view(np.uint64), orc.witness_map_plain(a, b, c, log_d))


def test_r1cs_matrix_rejects_malformed_input(ctx, czk, orc):
    one = orc.fr_from_repr(np.array([[1, 0, 0, 0]], dtype=np.uint64))
    good_rp = np.array([0, 1, 2], dtype=np.uint64)
    with pytest.raises(czk.CzkError):                              # index out of range: reference panics on assignment[index]
        ctx.r1cs_matrix_register(good_rp, np.array([0, 5], dtype=np.uint32), np.tile(one, (2, 1)), 5)
    with pytest.raises(czk.CzkError):                              # row_ptr not monotone
        ctx.r1cs_matrix_register(np.array([0, 2, 1, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint32), np.tile(one, (2, 1)), 5)
    mat = ctx.r1cs_matrix_register(good_rp, np.array([0, 4], dtype=np.uint32), np.tile(one, (2, 1)), 5)
    with pytest.raises(czk.CzkError):                              # assignment shorter than n_vars
        ctx.r1cs_matvec(mat, np.zeros((1, 4, 4), dtype=np.uint64), lanes=1)
    mat.release()


@pytest.mark.parametrize("log_d,in_len,stride", [(3, 8, 8), (6, 40, 50), (10, 1024, 1024), (11, 2000, 2048), (13, 5000, 5003), (16, 1 << 16, 1 << 16), (18, 200001, 262144 + 64),
                                                  (21, (1 << 20) + 2, (1 << 20) + 2)])
def test_ntt_out_of_place_equals_in_place(ctx, czk, orc, log_d, in_len, stride):
    """czk_ntt_fr_to (EvaluationDomain::fft(&coeffs) -> Vec, domain/mod.rs:72-76 and its three siblings): every kind, 3 lanes, a source whose lane
    stride differs from the domain size and whose tail beyond in_len is garbage -- bit-exact against czk_ntt_fr on a zero-extended copy (itself
    checked against the oracle), source untouched."""
    import torch
    lanes, D = 3, 1 << log_d
    src = torch.from_numpy(orc.fr_from_repr(rand_fr_canonical(900 + log_d, lanes * stride)).view(np.int64).copy()).reshape(lanes, stride, 4).cuda()
    src[:, in_len:] = 0x5A5A5A5A5A5A5A5A                              # garbage beyond in_len: must not be read
    keep = src.clone()
    for kind in (czk.CZK_FFT, czk.CZK_IFFT, czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT):
        ref = torch.zeros((lanes, D, 4), dtype=torch.int64, device="cuda")
        ref[:, :in_len] = src[:, :in_len]
        dst = torch.full((lanes, D, 4), 0x7777777777777777, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.ntt_fr(ref.data_ptr(), log_d, kind, lanes=lanes, in_len=in_len, mem=czk.CZK_MEM_DEVICE)
        ctx.ntt_fr_to(src.data_ptr(), stride, dst.data_ptr(), log_d, kind, lanes=lanes, in_len=in_len)
        ctx.sync()
        assert torch.equal(dst, ref), (log_d, kind)
        assert torch.equal(src, keep)
    if log_d <= 13:                                                   # and against the checker directly
        x = src[1, :in_len].cpu().numpy().view(np.uint64)
        dst = torch.empty((lanes, D, 4), dtype=torch.int64, device="cuda")
        ctx.ntt_fr_to(src.data_ptr(), stride, dst.data_ptr(), log_d, czk.CZK_COSET_FFT, lanes=lanes, in_len=in_len)
        ctx.sync()
        assert np.array_equal(dst[1].cpu().numpy().view(np.uint64), orc.ntt_fr(x, log_d, orc.COSET_FFT, in_len))


@pytest.mark.parametrize("n", [0, 1, 2, 31, 32, 33, 127, 129, 32 * 32 + 5, 32 * 32 * 32 + 7, (1 << 17) + 3])   # around the 32-coefficient segment levels
def test_poly_div_linear_matches_oracle(ctx, czk, orc, n):
    lanes = 2
    p = orc.fr_from_repr(rand_fr_canonical(300 + n, lanes * max(n, 1)))[: lanes * n].reshape(lanes, n, 4)
    if n > 4:
        p[1, n - 2:] = 0                                           # leading zeros: DensePolynomial truncates them
    z = orc.fr_from_repr(rand_fr_canonical(301, 1))[0]
    q, r = ctx.poly_div_linear(p, z, lanes=lanes)
    for ln in range(lanes):
        qw, rw = orc.poly_div_linear(p[ln], z)
        assert np.array_equal(q[ln], qw) and np.array_equal(r[ln], rw), (n, ln)
    # czk_poly_evaluate (DensePolynomial::evaluate, no quotient): the same values
    v = ctx.poly_evaluate(p, z, lanes=lanes)
    for ln in range(lanes):
        assert np.array_equal(v[ln], orc.fr_horner(p[ln], z) if n else np.zeros(4, dtype=np.uint64)), (n, ln)


@pytest.mark.parametrize("m,n", [(5, 5), (6, 5), (17, 4), (1000, 64), (7 * 4096 + 3, 4096), (3 * (1 << 14) - 1, 1 << 14), (2 * 768, 768), ((1 << 18) + 5, 3 << 12)])
def test_poly_div_vanishing_matches_checker_and_definition(ctx, czk, orc, m, n):
    """czk_poly_div_vanishing (DensePolynomial::divide_by_vanishing_poly, dense.rs:172-179, for X^n - 1): against the suffix sums of the n-coefficient chunks
    computed with the checker's field addition, and against the definition a = q X^n - q + r, deg r < n, which determines (q, r) uniquely --
    incl. ragged lengths (m not a multiple of n), m == n (empty quotient) and a mixed-radix size."""
    lanes = 2
    a = orc.fr_from_repr(rand_fr_canonical(900 + m + n, lanes * m)).reshape(lanes, m, 4)
    q, r = ctx.poly_div_vanishing(a, n, lanes=lanes)
    assert q.shape == (lanes, m - n, 4) and r.shape == (lanes, n, 4)
    chunks = -(-m // n)
    for ln in range(lanes):
        pad = np.zeros((chunks * n, 4), dtype=np.uint64)
        pad[:m] = a[ln]
        suffix = np.zeros((n, 4), dtype=np.uint64)
        want_q = np.zeros((chunks * n, 4), dtype=np.uint64)
        for k in range(chunks - 1, 0, -1):
            suffix = orc.fr_add(suffix, pad[k * n:(k + 1) * n])
            want_q[(k - 1) * n:k * n] = suffix
        assert np.array_equal(q[ln], want_q[:m - n]) and np.array_equal(r[ln], orc.fr_add(suffix, pad[:n])), (m, n, ln)
        # the definition: a_j = q_(j - n) - q_j + r_j
        qx = np.zeros((m + n, 4), dtype=np.uint64)
        qx[:m - n] = q[ln]
        shifted = np.zeros((m + n, 4), dtype=np.uint64)
        shifted[n:m] = q[ln]
        rr = np.zeros((m + n, 4), dtype=np.uint64)
        rr[:n] = r[ln]
        back = orc.fr_add(orc.fr_sub(shifted, qx), rr)
        assert np.array_equal(back[:m], a[ln]) and not back[m:].any(), (m, n, ln)


def test_poly_evaluate_many_matches_checker(ctx, czk, orc):
    """czk_poly_evaluate_many: 21 polynomials of ragged lengths (around the 32-coefficient segment levels, the zero polynomial, one coefficient), 1 / 2 / 4
    lanes, each at its own point, in one call (two batches of the kernel's 16 descriptors) -- every value against the checker's Horner evaluation, and against
    czk_poly_evaluate."""
    import torch
    sizes = [0, 1, 2, 31, 32, 33, 1023, 1024, 1025, 32 * 32 * 32, 32 * 32 * 32 + 1, (1 << 16) + 5, 7, 100, 5000, 40000, 3, 64, 65, 2049, 12345]
    lanes = [1, 2, 4, 1, 2, 4, 1, 2, 4, 1, 2, 4, 3, 3, 1, 2, 4, 1, 2, 4, 2]
    polys, zs = [], []
    for k, (n, ln) in enumerate(zip(sizes, lanes)):
        polys.append(orc.fr_from_repr(rand_fr_canonical(700 + k, ln * max(n, 1)))[: ln * n].reshape(ln, n, 4))
        zs.append(orc.fr_from_repr(rand_fr_canonical(750 + k, 1))[0])
    dev = [torch.from_numpy(p.view(np.int64).copy()).cuda() for p in polys]
    vals = torch.full((sum(lanes), 4), -1, dtype=torch.int64, device="cuda")
    at, outs = 0, []
    for ln in lanes:
        outs.append(vals[at:at + ln])
        at += ln
    torch.cuda.synchronize()
    ctx.poly_evaluate_many([d.data_ptr() for d in dev], sizes, lanes, zs, [o.data_ptr() for o in outs])
    ctx.sync()
    got = vals.cpu().numpy().view(np.uint64)
    at = 0
    for k, (n, ln) in enumerate(zip(sizes, lanes)):
        for l in range(ln):
            want = orc.fr_horner(polys[k][l], zs[k]) if n else np.zeros(4, dtype=np.uint64)
            assert np.array_equal(got[at + l], want), (k, n, l)
        if n:
            assert np.array_equal(got[at:at + ln], ctx.poly_evaluate(polys[k], zs[k], lanes=ln)), k
        at += ln


def test_fr_lincomb_matches_checker(ctx, czk, orc):
    """czk_fr_lincomb: shared (4-lane) and public (1-lane) terms of ragged lengths, a unit coefficient, a term longer than the result; public terms must land
    on the lanes of the lift mask only (AdditiveFieldShare::shift: the king's lanes) -- against the same sum built from the checker's field operations."""
    import torch
    lanes, out_len, mask = 4, 5000, 0b0011
    spec = [(4, 5000), (1, 4097), (4, 1), (1, 5000), (4, 6000), (4, 4999), (1, 0), (4, 3000)]      # (lanes, length)
    one = orc.fr_from_repr(np.array([[1, 0, 0, 0]], dtype=np.uint64))[0]
    terms = [orc.fr_from_repr(rand_fr_canonical(800 + k, ln * max(n, 1)))[: ln * n].reshape(ln, n, 4) for k, (ln, n) in enumerate(spec)]
    coeffs = [orc.fr_from_repr(rand_fr_canonical(850 + k, 1))[0] for k in range(len(spec))]
    coeffs[2] = one
    dev = [torch.from_numpy(t.view(np.int64).copy()).cuda() for t in terms]
    out = torch.full((lanes, out_len, 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    cst = orc.fr_from_repr(rand_fr_canonical(899, 1))[0]
    ctx.fr_lincomb([d.data_ptr() for d in dev], [n for _, n in spec], [ln for ln, _ in spec], coeffs, lanes, mask, out.data_ptr(), out_len, constant=cst)
    ctx.sync()
    got = out.cpu().numpy().view(np.uint64)
    for l in range(lanes):
        want = np.tile(cst, (out_len, 1)) if (mask >> l) & 1 else np.zeros((out_len, 4), dtype=np.uint64)   # the constant is public: lifting lanes only
        for (ln, n), t, c in zip(spec, terms, coeffs):
            if ln == 1 and not (mask >> l) & 1:
                continue
            m = min(n, out_len)
            if m:
                want[:m] = orc.fr_add(want[:m], orc.fr_mul(t[l if ln > 1 else 0][:m], np.tile(c, (m, 1))))
        assert np.array_equal(got[l], want), l
    # a public result takes every public term whatever the mask; more than 12 terms is an error, not a truncation
    out1 = torch.full((1, 4097, 4), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.fr_lincomb([dev[1].data_ptr(), dev[3].data_ptr()], [4097, 5000], [1, 1], [coeffs[1], coeffs[3]], 1, 0, out1.data_ptr(), 4097)
    ctx.sync()
    want1 = orc.fr_add(orc.fr_mul(terms[1][0], np.tile(coeffs[1], (4097, 1))), orc.fr_mul(terms[3][0][:4097], np.tile(coeffs[3], (4097, 1))))
    assert np.array_equal(out1.cpu().numpy().view(np.uint64)[0], want1)
    with pytest.raises(czk.CzkError):
        ctx.fr_lincomb([dev[0].data_ptr()] * 13, [5000] * 13, [4] * 13, [one] * 13, lanes, mask, out.data_ptr(), out_len)


def test_poly_div_linear_full_size_identity(ctx, czk, orc):
    """2^21 coefficients x 2 lanes on device: remainder == p(z) (oracle Horner) and p(x) == q(x) (x - z) + r at a random x."""
    import torch
    n, lanes = 1 << 21, 2
    p = orc.fr_from_repr(rand_fr_canonical(310, 4096))
    pt = torch.from_numpy(p.view(np.int64).copy()).cuda().repeat(lanes * n // 4096, 1).contiguous()
    pt[n + 7, 0] += 1                                              # make the two lanes differ
    z = orc.fr_from_repr(rand_fr_canonical(311, 1))[0]
    x = orc.fr_from_repr(rand_fr_canonical(312, 1))[0]
    q = torch.zeros((lanes, n - 1, 4), dtype=torch.int64, device="cuda")
    r = torch.zeros((lanes, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()                                       # torch's stream is not the context's
    ctx.poly_div_linear(pt.data_ptr(), z, lanes=lanes, n=n, quotient=q.data_ptr(), remainder=r.data_ptr(), mem=czk.CZK_MEM_DEVICE)
    ctx.sync()
    ph, qh, rh = pt.cpu().numpy().view(np.uint64).reshape(lanes, n, 4), q.cpu().numpy().view(np.uint64), r.cpu().numpy().view(np.uint64)
    v = torch.zeros((lanes, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ctx.poly_evaluate(pt.data_ptr(), z, lanes=lanes, n=n, values=v.data_ptr(), mem=czk.CZK_MEM_DEVICE)
    ctx.sync()
    assert np.array_equal(v.cpu().numpy().view(np.uint64), rh)     # evaluation without the quotient: the remainder, bit for bit
    for ln in range(lanes):
        assert np.array_equal(rh[ln], orc.fr_horner(ph[ln], z))
        lhs = orc.fr_horner(ph[ln], x)
        rhs = orc.fr_add(orc.fr_mul(orc.fr_horner(qh[ln], x), orc.fr_sub(x, z)), rh[ln])
        assert np.array_equal(lhs, rhs)


@pytest.mark.parametrize("parties,size", [(2, ["--log-n", "12"]), (3, ["--log-n", "10"]), (8, ["--constraints", "100"])])
def test_party_per_rank_layout_matches_single_gpu_layout(parties, size):
    """bench.py --layout party (one MPC party per rank; the witness map's two opens are all-gathers + the fused
    open/MAC-check kernel) must produce the same proof elements as the default layout with all parties on one GPU
    (BASELINE configs[4] shape at 8 parties).  bench.py --gpus N launches the N ranks itself; they share this box's
    single GPU, so the exchange runs over gloo (RCCL needs one device per rank)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = size + ["--parties", str(parties), "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-seam-report"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common, capture_output=True, text=True, timeout=280, env=env, cwd=root)
    assert one.returncode == 0, __import__('util').child_errors(one.stderr)
    two = __import__('util').run_ranks([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(parties), "--layout", "party", "--backend", "gloo",
                          "--device", "0"] + common, capture_output=True, text=True, timeout=280, env=env, cwd=root)
    assert two.returncode == 0, __import__('util').child_errors(two.stderr)
    d1 = json.loads(one.stdout.strip().splitlines()[-1])
    d2 = json.loads(two.stdout.strip().splitlines()[-1])
    assert d2["n_gpus"] == parties and d2["ranks_seen_by_backend"] == parties and d2["config"]["layout"] == "party"
    assert d1["results_checked"] and d2["results_checked"]
    assert d1["config"]["results_sha256"] == d2["config"]["results_sha256"]


@pytest.mark.parametrize("scheme,parties,net", [("gsz", 3, "torch"), ("gsz", 4, "czk"), ("hbc", 3, "czk-ipc")])
def test_party_layout_under_the_other_sharings(scheme, parties, net):
    """bench.py --layout party for the reference's other sharings: HBC (AdditiveFieldShare::batch_open between the ranks) and GSZ (one Shamir lane per
    rank; the product's degree reduction is gsz20::batch_king_compute -- every rank's lane to the king, open at degree 2t, the value back to everyone),
    over torch.distributed and over the library's communicator (czk_net, shared memory: the ranks share this box's GPU).  Same proof elements as the
    layout with all parties' lanes on one GPU."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--constraints", "1000", "--parties", str(parties), "--scheme", scheme, "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-seam-report",
              "--no-other-workloads"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common, capture_output=True, text=True, timeout=280, env=env, cwd=root)
    assert one.returncode == 0, __import__('util').child_errors(one.stderr)
    many = __import__('util').run_ranks([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(parties), "--layout", "party", "--backend", "gloo", "--device", "0", "--net", net]
                          + common, capture_output=True, text=True, timeout=280, env=env, cwd=root)
    assert many.returncode == 0, __import__('util').child_errors(many.stderr)
    d1 = json.loads(one.stdout.strip().splitlines()[-1])
    d2 = json.loads(many.stdout.strip().splitlines()[-1])
    assert d2["n_gpus"] == parties and d2["config"]["layout"] == "party" and d2["net"] == {"czk": "czk_net shm", "czk-ipc": "czk_net ipc", "torch": "torch.distributed"}[net]
    assert d1["results_checked"] and d2["results_checked"]
    assert d1["config"]["results_sha256"] == d2["config"]["results_sha256"]


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 1029, 32 * 32 * 32 + 7, (1 << 18) + 1])
def test_fr_prefix_product_matches_oracle(ctx, czk, orc, n):
    """czk_fr_prefix_product vs the sequential loop of partial_products (share/field.rs:169-172)."""
    x = orc.fr_from_repr(rand_fr_canonical(400 + n, max(n, 1)))[:n]
    if n > 40:
        x[37] = orc.fr_from_repr(np.array([[1, 0, 0, 0]], dtype=np.uint64))[0]
    got = ctx.fr_prefix_product(x)
    assert np.array_equal(got, orc.fr_prefix_product(x))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, (1 << 17) + 5])
def test_fr_batch_inverse_matches_oracle(ctx, czk, orc, n):
    """czk_fr_batch_inverse vs serial_batch_inversion_and_mul (fields/mod.rs:642-677), zeros included."""
    v = orc.fr_from_repr(rand_fr_canonical(500 + n, max(n, 1)))[:n]
    if n > 70:
        v[[0, 5, 63, 64, 69]] = 0
        v[128:192] = 0                                             # an all-zero segment
    coeff = orc.fr_from_repr(rand_fr_canonical(501, 1))[0]
    assert np.array_equal(ctx.fr_batch_inverse(v, coeff), orc.fr_batch_inverse(v, coeff))
    one = orc.fr_from_repr(np.array([[1, 0, 0, 0]], dtype=np.uint64))[0]
    assert np.array_equal(ctx.fr_batch_inverse(v), orc.fr_batch_inverse(v, one))


def test_poly_and_scan_entry_points_reject_bad_arguments(ctx, czk, orc):
    import ctypes as C
    import torch
    L = czk.lib()
    h = ctx._h
    ERR_ARG, OK = 3, 0                                             # include/czk.h: CZK_ERR_ARG, CZK_OK
    one = orc.fr_from_repr(np.array([[1, 0, 0, 0]], dtype=np.uint64))
    buf = torch.zeros((8, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p = C.c_void_p(buf.data_ptr())
    null = C.c_void_p(0)
    z = one.ctypes.data_as(C.c_void_p)
    assert L.czk_poly_div_linear(h, p, C.c_size_t(8), C.c_size_t(1), null, p, null, C.c_int(czk.CZK_MEM_DEVICE)) == ERR_ARG      # no point
    assert L.czk_poly_div_linear(h, null, C.c_size_t(8), C.c_size_t(1), z, p, null, C.c_int(czk.CZK_MEM_DEVICE)) == ERR_ARG   # no coefficients
    assert L.czk_poly_evaluate(h, p, C.c_size_t(8), C.c_size_t(1), null, p, C.c_int(czk.CZK_MEM_DEVICE)) == ERR_ARG           # no point
    assert L.czk_poly_evaluate(h, p, C.c_size_t(8), C.c_size_t(1), z, null, C.c_int(czk.CZK_MEM_DEVICE)) == ERR_ARG           # no destination
    assert L.czk_poly_evaluate(h, null, C.c_size_t(8), C.c_size_t(1), z, p, C.c_int(czk.CZK_MEM_DEVICE)) == ERR_ARG        # no coefficients
    assert L.czk_fr_batch_inverse(h, p, C.c_size_t(8), null, p, C.c_int(czk.CZK_MEM_DEVICE)) == ERR_ARG                        # in-place on device
    assert L.czk_fr_prefix_product(h, null, C.c_size_t(8), p, C.c_int(czk.CZK_MEM_DEVICE)) == ERR_ARG
    assert L.czk_fr_prefix_product(h, null, C.c_size_t(0), null, C.c_int(czk.CZK_MEM_DEVICE)) == OK                            # empty vector
    assert L.czk_r1cs_matvec(h, null, p, C.c_size_t(8), C.c_size_t(1), p, C.c_size_t(8), C.c_int(czk.CZK_MEM_DEVICE)) == ERR_ARG   # no matrix


@pytest.mark.parametrize("g,n", [(1, 70000), (2, 9000), (1, (1 << 21) - 1)])
def test_msm_over_full_buckets(ctx, czk, orc, g, n):
    """Skewed scalars as boolean-heavy witnesses produce them: most scalars are 1 (one bucket of window 0 receives tens of
    thousands of points), some are r - 1 (the negated digit), a few are random.  The over-full bucket is folded in
    2048-entry chunks by k_accumulate_heavy / k_heavy_combine instead of one thread walking all of it; the reference
    special-cases scalar == 1 (variable_base.rs:44-48).  Checked against [sum k_i s_i] G.  (The partition that holds the full bucket
    exceeds k_part_sort's LDS staging area: the direct placement path; at 2^21 - 1 points with the h query's 1024 smaller partitions.)"""
    import time
    k = rand_fr_canonical(600 + g, n)
    bases = ctx.fixed_base_points(g, k)
    s = np.zeros((2, n, 4), dtype=np.uint64)
    s[:, :, 0] = 1                                                 # scalar 1 everywhere
    rm1 = ints_to_limbs([R_MOD - 1], 4)[0]
    s[0, ::7] = rm1                                                # lane 0: every 7th scalar is -1
    s[1, ::5] = rand_fr_canonical(601, len(s[1, ::5]))             # lane 1: every 5th is random
    s[1, 3] = 0
    b = ctx.register_bases(g, bases, None)
    t0 = time.perf_counter()
    out = ctx.msm(b, s, lanes=2)
    dt = time.perf_counter() - t0
    gen = ctx.fixed_base_points(g, ints_to_limbs([1], 4))[0]
    for ln in range(2):
        e = dot_mod_r(k, s[ln])
        assert _same_point(ctx, orc, g, out[ln], orc.scalar_mul(g, gen, False, ints_to_limbs([e], 4)[0])), (g, ln)
    assert dt < 1.0, f"over-full bucket path took {dt:.2f} s"    # one thread per bucket would need seconds here
    b.release()


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 8, 10, 11, 13, 16])
def test_mixed_radix_ntt_all_kinds_bit_exact(ctx, czk, orc, k):
    """MixedRadixEvaluationDomain (size 3 * 2^k) transforms against the checker's restatement of serial_mixed_radix_fft
    (mixed_radix.rs:286-404): every output limb, all four kinds, 2 lanes, ragged prefix with a garbage tail."""
    size = 3 << k
    kc = ctx.mixed_domain_constants(size)
    assert np.array_equal(kc["group_gen"], orc.fr_root_of_unity_mixed(size))
    for in_len in sorted({size, max(1, size - 5), (size + 1) // 2}):
        lanes = 2
        x = orc.fr_from_repr(rand_fr_canonical(300 + k, lanes * in_len)).reshape(lanes, in_len, 4)
        for kind in (czk.CZK_FFT, czk.CZK_IFFT, czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT):
            buf = np.full((lanes, size, 4), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
            buf[:, :in_len] = x
            ctx.ntt_fr_mixed(buf, size, kind, lanes=lanes, in_len=in_len)
            for ln in range(lanes):
                assert np.array_equal(buf[ln], orc.ntt_fr_mixed(x[ln], size, kind, in_len)), (k, in_len, kind, ln)


def test_mixed_radix_ntt_plonk_wire_domain_and_errors(ctx, czk, orc):
    """The wire domain of BASELINE configs[2] (Plonk, 2^18 gates: 3 * 2^18 points), one GSZ lane, device memory: bit-exact
    against the checker for the forward transforms, exact round trips; sizes without a domain are refused."""
    import torch
    import czk_amd
    size = 3 << 18
    x = orc.fr_from_repr(rand_fr_canonical(31337, size))
    for fwd, inv in ((czk.CZK_FFT, czk.CZK_IFFT), (czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT)):
        t = torch.from_numpy(x.view(np.int64)).cuda()
        ctx.ntt_fr_mixed(t.data_ptr(), size, fwd, mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        assert np.array_equal(t.cpu().numpy().view(np.uint64), orc.ntt_fr_mixed(x, size, fwd))
        ctx.ntt_fr_mixed(t.data_ptr(), size, inv, mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        assert np.array_equal(t.cpu().numpy().view(np.uint64), x)
    for bad in (5, 9, 3 * 5, 3 * 3 * 4):
        with pytest.raises(czk_amd.CzkError) as e:
            ctx.ntt_fr_mixed(np.zeros((bad, 4), dtype=np.uint64), bad, czk.CZK_FFT)
        assert e.value.code == 1
    # a power-of-two size is the radix-2 domain
    y = orc.fr_from_repr(rand_fr_canonical(5, 64))
    buf = y.copy()
    ctx.ntt_fr_mixed(buf, 64, czk.CZK_COSET_FFT)
    assert np.array_equal(buf, orc.ntt_fr(y, 6, orc.COSET_FFT))


@pytest.mark.parametrize("rounds", [1, 3])
def test_msm_batched_affine_rounds_still_match(czk, orc, rounds):
    """LAB library: the batched-affine pre-reduction of the bucket lists (csrc/lab/msm_aff.h, option "msm_affine_rounds" = R; measured slower
    than the XYZZ kernel and therefore not in the product -- profiles/r02_affine_prototype.json) computes the same group elements: checker's
    Pippenger at n = 4096 with zero / unit scalars and infinity bases, equal and opposite points in one bucket, 4 lanes."""
    c = czk.Context(0, lab=True, options={"msm_affine_rounds": rounds})
    n = 4096
    k = rand_fr_canonical(77, n)
    bases = c.fixed_base_points(1, k)
    bases[10] = bases[11]                                   # equal points meeting in one bucket (same scalar below)
    bases[20, 6:] = orc.fq_neg(bases[21, 6:].reshape(1, 6))[0]   # -P next to P
    bases[20, :6] = bases[21, :6]
    inf = np.zeros(n, dtype=np.uint8)
    inf[5] = 1
    s = rand_fr_canonical(78, 4 * n).reshape(4, n, 4)
    s[:, 11] = s[:, 10]
    s[:, 21] = s[:, 20]
    s[0, 7] = 0
    s[1, 8] = (1, 0, 0, 0)
    b = c.register_bases(1, bases, inf)
    out = c.msm(b, s, lanes=4)
    for ln in range(4):
        assert _same_point(c, orc, 1, out[ln], orc.msm(1, bases, inf, s[ln])), (rounds, ln)
    b.release()
    c.close()


def test_ntt_first_generation_passes_still_match(czk, orc):
    """The option "ntt_gen1" keeps the first-generation passes (ntt.hip) for every size -- the A/B switch behind the figures in
    profiles/r02_pmc_ntt.json; they serve the domains below 2^11 by default.  Bit-exact at sizes that exercise their 6- and
    7-stage tiles (2^13, 2^14) and all four kinds."""
    c = czk.Context(0, options={"ntt_gen1": 1})
    for log_d in (13, 14):
        d = 1 << log_d
        x = orc.fr_from_repr(rand_fr_canonical(900 + log_d, 2 * d)).reshape(2, d, 4)
        for kind in (czk.CZK_FFT, czk.CZK_IFFT, czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT):
            buf = x.copy()
            c.ntt_fr(buf, log_d, kind, lanes=2)
            for ln in range(2):
                assert np.array_equal(buf[ln], orc.ntt_fr(x[ln], log_d, kind)), (log_d, kind, ln)
    c.close()


@pytest.mark.parametrize("g,n", [(1, 1), (1, 7), (1, 33), (1, 300), (1, 4096), (1, 70001), (2, 1), (2, 33), (2, 700)])
def test_msm_without_window_tables_matches_reference_pippenger(ctx, czk, orc, g, n):
    """CZK_MEM_NO_TABLES: the points are registered as they are and every window runs as its own bucket set (the windows are
    extra lanes of the same kernels), then sum_w 2^(c w) R_w like the reference's final loop (variable_base.rs:92-105).  Same
    special cases as the table form: zero / unit scalars, infinity bases, equal and opposite points, both scalar forms,
    fewer scalars than bases; two lanes."""
    _, bases = _bases(ctx, g, n, 900 + n)
    inf = np.zeros(n, dtype=np.uint8)
    sc = rand_fr_canonical(901 + n, 2 * n).reshape(2, n, 4)
    if n >= 10:
        bases[3] = bases[2]
        aw = bases.shape[1] // 2
        neg = bases[4].copy()
        if g == 1:
            neg[aw:] = orc.fq_neg(bases[4][aw:])
        else:
            neg[aw:] = np.concatenate([orc.fq_neg(bases[4][aw:aw + 6]), orc.fq_neg(bases[4][aw + 6:])])
        bases[5] = neg
        inf[7] = 1
        sc[:, 0] = 0
        sc[:, 1] = ints_to_limbs([1], 4)[0]
        sc[:, 2] = sc[:, 3] = ints_to_limbs([5], 4)[0]
        sc[:, 4] = sc[:, 5] = ints_to_limbs([R_MOD - 3], 4)[0]
        sc[1, 8] = ints_to_limbs([R_MOD - 1], 4)[0]                     # every signed digit carries
    b = ctx.register_bases(g, bases, inf, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_NO_TABLES)
    assert len(b) == n
    got = ctx.msm(b, sc, lanes=2)
    for ln in range(2):
        assert _same_point(ctx, orc, g, got[ln], orc.msm(g, bases, inf, sc[ln])), (g, n, ln)
    scm = orc.fr_from_repr(np.vstack([sc[0], ints_to_limbs([77], 4)]))
    got_m = ctx.msm(b, scm, lanes=1, scalar_form=czk.CZK_SCALAR_MONTGOMERY)
    assert _same_point(ctx, orc, g, got_m[0], orc.multi_scalar_mul(g, bases, inf, scm))
    if n > 2:
        got_s = ctx.msm(b, sc[0, : n - 1], lanes=1)
        assert _same_point(ctx, orc, g, got_s[0], orc.msm(g, bases[: n - 1], inf[: n - 1], sc[0, : n - 1]))
    # the same handle through the asynchronous entry point, two MSMs in flight
    import torch
    sd = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()
    o1, o2 = np.zeros((2, 18 * g), dtype=np.uint64), np.zeros((1, 18 * g), dtype=np.uint64)
    torch.cuda.synchronize()
    ctx.msm_async(b, sd.data_ptr(), n, 2, czk.CZK_SCALAR_CANONICAL, o1)
    ctx.msm_async(b, sd[1].data_ptr(), n, 1, czk.CZK_SCALAR_CANONICAL, o2)
    ctx.sync()
    assert _same_point(ctx, orc, g, o1[1], orc.msm(g, bases, inf, sc[1])) and _same_point(ctx, orc, g, o2[0], orc.msm(g, bases, inf, sc[1]))
    b.release()


@pytest.mark.parametrize("g,n", [(1, (1 << 20) + 1), (2, (1 << 18) + 1)])
def test_msm_without_window_tables_full_size(ctx, czk, orc, g, n):
    """The a-query size of BASELINE configs[1] without window tables, 4 share lanes, by known discrete logs and against the
    table form of the same bases."""
    import torch
    lanes = 4
    k = rand_fr_canonical(0xBA5E5 + 9, n)
    aw = 12 if g == 1 else 24
    kd = torch.from_numpy(k.view(np.int64)).cuda()
    pts = torch.empty((n, aw), dtype=torch.int64, device="cuda")
    ctx.fixed_base_points(g, kd.data_ptr(), out=pts.data_ptr(), n=n, mem=czk.CZK_MEM_DEVICE)
    b = ctx.register_bases(g, pts.data_ptr(), None, n=n, mem=czk.CZK_MEM_DEVICE | czk.CZK_MEM_NO_TABLES)
    bt = ctx.register_bases(g, pts.data_ptr(), None, n=n, mem=czk.CZK_MEM_DEVICE)
    del pts
    s = rand_fr_canonical(0xC0FFEE + 9, lanes * n).reshape(lanes, n, 4)
    s[3, : n // 2] = ints_to_limbs([1], 4)[0]                            # half of one lane's scalars are 1: over-full buckets in window 0
    sd = torch.from_numpy(s.view(np.int64)).cuda()
    out = ctx.msm(b, sd.data_ptr(), n_scalars=n, lanes=lanes, mem=czk.CZK_MEM_DEVICE)
    out_t = ctx.msm(bt, sd.data_ptr(), n_scalars=n, lanes=lanes, mem=czk.CZK_MEM_DEVICE)
    gen = ctx.fixed_base_points(g, ints_to_limbs([1], 4))[0]
    for ln in range(lanes):
        e = dot_mod_r(k, s[ln])
        assert _same_point(ctx, orc, g, out[ln], orc.scalar_mul(g, gen, False, ints_to_limbs([e], 4)[0])), (g, ln)
        assert _same_point(ctx, orc, g, out[ln], out_t[ln])
    b.release()
    bt.release()


def test_many_share_lanes(ctx, czk, orc):
    """8 SPDZ parties on one GPU are 16 share lanes (lanes ride on gridDim.y of every kernel): NTT with 7 and 16 lanes incl. an
    all-zero and a one-element input, G1 MSM with 16 lanes, G2 with 6."""
    for log_d, lanes in ((12, 7), (11, 16)):
        d = 1 << log_d
        x = orc.fr_from_repr(rand_fr_canonical(7700 + log_d, lanes * d)).reshape(lanes, d, 4)
        for kind in (czk.CZK_FFT, czk.CZK_IFFT, czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT):
            buf = x.copy()
            ctx.ntt_fr(buf, log_d, kind, lanes=lanes)
            for ln in range(lanes):
                assert np.array_equal(buf[ln], orc.ntt_fr(x[ln], log_d, kind, d)), (log_d, kind, ln)
            for in_len in (0, 1):
                buf = np.full((2, d, 4), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
                buf[:, :in_len] = x[:2, :in_len]
                ctx.ntt_fr(buf, log_d, kind, lanes=2, in_len=in_len)
                for ln in range(2):
                    assert np.array_equal(buf[ln], orc.ntt_fr(x[ln, :in_len], log_d, kind, in_len)), (log_d, kind, in_len)
    for g, n, lanes in ((1, 5000, 16), (2, 300, 6)):
        _, bases = _bases(ctx, g, n, 8800 + n)
        sc = rand_fr_canonical(8801 + n, lanes * n).reshape(lanes, n, 4)
        for no_tables in (0, czk.CZK_MEM_NO_TABLES):
            b = ctx.register_bases(g, bases, None, mem=czk.CZK_MEM_HOST | no_tables)
            got = ctx.msm(b, sc, lanes=lanes)
            for ln in range(lanes):
                assert _same_point(ctx, orc, g, got[ln], orc.msm(g, bases, np.zeros(n, dtype=np.uint8), sc[ln])), (g, ln, no_tables)
            b.release()


@pytest.mark.parametrize("log_d,lanes", [(12, 3), (14, 2), (15, 1), (18, 4), (21, 4), (13, 2), (16, 2)])
def test_witness_map_fused_ifft_coset_fft_pass(czk, orc, log_d, lanes):
    """czk_witness_map_pre / _post run `coset_fft(ifft(x))` with the inverse transform's last pass and the forward transform's first pass as ONE kernel where
    their tiles line up (2^12, 2^14, 2^15, 2^18, 2^21: the stage bits split into equal groups).  Bit for bit the two-transform form: against the library
    with the option off for every size (incl. 2^13 and 2^16, which do not fuse, and zero-extended inputs), and against the checker's ifft + coset_fft up to 2^15."""
    import torch
    d = 1 << log_d
    a_len, b_len = d - 5, (3 * d) // 4
    x = orc.fr_from_repr(rand_fr_canonical(5100 + log_d, 4096))
    src = torch.from_numpy(x.view(np.int64).copy()).cuda().repeat((3 * lanes * d) // 4096 + 1, 1)[: 3 * lanes * d].contiguous().view(3, lanes, d, 4)
    src[:, :, 17, 0] += torch.arange(3 * lanes, device="cuda", dtype=torch.int64).view(3, lanes) + 1      # lanes differ
    outs = []
    for fuse in (1, 0):
        c = czk.Context(0, options={"ntt_fuse_pairs": fuse})
        a, b, cc = (src[i].clone() for i in range(3))
        ab = src[0].clone()
        torch.cuda.synchronize()
        c.witness_map_pre(a.data_ptr(), b.data_ptr(), log_d, lanes, a_len=a_len, b_len=b_len)
        c.witness_map_post(ab.data_ptr(), cc.data_ptr(), log_d, lanes, c_len=a_len)
        c.sync()
        outs.append([t.cpu().numpy().view(np.uint64) for t in (a, b, cc, ab)])
        c.close()
    for got, want in zip(*outs):
        assert np.array_equal(got, want)
    if log_d <= 15:
        h = src.cpu().numpy().view(np.uint64)
        for ln in range(lanes):
            for got, raw, n_in in ((outs[0][0], h[0], a_len), (outs[0][1], h[1], b_len), (outs[0][2], h[2], a_len)):
                coeffs = orc.ntt_fr(raw[ln][:n_in], log_d, orc.IFFT, n_in)
                assert np.array_equal(got[ln], orc.ntt_fr(coeffs, log_d, orc.COSET_FFT, d)), (log_d, ln)


@pytest.mark.parametrize("interleave", [0, 1, 2, 3, 4, 8])
def test_msm_lane_interleave_matches_checker(czk, orc, interleave):
    """czk_ctx_set_option "msm_lane_interleave": the accumulate kernels' threads take the same bucket rank of G neighbouring lanes.  Every group size
    (0 = the library's rule) against the checker's Pippenger for lane counts that leave a short last group (1, 3, 5, 7 lanes), G1 and G2, with
    over-full buckets (a third of the scalars equal to one) and on the table-free path, whose lanes are windows."""
    c = czk.Context(0, options={"msm_lane_interleave": interleave})
    for g, n in ((1, 3000), (2, 400)):
        _, bases = _bases(c, g, n, 9900 + n)
        for lanes in (1, 3, 5, 7):
            sc = rand_fr_canonical(9901 + n + lanes, lanes * n).reshape(lanes, n, 4)
            sc[:, ::3] = np.array([1, 0, 0, 0], dtype=np.uint64)
            want = [orc.msm(g, bases, np.zeros(n, dtype=np.uint8), sc[ln]) for ln in range(lanes)]
            for no_tables in (0, czk.CZK_MEM_NO_TABLES):
                b = c.register_bases(g, bases, None, mem=czk.CZK_MEM_HOST | no_tables)
                got = c.msm(b, sc, lanes=lanes)
                for ln in range(lanes):
                    assert _same_point(c, orc, g, got[ln], want[ln]), (interleave, g, lanes, ln, no_tables)
                b.release()
    c.close()


@pytest.mark.parametrize("n", [3000, 70000])
def test_msm_same_scalars_shares_the_digit_sort(czk, orc, n):
    """CZK_MEM_SAME_SCALARS: MSMs of one scalar vector against several keys (create_proof's a, b_g1, b_g2 all take `assignment`, groth16/src/prover.rs:
    130-166) keep ONE digit sort where the keys' layouts and points at infinity agree.  Counted through the profiling brackets ("msm_sort" / "msm_sort_reused"),
    results against the checker either way; a key with other points at infinity, a call after czk_ctx_sync, a call without the flag and the option
    "msm_sort_reuse" = 0 all sort for themselves -- and so does the next group (the next proof's calls over the same buffer)."""
    import torch
    lanes = 3
    c = czk.Context(0, options={"msm_sort_reuse": 1})       # (off by default: EXPERIMENTS.md section 14)
    c.profile_enable(True)
    inf_b = np.zeros(n, dtype=np.uint8)
    inf_b[[0, n // 2]] = 1
    inf_0 = np.zeros(n, dtype=np.uint8)
    keys = {}
    for name, g, inf, seed in (("b_g2", 2, inf_b, 1), ("a", 1, inf_0, 2), ("b_g1", 1, inf_b, 3), ("x", 1, inf_b, 4)):
        _, pts = _bases(c, g, n, 7700 + seed)
        keys[name] = (g, pts, inf, c.register_bases(g, pts, inf, mem=czk.CZK_MEM_HOST))
    sc = rand_fr_canonical(7710 + n, lanes * n).reshape(lanes, n, 4)
    sc[:, ::5] = np.array([1, 0, 0, 0], dtype=np.uint64)     # (over-full buckets: the heavy path reads the shared entries too)
    sd = torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()
    torch.cuda.synchronize()
    want = {k: [orc.msm(g, pts, inf, sc[ln]) for ln in range(lanes)] for k, (g, pts, inf, _) in keys.items()} if n <= 3000 else None

    def run(order, flags):
        outs = {}
        for k, same in zip(order, flags):
            g = keys[k][0]
            outs[k] = np.zeros((lanes, 18 * g), dtype=np.uint64)
            c.msm_async(keys[k][3], sd.data_ptr(), n, lanes, czk.CZK_SCALAR_CANONICAL, outs[k], stable=True, same_scalars=same)
        c.sync()
        return outs

    def same(k, o):     # (Jacobian triples are not canonical and the order inside a bucket is not fixed: compare the points)
        return all(_same_point(c, orc, keys[k][0], o[ln], ref[k][ln]) for ln in range(lanes))

    def counts():
        return c.profile_read("msm_sort")[1], c.profile_read("msm_sort_reused")[1]

    ref = run(["b_g2", "a", "b_g1", "x"], [False] * 4)          # every call sorts
    assert counts() == (4, 0)
    if want:
        for k in ref:
            for ln in range(lanes):
                assert _same_point(c, orc, keys[k][0], ref[k][ln], want[k][ln]), (k, ln)
    c.profile_reset()
    # b_g2 sorts; a has other points at infinity: sorts; b_g1 and x find b_g2's entries two slots back (a G2 sort read by the twisted Edwards kernels)
    got = run(["b_g2", "a", "b_g1", "x"], [False, True, True, True])
    assert counts() == (2, 2)
    for k in got:
        assert same(k, got[k]), k
    c.profile_reset()
    got = run(["b_g2", "b_g1", "x", "a"], [False, True, True, True])
    assert counts() == (2, 2)
    for k in got:
        assert same(k, got[k]), k
    c.profile_reset()
    # nothing survives czk_ctx_sync; the flag on a first call has nothing to take
    got = run(["b_g1"], [True])
    got2 = run(["x"], [True])
    assert counts() == (2, 0) and same("b_g1", got["b_g1"]) and same("x", got2["x"])
    c.profile_reset()
    # more calls in flight than workspace slots: the borrowed entries are protected until their last reader is done
    order = ["b_g2"] + ["b_g1", "x"] * 5 + ["b_g2", "b_g1"]
    got_l = []
    outs = []
    for i, k in enumerate(order):
        o = np.zeros((lanes, 18 * keys[k][0]), dtype=np.uint64)
        c.msm_async(keys[k][3], sd.data_ptr(), n, lanes, czk.CZK_SCALAR_CANONICAL, o, stable=True, same_scalars=i > 0)
        outs.append((k, o))
    c.sync()
    assert counts() == (1, len(order) - 1)
    for k, o in outs:
        assert same(k, o), k
    # a group ends where the next call without the flag begins: the second proof over the same buffer sorts again, with or without a czk_ctx_sync in between
    c.profile_reset()
    got = run(["b_g2", "b_g1", "b_g2", "b_g1", "x"], [False, True, False, True, True])
    assert counts() == (2, 3)
    for k in got:
        assert same(k, got[k]), k
    # ... and a call over OTHER scalars without the flag ends it too (the flag names the most recent unflagged call's scalars)
    sd2 = sd.clone()
    torch.cuda.synchronize()
    c.profile_reset()
    o = [np.zeros((lanes, 18 * g), dtype=np.uint64) for g in (2, 1, 1)]
    c.msm_async(keys["b_g2"][3], sd.data_ptr(), n, lanes, czk.CZK_SCALAR_CANONICAL, o[0], stable=True)
    c.msm_async(keys["a"][3], sd2.data_ptr(), n, lanes, czk.CZK_SCALAR_CANONICAL, o[1], stable=True)
    c.msm_async(keys["b_g1"][3], sd.data_ptr(), n, lanes, czk.CZK_SCALAR_CANONICAL, o[2], stable=True, same_scalars=True)
    c.sync()
    assert counts() == (3, 0) and same("b_g2", o[0]) and same("a", o[1]) and same("b_g1", o[2])
    c.set_option("msm_sort_reuse", 0)
    c.profile_reset()
    got = run(["b_g2", "b_g1", "x"], [False, True, True])
    assert counts() == (3, 0)
    for k in got:
        assert same(k, got[k]), k
    # a shorter call under the same keys (another table set or size): the key of the previous sort does not match
    c.set_option("msm_sort_reuse", 1)
    c.profile_reset()
    o1, o2 = np.zeros((lanes, 36), dtype=np.uint64), np.zeros((lanes, 18), dtype=np.uint64)
    c.msm_async(keys["b_g2"][3], sd.data_ptr(), n, lanes, czk.CZK_SCALAR_CANONICAL, o1, stable=True)
    c.msm_async(keys["b_g1"][3], sd.data_ptr(), n - 1, lanes, czk.CZK_SCALAR_CANONICAL, o2, stable=True, same_scalars=True)
    c.sync()
    assert counts() == (2, 0) and same("b_g2", o1)
    for _, _, _, b in keys.values():
        b.release()
    c.close()


def _msm_random_case(ctx, czk, orc, rng, g, n, seed, tag):
    """One randomised MSM comparison: odd lane counts, random infinity patterns, repeated bases, scalar mixes with many zeros, ones, small
    values and r - small values; table form and CZK_MEM_NO_TABLES against the checker's Pippenger."""
    lanes = int(rng.integers(1, 6))
    _, bases = _bases(ctx, g, n, seed)
    if n > 8:                                               # repeated and opposite bases
        idx = rng.integers(0, n, size=max(2, n // 50))
        bases[idx[1:]] = bases[idx[0]]
    inf = (rng.random(n) < 0.1).astype(np.uint8)
    sc = rand_fr_canonical(seed + 1000, lanes * n).reshape(lanes, n, 4)
    kind = rng.integers(0, 6, size=(lanes, n))
    small = ints_to_limbs([int(v) for v in rng.integers(0, 1 << 20, size=64)], 4)
    for ln in range(lanes):
        sc[ln, kind[ln] == 0] = 0
        sc[ln, kind[ln] == 1] = ints_to_limbs([1], 4)[0]
        m2 = np.nonzero(kind[ln] == 2)[0]
        sc[ln, m2] = small[rng.integers(0, 64, size=m2.size)]
        m3 = np.nonzero(kind[ln] == 3)[0]
        sc[ln, m3] = ints_to_limbs([R_MOD - 1 - int(v) for v in rng.integers(0, 1000, size=max(1, m3.size))], 4)[: m3.size]
    want = [orc.msm(g, bases, inf, sc[ln]) for ln in range(lanes)]
    for flag in (0, czk.CZK_MEM_NO_TABLES):
        b = ctx.register_bases(g, bases, inf, mem=czk.CZK_MEM_HOST | flag)
        got = ctx.msm(b, sc, lanes=lanes)
        for ln in range(lanes):
            assert _same_point(ctx, orc, g, got[ln], want[ln]), (tag, g, n, lanes, ln, flag)
        b.release()


@pytest.mark.parametrize("case", range(14))
def test_msm_randomised_shapes_both_table_forms(ctx, czk, orc, case):
    """Seeded fuzz over the shapes the fixed cases do not hit: sizes around the window-width switches (16 383 / 16 384 points,
    where narrow top windows stop being allowed), odd lane counts, random infinity patterns, scalar mixes with many zeros, ones,
    small values, r - small values and repeated bases -- table form and CZK_MEM_NO_TABLES against the checker's Pippenger."""
    rng = np.random.default_rng(0x5EED + case)
    g = 1 if case % 4 else 2
    n = int([1, 2, 3, 17, 255, 1023, 1025, 4097, 16383, 16384, 16385, 40000, 65537, 9][case])
    if g == 2:
        n = min(n, 1500)
    _msm_random_case(ctx, czk, orc, rng, g, n, 12000 + case, case)


def _ntt_random_case(ctx, czk, orc, rng, mixed, device, seed, tag, max_log=18):
    """One randomised NTT comparison: any prefix length (0 .. D) with a garbage tail, 1 .. 5 lanes, all four kinds -- every limb
    against the checker."""
    import torch
    if mixed:
        k = int(rng.integers(0, max_log - 3))
        size = 3 << k
        log_d = None
    else:
        log_d = int(rng.integers(0, max_log + 1))
        size = 1 << log_d
    lanes = int(rng.integers(1, 6))
    in_len = int(rng.integers(0, size + 1))
    x = orc.fr_from_repr(rand_fr_canonical(seed, lanes * max(in_len, 1))).reshape(lanes, max(in_len, 1), 4)[:, :in_len]
    for kind in (czk.CZK_FFT, czk.CZK_IFFT, czk.CZK_COSET_FFT, czk.CZK_COSET_IFFT):
        buf = np.full((lanes, size, 4), 0xDEADBEEFDEADBEEF, dtype=np.uint64)
        buf[:, :in_len] = x
        if device:
            t = torch.from_numpy(buf.view(np.int64)).cuda()
            torch.cuda.synchronize()
            if mixed:
                ctx.ntt_fr_mixed(t.data_ptr(), size, kind, lanes=lanes, in_len=in_len, mem=czk.CZK_MEM_DEVICE)
            else:
                ctx.ntt_fr(t.data_ptr(), log_d, kind, lanes=lanes, in_len=in_len, mem=czk.CZK_MEM_DEVICE)
            ctx.sync()
            got = t.cpu().numpy().view(np.uint64)
        else:
            if mixed:
                ctx.ntt_fr_mixed(buf, size, kind, lanes=lanes, in_len=in_len)
            else:
                ctx.ntt_fr(buf, log_d, kind, lanes=lanes, in_len=in_len)
            got = buf
        for ln in range(lanes):
            want = orc.ntt_fr_mixed(x[ln], size, kind, in_len) if mixed else orc.ntt_fr(x[ln], log_d, kind, in_len)
            assert np.array_equal(got[ln], want), (tag, size, in_len, lanes, kind, ln)


@pytest.mark.parametrize("case", range(16))
def test_ntt_randomised_shapes(ctx, czk, orc, case):
    """Seeded fuzz: domain sizes 2^0 .. 2^18 and 3 * 2^k, any prefix length (0 .. D) with a garbage tail, 1 .. 5 lanes, all four
    kinds, host and device memory -- every limb against the checker."""
    rng = np.random.default_rng(0xF17 + case)
    _ntt_random_case(ctx, czk, orc, rng, case % 4 == 3, bool(case % 2), 15000 + case, case)


def _poly_random_case(ctx, czk, orc, rng, seed, tag):
    """One randomised comparison of the polynomial / scan entry points (division by X - z, evaluation, running products, batch inversion with
    zeros sprinkled in, the constraint mat-vec) at a size nobody picked."""
    n = int(2 ** rng.uniform(0, 17.5)) - 1
    lanes = int(rng.integers(1, 4))
    p = orc.fr_from_repr(rand_fr_canonical(seed, lanes * max(n, 1)))[: lanes * n].reshape(lanes, n, 4)
    z = orc.fr_from_repr(rand_fr_canonical(seed + 1, 1))[0]
    q, r = ctx.poly_div_linear(p, z, lanes=lanes)
    v = ctx.poly_evaluate(p, z, lanes=lanes)
    for ln in range(lanes):
        qw, rw = orc.poly_div_linear(p[ln], z)
        assert np.array_equal(q[ln], qw) and np.array_equal(r[ln], rw), (tag, n, ln)
        assert np.array_equal(v[ln], orc.fr_horner(p[ln], z) if n else np.zeros(4, dtype=np.uint64)), (tag, n, ln)
    x = p[0].copy()
    assert np.array_equal(ctx.fr_prefix_product(x), orc.fr_prefix_product(x)), (tag, n)
    if n:
        x[rng.random(n) < 0.02] = 0
    assert np.array_equal(ctx.fr_batch_inverse(x, z), orc.fr_batch_inverse(x, z)), (tag, n)
    m, n_vars = int(2 ** rng.uniform(0, 14)), int(2 ** rng.uniform(0, 13))
    row_ptr, col, coeff = _random_csr_limbs(orc, seed + 2, m, n_vars)
    zz = orc.fr_from_repr(rand_fr_canonical(seed + 3, lanes * n_vars)).reshape(lanes, n_vars, 4)
    mat = ctx.r1cs_matrix_register(row_ptr, col, coeff, n_vars)
    got = ctx.r1cs_matvec(mat, zz, lanes=lanes)
    for ln in range(lanes):
        assert np.array_equal(got[ln], orc.r1cs_matvec(row_ptr, col, coeff, zz[ln])), (tag, m, n_vars, ln)
    mat.release()


def test_soak_with_a_fresh_seed(ctx, czk, orc):
    """The fuzzers above on a seed nobody has seen (printed, and named in any failure: CZK_SOAK_SEED reproduces it).  A few cases per
    session by default; CZK_SOAK_SECONDS=600 turns it into a soak run (tools/soak.sh keeps the log under profiles/)."""
    import os
    import time
    seed = int(os.environ.get("CZK_SOAK_SEED", "0"), 0) or int.from_bytes(os.urandom(4), "little")
    budget = float(os.environ.get("CZK_SOAK_SECONDS", "0"))
    rng = np.random.default_rng(seed)
    t0, cases = time.time(), 0
    print(f"soak seed {seed:#x}")
    while True:
        tag = (hex(seed), cases)
        g = 2 if rng.random() < 0.25 else 1
        n = int(2 ** rng.uniform(0, 11 if g == 2 else 16.5))
        _msm_random_case(ctx, czk, orc, rng, g, n, int(rng.integers(1, 1 << 40)), tag)
        _ntt_random_case(ctx, czk, orc, rng, rng.random() < 0.25, rng.random() < 0.5, int(rng.integers(1, 1 << 40)), tag, max_log=17)
        _poly_random_case(ctx, czk, orc, rng, int(rng.integers(1, 1 << 40)), tag)
        cases += 1
        if time.time() - t0 >= budget and cases >= 3:
            break
    print(f"soak seed {seed:#x}: {cases} MSM + {cases} NTT + {cases} polynomial / mat-vec cases in {time.time() - t0:.0f} s, no mismatch")


def test_msm_without_window_tables_empty_and_all_zero(ctx, czk, orc):
    """zero() for empty inputs, all-zero scalars and all-infinity bases in the table-free form as well (variable_base.rs:16-19)."""
    _, bases = _bases(ctx, 1, 8, 5)
    for n in (8, 0):
        b = ctx.register_bases(1, bases[:n] if n else np.zeros((0, 12), dtype=np.uint64), None, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_NO_TABLES)
        out = ctx.msm(b, np.zeros((max(n, 1), 4), dtype=np.uint64)[:n] if n else rand_fr_canonical(1, 4), n_scalars=n if n else 4)
        assert ctx.jac_to_affine(1, out[0])[1][0] == 1
        b.release()
    b = ctx.register_bases(1, bases, np.ones(8, dtype=np.uint8), mem=czk.CZK_MEM_HOST | czk.CZK_MEM_NO_TABLES)
    assert ctx.jac_to_affine(1, ctx.msm(b, rand_fr_canonical(2, 8))[0])[1][0] == 1
    b.release()
    one = ctx.msm_oneshot(2, np.zeros((0, 24), dtype=np.uint64), None, np.zeros((0, 4), dtype=np.uint64))
    assert ctx.jac_to_affine(2, one[0])[1][0] == 1


@pytest.mark.parametrize("g", [1, 2])
def test_msm_short_calls_under_a_long_key_use_narrower_tables(ctx, czk, orc, g):
    """Window width per call (the reference derives c from each call's size, variable_base.rs:21-25): MSMs that use a short prefix of
    a long registered key -- KZG commitments of low-degree polynomials under `powers_of_g`, poly-commit/src/kzg10/mod.rs:159-162 --
    run on secondary table sets (c = 13 / 15 / 17); every size class against the checker's Pippenger on the same prefix, infinity
    bases included, 2 lanes; the key's own tables still serve the long calls; czk_bases_prepare builds a set up front."""
    import torch
    n = (1 << 18) + 3 if g == 1 else (1 << 16) + 3
    k = rand_fr_canonical(0xBA5E5 + 9, n)
    aw = 12 if g == 1 else 24
    kd = torch.from_numpy(k.view(np.int64)).cuda()
    pts = torch.empty((n, aw), dtype=torch.int64, device="cuda")
    ctx.fixed_base_points(g, kd.data_ptr(), out=pts.data_ptr(), n=n, mem=czk.CZK_MEM_DEVICE)
    inf = np.zeros(n, dtype=np.uint8)
    inf[[0, 17, 4099]] = 1
    infd = torch.from_numpy(inf).cuda()
    b = ctx.register_bases(g, pts.data_ptr(), infd.data_ptr(), n=n, mem=czk.CZK_MEM_DEVICE)
    bases_host = pts.cpu().numpy().view(np.uint64)
    c_key, w_key = b.layout()
    assert b.layout_for(n) == (c_key, w_key)
    sizes = [1, 700, 5000, 20000, 70000] + ([150000] if g == 1 else [])
    seen = set()
    b.prepare(5000)                                                  # built up front; the others on first use
    for m in sizes:
        c_m, w_m = b.layout_for(m)
        assert c_m <= c_key and w_m == -(-254 // c_m)
        seen.add(c_m)
        s = orc.fr_from_repr(rand_fr_canonical(0xFACE + m, 2 * m)).reshape(2, m, 4)
        s[1, 0] = 0
        out = ctx.msm(b, s, n_scalars=m, lanes=2, scalar_form=czk.CZK_SCALAR_MONTGOMERY)
        for ln in range(2):
            assert _same_point(ctx, orc, g, out[ln], orc.multi_scalar_mul(g, bases_host[:m], inf[:m], s[ln])), (g, m, ln)
    assert len(seen) >= 3, seen                                      # several width classes were exercised
    # and the full-length call afterwards still runs on the key's own tables (checked through the discrete logs)
    s = rand_fr_canonical(0xC0FFEE + g, n)
    out = ctx.msm(b, s, lanes=1)
    k[inf == 1] = 0
    gen = ctx.fixed_base_points(g, ints_to_limbs([1], 4))[0]
    assert _same_point(ctx, orc, g, out[0], orc.scalar_mul(g, gen, False, ints_to_limbs([dot_mod_r(k, s)], 4)[0]))
    b.release()


def test_g1_bucket_arithmetic_selection_and_any_points_flag(ctx, czk, orc):
    """G1 handles run their buckets in twisted Edwards form (csrc/te.h: the unified 7M addition, exception-free on the prime-order
    subgroup) unless the caller registers arbitrary curve points (CZK_MEM_ANY_POINTS) or a base has no image under the map -- then
    the XYZZ kernels with the reference's complete case analysis (short_weierstrass_jacobian.rs:570-597) stay.  Both forms against the
    checker's Pippenger on the same inputs, equal / opposite / infinity bases and zero / unit scalars included; G2 is always XYZZ."""
    n = 3000
    _, bases = _bases(ctx, 1, n, 777)
    inf = np.zeros(n, dtype=np.uint8)
    bases[3] = bases[2]
    neg = bases[4].copy()
    neg[6:] = orc.fq_neg(bases[4][6:])
    bases[5] = neg
    inf[7] = 1
    sc = rand_fr_canonical(778, 2 * n).reshape(2, n, 4)
    sc[:, 0] = 0
    sc[:, 1] = ints_to_limbs([1], 4)[0]
    sc[:, 2] = sc[:, 3] = ints_to_limbs([5], 4)[0]
    sc[:, 4] = sc[:, 5] = ints_to_limbs([R_MOD - 3], 4)[0]
    want = [orc.msm(1, bases, inf, sc[ln]) for ln in range(2)]
    for flags, arith in ((0, 2), (czk.CZK_MEM_ANY_POINTS, 1), (czk.CZK_MEM_NO_TABLES, 2), (czk.CZK_MEM_NO_TABLES | czk.CZK_MEM_ANY_POINTS, 1)):
        b = ctx.register_bases(1, bases, inf, mem=czk.CZK_MEM_HOST | flags)
        assert b.arith() == arith, (flags, b.arith())
        got = ctx.msm(b, sc, lanes=2)
        for ln in range(2):
            assert _same_point(ctx, orc, 1, got[ln], want[ln]), (flags, ln)
        b.release()
    # a base without an image under the map -- the 2-torsion point (-1, 0): on the curve, not in G1 -- sends the handle to the XYZZ path
    odd = bases.copy()
    minus_one = orc.fq_neg(orc.fq_from_repr(ints_to_limbs([1], 6)))[0]
    odd[9, :6] = minus_one
    odd[9, 6:] = 0
    b = ctx.register_bases(1, odd, inf)
    assert b.arith() == 1
    got = ctx.msm(b, sc[0], lanes=1)
    assert _same_point(ctx, orc, 1, got[0], orc.msm(1, odd, inf, sc[0]))
    b.release()
    _, b2 = _bases(ctx, 2, 50, 779)
    h = ctx.register_bases(2, b2, None)
    assert h.arith() == 1
    h.release()


def _full_order_exceptional_pair(orc):
    """(A, B = A + T): A a curve point of E(Fq) outside G1 (order divisible by the cofactor) WITH an image under the twisted Edwards map,
    T a rational 2-torsion point that maps to a point at infinity of the Edwards model -- the unified law's denominator 1 - D x1 x2 y1 y2
    vanishes for the pair (tools/gen_te_constants.py holds the map; checked here with integers).  Returns Montgomery-form affine limbs."""
    import os
    import random
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gen_te_constants as te
    Q = te.Q
    g = 2
    while pow(g, (Q - 1) // 3, Q) == 1:
        g += 1
    zeta = pow(g, (Q - 1) // 3, Q)                       # a primitive cube root of unity: x^3 + 1 = (x + 1)(x + zeta)(x + zeta^2)
    rng = random.Random(5)
    while True:
        x = rng.randrange(Q)
        if te.is_sq((x ** 3 + 1) % Q):
            A = (x, te.sqrt((x ** 3 + 1) % Q))
            break
    T = ((-zeta) % Q, 0)
    B = te.sw_add(A, T)
    a, b = te.sw_to_te(A), te.sw_to_te(B)
    assert (1 - te.C["D"] * a[0] * b[0] * a[1] * b[1]) % Q == 0      # the exceptional pair of the unified law
    return np.stack([np.concatenate([orc.fq_from_repr(ints_to_limbs([P[0]], 6))[0], orc.fq_from_repr(ints_to_limbs([P[1]], 6))[0]]) for P in (A, B)])


def test_g1_full_order_bases_subgroup_check_and_fallback(ctx, czk, orc):
    """VERDICT r03 item 2.  The reference's MSM is complete on every curve point; its subgroup check lives in deserialisation
    (short_weierstrass_jacobian.rs:131, :868, :881).  Two full-order points forming an exceptional pair of the twisted Edwards law, in ONE bucket:
    (i) CZK_MEM_ANY_POINTS -> the checker's result; (ii) CZK_MEM_CHECK_SUBGROUP -> the check fails, the handle falls back to XYZZ, the checker's
    result; (iii) default -> the handle trusts its caller (documented in czk.h): twisted Edwards kernels, and czk_bases_check_subgroup tells."""
    pair = _full_order_exceptional_pair(orc)
    inf = np.zeros(2, dtype=np.uint8)
    assert orc.g1_on_curve(pair[0]) and orc.g1_on_curve(pair[1])
    for name, sc in (("unit", ints_to_limbs([1, 1], 4)), ("same", np.repeat(rand_fr_canonical(4242, 1), 2, axis=0))):
        want = orc.msm(1, pair, inf, sc)
        for tables in (0, czk.CZK_MEM_NO_TABLES):
            b = ctx.register_bases(1, pair, inf, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_ANY_POINTS | tables)
            assert b.arith() == 1 and b.check_subgroup() == 2
            assert _same_point(ctx, orc, 1, ctx.msm(b, sc)[0], want), (name, tables, "any points")
            b.release()
            b = ctx.register_bases(1, pair, inf, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_CHECK_SUBGROUP | tables)
            assert b.arith() == 1 and b.check_subgroup() == 2, "a failed registration-time check must keep the XYZZ kernels"
            assert _same_point(ctx, orc, 1, ctx.msm(b, sc)[0], want), (name, tables, "checked")
            b.release()
        # the reference's own signature (bases not kept) makes no subgroup assumption either
        assert _same_point(ctx, orc, 1, ctx.msm_oneshot(1, pair, inf, sc)[0], want), (name, "one-shot")
        # default: the caller vouches for its bases.  The handle runs the unified law, which has no answer for this pair -- the hazard the
        # two flags exist for -- and the check, run on request, reports both bases
        b = ctx.register_bases(1, pair, inf)
        assert b.arith() == 2 and b.check_subgroup() == 2
        if name == "unit":      # the two bases alone in one bucket: the exceptional pair is met for certain (under a random scalar other
            # window multiples usually reach the bucket first, and the pair never forms)
            assert not _same_point(ctx, orc, 1, ctx.msm(b, sc)[0], want), "the default path became complete on E: update czk.h / INTEGRATION.md"
        b.release()
    # bases that ARE in G1: the check passes, the fast path stays; mixed with one outsider / one off-curve point it does not
    n = 500
    _, good = _bases(ctx, 1, n, 4243)
    ginf = np.zeros(n, dtype=np.uint8)
    ginf[3] = 1                                                       # a point at infinity passes
    sc = rand_fr_canonical(4244, n)
    b = ctx.register_bases(1, good, ginf, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_CHECK_SUBGROUP)
    assert b.arith() == 2 and b.check_subgroup() == 0
    assert _same_point(ctx, orc, 1, ctx.msm(b, sc)[0], orc.msm(1, good, ginf, sc))
    b.release()
    b = ctx.register_bases(1, good, ginf)
    assert b.check_subgroup() == 0                                    # on request, on a twisted Edwards handle (uses the kept registered points)
    b.release()
    mixed = good.copy()
    mixed[17] = pair[0]
    b = ctx.register_bases(1, mixed, ginf, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_CHECK_SUBGROUP)
    assert b.arith() == 1 and b.check_subgroup() == 1
    assert _same_point(ctx, orc, 1, ctx.msm(b, sc)[0], orc.msm(1, mixed, ginf, sc))
    b.release()
    off = good.copy()
    off[20, 0] ^= np.uint64(1)                                        # not on the curve at all
    b = ctx.register_bases(1, off, ginf, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_ANY_POINTS)
    assert b.check_subgroup() == 1
    b.release()
    # G2 handles always run the complete XYZZ kernels; the check is offered for them too
    _, g2 = _bases(ctx, 2, 40, 4245)
    h = ctx.register_bases(2, g2, None, mem=czk.CZK_MEM_HOST | czk.CZK_MEM_CHECK_SUBGROUP)
    assert h.arith() == 1 and h.check_subgroup() == 0
    h.release()
    g2[5, 0] ^= np.uint64(1)
    h = ctx.register_bases(2, g2, None)
    assert h.check_subgroup() == 1
    h.release()


def test_options_are_explicit_and_the_product_library_ignores_the_environment(czk, orc, monkeypatch):
    """no getenv dispatch in libczk_hip.so.  An environment variable that used to switch kernels changes nothing; the
    rejected variants' options are unknown to the product library (CZK_ERR_ARG) and known to the lab library, which exports the same ABI."""
    for e in ("CZK_MSM_NO_TE", "CZK_MSM_SAT", "CZK_REDUCE_SAT", "CZK_NTT_GEN1", "CZK_SORT_ONEPASS"):
        monkeypatch.setenv(e, "1")
    monkeypatch.setenv("CZK_G2_MODE", "1")
    monkeypatch.setenv("CZK_MSM_C_G1", "9")
    c = czk.Context(0)
    assert c._L.czk_build_is_lab() == 0
    _, bases = _bases(c, 1, 600, 9001)
    b = c.register_bases(1, bases, None)
    assert b.arith() == 2 and b.layout()[0] != 9            # twisted Edwards tables, the cost model's window: the environment was not read
    sc = rand_fr_canonical(9002, 600)
    assert _same_point(c, orc, 1, c.msm(b, sc)[0], orc.msm(1, bases, np.zeros(600, np.uint8), sc))
    b.release()
    for name in ("msm_sat", "msm_no_te", "msm_g2_mode", "msm_affine_rounds", "msm_reduce_sat", "no_such_option"):
        with pytest.raises(czk.CzkError) as ei:
            c.set_option(name, 1)
        assert ei.value.code == 3 and name in str(ei.value)
    with pytest.raises(czk.CzkError):
        c.set_option("msm_window_g1", 5)                    # out of range
    with pytest.raises(czk.CzkError):
        c.set_option("msm_slots", 2)                        # the pipeline exists already
    c.set_option("msm_window_g1", 9)
    b = c.register_bases(1, bases, None)
    assert b.layout()[0] == 9
    assert _same_point(c, orc, 1, c.msm(b, sc)[0], orc.msm(1, bases, np.zeros(600, np.uint8), sc))
    b.release()
    c.close()
    lab = czk.Context(0, lab=True)                          # the lab build translates the tools' environment switches into options
    assert lab._L.czk_build_is_lab() == 1
    b = lab.register_bases(1, bases, None)
    assert b.arith() == 0 and b.layout()[0] == 9            # CZK_MSM_SAT: saturated tables; CZK_MSM_C_G1=9
    assert _same_point(lab, orc, 1, lab.msm(b, sc)[0], orc.msm(1, bases, np.zeros(600, np.uint8), sc))
    b.release()
    lab.close()


@pytest.mark.parametrize("n_constraints,parties", [(10, 2), (1000, 3)])
def test_groth16_local_hbc_scheme_matches_reference(ctx, czk, orc, n_constraints, parties):
    """The reference's `--alg hbc` (mpc-snarks/src/proof.rs:379-387): AdditiveFieldShare (share/add.rs:26-29), ONE lane per party, an open is
    the sum of the lanes (add.rs:256-259), no MAC lane.  Groth16Local(scheme="hbc"): the witness map with the Beaver local half on `parties`
    lanes against the checker's lane-wise sequence, the reconstructed h against the single prover's, the MSMs against the checker's Pippenger."""
    import torch
    from czk_amd.provers import Groth16Local
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        c2 = czk.Context(0, ts.cuda_stream)
        p = Groth16Local(czk, c2, n_constraints, parties, scheme="hbc")
        assert p.lanes == parties and p.lpp == 1 and p.king_lanes == [0]
        a0, b0, c0 = (t.cpu().numpy().view(np.uint64).copy() for t in (p.a0, p.b0, p.c0))
        tx, ty, tz = (t.cpu().numpy().view(np.uint64).copy() for t in (p.tx, p.ty, p.tz))
        wit, asg = p.wit.cpu().numpy().view(np.uint64).copy(), p.asg.cpu().numpy().view(np.uint64).copy()
        p.step()
        torch.cuda.synchronize()
        h_gpu = p.ab.cpu().numpy().view(np.uint64)
    L, D, ld, N = parties, p.D, p.log_d, p.N
    A = [orc.witness_map_pre(a0[ln], b0[ln], ld) for ln in range(L)]
    sa = [orc.fr_add(A[ln][0], tx[ln]) for ln in range(L)]
    sb = [orc.fr_add(A[ln][1], ty[ln]) for ln in range(L)]
    sx, oy = sa[0], sb[0]
    for ln in range(1, L):
        sx, oy = orc.fr_add(sx, sa[ln]), orc.fr_add(oy, sb[ln])
    hs = []
    for ln in range(L):
        ab = orc.fr_sub(orc.fr_sub(tz[ln], orc.fr_mul(ty[ln], sx)), orc.fr_mul(tx[ln], oy))
        if ln == 0:
            ab = orc.fr_add(ab, orc.fr_mul(sx, oy))                        # the king applies the shift
        hs.append(orc.witness_map_post(ab, c0[ln], ld))
        assert np.array_equal(h_gpu[ln], hs[-1]), ln

    def lane_sum(v):
        t = v[0]
        for ln in range(1, L):
            t = orc.fr_add(t, v[ln])
        return t
    assert np.array_equal(lane_sum(h_gpu), orc.witness_map_plain(lane_sum(a0), lane_sum(b0), lane_sum(c0), ld))
    for name, g, n, sd, inf_first, scal in (("h", 1, D - 1, 1, False, h_gpu), ("l", 1, N, 2, False, wit), ("a", 1, N + 1, 3, False, asg),
                                             ("b_g1", 1, N + 1, 4, True, asg), ("b_g2", 2, N + 1, 5, True, asg)):
        bases = ctx.fixed_base_points(g, rand_fr_canonical(0xBA5E5 + sd, n))
        inf = np.zeros(n, dtype=np.uint8)
        inf[0] = 1 if inf_first else 0
        for ln in range(L):
            assert _same_point(ctx, orc, g, p.results[name][ln], orc.multi_scalar_mul(g, bases, inf, scal[ln].reshape(-1, 4))), (name, ln)
    c2.close()


@pytest.mark.parametrize("n_constraints,parties", [(10, 3), (1000, 4)])
def test_groth16_local_gsz_scheme_matches_reference(ctx, czk, orc, n_constraints, parties):
    """The reference's `--alg gsz` (mpc-snarks/src/proof.rs:379-387): GszFieldShare (share/gsz20/mod.rs:115-118), ONE Shamir-share lane per party
    (degree t = (n - 1) / 2), public addends on every lane, products by batch_mult (:556-595): x y + r2, the king opens at degree 2t and hands the
    value back (batch_king_compute, f = identity), minus r, with the stubbed double share r = r2 = 1.  Groth16Local(scheme="gsz") against the
    checker's lane-wise restatement (its own Shamir open, share/gsz20/mod.rs:440-466); the lanes of h must open (degree t) to the single prover's
    h; the five MSMs against the checker's Pippenger on every lane."""
    import torch
    from czk_amd.provers import Groth16Local
    ts = torch.cuda.Stream()
    with torch.cuda.stream(ts):
        c2 = czk.Context(0, ts.cuda_stream)
        p = Groth16Local(czk, c2, n_constraints, parties, scheme="gsz")
        t = (parties - 1) // 2
        assert p.lanes == parties and p.lpp == 1 and p.king_lanes == list(range(parties)) and p.gsz_t == t
        a0, b0, c0 = (v.cpu().numpy().view(np.uint64).copy() for v in (p.a0, p.b0, p.c0))
        wit, asg = p.wit.cpu().numpy().view(np.uint64).copy(), p.asg.cpu().numpy().view(np.uint64).copy()
        p.step()
        torch.cuda.synchronize()
        h_gpu = p.ab.cpu().numpy().view(np.uint64)
    L, D, ld, N = parties, p.D, p.log_d, p.N
    one = orc.fr_from_repr(ints_to_limbs([1], 4))
    ones = np.tile(one[0], (D, 1))
    # the lanes really are degree-t Shamir shares of the witness: they open to the squaring chain, and a tighter bound fails
    w_open, bad = orc.gsz_open(wit, degree=t)
    assert bad == 0 and orc.gsz_open(wit, degree=t - 1)[1] > 0
    assert np.array_equal(orc.fr_mul(w_open[:-1], w_open[:-1]), w_open[1:])
    A = [orc.witness_map_pre(a0[ln], b0[ln], ld) for ln in range(L)]
    prod = np.stack([orc.fr_add(orc.fr_mul(A[ln][0], A[ln][1]), ones) for ln in range(L)])       # x * y + r2
    value, bad = orc.gsz_open(prod, degree=2 * t)                                                  # the king's open_degree_vec
    assert bad == 0
    ab = orc.fr_sub(value, ones)                                                                   # - r
    for ln in range(L):
        assert np.array_equal(h_gpu[ln], orc.witness_map_post(ab, c0[ln], ld)), ln
    h_open, bad = orc.gsz_open(h_gpu, degree=t)
    a_open, b_open, c_open = (orc.gsz_open(v, degree=t)[0] for v in (a0, b0, c0))
    assert bad == 0 and np.array_equal(h_open, orc.witness_map_plain(a_open, b_open, c_open, ld))
    for name, g, n, sd, inf_first, scal in (("h", 1, D - 1, 1, False, h_gpu), ("l", 1, N, 2, False, wit), ("a", 1, N + 1, 3, False, asg),
                                             ("b_g1", 1, N + 1, 4, True, asg), ("b_g2", 2, N + 1, 5, True, asg)):
        bases = ctx.fixed_base_points(g, rand_fr_canonical(0xBA5E5 + sd, n))
        inf = np.zeros(n, dtype=np.uint8)
        inf[0] = 1 if inf_first else 0
        for ln in range(L):
            assert _same_point(ctx, orc, g, p.results[name][ln], orc.multi_scalar_mul(g, bases, inf, scal[ln].reshape(-1, 4))), (name, ln)
    c2.close()


@pytest.mark.parametrize("n_constraints,parties,scheme", [(10, 2, "spdz"), (1000, 2, "spdz"), (1000, 3, "hbc"), (1000, 1, "hbc"), (1000, 3, "gsz")])
def test_create_proof_matches_checker(ctx, czk, orc, n_constraints, parties, scheme):
    """The whole of create_proof (mpc-snarks/src/groth/prover.rs:66-178) for public r, s: the five MSMs of step(), then calculate_coeff
    (:216-232: query[0], vk_param and r delta / s delta on the king's lanes) and Proof{a, b, c} per share lane (Groth16Local.create_proof)
    against the checker's restatement fed with the checker's own Pippenger results, in affine.  With the parties' sh lanes added up the
    proof must be the SINGLE prover's (parties = 1: T = Fr, no sharing), element for element."""
    import torch
    from czk_amd.provers import Groth16Local
    from test_device_handles import checker_create_proof, groth16_pk_extras
    rs = rand_fr_canonical(0xC0FFEE + 99, 2)

    def prove(parties, scheme):
        ts = torch.cuda.Stream()
        with torch.cuda.stream(ts):
            c2 = czk.Context(0, ts.cuda_stream)
            p = Groth16Local(czk, c2, n_constraints, parties, scheme=scheme)
            p.step()
            torch.cuda.synchronize()
            scal = {"h": p.ab.cpu().numpy().view(np.uint64).copy(), "l": p.wit.cpu().numpy().view(np.uint64).copy(),
                    "a": p.asg.cpu().numpy().view(np.uint64).copy()}
            scal["b_g1"] = scal["b_g2"] = scal["a"]
            res = {k: v.copy() for k, v in p.results.items()}
            proof = p.create_proof(res, rs[0], rs[1])
            aff = [{k: c2.jac_to_affine(2 if k == "b" else 1, proof[k][ln]) for k in ("a", "b", "c")} for ln in range(p.lanes)]
            out = (p.lanes, p.lpp, list(p.king_lanes), p.D, p.N, scal, res, proof, aff)
            del p
            c2.close()
        return out
    L, lpp, king, D, N, scal, res, proof, aff = prove(parties, scheme)
    # the checker's MSM results on the lanes' scalars, then its create_proof
    want_jac = {}
    for name, g, n, sd, inf_first in (("h", 1, D - 1, 1, False), ("l", 1, N, 2, False), ("a", 1, N + 1, 3, False), ("b_g1", 1, N + 1, 4, True), ("b_g2", 2, N + 1, 5, True)):
        bases = ctx.fixed_base_points(g, rand_fr_canonical(0xBA5E5 + sd, n))
        inf = np.zeros(n, dtype=np.uint8)
        inf[0] = 1 if inf_first else 0
        want_jac[name] = [orc.multi_scalar_mul(g, bases, inf, scal[name][ln].reshape(-1, 4)) for ln in range(L)]
    pk = groth16_pk_extras(lambda g, k: orc.fixed_base_points(g, k)[0])
    want = checker_create_proof(orc, pk, want_jac, rs[0], rs[1], king_lanes=king)
    for ln in range(L):
        for key in ("a", "b", "c"):
            waff, winf = want[ln][key]
            assert bool(aff[ln][key][1][0]) == bool(winf) and (winf or np.array_equal(aff[ln][key][0][0], waff)), (ln, key)
    if parties > 1:
        # open the proof: sum of the parties' sh lanes (czk_jac_add) -- times 1 / n for Shamir shares on the n-th roots of unity, whose
        # interpolating polynomial has p(0) = (1 / n) sum_j p(w^j) -- == the single prover's proof
        _, _, _, _, _, _, _, _, aff1 = prove(1, "hbc")
        for key, g in (("a", 1), ("b", 2), ("c", 1)):
            acc = proof[key][0]
            for j in range(1, parties):
                acc = ctx.jac_add(g, acc, proof[key][lpp * j])
            if scheme == "gsz":
                from util import R_MOD
                acc = ctx.jac_scalar_mul(g, acc, ints_to_limbs([pow(parties, -1, R_MOD)], 4)[0])
            got = ctx.jac_to_affine(g, acc)
            assert not got[1][0] and np.array_equal(got[0][0], aff1[0][key][0][0]), key


@pytest.mark.parametrize("ranks,size", [(2, ["--constraints", "1000"]), (3, ["--log-n", "12"])])
def test_groth16_intra_party_split_matches_the_one_gpu_layout(ranks, size):
    """SURVEY.md section 8e, "optional intra-party split (MSM by base range -> one extra point-add)": bench.py --layout split runs ONE proof over N
    ranks -- the witness map in full on every rank, every MSM over that rank's range of the bases (1 / N of the window tables), the N partial
    sums of each MSM gathered and added on rank 0 (parallel.combine_split_results, czk_jac_add).  The 20 group elements must equal the
    one-GPU layout's (digest over their affine forms) and verify against the known discrete logs.  The ranks share this box's GPU: gloo."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = size + ["--parties", "2", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-seam-report", "--no-other-workloads"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common, capture_output=True, text=True, timeout=280, env=env, cwd=root)
    assert one.returncode == 0, __import__('util').child_errors(one.stderr)
    many = __import__('util').run_ranks([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(ranks), "--layout", "split", "--backend", "gloo",
                           "--device", "0"] + common, capture_output=True, text=True, timeout=280, env=env, cwd=root)
    assert many.returncode == 0, __import__('util').child_errors(many.stderr)
    d1 = json.loads(one.stdout.strip().splitlines()[-1])
    d2 = json.loads(many.stdout.strip().splitlines()[-1])
    assert d2["n_gpus"] == ranks and d2["ranks_seen_by_backend"] == ranks and d2["config"]["layout"] == "split" and d2["scaling"] == "strong"
    assert d1["results_checked"] and d2["results_checked"]
    assert d1["config"]["results_sha256"] == d2["config"]["results_sha256"]


def test_fr_copy_3d_matches_numpy_indexing(ctx, czk):
    """czk_fr_copy_3d: the one strided copy / fill behind every re-layout of the polynomial provers -- dense copies (copy-engine path), prefix
    copies with different lane strides, zero fill of a tail, interleave / de-interleave by a stride, a lane broadcast (source stride 0)."""
    import torch
    lanes, n = 3, 60
    src = torch.from_numpy(rand_fr_canonical(77, lanes * n).reshape(lanes, n, 4).view(np.int64)).cuda()
    h = src.cpu().numpy()

    def run(dst_shape, dst_off, ds, s_off, ss, n3, fill=False):
        dst = torch.full(dst_shape + (4,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ctx.fr_copy_3d(dst.data_ptr() + 32 * dst_off, ds, None if fill else src.data_ptr() + 32 * s_off, None if fill else ss, n3)
        ctx.sync()
        return dst.cpu().numpy()
    got = run((lanes, n), 0, (0, n, 1), 0, (0, n, 1), (1, lanes, n))                       # dense
    assert np.array_equal(got, h)
    got = run((lanes, 100), 0, (0, 100, 1), 0, (0, n, 1), (1, lanes, 40))                  # resized: prefix into wider lanes, the rest untouched
    assert np.array_equal(got[:, :40], h[:, :40]) and (got[:, 40:] == -1).all()
    got = run((lanes, 100), 40, (0, 100, 1), 0, None, (1, lanes, 60), fill=True)           # ... and the tail cleared
    assert (got[:, 40:] == 0).all() and (got[:, :40] == -1).all()
    got = run((lanes, 50), 0, (0, 50, 1), 10, (0, n, 1), (1, lanes, 50))                   # drop_first
    assert np.array_equal(got, h[:, 10:])
    k = 4                                                                                  # strided_split: out[l * k + j][i] = a[l][i * k + j]
    got = run((lanes * k, n // k), 0, (k * (n // k), n // k, 1), 0, (n, 1, k), (lanes, k, n // k))
    want = h.reshape(lanes, n // k, k, 4).transpose(0, 2, 1, 3).reshape(lanes * k, n // k, 4)
    assert np.array_equal(got, want)
    got = run((5, n), 0, (0, n, 1), n, (0, 0, 1), (1, 5, n))                               # lane 1 of the source on five lanes
    assert all(np.array_equal(got[j], h[1]) for j in range(5))
    ctx.fr_copy_3d(0, (0, 0, 1), None, None, (0, 3, 3))                                     # nothing to do: no dereference
    with pytest.raises(czk.CzkError):
        ctx.fr_copy_3d(0, (0, 0, 1), None, None, (1, 1, 1))


def test_vec_scale_with_a_host_scalar(ctx, czk, orc):
    """czk_fr_vec_scale with CZK_MEM_DEVICE | CZK_MEM_SCALAR_HOST: device vectors, the scalar by value with the launch"""
    import torch
    from czk_amd import binding
    n = 1000
    a = orc.fr_from_repr(rand_fr_canonical(5, n))
    k = orc.fr_from_repr(rand_fr_canonical(6, 1))[0]
    ad = torch.from_numpy(a.view(np.int64)).cuda()
    out = torch.empty_like(ad)
    ctx.fr_vec_scale(ad.data_ptr(), k, out=out.data_ptr(), n=n, mem=czk.CZK_MEM_DEVICE | binding.CZK_MEM_SCALAR_HOST)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), orc.fr_mul(a, np.tile(k, (n, 1))))


@pytest.mark.parametrize("g", [1, 2])
def test_jac_scalar_mul_and_neg_match_reference_group_law(ctx, czk, orc, g):
    """czk_jac_scalar_mul = ProjectiveCurve::mul (algebra/ec/src/lib.rs:215-226), czk_jac_neg = Neg (short_weierstrass_jacobian.rs:737-748),
    host-side: against the checker's double-and-add, for canonical and Montgomery scalars, 0, 1, r - 1 and the identity"""
    from util import R_MOD
    _, bases = _bases(ctx, g, 3, 91)
    ks = np.concatenate([rand_fr_canonical(92, 3), ints_to_limbs([0, 1, R_MOD - 1], 4)])
    one = orc.fr_from_repr(ints_to_limbs([1], 4))[0]
    for i, k in enumerate(ks):
        base = bases[i % 3]
        jac = orc.scalar_mul(g, base, False, ints_to_limbs([1], 4)[0])                     # into_projective
        want = orc.scalar_mul(g, base, False, k)
        assert _same_point(ctx, orc, g, ctx.jac_scalar_mul(g, jac, k), want), i
        km = orc.fr_from_repr(k.reshape(1, 4))[0]
        assert _same_point(ctx, orc, g, ctx.jac_scalar_mul(g, jac, km, czk.CZK_SCALAR_MONTGOMERY), want), i
        neg = ctx.jac_neg(g, want)
        assert ctx.jac_to_affine(g, ctx.jac_add(g, want, neg))[1][0] == 1                 # P + (-P) = identity
    zero = np.zeros(18 if g == 1 else 36, dtype=np.uint64)
    assert ctx.jac_to_affine(g, ctx.jac_scalar_mul(g, zero, ks[0]))[1][0] == 1
    assert one.any()
