"""The shortened Groth16 witness map: czk_witness_map_post_h (one transform of c), czk_witness_map_pre_masked, czk_spdz_open_combine.

Every expected value comes from the CPU checker (oracle/orc.py): its witness_map_pre / witness_map_post per lane and its field operations
composed here; comparisons are limb for limb.  The context option "witness_map_short" (a bit per shortened call: 7 = the default, all three;
0 = the longer kernel sequences) must not change a value, so the cases run under both and each is compared with the checker, never with the other.

Domain sizes: 2^3 and 2^10 run the first-generation passes (one and two of them), 2^11 is the first size of the second generation
(passes of 6 + 5 stage bits), 2^14 = 7 + 7, 2^15 = 5 + 5 + 5, 2^16 = 6 + 5 + 5: every last-pass kernel that carries the new stores."""
import numpy as np
import pytest

from guarded import Guards, grid_threads
from util import R_MOD, ints_to_limbs, rand_fr_canonical

pytestmark = pytest.mark.gpu

LOG_DS = [3, 10, 11, 14, 15, 16]
DEVICE, MUL = 1, 2


@pytest.fixture(scope="module")
def czk():
    import czk_amd
    return czk_amd


@pytest.fixture(scope="module")
def ctxs(czk):
    """option value -> context"""
    c = {v: czk.Context(0, options={"witness_map_short": v}) for v in (7, 0)}
    yield c
    for x in c.values():
        x.close()


@pytest.fixture(scope="module")
def pool(orc):
    """Montgomery Fr elements shared by the cases (every limb pattern below r is one); the first four of a draw are 0, 1, r - 1, r - 2"""
    base = rand_fr_canonical(0x5107, 9 * (1 << 16))
    edge = ints_to_limbs([0, 1, R_MOD - 1, R_MOD - 2], 4)

    def draw(seed, lanes, n):
        off = (seed * 7919) % (base.shape[0] - lanes * n + 1)
        a = base[off:off + lanes * n].reshape(lanes, n, 4).copy()
        k = min(n, 4)
        a[:, :k] = edge[:k]
        return a
    return draw


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def run(ctx, fn, *a, **k):
    import torch
    torch.cuda.synchronize()
    fn(*a, **k)
    ctx.sync()


def padded(x, n, d):
    out = np.zeros((d, 4), dtype=np.uint64)
    out[:n] = x[:n]
    return out


@pytest.mark.parametrize("lanes", [1, 3, 4])
@pytest.mark.parametrize("log_d", LOG_DS)
def test_witness_map_post_h(ctxs, orc, pool, log_d, lanes):
    d = 1 << log_d
    ab = pool(1 + log_d, lanes, d)
    c = pool(2 + log_d, lanes, d)                       # elements from c_len on are garbage the call must not read
    for c_len in (1, d - 3, d):
        want = [orc.witness_map_post(ab[ln], padded(c[ln], c_len, d), log_d) for ln in range(lanes)]
        for opt, ctx in ctxs.items():
            tab, tc = dev(ab), dev(c)
            run(ctx, ctx.witness_map_post_h, tab.data_ptr(), tc.data_ptr(), log_d, lanes, c_len=c_len)
            got = host(tab)
            for ln in range(lanes):
                assert np.array_equal(got[ln], want[ln]), (opt, c_len, ln)


@pytest.mark.parametrize("log_d", LOG_DS)
def test_witness_map_of_a_satisfied_instance(ctxs, orc, log_d):
    """The squaring circuit (a_i = b_i = w_i, c_i = w_{i+1}, a[N] = 1, a[N + 1] = out) with N = D - 3 constraints: h equals the checker's
    witness map and its top coefficient is zero (the quotient is exact, deg h <= D - 2)."""
    d = 1 << log_d
    n_c = d - 3
    one = orc.fr_from_repr(ints_to_limbs([1], 4))
    w = [orc.fr_from_repr(rand_fr_canonical(9 + log_d, 1))]
    for _ in range(n_c):
        w.append(orc.fr_sqr(w[-1]))
    w = np.vstack(w)
    a, b, c = (np.zeros((d, 4), dtype=np.uint64) for _ in range(3))
    a[:n_c], b[:n_c], c[:n_c] = w[:n_c], w[:n_c], w[1:n_c + 1]
    a[n_c], a[n_c + 1] = one[0], w[n_c]
    want = orc.witness_map_plain(a, b, c, log_d)
    assert not want[d - 1].any()
    for opt, ctx in ctxs.items():
        ta, tb, tc = dev(a), dev(b), dev(c)
        ctx.witness_map_pre(ta.data_ptr(), tb.data_ptr(), log_d, 1, a_len=n_c + 2, b_len=n_c)
        ctx.fr_vec_op(MUL, ta.data_ptr(), tb.data_ptr(), out=ta.data_ptr(), n=d, mem=DEVICE)
        run(ctx, ctx.witness_map_post_h, ta.data_ptr(), tc.data_ptr(), log_d, 1, c_len=n_c)
        h = host(ta)
        assert np.array_equal(h, want), opt
        assert not h[d - 1].any(), opt


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("log_d", LOG_DS)
def test_witness_map_pre_masked(ctxs, orc, pool, log_d, lanes):
    d = 1 << log_d
    a_len, b_len = d - 3, d - 5
    a, b = pool(3 + log_d, lanes, d), pool(4 + log_d, lanes, d)
    ma, mb = pool(5 + log_d, lanes, d), pool(6 + log_d, lanes, d)      # start with 0, 1, r - 1, r - 2
    ma[:, 5::3] = ints_to_limbs([R_MOD - 1], 4)[0]                      # r - 1 on a third of the indices: the canonical sum wraps wherever the transform is not 0
    mb[:, 4::2] = 0
    mb[:, 7::5] = ints_to_limbs([R_MOD - 1], 4)[0]
    want = []
    for ln in range(lanes):
        ea, eb = orc.witness_map_pre(padded(a[ln], a_len, d), padded(b[ln], b_len, d), log_d)
        want.append((orc.fr_add(ea, ma[ln]), orc.fr_add(eb, mb[ln])))
    for opt, ctx in ctxs.items():
        g = Guards("cuda")
        fma, fmb = g.freeze(ma, "mask_a"), g.freeze(mb, "mask_b")
        ta, tb = dev(a), dev(b)
        run(ctx, ctx.witness_map_pre_masked, ta.data_ptr(), tb.data_ptr(), fma.ptr, fmb.ptr, log_d, lanes, a_len=a_len, b_len=b_len)
        g.check()
        ga, gb = host(ta), host(tb)
        for ln in range(lanes):
            assert np.array_equal(ga[ln], want[ln][0]), (opt, "a", ln)
            assert np.array_equal(gb[ln], want[ln][1]), (opt, "b", ln)


def _sum(orc, rows):
    s = rows[0]
    for r in rows[1:]:
        s = orc.fr_add(s, r)
    return s


OPEN_SIZES = ["1", "255", "256", "257", "sweep+257"]


@pytest.mark.parametrize("king", ["first", "none"])
@pytest.mark.parametrize("size", OPEN_SIZES)
@pytest.mark.parametrize("parties", [2, 3])
def test_spdz_open_combine(ctxs, orc, pool, parties, size, king):
    """n = 256 k + 1 with k one block more than a grid sweep of 8 blocks per CU covers: the loop's second trip writes the tail.  The MAC lanes are
    consistent (party 0's MAC = value - the others') except at one index of `a` and another of `b`, where chk must be non-zero and nowhere else."""
    t = grid_threads(8)
    n = t + 257 if size == "sweep+257" else int(size)
    assert size != "sweep+257" or (n > t and n % 256 == 1)
    L = 2 * parties
    a, b, tx, ty, tz = (pool(20 + i + parties, L, n) if n <= (1 << 16) else np.tile(pool(20 + i + parties, L, 1 << 15), (1, -(-n // (1 << 15)), 1))[:, :n].copy()
                        for i in range(5))
    for v in (a, b):                                   # consistent MACs: mac_0 = value - the other parties' MAC lanes
        v[1] = orc.fr_sub(_sum(orc, [v[2 * p] for p in range(parties)]), _sum(orc, [v[2 * p + 1] for p in range(1, parties)]))
    bad_a, bad_b = n - 1, n // 2
    one = orc.fr_from_repr(ints_to_limbs([1], 4))[0]
    a[3, bad_a] = orc.fr_add(a[3, bad_a].reshape(1, 4), one.reshape(1, 4))[0]
    b[1, bad_b] = orc.fr_add(b[1, bad_b].reshape(1, 4), one.reshape(1, 4))[0]
    mask = 0b11 if king == "first" else 0
    sx, oy = _sum(orc, [a[2 * p] for p in range(parties)]), _sum(orc, [b[2 * p] for p in range(parties)])
    chk_a, chk_b = sx, oy
    for p in range(parties):
        chk_a, chk_b = orc.fr_sub(chk_a, a[2 * p + 1]), orc.fr_sub(chk_b, b[2 * p + 1])
    assert np.nonzero(chk_a.any(axis=1))[0].tolist() == [bad_a] and np.nonzero(chk_b.any(axis=1))[0].tolist() == [bad_b]
    open_ = orc.fr_mul(sx, oy)
    ab = []
    for ln in range(L):
        r = orc.fr_sub(orc.fr_sub(tz[ln], orc.fr_mul(ty[ln], sx)), orc.fr_mul(tx[ln], oy))
        ab.append(orc.fr_add(r, open_) if (mask >> ln) & 1 else r)
    for opt, ctx in ctxs.items():
        g = Guards("cuda")
        f = [g.freeze(v, nm) for v, nm in zip((a, b, tx, ty, tz), ("a", "b", "tx", "ty", "tz"))]
        o = [g.out(1, n, name=nm) for nm in ("sx", "oy", "chk_a", "chk_b")] + [g.out(L, n, name="ab")]
        run(ctx, ctx.spdz_open_combine, *[x.ptr for x in f], parties, mask, *[x.ptr for x in o], n)
        got = g.check()                                # inputs unchanged, nothing outside the five footprints written
        for have, want, nm in zip(got[:4], (sx, oy, chk_a, chk_b), ("sx", "oy", "chk_a", "chk_b")):
            assert np.array_equal(have[0], want), (opt, nm)
        for ln in range(L):
            assert np.array_equal(got[4][ln], ab[ln]), (opt, "ab", ln)
        assert np.nonzero(got[2][0].any(axis=1))[0].tolist() == [bad_a] and np.nonzero(got[3][0].any(axis=1))[0].tolist() == [bad_b]


def _same_point(ctx, orc, g, have_jac, want_jac):
    want_aff, want_inf = orc.jac_to_affine(g, want_jac)
    have_aff, have_inf = ctx.jac_to_affine(g, have_jac)
    return bool(have_inf[0]) == want_inf and (want_inf or np.array_equal(have_aff[0], want_aff))


@pytest.mark.parametrize("scheme,parties", [("spdz", 2), ("spdz", 3), ("hbc", 2)])
@pytest.mark.parametrize("n_constraints", [10, 1024, 8])
def test_groth16_local_end_to_end(czk, orc, n_constraints, scheme, parties):
    """Groth16Local.step under both option values: the same `h`, and `h` and the five MSM results per lane equal the checker's pipeline (the lane-wise witness map with
    the Beaver local half, then Pippenger on the same bases and scalars) -- the comparison of test_gpu_parity's config-0 test, for every local scheme."""
    import torch
    from czk_amd.provers import Groth16Local
    runs = {}
    for opt in (7, 0):
        ts = torch.cuda.Stream()
        with torch.cuda.stream(ts):
            c2 = czk.Context(0, ts.cuda_stream, options={"witness_map_short": opt})
            p = Groth16Local(czk, c2, n_constraints, parties, scheme=scheme)
            inp = {k: host(getattr(p, k)).copy() for k in ("a0", "b0", "c0", "tx", "ty", "tz", "wit", "asg")}
            p.step()
            torch.cuda.synchronize()
            runs[opt] = (host(p.ab).copy(), {k: v.copy() for k, v in p.results.items()}, inp, p.N, p.D, p.log_d, p.lanes, list(p.king_lanes))
            if scheme == "spdz":
                assert not bool(p.chk.any().item())
        c2.close()
    h_gpu, res, inp, N, D, ld, L, kings = runs[7]
    assert L == (2 * parties if scheme == "spdz" else parties) and kings == list(range(L // parties))
    assert np.array_equal(runs[0][0], h_gpu)
    # the checker's pipeline
    sh_lanes = range(0, L, L // parties)
    A = [orc.witness_map_pre(inp["a0"][ln], inp["b0"][ln], ld) for ln in range(L)]
    sa = [orc.fr_add(A[ln][0], inp["tx"][ln]) for ln in range(L)]
    sb = [orc.fr_add(A[ln][1], inp["ty"][ln]) for ln in range(L)]
    sx, oy = _sum(orc, [sa[ln] for ln in sh_lanes]), _sum(orc, [sb[ln] for ln in sh_lanes])
    for ln in range(L):
        ab = orc.fr_sub(orc.fr_sub(inp["tz"][ln], orc.fr_mul(inp["ty"][ln], sx)), orc.fr_mul(inp["tx"][ln], oy))
        if ln in kings:
            ab = orc.fr_add(ab, orc.fr_mul(sx, oy))
        assert np.array_equal(h_gpu[ln], orc.witness_map_post(ab, inp["c0"][ln], ld)), ln
    # the five MSMs of both runs against the checker's Pippenger, in affine (a Jacobian triple depends on the order of the bucket additions)
    c3 = czk.Context(0)
    for name, g, n, sd, inf_first, scal in (("h", 1, D - 1, 1, False, h_gpu), ("l", 1, N, 2, False, inp["wit"]), ("a", 1, N + 1, 3, False, inp["asg"]),
                                             ("b_g1", 1, N + 1, 4, True, inp["asg"]), ("b_g2", 2, N + 1, 5, True, inp["asg"])):
        bases = c3.fixed_base_points(g, rand_fr_canonical(0xBA5E5 + sd, n))
        inf = np.zeros(n, dtype=np.uint8)
        inf[0] = 1 if inf_first else 0
        for ln in range(L):
            want = orc.multi_scalar_mul(g, bases, inf, scal[ln].reshape(-1, 4))
            for opt in (7, 0):
                assert _same_point(c3, orc, g, runs[opt][1][name][ln], want), (opt, name, ln)
    c3.close()
