"""Where the device-memory entry points write, and the second trip of their grid-stride loops.

Every case passes DEVICE pointers.  Every output lives in a guarded buffer (tests/guarded.py: sentinel pads before, after and in the stride
padding between lanes) and every input is frozen; values are compared limb for limb with the CPU checker (oracle/orc.py), or with the
checker's field operations composed here.  The pointwise calls run at grid_tail_sizes(K): one element, around one block of 256, and
either side of T = K x CUs x 256, the size above which the capped grid-stride loop runs a second time.  The group-side calls compare with
the same call through host memory (which the existing tests compare with the reference): only their footprint is new here."""
import ctypes as C
import functools

import numpy as np
import pytest

from guarded import Guards, grid_tail_sizes, grid_threads, per_cu_blocks
from util import R_MOD, ints_to_limbs, rand_fr_canonical, splitmix_u64

pytestmark = pytest.mark.gpu

SIZES = ["1", "255", "256", "257", "T-1", "T+3"]          # labels of grid_tail_sizes (the CU count is only known on the GPU)
SIZES_INPLACE = ["1", "255", "256", "257", "T+3"]
EDGE = ints_to_limbs([0, 1, R_MOD - 1, R_MOD - 2], 4)
EDGE_NZ = ints_to_limbs([2, 1, R_MOD - 1, R_MOD - 2], 4)
ADD, SUB, MUL = 0, 1, 2
FFT, IFFT, COSET_FFT, COSET_IFFT = 0, 1, 2, 3
DEVICE, SCALAR_HOST = 1, 256


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def size_of(label, per_cu):
    return grid_tail_sizes(per_cu)[SIZES.index(label)]


def crosses(label, n, per_cu):
    """A `T+3` case must really run the loop's second trip on this GPU; returns T."""
    t = grid_threads(per_cu)
    if label == "T+3":
        assert n > t, (n, t)
    return t


@functools.lru_cache(maxsize=4)
def _words(seed, n):
    w = splitmix_u64(seed, 4 * n).reshape(n, 4)
    w[:, 3] &= np.uint64((1 << 60) - 1)                   # < 2^252 < r: a valid element without the rejection loop
    return w


def fr(seed, n, edge=EDGE):
    """(n, 4) Fr elements (any limbs below r are a Montgomery value) whose first elements are 0, 1, r - 1, r - 2."""
    a = (rand_fr_canonical(seed, n) if n <= 40000 else _words(seed, n).copy()) if n else np.zeros((0, 4), dtype=np.uint64)
    k = min(n, 4)
    a[:k] = edge[:k]
    return a


def one(orc):
    return orc.fr_from_repr(np.array([[1, 0, 0, 0]], dtype=np.uint64))[0]


def small(orc, v):
    return orc.fr_from_repr(np.array([[v, 0, 0, 0]], dtype=np.uint64))[0]


def tile(k, n):
    return np.tile(np.asarray(k, dtype=np.uint64).reshape(1, 4), (n, 1))


def fr_pow(orc, base, e):
    r, b = one(orc), np.asarray(base, dtype=np.uint64).reshape(4)
    while e:
        if e & 1:
            r = orc.fr_mul(r, b)
        b = orc.fr_sqr(b)
        e >>= 1
    return r


def run(ctx, fn, *a, **k):
    """The context has a stream of its own: torch's fills first, the call, then the context's work."""
    import torch
    torch.cuda.synchronize()
    r = fn(*a, **k)
    ctx.sync()
    return r


def G():
    return Guards("cuda")


def eq(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
        raise AssertionError(f"{what}: {bad.size} of {got.shape[0]} rows differ, first at {bad[:6].tolist()}, last at {int(bad[-1])}")


def corrupt_at(n, t):
    """Index 0, one index in the loop's second trip when there is one (else the middle), and the last."""
    return sorted({0, t + 1 if n > t + 1 else n // 2, n - 1})


# ------------------------------------------------------------------------------------------------ pointwise, 8 blocks per CU
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("op", [ADD, SUB, MUL])
def test_fr_vec_op(ctx, orc, op, size):
    n = size_of(size, per_cu_blocks("k_vec_op"))
    crosses(size, n, 8)
    g = G()
    a, b = fr(101, n), fr(102, n)[::-1].copy()
    fa, fb, out = g.freeze(a, "a"), g.freeze(b, "b"), g.out(1, n)
    run(ctx, ctx.fr_vec_op, op, fa.ptr, fb.ptr, out=out.ptr, n=n, mem=DEVICE)
    eq(g.check()[0][0], (orc.fr_add, orc.fr_sub, orc.fr_mul)[op](a, b), "fr_vec_op")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("scalar", ["device", "host"])
def test_fr_vec_scale(ctx, orc, scalar, size):
    n = size_of(size, per_cu_blocks("k_vec_scale_dev" if scalar == "device" else "k_vec_scale"))
    crosses(size, n, 8)
    g = G()
    a, k = fr(103, n), fr(104, 8)[7]
    fa, out = g.freeze(a, "a"), g.out(1, n)
    if scalar == "device":
        fk = g.freeze(k.reshape(1, 4), "k")
        run(ctx, ctx.fr_vec_scale, fa.ptr, fk.ptr, out=out.ptr, n=n, mem=DEVICE)
    else:
        run(ctx, ctx.fr_vec_scale, fa.ptr, k, out=out.ptr, n=n, mem=DEVICE | SCALAR_HOST)
    eq(g.check()[0][0], orc.fr_mul(a, tile(k, n)), "fr_vec_scale")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("add_open", [False, True])
def test_fr_beaver_combine(ctx, orc, add_open, size):
    n = size_of(size, per_cu_blocks("k_beaver"))
    crosses(size, n, 8)
    g = G()
    v = [fr(110 + i, n) for i in range(5)]
    v[3], v[4] = v[3][::-1].copy(), np.roll(v[4], 1, axis=0)
    f = [g.freeze(x, nm) for x, nm in zip(v, ("x", "y", "z", "sx", "oy"))]
    out = g.out(1, n)
    run(ctx, ctx.fr_beaver_combine, *[x.ptr for x in f], add_open, out=out.ptr, n=n, mem=DEVICE)
    x, y, z, sx, oy = v
    want = orc.fr_sub(orc.fr_sub(z, orc.fr_mul(y, sx)), orc.fr_mul(x, oy))
    eq(g.check()[0][0], orc.fr_add(want, orc.fr_mul(sx, oy)) if add_open else want, "fr_beaver_combine")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("which", ["fr_into_repr", "fr_from_repr"])
def test_fr_repr(ctx, orc, which, size):
    n = size_of(size, per_cu_blocks("k_repr"))
    crosses(size, n, 8)
    g = G()
    a = fr(120, n)
    fa, out = g.freeze(a, "a"), g.out(1, n)
    run(ctx, getattr(ctx, which), fa.ptr, out=out.ptr, n=n, mem=DEVICE)
    eq(g.check()[0][0], getattr(orc, which)(a), which)


def _spdz_shares(orc, n, parties, seed):
    """parties x 2 x n with consistent MACs (mac_0 = value - the other parties' MACs: the king's mac_share is one, spdz.rs:31-37)"""
    sh = fr(seed, parties * 2 * n).reshape(parties, 2, n, 4)
    value = sh[0, 0]
    rest = np.zeros((n, 4), dtype=np.uint64)
    for p in range(1, parties):
        value = orc.fr_add(value, sh[p, 0])
        rest = orc.fr_add(rest, sh[p, 1])
    sh[0, 1] = orc.fr_sub(value, rest)
    return sh, value


@pytest.mark.parametrize("size", SIZES)
def test_fr_spdz_open(ctx, orc, size):
    n = size_of(size, per_cu_blocks("k_spdz_open"))
    t = crosses(size, n, 8)
    parties = 3
    sh, value = _spdz_shares(orc, n, parties, 130)
    for bad_at in ([], corrupt_at(n, t)):
        g = G()
        s = sh.copy()
        for i in bad_at:
            s[1, 1, i] = orc.fr_add(s[1, 1, i], one(orc))          # a MAC share: the value is untouched, the check fails
        chk = value
        for p in range(parties):
            chk = orc.fr_sub(chk, s[p, 1])
        want_bad = int(np.count_nonzero(chk.any(axis=1)))
        assert want_bad == len(bad_at)
        fs, out = g.freeze(s, "shares"), g.out(1, n, name="out_value")
        got_bad = run(ctx, ctx.fr_spdz_open, fs.ptr, parties, n, out.ptr)
        eq(g.check()[0][0], value, "fr_spdz_open value")
        assert got_bad == want_bad, (got_bad, bad_at)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("mode", ["out", "count", "both"])
def test_fr_lanes_sum(ctx, orc, mode, size):
    n = size_of(size, per_cu_blocks("k_lanes_sum"))
    t = crosses(size, n, 8)
    k = 3
    x = fr(140, k * n).reshape(k, n, 4)
    bad_at = []
    if mode != "out":                                               # sums that vanish except at three places
        x[2] = orc.fr_sub(np.zeros((n, 4), dtype=np.uint64), orc.fr_add(x[0], x[1]))
        bad_at = corrupt_at(n, t)
        for i in bad_at:
            x[1, i] = orc.fr_add(x[1, i], one(orc))
    want = orc.fr_add(orc.fr_add(x[0], x[1]), x[2])
    want_nz = int(np.count_nonzero(want.any(axis=1)))
    g = G()
    fx = g.freeze(x, "x")
    out = g.out(1, n) if mode != "count" else None
    nz = run(ctx, ctx.fr_lanes_sum, fx.ptr, k, n, out_ptr=out.ptr if out else None, count_nonzero=mode != "out")
    got = g.check()
    if out:
        eq(got[0][0], want, "fr_lanes_sum")
    if mode != "out":
        assert want_nz == len(bad_at) and nz == want_nz, (nz, want_nz, bad_at)
        assert sorted(np.nonzero(want.any(axis=1))[0].tolist()) == bad_at


@pytest.mark.parametrize("size", SIZES)
def test_fr_spdz_dx(ctx, orc, size):
    n = size_of(size, per_cu_blocks("k_spdz_dx"))
    crosses(size, n, 8)
    g = G()
    value, mac, ms = fr(150, n), fr(151, n)[::-1].copy(), fr(152, 8)[6]
    fv, fm, out = g.freeze(value, "value"), g.freeze(mac, "mac"), g.out(1, n)
    run(ctx, ctx.fr_spdz_dx, fv.ptr, fm.ptr, ms, out.ptr, n)
    eq(g.check()[0][0], orc.fr_sub(orc.fr_mul(tile(ms, n), value), mac), "fr_spdz_dx")


def _gsz_shares(orc, n, parties, seed):
    """Shares of degree-1 polynomials c0 + c1 X at the powers of the order-`parties` root: (parties, n, 4), and c0"""
    w = orc.fr_root_of_unity_mixed(parties)
    c = fr(seed, 2 * n).reshape(2, n, 4)
    sh, wj = np.zeros((parties, n, 4), dtype=np.uint64), one(orc)
    for j in range(parties):
        sh[j] = orc.fr_add(c[0], orc.fr_mul(c[1], tile(wj, n)))
        wj = orc.fr_mul(wj, w)
    return sh, c[0]


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("bound", ["degree", "degrees", "random"])
@pytest.mark.parametrize("parties", [3, 4])
def test_fr_gsz_open(ctx, orc, parties, bound, size):
    n = size_of(size, per_cu_blocks("k_gsz_open"))
    t = crosses(size, n, 8)
    degrees = None
    if bound == "random":                                           # any field elements: the checker reports value and violation count for them too
        sh = fr(160 + parties, parties * n).reshape(parties, n, 4)
        degrees = (np.arange(n, dtype=np.uint32) * 7 % parties).astype(np.uint32)
        bad_at = None
    else:
        sh, c0 = _gsz_shares(orc, n, parties, 170 + parties)
        bad_at = corrupt_at(n, t)
        for i in bad_at:
            sh[0, i] = orc.fr_add(sh[0, i], one(orc))               # adds a multiple of a degree-(parties - 1) Lagrange polynomial
        if bound == "degrees":                                      # bound 1 everywhere but at the last element, whose bound admits any polynomial
            degrees = np.ones(n, dtype=np.uint32)
            degrees[n - 1] = parties - 1
    want, want_bad = orc.gsz_open(sh, degree=1, degrees=degrees)
    if bad_at is not None:
        ok = np.ones(n, dtype=bool)
        ok[bad_at] = False
        eq(want[ok], c0[ok], "checker: untouched elements open to c0")
        assert want_bad == sum(1 for i in bad_at if degrees is None or degrees[i] == 1)
    g = G()
    fs, out = g.freeze(sh, "shares"), g.out(1, n, name="out_value")
    fd = g.freeze(degrees, "degrees") if degrees is not None else None
    got_bad = run(ctx, ctx.fr_gsz_open, fs.ptr, parties, n, out.ptr, degree=1, degrees_ptr=fd.ptr if fd else None)
    eq(g.check()[0][0], want, "fr_gsz_open value")
    assert got_bad == want_bad, (got_bad, want_bad)


# ------------------------------------------------------------------------------------------------ in place
# The aliasings callers rely on: czk_fr_vec_op with out == a (keygen.py, provers.py's accumulations and opens, czk_fr_lagrange_coefficients in
# poly.hip) and czk_fr_from_repr / czk_fr_into_repr with out == a (provers.py, tools/polyvm_host.hpp).  out == b is allowed by the header as well.
@pytest.mark.parametrize("size", SIZES_INPLACE)
@pytest.mark.parametrize("case", ["add_out_is_a", "sub_out_is_a", "mul_out_is_a", "mul_out_is_b", "sub_out_is_b"])
def test_fr_vec_op_in_place(ctx, orc, case, size):
    n = size_of(size, 8)
    crosses(size, n, 8)
    op = {"add": ADD, "sub": SUB, "mul": MUL}[case[:3]]
    import torch
    a, b = fr(180, n), fr(181, n)[::-1].copy()
    g = G()
    io = g.out(1, n, name="in/out")
    alias_a = case.endswith("a")
    io.view()[0, :n] = torch.from_numpy((a if alias_a else b).view(np.int64)).cuda()
    other = g.freeze(b if alias_a else a, "other")
    pa, pb = (io.ptr, other.ptr) if alias_a else (other.ptr, io.ptr)
    run(ctx, ctx.fr_vec_op, op, pa, pb, out=io.ptr, n=n, mem=DEVICE)
    eq(g.check()[0][0], (orc.fr_add, orc.fr_sub, orc.fr_mul)[op](a, b), case)


@pytest.mark.parametrize("size", SIZES_INPLACE)
@pytest.mark.parametrize("which", ["fr_into_repr", "fr_from_repr"])
def test_fr_repr_in_place(ctx, orc, which, size):
    import torch
    n = size_of(size, 8)
    crosses(size, n, 8)
    a = fr(182, n)
    g = G()
    io = g.out(1, n, name="in/out")
    io.view()[0, :n] = torch.from_numpy(a.view(np.int64)).cuda()
    run(ctx, getattr(ctx, which), io.ptr, out=io.ptr, n=n, mem=DEVICE)
    eq(g.check()[0][0], getattr(orc, which)(a), which)


# ------------------------------------------------------------------------------------------------ 16 blocks per CU
def _lincomb(ctx, orc, spec, coeffs, cst, lanes, mask, out_len, pool):
    """spec: (term lanes, length); term k is the pool from element 977 k on.  Returns (guards, wanted (lanes, out_len, 4))."""
    g = G()
    fp = g.freeze(pool, "terms")
    offs = [977 * k for k in range(len(spec))]
    terms = [pool[o:o + ln * n].reshape(ln, n, 4) for o, (ln, n) in zip(offs, spec)]
    out = g.out(lanes, out_len)
    run(ctx, ctx.fr_lincomb, [fp.ptr + 32 * o for o in offs], [n for _, n in spec], [ln for ln, _ in spec], coeffs, lanes, mask, out.ptr, out_len, constant=cst)
    want = np.zeros((lanes, out_len, 4), dtype=np.uint64)
    for l in range(lanes):
        lifts = lanes == 1 or (mask >> l) & 1
        if cst is not None and lifts:
            want[l] = tile(cst, out_len)
        for (ln, n), t, c in zip(spec, terms, coeffs):
            m = min(n, out_len)
            if (ln == 1 and lanes > 1 and not lifts) or not m:
                continue
            want[l, :m] = orc.fr_add(want[l, :m], orc.fr_mul(t[l if ln > 1 else 0][:m], tile(c, m)))
    return g, want


@pytest.mark.parametrize("size", SIZES)
def test_fr_lincomb(ctx, orc, size):
    """A shared term, a public term, a unit coefficient, a term 7 elements shorter than the result, one longer, and a constant."""
    L = size_of(size, per_cu_blocks("k_lincomb"))
    t = crosses(size, L, 16)
    coeffs = [fr(190, 12)[5 + k] for k in range(5)]
    coeffs[2] = one(orc)
    cst = fr(191, 8)[5]
    for lanes, mask in ([(2, 0b01)] if L > 1000 else [(1, 0), (3, 0b101)]):
        spec = [(lanes, L), (1, L), (lanes, L), (lanes, max(L - 7, 0)), (lanes, L + 1)]
        pool = fr(192, lanes * (L + 1) + 977 * len(spec))
        g, want = _lincomb(ctx, orc, spec, coeffs, cst, lanes, mask, L, pool)
        got = g.check()[0]
        for l in range(lanes):
            eq(got[l], want[l], f"fr_lincomb lane {l} of {lanes}")
        if size == "T+3":
            assert got.shape[1] > t and np.array_equal(got[:, t:], want[:, t:])


def test_fr_lincomb_full_spec_at_257(ctx, orc):
    """The term mix of test_fr_lincomb_matches_checker (4 lanes, mask 0b0011, ragged shared and public terms, an empty one) at out_len = 257."""
    lanes, out_len, mask = 4, 257, 0b0011
    spec = [(4, 257), (1, 211), (4, 1), (1, 257), (4, 300), (4, 256), (1, 0), (4, 150)]
    coeffs = [fr(193, 16)[5 + k] for k in range(len(spec))]
    coeffs[2] = one(orc)
    g, want = _lincomb(ctx, orc, spec, coeffs, fr(194, 8)[5], lanes, mask, out_len, fr(195, 4 * 300 + 977 * len(spec)))
    eq(g.check()[0], want, "fr_lincomb")


@pytest.mark.parametrize("size", ["small", "T+"])
def test_fr_copy_3d_interleave(ctx, size):
    """The strided_split shape (de-interleave by 4) into lanes with gaps: out[l * 4 + j][k] = a[l][4 k + j]."""
    t = grid_threads(per_cu_blocks("k_copy_3d"))
    lanes, n, L = (3, 4, 17) if size == "small" else (1, 4, t // 4 + 1)
    total = n * L
    if size != "small":
        assert lanes * total > t
    a = fr(200, lanes * total).reshape(lanes, total, 4)
    g = G()
    fa, out = g.freeze(a, "src"), g.out(lanes * n, L, L + 5)
    run(ctx, ctx.fr_copy_3d, out.ptr, (n * (L + 5), L + 5, 1), fa.ptr, (total, 1, n), (lanes, n, L))
    want = a.reshape(lanes, L, n, 4).transpose(0, 2, 1, 3).reshape(lanes * n, L, 4)
    eq(g.check()[0].reshape(-1, 4), want.reshape(-1, 4), "fr_copy_3d")


@pytest.mark.parametrize("size", ["small", "T+"])
def test_fr_copy_3d_fill(ctx, size):
    """A zero fill of four lanes with gaps between them (not a memset)."""
    t = grid_threads(per_cu_blocks("k_copy_3d"))
    L = 33 if size == "small" else t // 4 + 1
    if size != "small":
        assert 4 * L > t
    g = G()
    out = g.out(4, L, L + 5)
    run(ctx, ctx.fr_copy_3d, out.ptr, (0, L + 5, 1), None, None, (1, 4, L))
    assert not g.check()[0].any()


@pytest.mark.parametrize("size", ["257", "T+3"])
def test_r1cs_matvec(ctx, orc, size):
    """One or two entries per row, every 16th row with a coefficient of one (the bit-31 path), 2 lanes at strides n_vars + 5 and m + 5."""
    m = size_of(size, per_cu_blocks("k_r1cs_matvec"))
    t = crosses(size, m, 16)
    n_vars, lanes = 5000, 2
    per_row = 1 + (np.arange(m) % 2)
    row_ptr = np.concatenate([[0], np.cumsum(per_row)]).astype(np.uint64)
    nnz = int(row_ptr[-1])
    col = (splitmix_u64(210, nnz) % np.uint64(n_vars)).astype(np.uint32)
    coeff = fr(211, nnz)
    unit_rows = np.arange((m - 2) % 16, m, 16)                      # row m - 2 among them: the second trip takes both branches too
    coeff[row_ptr[unit_rows].astype(np.int64)] = one(orc)
    z = fr(212, lanes * (n_vars + 5)).reshape(lanes, n_vars + 5, 4)
    g = G()
    frp, fc, fk, fz = g.freeze(row_ptr, "row_ptr"), g.freeze(col, "col_idx"), g.freeze(coeff, "coeff"), g.freeze(z, "z")
    mat = run(ctx, ctx.r1cs_matrix_register, frp.ptr, fc.ptr, fk.ptr, n_vars, mem=DEVICE, m=m, nnz=nnz)
    try:
        out = g.out(lanes, m, m + 5)
        run(ctx, ctx.r1cs_matvec, mat, fz.ptr, lanes=lanes, out=out.ptr, z_stride=n_vars + 5, out_stride=m + 5, mem=DEVICE)
    finally:
        mat.release()
    got = g.check()[0]                                              # rows [m, out_stride) of both lanes still hold the sentinel
    for l in range(lanes):
        want = orc.r1cs_matvec(row_ptr, col, coeff, z[l, :n_vars])
        eq(got[l], want, f"r1cs_matvec lane {l}")
        if size == "T+3":
            assert np.array_equal(got[l, t:], want[t:]) and unit_rows[-1] >= t


# ------------------------------------------------------------------------------------------------ segmented scans
SCAN_SIZES = [1, 2, 31, 32, 33, 1023, 1024, 1025, 32 ** 3 + 1]


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("lanes", [1, 3])
def test_poly_div_linear(ctx, orc, lanes, n):
    p = fr(300, lanes * n).reshape(lanes, n, 4)
    z = fr(301, 8)[5]
    for with_rem in (True, False):
        g = G()
        fp = g.freeze(p, "coeffs")
        q = g.out(lanes, n - 1, name="quotient")
        rem = g.out(1, lanes, name="remainder") if with_rem else None
        run(ctx, ctx.poly_div_linear, fp.ptr, z, lanes=lanes, n=n, quotient=q.ptr, remainder=rem.ptr if rem else None, mem=DEVICE)
        got = g.check()
        if n == 1:
            assert q.untouched()                                    # a constant has no quotient word
        for l in range(lanes):
            wq, wr = orc.poly_div_linear(p[l], z)
            eq(got[0][l], wq, f"quotient lane {l}")
            if with_rem:
                assert np.array_equal(got[1][0][l], wr), l


@pytest.mark.parametrize("n", SCAN_SIZES)
@pytest.mark.parametrize("lanes", [1, 3])
def test_poly_evaluate(ctx, orc, lanes, n):
    p = fr(310, lanes * n).reshape(lanes, n, 4)
    z = fr(311, 8)[5]
    g = G()
    fp, val = g.freeze(p, "coeffs"), g.out(1, lanes, name="values")
    run(ctx, ctx.poly_evaluate, fp.ptr, z, lanes=lanes, n=n, values=val.ptr, mem=DEVICE)
    got = g.check()[0][0]
    for l in range(lanes):
        assert np.array_equal(got[l], orc.fr_horner(p[l], z)), l


def test_poly_evaluate_many(ctx, orc):
    """17 polynomials (two batches of the kernel's 16 descriptors); every value buffer is a slice of ONE guarded buffer, so a value written to a
    neighbour's slot or past the last one shows."""
    sizes = SCAN_SIZES + [3, 64, 65, 100, 2049, 5000, 7, 1]
    lanes = [1, 3] * 8 + [3]
    assert len(sizes) == 17 == len(lanes)
    polys = [fr(320 + k, ln * n).reshape(ln, n, 4) for k, (n, ln) in enumerate(zip(sizes, lanes))]
    zs = [fr(340 + k, 8)[5] for k in range(17)]
    g = G()
    fps = [g.freeze(p, f"poly {k}") for k, p in enumerate(polys)]
    vals = g.out(1, sum(lanes), name="values")
    at = np.concatenate([[0], np.cumsum(lanes)])
    run(ctx, ctx.poly_evaluate_many, [f.ptr for f in fps], sizes, lanes, zs, [vals.lane_ptr(0, int(at[k])) for k in range(17)])
    got = g.check()[0][0]
    for k in range(17):
        for l in range(lanes[k]):
            assert np.array_equal(got[at[k] + l], orc.fr_horner(polys[k][l], zs[k])), (k, l)


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_fr_prefix_product(ctx, orc, n):
    x = fr(330, n, EDGE_NZ)
    g = G()
    fx, out = g.freeze(x, "x"), g.out(1, n)
    run(ctx, ctx.fr_prefix_product, fx.ptr, out=out.ptr, n=n, mem=DEVICE)
    eq(g.check()[0][0], orc.fr_prefix_product(x), "fr_prefix_product")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 128 - 1, 64 * 128 + 1])
def test_fr_batch_inverse(ctx, orc, n):
    """Zeros at the ends of the 64-element segments, one segment all zero, with and without the coefficient; refuses out == v."""
    import czk_amd
    v = fr(335, n, EDGE_NZ)
    v[63::64] = 0
    v[64::64] = 0
    v[n - 1] = 0
    if n >= 192:
        v[128:192] = 0
    if n == 1:
        v = fr(335, 1, EDGE_NZ)                                     # a single non-zero element; the single zero follows
    for vv in ([v] if n > 1 else [v, np.zeros((1, 4), dtype=np.uint64)]):
        for coeff in (None, fr(336, 8)[5]):
            g = G()
            fv, out = g.freeze(vv, "v"), g.out(1, n)
            run(ctx, ctx.fr_batch_inverse, fv.ptr, coeff, out=out.ptr, n=n, mem=DEVICE)
            eq(g.check()[0][0], orc.fr_batch_inverse(vv, one(orc) if coeff is None else coeff), "fr_batch_inverse")
    with pytest.raises(czk_amd.CzkError):
        ctx.fr_batch_inverse(fv.ptr, None, out=fv.ptr, n=n, mem=DEVICE)
    fv.check()


@pytest.mark.parametrize("m,n", [(5, 5), (6, 5), (257, 256), (3 * 256 + 1, 256)])
@pytest.mark.parametrize("lanes", [1, 3])
def test_poly_div_vanishing(ctx, orc, lanes, m, n):
    """a = q (X^n - 1) + r: q_i = sum_{k >= 1} a_{i + k n}, r_i = sum_{k >= 0} a_{i + k n}, from the checker's additions."""
    a = fr(340, lanes * m).reshape(lanes, m, 4)
    chunks = -(-m // n)
    wq, wr = np.zeros((lanes, m - n, 4), dtype=np.uint64), np.zeros((lanes, n, 4), dtype=np.uint64)
    for l in range(lanes):
        pad = np.zeros((chunks * n, 4), dtype=np.uint64)
        pad[:m] = a[l]
        acc = np.zeros((n, 4), dtype=np.uint64)
        for k in range(chunks - 1, 0, -1):
            acc = orc.fr_add(acc, pad[k * n:(k + 1) * n])
            lo, hi = (k - 1) * n, min(k * n, m - n)
            wq[l, lo:hi] = acc[:hi - lo]
        wr[l] = orc.fr_add(acc, pad[:n])
    for with_rem in (False, True):
        g = G()
        fa = g.freeze(a, "coeffs")
        q = g.out(lanes, m - n, name="quotient")
        rem = g.out(lanes, n, name="remainder") if with_rem else None
        run(ctx, ctx.poly_div_vanishing, fa.ptr, n, lanes=lanes, m=m, quotient=q.ptr, remainder=rem.ptr if rem else None, mem=DEVICE)
        got = g.check()
        if m == n:
            assert q.untouched()
        eq(got[0].reshape(-1, 4), wq.reshape(-1, 4), "quotient")
        if with_rem:
            eq(got[1].reshape(-1, 4), wr.reshape(-1, 4), "remainder")


# ------------------------------------------------------------------------------------------------ powers and Lagrange coefficients
@functools.lru_cache(maxsize=None)
def _power_table(which):
    import orc
    base = {"random": fr(400, 8)[5], "one": one(orc), "zero": np.zeros(4, dtype=np.uint64)}[which]
    out = np.zeros((8193, 4), dtype=np.uint64)
    out[0] = one(orc)
    for i in range(1, 8193):                                        # g^i by the checker's multiplications, one at a time
        out[i] = orc.fr_mul(out[i - 1], base)
    return base, out


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 8191, 8192, 8193])
@pytest.mark.parametrize("mem", ["host", "device"])
def test_fr_powers(ctx, orc, mem, n):
    """out[i] = c g^i: 64 entries per thread, 128 threads per block -- either side of one thread's and one block's share."""
    c = fr(401, 8)[6]
    for which in ("random", "one", "zero"):
        base, table = _power_table(which)
        for cc in (None, c):
            want = table[:n] if cc is None else orc.fr_mul(table[:n], tile(cc, n))
            if mem == "host":
                got = ctx.fr_powers(base, n, c=cc)
            else:
                g = G()
                out = g.out(1, n)
                run(ctx, ctx.fr_powers, base, n, c=cc, out=out.ptr, mem=DEVICE)
                got = g.check()[0][0]
                if n == 0:
                    assert out.untouched()
            eq(got, want, f"fr_powers g = {which}, c {'given' if cc is not None else 'absent'}")


@pytest.mark.parametrize("log_d", [3, 7])
def test_fr_lagrange_coefficients(ctx, orc, log_d):
    D = 1 << log_d
    dc = orc.domain_constants(log_d)
    w = np.zeros((D, 4), dtype=np.uint64)
    w[0] = one(orc)
    for j in range(1, D):
        w[j] = orc.fr_mul(w[j - 1], dc["group_gen"])
    tau = fr(410, 8)[5]
    zt = orc.fr_sub(fr_pow(orc, tau, D), one(orc))
    assert zt.any()
    k = orc.fr_mul(zt, dc["size_inv"])
    outside = orc.fr_mul(orc.fr_mul(tile(k, D), w), orc.fr_inv(orc.fr_sub(tile(tau, D), w)))     # L_j(tau) = Z(tau) / D * w^j / (tau - w^j)
    unit = np.zeros((D, 4), dtype=np.uint64)
    unit[2] = one(orc)
    for t, want, n_outs in ((tau, outside, (1, D - 1, D)), (w[2], unit, (2, D))):
        for n_out in n_outs:
            g = G()
            out = g.out(1, n_out)
            run(ctx, ctx.fr_lagrange_coefficients, log_d, t, n_out=n_out, out=out.ptr, mem=DEVICE)
            eq(g.check()[0][0], want[:n_out], f"lagrange n_out {n_out}")     # tau = w^2 with n_out = 2: the unit lies outside the output, all zero


# ------------------------------------------------------------------------------------------------ transforms
def _fill(out, data, in_len):
    """The first in_len elements of every lane; the rest keeps the sentinel as the garbage beyond in_len."""
    import torch
    out.view()[:, :in_len] = torch.from_numpy(np.ascontiguousarray(data[:, :in_len]).view(np.int64)).cuda()


@pytest.mark.parametrize("log_d", [0, 1, 5, 9, 13])
def test_ntt_fr(ctx, orc, log_d):
    D, lanes = 1 << log_d, 3
    x = fr(500 + log_d, lanes * D).reshape(lanes, D, 4)
    for in_len in sorted({D, max(D - 3, 1)}):
        for kind in (FFT, IFFT, COSET_FFT, COSET_IFFT):
            g = G()
            io = g.out(lanes, D, name="data")
            _fill(io, x, in_len)
            run(ctx, ctx.ntt_fr, io.ptr, log_d, kind, lanes=lanes, in_len=in_len, mem=DEVICE)
            got = g.check()[0]
            for l in range(lanes):
                eq(got[l], orc.ntt_fr(x[l], log_d, kind, in_len), f"ntt_fr kind {kind} in_len {in_len} lane {l}")


@pytest.mark.parametrize("k", [0, 1, 4, 9])
def test_ntt_fr_mixed(ctx, orc, k):
    N, lanes = 3 << k, 2
    x = fr(520 + k, lanes * N).reshape(lanes, N, 4)
    for in_len in sorted({N, max(N - 2, 1)}):
        for kind in (FFT, IFFT, COSET_FFT, COSET_IFFT):
            g = G()
            io = g.out(lanes, N, name="data")
            _fill(io, x, in_len)
            run(ctx, ctx.ntt_fr_mixed, io.ptr, N, kind, lanes=lanes, in_len=in_len, mem=DEVICE)
            got = g.check()[0]
            for l in range(lanes):
                eq(got[l], orc.ntt_fr_mixed(x[l], N, kind, in_len), f"ntt_fr_mixed kind {kind} in_len {in_len} lane {l}")


def _mixed_consts(orc, N):
    w = orc.fr_root_of_unity_mixed(N)
    return w, orc.fr_inv(w), orc.fr_inv(small(orc, N)), orc.fr_inv(small(orc, 22))


def test_ntt_fr_mixed_split_second_trip(ctx, orc):
    """N = 3 * 2^19: the first size at which k_mixed_split loops.  The full transform on one CPU core takes several seconds, so eight outputs per
    transform are evaluated with the checker's Horner rule: X[i] = x(w^i) for FFT, y[j] = x(w^-j) / N * 22^-j for COSET_IFFT."""
    k = 19
    N = 3 << k
    t = grid_threads(per_cu_blocks("k_mixed_split"))
    assert N > t
    w, w_inv, n_inv, g_inv = _mixed_consts(orc, N)
    x = fr(540, N)
    idx = [0, 1, 255, t - 1, t, t + 1, (t + N) // 2, N - 1]
    assert sum(i >= t for i in idx) >= 3
    for kind in (FFT, COSET_IFFT):
        g = G()
        io = g.out(1, N, name="data")
        _fill(io, x[None], N)
        run(ctx, ctx.ntt_fr_mixed, io.ptr, N, kind, lanes=1, in_len=N, mem=DEVICE)
        got = g.check()[0][0]
        for i in idx:
            if kind == FFT:
                want = orc.fr_horner(x, fr_pow(orc, w, i))
            else:
                want = orc.fr_mul(orc.fr_mul(orc.fr_horner(x, fr_pow(orc, w_inv, i)), n_inv), fr_pow(orc, g_inv, i))
            assert np.array_equal(got[i], want), (kind, i)


@pytest.fixture(scope="module")
def mixed21(ctx):
    """x and FFT(x) at N = 3 * 2^21 (M = 2^21: the first size at which k_mixed_combine loops), computed once in a guarded buffer."""
    N = 3 << 21
    x = fr(541, N)
    g = G()
    io = g.out(1, N, name="data")
    _fill(io, x[None], N)
    run(ctx, ctx.ntt_fr_mixed, io.ptr, N, FFT, lanes=1, in_len=N, mem=DEVICE)
    g.check()
    return x, g, io


def test_ntt_fr_mixed_combine_second_trip_values(ctx, orc, mixed21):
    """Outputs i0, i0 + M, i0 + 2 M (the three a combine thread writes) for two i0 in the first block and two in the second trip."""
    x, g, io = mixed21
    N, M = 3 << 21, 1 << 21
    t = grid_threads(per_cu_blocks("k_mixed_combine"))
    assert M > t
    w = orc.fr_root_of_unity_mixed(N)
    got = g.check()[0][0]
    for i0 in (0, 201, t, M - 1):
        for c in range(3):
            i = i0 + c * M
            assert np.array_equal(got[i], orc.fr_horner(x, fr_pow(orc, w, i))), (i0, c)


def test_ntt_fr_mixed_combine_second_trip_round_trip(ctx, orc, mixed21):
    """IFFT(FFT(x)) == x bit for bit: the inverse combine with its constant post-scale, every index of the second trip included."""
    import torch
    x, g, io = mixed21
    N = 3 << 21
    g2 = G()
    back = g2.out(1, N, name="data")
    back.view().copy_(io.view())
    run(ctx, ctx.ntt_fr_mixed, back.ptr, N, IFFT, lanes=1, in_len=N, mem=DEVICE)
    back.check()
    want = torch.from_numpy(x.view(np.int64)).cuda()
    same = (back.view()[0] == want).all(dim=1)
    assert bool(same.all()), f"{int((~same).sum())} elements differ, first at {int(torch.nonzero(~same)[0])}"


def test_witness_map_pre_post(ctx, orc):
    log_d, lanes = 9, 3
    D = 1 << log_d
    a_len, b_len = D - 2, D - 4
    a, b, c, ab = (fr(560 + i, lanes * D).reshape(lanes, D, 4) for i in range(4))
    g = G()
    ga, gb = g.out(lanes, D, name="a"), g.out(lanes, D, name="b")
    _fill(ga, a, a_len)
    _fill(gb, b, b_len)
    run(ctx, ctx.witness_map_pre, ga.ptr, gb.ptr, log_d, lanes, a_len=a_len, b_len=b_len)
    got_a, got_b = g.check()
    a[:, a_len:], b[:, b_len:], c[:, b_len:] = 0, 0, 0
    for l in range(lanes):
        wa, wb = orc.witness_map_pre(a[l], b[l], log_d)
        eq(got_a[l], wa, f"witness_map_pre a lane {l}")
        eq(got_b[l], wb, f"witness_map_pre b lane {l}")
    g = G()
    gab, gc = g.out(lanes, D, name="ab"), g.out(lanes, D, name="c")
    _fill(gab, ab, D)
    _fill(gc, c, b_len)
    run(ctx, ctx.witness_map_post, gab.ptr, gc.ptr, log_d, lanes, c_len=b_len)
    got_ab, _ = g.check()
    for l in range(lanes):
        eq(got_ab[l], orc.witness_map_post(ab[l], c[l], log_d), f"witness_map_post lane {l}")


# ------------------------------------------------------------------------------------------------ group-side device outputs (blocks of 128)
GROUP_SIZES = [1, 127, 128, 129]


@pytest.fixture(scope="module")
def points(ctx):
    """per group: 129 subgroup points, a second set, infinity flags for both, canonical scalars with edge values"""
    out = {}
    for group in (1, 2):
        a = ctx.fixed_base_points(group, rand_fr_canonical(600 + group, 129))
        b = ctx.fixed_base_points(group, rand_fr_canonical(610 + group, 129))
        b[5] = a[5]                                                 # a doubling
        a_inf, b_inf = np.zeros(129, dtype=np.uint8), np.zeros(129, dtype=np.uint8)
        a_inf[[0, 100]] = 1
        b_inf[[0, 7, 128]] = 1
        k = rand_fr_canonical(620 + group, 129)
        k[:4] = EDGE
        out[group] = (a, a_inf, b, b_inf, k)
    return out


def _same_as_host(got, host, what):
    for x, y, nm in zip(got, host, what):
        assert np.array_equal(np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)), nm


@pytest.mark.parametrize("n", GROUP_SIZES)
@pytest.mark.parametrize("group", [1, 2])
def test_points_add(ctx, points, group, n):
    a, a_inf, b, b_inf, _ = (x[:n] for x in points[group])
    aw = 12 * group
    for negate in (False, True):
        g = G()
        f = [g.freeze(x, nm) for x, nm in ((a, "a"), (a_inf, "a_inf"), (b, "b"), (b_inf, "b_inf"))]
        out, oinf = g.out(1, n, words=aw, name="out"), g.bytes(n, "out_inf")
        run(ctx, ctx.points_add, group, f[0].ptr, f[2].ptr, a_inf=f[1].ptr, b_inf=f[3].ptr, negate_b=negate, n=n, out=out.ptr, out_inf=oinf.ptr, mem=DEVICE)
        _same_as_host(g.check(), ctx.points_add(group, a, b, a_inf=a_inf, b_inf=b_inf, negate_b=negate), ("out", "out_inf"))


@pytest.mark.parametrize("n", GROUP_SIZES)
@pytest.mark.parametrize("stride", [0, 1])
@pytest.mark.parametrize("group", [1, 2])
def test_points_mul(ctx, points, group, stride, n):
    a, a_inf, _, _, k = points[group]
    pts, inf, k = (a[:n], a_inf[:n], k[:n]) if stride else (a[1:2], a_inf[1:2], k[:n])
    g = G()
    fp, fi, fk = g.freeze(pts, "pts"), g.freeze(inf, "inf"), g.freeze(k, "scalars")
    out, oinf = g.out(1, n, words=12 * group, name="out"), g.bytes(n, "out_inf")
    run(ctx, ctx.points_mul, group, fp.ptr, fk.ptr, inf=fi.ptr, stride=stride, n=n, out=out.ptr, out_inf=oinf.ptr, mem=DEVICE)
    _same_as_host(g.check(), ctx.points_mul(group, pts, k, inf=inf, stride=stride), ("out", "out_inf"))


@pytest.mark.parametrize("n", GROUP_SIZES)
@pytest.mark.parametrize("group", [1, 2])
def test_points_sum(ctx, points, group, n):
    """Three ragged segments, one of them empty."""
    a, a_inf = points[group][0][:n], points[group][1][:n]
    offsets = [0, n // 3, n // 3, n]
    g = G()
    fp, fi = g.freeze(a, "pts"), g.freeze(a_inf, "inf")
    out, oinf = g.out(1, 3, words=12 * group, name="out"), g.bytes(3, "out_inf")
    run(ctx, ctx.points_sum, group, fp.ptr, offsets, inf=fi.ptr, out=out.ptr, out_inf=oinf.ptr, mem=DEVICE)
    host = ctx.points_sum(group, a, offsets, inf=a_inf)
    assert host[1][1] == 1                                          # the empty segment is infinity
    _same_as_host(g.check(), host, ("out", "out_inf"))


@pytest.mark.parametrize("n", GROUP_SIZES)
@pytest.mark.parametrize("group", [1, 2])
def test_fixed_base_msm(ctx, points, group, n):
    a, _, _, _, k = points[group]
    fb = ctx.fixed_base(group, a[1], n_hint=n)
    try:
        g = G()
        fk = g.freeze(k[:n], "scalars")
        out, oinf = g.out(1, n, words=12 * group, name="out"), g.bytes(n, "out_inf")
        run(ctx, ctx.fixed_base_msm, fb, fk.ptr, out=out.ptr, n=n, mem=DEVICE, out_inf=oinf.ptr)
        host = ctx.fixed_base_msm(fb, k[:n])
        assert host[1][0] == 1                                      # the zero scalar: infinity
        _same_as_host(g.check(), host, ("out", "out_inf"))
    finally:
        fb.release()


@pytest.mark.parametrize("n", GROUP_SIZES)
@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("group", [1, 2])
def test_points_serialize(ctx, points, group, compressed, n):
    a, a_inf = points[group][0][:n], points[group][1][:n]
    size = 12 * group * (4 if compressed else 8)
    g = G()
    fp, fi = g.freeze(a, "pts"), g.freeze(a_inf, "inf")
    out = g.bytes(n * size, "out_bytes")
    run(ctx, ctx.points_serialize, group, fp.ptr, inf=fi.ptr, compressed=compressed, n=n, out=out.ptr, mem=DEVICE)
    _same_as_host(g.check(), [ctx.points_serialize(group, a, inf=a_inf, compressed=compressed)], ("out_bytes",))


@pytest.mark.parametrize("n", GROUP_SIZES)
@pytest.mark.parametrize("compressed", [True, False])
@pytest.mark.parametrize("group", [1, 2])
def test_points_deserialize(ctx, points, group, compressed, n):
    """Checked decoding of valid encodings with one damaged in the last place (a status other than OK must land in its own byte)."""
    a, a_inf = points[group][0][:n], points[group][1][:n]
    data = ctx.points_serialize(group, a, inf=a_inf, compressed=compressed).copy()
    data[-1] ^= 0x3f if not compressed else 0x20
    g = G()
    fd = g.freeze(data, "bytes")
    out, oinf, ost = g.out(1, n, words=12 * group, name="out_pts"), g.bytes(n, "out_inf"), g.bytes(n, "out_status")
    dev = run(ctx, ctx.points_deserialize, group, fd.ptr, n=n, compressed=compressed, checked=True, out=out.ptr, out_inf=oinf.ptr, out_status=ost.ptr, mem=DEVICE)
    host = ctx.points_deserialize(group, data, compressed=compressed, checked=True)
    _same_as_host(g.check(), host[:3], ("out_pts", "out_inf", "out_status"))
    assert dev[3:] == host[3:]


@pytest.mark.parametrize("n", GROUP_SIZES)
@pytest.mark.parametrize("group", [1, 2])
def test_jac_to_affine(ctx, orc, points, group, n):
    """czk_jac_to_affine takes HOST memory only: the guards are host buffers here."""
    a = points[group][0][:n]
    jac = np.zeros((n, 18 * group), dtype=np.uint64)
    fq_one = orc.fq_from_repr(np.array([[1, 0, 0, 0, 0, 0]], dtype=np.uint64))[0]
    for i in range(n):
        p = np.zeros(18 * group, dtype=np.uint64)
        p[:12 * group] = a[i]
        p[12 * group:12 * group + 6] = fq_one
        jac[i] = orc.jac_double(group, p)                           # a z other than one
    if n > 2:
        jac[2, 12 * group:] = 0                                     # z = 0: infinity
    g = Guards("cpu")
    fj = g.freeze(jac, "jac")
    out, oinf = g.out(1, n, words=12 * group, name="out_aff"), g.bytes(n, "out_inf")
    ctx._ck(ctx._L.czk_jac_to_affine(ctx._h, C.c_int(group), C.c_void_p(fj.ptr), C.c_size_t(n), C.c_void_p(out.ptr), C.c_void_p(oinf.ptr)))
    _same_as_host(g.check(), ctx.jac_to_affine(group, jac), ("out_aff", "out_inf"))
