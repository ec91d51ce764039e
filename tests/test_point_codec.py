"""czk_fq_sqrt, czk_points_serialize and czk_points_deserialize on the GPU against the big-integer model (tests/point_codec_ref.py).
Every comparison is bit for bit: roots normalised by the library's rule (y <= -y), bytes, points, infinity flags, statuses and the two counts."""
import numpy as np
import pytest

import point_codec_ref as M
from pyref import INF, Q_MOD, R_MOD, ec_mul, ec_neg, splitmix64

pytestmark = pytest.mark.gpu
Q = Q_MOD
SIZES = (0, 1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


def _rand_fq(seed, n):
    out, st = [], seed
    while len(out) < n:
        v = 0
        for i in range(6):
            st, z = splitmix64(st)
            v |= z << (64 * i)
        v &= (1 << 377) - 1
        if v < Q:
            out.append(v)
    return out


# ----------------------------------------------------------------------------- square roots
def _fq_inputs():
    g, z = M.FQ_GENERATOR, M.FQ_TWO_ADIC_ROOT
    vals = [0, 1, 4, Q - 1, Q - 5]
    vals += [pow(g, 2 * j, Q) for j in (1, 3, 5, 7)]                  # a^t of maximal order 2^45: the reference loop's worst case
    cs = _rand_fq(0xC0DE, 60)
    vals += [pow(c, 1 << 46, Q) for c in cs[:6]]                       # a^t = 1: no correction
    # one input for every 2-adic order of a^t, 2^0 .. 2^45, residues; and the same with order 2^46 and a few more non-residues
    for i in range(46):
        v = pow(z, 1 << i, Q) * pow(cs[6 + i], 1 << 46, Q) % Q        # a^t = z^(2^i t'), of order 2^(46 - i)
        vals.append(v if i > 0 else v * v % Q)                         # i = 0 is a non-residue: its square has order 2^45
    vals += [z * pow(cs[52], 1 << 46, Q) % Q, pow(z, 3, Q), pow(z, (1 << 40) + 1, Q)]   # odd logarithms: non-residues
    vals += _rand_fq(0x5EED, 257 - len(vals))
    assert len(vals) == 257
    return vals


def _fq2_inputs():
    a, b = _rand_fq(0xF2A, 257), _rand_fq(0xF2B, 257)
    vals = [(0, 0), (1, 0), (4, 0), (Q - 1, 0), (Q - 5, 0), (7, 0), (11, 0), (0, 1), (0, 5), (0, Q - 3), (0, a[0])]   # c1 = 0 and c0 = 0
    vals += [(a[i], 0) for i in range(1, 9)] + [(0, b[i]) for i in range(1, 9)]
    # norm a residue of Fq but the element no square: impossible (a is a square iff its norm is), so the class is empty -- the nearest
    # cases are elements of Fq that are non-residues there, which ARE squares in Fq2
    vals += [(v, 0) for v in _rand_fq(0xF2C, 12) if pow(v, (Q - 1) // 2, Q) == Q - 1]
    vals += [M.FIELD[2].mul(v, v) for v in zip(a[20:40], b[20:40])]    # squares
    vals += list(zip(a[40:], b[40:]))
    return vals[:257]


FQ_IN = {1: _fq_inputs(), 2: _fq2_inputs()}


@pytest.fixture(scope="module")
def sqrt_want():
    """{ext: (roots (257, 6|12), exists (257,))} from the model, computed once"""
    out = {}
    for ext in (1, 2):
        res = [M.f_sqrt(ext, a) for a in FQ_IN[ext]]
        roots = np.array([M.f_mont_limbs(ext, r) for _, r in res], dtype=np.uint64)
        exists = np.array([ok for ok, _ in res], dtype=np.uint8)
        assert 40 < int(exists.sum()) < 230                            # both classes occur
        roots.setflags(write=False)
        exists.setflags(write=False)
        out[ext] = (roots, exists)
    return out


@pytest.mark.parametrize("ext", (1, 2))
@pytest.mark.parametrize("n", SIZES)
def test_fq_sqrt(ctx, sqrt_want, ext, n):
    a = np.array([M.f_mont_limbs(ext, v) for v in FQ_IN[ext][:n]], dtype=np.uint64).reshape(n, 6 * ext)
    got, exists = ctx.fq_sqrt(a, ext)
    assert got.shape == (n, 6 * ext) and np.array_equal(exists, sqrt_want[ext][1][:n])
    assert np.array_equal(got, sqrt_want[ext][0][:n])


def test_fq_sqrt_device_memory(ctx, sqrt_want):
    import torch
    import czk_amd
    for ext in (1, 2):
        n = 257
        a = np.array([M.f_mont_limbs(ext, v) for v in FQ_IN[ext]], dtype=np.uint64)
        ad = torch.from_numpy(a.view(np.int64)).to("cuda:0")
        out = torch.full((n, 6 * ext), -1, dtype=torch.int64, device="cuda:0")
        ex = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
        ctx.fq_sqrt(ad.data_ptr(), ext, out=out.data_ptr(), out_exists=ex.data_ptr(), n=n, mem=czk_amd.CZK_MEM_DEVICE)
        ctx.sync()
        assert np.array_equal(out.cpu().numpy().view(np.uint64), sqrt_want[ext][0]) and np.array_equal(ex.cpu().numpy(), sqrt_want[ext][1])


# ----------------------------------------------------------------------------- points
def _scalars():
    st, ks = 0xEC0DE, list(range(1, 33))
    while len(ks) < 60:
        st, z0 = splitmix64(st)
        st, z1 = splitmix64(st)
        st, z2 = splitmix64(st)
        st, z3 = splitmix64(st)
        ks.append((z0 | z1 << 64 | z2 << 128 | z3 << 192) % R_MOD)
    return ks


def _top_bits_set(group, P):
    """y's top canonical bits are set: y (its c1 for G2) is at least 2^376"""
    y = P[1] if group == 1 else P[1][1]
    return y >> 376 == 1


@pytest.fixture(scope="module")
def good_points():
    """{group: [points]}: [k] G for k = 1 .. 32 and random k, their negatives where that sets y's top bits, infinity first, last and inside"""
    out = {}
    for group in (1, 2):
        F = M.FIELD[group]
        pts = [ec_mul(F, k, M.GEN[group]) for k in _scalars()]
        pts += [ec_neg(F, P) for P in pts[:12]]
        assert sum(_top_bits_set(group, P) for P in pts) >= 3
        pts = [INF] + pts[:30] + [INF] + pts[30:] + [INF]
        out[group] = pts
    return out


@pytest.fixture(scope="module")
def good_bytes(good_points):
    return {(g, c): M.encode_points(g, good_points[g], c) for g in (1, 2) for c in (True, False)}


@pytest.mark.parametrize("group", (1, 2))
@pytest.mark.parametrize("compressed", (True, False))
def test_encode(ctx, good_points, good_bytes, group, compressed):
    import torch
    import czk_amd
    pts, inf = M.points_to_arrays(group, good_points[group])
    want = good_bytes[group, compressed]
    assert ctx.points_serialize(group, pts, inf, compressed).tobytes() == want
    # an infinite point is written as zero() whatever its coordinates hold
    junk = pts.copy()
    junk[inf == 1] = pts[1]
    assert ctx.points_serialize(group, junk, inf, compressed).tobytes() == want
    # no flags = none infinite
    fin = inf == 0
    assert ctx.points_serialize(group, pts[fin], None, compressed).tobytes() == M.encode_points(group, [P for P in good_points[group] if P is not INF], compressed)
    assert ctx.points_serialize(group, pts[:0], None, compressed).size == 0
    # device memory
    n = pts.shape[0]
    pd = torch.from_numpy(pts.view(np.int64)).to("cuda:0")
    fd = torch.from_numpy(inf).to("cuda:0")
    out = torch.zeros(len(want), dtype=torch.uint8, device="cuda:0")
    ctx.points_serialize(group, pd.data_ptr(), fd.data_ptr(), compressed, n=n, out=out.data_ptr(), mem=czk_amd.CZK_MEM_DEVICE)
    ctx.sync()
    assert out.cpu().numpy().tobytes() == want
    with pytest.raises(czk_amd.CzkError):   # device byte buffers are 8-byte aligned
        ctx.points_serialize(group, pd.data_ptr(), fd.data_ptr(), compressed, n=n - 1, out=out.data_ptr() + 4, mem=czk_amd.CZK_MEM_DEVICE)


def _fq_bytes(v, flags=0):
    return (v | flags << 376).to_bytes(48, "little")


def _bad_cases(group, compressed, gen):
    """byte strings of single points that exercise every status; `gen` = the generator (model form)"""
    cases = []
    if compressed:
        if group == 1:
            cases += [_fq_bytes(0), _fq_bytes(0, 0x80)]                          # (0, +-1): on the curve, not in the subgroup
            cases += [_fq_bytes(Q - 1), _fq_bytes(Q - 1, 0x80)]                  # the 2-torsion point (-1, 0)
            cases += [_fq_bytes(x, s) for x in (4, 7, 9, 10, 11) for s in (0, 0x80)]   # x^3 + 1 is a non-residue
            cases += [_fq_bytes(5, 0xC0), _fq_bytes(0, 0xC0)]                    # both flag bits
            cases += [_fq_bytes(0, 0x40), _fq_bytes(12345, 0x40)]                # infinity, with and without x = 0
            cases += [Q.to_bytes(48, "little"), ((1 << 377) - 1).to_bytes(48, "little")]   # not canonical
        else:
            cases += [_fq_bytes(0) + _fq_bytes(0), _fq_bytes(0) + _fq_bytes(0, 0x80)]
            cases += [_fq_bytes(a) + _fq_bytes(b, s) for a in range(6) for b in range(3) for s in (0, 0x80)]   # small x: a mix of NO_POINT and off-subgroup points
            cases += [_fq_bytes(5) + _fq_bytes(1, 0xC0)]
            cases += [_fq_bytes(0) + _fq_bytes(0, 0x40), _fq_bytes(77) + _fq_bytes(3, 0x40)]
            cases += [_fq_bytes(1) + Q.to_bytes(48, "little"), Q.to_bytes(48, "little") + _fq_bytes(1), _fq_bytes(1) + ((1 << 377) - 1).to_bytes(48, "little")]
            cases += [_fq_bytes(gen[0][0], 0x80) + _fq_bytes(gen[0][1]), _fq_bytes(gen[0][0], 0x40) + _fq_bytes(gen[0][1])]   # a flag bit on c0
    else:
        F = M.FIELD[group]
        enc = lambda x, y, fl=0, flx=0: M._f_bytes(group, x, flx) + M._f_bytes(group, y, fl)   # noqa: E731
        x, y = gen
        y_off = F.add(y, F.one)
        cases += [enc(x, y_off), enc(x, y, 0x80), enc(x, y_off, 0x80)]           # off the curve; bit 7 is ignored
        cases += [enc(x, y, 0xC0), enc(x, y, 0x40), enc(F.zero, F.one, 0x40)]    # both bits; infinity with and without zero()'s coordinates
        cases += [enc(x, y, 0, 0x80), enc(x, y, 0, 0x40)]                        # flag bits on x: not canonical
        if group == 1:
            cases += [enc(0, 1), enc(0, Q - 1), enc(Q - 1, 0)]                   # on the curve, outside the subgroup
            cases += [Q.to_bytes(48, "little") + _fq_bytes(1), _fq_bytes(1) + Q.to_bytes(48, "little")]
        else:
            cases += [_fq_bytes(x[0], 0x80) + _fq_bytes(x[1]) + M._f_bytes(2, y), M._f_bytes(2, x) + _fq_bytes(y[0], 0x40) + _fq_bytes(y[1])]
            cases += [M._f_bytes(2, x) + Q.to_bytes(48, "little") + _fq_bytes(y[1])]
            small = [(a, b) for a in range(6) for b in range(3)]               # curve points with a small x: outside the subgroup
            roots = [(v, M.f_sqrt(2, F.add(F.mul(v, F.mul(v, v)), M.CURVE_B[2]))) for v in small]
            cases += [enc(v, r) for v, (ok, r) in roots if ok][:3]
    return cases


@pytest.fixture(scope="module")
def decode_cases(good_points, good_bytes):
    """{(group, compressed): (bytes, {checked: (statuses, points, bad, first)})}: the good points with the special cases spliced in between them"""
    out = {}
    for group in (1, 2):
        for compressed in (True, False):
            size = M.point_size(group, compressed)
            good = good_bytes[group, compressed]
            good = [good[i:i + size] for i in range(0, len(good), size)]
            cases = _bad_cases(group, compressed, M.GEN[group])
            seq, gi = good[:5], 5
            for c in cases:                     # two good points between neighbours
                seq += [c] + good[gi:gi + 2]
                gi += 2
            seq += good[gi:]
            data = b"".join(seq)
            if group == 2:
                # the model's G2 subgroup test ([r] P with Python integers) is slow: the good points are known members
                want = {}
                for checked in (False, True):
                    res = []
                    for s in seq:
                        if s in good and checked:
                            st, P = M.decode_point(group, s, compressed, False)
                        else:
                            st, P = M.decode_point(group, s, compressed, checked)
                        res.append((st, P))
                    bad = [i for i, r in enumerate(res) if r[0] != M.OK]
                    want[checked] = ([r[0] for r in res], [r[1] for r in res], len(bad), bad[0] if bad else len(res))
            else:
                want = {checked: M.decode_points(group, data, compressed, checked) for checked in (False, True)}
            out[group, compressed] = (data, want)
    return out


@pytest.mark.parametrize("group", (1, 2))
@pytest.mark.parametrize("compressed", (True, False))
@pytest.mark.parametrize("checked", (True, False))
def test_decode(ctx, decode_cases, group, compressed, checked):
    data, want = decode_cases[group, compressed]
    st, pts, bad, first = want[checked]
    wpts, winf = M.points_to_arrays(group, pts)
    got, inf, status, n_bad, n_first = ctx.points_deserialize(group, data, compressed=compressed, checked=checked)
    assert list(status) == st
    assert (n_bad, n_first) == (bad, first) and bad > 0
    assert np.array_equal(inf, winf) and np.array_equal(got, wpts)
    seen = set(st)
    if compressed:
        assert {M.BAD_FLAGS, M.NOT_CANONICAL, M.NO_POINT} <= seen and ((M.NOT_IN_SUBGROUP in seen) == checked)
    else:
        assert {M.BAD_FLAGS, M.NOT_CANONICAL} <= seen and ((M.NOT_ON_CURVE in seen) == checked) and ((M.NOT_IN_SUBGROUP in seen) == checked)
    # the good points alone: nothing fails, the first bad index is n
    n_good = 5
    size = M.point_size(group, compressed)
    got, inf, status, n_bad, n_first = ctx.points_deserialize(group, data[:n_good * size], compressed=compressed, checked=checked)
    assert (n_bad, n_first) == (0, n_good) and not status.any() and np.array_equal(got, wpts[:n_good]) and np.array_equal(inf, winf[:n_good])
    assert ctx.points_deserialize(group, b"", compressed=compressed, checked=checked)[3:] == (0, 0)


@pytest.mark.parametrize("group", (1, 2))
def test_decode_device_memory(ctx, decode_cases, group):
    import torch
    import czk_amd
    data, want = decode_cases[group, True]
    st, pts, bad, first = want[True]
    n = len(st)
    wpts, winf = M.points_to_arrays(group, pts)
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0")
    out = torch.full((n, 12 * group), -1, dtype=torch.int64, device="cuda:0")
    inf = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    status = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    res = ctx.points_deserialize(group, src.data_ptr(), n, True, True, out=out.data_ptr(), out_inf=inf.data_ptr(), out_status=status.data_ptr(),
                                 mem=czk_amd.CZK_MEM_DEVICE)
    assert res[3:] == (bad, first)
    assert list(status.cpu().numpy()) == st and np.array_equal(inf.cpu().numpy(), winf) and np.array_equal(out.cpu().numpy().view(np.uint64), wpts)
    # enqueue only: no status array, no counts
    out.fill_(-1)
    res = ctx.points_deserialize(group, src.data_ptr(), n, True, True, out=out.data_ptr(), out_inf=inf.data_ptr(), count=False, mem=czk_amd.CZK_MEM_DEVICE)
    assert res[3:] == (None, None)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), wpts)
    with pytest.raises(czk_amd.CzkError):
        ctx.points_deserialize(group, src.data_ptr() + 4, n - 1, True, True, out=out.data_ptr(), out_inf=inf.data_ptr(), mem=czk_amd.CZK_MEM_DEVICE)


@pytest.mark.parametrize("group", (1, 2))
@pytest.mark.parametrize("compressed", (True, False))
def test_round_trip_through_device_memory(ctx, group, compressed):
    """deserialize(serialize(P)) == P for 1000 points, checked, with no host copy in between"""
    import torch
    import czk_amd
    from util import rand_fr_canonical
    n, aw = 1000, 12 * group
    k = rand_fr_canonical(0x707 + group, n)
    k[17] = 0
    k[999] = 0
    pts = torch.from_numpy(ctx.fixed_base_points(group, k).view(np.int64)).to("cuda:0")
    inf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    inf[17] = 1
    inf[999] = 1
    pts[17] = torch.from_numpy(M.points_to_arrays(group, [INF])[0].view(np.int64))[0]
    pts[999] = pts[17]
    data = torch.zeros(n * M.point_size(group, compressed), dtype=torch.uint8, device="cuda:0")
    back = torch.full((n, aw), -1, dtype=torch.int64, device="cuda:0")
    binf = torch.full((n,), 9, dtype=torch.uint8, device="cuda:0")
    dev = czk_amd.CZK_MEM_DEVICE
    ctx.points_serialize(group, pts.data_ptr(), inf.data_ptr(), compressed, n=n, out=data.data_ptr(), mem=dev)
    res = ctx.points_deserialize(group, data.data_ptr(), n, compressed, True, out=back.data_ptr(), out_inf=binf.data_ptr(), mem=dev)
    assert res[3:] == (0, n)
    assert torch.equal(back, pts) and torch.equal(binf, inf)
