"""The twisted Edwards bucket reduction without its neutral additions and with the shared 2 D T product (context option
"msm_reduce_lean", a bit set: 1 = the running sums start from the chunk's entries instead of the neutral element, 2 = one 2 D T product
serves both additions a running sum takes part in; 0 = the kernels of before, which stay in the library).  Every result is compared in
affine with the checker's AffineCurve::multi_scalar_mul, under option values 0, 1 and 3.

The window is forced as tests/test_gpu_parity.py test_msm_partition_scatter_widths does it ("msm_window_g1", "msm_fixed_c", one workspace
slot); a key of window c has B = 2^(c-1) buckets, the level kernel shrinks a bucket set by 8 while it has more than 1 024 entries, and the
tail kernels finish.  B is a power of two on every path of the library, so a chunk of the level kernel is never clipped (end - start is
always 8) and its clipped-chunk branch cannot be reached from here: it is kept right by construction (msm_acc.h)."""
import numpy as np
import pytest

from util import ints_to_limbs, rand_fr_canonical, R_MOD

pytestmark = pytest.mark.gpu

LEAN = (0, 1, 3)


@pytest.fixture(scope="module")
def czk():
    import czk_amd
    return czk_amd


@pytest.fixture(scope="module")
def ctxs(czk):
    """One context per window width, made on demand: "msm_window_g1" applies to the keys registered afterwards."""
    made = {}

    def get(c):
        if c not in made:
            made[c] = czk.Context(0, options={"msm_slots": 1, "msm_window_g1": c, "msm_fixed_c": 1})
        return made[c]
    yield get
    for c2 in made.values():
        c2.close()


@pytest.fixture(scope="module")
def points(czk, orc):
    """5 000 G1 points, computed once and shared (read only)."""
    c2 = czk.Context(0)
    p = c2.fixed_base_points(1, rand_fr_canonical(0x1EA0, 5000))
    c2.close()
    return p


def _same_point(ctx, orc, g, have_jac, want_jac):
    want_aff, want_inf = orc.jac_to_affine(g, want_jac)
    have_aff, have_inf = ctx.jac_to_affine(g, have_jac)
    chk_aff, chk_inf = orc.jac_to_affine(g, have_jac)     # product's own to-affine agrees with the checker's
    assert chk_inf == bool(have_inf[0]) and (chk_inf or np.array_equal(chk_aff, have_aff[0]))
    return bool(have_inf[0]) == want_inf and (want_inf or np.array_equal(have_aff[0], want_aff))


def _check(ctx, orc, b, g, bases, inf, sc, lanes, tag, opts=LEAN):
    """sc: (lanes, n, 4) canonical scalars; the MSM under every option value against the checker (computed once)."""
    want = [orc.multi_scalar_mul(g, bases, inf, orc.fr_from_repr(sc[ln])) for ln in range(lanes)]
    got = {}
    for opt in opts:
        ctx.set_option("msm_reduce_lean", opt)
        got[opt] = ctx.msm(b, sc, lanes=lanes)
        for ln in range(lanes):
            assert _same_point(ctx, orc, g, got[opt][ln], want[ln]), (tag, "msm_reduce_lean", opt, "lane", ln)
    ctx.set_option("msm_reduce_lean", 3)
    return got


@pytest.mark.parametrize("n,lanes", [(300, 1), (5000, 1), (5000, 3), (5000, 4)])
@pytest.mark.parametrize("c", [8, 11, 12, 14, 15])
def test_level_shapes(ctxs, orc, points, c, n, lanes):
    """c = 8: 128 buckets, tail only; 11: 1 024, the tail at its limit; 12: 2 048 -> 256, one level; 14: 8 192 -> 1 024; 15: 16 384 -> 2 048 -> 256,
    two levels (the second one reads E_in).  n = 300 leaves most buckets neutral from c = 11 on; n = 5 000 fills them at c <= 12.  A base at
    infinity and a zero scalar ride along."""
    ctx = ctxs(c)
    bases = np.ascontiguousarray(points[:n])
    inf = np.zeros(n, dtype=np.uint8)
    inf[[3, n - 50]] = 1
    sc = rand_fr_canonical(0x1EA1 + 16 * c + lanes, lanes * n).reshape(lanes, n, 4)
    sc[:, 7] = 0
    b = ctx.register_bases(1, bases, inf)
    assert b.layout_for(n)[0] == c
    _check(ctx, orc, b, 1, bases, inf, sc, lanes, (c, n, lanes))
    b.release()


def _small(vals):
    return ints_to_limbs([int(v) % R_MOD for v in vals], 4)


# c = 12: B = 2 048 buckets, 256 chunks of 8; a scalar s in [1, B] is the single digit s and lands in bucket s - 1, 2^c - s puts the negated point there
# (and its carry into bucket 0), r - s is the negated group element.  Buckets by name:
AIMED = {
    "first entry of a chunk (no A addition)": [800],
    "last entry of a chunk (running starts here)": [807],
    "bucket 0": [0],
    "bucket B - 1": [2047],
    "only the last entry of a chunk": [1039],
    "only the first entry of a chunk": [1032],
    "first and last entry of one chunk": [1200, 1207],
    "a full chunk and its neighbours' edges": list(range(1599, 1609)),
    "the last chunk": list(range(2040, 2048)),
    "the first chunk": list(range(0, 8)),
}


@pytest.mark.parametrize("name", list(AIMED))
def test_aimed_buckets(ctxs, orc, points, name):
    """Single points placed at the entries of a level-0 chunk that the lean kernel treats on their own: lane 0 positive digits, lane 1 the negated
    entries (2^c - s), lane 2 the scalars r - s."""
    c, ctx = 12, ctxs(12)
    bk = AIMED[name]
    n = len(bk)
    bases = np.ascontiguousarray(points[100:100 + n])
    inf = np.zeros(n, dtype=np.uint8)
    sc = np.stack([_small([b + 1 for b in bk]), _small([(1 << c) - (b + 1) for b in bk]), _small([R_MOD - (b + 1) for b in bk])])
    b = ctx.register_bases(1, bases, inf)
    assert b.layout_for(n)[0] == c
    _check(ctx, orc, b, 1, bases, inf, sc, 3, name)
    b.release()


@pytest.mark.parametrize("c", [8, 12, 15])
def test_all_neutral_and_one_point(ctxs, orc, points, c):
    """Every scalar zero: every bucket neutral, the result is infinity.  One point alone: n = 1."""
    ctx = ctxs(c)
    n = 40
    bases = np.ascontiguousarray(points[:n])
    inf = np.zeros(n, dtype=np.uint8)
    b = ctx.register_bases(1, bases, inf)
    got = _check(ctx, orc, b, 1, bases, inf, np.zeros((2, n, 4), dtype=np.uint64), 2, ("zero", c))
    for opt in LEAN:
        assert ctx.jac_to_affine(1, got[opt][0])[1][0] == 1
    b.release()
    one = np.ascontiguousarray(points[7:8])
    b = ctx.register_bases(1, one, np.zeros(1, dtype=np.uint8))
    _check(ctx, orc, b, 1, one, np.zeros(1, dtype=np.uint8), rand_fr_canonical(0x1EA2 + c, 2).reshape(2, 1, 4), 2, ("one point", c))
    b.release()


@pytest.mark.parametrize("g,no_tables", [(2, False), (1, True)])
def test_untouched_paths_same_under_every_option(czk, orc, points, g, no_tables):
    """The G2 reduction (Xyzz2Ops) and the table-free G1 reduction (XyzzOps) carry an infinity flag and have no lean form: options 0 and 3
    give the same point, and the right one."""
    ctx = czk.Context(0, options={"msm_slots": 1})
    n = 3000 if g == 1 else 1200
    bases = np.ascontiguousarray(points[:n]) if g == 1 else ctx.fixed_base_points(2, rand_fr_canonical(0x1EA3, n))
    inf = np.zeros(n, dtype=np.uint8)
    inf[5] = 1
    sc = rand_fr_canonical(0x1EA4 + g, 2 * n).reshape(2, n, 4)
    b = ctx.register_bases(g, bases, inf, mem=czk.CZK_MEM_HOST | (czk.CZK_MEM_NO_TABLES if no_tables else 0))
    got = _check(ctx, orc, b, g, bases, inf, sc, 2, (g, no_tables), opts=(0, 3))
    for ln in range(2):   # (in affine: the entries of a bucket are added in the order the sort's atomics left them, so the Jacobian triple varies from call to call)
        a0, a3 = ctx.jac_to_affine(g, got[0][ln]), ctx.jac_to_affine(g, got[3][ln])
        assert a0[1][0] == a3[1][0] == 0 and np.array_equal(a0[0], a3[0]), (g, no_tables, ln)
    b.release()
    ctx.close()


def test_option_range(czk):
    ctx = czk.Context(0)
    for v in (0, 1, 2, 3):
        ctx.set_option("msm_reduce_lean", v)
    for v in (-1, 4):
        with pytest.raises(czk.CzkError):
            ctx.set_option("msm_reduce_lean", v)
    ctx.close()
