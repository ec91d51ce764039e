"""czk_fr_merkle_commit / _open / _verify, czk_fr_fri_fold and czk_amd.fri on the GPU against tests/merkle_fri_model.py (hashlib and big integers, written
from com.rs and client.rs): every comparison is for exact equality, there are no tolerances.

1. commit: the whole tree, not only the root -- sizes either side of every launch seam of the fused form (S = MERKLE_SUBTREE_LOG, read from the source;
   that form is the lab library's, the shipped one launches per level) and
   of a 256-thread block, 1 and 3 lanes, strides with sentinel padding that must stay, host and device memory, the elements 0, 1 and r - 1 at index 0, at a
   subtree seam and at n - 1; the smallest lanes x n at which the grid-stride loop takes a second trip; the form kept in the lab library.
2. open / verify: every index, one block and more, n = 1, every kind of tampering, indices out of range, the error codes.
3. fold.  4. fri.commit_phase / query_phase / verify against the model, and two dishonest provers.
"""
import hashlib
import os
import re

import numpy as np
import pytest

import merkle_fri_model as M
from guarded import Guards, device_cus
from util import R_MOD, ints_to_limbs, limbs_to_ints, rand_fr_canonical

pytestmark = pytest.mark.gpu
RR = (1 << 256) % R_MOD
ERR_SIZE, ERR_ARG = 1, 3
FILL = 0xA5
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "collaborative-zksnark_amd", "csrc")
S = int(re.search(r"constexpr unsigned MERKLE_SUBTREE_LOG = (\d+);", open(os.path.join(CSRC, "lab", "merkle_tree_fused.h")).read()).group(1))
BLOCKS_PER_CU = int(re.search(r"constexpr unsigned MERKLE_BLOCKS_PER_CU = (\d+);", open(os.path.join(CSRC, "merkle_hash.h")).read()).group(1))


def mont(vals):
    return ints_to_limbs([v % R_MOD * RR % R_MOD for v in vals], 4).reshape(-1, 4)


def unmont(limbs):
    inv = pow(1 << 256, -1, R_MOD)
    return [v * inv % R_MOD for v in limbs_to_ints(np.asarray(limbs).reshape(-1, 4))]


@pytest.fixture(scope="module")
def gpu():
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    yield czk_amd, ctx
    ctx.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


_CASES = {}


def vector_case(orc, lanes, n):
    """(canonical limbs (lanes, n, 4), Montgomery limbs, the model's tree bytes per lane), made once per shape: random elements with 0, 1 and r - 1 at
    index 0, at a subtree seam (or the middle of a vector below one subtree) and at n - 1 of lane 0, 1 and 2 in turn"""
    if (lanes, n) not in _CASES:
        canon = rand_fr_canonical(7000 + 31 * lanes + n.bit_length(), lanes * n).reshape(lanes, n, 4)
        special = ints_to_limbs([0, 1, R_MOD - 1], 4).reshape(3, 4)
        seam = (1 << S) if n > (1 << S) else n // 2
        for ln in range(lanes):
            for j, at in enumerate((0, seam - 1 if seam else 0, seam, n - 1)):
                canon[ln, min(at, n - 1)] = special[(ln + j) % 3]
        mont_limbs = orc.fr_from_repr(canon.reshape(-1, 4)).reshape(lanes, n, 4)
        trees = [M.tree_bytes(M.tree_levels_of_bytes(canon[ln].tobytes())) for ln in range(lanes)]
        _CASES[(lanes, n)] = (canon, mont_limbs, trees)
    return _CASES[(lanes, n)]


def test_the_model_reads_elements_as_the_library_serializes_them(gpu, orc):
    czk, ctx = gpu
    canon, mont_limbs, _ = vector_case(orc, 1, 4)
    assert ctx.fr_vec_serialize(mont_limbs[0])[8:] == canon[0].tobytes() == b"".join(M.elem_bytes(v) for v in limbs_to_ints(canon[0]))
    assert unmont(mont_limbs[0]) == limbs_to_ints(canon[0])
    for log_d in (1, 4, 11):                                                         # ... and evaluates over the domains the library's transforms use
        assert unmont(ctx.domain_constants(log_d)["group_gen"]) == [M.root_of_unity(1 << log_d)] == [czk.fri.root_of_unity(1 << log_d)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. commit
# ---------------------------------------------------------------------------------------------------------------------------------------
SIZES = sorted({1, 2, 4, 1 << S, 1 << (S + 1), 1 << min(2 * S + 2, 16)})


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_commit_whole_tree_matches_the_model(gpu, orc, n, lanes, mem):
    czk, ctx = gpu
    _, a, trees = vector_case(orc, lanes, n)
    stride, tree_stride = n + 3, 2 * n - 1 + 5
    src = np.full((lanes, stride, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    src[:, :n] = a
    if mem == "host":
        tree = np.full((lanes, tree_stride, 32), FILL, dtype=np.uint8)
        got, roots = ctx.fr_merkle_commit(src, lanes=lanes, n=n, tree=tree)
        assert got is tree and (tree[:, 2 * n - 1:] == FILL).all()                       # the padding between the lanes is as it was
        got = tree[:, :2 * n - 1]
        dense, roots2 = ctx.fr_merkle_commit(a, lanes=lanes)                            # stride == n, tree_stride == 2n - 1: nothing uploaded first
        assert dense.shape == (lanes, 2 * n - 1, 32) and np.array_equal(dense, got) and np.array_equal(roots, roots2)
    else:
        G = Guards("cuda")
        d_a = G.freeze(src, "a")
        g_tree = G.out(lanes, 2 * n - 1, tree_stride, name="tree")
        _, roots = ctx.fr_merkle_commit(d_a.ptr, lanes=lanes, n=n, stride=stride, tree=g_tree.ptr, tree_stride=tree_stride, mem=czk.CZK_MEM_DEVICE)
        got = G.check()[0].view(np.uint8).reshape(lanes, 2 * n - 1, 32)                 # ... and nothing outside 2n - 1 digests per lane was written
        # enqueue-only form: no roots asked for
        g2 = G.out(lanes, 2 * n - 1, tree_stride, name="tree (no roots)")
        _, none = ctx.fr_merkle_commit(d_a.ptr, lanes=lanes, n=n, stride=stride, tree=g2.ptr, tree_stride=tree_stride, roots=False, mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        assert none is None and np.array_equal(G.check()[1].view(np.uint8).reshape(lanes, 2 * n - 1, 32), got)
    for ln in range(lanes):
        assert got[ln].tobytes() == trees[ln], (n, ln)
        assert roots[ln].tobytes() == trees[ln][-32:]


def test_commit_second_trip_of_the_grid_stride_loop(gpu, orc):
    """The smallest lanes x n (lanes <= 3) above one trip of the shipped kernels' loop: MERKLE_BLOCKS_PER_CU blocks of 256 threads per CU, a leaf per thread."""
    czk, ctx = gpu
    one_trip = BLOCKS_PER_CU * device_cus() * 256
    lanes, n = min(((ln, 1 << (one_trip // ln).bit_length()) for ln in (1, 2, 3)), key=lambda c: c[0] * c[1])
    assert lanes * n > one_trip and lanes * n <= 1 << 21
    _, a, trees = vector_case(orc, lanes, n)
    G = Guards("cuda")
    d_a = G.freeze(a, "a")
    g_tree = G.out(lanes, 2 * n - 1, name="tree")
    _, roots = ctx.fr_merkle_commit(d_a.ptr, lanes=lanes, n=n, stride=n, tree=g_tree.ptr, tree_stride=2 * n - 1, mem=czk.CZK_MEM_DEVICE)
    got = G.check()[0].view(np.uint8).reshape(lanes, -1)
    for ln in range(lanes):
        assert got[ln].tobytes() == trees[ln] and roots[ln].tobytes() == trees[ln][-32:]


@pytest.mark.parametrize("n", [1, 2, 1 << (S + 1)])
def test_commit_form_kept_in_the_lab_library_makes_the_same_tree(gpu, orc, n):
    czk, _ = gpu
    lanes = 3
    _, a, trees = vector_case(orc, lanes, n)
    lab = czk.Context(0, lab=True)
    try:
        G = Guards("cuda")
        d_a = G.freeze(a, "a")
        g_tree = G.out(lanes, 2 * n - 1, 2 * n + 1, name="tree")
        import torch
        torch.cuda.synchronize()
        lab.lab_merkle_commit(d_a.ptr, lanes, n, n, g_tree.ptr, 2 * n + 1)
        lab.sync()
        got = G.check()[0].view(np.uint8).reshape(lanes, -1)
        for ln in range(lanes):
            assert got[ln].tobytes() == trees[ln]
    finally:
        lab.close()


def test_commit_error_codes_and_empty_calls(gpu, orc):
    czk, ctx = gpu
    _, a, _ = vector_case(orc, 3, 1 << S)
    for n in (0, 3, (1 << S) - 1):
        with pytest.raises(czk.CzkError, match="power of two") as e:
            ctx.fr_merkle_commit(a[:, :max(n, 1)], lanes=3, n=n, tree=np.zeros((3, 2 * (1 << S), 32), dtype=np.uint8))
        assert e.value.code == ERR_SIZE
    G = Guards("cuda")
    d_a = G.freeze(a, "a")
    g_tree = G.out(3, 2 * (1 << S) - 1, name="tree")
    n = 1 << S
    for kw, msg in ((dict(stride=n - 1, tree_stride=2 * n - 1), "stride < n"), (dict(stride=n, tree_stride=2 * n - 2), "tree_stride < 2n - 1"),
                    (dict(stride=1 << 62, tree_stride=2 * n - 1), "overflows"), (dict(stride=n, tree_stride=1 << 62), "overflows")):
        with pytest.raises(czk.CzkError, match=msg) as e:
            ctx.fr_merkle_commit(d_a.ptr, lanes=3, n=n, tree=g_tree.ptr, mem=czk.CZK_MEM_DEVICE, **kw)
        assert e.value.code == ERR_SIZE
    with pytest.raises(czk.CzkError) as e:
        ctx.fr_merkle_commit(d_a.ptr, lanes=3, n=n, stride=n, tree=g_tree.ptr, tree_stride=2 * n - 1, mem=7)
    assert e.value.code == ERR_ARG
    _, roots = ctx.fr_merkle_commit(d_a.ptr, lanes=0, n=n, stride=n, tree=g_tree.ptr, tree_stride=2 * n - 1, mem=czk.CZK_MEM_DEVICE)   # lanes = 0: CZK_OK
    ctx.sync()
    assert roots.shape == (0, 32) and g_tree.untouched()
    G.check()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. open / verify
# ---------------------------------------------------------------------------------------------------------------------------------------
def model_opening(canon, trees_bytes, n, idx):
    """(shares (q, lanes, 4) canonical ints as a list of lists, paths bytes (q, lanes, log n, 32)) from the model"""
    lanes = canon.shape[0]
    levels = [M.tree_levels_of_bytes(canon[ln].tobytes()) for ln in range(lanes)]
    vals = [limbs_to_ints(canon[ln]) for ln in range(lanes)]
    shares, paths = [], b""
    for i in idx:
        _, sh, pa = M.open_at(vals, levels, int(i))
        shares.append(sh)
        paths += b"".join(b"".join(p) for p in pa)
    return shares, paths


def test_open_every_index_of_eight_by_three_lanes_and_verify_accepts(gpu, orc):
    czk, ctx = gpu
    canon, a, trees = vector_case(orc, 3, 8)
    tree, roots = ctx.fr_merkle_commit(a, lanes=3)
    idx = np.arange(8, dtype=np.uint64)
    shares, paths = ctx.fr_merkle_open(a, tree, idx, lanes=3)
    want_sh, want_pa = model_opening(canon, trees, 8, idx)
    assert shares.shape == (8, 3, 4) and paths.shape == (8, 3, 3, 32)
    assert [unmont(shares[i]) for i in range(8)] == want_sh and paths.tobytes() == want_pa
    values = mont([sum(s) % R_MOD for s in want_sh])
    ok, bad = ctx.fr_merkle_verify(roots, idx, shares, paths, 8, values=values)
    assert ok.tolist() == [1] * 8 and bad == 0
    ok, bad = ctx.fr_merkle_verify(roots, idx, shares, paths, 8)                        # values = NULL: the paths alone
    assert ok.tolist() == [1] * 8 and bad == 0
    # the model accepts what the library opened, and the library what the model opened
    model_roots = [t[-32:] for t in trees]
    for i in range(8):
        pa = [[paths[i, ln, lv].tobytes() for lv in range(3)] for ln in range(3)]
        assert M.check_opening(model_roots, unmont(shares[i]), pa, i, sum(want_sh[i]) % R_MOD)
    # the same path under the wrong index fails at every query but those it cannot tell apart (none: every index differs in a bit)
    ok, bad = ctx.fr_merkle_verify(roots, idx[::-1].copy(), shares, paths, 8, values=values)
    assert ok.tolist() == [0] * 8 and bad == 8


@pytest.mark.parametrize("q", [1, 300])
def test_open_and_verify_in_device_memory_past_one_block(gpu, orc, q):
    czk, ctx = gpu
    n, lanes, log_n = 1 << 12, 2, 12
    canon, a, trees = vector_case(orc, lanes, n)
    rng = np.random.default_rng(q)
    idx = rng.integers(0, n, size=q, dtype=np.uint64)
    idx[0], idx[-1] = n - 1, (0 if q > 1 else n - 1)
    G = Guards("cuda")
    d_a, d_idx = G.freeze(a, "a"), G.freeze(idx.view(np.int64), "idx")
    d_tree = G.freeze(np.frombuffer(b"".join(trees), dtype=np.uint8).copy(), "tree")
    g_sh = G.out(1, q * lanes, name="shares")
    g_pa = G.out(1, q * lanes * log_n, name="paths")
    ctx.fr_merkle_open(d_a.ptr, d_tree.ptr, d_idx.ptr, lanes=lanes, n=n, stride=n, tree_stride=2 * n - 1, q=q, out_shares=g_sh.ptr, out_paths=g_pa.ptr,
                       mem=czk.CZK_MEM_DEVICE)
    ctx.sync()
    shares, paths = G.check()
    want_sh, want_pa = model_opening(canon, trees, n, idx)
    assert [unmont(shares[0, i * lanes:(i + 1) * lanes]) for i in range(q)] == want_sh and paths.view(np.uint8).tobytes() == want_pa
    # verify in device memory: roots straight from the trees
    values = mont([sum(s) % R_MOD for s in want_sh])
    d_roots = to_dev(np.frombuffer(b"".join(t[-32:] for t in trees), dtype=np.uint8).copy())
    d_val = G.freeze(values, "values")
    g_ok = G.bytes(q, "ok")
    _, bad = ctx.fr_merkle_verify(d_roots.data_ptr(), d_idx.ptr, g_sh.ptr, g_pa.ptr, n, values=d_val.ptr, lanes=lanes, q=q, ok=g_ok.ptr, mem=czk.CZK_MEM_DEVICE)
    assert bad == 0 and G.check()[2].reshape(-1).tolist() == [1] * q
    host_ok, bad = ctx.fr_merkle_verify(np.frombuffer(b"".join(t[-32:] for t in trees), dtype=np.uint8), idx, shares.reshape(q, lanes, 4),
                                        paths.view(np.uint8).reshape(q, lanes, log_n, 32), n, values=values)
    assert bad == 0 and host_ok.tolist() == [1] * q


def test_single_leaf_tree_has_empty_paths(gpu, orc):
    czk, ctx = gpu
    canon, a, trees = vector_case(orc, 3, 1)
    tree, roots = ctx.fr_merkle_commit(a, lanes=3)
    assert tree.shape == (3, 1, 32) and np.array_equal(tree[:, 0], roots)
    assert [roots[ln].tobytes() for ln in range(3)] == [hashlib.sha256(canon[ln, 0].tobytes()).digest() for ln in range(3)]
    shares, paths = ctx.fr_merkle_open(a, tree, [0, 0], lanes=3)
    assert paths.shape == (2, 3, 0, 32) and np.array_equal(shares[0], a[:, 0]) and np.array_equal(shares[1], a[:, 0])
    ok, bad = ctx.fr_merkle_verify(roots, [0, 0], shares, paths, 1, values=mont([sum(limbs_to_ints(canon[:, 0])) % R_MOD] * 2))
    assert ok.tolist() == [1, 1] and bad == 0
    shares[1, 2, 0] ^= np.uint64(1)
    ok, bad = ctx.fr_merkle_verify(roots, [0, 0], shares, paths, 1)
    assert ok.tolist() == [1, 0] and bad == 1


def test_verify_reports_exactly_the_tampered_queries(gpu, orc):
    czk, ctx = gpu
    n, lanes, log_n, q = 1 << 12, 2, 12, 300
    canon, a, trees = vector_case(orc, lanes, n)
    tree, roots = ctx.fr_merkle_commit(a, lanes=lanes)
    idx = np.random.default_rng(5).integers(0, n, size=q, dtype=np.uint64)
    shares, paths = ctx.fr_merkle_open(a, tree, idx, lanes=lanes)
    values = mont([sum(unmont(shares[i])) % R_MOD for i in range(q)])
    sh, pa, va = shares.copy(), paths.copy(), values.copy()
    sh[3, 1, 2] ^= np.uint64(1 << 17)                  # one share limb (the value no longer matches either: one bad query all the same)
    pa[40, 0, 0, 31] ^= 1                              # a sibling byte at the lowest level
    pa[257, 1, log_n - 1, 0] ^= 0x80                   # ... and at the highest, past the first block of queries
    va[299, 0] ^= np.uint64(1)                         # one value
    ok, bad = ctx.fr_merkle_verify(roots, idx, sh, pa, n, values=va)
    want = np.ones(q, dtype=np.uint8)
    want[[3, 40, 257, 299]] = 0
    assert ok.tolist() == want.tolist() and bad == 4
    # a share changed with its value moved along: the sum holds, the path does not
    va2 = values.copy()
    va2[3] = mont([sum(unmont(sh[3])) % R_MOD])[0]
    ok, bad = ctx.fr_merkle_verify(roots, idx, sh, paths, n, values=va2)
    assert bad == 1 and ok[3] == 0
    # one root byte: every query fails
    r2 = roots.copy()
    r2[1, 5] ^= 4
    ok, bad = ctx.fr_merkle_verify(r2, idx, shares, paths, n, values=values)
    assert ok.tolist() == [0] * q and bad == q
    ok, bad = ctx.fr_merkle_verify(roots, idx, shares, paths, n, values=values)
    assert ok.tolist() == [1] * q and bad == 0


def test_indices_out_of_range_error_codes_and_empty_calls(gpu, orc):
    czk, ctx = gpu
    n, lanes, log_n = 8, 3, 3
    canon, a, trees = vector_case(orc, lanes, n)
    tree, roots = ctx.fr_merkle_commit(a, lanes=lanes)
    idx = np.array([1, 8, 6, 1 << 63], dtype=np.uint64)
    with pytest.raises(czk.CzkError, match="index beyond the vector") as e:
        ctx.fr_merkle_open(a, tree, idx, lanes=lanes)
    assert e.value.code == ERR_ARG
    good_sh, good_pa = ctx.fr_merkle_open(a, tree, [1, 0, 6, 0], lanes=lanes)
    with pytest.raises(czk.CzkError, match="index beyond the vector") as e:
        ctx.fr_merkle_verify(roots, idx, good_sh, good_pa, n)
    assert e.value.code == ERR_ARG
    # device memory: zero shares and zero paths for the two bad queries, the others as ever; nothing outside the outputs is written
    G = Guards("cuda")
    d_a, d_tree, d_idx = G.freeze(a, "a"), G.freeze(tree, "tree"), G.freeze(idx.view(np.int64), "idx")
    g_sh, g_pa = G.out(1, 4 * lanes, name="shares"), G.out(1, 4 * lanes * log_n, name="paths")
    ctx.fr_merkle_open(d_a.ptr, d_tree.ptr, d_idx.ptr, lanes=lanes, n=n, stride=n, tree_stride=2 * n - 1, q=4, out_shares=g_sh.ptr, out_paths=g_pa.ptr,
                       mem=czk.CZK_MEM_DEVICE)
    ctx.sync()
    shares, paths = G.check()
    shares, paths = shares.reshape(4, lanes, 4), paths.view(np.uint8).reshape(4, lanes, log_n, 32)
    assert np.array_equal(shares[[0, 2]], good_sh[[0, 2]]) and np.array_equal(paths[[0, 2]], good_pa[[0, 2]])
    assert not shares[[1, 3]].any() and not paths[[1, 3]].any()
    # ... and the verify calls those queries bad, whatever shares and paths come with them
    d_roots, d_sh, d_pa = to_dev(roots), to_dev(good_sh), to_dev(good_pa)
    g_ok = G.bytes(4, "ok")
    _, bad = ctx.fr_merkle_verify(d_roots.data_ptr(), d_idx.ptr, d_sh.data_ptr(), d_pa.data_ptr(), n, lanes=lanes, q=4, ok=g_ok.ptr, mem=czk.CZK_MEM_DEVICE)
    assert bad == 2 and G.check()[2].reshape(-1).tolist() == [1, 0, 1, 0]
    # sizes
    for call in (lambda: ctx.fr_merkle_open(a[:, :6], tree, [0], lanes=lanes), lambda: ctx.fr_merkle_verify(roots, [0], good_sh[:1], good_pa[:1, :, :2], 6),
                 lambda: ctx.fr_merkle_open(a, tree, [0], lanes=lanes, tree_stride=2 * n - 2),
                 lambda: ctx.fr_merkle_open(d_a.ptr, d_tree.ptr, d_idx.ptr, lanes=lanes, n=n, stride=n - 1, tree_stride=2 * n - 1, q=4, out_shares=g_sh.ptr,
                                            out_paths=g_pa.ptr, mem=czk.CZK_MEM_DEVICE)):
        with pytest.raises(czk.CzkError) as e:
            call()
        assert e.value.code == ERR_SIZE
    # q = 0 and lanes = 0: CZK_OK, nothing touched
    g_sh2, g_ok2 = G.out(1, 4 * lanes, name="shares (empty calls)"), G.bytes(4, "ok (empty calls)")
    for ln, q in ((lanes, 0), (0, 4)):
        ctx.fr_merkle_open(d_a.ptr, d_tree.ptr, d_idx.ptr, lanes=ln, n=n, stride=n, tree_stride=2 * n - 1, q=q, out_shares=g_sh2.ptr, out_paths=g_pa.ptr,
                           mem=czk.CZK_MEM_DEVICE)
        _, bad = ctx.fr_merkle_verify(d_roots.data_ptr(), d_idx.ptr, d_sh.data_ptr(), d_pa.data_ptr(), n, lanes=ln, q=q, ok=g_ok2.ptr, mem=czk.CZK_MEM_DEVICE)
        assert bad == 0
    ctx.sync()
    assert g_sh2.untouched() and g_ok2.untouched()
    sh0, pa0 = ctx.fr_merkle_open(a, tree, np.zeros(0, dtype=np.uint64), lanes=lanes)
    assert sh0.shape == (0, lanes, 4) and pa0.shape == (0, lanes, log_n, 32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. fold
# ---------------------------------------------------------------------------------------------------------------------------------------
ALPHAS = {"zero": 0, "one": 1, "minus_one": R_MOD - 1, "random": int.from_bytes(hashlib.sha256(b"fold alpha").digest(), "little") % R_MOD}


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("alpha", sorted(ALPHAS))
@pytest.mark.parametrize("n", [2, 4, 514])
def test_fold_matches_the_model_and_leaves_the_rest(gpu, orc, n, alpha, mem):
    czk, ctx = gpu
    lanes, al, half = 3, ALPHAS[alpha], n // 2
    canon = rand_fr_canonical(900 + n, lanes * n).reshape(lanes, n, 4)
    canon[0, 0], canon[1, 1], canon[2, n - 1] = 0, ints_to_limbs([R_MOD - 1], 4).reshape(4), ints_to_limbs([R_MOD - 1], 4).reshape(4)
    f = orc.fr_from_repr(canon.reshape(-1, 4)).reshape(lanes, n, 4)
    want = [M.fold(limbs_to_ints(canon[ln]), al) for ln in range(lanes)]
    stride, out_stride = n + 2, half + 3
    src = np.full((lanes, stride, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    src[:, :n] = f
    if mem == "host":
        out = np.full((lanes, out_stride, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        assert ctx.fri_fold(src, mont([al])[0], lanes=lanes, n=n, out=out) is out
        assert (out[:, half:] == 0xA5A5A5A5A5A5A5A5).all()                             # the output past n / 2 is untouched
        got = out[:, :half]
        assert np.array_equal(ctx.fri_fold(f, mont([al])[0], lanes=lanes), got)         # dense strides
    else:
        G = Guards("cuda")
        d_f = G.freeze(src, "f")
        g_out = G.out(lanes, half, out_stride, name="out")
        ctx.fri_fold(d_f.ptr, mont([al])[0], lanes=lanes, n=n, stride=stride, out=g_out.ptr, out_stride=out_stride, mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        got = G.check()[0]
    assert [unmont(got[ln]) for ln in range(lanes)] == want


def test_fold_error_codes(gpu, orc):
    czk, ctx = gpu
    f = mont(list(range(1, 9))).reshape(1, 8, 4)
    one = mont([1])[0]
    for call in (lambda: ctx.fri_fold(f[:, :1], one, n=1), lambda: ctx.fri_fold(f, one, n=0),
                 lambda: ctx.fri_fold(f, one, n=8, out=np.zeros((1, 3, 4), dtype=np.uint64))):
        with pytest.raises(czk.CzkError) as e:
            call()
        assert e.value.code == ERR_SIZE
    d_f = to_dev(f)
    with pytest.raises(czk.CzkError, match="overlaps") as e:                             # out inside f
        ctx.fri_fold(d_f.data_ptr(), one, lanes=1, n=8, stride=8, out=d_f.data_ptr() + 64, out_stride=4, mem=czk.CZK_MEM_DEVICE)
    assert e.value.code == ERR_ARG
    assert ctx.fri_fold(np.zeros((0, 8, 4), dtype=np.uint64), one, lanes=0, n=8, out=np.zeros((0, 4, 4), dtype=np.uint64)).shape == (0, 4, 4)   # lanes = 0: CZK_OK


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. czk_amd.fri
# ---------------------------------------------------------------------------------------------------------------------------------------
def challenge(i, roots):
    return int.from_bytes(hashlib.sha256(b"alpha" + bytes([i]) + b"".join(roots)).digest(), "little") % R_MOD


def fri_case(k, parties):
    """additive lanes of a random polynomial of 2^k coefficients, and 4 start indices with the first and the last of the 2^(k+1)-point domain"""
    canon = rand_fr_canonical(4000 + 10 * k + parties, parties << k).reshape(parties, 1 << k, 4)
    top = (1 << (k + 1)) - 1
    return canon, [0, top, top // 3, (5 * top) // 7]


def assert_proof_equals_model(proof, model):
    assert proof["k"] == model["k"] and proof["lanes"] == model["lanes"] and proof["constant"] == model["constant"]
    assert proof["roots"] == model["roots"] and proof["x_indices"] == model["x_indices"]
    for rd, want in zip(proof["rounds"], model["rounds"]):
        q = len(want["idx"])
        assert rd["idx"].tolist() == want["idx"]
        assert unmont(rd["values"]) == want["values"]
        assert [unmont(rd["shares"][i]) for i in range(q)] == want["shares"]
        assert rd["paths"].tobytes() == b"".join(b"".join(b"".join(p) for p in pa) for pa in want["paths"])


@pytest.mark.parametrize("parties", [2, 3])
@pytest.mark.parametrize("k", [0, 1, 2, 5, 10])
def test_fri_commit_query_verify_equal_the_model(gpu, orc, k, parties):
    czk, ctx = gpu
    fri = czk.fri
    canon, starts = fri_case(k, parties)
    f = orc.fr_from_repr(canon.reshape(-1, 4)).reshape(parties, 1 << k, 4)
    want_state = M.commit_phase([limbs_to_ints(canon[ln]) for ln in range(parties)], challenge)
    state = fri.commit_phase(ctx, f, challenge)
    try:
        assert state["k"] == k and state["constant"] == want_state["constant"]
        assert [rd["roots"] for rd in state["rounds"]] == [rd["roots"] for rd in want_state["rounds"]]
        assert [rd["alpha"] for rd in state["rounds"]] == [rd["alpha"] for rd in want_state["rounds"]]
        if k:   # a whole tree and a whole evaluation vector, not only what the queries touch
            rd, wrd = state["rounds"][0], want_state["rounds"][0]
            assert unmont(rd["evals"].download(lane=parties - 1)) == wrd["evals"][parties - 1]
            assert rd["tree"].download(lane=0).view(np.uint8).tobytes() == M.tree_bytes(wrd["trees"][0])
            assert fri.commitment_bytes(rd["roots"]) == M.commitment_bytes(wrd["roots"])
        proof = fri.query_phase(ctx, state, starts)
        assert_proof_equals_model(proof, M.query_phase(want_state, starts))
        assert fri.verify(ctx, proof, challenge) is True
        assert M.verify(M.query_phase(want_state, starts), challenge)
        if k:
            assert fri.verify(ctx, proof, lambda i, roots: challenge(i, roots) + (i == k - 1)) is False      # the verifier's alpha differs
            proof["constant"] = (proof["constant"] + 1) % R_MOD
            assert fri.verify(ctx, proof, challenge) is False
    finally:
        fri.release(state)


@pytest.mark.parametrize("parties", [2, 3])
def test_fri_rejects_a_changed_evaluation_and_a_fold_with_another_alpha(gpu, orc, parties):
    czk, ctx = gpu
    fri = czk.fri
    k = 5
    canon, starts = fri_case(k, parties)
    f = orc.fr_from_repr(canon.reshape(-1, 4)).reshape(parties, 1 << k, 4)
    # one evaluation of round 1 changed on the device after its tree was committed: the opening fails
    state = fri.commit_phase(ctx, f, challenge)
    try:
        at = fri.chain_indices(k, starts)[1][2]                     # round 1's x of the third start
        ev = state["rounds"][1]["evals"]
        changed = ev.download(lane=parties - 1, elem=at, n=1)
        changed[0, 0] ^= np.uint64(1)
        ev.upload(changed, lane=parties - 1, elem=at)
        proof = fri.query_phase(ctx, state, starts)
        ok, bad = fri.check_opening(ctx, proof["roots"][1], 1 << k, proof["rounds"][1])
        hit = [j for j, i in enumerate(proof["rounds"][1]["idx"].tolist()) if i == at]
        assert bad == len(hit) >= 2 and [j for j in range(len(ok)) if not ok[j]] == hit
        assert fri.verify(ctx, proof, challenge) is False
        assert fri.verify(ctx, fri.query_phase(ctx, state, starts[:2]), challenge) is True   # chains that do not pass through it still hold
    finally:
        fri.release(state)
    # the prover folds round 2 with another alpha: every path holds, the relation fails
    state = fri.commit_phase(ctx, f, challenge, fold_alpha=lambda i, a: a + (i == 2))
    try:
        proof = fri.query_phase(ctx, state, starts)
        for i, rd in enumerate(proof["rounds"]):
            assert fri.check_opening(ctx, proof["roots"][i], 1 << (k + 1 - i), rd)[1] == 0
        assert fri.verify(ctx, proof, challenge) is False
        model = M.query_phase(M.commit_phase([limbs_to_ints(canon[ln]) for ln in range(parties)], challenge, fold_alpha=lambda i, a: a + (i == 2)), starts)
        assert_proof_equals_model(proof, model)
    finally:
        fri.release(state)
