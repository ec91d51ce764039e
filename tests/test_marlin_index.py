"""Marlin's index on the GPU and the Marlin verifier (czk_amd.marlin, csrc/marlin_index.hip).

1. czk_marlin_arithmetize against a big-integer model of arithmetize_matrix (marlin/src/ahp/constraint_systems.rs:152-262) written here in the reference's
   form -- val * (|H| e^(|H| - 1))^-1 with a real modular inverse -- so the kernel's shortcut e / |H| is checked, not assumed; every limb is compared.
2. marlin.index / prover_inputs equal tests/polyiop_real.py::marlin_real_inputs, the hand-built index of one hard-wired circuit, limb for limb.  That circuit's
   A and B hold one entry per row: the densities tie, a tie counts as "A is denser" (balance_matrices, :25-41), so the indexer swaps EVERY row and the index's
   A is the helper's B and the other way round (the helper does not balance; a . b = c does not care).  The comparison exchanges the two names and nothing else.
3. index -> prover_inputs -> polyvm.marlin_prove -> marlin.verify on a circuit that is not that chain, and the verifier's negative cases.
"""
import random

import numpy as np
import pytest

from groth16_real_key import omega_for
from util import R_MOD, ints_to_limbs, limbs_to_ints, rand_fr_canonical

pytestmark = pytest.mark.gpu
RR = (1 << 256) % R_MOD
R_INV = pow(1 << 256, -1, R_MOD)
ERR_SIZE, ERR_ARG = 1, 3


def mont(vals):
    return ints_to_limbs([v % R_MOD * RR % R_MOD for v in vals], 4).reshape(-1, 4)


def unmont(limbs):
    return [v * R_INV % R_MOD for v in limbs_to_ints(np.asarray(limbs).reshape(-1, 4))]


@pytest.fixture(scope="module")
def gpu():
    """(czk_amd, context, two-lane backend with public data on every lane: each lane is the plain prover)"""
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    B = polyvm.GpuBackend(czk_amd, ctx, 2, polyvm.marlin_max_degree(64), lift=(1, 1))
    yield czk_amd, ctx, B
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
def reindex(H, X, index):
    period = H // X
    if index < X:
        return index * period
    i = index - X
    return i + i // (period - 1) + 1


def model(rows, H, X, n_instance, k):
    """rows: list of rows of (coefficient, variable) -> four lists of k integers: row, col, val, row_col"""
    w = omega_for(H.bit_length() - 1)
    elems = [pow(w, i, R_MOD) for i in range(H)]
    u = {e: H * pow(e, H - 1, R_MOD) % R_MOD for e in elems}                    # u_H(e, e), eq_poly_vals (:169-172)
    row_v, col_v, val_v = [], [], []
    for r, row in enumerate(rows):
        for cf, i in row:
            i_pad = i if i < n_instance else i + (X - n_instance)
            e = elems[reindex(H, X, i_pad)]
            row_v.append(e)
            col_v.append(elems[r])
            val_v.append(cf * pow(u[e], -1, R_MOD) % R_MOD)
    pad = k - len(row_v)
    row_v, col_v, val_v = row_v + [1] * pad, col_v + [1] * pad, val_v + [0] * pad
    return row_v, col_v, val_v, [a * b % R_MOD for a, b in zip(row_v, col_v)]


def csr(rows):
    rp, col, cf = [0], [], []
    for row in rows:
        for c, i in row:
            col.append(i)
            cf.append(c)
        rp.append(len(col))
    return np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint32), mont(cf)


def rows_of(lens, n_vars, seed):
    """rows of the given lengths over n_vars variables: random coefficients and columns in the order drawn; the first row of two or more entries repeats a
    column, the first entry is a stored zero, the second a one"""
    rng = random.Random(seed)
    rows = [[(rng.randrange(R_MOD), rng.randrange(n_vars)) for _ in range(n)] for n in lens]
    flat = [(r, t) for r, row in enumerate(rows) for t in range(len(row))]
    for (r, t), cf in zip(flat, (0, 1)):
        rows[r][t] = (cf, rows[r][t][1])
    for row in rows:
        if len(row) >= 2:
            row[1] = (row[1][0], row[0][1])
            break
    return rows


rng64 = random.Random(64)
KERNEL_CASES = {
    # name: (H, X, n_instance, row lengths, k)
    "H2_partly_filled": (2, 2, 2, [1, 2], 4),
    "H2_full": (2, 2, 2, [2, 2], 4),
    "H4_empty_rows_first_and_between": (4, 2, 2, [0, 3, 0, 1], 4),
    "H4_no_entries": (4, 2, 2, [0, 0, 0], 2),
    "H4_no_rows": (4, 2, 2, [], 3),
    "H8_one_input_fewer_rows_than_H": (8, 1, 1, [0, 0, 5, 0, 0, 2, 1], 16),
    "H8_padded_inputs_empty_rows_last": (8, 4, 3, [1, 4, 0, 0, 0, 3, 2, 0], 10),
    "H8_padded_inputs_full": (8, 4, 3, [2, 2, 0, 0, 4, 0, 0, 0], 8),
    "H64_partial_block": (64, 4, 4, [rng64.randrange(6) for _ in range(60)], 257),
    "H64_two_blocks_full": (64, 4, 4, [5] * 60, 300),
}


@pytest.mark.parametrize("name", sorted(KERNEL_CASES))
def test_arithmetize_matches_the_big_integer_model(gpu, name):
    czk, ctx, _ = gpu
    H, X, ni, lens, k = KERNEL_CASES[name]
    rows = rows_of(lens, H - X + ni, 7 + len(name))
    assert sum(lens) <= k and len(lens) <= H
    log_h, log_x = H.bit_length() - 1, X.bit_length() - 1
    assert unmont(ctx.domain_constants(log_h)["group_gen"])[0] == omega_for(log_h)          # the library's get_root_of_unity(|H|)
    got = ctx.marlin_arithmetize(*csr(rows), log_h, log_x, ni, k)
    want = model(rows, H, X, ni, k)
    for j, part in enumerate(("row", "col", "val", "row_col")):
        assert np.array_equal(got[j], mont(want[j])), (name, part)


def test_arithmetize_on_device_buffers_equals_host_buffers(gpu):
    import torch
    czk, ctx, _ = gpu
    H, X, ni, lens, k = KERNEL_CASES["H64_partial_block"]
    rp, col, cf = csr(rows_of(lens, H - X + ni, 99))
    want = ctx.marlin_arithmetize(rp, col, cf, 6, 2, ni, k)
    dev = [torch.from_numpy(a).cuda() for a in (rp.view(np.int64), col.view(np.int32), cf.view(np.int64))]
    out = torch.empty((4, k, 4), dtype=torch.int64, device="cuda")
    ctx.marlin_arithmetize(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 6, 2, ni, k, out=out.data_ptr(), mem=czk.CZK_MEM_DEVICE, m=len(lens), nnz=col.size)
    ctx.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want)


def test_arithmetize_error_codes(gpu):
    czk, ctx, _ = gpu
    rows = [[(1, 0)], [(2, 5), (3, 1)], []]                                                 # H = 8, X = 2, two inputs: variables 0 .. 7
    rp, col, cf = csr(rows)

    def code(*a, **kw):
        with pytest.raises(czk.CzkError) as e:
            ctx.marlin_arithmetize(*a, **kw)
        return e.value.code
    assert ctx.marlin_arithmetize(rp, col, cf, 3, 1, 2, 4).shape == (4, 4, 4)
    assert code(np.array([0, 2, 1, 3], dtype=np.uint64), col, cf, 3, 1, 2, 4) == ERR_ARG       # row_ptr not monotone
    assert code(np.array([0, 1, 2, 2], dtype=np.uint64), col, cf, 3, 1, 2, 4) == ERR_ARG       # row_ptr[m] != nnz
    assert code(np.array([1, 1, 3, 3], dtype=np.uint64), col, cf, 3, 1, 2, 4) == ERR_ARG       # row_ptr[0] != 0
    assert code(rp, np.array([0, 8, 1], dtype=np.uint32), cf, 3, 1, 2, 4) == ERR_ARG           # variable 8 of 8
    assert code(rp, np.array([0, 7, 1], dtype=np.uint32), cf, 3, 1, 1, 4) == ERR_ARG           # one input padded to X = 2: 7 variables fit
    assert ctx.marlin_arithmetize(rp, np.array([0, 6, 1], dtype=np.uint32), cf, 3, 1, 1, 4).shape == (4, 4, 4)
    assert code(rp, col, cf, 1, 1, 2, 4) == ERR_SIZE                                           # three rows, |H| = 2
    assert code(rp, col, cf, 3, 1, 2, 2) == ERR_SIZE                                           # k < nnz
    assert code(rp, col, cf, 3, 4, 2, 4) == ERR_SIZE                                           # log_x > log_h
    assert code(rp, col, cf, 3, 1, 3, 4) == ERR_SIZE                                           # n_instance > X


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. marlin.index against the hand-built index of the squaring chain
# ---------------------------------------------------------------------------------------------------------------------------------------
def chain_circuit(H, seed):
    """marlin_real_inputs' circuit as CSR matrices and its assignment: formatted input [1, out], the chain w_{i+1} = w_i^2 ending in out, the rows
    1 * out = out and 3 * 1 = 3"""
    X, nw = 2, H - 2
    w = limbs_to_ints(rand_fr_canonical(seed, 1))
    for _ in range(nw - 1):
        w.append(w[-1] * w[-1] % R_MOD)
    out_v = w[-1] * w[-1] % R_MOD
    rows = {"a": [[(1, X + i)] for i in range(nw)] + [[(1, 0)], [(3, 0)]],
            "b": [[(1, X + i)] for i in range(nw)] + [[(1, 1)], [(1, 0)]],
            "c": [[(1, X + i + 1 if i + 1 < nw else 1)] for i in range(nw)] + [[(1, 1)], [(3, 0)]]}
    return {m: csr(rows[m]) for m in "abc"}, [1, out_v], w


@pytest.mark.parametrize("H", [16, 64])
def test_index_equals_the_hand_built_index(gpu, H):
    czk, ctx, B = gpu
    from czk_amd import marlin, polyvm
    import polyiop_real
    seed = 0x3A21 + H
    want = polyiop_real.marlin_real_inputs(B, polyvm, H, seed)
    mats, instance, witness = chain_circuit(H, seed)
    idx = marlin.index(B, mats["a"], mats["b"], mats["c"], 2, H - 2)
    assert idx["info"] == {"num_variables": H, "num_constraints": H, "num_non_zero": H, "num_instance_variables": 2}
    for key in ("H", "K", "X", "b_size", "real_lcs", "t_rows"):
        assert idx[key] == want[key], key
    other = {"a": "b", "b": "a", "c": "c"}                     # balance_matrices swaps every row of A and B here (module docstring)
    dl = lambda a: B.download(a).copy()   # noqa: E731
    v = B.random(0x77, H)
    for i, m in enumerate("abc"):
        o = "abc".index(other[m])
        for part in ("on_K", "on_B"):
            assert len(idx["star"][m][part]) == len(want["star"][other[m]][part])
            for j, (g, w) in enumerate(zip(idx["star"][m][part], want["star"][other[m]][part])):
                assert np.array_equal(dl(g), dl(w)), (m, part, j)
        for j in range(4):
            assert np.array_equal(dl(idx["index_polys"][4 * i + j]), dl(want["index_polys"][4 * o + j])), (m, j)
            for g, w in zip(idx["index_cmts"][4 * i + j], want["index_cmts"][4 * o + j]):
                assert np.array_equal(np.asarray(g), np.asarray(w)), (m, j)
        assert np.array_equal(dl(B.matvec(idx["matrices_T"][m], v)), dl(B.matvec(want["matrices_T"][other[m]], v))), m
    inp = marlin.prover_inputs(B, idx, instance, witness)
    assert inp["x_ints"] == want["x_ints"] and np.array_equal(dl(inp["x"]), dl(want["x"]))
    for key, wkey in (("w", "w"), ("z_a", "z_b"), ("z_b", "z_a")):
        g, w = dl(inp[key]), dl(want[wkey])
        assert g.shape == w.shape == (2, H, 4) and np.array_equal(g, w), key
    mask = unmont(dl(inp["mask_poly"])[0])
    assert len(mask) == 3 * H and (mask[0] + mask[H] + mask[2 * H]) % R_MOD == 0 and np.array_equal(dl(inp["mask_poly"])[0], dl(inp["mask_poly"])[1])


def test_index_refuses_fewer_than_two_entries(gpu):
    from czk_amd import marlin
    one = csr([[(1, 0)], []])
    with pytest.raises(ValueError):
        marlin.index(gpu[2], one, one, one, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. end to end on another circuit
# ---------------------------------------------------------------------------------------------------------------------------------------
def other_circuit(seed):
    """13 constraints over the formatted input [1, out, 3] (X = 4 after padding) and 9 witnesses: 4 + 9 = 13 variables, H = 16.  Multi-term rows, a row
    that names one variable twice, rows whose entries are not in column order, A (22 entries) denser than B (14): balancing swaps rows 0 .. 11 and stops."""
    ONE, OUT, THREE = 0, 1, 2
    W = lambda i: 3 + i   # noqa: E731
    neg = R_MOD - 1
    a = [[(1, W(0))], [(1, W(1))], [(1, W(2)), (1, W(0)), (5, ONE)], [(1, W(1)), (1, W(0))], [(1, THREE)], [(1, W(5)), (1, W(5))], [(1, W(6))],
         [(1, W(7)), (neg, W(1))], [(1, W(8))], [(1, THREE)], [(1, ONE)], [(1, W(3)), (1, W(0)), (1, W(2)), (1, W(1))], [(2, W(4)), (1, W(5))]]
    b = [[(1, W(0))], [(1, W(0))], [(1, ONE)], [(1, W(3)), (1, W(2))], [(1, W(4))], [(1, ONE)], [(1, W(6))], [(1, ONE)], [(1, W(0))], [(1, ONE)], [(1, OUT)],
         [(1, ONE)], [(1, ONE)]]
    c = [[(1, W(1))], [(1, W(2))], [(1, W(3))], [(1, W(4))], [(1, W(5))], [(1, W(6))], [(1, W(7))], [(1, W(8))], [(1, OUT)], [(3, ONE)], [(1, OUT)],
         [(1, W(2)), (1, W(3)), (1, W(0)), (1, W(1))], [(5, W(4))]]
    w = limbs_to_ints(rand_fr_canonical(seed, 1))
    w.append(w[0] * w[0] % R_MOD)
    w.append(w[1] * w[0] % R_MOD)
    w.append((w[2] + w[0] + 5) % R_MOD)
    w.append((w[0] + w[1]) * (w[2] + w[3]) % R_MOD)
    w.append(3 * w[4] % R_MOD)
    w.append(2 * w[5] % R_MOD)
    w.append(w[6] * w[6] % R_MOD)
    w.append((w[7] - w[1]) % R_MOD)
    z = [1, w[8] * w[0] % R_MOD, 3] + w
    dot = lambda row: sum(cf * z[i] for cf, i in row) % R_MOD   # noqa: E731
    assert len(a) == len(b) == len(c) == 13 and all(dot(x) * dot(y) % R_MOD == dot(v) for x, y, v in zip(a, b, c))
    assert sum(map(len, a)) == 22 and sum(map(len, b)) == 14
    return csr(a), csr(b), csr(c), z[:3], w


@pytest.fixture(scope="module")
def proof(gpu):
    czk, ctx, B = gpu
    from czk_amd import marlin, polyvm
    A, Bm, C, instance, witness = other_circuit(0x0C1C)
    idx = marlin.index(B, A, Bm, C, 3, 9)
    assert (idx["H"], idx["K"], idx["X"], idx["b_size"]) == (16, 32, 4, 128)
    assert idx["info"] == {"num_variables": 13, "num_constraints": 13, "num_non_zero": 22, "num_instance_variables": 4}
    assert [int(idx["matrices"][m][0][-1]) for m in "abc"] == [15, 21, 16]          # rows 0 .. 11 swapped: A keeps 22 - 7 entries, B holds 14 + 7
    inp = marlin.prover_inputs(B, idx, instance, witness)
    assert inp["x_ints"] == instance + [0]
    return idx, instance, polyvm.marlin_prove(B, inp)


def test_proof_of_another_circuit_verifies(gpu, proof):
    from czk_amd import marlin
    idx, instance, out = proof
    assert marlin.verify(gpu[2], idx, instance, out, rng=random.Random(1)) is True
    assert marlin.verify(gpu[2], marlin.verifier_key(idx), instance + [0], out, rng=random.Random(2)) is True


def test_verifier_does_not_read_the_provers_combinations(gpu, proof):
    from czk_amd import marlin
    idx, instance, out = proof
    forged = dict(out, lcs={"outer_sumcheck": [(1, "w")], "inner_sumcheck": []}, lc_consts={"outer_sumcheck": 12345})
    forged["open_beta"] = dict(out["open_beta"], terms=[(7, "w")])
    assert marlin.verify(gpu[2], idx, instance, forged, rng=random.Random(3)) is True
    assert marlin.verify(gpu[2], idx, instance, {k: v for k, v in out.items() if k not in ("lcs", "lc_consts")}, rng=random.Random(4)) is True


@pytest.mark.parametrize("which", [1, 2])
def test_wrong_public_input_is_rejected(gpu, proof, which):
    from czk_amd import marlin
    idx, instance, out = proof
    x = list(instance)
    x[which] = (x[which] + 1) % R_MOD                          # out, or the 3
    assert marlin.verify(gpu[2], idx, x, out, rng=random.Random(5)) is False


@pytest.mark.parametrize("tag,at", [("beta", 5), ("gamma", 20)])
def test_changed_evaluation_is_rejected(gpu, proof, tag, at):
    """z_a(beta) -- read by the outer combination -- and a_val(gamma) -- by the inner one -- published as one more than they are, on every lane"""
    from czk_amd import marlin
    idx, instance, out = proof
    evals = list(out["evals_" + tag])
    evals[at] = np.tile(mont([unmont(evals[at])[0] + 1]), (2, 1))
    assert marlin.verify(gpu[2], idx, instance, dict(out, **{"evals_" + tag: evals}), rng=random.Random(6)) is False


def test_replaced_index_commitment_is_rejected(gpu, proof):
    """the key's commitment to a_val replaced by its commitment to a_row: the proof's own (honest) copy in `out` must not be what is checked"""
    from czk_amd import marlin
    idx, instance, out = proof
    vk = marlin.verifier_key(idx)
    vk["index_cmts"][2] = vk["index_cmts"][0]
    assert not np.array_equal(idx["index_cmts"][2][0], idx["index_cmts"][0][0])
    assert marlin.verify(gpu[2], vk, instance, out, rng=random.Random(7)) is False
    assert marlin.verify(gpu[2], marlin.verifier_key(idx), instance, out, rng=random.Random(8)) is True
