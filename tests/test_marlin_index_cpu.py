"""marlin.square_and_balance and marlin.reindex (host numpy on the CSR index arrays) against a deliberately naive restatement of the reference's
matrix preparation, row by row over Python lists as the reference walks its Vec<Vec<(F, usize)>>: pad_input_for_indexer_and_prover and
make_matrices_square (marlin/src/ahp/constraint_systems.rs:75-111), num_non_zero before balancing (indexer.rs:138-140), balance_matrices (:25-41, a tie
counts as "A is denser", one row at a time), the per-row stable sort of arithmetize_matrix (:183-185), reindex_by_subdomain
(algebra/poly/src/domain/mod.rs:196-218).  Every coefficient carries its own tag, so a misplaced entry shows even where columns repeat."""
import random

import numpy as np
import pytest

import czk_amd  # noqa: F401
from czk_amd import marlin


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def naive_reindex(H, X, index):
    period = H // X
    if index < X:
        return index * period
    i = index - X
    return i + i // (period - 1) + 1


def naive_square_and_balance(rows, ni, nw):
    """rows: {"a" | "b" | "c": list of rows, a row a list of (tag, column)} -> the same after the reference's preparation, and IndexInfo's numbers"""
    X = next_pow2(ni)
    rows = {m: [[(tag, c if c < ni else c + (X - ni)) for tag, c in row] for row in rs] for m, rs in rows.items()}
    n_vars, n_cons = X + nw, len(rows["a"])
    if n_vars > n_cons:
        for m in "abc":
            rows[m] += [[] for _ in range(n_vars - n_cons)]
    else:
        nw += n_cons - n_vars
    n_cons = len(rows["a"])
    num_non_zero = max(sum(len(r) for r in rows[m]) for m in "abc")
    a, b = rows["a"], rows["b"]
    a_density, b_density = sum(len(r) for r in a), sum(len(r) for r in b)
    max_density = max(a_density, b_density)
    a_is_denser = a_density == max_density
    for r in range(n_cons):
        if a_is_denser:
            la, lb = len(a[r]), len(b[r])
            a[r], b[r] = b[r], a[r]
            a_density = a_density - la + lb
            b_density = b_density - lb + la
            max_density = max(a_density, b_density)
            a_is_denser = a_density == max_density
    for m in "abc":
        for row in rows[m]:
            row.sort(key=lambda e: e[1])                       # list.sort is stable, as slice::sort_by is
    return rows, {"num_variables": X + nw, "num_constraints": n_cons, "num_non_zero": num_non_zero, "num_instance_variables": X}


def to_csr(rs):
    rp, col, tags = [0], [], []
    for row in rs:
        for tag, c in row:
            col.append(c)
            tags.append([tag, tag ^ 0x5A5A, 7, 0])             # four limbs that name the entry
        rp.append(len(col))
    return np.array(rp, dtype=np.uint64), np.array(col, dtype=np.uint32), np.array(tags, dtype=np.uint64).reshape(-1, 4)


def make_rows(lens, ni, nw, seed):
    """rows with the given lengths per matrix; columns drawn with replacement (so they repeat and arrive unsorted), across inputs and witnesses"""
    rng = random.Random(seed)
    tag = iter(range(1, 1 << 30))
    rows = {m: [[(next(tag), rng.randrange(ni + nw)) for _ in range(n)] for n in lens[m]] for m in "abc"}
    for m in "abc":
        for row in rows[m][::2]:
            row.sort(key=lambda e: -e[1])                      # every other row arrives in descending order for certain
    return rows


CASES = {
    # name: (row lengths of A, B, C, formatted inputs, witnesses)
    "a_denser": ([3, 2, 4, 1, 3], [1, 1, 0, 1, 1], [1, 1, 1, 1, 1], 2, 3),
    "b_denser": ([1, 0, 1, 1, 1], [3, 2, 4, 1, 3], [1, 2, 1, 0, 1], 2, 3),
    "equal_densities": ([1, 2, 3, 2], [2, 3, 2, 1], [1, 1, 1, 1], 2, 2),                 # the tie swaps rows 0 and 1, then A stays denser to the end
    "first_swap_flips": ([3, 1, 1, 2], [1, 1, 2, 2], [1, 0, 0, 5], 2, 2),               # A leads by one entry; swapping row 0 puts B ahead for good
    "flips_in_the_middle": ([2, 2, 5, 1, 1, 4], [1, 1, 1, 3, 3, 1], [0, 0, 0, 0, 0, 1], 2, 4),
    "fewer_constraints_than_variables": ([2, 1, 3], [1, 1, 1], [1, 1, 1], 2, 9),
    "more_constraints_than_variables": ([2, 1, 3, 1, 1, 2, 2, 1, 4], [1, 1, 1, 2, 0, 1, 1, 1, 1], [1] * 9, 2, 3),
    "one_input": ([2, 1, 3, 2], [1, 1, 1, 1], [1, 1, 1, 1], 1, 5),                       # X = 1
    "three_inputs": ([2, 1, 3, 2, 5], [1, 1, 1, 1, 0], [1, 1, 1, 1, 2], 3, 4),           # X = 4: witness columns move up by one
    "five_inputs": ([2, 1, 3, 2, 5, 4], [1, 1, 1, 1, 0, 6], [1, 1, 1, 1, 2, 0], 5, 4),   # X = 8: by three
    "empty_matrix": ([0, 0, 0], [1, 2, 0], [0, 0, 0], 2, 2),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_square_and_balance_matches_the_naive_restatement(name):
    la, lb, lc, ni, nw = CASES[name]
    for seed in range(4):
        rows = make_rows({"a": la, "b": lb, "c": lc}, ni, nw, 1000 * seed + len(name))
        got = marlin.square_and_balance(to_csr(rows["a"]), to_csr(rows["b"]), to_csr(rows["c"]), ni, nw)
        want, info = naive_square_and_balance(rows, ni, nw)
        assert got[3] == info, (name, seed)
        assert info["num_variables"] == info["num_constraints"]
        for m, g in zip("abc", got[:3]):
            w = to_csr(want[m])
            for part, (x, y) in enumerate(zip(g, w)):
                assert x.dtype == y.dtype and np.array_equal(x, y.reshape(x.shape)), (name, seed, m, part)


def test_repeated_columns_keep_their_order_and_are_not_merged():
    rows = {"a": [[(1, 3), (2, 1), (3, 3), (4, 1), (5, 0)]], "b": [[(6, 2)]], "c": [[(7, 2), (8, 2)]]}
    a, b, c, info = marlin.square_and_balance(to_csr(rows["a"]), to_csr(rows["b"]), to_csr(rows["c"]), 2, 2)
    # A is denser: row 0 is swapped, so B holds A's row, sorted by column with ties in the given order
    assert b[1].tolist() == [0, 1, 1, 3, 3] and b[2][:, 0].tolist() == [5, 2, 4, 1, 3]
    assert a[1].tolist() == [2] and c[1].tolist() == [2, 2] and c[2][:, 0].tolist() == [7, 8]
    assert info == {"num_variables": 4, "num_constraints": 4, "num_non_zero": 5, "num_instance_variables": 2}
    assert all(m[0].tolist() == [0, len(m[1])] + [len(m[1])] * 3 for m in (a, b, c))     # three empty rows appended


def test_witness_columns_shift_by_the_input_padding():
    rows = {"a": [[(1, 0), (2, 2), (3, 3), (4, 6)]], "b": [[]], "c": [[]]}
    a, b, _, info = marlin.square_and_balance(to_csr(rows["a"]), to_csr(rows["b"]), to_csr(rows["c"]), 3, 4)
    assert info["num_instance_variables"] == 4 and info["num_variables"] == 8
    assert b[1].tolist() == [0, 2, 4, 7]                   # (A, the denser one, went to B) inputs 0 and 2 stay, witnesses 0 and 3 sit at 4 + 0 and 4 + 3


@pytest.mark.parametrize("H,X", [(2, 2), (4, 2), (8, 1), (8, 8), (64, 4)])
def test_reindex_every_index(H, X):
    got = marlin.reindex(H, X, np.arange(H))
    assert got.tolist() == [naive_reindex(H, X, i) for i in range(H)]
    assert sorted(got.tolist()) == list(range(H))          # a permutation of H: every variable has its own position


def test_malformed_matrices_are_refused():
    good = to_csr([[(1, 0)], [(2, 1)]])
    with pytest.raises(ValueError):
        marlin.square_and_balance(good, good, to_csr([[(1, 0)]]), 1, 1)                        # C has fewer rows
    with pytest.raises(ValueError):
        marlin.square_and_balance(good, good, to_csr([[(1, 0)], [(2, 2)]]), 1, 1)              # column 2 of 2 variables
    bad = (np.array([0, 2, 1], dtype=np.uint64), good[1], good[2])
    with pytest.raises(ValueError):
        marlin.square_and_balance(bad, good, good, 1, 1)
