"""tests/merkle_fri_model.py -- the hashlib / big-integer model that czk_fr_merkle_* , czk_fr_fri_fold and czk_amd.fri are held to on the GPU
(tests/test_merkle_fri.py) -- against cases assembled by hand from com.rs and client.rs, and the new entry points' presence in the header and the library.
No GPU."""
import hashlib
import os
import random
import sys

import pytest

import merkle_fri_model as M
from merkle_fri_model import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("czk_fr_merkle_commit", "czk_fr_merkle_open", "czk_fr_merkle_verify", "czk_fr_fri_fold")


def H(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def le(v: int) -> bytes:
    return v.to_bytes(32, "little")


def rand_lanes(seed, parties, n):
    rng = random.Random(seed)
    return [[rng.randrange(R_MOD) for _ in range(n)] for _ in range(parties)]


# ---- the tree, the path, the check ---------------------------------------------------------------------------------------------------
def test_trees_of_one_two_and_four_leaves_by_hand():
    a, b, c, d = 0, 1, R_MOD - 1, 0x0123456789ABCDEF << 190
    assert M.elem_bytes(R_MOD - 1) == le(R_MOD - 1) and M.elem_bytes(1) == b"\x01" + bytes(31)
    assert M.tree_levels([c]) == [[H(le(c))]]                                      # n = 1: the one leaf hash
    assert M.tree_bytes(M.tree_levels([c])) == H(le(c)) and M.path(M.tree_levels([c]), 0) == []
    la, lb, lc, ld = (H(le(v)) for v in (a, b, c, d))
    assert M.tree_levels([a, b]) == [[la, lb], [H(la + lb)]]
    n01, n23 = H(la + lb), H(lc + ld)
    t4 = M.tree_levels([a, b, c, d])
    assert t4 == [[la, lb, lc, ld], [n01, n23], [H(n01 + n23)]]
    assert M.tree_bytes(t4) == la + lb + lc + ld + n01 + n23 + H(n01 + n23)        # 2n - 1 digests: level 1 at offset n, the root at 2n - 2
    assert len(M.tree_bytes(t4)) == 7 * 32
    with pytest.raises(AssertionError):
        M.tree_levels([a, b, c])                                                   # the reference asserts a power of two


def test_paths_at_the_first_and_the_last_index_and_the_side_at_each_bit():
    vals = rand_lanes(1, 1, 8)[0]
    lv = M.tree_levels(vals)
    leaf = [H(le(v)) for v in vals]
    n2 = [H(leaf[2 * i] + leaf[2 * i + 1]) for i in range(4)]
    n4 = [H(n2[0] + n2[1]), H(n2[2] + n2[3])]
    root = H(n4[0] + n4[1])
    assert lv[-1] == [root]
    assert M.path(lv, 0) == [leaf[1], n2[1], n4[1]]
    assert M.path(lv, 7) == [leaf[6], n2[2], n4[0]]
    assert M.path(lv, 5) == [leaf[4], n2[3], n4[0]]                                # 5 = 0b101: right, left, right
    # the walk of check_opening, by hand for index 5: bit 0 set -> sibling first; bit 1 clear -> hash first; bit 2 set -> sibling first
    h = H(leaf[4] + leaf[5])
    h = H(h + n2[3])
    assert H(n4[0] + h) == root
    for i in range(8):
        assert M.check_opening([root], [vals[i]], [M.path(lv, i)], i, vals[i])
        for wrong in range(8):                                                     # the same path under another index: a flipped bit swaps a side
            if wrong != i:
                assert not M.check_opening([root], [vals[i]], [M.path(lv, i)], wrong, vals[i])


@pytest.mark.parametrize("parties", [2, 3])
def test_open_and_check_and_every_tampering_is_rejected(parties):
    lanes = rand_lanes(2 + parties, parties, 16)
    trees, roots = M.commit(lanes)
    for i in (0, 9, 15):
        value, shares, paths = M.open_at(lanes, trees, i)
        assert value == sum(v[i] for v in lanes) % R_MOD and shares == [v[i] for v in lanes]
        assert M.check_opening(roots, shares, paths, i, value) and M.check_opening(roots, shares, paths, i, None)
        for ln in range(parties):
            bad = list(shares)
            bad[ln] = (bad[ln] + 1) % R_MOD
            assert not M.check_opening(roots, bad, paths, i, value)                           # a share (the sum breaks) ...
            assert not M.check_opening(roots, bad, paths, i, (value + 1) % R_MOD)            # ... and with the value moved along, its path
            for level in (0, 3):
                p2 = [list(p) for p in paths]
                p2[ln][level] = bytes([p2[ln][level][0] ^ 1]) + p2[ln][level][1:]
                assert not M.check_opening(roots, shares, p2, i, value)                       # a sibling, lowest and highest level
            r2 = list(roots)
            r2[ln] = r2[ln][:31] + bytes([r2[ln][31] ^ 0x80])
            assert not M.check_opening(r2, shares, paths, i, value)                           # a root
        assert not M.check_opening(roots, shares, paths, i, (value + 1) % R_MOD)              # the value
        # shares that keep the sum but move between the parties: the sum holds, the paths do not
        moved = [(shares[0] + 5) % R_MOD, (shares[1] - 5) % R_MOD] + shares[2:]
        assert not M.check_opening(roots, moved, paths, i, value)


def test_commitment_bytes_of_two_parties_is_the_reference_pair():
    r0, r1 = H(b"party 0"), H(b"party 1")
    want = (32).to_bytes(8, "little") + r1 + (32).to_bytes(8, "little") + r0            # (Vec<u8>, Vec<u8>) = (other, slf) on party 0 (com.rs:62-66)
    assert M.commitment_bytes([r0, r1]) == want and len(want) == 80
    r2 = H(b"party 2")
    assert M.commitment_bytes([r0, r1, r2]) == b"".join((32).to_bytes(8, "little") + r for r in (r0, r1, r2))
    sys.path.insert(0, ROOT)
    from czk_amd import fri
    assert fri.commitment_bytes([r0, r1]) == want and fri.commitment_bytes([r0, r1, r2]) == M.commitment_bytes([r0, r1, r2])


# ---- FRI -----------------------------------------------------------------------------------------------------------------------------
def challenge(i, roots):
    return int.from_bytes(H(b"alpha" + bytes([i]) + b"".join(roots)), "little") % R_MOD


def test_root_of_unity_fft_and_fold():
    assert pow(M.TWO_ADIC_ROOT, 1 << 47, R_MOD) == 1 and pow(M.TWO_ADIC_ROOT, 1 << 46, R_MOD) == R_MOD - 1
    assert M.root_of_unity(1) == 1 and M.root_of_unity(2) == R_MOD - 1
    assert pow(M.LARGE_ROOT, 3 << 47, R_MOD) == 1 and pow(M.LARGE_ROOT, 1 << 47, R_MOD) != 1 and pow(M.LARGE_ROOT, 3 << 46, R_MOD) != 1
    assert M.root_of_unity(16) != pow(22, (R_MOD - 1) >> 4, R_MOD)                  # not the root TWO_ADIC_ROOT_OF_UNITY would give (they part at order 16)
    w = M.root_of_unity(8)
    c = rand_lanes(7, 1, 5)[0]
    assert M.fft(c, 8) == [sum(ci * pow(w, i * j, R_MOD) for i, ci in enumerate(c)) % R_MOD for j in range(8)]
    assert M.fold([1, 2, 3, 4], 10) == [21, 43] and M.fold([5, 6], 0) == [5] and M.fold([5, 6], R_MOD - 1) == [R_MOD - 1]
    # the index rule of client.rs:795: ((2 x) mod n) / 2 = x mod (n / 2)
    for n in (2, 4, 32):
        for x in range(n):
            assert 2 * x % n // 2 == x % (n // 2)
    assert M.chain_indices(2, [5]) == [[5, 1], [1, 3, 1]]


@pytest.mark.parametrize("parties", [2, 3])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_fri_accepts_an_honest_run_at_every_start_index(parties, k):
    f = rand_lanes(100 * parties + k, parties, 1 << k)
    state = M.commit_phase(f, challenge)
    assert len(state["rounds"]) == k and state["lanes"] == parties
    # the constant is the polynomial folded all the way, in the open
    g = [sum(col) % R_MOD for col in zip(*f)]
    for i, rd in enumerate(state["rounds"]):
        assert rd["n"] == 2 * len(g) and rd["alpha"] == challenge(i, rd["roots"])
        g = M.fold(g, rd["alpha"])
    assert g == [state["constant"]]
    starts = list(range(1 << (k + 1)))
    proof = M.query_phase(state, starts)
    assert M.verify(proof, challenge)
    for rd, i in zip(proof["rounds"], range(k)):
        assert len(rd["idx"]) == (3 if i else 2) * len(starts) and all(len(p[0]) == k + 1 - i for p in rd["paths"])


@pytest.mark.parametrize("k", [1, 3, 4])
def test_fri_rejects_a_wrong_alpha_a_long_vector_and_tampering(k):
    parties, starts = 2, list(range(1 << (k + 1)))
    f = rand_lanes(50 + k, parties, 1 << k)
    # folded with another alpha than the challenge: every path holds, the relation fails
    state = M.commit_phase(f, challenge, fold_alpha=lambda i, a: a + 1 if i == k - 1 else a)
    proof = M.query_phase(state, starts)
    assert all(M.check_opening(roots, s, p, j, v) for rd, roots in zip(proof["rounds"], proof["roots"])
               for j, v, s, p in zip(rd["idx"], rd["values"], rd["shares"], rd["paths"]))
    assert not M.verify(proof, challenge)
    # ... and the verifier with another challenge than the prover's
    honest = M.query_phase(M.commit_phase(f, challenge), starts)
    assert M.verify(honest, challenge) and not M.verify(honest, lambda i, roots: challenge(i, roots) + (i == 0))
    # one coefficient too many, committed in full and folded as if it fitted: rejected at a start index (the low-degree test)
    long_f = [lane + [1 + ln] for ln, lane in enumerate(f)]
    cheat = M.query_phase(M.commit_phase(f, challenge, committed_lanes=long_f), starts)
    assert not M.verify(cheat, challenge)
    assert any(not M.verify(M.query_phase(M.commit_phase(f, challenge, committed_lanes=long_f), [x]), challenge) for x in starts)
    # a proof that was changed afterwards
    for what in ("value", "constant", "root", "idx"):
        p = M.query_phase(M.commit_phase(f, challenge), starts)
        if what == "value":
            p["rounds"][0]["values"][1] = (p["rounds"][0]["values"][1] + 1) % R_MOD
        elif what == "constant":
            p["constant"] = (p["constant"] + 1) % R_MOD
        elif what == "root":
            p["roots"][k - 1][0] = H(p["roots"][k - 1][0])
        else:
            p["rounds"][0]["idx"][0] ^= 1
        assert not M.verify(p, challenge), what


# ---- the library's surface -------------------------------------------------------------------------------------------------------------
def test_the_four_entry_points_are_declared_and_exported():
    sys.path.insert(0, ROOT)
    import czk_amd
    for sym in SYMBOLS:
        assert sym in czk_amd.header_symbols(), sym
        assert sym in czk_amd.exported_symbols(), sym
    rust = open(os.path.join(ROOT, "rust", "czk-sys", "src", "lib.rs")).read()
    for sym in SYMBOLS:
        assert f"pub fn {sym}(" in rust
    for name in ("fr_merkle_commit", "fr_merkle_open", "fr_merkle_verify", "fri_fold"):
        assert callable(getattr(czk_amd.Context, name))
    assert czk_amd.fri.chain_indices(2, [5]) == M.chain_indices(2, [5]) and czk_amd.fri.root_of_unity(8) == M.root_of_unity(8)
