"""The tree commitment's model (tests/commit_tree_model.py) against cases assembled by hand from include/czk.h's text, the three tags, and the
constants of the format in czk.h, binding.py and rust/czk-sys.  No GPU."""
import hashlib
import os
import re
import sys

import pytest

import commit_tree_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sha(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def _elem(i: int) -> bytes:
    """32 canonical little-endian bytes, different for every i"""
    return (0x0123456789ABCDEF0FEDCBA987654321 * (i + 1) + i).to_bytes(32, "little")


def _tag(s: str) -> bytes:
    return s.encode("ascii") + bytes(64 - len(s))


LEAF, NODE, ROOT_TAG = _tag("czk-commit-v1/leaf"), _tag("czk-commit-v1/node"), _tag("czk-commit-v1/root")


def test_tags_are_one_sha256_block_each():
    assert (model.TAG_LEAF, model.TAG_NODE, model.TAG_ROOT) == (LEAF, NODE, ROOT_TAG)
    assert all(len(t) == 64 for t in (model.TAG_LEAF, model.TAG_NODE, model.TAG_ROOT))
    assert model.TAG_LEAF[:18] == b"czk-commit-v1/leaf" and model.TAG_LEAF[18:] == bytes(46)
    assert len({model.TAG_LEAF, model.TAG_NODE, model.TAG_ROOT}) == 3


@pytest.mark.parametrize("E,F", [(32, 32), (8, 8), (16, 64)])
def test_model_matches_hand_assembled_cases(E, F):
    rnd = bytes(range(100, 132))

    def root(n, top):
        return _sha(ROOT_TAG + n.to_bytes(8, "little") + top + rnd)
    # n = 0: the one leaf is the hash of the tag alone
    assert model.commit(b"", rnd, E, F) == root(0, _sha(LEAF))
    # one element; exactly one full leaf: a single leaf is the top, there is no node level
    assert model.commit(_elem(0), rnd, E, F) == root(1, _sha(LEAF + _elem(0)))
    full = b"".join(_elem(i) for i in range(E))
    assert model.commit(full, rnd, E, F) == root(E, _sha(LEAF + full))
    # E + 1 elements: two leaves (the second of one element) under one node
    more = full + _elem(E)
    assert model.commit(more, rnd, E, F) == root(E + 1, _sha(NODE + _sha(LEAF + full) + _sha(LEAF + _elem(E))))
    # (and one past a full node: F + 1 leaves -> two nodes -> one node above them)
    big = b"".join(_elem(i) for i in range(E * F + 1))
    leaves = [_sha(LEAF + big[k:k + 32 * E]) for k in range(0, len(big), 32 * E)]
    assert len(leaves) == F + 1
    top = _sha(NODE + _sha(NODE + b"".join(leaves[:F])) + _sha(NODE + leaves[F]))
    assert model.commit(big, rnd, E, F) == root(E * F + 1, top)
    # the randomness and the length are part of the root
    assert model.commit(more, bytes(32), E, F) != model.commit(more, rnd, E, F)
    assert model.commit(more[:-32], rnd, E, F) != model.commit(more, rnd, E, F)


def test_model_takes_limb_arrays():
    import numpy as np
    vals = [int.from_bytes(_elem(i), "little") for i in range(40)]
    limbs = np.array([[(v >> (64 * j)) & (2**64 - 1) for j in range(4)] for v in vals], dtype=np.uint64)
    assert model.commit(limbs, bytes(32), 32, 32) == model.commit(b"".join(_elem(i) for i in range(40)), bytes(32), 32, 32)


def test_header_binding_and_rust_agree_on_the_constants():
    sys.path.insert(0, ROOT)
    import czk_amd
    hdr = open(os.path.join(ROOT, "include", "czk.h")).read()
    rust = open(os.path.join(ROOT, "rust", "czk-sys", "src", "lib.rs")).read()
    for name in ("CZK_COMMIT_LEAF_ELEMS", "CZK_COMMIT_FANOUT", "CZK_OPEN_COMMIT_TREE"):
        h = int(re.search(r"^#define %s (\d+)\s*$" % name, hdr, re.M).group(1))
        r = int(re.search(r"pub const %s: c_int = (\d+);" % name, rust).group(1))
        assert h == r == getattr(czk_amd.binding, name), name
    E, F = czk_amd.binding.CZK_COMMIT_LEAF_ELEMS, czk_amd.binding.CZK_COMMIT_FANOUT
    assert E >= 8 and F >= 8 and E & (E - 1) == 0 and F & (F - 1) == 0
    assert czk_amd.binding.CZK_OPEN_COMMIT_TREE == 2 and czk_amd.binding.CZK_OPEN_COMMIT == 1
    assert czk_amd.binding.open_commit_flags("tree") & 2 and czk_amd.binding.open_commit_flags(True) == 1 and czk_amd.binding.open_commit_flags(False) == 0
    for sym in ("czk_fr_vec_commit", "czk_net_atomic_broadcast_tree"):
        assert sym in czk_amd.header_symbols()
