"""The "czk tree commitment v1" of include/czk.h in hashlib (TEST INFRASTRUCTURE ONLY): what czk_fr_vec_commit must produce.

`canon` is the vector's canonical bytes -- 32 little-endian bytes of into_repr() per element, czk_fr_vec_serialize's payload -- as bytes or an
(n, 4) uint64 array of canonical limbs.  E elements per leaf, F digests per node."""
import hashlib

import numpy as np

TAG_LEAF, TAG_NODE, TAG_ROOT = (("czk-commit-v1/" + k).encode("ascii").ljust(64, b"\0") for k in ("leaf", "node", "root"))


def _h(*parts) -> bytes:
    return hashlib.sha256(b"".join(parts)).digest()


def top_digest(canon, E: int, F: int) -> bytes:
    data = np.ascontiguousarray(canon, dtype="<u8").tobytes() if isinstance(canon, np.ndarray) else bytes(canon)
    assert len(data) % 32 == 0
    level = [_h(TAG_LEAF, data[i:i + 32 * E]) for i in range(0, len(data), 32 * E)] or [_h(TAG_LEAF)]
    while len(level) > 1:
        level = [_h(TAG_NODE, *level[j:j + F]) for j in range(0, len(level), F)]
    return level[0]


def commit(canon, rand32: bytes, E: int, F: int) -> bytes:
    n = (canon.size // 4) if isinstance(canon, np.ndarray) else len(canon) // 32
    assert len(rand32) == 32
    return _h(TAG_ROOT, n.to_bytes(8, "little"), top_digest(canon, E, F), rand32)
