"""Fiat-Shamir transcripts: the reference's FiatShamirRng<Blake2s> (marlin/src/rng.rs, mpc-plonk/src/util.rs:44-108) over czk_fs (include/czk.h, csrc/fs.hip).

    t = Transcript()                      # state in host memory, no GPU needed: what a verifier uses
    t = Transcript(ctx, device=True)      # state in device memory, every operation a kernel on the context's stream

A message is put piece by piece -- bytes, Fr elements, affine points, written as the reference's ToBytes -- and closed by seed() (FiatShamirRng::from_seed)
or absorb() (FiatShamirRng::absorb).  Draws: squeeze_fr (Fr::rand), squeeze_u64, squeeze_u128.  Integers in and out are canonical; the limb arrays the
library's calls take (Montgomery form) go through put_fr / put_points as they are.
"""
from __future__ import annotations

import numpy as np

from .binding import CZK_G1, CZK_G2, Fs

R_MOD = 0x12ab655e9a2ca55660b44d1e5c37b00159aa76fed00000010a11800000000001
_MONT_R = (1 << 256) % R_MOD
_MONT_R_INV = pow(1 << 256, -1, R_MOD)


def _limbs(v: int) -> list:
    return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]


class Transcript:
    def __init__(self, ctx=None, device: bool = False):
        self.fs = Fs(ctx, device)
        self.device = bool(device)

    # ---- the pending message ------------------------------------------------------------------------------------------------------------------
    def put_bytes(self, data, n: int | None = None):
        """bytes or a uint8 array; or a device pointer and its byte count"""
        self.fs.put_bytes(data, n)
        return self

    def put_u64(self, *values: int):
        """u64::write: 8 little-endian bytes each"""
        return self.put_bytes(b"".join(int(v).to_bytes(8, "little") for v in values))

    def put_bool(self, value: bool):
        return self.put_bytes(b"\x01" if value else b"\x00")

    def put_fr(self, v, n: int | None = None):
        """(n, 4) Montgomery limbs (a numpy array, or a device pointer with n); or a list of canonical integers"""
        if isinstance(v, (list, tuple)):
            v = np.array([_limbs(int(x) % R_MOD * _MONT_R % R_MOD) for x in v], dtype=np.uint64).reshape(-1, 4)
        self.fs.put_fr(v, n)
        return self

    def put_points(self, group: int, pts, inf=None, n: int | None = None):
        """affine points in the library's layout, (n, 12) for CZK_G1 or (n, 24) for CZK_G2 Montgomery limbs, with their infinity flags (None: none)"""
        if group not in (CZK_G1, CZK_G2):
            raise ValueError("group is CZK_G1 or CZK_G2")
        self.fs.put_points(group, pts, inf, n)
        return self

    def seed(self):
        self.fs.seed()
        return self

    def absorb(self):
        self.fs.absorb()
        return self

    # ---- draws ----------------------------------------------------------------------------------------------------------------------------------
    def squeeze_fr_mont(self, n: int = 1, out: int | None = None):
        """n draws as (n, 4) Montgomery limbs, or into device memory at `out` (only enqueued)"""
        return self.fs.squeeze_fr(n, out)

    def squeeze_fr(self, n: int | None = None):
        """Fr::rand: one canonical integer, or a list of n"""
        a = self.fs.squeeze_fr(1 if n is None else n)
        vals = [sum(int(row[j]) << (64 * j) for j in range(4)) * _MONT_R_INV % R_MOD for row in a]
        return vals[0] if n is None else vals

    def squeeze_u64(self, n: int | None = None, out: int | None = None):
        if out is not None:
            return self.fs.squeeze_u64(n or 1, out)
        a = self.fs.squeeze_u64(1 if n is None else n)
        return int(a[0]) if n is None else [int(x) for x in a]

    def squeeze_u128(self, n: int | None = None):
        """u128::rand (rand 0.7): two next_u64, low first"""
        a = self.fs.squeeze_u64(2 * (1 if n is None else n))
        vals = [int(a[2 * i]) | int(a[2 * i + 1]) << 64 for i in range(a.size // 2)]
        return vals[0] if n is None else vals

    def state(self):
        """(seed, generator position in 32-bit keystream words); blocks for a device transcript"""
        return self.fs.state()

    def release(self):
        self.fs.release()
