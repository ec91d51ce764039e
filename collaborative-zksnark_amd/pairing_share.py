"""Pairings of shared points and the multiplicative target-group shares they yield, driven through the C ABI (binding.py; csrc/pairing_share.hip):
MpcPairingEngine::pairing (mpc-algebra/src/wire/pairing.rs:194-229) and the reference's PairingDh / PairingProd / PairingDiv computations
(mpc-snarks/src/client.rs:503-581).  Lanes form: every party's lanes are on one GPU, lane lpp p = party p's sh, lpp p + 1 its mac (SPDZ).

  SharedPairing   pairing (both operands shared, one pairing triple per element), pairing_public (one operand public), mul / div (lane-wise),
                  scale (by a public Fq12; from_public with no lanes), open (the product of the sh lanes, MAC-checked)
  pairing_dh, pairing_prod, pairing_div   the three computations on shared scalars; each returns its two opened sides, which the reference asserts equal

A share vector is a device tensor: scalars (L, n, 4) Montgomery Fr, G1 / G2 points ((L, n, 12 | 24) int64, (L, n) uint8 infinity bytes), target-group
shares (L, n, 72) int64.  A failed MAC check raises polyvm.SharingError.  torch provides device memory only."""
from __future__ import annotations

import importlib

import numpy as np
import torch

from .binding import CZK_FQ12_OP_DIV, CZK_FQ12_OP_MUL, CZK_G1, CZK_G2, CZK_MEM_DEVICE
from .polyvm import SharingError
from .provers import Groth16Local, _dev, to_mont_limbs


class SharedPairing:
    """lpp = 1 additive, lpp = 2 SPDZ shares of `parties` parties; mac_shares: the parties' shares of the MAC key as ints (None for lpp = 1);
    source: where pairing triples come from (provers.DummyGroupSource, provers.SeededGroupDealer: its pairing_triples(self, n)).  The object is also
    what a source asks for the sharing in use (lanes, lpp, P, mac_shares(), share_values, lift_lanes)."""

    share_values = Groth16Local.share_values     # a random sharing of ints in this lane order
    lift_lanes = Groth16Local.lift_lanes         # lanes of scalars -> lanes of [k] G

    def __init__(self, ctx, lpp: int, parties: int, mac_shares=None, source=None):
        assert lpp in (1, 2) and (lpp == 1 or len(mac_shares) == parties)
        self.czk, self.ctx, self.lpp, self.P, self.source = importlib.import_module(__package__), ctx, lpp, parties, source
        self.scheme, self.lanes, self.king_lanes = ("spdz" if lpp == 2 else "hbc"), lpp * parties, list(range(lpp))
        self._mac = None if lpp == 1 else [int(m) for m in mac_shares]
        self._mac_limbs = None if lpp == 1 else to_mont_limbs(self._mac)

    def mac_shares(self):
        return self._mac or [0] * self.P

    def share_scalars(self, values, rng):
        """a random sharing of the ints in `values` -> (L, n, 4) device tensor of Montgomery lanes"""
        return _dev(np.stack([to_mont_limbs(ln) for ln in self.share_values(values, rng)]))

    def _gt(self, n):
        return torch.empty((self.lanes, n, 72), dtype=torch.int64, device="cuda")

    # ---- pairings ------------------------------------------------------------------------------------------------------------------------------
    def pairing(self, a, a_inf, b, b_inf):
        """e(a, b) for shared a (G1) and shared b (G2): one pairing triple per element from the source -> target-group shares (L, n, 72)"""
        n = a.shape[1]
        tx, tx_inf, ty, ty_inf, tz = self.source.pairing_triples(self, n)
        out = self._gt(n)
        p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
        bad = self.ctx.share_pairing(self.lpp, self.P, self._mac_limbs, p(a), p(a_inf), p(b), p(b_inf), p(tx), p(tx_inf), p(ty), p(ty_inf), p(tz), p(out), n)
        if bad:
            raise SharingError(f"pairing: the MAC check of an opened point failed for {bad} element(s)")
        return out

    def pairing_public(self, shared, shared_inf, public, public_inf=None, shared_group: int = CZK_G1):
        """e of a shared point with a PUBLIC one ((n, 12 | 24) host limbs): every lane is paired with the public point through czk_pairing, so by
        bilinearity the lanes are multiplicative shares of the pairing (the mac lanes of its key-th power) and nothing is revealed; the reference
        reveals both operands here (pairing.rs:226-228).  shared_group: the group of the shared operand."""
        L, n = shared.shape[0], shared.shape[1]
        sw, pw = (12, 24) if shared_group == CZK_G1 else (24, 12)
        s = shared.cpu().numpy().view(np.uint64).reshape(L * n, sw)
        si = None if shared_inf is None else shared_inf.cpu().numpy().reshape(L * n)
        pub = np.tile(np.ascontiguousarray(public, np.uint64).reshape(1, n, pw), (L, 1, 1)).reshape(L * n, pw)
        pi = None if public_inf is None else np.tile(np.ascontiguousarray(public_inf, np.uint8).reshape(1, n), (L, 1)).reshape(L * n)
        gt = self.ctx.pairing(s, pub, si, pi) if shared_group == CZK_G1 else self.ctx.pairing(pub, s, pi, si)
        return _dev(gt.reshape(L, n, 72))

    # ---- target-group share arithmetic ------------------------------------------------------------------------------------------------------------
    def _vec(self, op, x, y):
        out = torch.empty_like(x)
        self.ctx.fq12_vec_op(op, x.data_ptr(), y.data_ptr(), n=x.shape[0] * x.shape[1], out=out.data_ptr(), mem=CZK_MEM_DEVICE)
        self.ctx.sync()                                        # the operands may be dropped by the caller: they are read in stream order
        return out

    def mul(self, x, y):
        """lane-wise product: shares of the product of the values (both lanes, where the reference's SPDZ form drops its products)"""
        return self._vec(CZK_FQ12_OP_MUL, x, y)

    def div(self, x, y):
        return self._vec(CZK_FQ12_OP_DIV, x, y)

    def scale(self, v, f):
        """v scaled by the public f ((n, 72) host limbs); v None: from_public(f)"""
        f = _dev(np.ascontiguousarray(f, np.uint64).reshape(-1, 72))
        out = self._gt(f.shape[0])
        self.ctx.gt_share_scale(self.lpp, self.P, self._mac_limbs, None if v is None else v.data_ptr(), f.data_ptr(), out.data_ptr(), f.shape[0])
        self.ctx.sync()                                        # `f` is read in stream order
        return out

    def open(self, v):
        """reveal -> (n, 72) host limbs; raises when a MAC check fails"""
        n = v.shape[1]
        out = torch.empty((n, 72), dtype=torch.int64, device="cuda")
        bad = self.ctx.gt_share_open(self.lpp, self.P, self._mac_limbs, v.data_ptr(), n, out.data_ptr())
        if bad:
            raise SharingError(f"open: the MAC check failed for {bad} element(s)")
        return out.cpu().numpy().view(np.uint64)

    # ---- lane-wise sums of shared points (MPC group addition is local) --------------------------------------------------------------------------------
    def points_add(self, group, a, a_inf, b, b_inf, negate_b: bool = False):
        out, out_inf = torch.empty_like(a), torch.empty_like(a_inf)
        self.ctx.points_add(group, a.data_ptr(), b.data_ptr(), a_inf.data_ptr(), b_inf.data_ptr(), negate_b, n=a.shape[0] * a.shape[1], out=out.data_ptr(),
                            out_inf=out_inf.data_ptr(), mem=CZK_MEM_DEVICE)
        self.ctx.sync()
        return out, out_inf


def _generator(sp, group, n):
    return np.tile(sp.ctx.fixed_base_points(group, np.array([[1, 0, 0, 0]], np.uint64))[0].reshape(1, -1), (n, 1))


def pairing_dh(sp: SharedPairing, a, b, c):
    """PairingDh (client.rs:503-519) on shared scalars a, b, c ((L, n, 4) lanes): -> (open e([c] G1, G2), open e([a] G1, [b] G2)); equal when c = a b"""
    n = a.shape[1]
    g1a, g2b, g1c = sp.lift_lanes(CZK_G1, a), sp.lift_lanes(CZK_G2, b), sp.lift_lanes(CZK_G1, c)
    gc = sp.open(sp.pairing_public(g1c[0], g1c[1], _generator(sp, CZK_G2, n)))
    return gc, sp.open(sp.pairing(g1a[0], g1a[1], g2b[0], g2b[1]))


def _four(sp, a, b, c, d, negate: bool):
    """e([a +- b] G1, [c +- d] G2) against e(a, c) e(b, c)^+-1 e(a, d)^+-1 e(b, d), both opened"""
    g1a, g1b, g2c, g2d = sp.lift_lanes(CZK_G1, a), sp.lift_lanes(CZK_G1, b), sp.lift_lanes(CZK_G2, c), sp.lift_lanes(CZK_G2, d)
    g1ab, g2cd = sp.points_add(CZK_G1, *g1a, *g1b, negate_b=negate), sp.points_add(CZK_G2, *g2c, *g2d, negate_b=negate)
    whole = sp.pairing(*g1ab, *g2cd)
    op = sp.div if negate else sp.mul
    parts = sp.mul(op(op(sp.pairing(*g1a, *g2c), sp.pairing(*g1b, *g2c)), sp.pairing(*g1a, *g2d)), sp.pairing(*g1b, *g2d))
    return sp.open(whole), sp.open(parts)


def pairing_prod(sp: SharedPairing, a, b, c, d):
    """PairingProd (client.rs:520-550): -> (open e([a + b] G1, [c + d] G2), open of e(a, c) e(b, c) e(a, d) e(b, d))"""
    return _four(sp, a, b, c, d, False)


def pairing_div(sp: SharedPairing, a, b, c, d):
    """PairingDiv (client.rs:551-581): -> (open e([a - b] G1, [c - d] G2), open of e(a, c) / e(b, c) / e(a, d) * e(b, d))"""
    return _four(sp, a, b, c, d, True)
