"""KZG10 on the GPU next to the polynomial provers: `KZG10::setup` with the toxic values passed in, `trim`, `check` and `batch_check`
(poly-commit/src/kzg10/mod.rs:39-138, 295-371, 452-477), and the verifier's side of a plonk_prove / marlin_prove result.

setup is built from czk_fr_powers (the powers of beta, on the device), one czk_fixed_base table per base and czk_fixed_base_msm -- the same
pieces as keygen.groth16_setup; check / batch_check are Context.kzg10_check / kzg10_batch_check (csrc/kzg.hip), the randomizers of batch_check
drawn here as the reference draws them: 1 for a batch's first opening, 128-bit values after it (mod.rs:333, :349-351).
"""
from __future__ import annotations

import secrets

import numpy as np

from . import binding as czk
from .keygen import R_MOD, _mont


class DegreeIsZero(ValueError):
    """Error::DegreeIsZero (poly-commit/src/error.rs): setup needs max_degree >= 1 (kzg10/mod.rs:44-46)"""


def _limbs(v: int) -> list:
    return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]


def setup(ctx, max_degree: int, beta: int, gamma: int, produce_g2_powers: bool = False, g=None, gamma_g=None, h=None, to_host: bool = True) -> dict:
    """KZG10::setup for the toxic value `beta`.  g, h: affine Montgomery limbs of the bases the reference draws at random (mod.rs:49-51); None = the
    group generators.  gamma_g: the hiding base; None = [gamma] g (`gamma` is not used otherwise).

    Returns a dict: "powers_of_g" = [beta^i] g for i <= max_degree and "powers_of_gamma_g" = [beta^i] gamma_g for i <= max_degree + 1 (one more:
    mod.rs:81-83), each as (points, infinity flags) -- numpy arrays, or torch tensors on the context's GPU with to_host=False; "h", "beta_h" (numpy);
    "neg_powers_of_h" = [beta^-i] h for i <= max_degree as such a pair with produce_g2_powers, else None; "max_degree".
    max_degree < 1 raises DegreeIsZero; beta = 0 with produce_g2_powers (the reference divides by it, :96) is ValueError."""
    max_degree = int(max_degree)
    if max_degree < 1:
        raise DegreeIsZero("max_degree must be at least 1")
    beta, gamma = int(beta) % R_MOD, int(gamma) % R_MOD
    if produce_g2_powers and beta == 0:
        raise ValueError("beta must be invertible to produce the negative powers of h")
    for name, base, width in (("g", g, 12), ("gamma_g", gamma_g, 12), ("h", h, 24)):
        if base is not None and np.asarray(base).size != width:
            raise ValueError(f"{name} must be {width} uint64 limbs")
    import torch
    dev = torch.device("cuda", ctx.device)
    dev_mem, mont_form = czk.CZK_MEM_DEVICE, czk.CZK_SCALAR_MONTGOMERY
    one = np.array([_limbs(1)], dtype=np.uint64)
    g = ctx.fixed_base_points(czk.CZK_G1, one)[0] if g is None else np.ascontiguousarray(g, np.uint64).reshape(12)
    h = ctx.fixed_base_points(czk.CZK_G2, one)[0] if h is None else np.ascontiguousarray(h, np.uint64).reshape(24)
    n = max_degree + 1
    pw = torch.empty((n + 1, 4), dtype=torch.int64, device=dev)                # beta^i, i <= max_degree + 1
    ctx.fr_powers(_mont(beta), n + 1, out=pw.data_ptr(), mem=dev_mem)

    def powers(fb, aw, src, count):
        pts = torch.empty((count, aw), dtype=torch.int64, device=dev)
        inf = torch.empty(count, dtype=torch.uint8, device=dev)
        ctx.fixed_base_msm(fb, src, out=pts.data_ptr(), n=count, scalar_form=mont_form, mem=dev_mem, out_inf=inf.data_ptr())
        return pts, inf

    pp = {"max_degree": max_degree, "h": h, "neg_powers_of_h": None}
    t = ctx.fixed_base(czk.CZK_G1, g, n_hint=n)
    try:
        pp["powers_of_g"] = powers(t, 12, pw.data_ptr(), n)
        if gamma_g is None:
            gamma_g, g_inf = (x[0] for x in ctx.fixed_base_msm(t, _mont(gamma).reshape(1, 4), scalar_form=mont_form))
            if g_inf:
                raise ValueError("gamma_g = [gamma] g is the point at infinity")
        else:
            gamma_g = np.ascontiguousarray(gamma_g, np.uint64).reshape(12)
    finally:
        ctx.sync()
        t.release()
    t = ctx.fixed_base(czk.CZK_G1, gamma_g, n_hint=n + 1)
    try:
        pp["powers_of_gamma_g"] = powers(t, 12, pw.data_ptr(), n + 1)
    finally:
        ctx.sync()
        t.release()
    t = ctx.fixed_base(czk.CZK_G2, h, n_hint=n if produce_g2_powers else 1)
    try:
        pp["beta_h"] = ctx.fixed_base_msm(t, _mont(beta).reshape(1, 4), scalar_form=mont_form)[0][0]
        if produce_g2_powers:
            ctx.fr_powers(_mont(pow(beta, -1, R_MOD)), n, out=pw.data_ptr(), mem=dev_mem)
            pp["neg_powers_of_h"] = powers(t, 24, pw.data_ptr(), n)
    finally:
        ctx.sync()
        t.release()
    if to_host:
        for name in ("powers_of_g", "powers_of_gamma_g", "neg_powers_of_h"):
            if pp[name] is not None:
                pts, inf = pp[name]
                pp[name] = (pts.cpu().numpy().view(np.uint64), inf.cpu().numpy())
    return pp


def trim(pp: dict, supported_degree: int):
    """(powers, vk) of a setup result, as the reference's trim (mod.rs:452-477): powers = {"powers_of_g", "powers_of_gamma_g"}, both cut to
    supported_degree + 1 entries (a supported degree of 1 is raised to 2, :456-458); vk = {"g", "gamma_g", "h", "beta_h"} as numpy limbs, the
    keyword arguments of Context.kzg10_vk."""
    d = int(supported_degree)
    if d == 1:
        d = 2
    if d < 1 or d > pp["max_degree"]:
        raise ValueError(f"supported_degree {supported_degree} is outside 1..{pp['max_degree']}")
    powers = {name: (pp[name][0][:d + 1], pp[name][1][:d + 1]) for name in ("powers_of_g", "powers_of_gamma_g")}

    def first(name):
        p = pp[name][0][0]
        return p.cpu().numpy().view(np.uint64) if hasattr(p, "data_ptr") else np.array(p, dtype=np.uint64)
    vk = {"g": first("powers_of_g"), "gamma_g": first("powers_of_gamma_g"), "h": np.array(pp["h"], dtype=np.uint64),
          "beta_h": np.array(pp["beta_h"], dtype=np.uint64)}
    return powers, vk


def _handle(ctx, vk):
    return ctx.kzg10_vk(**vk) if isinstance(vk, dict) else vk


def draw_randomizers(offsets, rng=None) -> np.ndarray:
    """One canonical randomizer per opening: 1 for the first opening of each batch, a 128-bit value for every other (mod.rs:333, :349-351).
    rng: an object with getrandbits (random.Random); None = the operating system's source."""
    offs = [int(x) for x in offsets]
    bits = secrets.randbits if rng is None else rng.getrandbits
    r = np.zeros((offs[-1] if offs else 0, 4), dtype=np.uint64)
    for lo, hi in zip(offs, offs[1:]):
        for i in range(lo, hi):
            r[i] = _limbs(1 if i == lo else bits(128))
    return r


def check(ctx, vk, comm, points, values, w, comm_inf=None, w_inf=None, random_v=None) -> np.ndarray:
    """KZG10::check of k openings -> (k,) bool.  vk: a Kzg10VerifierKey or trim's dict; the arrays as Context.kzg10_check takes them."""
    return ctx.kzg10_check(_handle(ctx, vk), comm, points, values, w, comm_inf=comm_inf, w_inf=w_inf, random_v=random_v)


def batch_check(ctx, vk, comm, points, values, w, offsets=None, comm_inf=None, w_inf=None, random_v=None, randomizers=None, rng=None) -> np.ndarray:
    """KZG10::batch_check -> one bool per batch.  offsets: batch j covers openings [offsets[j], offsets[j+1]); None = all openings in one batch.
    randomizers: (k, 4) canonical limbs; None = drawn by draw_randomizers(offsets, rng)."""
    k = np.asarray(comm).reshape(-1, 12).shape[0]
    offsets = [0, k] if offsets is None else offsets
    if randomizers is None:
        randomizers = draw_randomizers(offsets, rng)
    return ctx.kzg10_batch_check(_handle(ctx, vk), comm, points, values, w, randomizers, offsets, comm_inf=comm_inf, w_inf=w_inf, random_v=random_v)


def _folded_commitment(B, out, key):
    """sum_j coef_j C_j per lane for one of Marlin's folded openings (its "terms"), on the GPU: one czk_points_mul over every (lane, term), one
    czk_points_sum with a segment per lane.  A public polynomial enters a share-wise sum on the lifting lanes only."""
    o = out[key]
    lanes = o["value"].shape[0]
    pts, inf, ks, offs = [], [], [], [0]
    for ln in range(lanes):
        for coef, name in o["terms"]:
            cm = out[name + "_cmt"]
            public = cm[0].shape[0] == 1
            if not public or lanes == 1 or B.lift[ln]:
                l2 = 0 if public else ln
                pts.append(np.asarray(cm[0][l2], dtype=np.uint64))
                inf.append(int(cm[1][l2]))
                ks.append(_limbs(int(coef) % R_MOD))
        offs.append(len(pts))
    ctx = B.ctx
    prod, prod_inf = ctx.points_mul(czk.CZK_G1, np.array(pts, dtype=np.uint64).reshape(-1, 12), np.array(ks, dtype=np.uint64).reshape(-1, 4),
                                    inf=np.array(inf, dtype=np.uint8))
    return ctx.points_sum(czk.CZK_G1, prod, offs, inf=prod_inf)


def check_openings(B, out, rng=None, details: bool = False):
    """The verifier's KZG side of a plonk_prove / marlin_prove result `out` made on the GpuBackend `B`: every opening against its commitment through
    kzg10_batch_check under the verifier key of B's SRS (B.verifier_key(): no toxic value is used) -- one batch per opening, its lanes the batch's
    members; Marlin's two folded openings against sum_j coef_j C_j, the hiding ones with their random_v.  Returns True iff every batch verifies;
    details=True returns {opening label: bool} instead."""
    ctx = B.ctx
    groups = []   # (label, commitments, flags, opening)
    for label, o in out.items():
        if isinstance(o, dict) and o.get("of"):
            c = out[o["of"] + "_cmt"]
            groups.append((label, np.asarray(c[0], dtype=np.uint64), np.asarray(c[1], dtype=np.uint8), o))
    for label in ("open_beta", "open_gamma"):
        if label in out:
            c, c_inf = _folded_commitment(B, out, label)
            groups.append((label, c, c_inf, out[label]))
    comm, comm_inf, points, values, w, w_inf, random_v, offs = [], [], [], [], [], [], [], [0]
    for label, c, c_inf, o in groups:
        lanes = o["value"].shape[0]
        if c.shape[0] != lanes:
            raise ValueError(f"{label}: {c.shape[0]} commitments for {lanes} evaluations")
        comm.append(c.reshape(lanes, 12))
        comm_inf.append(c_inf.reshape(lanes))
        points.append(np.tile(_mont(int(o["point"])), (lanes, 1)))
        values.append(np.asarray(o["value"], dtype=np.uint64).reshape(lanes, 4))
        w.append(np.asarray(o["proof"][0], dtype=np.uint64).reshape(lanes, 12))
        w_inf.append(np.asarray(o["proof"][1], dtype=np.uint8).reshape(lanes))
        # an opening that is not hiding has no random_v: zero decides the same
        random_v.append(np.asarray(o["random_v"], dtype=np.uint64).reshape(lanes, 4) if "random_v" in o else np.zeros((lanes, 4), dtype=np.uint64))
        offs.append(offs[-1] + lanes)
    if not groups:
        return {} if details else True
    vk = ctx.kzg10_vk(*B.verifier_key())
    try:
        ok = batch_check(ctx, vk, np.concatenate(comm), np.concatenate(points), np.concatenate(values), np.concatenate(w), offsets=offs,
                         comm_inf=np.concatenate(comm_inf), w_inf=np.concatenate(w_inf), random_v=np.concatenate(random_v), rng=rng)
    finally:
        vk.release()
    return {g[0]: bool(v) for g, v in zip(groups, ok)} if details else bool(ok.all())
