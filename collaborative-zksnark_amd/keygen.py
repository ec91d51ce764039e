"""Groth16 key generation on the GPU: `generate_parameters` (groth16/src/generator.rs:33-230) for an R1CS given as CSR matrices.

Everything of size O(constraints) stays on the device: the Lagrange coefficients u_j = L_j(tau) (czk_fr_lagrange_coefficients), the QAP
evaluation a_i = sum_j A[j][i] u_j -- instance_map_with_evaluation (groth16/src/r1cs_to_qap.rs:51-93) is the product of the TRANSPOSED
constraint matrices with u, so the transposes are registered as czk_r1cs_matrix and run through czk_r1cs_matvec -- the scalar vectors
(czk_fr_lincomb, czk_fr_vec_scale, czk_fr_powers) and the six queries (czk_fixed_base_msm: FixedBaseMSM over one table per group).  The host
transposes the CSR index arrays, inverts gamma and delta, and multiplies the six single points of the key.
"""
from __future__ import annotations

import numpy as np

from . import binding as czk

R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041


def _mont(v: int) -> np.ndarray:
    """canonical integer -> (4,) uint64 Montgomery limbs"""
    return np.frombuffer(((v % R_MOD) * (1 << 256) % R_MOD).to_bytes(32, "little"), dtype=np.uint64).copy()


def csr_transpose(row_ptr, col_idx, coeff, n_cols: int):
    """CSR (row_ptr (m + 1,), col_idx (nnz,), coeff (nnz, 4)) of an m x n_cols matrix -> the CSR of its transpose (n_cols rows; the column indices
    of the result are the row numbers of the input, ascending within a row).  Entries are moved, never merged: a column index that occurs twice
    in a row gives two entries in the transpose."""
    row_ptr = np.asarray(row_ptr, dtype=np.uint64)
    col_idx = np.asarray(col_idx, dtype=np.uint32).reshape(-1)
    coeff = np.asarray(coeff, dtype=np.uint64).reshape(-1, 4)
    m, nnz = row_ptr.size - 1, col_idx.size
    if m < 0 or int(row_ptr[0]) != 0 or int(row_ptr[-1]) != nnz or coeff.shape[0] != nnz or np.any(row_ptr[1:] < row_ptr[:-1]):
        raise ValueError("malformed CSR matrix")
    if nnz and int(col_idx.max()) >= n_cols:
        raise ValueError("column index outside the matrix")
    rows = np.repeat(np.arange(m, dtype=np.uint32), np.diff(row_ptr.astype(np.int64)))
    order = np.argsort(col_idx, kind="stable")
    t_ptr = np.zeros(n_cols + 1, dtype=np.uint64)
    t_ptr[1:] = np.cumsum(np.bincount(col_idx, minlength=n_cols)[:n_cols])
    return t_ptr, np.ascontiguousarray(rows[order]), np.ascontiguousarray(coeff[order])


def groth16_setup(ctx, A, B, C, num_instance: int, num_witness: int, toxic, g1_base=None, g2_base=None, to_host: bool = True):
    """generate_parameters for the R1CS (A, B, C): each matrix a CSR triple (row_ptr, col_idx, coeff) as czk_r1cs_matrix_register takes it (one row per
    constraint, columns = variables [instance | witness], coeff Montgomery limbs).  toxic = (tau, alpha, beta, gamma, delta) as integers.  g1_base /
    g2_base: affine Montgomery limbs of the bases the reference draws at random (generator.rs:106-107); None = the group generators.

    Returns a dict: the queries "a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "gamma_abc_g1" as (points, infinity flags) -- numpy arrays,
    or torch tensors on the context's GPU with to_host=False -- the single points "alpha_g1", "beta_g1", "delta_g1", "beta_g2", "gamma_g2", "delta_g2"
    (numpy), and "vk": the keyword arguments of Context.groth16_pvk.  b queries of variables without a B term are infinity (flag 1).

    Errors follow the reference: a domain beyond 2^47 (PolynomialDegreeTooLarge) is CzkError CZK_ERR_SIZE; tau inside the domain, where the
    reference divides by Z(tau) = 0, and gamma or delta = 0 (UnexpectedIdentity, generator.rs:89-90) are ValueError."""
    import torch
    tau, alpha, beta, gamma, delta = (int(v) % R_MOD for v in toxic)
    ni, nv = int(num_instance), int(num_instance) + int(num_witness)
    m = len(A[0]) - 1
    if len(B[0]) - 1 != m or len(C[0]) - 1 != m:
        raise ValueError("A, B and C must have one row per constraint")
    dsize = m + ni                                                     # generator.rs:65
    log_d = max(dsize - 1, 0).bit_length()
    if log_d > 47:
        raise czk.CzkError(1, "domain larger than 2^TWO_ADICITY (PolynomialDegreeTooLarge, generator.rs:66)")
    D = 1 << log_d
    zt = (pow(tau, D, R_MOD) - 1) % R_MOD                             # evaluate_vanishing_polynomial
    if zt == 0:
        raise ValueError("tau lies in the evaluation domain: Z(tau) = 0")
    if gamma == 0 or delta == 0:
        raise ValueError("gamma and delta must be invertible (UnexpectedIdentity)")
    g_inv, d_inv = pow(gamma, -1, R_MOD), pow(delta, -1, R_MOD)
    dev_mem, host_scalar = czk.CZK_MEM_DEVICE, czk.CZK_MEM_DEVICE | czk.CZK_MEM_SCALAR_HOST

    # one zero-filled device allocation: u | a | b | c | lin | scaled (gamma_abc, l) | h
    off, total = {}, 0
    for name, size in (("u", dsize), ("a", nv), ("b", nv), ("c", nv), ("lin", nv), ("sc", nv), ("h", max(D - 1, 0))):
        off[name], total = total, total + size
    lanes = ctx.lanes_alloc(1, max(total, 1))
    mats = []
    try:
        p = {k: lanes.ptr(0, v) for k, v in off.items()}
        ctx.fr_lagrange_coefficients(log_d, _mont(tau), n_out=dsize, out=p["u"], mem=dev_mem)
        for name, M in (("a", A), ("b", B), ("c", C)):
            t_ptr, t_idx, t_val = csr_transpose(M[0], M[1], M[2], nv)
            if t_idx.size and m:
                mats.append(ctx.r1cs_matrix_register(t_ptr, t_idx, t_val, m))
                ctx.r1cs_matvec(mats[-1], p["u"], lanes=1, out=p[name], z_stride=dsize, out_stride=nv, mem=dev_mem)
        if ni:                                                         # the instance rows (r1cs_to_qap.rs:75-80)
            ctx.fr_vec_op(czk.CZK_OP_ADD, p["a"], lanes.ptr(0, off["u"] + m), out=p["a"], n=ni, mem=dev_mem)
        # beta a + alpha b + c, then / gamma for the instance variables and / delta for the witness variables (generator.rs:92-102)
        ctx.fr_lincomb([p["a"], p["b"], p["c"]], [nv] * 3, [1] * 3, [_mont(beta), _mont(alpha), _mont(1)], 1, 1, p["lin"], nv)
        if ni:
            ctx.fr_vec_scale(p["lin"], _mont(g_inv), out=p["sc"], n=ni, mem=host_scalar)
        if nv > ni:
            ctx.fr_vec_scale(lanes.ptr(0, off["lin"] + ni), _mont(d_inv), out=lanes.ptr(0, off["sc"] + ni), n=nv - ni, mem=host_scalar)
        if D > 1:                                                      # h_i = tau^i Z(tau) / delta, i < D - 1 (generator.rs:156-163)
            ctx.fr_powers(_mont(tau), D - 1, c=_mont(zt * d_inv), out=p["h"], mem=dev_mem)

        one = np.array([[1, 0, 0, 0]], dtype=np.uint64)
        if g1_base is None:
            g1_base = ctx.fixed_base_points(czk.CZK_G1, one)[0]
        if g2_base is None:
            g2_base = ctx.fixed_base_points(czk.CZK_G2, one)[0]
        dev = torch.device("cuda", ctx.device)
        key = {}

        def query(fb, aw, src, n):
            pts = torch.empty((n, aw), dtype=torch.int64, device=dev)
            inf = torch.empty(n, dtype=torch.uint8, device=dev)
            if n:
                ctx.fixed_base_msm(fb, src, out=pts.data_ptr(), n=n, scalar_form=czk.CZK_SCALAR_MONTGOMERY, mem=dev_mem, out_inf=inf.data_ptr())
            return pts, inf

        t1 = ctx.fixed_base(czk.CZK_G1, g1_base, n_hint=3 * nv + D)
        try:
            key["a_query"] = query(t1, 12, p["a"], nv)
            key["b_g1_query"] = query(t1, 12, p["b"], nv)
            key["h_query"] = query(t1, 12, p["h"], max(D - 1, 0))
            key["l_query"] = query(t1, 12, lanes.ptr(0, off["sc"] + ni), nv - ni)
            key["gamma_abc_g1"] = query(t1, 12, p["sc"], ni)
            single = ctx.fixed_base_msm(t1, np.stack([_mont(alpha), _mont(beta), _mont(delta)]), scalar_form=czk.CZK_SCALAR_MONTGOMERY)[0]
            key["alpha_g1"], key["beta_g1"], key["delta_g1"] = single[0], single[1], single[2]
        finally:
            ctx.sync()
            t1.release()
        t2 = ctx.fixed_base(czk.CZK_G2, g2_base, n_hint=nv)
        try:
            key["b_g2_query"] = query(t2, 24, p["b"], nv)
            single = ctx.fixed_base_msm(t2, np.stack([_mont(beta), _mont(gamma), _mont(delta)]), scalar_form=czk.CZK_SCALAR_MONTGOMERY)[0]
            key["beta_g2"], key["gamma_g2"], key["delta_g2"] = single[0], single[1], single[2]
        finally:
            ctx.sync()
            t2.release()
    finally:
        ctx.sync()
        for mat in mats:
            mat.release()
        lanes.free()
    if to_host:
        for name in ("a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "gamma_abc_g1"):
            pts, inf = key[name]
            key[name] = (pts.cpu().numpy().view(np.uint64), inf.cpu().numpy())
    abc, abc_inf = key["gamma_abc_g1"]
    if not to_host:
        abc, abc_inf = abc.cpu().numpy().view(np.uint64), abc_inf.cpu().numpy()
    key["vk"] = {"alpha_g1": key["alpha_g1"], "beta_g2": key["beta_g2"], "gamma_g2": key["gamma_g2"], "delta_g2": key["delta_g2"],
                 "gamma_abc_g1": abc, "gamma_abc_inf": abc_inf}
    return key
