"""Marlin's index and verifier for any R1CS next to polyvm.marlin_prove: `AHPForR1CS::index` (marlin/src/ahp/indexer.rs:119-209) on the GPU for
constraint matrices in CSR form, the assignment side of the prover's inputs, and the AHP verifier's decision (marlin/src/ahp/mod.rs:115-260,
ahp/verifier.rs) with the KZG openings checked against the index commitments of the key.

index = square_and_balance (host numpy on the CSR index arrays: pad_input_for_indexer_and_prover, make_matrices_square, balance_matrices, the
per-row sort of arithmetize_matrix) + Context.marlin_arithmetize per matrix (csrc/marlin_index.hip: row / col / val / row_col on K) + the library's
lane transforms (12 inverse transforms on K, 12 forward on B) and commitments.  Nothing is computed element by element in Python.

Differences from the reference: Fiat-Shamir challenges are polyvm.challenge's fixed stand-ins, as in marlin_prove; an index with fewer than two
non-zero entries per matrix (num_non_zero < 2) is refused with ValueError -- the reference asks for a B domain of 3 |K| - 3 = 0 points there.
"""
from __future__ import annotations

import numpy as np

from . import binding as czk
from . import kzg, polyvm
from .keygen import R_MOD, csr_transpose
from .polyvm import FFT, IFFT, challenge, next_pow2, unmont, vanishing

_ONE = polyvm.mont(1)


def _csr(M):
    row_ptr = np.ascontiguousarray(M[0], dtype=np.uint64).reshape(-1)
    col = np.ascontiguousarray(M[1], dtype=np.uint32).reshape(-1)
    coeff = np.ascontiguousarray(M[2], dtype=np.uint64).reshape(-1, 4)
    m = row_ptr.size - 1
    if m < 0 or int(row_ptr[0]) != 0 or int(row_ptr[-1]) != col.size or coeff.shape[0] != col.size or np.any(row_ptr[1:] < row_ptr[:-1]):
        raise ValueError("malformed CSR matrix")
    return row_ptr, col, coeff


def reindex(H: int, X: int, index):
    """reindex_by_subdomain(H, X, index) (algebra/poly/src/domain/mod.rs:196-218) for an array of indices below H: where on H the variable sits when
    the first X variables take the positions of the sub-domain X."""
    i = np.asarray(index, dtype=np.int64)
    period = H // X
    if period == 1:
        return i.copy()
    j = np.maximum(i - X, 0)
    return np.where(i < X, i * period, j + j // (period - 1) + 1)


def square_and_balance(A, B, C, num_instance: int, num_witness: int):
    """The matrices as AHPForR1CS::index arithmetises them (indexer.rs:131-141), from the CSR triples (row_ptr, col_idx, coeff) of an R1CS with
    `num_instance` formatted inputs (the leading one included) and `num_witness` witness variables, columns numbered [instance | witness]:

      * the formatted inputs are padded to X = next_pow2(num_instance) (pad_input_for_indexer_and_prover): witness columns move up by X - num_instance;
      * make_matrices_square: empty rows are appended, or dummy witness variables without entries are added, until rows == variables;
      * num_non_zero = the largest of the three entry counts, taken BEFORE balancing (indexer.rs:138-140);
      * balance_matrices (constraint_systems.rs:25-41), exactly: rows of A and B are swapped one at a time while A holds at least as many entries as B
        (a tie counts as "A is denser").  Once B is denser nothing swaps any more, so the swapped rows are a prefix;
      * every row is stably sorted by column (:183-185); equal columns are never merged.

    Returns (A, B, C, info): CSR triples in the padded numbering, info = IndexInfo's four numbers."""
    ni, nw = int(num_instance), int(num_witness)
    if ni < 1 or nw < 0:
        raise ValueError("an R1CS has at least the formatted input 1")
    mats = [_csr(M) for M in (A, B, C)]
    m = mats[0][0].size - 1
    if any(M[0].size - 1 != m for M in mats):
        raise ValueError("A, B and C must have one row per constraint")
    if any(M[1].size and int(M[1].max()) >= ni + nw for M in mats):
        raise ValueError("column index outside the matrix")
    X = next_pow2(ni)
    nv = X + nw
    if nv > m:                                                                  # dummy constraints 0 * 0 = 0
        mats = [(np.concatenate([rp, np.full(nv - m, rp[-1], dtype=np.uint64)]), col, cf) for rp, col, cf in mats]
    else:                                                                       # dummy unconstrained witness variables
        nw += m - nv
    n = max(nv, m)
    mats = [(rp, np.where(col >= ni, col + np.uint32(X - ni), col).astype(np.uint32), cf) for rp, col, cf in mats]
    num_non_zero = max(M[1].size for M in mats)
    # balance_matrices: with D = |A| - |B|, row r is swapped iff D >= 0 when the loop reaches it, and a swap changes D by -2 (|A_r| - |B_r|)
    rpa, rpb = mats[0][0], mats[1][0]
    d = np.diff(rpa.astype(np.int64)) - np.diff(rpb.astype(np.int64))
    before = (int(rpa[-1]) - int(rpb[-1])) - 2 * np.concatenate([[0], np.cumsum(d)[:-1]]) if n else np.zeros(0, dtype=np.int64)
    stop = np.flatnonzero(before < 0)
    s = int(stop[0]) if stop.size else n                                       # rows [0, s) are swapped
    pa, pb = int(rpa[s]), int(rpb[s])

    def spliced(head, tail, ph, pt):
        rp = np.concatenate([head[0][:s + 1], tail[0][s + 1:] - np.uint64(pt) + np.uint64(ph)])
        return rp, np.concatenate([head[1][:ph], tail[1][pt:]]), np.concatenate([head[2][:ph], tail[2][pt:]])
    mats[0], mats[1] = spliced(mats[1], mats[0], pb, pa), spliced(mats[0], mats[1], pa, pb)
    out = []
    for rp, col, cf in mats:
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp.astype(np.int64)))
        order = np.lexsort((col, rows))                                          # stable: by row, then by column, ties in the given order
        out.append((rp, np.ascontiguousarray(col[order]), np.ascontiguousarray(cf[order])))
    info = {"num_variables": X + nw, "num_constraints": n, "num_non_zero": num_non_zero, "num_instance_variables": X}
    return out[0], out[1], out[2], info


def index(B, A, Bm, C, num_instance: int, num_witness: int, timings: dict | None = None) -> dict:
    """AHPForR1CS::index for the R1CS (A, Bm, C) on the polyvm.GpuBackend B: the index-side dict polyvm.marlin_prove takes.  "star"[m]["on_K"] = (row,
    col, val) and "on_B" = (row, col, row_col, val) of the arithmetised matrices, "index_polys" the twelve polynomials in Index::iter's order (row, col,
    val, row_col of A, B, C) with "index_cmts" their commitments, "matrices_T" the transposed, re-indexed matrices calculate_t walks, "info" IndexInfo's
    numbers and "matrices" the balanced matrices themselves (host CSR, for prover_inputs).  H = next_pow2(num_constraints), K = next_pow2(num_non_zero),
    b_size = next_pow2(3 K - 3).  ValueError for num_non_zero < 2.  timings: a dict that receives the seconds spent per phase ("balance", "arithmetize",
    "transforms", "commitments", "matrices_T"), each closed by a synchronisation that a call without it does not make (tools/marlin_index_bench.py)."""
    import time
    t_last = [time.perf_counter()]

    def lap(name):
        if timings is not None:
            B.ctx.sync()
            now = time.perf_counter()
            timings[name], t_last[0] = now - t_last[0], now
    *balanced, info = square_and_balance(A, Bm, C, num_instance, num_witness)
    lap("balance")
    mats = dict(zip("abc", balanced))
    if info["num_non_zero"] < 2:
        raise ValueError("num_non_zero < 2: the domain B of 3 |K| - 3 points is empty")
    n, X = info["num_constraints"], info["num_instance_variables"]
    H, K = next_pow2(n), next_pow2(info["num_non_zero"])
    b_size = next_pow2(3 * K - 3)
    log_h, log_x = H.bit_length() - 1, X.bit_length() - 1
    torch, ctx = B.torch, B.ctx
    evals = B._new(12, K)                                                       # row, col, val, row_col of A | B | C on K
    held = []                                                                  # the uploaded CSR arrays stay referenced until the kernels have read them
    for i, m in enumerate("abc"):
        rp, col, cf = mats[m]
        dev = [torch.from_numpy(a).to(B.dev) for a in (rp.view(np.int64), col.view(np.int32), cf.view(np.int64))]
        held.append(dev)
        ctx.marlin_arithmetize(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), log_h, log_x, X, K, out=evals[4 * i].data_ptr(),
                               mem=czk.CZK_MEM_DEVICE, m=n, nnz=col.size)
    lap("arithmetize")
    polys = B.ntt(evals, K, IFFT)                                               # twelve interpolations on K, one lane call
    on_b = B.ntt(polys, b_size, FFT)                                            # twelve evaluations on B
    lap("transforms")
    cm = B.commit(polys)
    B.transcript_point()
    aff, inf = polyvm.resolved(cm)
    lap("commitments")
    idx = {"H": H, "K": K, "X": X, "b_size": b_size, "star": {}, "matrices_T": {}, "real_lcs": True, "t_rows": None, "info": info, "matrices": mats,
           "index_polys": [polys[j:j + 1] for j in range(12)], "index_cmts": [(aff[j:j + 1].copy(), inf[j:j + 1].copy()) for j in range(12)]}
    for i, m in enumerate("abc"):
        idx["star"][m] = {"on_K": [evals[4 * i + j:4 * i + j + 1] for j in (0, 1, 2)], "on_B": [on_b[4 * i + j:4 * i + j + 1] for j in (0, 1, 3, 2)]}
        rp, col, cf = mats[m]
        t_ptr, t_idx, t_val = csr_transpose(rp, reindex(H, X, col).astype(np.uint32), cf, H)
        idx["matrices_T"][m] = B.matrix(t_ptr, t_idx, t_val, H)
    del held
    lap("matrices_T")
    return idx


def _as_mont(vals) -> np.ndarray:
    """(n, 4) Montgomery limbs of a sequence of integers, or of an (n, 4) uint64 array that holds them already"""
    if isinstance(vals, np.ndarray) and vals.dtype == np.uint64:
        return np.ascontiguousarray(vals).reshape(-1, 4)
    rr = (1 << 256) % R_MOD
    raw = b"".join((int(v) % R_MOD * rr % R_MOD).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def prover_inputs(B, idx: dict, instance, witness, mask=None, seed: int = 0x3A26) -> dict:
    """The assignment side of marlin_prove's inputs for an index made by `index`, merged with it: instance = the formatted input [1, ...], witness = the
    witness variables, both as integers or as (n, 4) Montgomery limbs; the witness may also be a (lanes, n, 4) device array of share lanes (B.lanes of
    them), as plonk.prover_inputs takes the assignment.  "x" / "x_ints": the input padded with zeros to X; "w": the full assignment on H
    at the re-indexed positions (dummy variables = 1, unused positions 0: prover.rs:334-351) on every lane; "z_a", "z_b": czk_r1cs_matvec of the BALANCED
    A and B over the share lanes; "mask_poly": 3 |H| coefficients -- `mask` as (1, 3 |H|, 4) backend array, or B.random(seed, 3 |H|) -- with coefficient 0
    lowered so that the remainder modulo v_H has constant term 0 (prover.rs:373-376)."""
    info, H, X = idx["info"], idx["H"], idx["X"]
    nv = info["num_variables"]
    shared = hasattr(witness, "data_ptr")
    x = _as_mont(instance)
    if shared:
        if witness.dim() != 3 or witness.shape[0] != B.lanes or witness.shape[2] != 4:
            raise ValueError(f"share lanes must be ({B.lanes}, n, 4)")
        n_w = int(witness.shape[1])
    else:
        w = _as_mont(witness)
        n_w = w.shape[0]
    if x.shape[0] > X or X + n_w > nv:
        raise ValueError("assignment longer than the index's variables")
    full = np.zeros((nv, 4), dtype=np.uint64)
    full[:x.shape[0]] = x
    if not shared:
        full[X:X + n_w] = w
    full[X + n_w:] = _ONE                                                      # make_matrices_square's dummy variables
    inp = dict(idx)
    inp["x"] = B.upload(full[:X])
    inp["x_ints"] = [unmont(v) for v in full[:X]]
    if shared:
        # the public entries (input, dummy variables) as from_public on the lifting lanes, the witness on its share lanes; placed on H by index
        z = B.lifted(B.upload(full))
        z[:, X:X + n_w] = witness
        at_h = B.torch.from_numpy(reindex(H, X, np.arange(nv)).astype(np.int64)).to(z.device)
        inp["w"] = B.zeros(B.lanes, H)
        inp["w"][:, at_h] = z
    else:
        on_h = np.zeros((H, 4), dtype=np.uint64)
        on_h[reindex(H, X, np.arange(nv))] = full
        inp["w"] = polyvm.shared_copy(B, B.upload(on_h))
        z = polyvm.shared_copy(B, B.upload(full))
    for key, m in (("z_a", "a"), ("z_b", "b")):
        rp, col, cf = idx["matrices"][m]
        mat = B.ctx.r1cs_matrix_register(rp, col, cf, nv)
        out = B.zeros(B.lanes, H)
        B.ctx.r1cs_matvec(mat, z.data_ptr(), lanes=B.lanes, out=out.data_ptr(), z_stride=nv, out_stride=H, mem=czk.CZK_MEM_DEVICE)
        B.ctx.sync()
        mat.release()
        inp[key] = out
    mask = B.random(seed, 3 * H) if mask is None else mask
    if B.lanes_of(mask) != 1 or B.length(mask) != 3 * H:
        raise ValueError("mask must be one lane of 3 |H| coefficients")
    at = lambda k: mask[:, k:k + 1]   # noqa: E731  (one lane: a slice is dense)
    c0 = B.sub(at(0), B.add(B.add(at(0), at(H)), at(2 * H)))
    inp["mask_poly"] = polyvm.shared_copy(B, B.concat([c0, mask[:, 1:]]))
    return inp


def verifier_key(idx: dict) -> dict:
    """What the verifier keeps of an index: the domain sizes and the twelve index commitments (IndexVerifierKey, marlin/src/data_structures.rs)"""
    return {"H": idx["H"], "K": idx["K"], "X": idx["X"], "info": dict(idx["info"]), "index_cmts": [(np.array(c[0], dtype=np.uint64), np.array(c[1], dtype=np.uint8)) for c in idx["index_cmts"]]}


_INDEX_LABELS = [m + "_" + part for m in "abc" for part in ("row", "col", "val", "row_col")]
# verifier_query_set (ahp/verifier.rs:143-146, :207-211): labels in BTreeSet order, and the polynomials each combination names (ahp/mod.rs:115-260)
_QUERY = {"beta": ("g_1", "outer_sumcheck", "t", "z_b"), "gamma": ("a_denom", "b_denom", "c_denom", "g_2", "inner_sumcheck")}
_LC_POLYS = {"z_b": ("z_b",), "g_1": ("g_1",), "t": ("t",), "g_2": ("g_2",), "outer_sumcheck": ("mask_poly", "z_a", "w", "h_1"),
             "inner_sumcheck": ("a_val", "b_val", "c_val", "h_2"), "a_denom": ("a_row", "a_col", "a_row_col"), "b_denom": ("b_row", "b_col", "b_row_col"),
             "c_denom": ("c_row", "c_col", "c_row_col")}


class _Reject(Exception):
    pass


def _decide(B, vk, x_ints, out, rng, fiat_shamir=False):
    H, K, X = vk["H"], vk["K"], vk["X"]
    x_pad = [int(v) % R_MOD for v in x_ints] + [0] * (X - len(x_ints))
    if len(x_pad) != X:
        raise _Reject("public input longer than the input domain")
    fs = None
    if fiat_shamir:   # the verifier's own transcript (Marlin::verify, lib.rs:351-408) over the key, the public input and the proof's commitments
        fs = polyvm.MarlinTranscript(polyvm.marlin_fs_info(vk), vk["index_cmts"], x_pad[1:], H)
    try:
        _decide_with(B, vk, x_pad, out, rng, fs)
    finally:
        if fs is not None:
            fs.release()


def _decide_with(B, vk, x_pad, out, rng, fs):
    H, K, X = vk["H"], vk["K"], vk["X"]
    if fs is None:
        alpha, eta_a, eta_b, eta_c, beta, gamma = (challenge("marlin." + t) for t in ("alpha", "eta_a", "eta_b", "eta_c", "beta", "gamma"))
    else:
        fs.absorb_round(out, polyvm.MARLIN_FS_ROUNDS[0])
        alpha, eta_a, eta_b, eta_c = fs.draw_outside_domain(), fs.draw(), fs.draw(), fs.draw()
        fs.absorb_round(out, polyvm.MARLIN_FS_ROUNDS[1])
        beta = fs.draw_outside_domain()
        fs.absorb_round(out, polyvm.MARLIN_FS_ROUNDS[2])
        gamma = fs.draw()
    point = {"beta": beta, "gamma": gamma}
    inv = lambda v: pow(v % R_MOD, -1, R_MOD)   # noqa: E731
    # the published evaluations by (polynomial, point): marlin_prove evaluates what the coefficients need first (mod.rs:155-157, :228-231), then every
    # queried combination in label order (lib.rs:283-292)
    it = {tag: iter(out["evals_" + tag]) for tag in point}
    ev = {}
    order = [("z_b", "beta"), ("t", "beta"), ("g_1", "beta"), ("a_denom", "gamma"), ("b_denom", "gamma"), ("c_denom", "gamma"), ("g_2", "gamma")]
    order += [(label, "beta" if label in _QUERY["beta"] else "gamma") for label in sorted(_LC_POLYS)]
    for label, tag in order:
        for name in _LC_POLYS[label]:
            lanes = [unmont(v) for v in np.asarray(next(it[tag]), dtype=np.uint64).reshape(-1, 4)]
            if any(v != lanes[0] for v in lanes) or ev.setdefault((name, tag), lanes[0]) != lanes[0]:
                raise _Reject(f"evaluation of {name} at {tag} is not one value")
    if next(it["beta"], None) is not None or next(it["gamma"], None) is not None:
        raise _Reject("more evaluations than the query set asks for")
    # the two sumcheck combinations, their coefficients from the challenges, the public input and the evaluations (mod.rs:155-250)
    wx, x_beta, acc = B.root_of_unity(X), 0, 1
    for xj in x_pad:                                                           # x(beta) = sum_j L_j(beta) x_j over the input domain (:158-163)
        x_beta = (x_beta + vanishing(X, beta) * acc % R_MOD * inv(X * (beta - acc)) % R_MOD * xj) % R_MOD
        acc = acc * wx % R_MOD
    vh_a, vh_b, vx_b = vanishing(H, alpha), vanishing(H, beta), vanishing(X, beta)
    r_ab = (vh_a - vh_b) * inv(alpha - beta) % R_MOD                           # eval_unnormalized_bivariate_lagrange_poly
    z_b_beta, t_beta, g_1_beta, g_2_gamma = ev[("z_b", "beta")], ev[("t", "beta")], ev[("g_1", "beta")], ev[("g_2", "gamma")]
    den = {m: (beta * alpha - alpha * ev[(m + "_row", "gamma")] - beta * ev[(m + "_col", "gamma")] + ev[(m + "_row_col", "gamma")]) % R_MOD for m in "abc"}
    lcs = {label: [(1, names[0])] for label, names in _LC_POLYS.items() if len(names) == 1}
    consts = {}
    lcs["outer_sumcheck"] = [(1, "mask_poly"), (r_ab * (eta_a + eta_c * z_b_beta) % R_MOD, "z_a"), (-t_beta * vx_b % R_MOD, "w"), (-vh_b % R_MOD, "h_1")]
    consts["outer_sumcheck"] = (r_ab * eta_b % R_MOD * z_b_beta - t_beta * x_beta - beta * g_1_beta) % R_MOD
    v2 = vh_a * vh_b % R_MOD
    lcs["inner_sumcheck"] = [(eta_a * den["b"] % R_MOD * den["c"] % R_MOD * v2 % R_MOD, "a_val"), (eta_b * den["a"] % R_MOD * den["c"] % R_MOD * v2 % R_MOD, "b_val"),
                             (eta_c * den["b"] % R_MOD * den["a"] % R_MOD * v2 % R_MOD, "c_val"), (-vanishing(K, gamma) % R_MOD, "h_2")]
    consts["inner_sumcheck"] = -(den["a"] * den["b"] % R_MOD * den["c"] % R_MOD) * (gamma * g_2_gamma + t_beta * inv(K)) % R_MOD
    for m in "abc":
        lcs[m + "_denom"] = [(R_MOD - alpha, m + "_row"), (R_MOD - beta, m + "_col"), (1, m + "_row_col")]
        consts[m + "_denom"] = beta * alpha % R_MOD
    lc_at = lambda label, tag: sum(cf * ev[(name, tag)] for cf, name in lcs[label]) % R_MOD   # noqa: E731  (without the LCTerm::One constant)
    if (lc_at("outer_sumcheck", "beta") + consts["outer_sumcheck"]) % R_MOD:
        raise _Reject("outer sumcheck")
    if (lc_at("inner_sumcheck", "gamma") + consts["inner_sumcheck"]) % R_MOD:
        raise _Reject("inner sumcheck")
    # the verifier's copy of the proof: the index commitments come from the key, and each folded opening is checked against sum_j coef_j C_j with the
    # coefficients recomputed here (batch_check folds with powers of the opening challenge; a degree-bounded polynomial takes two, marlin_pc/mod.rs:259-316)
    seen = {k: v for k, v in out.items() if k not in ("lcs", "lc_consts")}
    for label, cmt in zip(_INDEX_LABELS, vk["index_cmts"]):
        seen[label + "_cmt"] = cmt
    if fs is None:
        ch = challenge("marlin.opening_challenge")
    else:   # the evaluations the reference absorbs (lib.rs:283-299, the verifier's :392): recomputed here, constants included, never read from the proof
        fs.absorb_evaluations([(lc_at(label, tag) + consts.get(label, 0)) % R_MOD for label, tag in polyvm.MARLIN_FS_EVALS])
        ch = fs.opening_challenge()
    for tag in ("beta", "gamma"):
        want, c, terms = 0, 1, []
        for label in _QUERY[tag]:
            want = (want + c * lc_at(label, tag)) % R_MOD
            terms += [(c * cf % R_MOD, name) for cf, name in lcs[label]]
            c = c * ch % R_MOD * (ch if label in ("g_1", "g_2") else 1) % R_MOD
        o = dict(out["open_" + tag])
        sh = out["open_" + tag + "_shifted"]
        bounded = "g_1" if tag == "beta" else "g_2"
        if o["point"] != point[tag] or sh["point"] != point[tag] or sh.get("of") not in (bounded, bounded + "_shifted"):
            raise _Reject("an opening at another point or of another polynomial")
        if any(unmont(v) != want for v in np.asarray(o["value"], dtype=np.uint64).reshape(-1, 4)):
            raise _Reject("folded value at " + tag)
        if any(unmont(v) != ev[(bounded, tag)] for v in np.asarray(sh["value"], dtype=np.uint64).reshape(-1, 4)):
            raise _Reject("shifted opening of " + bounded)
        o["terms"] = terms
        seen["open_" + tag] = o
    if not kzg.check_openings(B, seen, rng=rng):
        raise _Reject("KZG openings")


def verify(B, idx_or_vk: dict, x_ints, out: dict, rng=None, fiat_shamir: bool = False) -> bool:
    """The AHP verifier's decision on a marlin_prove result `out` made on the GpuBackend B with public data lifted onto every lane, for the formatted
    public input x_ints = [1, ...] under the index (or verifier_key) `idx_or_vk`.  The coefficients of both sumcheck combinations are recomputed from the
    challenges, x_ints and the published evaluations -- out["lcs"] / out["lc_consts"] and the prover's "terms" are never read; both combinations must be
    zero, the folded opened values must match, and every KZG opening is checked (kzg.check_openings) with the twelve index commitments taken from the
    key, not from `out`.  fiat_shamir=True: the challenges are recomputed by a host transcript (polyvm.MarlinTranscript) from the key, x_ints, the
    proof's commitments and the evaluations the verifier derives, as a proof made by marlin_prove(..., fiat_shamir=True) needs; out["challenges"] is
    never read.  A malformed or rejected proof is False, never an exception."""
    try:
        _decide(B, idx_or_vk, x_ints, out, rng, fiat_shamir)
    except (_Reject, KeyError, IndexError, StopIteration, TypeError, ValueError, AttributeError, czk.CzkError):
        return False
    return True
