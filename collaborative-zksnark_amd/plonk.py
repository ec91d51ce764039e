"""Plonk's circuit layout and verifier for any arithmetic circuit next to polyvm.plonk_prove: `PlonkCircuit` (mpc-plonk/src/relations/structured.rs),
`CircuitLayout::from_circuit` (relations/flat.rs:35-137) with `setup` (lib.rs:42-80) on the GPU, the assignment side of the prover's inputs, and
`Verifier::verify` (lib.rs:511-582) with the index commitments taken from the key and every KZG opening checked.

layout = wiring (host numpy on the gate arrays: the slot layout and the wiring permutation) + Context.plonk_layout (csrc/plonk_layout.hip: the evaluation
vectors of w and s) + the library's transforms (s on the radix-2 gate domain, w on the mixed-radix wire domain) and commitments.  prover_inputs =
Context.fr_gather of the assignment's share lanes through the slot layout + the inverse transform on the wire domain.  Nothing is computed element by
element in Python.

Differences from the reference: Fiat-Shamir challenges are polyvm.challenge's fixed stand-ins, as in plonk_prove; the degree bound on p (lib.rs:517) is
not enforced; the key has no byte format.  A public variable that occurs in no gate is a ValueError (the reference drops it from public_indices and
panics later in inputs_poly), and so is a second public variable under a name already taken (the reference's public_indices would keep one of them).
polyvm.plonk_prove commits the witness of the selector's opening, which has n_gates - 1 coefficients: a circuit of ONE gate can be laid out but not
proved, and prover_inputs says so with a ValueError.
"""
from __future__ import annotations

import numpy as np

from . import binding as czk
from . import kzg, polyvm
from .marlin import _as_mont
from .polyvm import IFFT, R_MOD, challenge, unmont, vanishing


class Circuit:
    """PlonkCircuit (relations/structured.rs) without values: variables are numbers, a gate is (in0, in1, out) with a fresh output variable.  `prods`
    and `sums` are (k, 3) uint32 arrays in the order the gates were made, `pub_vars` maps a public variable to its name."""

    def __init__(self):
        self.n_vars = 0
        self.pub_vars: dict[int, str] = {}
        self._prods: list[tuple[int, int, int]] = []
        self._sums: list[tuple[int, int, int]] = []

    @property
    def prods(self) -> np.ndarray:
        return np.array(self._prods, dtype=np.uint32).reshape(-1, 3)

    @property
    def sums(self) -> np.ndarray:
        return np.array(self._sums, dtype=np.uint32).reshape(-1, 3)

    def new_var(self) -> int:
        self.n_vars += 1
        return self.n_vars - 1

    def publicize_var(self, v: int, name: str) -> None:
        if not 0 <= v < self.n_vars:
            raise ValueError(f"no variable {v}")
        if v in self.pub_vars:
            raise ValueError(f"Variable {v} was already public as {self.pub_vars[v]!r}, but is now being bound to {name!r}")
        if name in self.pub_vars.values():
            raise ValueError(f"the public name {name!r} is taken")
        self.pub_vars[v] = name

    def new_pub_var(self, name: str) -> int:
        v = self.new_var()
        self.publicize_var(v, name)
        return v

    def _gate(self, gates, a: int, b: int) -> int:
        if not (0 <= a < self.n_vars and 0 <= b < self.n_vars):
            raise ValueError("a gate's inputs must be variables made before it")
        gates.append((a, b, self.n_vars))
        return self.new_var()

    def new_sum(self, a: int, b: int) -> int:
        return self._gate(self._sums, a, b)

    def new_prod(self, a: int, b: int) -> int:
        return self._gate(self._prods, a, b)

    def n_gates(self) -> int:
        return len(self._prods) + len(self._sums)

    def pad_to_power_of_2(self) -> None:
        """sums of the last variable with itself until the gate count is a power of two (structured.rs:67-75)"""
        if not self.n_vars:
            raise ValueError("Cannot pad an empty circuit!")
        for _ in range(self.n_gates(), polyvm.next_pow2(self.n_gates())):
            self.new_sum(self.n_vars - 1, self.n_vars - 1)

    @classmethod
    def squaring_circuit(cls, steps: int) -> "Circuit":
        """new_squaring_circuit (structured.rs:76-85): v -> v^2 `steps` times, padded, the last square public as "out" """
        c = cls()
        v = c.new_var()
        for _ in range(steps):
            v = c.new_prod(v, v)
        c.pad_to_power_of_2()
        c.publicize_var(v, "out")
        return c

    def evaluate(self, free_values) -> list[int]:
        """Every variable's value as a canonical integer, from the values of the free variables (those no gate produces) in the order they were made."""
        kind = {o: (0, a, b) for a, b, o in self._prods}
        kind.update({o: (1, a, b) for a, b, o in self._sums})
        free = [int(v) % R_MOD for v in free_values]
        if len(free) != self.n_vars - len(kind):
            raise ValueError(f"{self.n_vars - len(kind)} free variables, {len(free)} values")
        vals, it = [], iter(free)
        for v in range(self.n_vars):                                              # a gate's inputs are older than its output
            if v in kind:
                s, a, b = kind[v]
                vals.append((vals[a] + vals[b]) % R_MOD if s else vals[a] * vals[b] % R_MOD)
            else:
                vals.append(next(it))
        return vals


def wiring(circuit: Circuit) -> dict:
    """The index arrays of CircuitLayout::from_circuit (flat.rs:62-80, :126-135): "var_layout" = the variable at each of the 3 n_gates wire slots
    (products first, then sums; in0, in1, out per gate), "succ" = the wiring permutation as slot indices -- the slots of one variable in ascending order,
    each pointing to the next and the last to the first (a variable used once is a fixed point) -- and "public_indices" = name -> the first slot of
    the public variable.  ValueError for a gate count that is not a power of two and for a public variable that occurs in no gate."""
    G = circuit.n_gates()
    if G < 1 or G & (G - 1):
        raise ValueError(f"{G} gates: the gate domain needs a power of two (pad_to_power_of_2)")
    var_layout = np.concatenate([circuit.prods, circuit.sums]).reshape(-1)
    order = np.argsort(var_layout, kind="stable")                                # slots grouped by variable, ascending inside a group
    by_var = var_layout[order]
    last = np.concatenate([by_var[1:] != by_var[:-1], [True]])                   # the last slot of each group ...
    first = np.concatenate([[True], last[:-1]])
    nxt = np.roll(order, -1)
    nxt[last] = order[first]                                                     # ... points back to the group's first
    succ = np.empty(3 * G, dtype=np.uint32)
    succ[order] = nxt
    used, first_slot = by_var[first], order[first]
    public_indices = {}
    for v, name in circuit.pub_vars.items():
        at = int(np.searchsorted(used, v))
        if at >= used.size or int(used[at]) != v:
            raise ValueError(f"public variable {v} ({name!r}) occurs in no gate")
        public_indices[name] = int(first_slot[at])
    return {"var_layout": np.ascontiguousarray(var_layout, dtype=np.uint32), "succ": succ, "public_indices": public_indices}


def layout(B, circuit: Circuit, timings: dict | None = None) -> dict:
    """CircuitLayout::from_circuit + setup for `circuit` on the polyvm.GpuBackend B: "s" / "w" the selector and wiring polynomials (public, on the
    device) with "s_cmt" / "w_cmt" their commitments, "var_layout" the slot layout on the device (for prover_inputs), "public_indices" name -> slot and
    "public_points" the canonical w^slot of the public wires in the order of the sorted names.  timings: a dict that receives the seconds spent per phase
    ("wiring", "kernel", "transforms", "commitments"), each closed by a synchronisation that a call without it does not make
    (tools/plonk_layout_bench.py)."""
    import time
    t_last = [time.perf_counter()]

    def lap(name):
        if timings is not None:
            B.ctx.sync()
            now = time.perf_counter()
            timings[name], t_last[0] = now - t_last[0], now
    wi = wiring(circuit)
    lap("wiring")
    G = circuit.n_gates()
    W = 3 * G
    torch = B.torch
    succ = torch.from_numpy(wi["succ"].view(np.int32)).to(B.dev)
    var_layout = torch.from_numpy(wi["var_layout"].view(np.int32)).to(B.dev)
    w_evals, s_evals = B._new(1, W), B._new(1, G)
    B.ctx.plonk_layout(succ.data_ptr(), G, len(circuit._prods), w_evals=w_evals.data_ptr(), s_evals=s_evals.data_ptr(), mem=czk.CZK_MEM_DEVICE)
    lap("kernel")
    s = B.ntt(s_evals, G, IFFT) if G > 1 else s_evals                            # gate_selector_evals.interpolate() on the radix-2 gate domain (one point: itself)
    w = B.ntt(w_evals, W, IFFT)                                                  # wire_evals.interpolate() on the mixed-radix wire domain
    lap("transforms")
    cm = {"s_cmt": B.commit(s), "w_cmt": B.commit(w)}
    B.transcript_point()
    cm = polyvm.resolved(cm)
    del succ                                                                     # (referenced until the kernel has read it: the commitments' wait is past it)
    lap("commitments")
    names = sorted(wi["public_indices"])
    omega = B.root_of_unity(W)
    return {"n_gates": G, "n_vars": circuit.n_vars, "s": s, "w": w, "s_cmt": cm["s_cmt"], "w_cmt": cm["w_cmt"], "var_layout": var_layout,
            "public_indices": wi["public_indices"], "public_points": [pow(omega, wi["public_indices"][name], R_MOD) for name in names]}


def verifier_key(lay: dict) -> dict:
    """What the verifier keeps of a layout (VerifierKey, lib.rs:62-80, with the public slots of the layout): host arrays only"""
    return {"n_gates": lay["n_gates"], "public_indices": dict(lay["public_indices"]),
            "s_cmt": (np.array(lay["s_cmt"][0], dtype=np.uint64), np.array(lay["s_cmt"][1], dtype=np.uint8)),
            "w_cmt": (np.array(lay["w_cmt"][0], dtype=np.uint64), np.array(lay["w_cmt"][1], dtype=np.uint8))}


def prover_inputs(B, lay: dict, values, timings: dict | None = None) -> dict:
    """The dict polyvm.plonk_prove takes, for a layout made by `layout` and an assignment of all its variables: `values` is a (lanes, n_vars, 4) device
    array of share lanes (B.lanes of them, Montgomery limbs), or plain values -- integers or (n_vars, 4) Montgomery limbs -- which are put on every lane
    as polyvm.shared_copy does.  p_evals[slot] = values[var_layout[slot]] (flat.rs:91-100) is one Context.fr_gather over the lanes, p its inverse
    transform on the wire domain.  timings receives "gather" and "transform" as in `layout`.  ValueError for a circuit of one gate (see the module's
    head) and for an assignment of another length."""
    import time
    G, n_vars = lay["n_gates"], lay["n_vars"]
    W = 3 * G
    if G < 2:
        raise ValueError("polyvm.plonk_prove needs at least two gates: the selector's opening witness has n_gates - 1 coefficients")
    if hasattr(values, "data_ptr"):
        vals = values.contiguous()
        if tuple(vals.shape) != (B.lanes, n_vars, 4):
            raise ValueError(f"share lanes must be ({B.lanes}, {n_vars}, 4)")
    else:
        plain = _as_mont(values)
        if plain.shape[0] != n_vars:
            raise ValueError(f"{n_vars} variables, {plain.shape[0]} values")
        vals = polyvm.shared_copy(B, B.upload(plain))
    t0 = time.perf_counter()
    p_evals = B._new(B.lanes, W)
    B.ctx.fr_gather(vals.data_ptr(), lay["var_layout"].data_ptr(), lanes=B.lanes, src_len=n_vars, src_stride=n_vars, n=W, out=p_evals.data_ptr(),
                    out_stride=W, mem=czk.CZK_MEM_DEVICE)
    if timings is not None:
        B.ctx.sync()
        timings["gather"], t0 = time.perf_counter() - t0, time.perf_counter()
    p = B.ntt(p_evals, W, IFFT)
    if timings is not None:
        B.ctx.sync()
        timings["transform"] = time.perf_counter() - t0
    return {"n_gates": G, "p": p, "s": lay["s"], "w": lay["w"], "public_points": list(lay["public_points"])}


class _Reject(Exception):
    pass


# every opening of a plonk_prove result: label -> (the commitment it opens, its point as a function of the challenges and the generator w)
_OPENINGS = {
    "pub_q_open": ("pub_q", lambda c, w, W: c["public.x"]), "pub_p_open": ("p", lambda c, w, W: c["public.x"]),
    "gates_s_open": ("s", lambda c, w, W: c["gates.x"]), "gates_p_open": ("p", lambda c, w, W: c["gates.x"]),
    "gates_q_open": ("gates_q", lambda c, w, W: c["gates.x"]), "gates_p_w_open": ("p", lambda c, w, W: w * c["gates.x"] % R_MOD),
    "gates_p_w2_open": ("p", lambda c, w, W: w * w % R_MOD * c["gates.x"] % R_MOD),
    "t_wr_open": ("t", lambda c, w, W: w * c["product.r"] % R_MOD), "t_r_open": ("t", lambda c, w, W: c["product.r"]),
    "t_wk_open": ("t", lambda c, w, W: pow(w, W - 1, R_MOD)), "f_wr_open": ("l1", lambda c, w, W: w * c["product.r"] % R_MOD),
    "q_r_open": ("q", lambda c, w, W: c["product.r"]),
    "l2_q_x_open": ("l2_q", lambda c, w, W: c["wiring.x"]), "w_x_open": ("w", lambda c, w, W: c["wiring.x"]),
    "l1_x_open": ("l1", lambda c, w, W: c["wiring.x"]), "p_x_open": ("p", lambda c, w, W: c["wiring.x"]),
}


def _decide(B, vk, public, out, rng, fiat_shamir=False):
    G = int(vk["n_gates"])
    W = 3 * G
    w = B.root_of_unity(W)
    if fiat_shamir:   # the verifier's own transcript over the proof's commitments (Verifier, lib.rs:461-572): nothing is read from out["challenges"]
        c = polyvm.plonk_fs_challenges(out)
    else:
        c = {t: challenge("plonk." + t) for t in ("public.x", "gates.x", "product.r", "wiring.y", "wiring.z", "wiring.x")}
    # the verifier's copy of the proof: the index commitments come from the key, and which commitment an opening belongs to and at which point is
    # the verifier's to say, not the proof's
    seen = {k: v for k, v in out.items() if k.endswith("_cmt")}
    seen["s_cmt"], seen["w_cmt"] = vk["s_cmt"], vk["w_cmt"]
    val = {}
    for label, (of, point) in _OPENINGS.items():
        o = dict(out[label])
        if o["point"] != point(c, w, W):
            raise _Reject(label + " opens at another point")
        lanes = [unmont(v) for v in np.asarray(o["value"], dtype=np.uint64).reshape(-1, 4)]
        if any(v != lanes[0] for v in lanes):
            raise _Reject(label + " is not one value")
        o["of"] = of
        seen[label], val[label] = o, lanes[0]
    # verify_public (lib.rs:526-540): z = prod (X - x_i) over the public wires, v = the interpolation through (x_i, public value)
    names = sorted(vk["public_indices"])
    xs = [pow(w, int(vk["public_indices"][n]), R_MOD) for n in names]
    ys = [int(public[n]) % R_MOD for n in names]
    x = c["public.x"]
    z_x, v_x = 1, 0
    for xi in xs:
        z_x = z_x * (x - xi) % R_MOD
    for i, (xi, yi) in enumerate(zip(xs, ys)):
        num = den = 1
        for j, xj in enumerate(xs):
            if j != i:
                num, den = num * (x - xj) % R_MOD, den * (xi - xj) % R_MOD
        v_x = (v_x + yi * num % R_MOD * pow(den, -1, R_MOD)) % R_MOD
    if (val["pub_p_open"] - v_x - val["pub_q_open"] * z_x) % R_MOD:
        raise _Reject("public wires")
    # verify_gates (:542-560)
    s, q, p, pw, pww = (val[k] for k in ("gates_s_open", "gates_q_open", "gates_p_open", "gates_p_w_open", "gates_p_w2_open"))
    if (s * (p + pw) + (1 - s) * p * pw - pww - q * vanishing(G, c["gates.x"])) % R_MOD:
        raise _Reject("gates")
    # verify_unit_product (:451-474)
    if (val["t_wr_open"] - val["t_r_open"] * val["f_wr_open"] - vanishing(W, c["product.r"]) * val["q_r_open"]) % R_MOD:
        raise _Reject("partial products")
    if val["t_wk_open"] != 1:
        raise _Reject("total product")
    # verify_wiring (:561-582)
    y, z, x = c["wiring.y"], c["wiring.z"], c["wiring.x"]
    p_x, l1_x, w_x, l2 = val["p_x_open"], val["l1_x_open"], val["w_x_open"], val["l2_q_x_open"]
    if ((p_x + y * x + z) * l1_x - (p_x + y * w_x + z) - l2 * vanishing(W, x)) % R_MOD:
        raise _Reject("wiring")
    checked = kzg.check_openings(B, seen, rng=rng, details=True)
    if len(checked) != len(_OPENINGS) or not all(checked.values()):
        raise _Reject("KZG openings")


def verify(B, vk: dict, public: dict, out: dict, rng=None, fiat_shamir: bool = False) -> bool:
    """Verifier::verify (lib.rs:511-582) on a plonk_prove result `out` made on the GpuBackend B, under the verifier_key `vk` and the public values
    `public` (name -> integer).  The four identities -- public wires, gates, unit product, wiring -- are recomputed from the challenges and the opened
    values; the sixteen KZG openings are checked (kzg.check_openings) on a copy of the proof in which s_cmt and w_cmt are the key's, never the proof's,
    and every opening is tied to the commitment and the point the verifier expects.  The public identity evaluates z(x) = prod (x - x_i) and the
    interpolation v(x) through (x_i, public[name_i]) by Lagrange's formula in host big integers: O(k^2) multiplications and k inversions for k public
    wires.  fiat_shamir=True: the challenges are recomputed by a host transcript from the proof's commitments (polyvm.plonk_fs_challenges), as a
    proof made by plonk_prove(..., fiat_shamir=True) needs; False: the fixed stand-ins.  A proof of one kind is rejected as the other: its openings
    are at other points.  ValueError if `public` does not name exactly the key's public wires; a malformed or rejected proof is False, never an exception."""
    if set(public) != set(vk["public_indices"]):
        raise ValueError(f"public values for {sorted(public)}, the key's public wires are {sorted(vk['public_indices'])}")
    try:
        _decide(B, vk, public, out, rng, fiat_shamir)
    except (_Reject, KeyError, IndexError, TypeError, ValueError, AttributeError, czk.CzkError):
        return False
    return True
