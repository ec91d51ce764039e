"""The reference's vector commitment of shared values (mpc-algebra/src/com.rs ComField) and its collaborative FRI (mpc-snarks/src/client.rs:739-842,
Computation::Fri) on share lanes that all live on one GPU: czk_fr_merkle_commit / _open / _verify, czk_fr_fri_fold and czk_ntt_fr_to (include/czk.h).

Everything is linear in the shares, so a lane is whatever the caller holds: an additive share, the sh lane of SPDZ, a Shamir evaluation.  Device memory is the
library's own (czk_lanes): a vector is `Lanes` of (parties, n) elements, a tree `Lanes` of (parties, 2n - 1) 32-byte slots holding digests.

Differences from the reference: any number of parties (the reference's Commitment is a pair); the challenge is a callable `challenge(round, roots) -> int`
that defaults to polyvm's fixed stand-in, and neither the merlin transcript nor the StdRng the reference draws from are reproduced: `prove` /
`verify_proof` below draw the challenges and the query indices from the library's own transcript (transcript.py, the FiatShamirRng<Blake2s> of the
reference's Marlin and Plonk) instead --; the query chain runs for any list of start indices, which are arguments; a vector of one element is a tree of one leaf hash
with empty paths.
"""
from __future__ import annotations

import numpy as np

from .binding import CZK_FFT, CZK_MEM_DEVICE, CZK_MEM_HOST, Lanes
from .polyvm import R_MOD, challenge as _fixed_challenge, mont, unmont
from .transcript import Transcript

_MONT_R_INV = pow(1 << 256, -1, R_MOD)
TWO_ADICITY = 47
# get_root_of_unity for a field with a small subgroup (algebra/ff/src/fields/mod.rs:337-367): LARGE_SUBGROUP_ROOT_OF_UNITY (fr.rs:23-28, Montgomery limbs,
# order 3 * 2^47) cubed, then squared down -- the root czk_ntt_fr's domains use, NOT Fr::TWO_ADIC_ROOT_OF_UNITY
_LARGE_ROOT_MONT = (0x9bfe9d90c790c167, 0x7175a69e39013bff, 0x3fbbb698adabcf93, 0x0c59f8d8d6f0dc97)
TWO_ADIC_ROOT = pow(sum(v << (64 * i) for i, v in enumerate(_LARGE_ROOT_MONT)) * _MONT_R_INV % R_MOD, 3, R_MOD)


def default_challenge(i: int, roots) -> int:
    """polyvm.challenge("fri.alpha.<i>"): a fixed, documented stand-in; a caller with a transcript passes its own callable"""
    return _fixed_challenge(f"fri.alpha.{i}")


def root_of_unity(n: int) -> int:
    """F::get_root_of_unity(n) for n a power of two, canonical"""
    log_n = n.bit_length() - 1
    if n != 1 << log_n or log_n > TWO_ADICITY:
        raise ValueError("no radix-2 domain of that size")
    return pow(TWO_ADIC_ROOT, 1 << (TWO_ADICITY - log_n), R_MOD)


def _limbs_to_ints(a) -> list:
    a = np.asarray(a, np.uint64).reshape(-1, 4)
    return [sum(int(row[j]) << (64 * j) for j in range(4)) for row in a]


def _ints_to_limbs(vals) -> np.ndarray:
    return np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


class _DeviceBytes:
    """A few bytes on the device for the calls that take every array from one kind of memory: 32-byte slots of the library's allocator."""

    def __init__(self, ctx, nbytes: int):
        self.n, self.l = nbytes, ctx.lanes_alloc(1, max(1, (nbytes + 31) // 32))

    @property
    def ptr(self) -> int:
        return self.l.ptr()

    def put(self, arr: np.ndarray):
        raw = np.zeros(self.l.len * 32, dtype=np.uint8)
        raw[:self.n] = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.l.upload(raw.view(np.uint64).reshape(-1, 4))
        return self

    def get(self, dtype, shape) -> np.ndarray:
        return self.l.download().view(np.uint8).reshape(-1)[:self.n].view(dtype).reshape(shape).copy()

    def free(self):
        self.l.free()


def upload_lanes(ctx, a: np.ndarray) -> Lanes:
    """(lanes, n, 4) Montgomery limbs -> device lanes"""
    a = np.ascontiguousarray(a, np.uint64)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError("lanes must have the shape (lanes, n, 4)")
    out = ctx.lanes_alloc(a.shape[0], a.shape[1])
    for ln in range(a.shape[0]):
        out.upload(a[ln], lane=ln)
    return out


# ---- ComField's three functions on device lanes -------------------------------------------------------------------------------------------
def merkle_commit(ctx, vec: Lanes, n: int | None = None, roots: bool = True) -> dict:
    """ComField::commit (com.rs:36-67) for every lane of `vec` (its first n elements, default all): {"n", "tree": Lanes of (lanes, 2n - 1) digests,
    "roots": the lanes' 32-byte roots in lane order (None, and nothing waited for, with roots=False)}.  The reference's Key is the tree without its
    last digest, its Commitment the tuple of roots (commitment_bytes)."""
    n = vec.len if n is None else n
    if n <= 0 or n & (n - 1):
        raise ValueError("the vector's length must be a power of two")    # the reference asserts this
    tree = ctx.lanes_alloc(vec.lanes, 2 * n - 1)
    _, r = ctx.fr_merkle_commit(vec.ptr(), lanes=vec.lanes, n=n, stride=vec.len, tree=tree.ptr(), tree_stride=2 * n - 1, roots=roots, mem=CZK_MEM_DEVICE)
    return {"n": n, "tree": tree, "roots": None if r is None else [r[ln].tobytes() for ln in range(vec.lanes)]}


def open_at(ctx, vec: Lanes, com: dict, indices) -> dict:
    """ComField::open_at (com.rs:68-94) at every index: {"idx" (q,) uint64, "shares" (q, lanes, 4), "paths" (q, lanes, log2 n, 32) uint8, "values" (q, 4)
    = the lanes' shares summed} -- the reference's OpeningProof per index is (shares, paths), its first result the value."""
    idx = np.ascontiguousarray(indices, np.uint64).reshape(-1)
    n, lanes, q = com["n"], vec.lanes, idx.size
    log_n = n.bit_length() - 1
    if q and int(idx.max()) >= n:
        raise IndexError("opening index beyond the vector")
    shares, paths = np.zeros((q, lanes, 4), dtype=np.uint64), np.zeros((q, lanes, log_n, 32), dtype=np.uint8)
    if q and lanes:
        d_idx = _DeviceBytes(ctx, 8 * q).put(idx)
        d_sh, d_pa = _DeviceBytes(ctx, shares.nbytes), _DeviceBytes(ctx, paths.nbytes)
        ctx.fr_merkle_open(vec.ptr(), com["tree"].ptr(), d_idx.ptr, lanes=lanes, n=n, stride=vec.len, tree_stride=com["tree"].len, q=q,
                           out_shares=d_sh.ptr, out_paths=d_pa.ptr if log_n else None, mem=CZK_MEM_DEVICE)
        shares = d_sh.get(np.uint64, shares.shape)
        if log_n:
            paths = d_pa.get(np.uint8, paths.shape)
        for b in (d_idx, d_sh, d_pa):
            b.free()
    sums = [sum(_limbs_to_ints(shares[i])) % R_MOD for i in range(q)]                   # Montgomery form is linear
    return {"idx": idx, "shares": shares, "paths": paths, "values": _ints_to_limbs(sums)}


def check_opening(ctx, roots, n: int, opening: dict, values="opened"):
    """ComField::check_opening (com.rs:95-123) for every index of an opening: (ok (q,) uint8, bad).  values: (q, 4) Montgomery limbs the shares must sum
    to; "opened" = the opening's own; None = paths only."""
    values = opening["values"] if isinstance(values, str) else values
    return ctx.fr_merkle_verify(np.frombuffer(b"".join(roots), dtype=np.uint8).reshape(-1, 32), opening["idx"], opening["shares"], opening["paths"], n,
                                values=values, mem=CZK_MEM_HOST)


def _vec_u8(b: bytes) -> bytes:
    return len(b).to_bytes(8, "little") + bytes(b)        # Vec<u8>::serialize


def commitment_bytes(roots) -> bytes:
    """Two parties: CanonicalSerialize of the reference's Commitment, the pair (party 1's root, party 0's root) of Vec<u8> (com.rs:62-66, :122) -- what
    client.rs appends to its transcript.  Any other count: the roots as Vec<u8> in lane order."""
    roots = [bytes(r) for r in roots]
    if len(roots) == 2:
        return _vec_u8(roots[1]) + _vec_u8(roots[0])
    return b"".join(_vec_u8(r) for r in roots)


# ---- client.rs Computation::Fri --------------------------------------------------------------------------------------------------------------
def commit_phase(ctx, f_lanes, challenge=default_challenge, fold_alpha=None, transcript=None) -> dict:
    """client.rs:745-777.  f_lanes: `Lanes` (left as it is) or a (lanes, 2^k, 4) array of Montgomery coefficients.  Round i = 0 .. k - 1: the 2^(k - i)
    coefficients, zero-padded to rate 1/2 by the transform's load, are evaluated over the domain of 2^(k - i + 1) points, committed, alpha_i =
    challenge(i, roots_i), and folded.  Evaluations and trees stay on the device.  fold_alpha(i, alpha) -> what to fold with (tests: a dishonest
    prover).  -> state {"k", "lanes", "rounds": [{"n", "evals", "tree", "roots", "alpha"}], "constant", "coeffs"}; release(state) frees it.
    transcript: a device `Transcript` in place of the hook (`prove`): a round's roots are absorbed from tree memory, alpha_i is squeezed into device
    memory and czk_fr_fri_fold_at reads it there, so nothing waits between rounds; one wait at the end brings back the roots, the alphas and the lanes'
    last element.  Whatever was allocated is freed when a step fails."""
    f = f_lanes if isinstance(f_lanes, Lanes) else upload_lanes(ctx, f_lanes)
    k = f.len.bit_length() - 1
    lanes, coeffs, rounds = f.lanes, [f], []
    state = {"k": k, "lanes": lanes, "rounds": rounds, "constant": None, "coeffs": coeffs, "own_input": not isinstance(f_lanes, Lanes)}
    alphas = None
    try:
        if f.len != 1 << k:
            raise ValueError("the number of coefficients must be a power of two")
        if transcript is not None and k:
            alphas = ctx.lanes_alloc(1, k)
        for i in range(k):
            m = 1 << (k - i)
            rd = {"n": 2 * m, "evals": ctx.lanes_alloc(lanes, 2 * m), "tree": None, "roots": None, "alpha": None}
            rounds.append(rd)
            ctx.ntt_fr_to(f.ptr(), f.len, rd["evals"].ptr(), k - i + 1, CZK_FFT, lanes=lanes, in_len=m)
            com = merkle_commit(ctx, rd["evals"], roots=transcript is None)
            rd["tree"], rd["roots"] = com["tree"], com["roots"]
            nxt = ctx.lanes_alloc(lanes, m // 2)
            coeffs.append(nxt)
            if transcript is None:
                rd["alpha"] = challenge(i, com["roots"]) % R_MOD
                used = rd["alpha"] if fold_alpha is None else fold_alpha(i, rd["alpha"]) % R_MOD
                ctx.fri_fold(f.ptr(), mont(used), lanes=lanes, n=m, stride=f.len, out=nxt.ptr(), out_stride=nxt.len, mem=CZK_MEM_DEVICE)
            else:
                for ln in range(lanes):
                    transcript.put_bytes(rd["tree"].ptr(ln, 4 * m - 2), 32)      # the lane's root, where the tree kernel left it
                transcript.absorb().squeeze_fr_mont(1, out=alphas.ptr(0, i))
                ctx.fri_fold_at(f.ptr(), alphas.ptr(0, i), lanes=lanes, n=m, stride=f.len, out=nxt.ptr(), out_stride=nxt.len)
            f = nxt
        if transcript is None:
            last = [f.download(lane=ln, n=1)[0] for ln in range(lanes)]
        else:
            h_roots, h_alpha, last = np.zeros((k, lanes, 4), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64), np.zeros((lanes, 4), dtype=np.uint64)
            for i, rd in enumerate(rounds):
                for ln in range(lanes):
                    rd["tree"].download_deferred(h_roots[i, ln], lane=ln, elem=2 * rd["n"] - 2)
            if k:
                alphas.download_deferred(h_alpha)
            for ln in range(lanes):
                f.download_deferred(last[ln], lane=ln)
            ctx.sync()                                                           # the one wait
            for i, rd in enumerate(rounds):
                rd["roots"], rd["alpha"] = [h_roots[i, ln].tobytes() for ln in range(lanes)], unmont(h_alpha[i])
        state["constant"] = sum(unmont(v) for v in last) % R_MOD                 # `constant.publicize()`: the lanes' sum
    except BaseException:
        release(state)
        raise
    finally:
        if alphas is not None:
            alphas.free()
    return state


def release(state: dict):
    for rd in state["rounds"]:
        rd["evals"].free()
        if rd["tree"] is not None:
            rd["tree"].free()
    for c in state["coeffs"][0 if state["own_input"] else 1:]:
        c.free()


def chain_indices(k: int, x_indices) -> list:
    """client.rs:787-795, :838 for every start index: per round the indices opened in that round's tree -- x_i of every start, (n/2 + x_i) mod n of every
    start and, from round 1 on, the previous round's x2 = x_i mod (n/2) of every start (the "next" opening of :813-828)."""
    xs, out = [int(x) % (1 << (k + 1)) for x in x_indices], []
    for i in range(k):
        n = 1 << (k + 1 - i)
        out.append(list(xs) + [(n // 2 + x) % n for x in xs] + (list(xs) if i else []))
        xs = [x % (n // 2) for x in xs]
    return out


def query_phase(ctx, state: dict, x_indices) -> dict:
    """client.rs:783-840 for any number of start indices: one czk_fr_merkle_open per round over all of them.  -> proof {"k", "lanes", "x_indices",
    "roots": per round, "constant", "rounds": [open_at's result over chain_indices' openings of the round]}."""
    rounds = [open_at(ctx, rd["evals"], {"n": rd["n"], "tree": rd["tree"]}, idx)
              for rd, idx in zip(state["rounds"], chain_indices(state["k"], x_indices))]
    return {"k": state["k"], "lanes": state["lanes"], "x_indices": [int(x) for x in x_indices], "roots": [rd["roots"] for rd in state["rounds"]],
            "constant": state["constant"], "rounds": rounds}


def verify(ctx, proof: dict, challenge=default_challenge) -> bool:
    """client.rs:801-836: one czk_fr_merkle_verify per round over all its openings; then, in host big integers, the fold relation
    next = (v + v-) / 2 + alpha_i (v - v-) / (2 x), x = w_n^(x_i), along every chain, the last round against the constant.  Indices and alphas are
    recomputed, not read from the proof."""
    k, q = proof["k"], len(proof["x_indices"])
    chains = chain_indices(k, proof["x_indices"])
    if len(proof["rounds"]) != k or len(proof["roots"]) != k:
        return False
    vals = []
    for i, (rd, roots, idx) in enumerate(zip(proof["rounds"], proof["roots"], chains)):
        if [int(j) for j in rd["idx"]] != idx:
            return False
        if idx:
            _, bad = check_opening(ctx, roots, 1 << (k + 1 - i), rd)
            if bad:
                return False
        vals.append([v * _MONT_R_INV % R_MOD for v in _limbs_to_ints(rd["values"])])
    inv2 = pow(2, -1, R_MOD)
    for i in range(k):
        n = 1 << (k + 1 - i)
        omega, alpha = root_of_unity(n), challenge(i, proof["roots"][i]) % R_MOD
        for s in range(q):
            x = pow(omega, chains[i][s], R_MOD)
            v, vneg = vals[i][s], vals[i][q + s]
            nxt = vals[i + 1][2 * q + s] if i + 1 < k else proof["constant"]
            if nxt % R_MOD != ((v + vneg) * inv2 + alpha * (v - vneg) % R_MOD * pow(2 * x, -1, R_MOD)) % R_MOD:
                return False
    return True


# ---- non-interactive: challenges and query indices from a Fiat-Shamir transcript ---------------------------------------------------------------
# The transcript: from_seed(seed); per round absorb(the lanes' roots, 32 bytes each, in lane order) and alpha_i = Fr::rand; after the last round
# absorb(the constant, as Fr::write) and one u64 per query, taken mod 2^(k + 1), as the start indices.
def _transcript_tail(t: Transcript, constant: int, k: int, queries: int) -> list:
    t.put_fr([constant]).absorb()
    return [x % (1 << (k + 1)) for x in t.squeeze_u64(queries)] if queries else []


def prove(ctx, f_lanes, queries: int = 1, seed: bytes = b"fri", device: bool = True) -> dict:
    """The commit phase with its challenges drawn from a transcript, then query_phase at the indices the transcript gives: query_phase's proof.
    device=True: the transcript's state lives on the device and commit_phase runs as one enqueued sequence with one wait at its end.  device=False: the
    same transcript in host memory through commit_phase's challenge hook (one stop per round), for comparison: the proofs are identical."""
    t = Transcript(ctx, device=True) if device else Transcript()
    state = None
    try:
        t.put_bytes(seed).seed()
        if device:
            state = commit_phase(ctx, f_lanes, transcript=t)
        else:
            state = commit_phase(ctx, f_lanes, challenge=lambda i, roots: t.put_bytes(b"".join(roots)).absorb().squeeze_fr())
        starts = _transcript_tail(t, state["constant"], state["k"], queries)
        t.state()                                   # blocking: raises if a squeeze on the device gave up (the transcript's sticky error word)
        return query_phase(ctx, state, starts)
    finally:
        if state is not None:
            release(state)
        t.release()


def verify_proof(ctx, proof: dict, seed: bytes = b"fri") -> bool:
    """`verify` with the alphas and the start indices recomputed by a host transcript from the proof's roots and constant: a proof whose roots, constant
    or indices were changed draws other challenges and fails."""
    t = Transcript()
    t.put_bytes(seed).seed()
    try:
        k = proof["k"]
        if len(proof["roots"]) != k or any(len(r) != proof["lanes"] or any(len(bytes(x)) != 32 for x in r) for r in proof["roots"]):
            return False
        alphas = [t.put_bytes(b"".join(bytes(x) for x in roots)).absorb().squeeze_fr() for roots in proof["roots"]]
        want = _transcript_tail(t, int(proof["constant"]) % R_MOD, k, len(proof["x_indices"]))
    finally:
        t.release()
    if [int(x) for x in proof["x_indices"]] != want:
        return False
    return verify(ctx, proof, challenge=lambda i, roots: alphas[i])
