"""The reference's vector commitment of shared values and its FRI computation in hashlib and big integers (TEST INFRASTRUCTURE ONLY): what
czk_fr_merkle_commit / _open / _verify, czk_fr_fri_fold and czk_amd.fri must produce.  Written from mpc-algebra/src/com.rs:36-123 (ComField::commit, open_at,
check_opening) and mpc-snarks/src/client.rs:739-842 (Computation::Fri), not from the kernels.

A lane is one party's vector of canonical integers mod r; `lanes` is the list of every party's lane.  Differences from the reference, as in the library:
any number of parties (the reference has two), the challenge is a callable `challenge(round, roots) -> int` (the reference draws it from a merlin
transcript), the query chain runs for any list of start indices, and n = 1 is a tree of one leaf hash with empty paths.
"""
import hashlib

R_MOD = 8444461749428370424248824938781546531375899335154063827935233455917409239041
TWO_ADICITY = 47
# Fr has SMALL_SUBGROUP_BASE = 3, so get_root_of_unity starts from LARGE_SUBGROUP_ROOT_OF_UNITY (curves/bls12_377/src/fields/fr.rs:23-28, Montgomery
# limbs; order 3 * 2^47) cubed, not from TWO_ADIC_ROOT_OF_UNITY (algebra/ff/src/fields/mod.rs:337-367): another generator of the same 2^47 roots
_LARGE_ROOT_MONT = (0x9bfe9d90c790c167, 0x7175a69e39013bff, 0x3fbbb698adabcf93, 0x0c59f8d8d6f0dc97)
LARGE_ROOT = sum(v << (64 * i) for i, v in enumerate(_LARGE_ROOT_MONT)) * pow(1 << 256, -1, R_MOD) % R_MOD
TWO_ADIC_ROOT = pow(LARGE_ROOT, 3, R_MOD)


def _h(*parts) -> bytes:
    return hashlib.sha256(b"".join(parts)).digest()


def elem_bytes(v: int) -> bytes:
    """`v.serialize()`: into_repr() as 32 little-endian bytes"""
    return (v % R_MOD).to_bytes(32, "little")


# ---- com.rs ------------------------------------------------------------------------------------------------------------------------------
def tree_levels(vals):
    """com.rs:37-60 for one party: every level, the leaf hashes first, the root's level (one digest) last"""
    return tree_levels_of_bytes(b"".join(elem_bytes(v) for v in vals))


def tree_levels_of_bytes(data: bytes):
    """the same from the vector's serialized elements, 32 bytes each"""
    hashes = [hashlib.sha256(data[i:i + 32]).digest() for i in range(0, len(data), 32)]
    assert hashes and len(hashes) & (len(hashes) - 1) == 0
    levels = [hashes]
    while len(hashes) > 1:
        hashes = [_h(hashes[2 * i], hashes[2 * i + 1]) for i in range(len(hashes) // 2)]
        levels.append(hashes)
    return levels


def tree_bytes(levels) -> bytes:
    """the library's tree: 2n - 1 digests, level by level"""
    return b"".join(b"".join(lv) for lv in levels)


def commit(lanes):
    """-> (trees, roots): trees[l] = tree_levels of lane l (the reference's Key is trees[l][:-1]), roots[l] its root"""
    trees = [tree_levels(v) for v in lanes]
    return trees, [t[-1][0] for t in trees]


def path(levels, i: int):
    """com.rs:71-75"""
    out = []
    for level in range(len(levels) - 1):
        out.append(levels[level][i ^ 1])
        i //= 2
    assert i // 2 == 0
    return out


def open_at(lanes, trees, i: int):
    """-> (value, shares, paths): shares[l] = lanes[l][i], paths[l] = lane l's siblings, value = the sum of the shares"""
    shares = [v[i] for v in lanes]
    return sum(shares) % R_MOD, shares, [path(t, i) for t in trees]


def check_opening(roots, shares, paths, i: int, value) -> bool:
    """com.rs:95-123; value None skips the sum (the library's values == NULL)"""
    if value is not None and sum(shares) % R_MOD != value % R_MOD:
        return False
    for root, share, pth in zip(roots, shares, paths):
        h = _h(elem_bytes(share))
        for j, sib in enumerate(pth):
            h = _h(h, sib) if (i >> j) & 1 == 0 else _h(sib, h)
        if h != root:
            return False
    return True


def _vec_u8(b: bytes) -> bytes:
    return len(b).to_bytes(8, "little") + b                   # Vec<u8>::serialize: u64 length, then the bytes


def commitment_bytes(roots) -> bytes:
    """Two parties: CanonicalSerialize of the reference's Commitment (Vec<u8>, Vec<u8>) = (party 1's root, party 0's root) (com.rs:62-66, :122).
    Any other count: the roots as Vec<u8> in lane order."""
    if len(roots) == 2:
        return _vec_u8(roots[1]) + _vec_u8(roots[0])
    return b"".join(_vec_u8(r) for r in roots)


# ---- client.rs Computation::Fri ----------------------------------------------------------------------------------------------------------
def root_of_unity(n: int) -> int:
    """F::get_root_of_unity(n), n a power of two"""
    log_n = n.bit_length() - 1
    assert n == 1 << log_n and log_n <= TWO_ADICITY
    return pow(TWO_ADIC_ROOT, 1 << (TWO_ADICITY - log_n), R_MOD)


def fft(coeffs, n: int):
    """Radix2EvaluationDomain::new(n).fft: [sum_i c_i w^(i j) for j < n], the coefficients zero-padded to n"""
    a = [c % R_MOD for c in coeffs] + [0] * (n - len(coeffs))
    assert len(a) == n

    def rec(v, w):
        if len(v) == 1:
            return v
        ev, od = rec(v[0::2], w * w % R_MOD), rec(v[1::2], w * w % R_MOD)
        out, t, half = [0] * len(v), 1, len(v) // 2
        for j in range(half):
            x = t * od[j] % R_MOD
            out[j], out[j + half] = (ev[j] + x) % R_MOD, (ev[j] - x) % R_MOD
            t = t * w % R_MOD
        return out
    return rec(a, root_of_unity(n))


def fold(f, alpha: int):
    """client.rs:767-770"""
    return [(f[2 * i] + f[2 * i + 1] * alpha) % R_MOD for i in range(len(f) // 2)]


def commit_phase(f_lanes, challenge, committed_lanes=None, fold_alpha=None):
    """client.rs:745-777.  f_lanes: per lane 2^k coefficients.  challenge(i, roots) -> alpha_i.  Two hooks for dishonest provers: `committed_lanes` = the
    coefficient lanes whose evaluations round 0 commits to in place of f_lanes' (a longer vector folded as if it fitted); fold_alpha(i, alpha) = what the
    prover folds with.  -> state: k, lanes, rounds[i] = {n, evals, trees, roots, alpha}, constant."""
    size = len(f_lanes[0])
    k = size.bit_length() - 1
    assert size == 1 << k and all(len(f) == size for f in f_lanes)
    fs, rounds = [[list(f) for f in f_lanes]], []
    for i in range(k):
        n = 1 << (k + 1 - i)
        src = committed_lanes if (i == 0 and committed_lanes is not None) else fs[-1]
        evals = [fft(f, n) for f in src]
        trees, roots = commit(evals)
        alpha = challenge(i, roots) % R_MOD
        used = alpha if fold_alpha is None else fold_alpha(i, alpha) % R_MOD
        fs.append([fold(f, used) for f in fs[-1]])
        rounds.append({"n": n, "evals": evals, "trees": trees, "roots": roots, "alpha": alpha})
    assert len(fs[-1][0]) == 1
    return {"k": k, "lanes": len(f_lanes), "rounds": rounds, "constant": sum(f[0] for f in fs[-1]) % R_MOD}


def chain_indices(k: int, x_indices):
    """client.rs:787-795, :838 for every start index.  -> per round the indices opened in that round's tree: x_i of every start, then (n/2 + x_i) mod n of
    every start, then -- from round 1 on -- the previous round's x2 = x_i mod (n/2) of every start (the "next" opening, :813-828)."""
    xs, out = [x % (1 << (k + 1)) for x in x_indices], []
    for i in range(k):
        n = 1 << (k + 1 - i)
        out.append(list(xs) + [(n // 2 + x) % n for x in xs] + (list(xs) if i else []))
        xs = [2 * x % n // 2 for x in xs]
    return out


def query_phase(state, x_indices):
    """-> proof: k, lanes, x_indices, roots[i], constant, rounds[i] = {idx, values, shares, paths} over chain_indices' openings of round i"""
    rounds = []
    for rd, idx in zip(state["rounds"], chain_indices(state["k"], x_indices)):
        opened = [open_at(rd["evals"], rd["trees"], j) for j in idx]
        rounds.append({"idx": idx, "values": [o[0] for o in opened], "shares": [o[1] for o in opened], "paths": [o[2] for o in opened]})
    return {"k": state["k"], "lanes": state["lanes"], "x_indices": list(x_indices), "roots": [rd["roots"] for rd in state["rounds"]],
            "constant": state["constant"], "rounds": rounds}


def verify(proof, challenge) -> bool:
    """client.rs:801-836: every opening against its round's roots, the fold relation next = (v + v-) / 2 + alpha (v - v-) / (2 x) along every chain, the
    last round against the constant.  The indices and the alphas are recomputed, not read from the proof."""
    k, q = proof["k"], len(proof["x_indices"])
    chains = chain_indices(k, proof["x_indices"])
    if len(proof["rounds"]) != k or len(proof["roots"]) != k:
        return False
    for rd, roots, idx in zip(proof["rounds"], proof["roots"], chains):
        if rd["idx"] != idx or not all(check_opening(roots, s, p, j, v) for j, v, s, p in zip(idx, rd["values"], rd["shares"], rd["paths"])):
            return False
    inv2 = pow(2, -1, R_MOD)
    for i in range(k):
        n = 1 << (k + 1 - i)
        omega, alpha, vals = root_of_unity(n), challenge(i, proof["roots"][i]) % R_MOD, proof["rounds"][i]["values"]
        for s in range(q):
            x = pow(omega, chains[i][s], R_MOD)
            v, vneg = vals[s], vals[q + s]
            nxt = proof["rounds"][i + 1]["values"][2 * q + s] if i + 1 < k else proof["constant"]
            if nxt % R_MOD != ((v + vneg) * inv2 + alpha * (v - vneg) % R_MOD * pow(2 * x, -1, R_MOD)) % R_MOD:
                return False
    return True
