"""Model of the GSZ material's generation (include/czk.h, czk_fr_random / czk_gsz_dn_*): the ChaCha20 block function of RFC 8439 vectorised in numpy, the
field sampler on top of it, and Damgard-Nielsen dealing, extraction and the consistency check over Python integers, read off the definition (every dealer's
shares first, then the extraction share-wise -- not the order the kernel takes).  TEST INFRASTRUCTURE ONLY.

Vectors are lists of `parties` lanes of canonical ints, lane j = party j's shares, as in gsz_mul_model.  `generate` is indexable: `items` names the dealt
items b the caller wants, and the result holds outputs k deal + b for those b alone (k-major, in the order of `items`)."""
import numpy as np

from gsz_mul_model import R_MOD, Domain  # noqa: F401  (the domain is part of this model's face)

KIND_DOUBLES, KIND_RANDS = 0, 1
_MASK252 = (1 << 252) - 1
_CONSTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _qr(x, a, b, c, d):
    x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 16)
    x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 12)
    x[a] += x[b]; x[d] ^= x[a]; x[d] = _rotl(x[d], 8)
    x[c] += x[d]; x[b] ^= x[c]; x[b] = _rotl(x[b], 7)


def chacha20_blocks(key: bytes, nonce: bytes, counters) -> np.ndarray:
    """The 64-byte blocks at (key, nonce, counter) for every counter: (n, 64) uint8.  RFC 8439 section 2.3, 32-bit counter."""
    assert len(key) == 32 and len(nonce) == 12
    ctr = np.asarray(counters, dtype=np.uint64)
    if ctr.size and int(ctr.max()) >> 32:
        raise ValueError("the 32-bit block counter would wrap")
    n = ctr.size
    kw, nw = np.frombuffer(key, "<u4"), np.frombuffer(nonce, "<u4")
    init = [np.full(n, v, np.uint32) for v in _CONSTS] + [np.full(n, v, np.uint32) for v in kw] + [ctr.astype(np.uint32)] + [np.full(n, v, np.uint32) for v in nw]
    x = [v.copy() for v in init]
    for _ in range(10):
        _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
        _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
    out = np.stack([a + b for a, b in zip(x, init)], axis=1).astype("<u4")
    return out.view(np.uint8).reshape(n, 64)


def chacha20_block(key: bytes, nonce: bytes, counter: int) -> bytes:
    return chacha20_blocks(key, nonce, [counter])[0].tobytes()


def element_of_block(block: bytes) -> int:
    """(lo + 2^252 hi) mod r: lo / hi = the block's two halves as little-endian integers mod 2^252"""
    lo, hi = int.from_bytes(block[:32], "little") & _MASK252, int.from_bytes(block[32:], "little") & _MASK252
    return (lo + (hi << 252)) % R_MOD


def sample_at(key: bytes, nonce: bytes, counters):
    raw = chacha20_blocks(key, nonce, counters).tobytes()
    return [element_of_block(raw[64 * i:64 * i + 64]) for i in range(len(raw) // 64)]


def sample(key: bytes, nonce: bytes, first: int, n: int):
    """czk_fr_random's elements first .. first + n - 1 (canonical ints)"""
    if first + n > 1 << 32:
        raise ValueError("first + n > 2^32: the 32-bit block counter would wrap")
    return sample_at(key, nonce, np.arange(first, first + n, dtype=np.uint64))


def draws(kind: int, d: int) -> int:
    return 1 + 3 * d if kind == KIND_DOUBLES else 1 + d


def counts(kind: int, parties: int, d: int, want: int):
    """(deal, outputs): what czk_gsz_dn_counts reports"""
    if kind not in (KIND_DOUBLES, KIND_RANDS) or (2 * d >= parties if kind == KIND_DOUBLES else d >= parties):
        raise ValueError("kind / degree")
    per = parties - d
    deal = -(-want // per)
    return deal, deal * per


def deal_shares(D: Domain, kind: int, d: int, keys, nonce: bytes, items, deal: int):
    """dealt[i][half][j][pos]: dealer i's share for party j of its item items[pos]; secrets[i][pos].  One half for random shares."""
    if deal * draws(kind, d) > 1 << 32:
        raise ValueError("deal draws > 2^32")
    nd, P = draws(kind, d), D.parties
    wp = D.points                                # w^e, e < parties
    dealt, secrets = [], []
    for i in range(P):
        ctr = np.array([b * nd + m for b in items for m in range(nd)], dtype=np.uint64)
        v = sample_at(keys[i], nonce, ctr)
        halves = []
        for half in range(2 if kind == KIND_DOUBLES else 1):
            deg, base = (2 * d, d) if half else (d, 0)
            lanes = [[0] * len(items) for _ in range(P)]
            for pos in range(len(items)):
                it = v[pos * nd:(pos + 1) * nd]
                for j in range(P):
                    lanes[j][pos] = (it[0] + sum(it[base + k] * wp[j * k % P] for k in range(1, deg + 1))) % R_MOD
            halves.append(lanes)
        dealt.append(halves)
        secrets.append([v[pos * nd] for pos in range(len(items))])
    return dealt, secrets


def extraction_matrix(D: Domain, d: int):
    """rows k < parties - d, columns i: w^(ik)"""
    return [[pow(D.w, i * k, R_MOD) for i in range(D.parties)] for k in range(D.parties - d)]


def extract(D: Domain, d: int, dealt):
    """dealt as deal_shares returns it -> per half, `parties` lanes of (parties - d) len(items) outputs, k-major"""
    P, M = D.parties, extraction_matrix(D, d)
    out = []
    for half in range(len(dealt[0])):
        n = len(dealt[0][half][0])
        out.append([[sum(M[k][i] * dealt[i][half][j][pos] for i in range(P)) % R_MOD for k in range(P - d) for pos in range(n)] for j in range(P)])
    return out


def generate(D: Domain, kind: int, d: int, keys, nonce: bytes, deal: int, items=None):
    """(r, r2): czk_gsz_dn_generate's lanes (r2 None for random shares), restricted to the items in `items` (all when None)"""
    items = list(range(deal)) if items is None else list(items)
    dealt, _ = deal_shares(D, kind, d, keys, nonce, items, deal)
    out = extract(D, d, dealt)
    return out[0], (out[1] if kind == KIND_DOUBLES else None)


def output_indices(D: Domain, d: int, deal: int, items):
    """where generate(..., items) sits in the full output: k deal + b, in generate's order"""
    return [k * deal + b for k in range(D.parties - d) for b in items]


def check(D: Domain, kind: int, d: int, r, r2):
    """czk_gsz_dn_check on full lanes -> (ok, bad, equal): bad = opens over their bound, equal = the two opened combinations agree (True for random shares)"""
    n = len(r[0])
    if n < 3:
        raise ValueError("fewer than 3 outputs")
    rho, bad = D.open([lane[n - 2] for lane in r], d)
    pw, acc = [], 1
    for _ in range(n - 2):
        acc = acc * rho % R_MOD
        pw.append(acc)

    def comb(v):
        return [(lane[n - 1] + sum(p * x for p, x in zip(pw, lane))) % R_MOD for lane in v]

    v1, b1 = D.open(comb(r), d)
    bad += b1
    equal = True
    if kind == KIND_DOUBLES:
        v2, b2 = D.open(comb(r2), 2 * d)
        bad += b2
        equal = v1 == v2
    return int(equal and not bad), bad, equal
