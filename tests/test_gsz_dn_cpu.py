"""The model of the GSZ material's generation (tests/gsz_dn_model.py) against outside facts: the ChaCha20 block of RFC 8439 section 2.3.2 and the local
`openssl enc -chacha20`; the sampler's formula; the dealt and extracted sharings' degrees, constant terms and secrets; the extraction matrix's minors,
exhaustively; and the consistency check on honest and on cheating dealers.  No GPU."""
import itertools
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import gsz_dn_model as DN
import gsz_mul_model as M
from gsz_mul_model import R_MOD

PARTIES = [3, 4, 6, 8, 12]
RFC_KEY = bytes(range(32))
RFC_NONCE = bytes.fromhex("000000090000004a00000000")
RFC_BLOCK = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")


def _keys(parties, seed):
    rng = random.Random(seed)
    return [bytes(rng.randrange(256) for _ in range(32)) for _ in range(parties)]


def _nonce(kind, seq):
    return kind.to_bytes(4, "little") + seq.to_bytes(8, "little")


def test_the_rfc_8439_block():
    assert DN.chacha20_block(RFC_KEY, RFC_NONCE, 1) == RFC_BLOCK


def test_a_hundred_thousand_blocks_are_quick_and_agree_with_single_ones():
    import time
    t0 = time.time()
    blocks = DN.chacha20_blocks(RFC_KEY, RFC_NONCE, np.arange(100000, dtype=np.uint64))
    assert time.time() - t0 < 5.0          # "well under a second" on an idle core; the bound leaves room for a loaded one
    assert blocks[1].tobytes() == RFC_BLOCK
    assert blocks[99999].tobytes() == DN.chacha20_block(RFC_KEY, RFC_NONCE, 99999)


@pytest.mark.skipif(shutil.which("openssl") is None, reason="no openssl binary")
def test_the_block_function_against_openssl():
    """openssl's 16-byte -iv is LE32(counter) || nonce; the keystream of zeros is the blocks themselves"""
    rng = random.Random(7)
    probe = subprocess.run(["openssl", "enc", "-chacha20", "-K", RFC_KEY.hex(), "-iv", ((1).to_bytes(4, "little") + RFC_NONCE).hex()], input=bytes(64),
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("this openssl has no chacha20")
    assert probe.stdout == RFC_BLOCK
    for _ in range(8):
        key, nonce = bytes(rng.randrange(256) for _ in range(32)), bytes(rng.randrange(256) for _ in range(12))
        ctr = rng.choice([0, 1, rng.randrange(1 << 32), (1 << 32) - 3])
        out = subprocess.run(["openssl", "enc", "-chacha20", "-K", key.hex(), "-iv", (ctr.to_bytes(4, "little") + nonce).hex()], input=bytes(192), capture_output=True,
                             check=True).stdout
        assert out == DN.chacha20_blocks(key, nonce, [ctr, ctr + 1, ctr + 2]).tobytes()


def test_the_counter_does_not_wrap():
    with pytest.raises(ValueError):
        DN.sample(RFC_KEY, RFC_NONCE, (1 << 32) - 1, 2)
    with pytest.raises(ValueError):
        DN.chacha20_blocks(RFC_KEY, RFC_NONCE, [1 << 32])
    assert len(DN.sample(RFC_KEY, RFC_NONCE, (1 << 32) - 2, 2)) == 2      # first + n = 2^32 exactly is the last legal call


def test_the_sampler_follows_its_formula():
    v = DN.sample(RFC_KEY, RFC_NONCE, 1, 300)
    assert all(0 <= x < R_MOD for x in v)
    lo = int.from_bytes(RFC_BLOCK[:32], "little") % (1 << 252)
    hi = int.from_bytes(RFC_BLOCK[32:], "little") % (1 << 252)
    assert lo < R_MOD and hi < R_MOD and (1 << 252) < R_MOD < (1 << 253)   # both halves are canonical as they stand
    assert v[0] == (lo + (hi << 252)) % R_MOD
    assert v[5] == DN.element_of_block(DN.chacha20_block(RFC_KEY, RFC_NONCE, 6))
    assert len(set(v)) == 300


def _coeffs(D, lanes, pos):
    return D.coeffs([lane[pos] for lane in lanes])


@pytest.mark.parametrize("parties", PARTIES)
def test_outputs_are_sharings_of_the_extracted_secrets(parties):
    D, d = M.Domain(parties), M.threshold(parties)
    keys, deal = _keys(parties, parties), 3
    for kind in (DN.KIND_DOUBLES, DN.KIND_RANDS):
        nonce = _nonce(kind, 1)
        r, r2 = DN.generate(D, kind, d, keys, nonce, deal)
        _, secrets = DN.deal_shares(D, kind, d, keys, nonce, range(deal), deal)
        assert len(r) == parties and len(r[0]) == deal * (parties - d) == DN.counts(kind, parties, d, deal * (parties - d))[1]
        for k in range(parties - d):
            for b in range(deal):
                c = _coeffs(D, r, k * deal + b)
                assert not any(c[d + 1:]) and (d == 0 or c[d] != 0)
                assert c[0] == sum(pow(D.w, i * k, R_MOD) * secrets[i][b] for i in range(parties)) % R_MOD
                if kind == DN.KIND_DOUBLES:
                    c2 = _coeffs(D, r2, k * deal + b)
                    assert not any(c2[2 * d + 1:]) and c2[0] == c[0] and (d == 0 or c2[1:] != c[1:])
        # the indexable form is the full one, restricted
        items = [2, 0]
        ri, ri2 = DN.generate(D, kind, d, keys, nonce, deal, items=items)
        idx = DN.output_indices(D, d, deal, items)
        assert ri == [[lane[t] for t in idx] for lane in r] and (ri2 is None or ri2 == [[lane[t] for t in idx] for lane in r2])


def _det(m):
    """determinant mod r by elimination"""
    m, n, det = [row[:] for row in m], len(m), 1
    for c in range(n):
        p = next((i for i in range(c, n) if m[i][c]), None)
        if p is None:
            return 0
        if p != c:
            m[c], m[p], det = m[p], m[c], -det
        det = det * m[c][c] % R_MOD
        inv = pow(m[c][c], -1, R_MOD)
        for i in range(c + 1, n):
            f = m[i][c] * inv % R_MOD
            if f:
                m[i] = [(a - f * b) % R_MOD for a, b in zip(m[i], m[c])]
    return det % R_MOD


@pytest.mark.parametrize("parties", PARTIES)
def test_every_minor_of_the_extraction_matrix_is_invertible(parties):
    """what makes the outputs uniform when parties - d dealers are honest: their columns alone already form an invertible map"""
    D, d = M.Domain(parties), M.threshold(parties)
    mat = DN.extraction_matrix(D, d)
    for cols in itertools.combinations(range(parties), parties - d):
        assert _det([[row[c] for c in cols] for row in mat]) != 0, cols


@pytest.mark.parametrize("parties", PARTIES)
def test_the_check_accepts_honest_output(parties):
    D, d = M.Domain(parties), M.threshold(parties)
    for kind in (DN.KIND_DOUBLES, DN.KIND_RANDS):
        for deal in (1, 2, 5) if parties > 3 else (2, 5):          # 3 outputs at least
            r, r2 = DN.generate(D, kind, d, _keys(parties, 40 + deal), _nonce(kind, 2), deal)
            if len(r[0]) >= 3:
                assert DN.check(D, kind, d, r, r2) == (1, 0, True)


def _cheat(D, kind, d, keys, nonce, deal, change):
    dealt, _ = DN.deal_shares(D, kind, d, keys, nonce, range(deal), deal)
    change(dealt)
    out = DN.extract(D, d, dealt)
    return out[0], (out[1] if kind == DN.KIND_DOUBLES else None)


@pytest.mark.parametrize("parties", PARTIES)
def test_the_check_rejects_a_polynomial_of_degree_d_plus_one(parties):
    D, d = M.Domain(parties), M.threshold(parties)
    deal = 3

    def change(dealt):           # dealer 1 adds 5 x^(d + 1) to its degree-d polynomial of item 1
        for j in range(parties):
            dealt[1][0][j][1] = (dealt[1][0][j][1] + 5 * pow(D.w, j * (d + 1), R_MOD)) % R_MOD
    for kind in (DN.KIND_DOUBLES, DN.KIND_RANDS):
        r, r2 = _cheat(D, kind, d, _keys(parties, 9), _nonce(kind, 3), deal, change)
        ok, bad, equal = DN.check(D, kind, d, r, r2)
        assert ok == 0 and bad >= 1 and equal          # the constant term is untouched: the degree bound is what catches it


@pytest.mark.parametrize("parties", PARTIES)
def test_the_check_rejects_different_secrets_in_the_two_halves(parties):
    D, d = M.Domain(parties), M.threshold(parties)
    deal = 3

    def change(dealt):           # dealer 2 (0 at fewer parties) shares s + 1 in the degree-2d half of item 0: still a polynomial of degree 2 d
        i = 2 % parties
        for j in range(parties):
            dealt[i][1][j][0] = (dealt[i][1][j][0] + 1) % R_MOD
    r, r2 = _cheat(D, DN.KIND_DOUBLES, d, _keys(parties, 10), _nonce(0, 4), deal, change)
    ok, bad, equal = DN.check(D, DN.KIND_DOUBLES, d, r, r2)
    assert (ok, bad, equal) == (0, 0, False)           # no bound is exceeded: the equality of the two opened values is the reason
    if parties == 3:                                   # ... and at 3 parties the only possible one: 2 d = parties - 1 bounds nothing
        assert 2 * d == parties - 1
        rng = random.Random(1)
        assert all(D.open([rng.randrange(R_MOD) for _ in range(3)], 2 * d)[1] == 0 for _ in range(20))


def test_the_library_counts_what_the_products_consume():
    """czk_gsz_dn_counts needs no GPU: for every op's material at n = 1, 2, 33 (plus the two sacrificed outputs) the deal is the smallest that yields it"""
    import ctypes as C

    import czk_amd
    L = czk_amd.lib()

    def counts(kind, parties, d, want):
        deal, outs = C.c_size_t(7), C.c_size_t(7)
        return L.czk_gsz_dn_counts(C.c_int(kind), C.c_size_t(parties), C.c_uint(d), C.c_size_t(want), C.byref(deal), C.byref(outs)), (deal.value, outs.value)

    def material(op, n):
        dd, rr = C.c_size_t(0), C.c_size_t(0)
        assert L.czk_gsz_material_counts(C.c_int(op), C.c_size_t(n), C.byref(dd), C.byref(rr)) == 0
        return dd.value, rr.value
    for parties in PARTIES + [1, 2]:
        d = M.threshold(parties)
        for op in (M.OP_MUL, M.OP_INV, M.OP_PARTIAL_PRODUCTS, M.OP_PRODUCT_CHECK):
            for n in (1, 2, 33):
                assert material(op, n) == M.material_counts(op, n)
                for kind, need in zip((DN.KIND_DOUBLES, DN.KIND_RANDS), material(op, n)):
                    rc, (deal, outs) = counts(kind, parties, d, need + 2)
                    assert rc == 0 and (deal, outs) == DN.counts(kind, parties, d, need + 2)
                    assert outs >= need + 2 > outs - (parties - d) and outs == deal * (parties - d)
    assert counts(DN.KIND_DOUBLES, 4, 2, 8) == (3, (0, 0)) and counts(DN.KIND_RANDS, 4, 4, 8) == (3, (0, 0)) and counts(2, 4, 1, 8) == (3, (0, 0))   # CZK_ERR_ARG
    assert counts(DN.KIND_RANDS, 4, 3, 8) == (0, (8, 8)) and counts(DN.KIND_DOUBLES, 3, 1, 0) == (0, (0, 0))
    assert counts(DN.KIND_RANDS, 128, 1, 8) == (1, (0, 0)) and counts(DN.KIND_RANDS, 4, 1, 1 << 60) == (1, (0, 0))                                   # CZK_ERR_SIZE
    assert L.czk_gsz_dn_counts(C.c_int(0), C.c_size_t(4), C.c_uint(1), C.c_size_t(8), None, None) == 3
