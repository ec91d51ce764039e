"""czk_blake2s, czk_fs_keystream and HOST transcripts (czk_fs_* with CZK_MEM_HOST, no context) through the C ABI against tests/fs_model.py: hashlib.blake2s and a
pure-Python ChaCha20.  Every comparison is for exact equality.  No GPU."""
import ctypes as C
import hashlib
import random

import numpy as np
import pytest

import fs_model as M
from fs_model import Q_MOD, R_MOD

ERR_ARG = 3
RR = (1 << 256) % R_MOD
QR = (1 << 384) % Q_MOD
# from_seed(SEED): the model's 64 draws below meet rejections, and its interleaved draws cross block edges (asserted where used)
SEED = b"czk fiat-shamir test seed"


@pytest.fixture(scope="module")
def czk():
    import czk_amd
    return czk_amd


def limbs(v: int, n: int) -> list:
    return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(n)]


def fr_mont(vals) -> np.ndarray:
    return np.array([limbs(v % R_MOD * RR % R_MOD, 4) for v in vals], dtype=np.uint64).reshape(-1, 4)


def fq_mont(vals) -> list:
    return [w for v in vals for w in limbs(v % Q_MOD * QR % Q_MOD, 6)]


def message(n: int, salt: int = 0) -> bytes:
    return bytes((7 * i + 13 * salt + (i >> 3)) & 0xFF for i in range(n))


def host(czk):
    return czk.binding.Fs(None, device=False)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 127, 128, 129, 1000])
def test_blake2s_equals_hashlib(czk, n):
    assert czk.binding.blake2s(message(n)) == hashlib.blake2s(message(n)).digest()


def test_keystream_of_the_zero_seed_is_the_published_chacha20_keystream(czk):
    w = czk.binding.fs_keystream(bytes(32), 0, 40)
    assert int(w[0]) == 0xade0b876                                       # RFC 8439's zero-key keystream starts 76 b8 e0 ad
    assert w[:16].tobytes()[:8].hex() == "76b8e0ada0f13d90"
    assert w.tolist() == M.chacha20_block(bytes(32), 0) + M.chacha20_block(bytes(32), 1) + M.chacha20_block(bytes(32), 2)[:8]
    key = hashlib.blake2s(b"k").digest()
    assert czk.binding.fs_keystream(key, 30, 5).tolist() == (M.chacha20_block(key, 1) + M.chacha20_block(key, 2))[14:19]
    far = (1 << 36) + 6                                                  # block 2^32: the counter's high word
    assert czk.binding.fs_keystream(key, far, 2).tolist() == M.chacha20_block(key, 1 << 32)[6:8]


def test_model_first_draws_by_hand():
    """(the model alone, against values assembled by hand: it says nothing about the library, only that the yardstick of the other tests is right)"""
    m = M.FsModel().put(b"abc").seed()
    assert m.seed_bytes == hashlib.blake2s(b"abc").digest() and m.pos == 0
    w = M.chacha20_block(m.seed_bytes, 0)
    assert m.squeeze_u64() == w[0] | w[1] << 32 and m.squeeze_u128() == w[2] | w[3] << 32 | w[4] << 64 | w[5] << 96 and m.pos == 6
    before = m.seed_bytes
    m.put(b"xy").absorb()
    assert m.seed_bytes == hashlib.blake2s(b"xy" + before).digest() and m.pos == 0
    assert M.fr_bytes(1) == b"\x01" + bytes(31) and len(M.g1_bytes(3, 4, False)) == 97 and len(M.g2_bytes((1, 2), (3, 4), True)) == 193
    assert M.g1_bytes(3, 4, True) == bytes(48) + b"\x01" + bytes(47) + b"\x01"


@pytest.mark.parametrize("length", [0] + [64 * j - 32 + d for j in (1, 2) for d in (-1, 0, 1)])
def test_seed_and_absorb_at_block_edges(czk, length):
    """L + 32 = 64 j - 1, 64 j, 64 j + 1 (the absorbed message is m || seed), and the same L for from_seed; L = 0"""
    t, m = host(czk), M.FsModel()
    for close in ("seed", "absorb", "absorb", "seed"):
        for salt in (1, 2):
            t.put_bytes(message(length, salt))
            m.put(message(length, salt))
            getattr(t, close)()
            getattr(m, close)()
            assert t.state() == m.state()
    for L in (31, 32, 33, 64, 128):                                      # the message alone on a block edge
        t.put_bytes(message(L))
        t.absorb()
        assert t.state() == m.put(message(L)).absorb().state()


def test_pieces_give_the_state_of_one_put(czk):
    msg = message(1 + 31 + 32 + 33 + 64 + 5)
    one, many, m = host(czk), host(czk), M.FsModel()
    one.put_bytes(msg)
    at = 0
    for piece in (1, 31, 32, 33, 64, 5):
        many.put_bytes(msg[at:at + piece])
        at += piece
    many.put_bytes(b"")
    for t in (one, many):
        t.seed()
    assert one.state() == many.state() == m.put(msg).seed().state()


def test_put_fr_and_put_points_write_the_models_bytes(czk):
    rng = random.Random(5)
    frs = [0, 1, R_MOD - 1] + [rng.randrange(R_MOD) for _ in range(70)]              # more than one 64-element step
    g1 = [(rng.randrange(Q_MOD), rng.randrange(Q_MOD), i in (0, 66)) for i in range(67)]
    g1[1] = (0, Q_MOD - 1, False)
    g2 = [((rng.randrange(Q_MOD), rng.randrange(Q_MOD)), (rng.randrange(Q_MOD), rng.randrange(Q_MOD)), i in (2, 64)) for i in range(66)]
    a, b = host(czk), host(czk)
    for t in (a, b):
        t.put_bytes(b"points")
        t.seed()
    a.put_fr(fr_mont(frs))
    b.put_bytes(b"".join(M.fr_bytes(v) for v in frs))
    a.absorb(), b.absorb()
    assert a.state() == b.state()
    a.put_points(czk.CZK_G1, np.array([fq_mont([x, y]) for x, y, _ in g1], dtype=np.uint64), np.array([inf for _, _, inf in g1], dtype=np.uint8))
    b.put_bytes(b"".join(M.g1_bytes(*p) for p in g1))
    a.absorb(), b.absorb()
    assert a.state() == b.state()
    a.put_points(czk.CZK_G2, np.array([fq_mont([*x, *y]) for x, y, _ in g2], dtype=np.uint64), np.array([inf for _, _, inf in g2], dtype=np.uint8))
    b.put_bytes(b"".join(M.g2_bytes(*p) for p in g2))
    a.absorb(), b.absorb()
    assert a.state() == b.state()
    # no flags given = none infinite
    a.put_points(czk.CZK_G1, np.array([fq_mont([x, y]) for x, y, _ in g1[:3]], dtype=np.uint64))
    b.put_bytes(b"".join(M.g1_bytes(x, y, False) for x, y, _ in g1[:3]))
    a.absorb(), b.absorb()
    assert a.state() == b.state()


def test_sixty_four_draws_equal_the_model_with_rejections(czk):
    t, m = host(czk), M.FsModel()
    t.put_bytes(SEED)
    t.seed()
    m.put(SEED).seed()
    want = [m.squeeze_fr_mont() for _ in range(64)]
    # From position 0 every Fr attempt is 8 words on an 8-word grid, so no single attempt can straddle a 16-word block here: what crosses an edge is an
    # element whose rejected and accepted attempts together do (edge_elements).  Single attempts that straddle an edge are in the interleaved test below.
    assert m.rejections >= 1 and m.edge_elements >= 1, "pick another SEED: the draws must meet a rejection and span a block edge"
    got = t.squeeze_fr(40).tolist() + t.squeeze_fr(24).tolist()
    assert got == [limbs(v, 4) for v in want]
    assert t.state() == m.state() and m.pos == 8 * (64 + m.rejections)
    assert all(v < R_MOD for v in want)


def test_interleaved_u64_and_fr_draws_cross_block_edges(czk):
    t, m = host(czk), M.FsModel()
    t.put_bytes(SEED)
    t.seed()
    m.put(SEED).seed()
    for step in range(12):
        assert int(t.squeeze_u64(1)[0]) == m.squeeze_u64()               # shifts the next Fr draws off the 8-word grid
        assert t.squeeze_fr(3).tolist() == [limbs(m.squeeze_fr_mont(), 4) for _ in range(3)]
        assert t.squeeze_u64(2).tolist() == limbs(m.squeeze_u128(), 2)
        assert t.state() == m.state()
    assert m.edge_draws >= 1 and m.rejections >= 1
    t.put_bytes(b"next")
    t.absorb()
    assert t.state() == m.put(b"next").absorb().state() and m.pos == 0
    assert int(t.squeeze_u64(1)[0]) == m.squeeze_u64()


def test_transcript_class_speaks_canonical_integers(czk):
    t, m = czk.Transcript(), M.FsModel()
    t.put_bytes(b"MARLIN-2019").put_u64(3, 5, 7).put_bool(True).put_fr([0, 1, R_MOD - 1, 12345]).seed()
    m.put(b"MARLIN-2019" + b"".join(v.to_bytes(8, "little") for v in (3, 5, 7)) + b"\x01" + b"".join(M.fr_bytes(v) for v in (0, 1, R_MOD - 1, 12345))).seed()
    assert t.state() == m.state()
    assert t.squeeze_fr() == m.squeeze_fr() and t.squeeze_fr(3) == [m.squeeze_fr() for _ in range(3)]
    assert t.squeeze_u128() == m.squeeze_u128() and t.squeeze_u64() == m.squeeze_u64() and t.squeeze_u64(2) == [m.squeeze_u64(), m.squeeze_u64()]
    assert t.state() == m.state()


def test_argument_rules(czk):
    L = czk.lib()
    code = lambda call: pytest.raises(czk.CzkError, call).value.code   # noqa: E731
    t = host(czk)
    assert code(lambda: t.squeeze_fr(1)) == ERR_ARG and code(lambda: t.squeeze_u64(1)) == ERR_ARG        # before the first seed
    assert t.squeeze_fr(0).shape == (0, 4) and t.squeeze_u64(0).size == 0                                    # n = 0: CZK_OK
    t.seed()                                                                                                 # an empty message is allowed
    assert t.state() == (hashlib.blake2s(b"").digest(), 0)
    t.squeeze_u64(1)
    before = t.state()
    t.put_bytes(b""), t.put_fr(np.zeros((0, 4), dtype=np.uint64)), t.put_points(czk.CZK_G2, np.zeros((0, 24), dtype=np.uint64))
    assert t.squeeze_u64(0).size == 0 and t.state() == before                                                # nothing changed: still no pending message
    t.squeeze_fr(1)
    t.put_bytes(b"x")
    assert code(lambda: t.squeeze_fr(1)) == ERR_ARG and code(lambda: t.squeeze_u64(1)) == ERR_ARG        # a pending message
    t.absorb()
    assert t.squeeze_u64(1).size == 1
    # device pointers given to a host transcript (never read: refused first)
    assert code(lambda: t.put_bytes(4096, 32)) == ERR_ARG and code(lambda: t.put_fr(4096, 1)) == ERR_ARG
    assert code(lambda: t.put_points(czk.CZK_G1, 4096, None, 1)) == ERR_ARG
    assert code(lambda: t.squeeze_fr(1, out=4096)) == ERR_ARG and code(lambda: t.squeeze_u64(1, out=4096)) == ERR_ARG
    assert code(lambda: t.put_points(3, np.zeros((1, 24), dtype=np.uint64))) == ERR_ARG                    # no such group
    # a device transcript needs a context; mem is HOST or DEVICE
    h = C.c_void_p(0)
    assert L.czk_fs_create(None, C.c_int(czk.CZK_MEM_DEVICE), C.byref(h)) == ERR_ARG and not h.value
    assert L.czk_fs_create(None, C.c_int(7), C.byref(h)) == ERR_ARG and L.czk_fs_create(None, C.c_int(0), None) == ERR_ARG
    assert L.czk_fs_seed(None) == ERR_ARG and L.czk_fs_state(None, None, None) == ERR_ARG
    with pytest.raises(ValueError):
        czk.Transcript(None, device=True)
    L.czk_fs_release(None)
    for sym in ("czk_blake2s", "czk_fs_keystream", "czk_fs_create", "czk_fs_release", "czk_fs_put_bytes", "czk_fs_put_fr", "czk_fs_put_points", "czk_fs_seed",
                "czk_fs_absorb", "czk_fs_squeeze_fr", "czk_fs_squeeze_u64", "czk_fs_state", "czk_fr_fri_fold_at"):
        assert sym in czk.header_symbols() and hasattr(L, sym), sym
