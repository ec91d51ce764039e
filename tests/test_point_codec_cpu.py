"""CPU-only checks around the point codec: the big-integer model (tests/point_codec_ref.py) against itself and against Euler's criterion, the
pure-Python layout arithmetic of czk_amd.keyio, and the new entry points' declarations and null-context behaviour."""
import ctypes as C

import numpy as np
import pytest

import point_codec_ref as M
from pyref import F1, F2, FQ_MONT_R, FQ_TWO_ADICITY, G1_GEN, INF, Q_MOD, ec_mul, splitmix64

Q = Q_MOD


def _rand_fq(seed, n):
    out, st = [], seed
    while len(out) < n:
        v = 0
        for i in range(6):
            st, z = splitmix64(st)
            v |= z << (64 * i)
        v &= (1 << 377) - 1
        if v < Q:
            out.append(v)
    return out


def test_fq_roots_square_back_and_agree_with_eulers_criterion():
    vals = _rand_fq(0x5A17, 200) + [0, 1, 4, Q - 1, Q - 5]
    n_res = n_non = 0
    for a in vals:
        r = M.fq_sqrt_reference(a)
        euler = a == 0 or pow(a, (Q - 1) // 2, Q) == 1
        assert (r is not None) == euler
        if r is None:
            n_non += 1
            assert M.f_sqrt(1, a) == (False, 0)
        else:
            n_res += 1
            assert r * r % Q == a
            ok, s = M.f_sqrt(1, a)
            assert ok and s * s % Q == a and s <= (Q - s) % Q
    assert n_res > 60 and n_non > 60


def test_fq2_roots_square_back_and_agree_with_eulers_criterion():
    vals = [(a, b) for a, b in zip(_rand_fq(0x5A18, 200), _rand_fq(0x5A19, 200))]
    vals += [(0, 0), (1, 0), (Q - 5, 0), (0, 1), (0, 7), (3, 0), (11, 0)]
    n_res = n_non = 0
    for a in vals:
        norm = (a[0] * a[0] + 5 * a[1] * a[1]) % Q
        euler = norm == 0 or pow(norm, (Q - 1) // 2, Q) == 1    # a is a square in Fq2 iff its norm is one in Fq
        ok, s = M.f_sqrt(2, a)
        assert ok == euler, a
        if ok:
            n_res += 1
            assert F2.mul(s, s) == a and not M.f_gt(2, s, M.f_neg(2, s))
        else:
            n_non += 1
            assert s == (0, 0)
    assert n_res > 60 and n_non > 60
    assert M.f_sqrt(2, (Q - 5, 0))[0] and M.fq_sqrt_reference(Q - 5) is None   # -5: a non-residue of Fq, the square of u in Fq2


def test_window_table_keys_are_distinct():
    """the kernel recognises a power of zeta = z^(2^38) (order 256) by the low 64 bits of its Montgomery form"""
    zeta = pow(M.FQ_TWO_ADIC_ROOT, 1 << (FQ_TWO_ADICITY - 8), Q)
    assert pow(zeta, 128, Q) == Q - 1
    keys = {(pow(zeta, j, Q) * FQ_MONT_R % Q) & ((1 << 64) - 1) for j in range(256)}
    assert len(keys) == 256


@pytest.mark.parametrize("group", (1, 2))
@pytest.mark.parametrize("compressed", (True, False))
def test_model_round_trip(group, compressed):
    F = M.FIELD[group]
    pts = [ec_mul(F, k, M.GEN[group]) for k in range(1, 33)] + [INF]
    data = M.encode_points(group, pts, compressed)
    assert len(data) == len(pts) * M.point_size(group, compressed) == len(pts) * (48 if compressed else 96) * group
    st, back, bad, first = M.decode_points(group, data, compressed, checked=(group == 1))   # (the G2 subgroup test is slow in Python)
    assert st == [M.OK] * len(pts) and back == pts and bad == 0 and first == len(pts)


def test_g1_generator_compressed_form():
    data = M.encode_point(1, G1_GEN)
    assert len(data) == 48 and int.from_bytes(data, "little") & ((1 << 377) - 1) == G1_GEN[0]
    positive = G1_GEN[1] > Q - G1_GEN[1]
    assert data[-1] >> 6 == (2 if positive else 0)
    assert M.encode_point(1, (G1_GEN[0], Q - G1_GEN[1]))[-1] >> 6 == (0 if positive else 2)
    assert M.encode_point(1, INF) == bytes(47) + b"\x40"
    assert M.encode_point(1, INF, False) == bytes(48) + b"\x01" + bytes(46) + b"\x40"


def test_model_statuses():
    x_bytes = lambda v, fl=0: (v | fl << 376).to_bytes(48, "little")   # noqa: E731
    for x in (4, 7, 9, 10, 11):
        assert M.decode_point(1, x_bytes(x))[0] == M.NO_POINT
    assert M.decode_point(1, x_bytes(0), checked=False) == (M.OK, (0, 1))
    assert M.decode_point(1, x_bytes(0, 0x80), checked=False) == (M.OK, (0, Q - 1))
    assert M.decode_point(1, x_bytes(0))[0] == M.NOT_IN_SUBGROUP
    assert M.decode_point(1, x_bytes(Q - 1), checked=False) == (M.OK, (Q - 1, 0))
    assert M.decode_point(1, x_bytes(Q - 1, 0x80))[0] == M.NOT_IN_SUBGROUP
    assert M.decode_point(1, x_bytes(5, 0xC0))[0] == M.BAD_FLAGS
    assert M.decode_point(1, x_bytes(Q))[0] == M.NOT_CANONICAL
    assert M.decode_point(1, ((1 << 377) - 1).to_bytes(48, "little"))[0] == M.NOT_CANONICAL
    assert M.decode_point(1, x_bytes(12345, 0x40)) == (M.OK, INF)
    assert M.decode_point(2, x_bytes(1, 0x80) + x_bytes(2))[0] == M.NOT_CANONICAL      # a flag bit on c0
    off = x_bytes(G1_GEN[0]) + x_bytes(G1_GEN[1] + 1)
    assert M.decode_point(1, off, False, False) == (M.OK, (G1_GEN[0], G1_GEN[1] + 1))
    assert M.decode_point(1, off, False, True)[0] == M.NOT_ON_CURVE
    assert M.decode_point(1, x_bytes(G1_GEN[0]) + x_bytes(G1_GEN[1], 0x80), False, True) == (M.OK, G1_GEN)   # bit 7 is ignored


def test_pk_layout_offsets_and_sizes():
    from czk_amd.keyio import groth16_pk_layout, point_size
    assert [point_size(g, c) for g in (1, 2) for c in (True, False)] == [48, 96, 96, 192]
    lay = groth16_pk_layout(0, 0, 0, 0, 0, 0)
    # alpha 48 | beta, gamma, delta 3 x 96 | len 8 | beta_g1, delta_g1 2 x 48 | five empty Vecs 5 x 8
    assert lay["vk_size"] == 48 + 288 + 8 == 344 and lay["size"] == 344 + 96 + 40 == 480
    assert lay["gamma_abc_g1"] == (344, 0, 1) and lay["beta_g1"] == (344, 1, 1) and lay["l_query"] == (480, 0, 1)
    lay = groth16_pk_layout(2, 7, 7, 7, 7, 5)
    assert lay["alpha_g1"] == (0, 1, 1) and lay["beta_g2"] == (48, 1, 2) and lay["gamma_g2"] == (144, 1, 2) and lay["delta_g2"] == (240, 1, 2)
    assert lay["gamma_abc_g1"] == (344, 2, 1) and lay["vk_size"] == 344 + 96 == 440
    assert lay["beta_g1"] == (440, 1, 1) and lay["delta_g1"] == (488, 1, 1)
    assert lay["a_query"] == (544, 7, 1)                      # 536 + 8
    assert lay["b_g1_query"] == (544 + 336 + 8, 7, 1) == (888, 7, 1)
    assert lay["b_g2_query"] == (888 + 336 + 8, 7, 2) == (1232, 7, 2)
    assert lay["h_query"] == (1232 + 672 + 8, 7, 1) == (1912, 7, 1)
    assert lay["l_query"] == (1912 + 336 + 8, 5, 1) == (2256, 5, 1)
    assert lay["size"] == 2256 + 240 == 2496
    unc = groth16_pk_layout(2, 7, 7, 7, 7, 5, compressed=False)
    assert unc["vk_size"] == 96 + 3 * 192 + 8 + 2 * 96 == 872 and unc["a_query"][0] == 872 + 192 + 8
    assert unc["size"] == 2 * (2496 - 6 * 8) + 6 * 8


class _NoGpu:
    """a context that fails the test if anything is launched"""
    device = 0

    def __getattr__(self, name):
        raise AssertionError(f"Context.{name} was reached: the buffer should have been rejected first")


def test_truncated_and_overlong_buffers_raise_before_any_launch():
    from czk_amd.keyio import groth16_pk_from_bytes, groth16_pk_layout, groth16_proof_from_bytes, groth16_vk_from_bytes
    lay = groth16_pk_layout(1, 2, 2, 2, 1, 1)
    blob = bytearray(lay["size"])
    for name, n in (("gamma_abc_g1", 1), ("a_query", 2), ("b_g1_query", 2), ("b_g2_query", 2), ("h_query", 1), ("l_query", 1)):
        blob[lay[name][0] - 8:lay[name][0]] = n.to_bytes(8, "little")
    ctx = _NoGpu()
    with pytest.raises(ValueError, match="l_query"):
        groth16_pk_from_bytes(ctx, bytes(blob[:-1]))
    with pytest.raises(ValueError, match="left after"):
        groth16_pk_from_bytes(ctx, bytes(blob) + b"\0")
    with pytest.raises(ValueError, match="beta_g2"):
        groth16_pk_from_bytes(ctx, bytes(blob[:100]))
    with pytest.raises(ValueError, match="length of a_query"):
        groth16_pk_from_bytes(ctx, bytes(blob[:lay["a_query"][0] - 4]))
    huge = bytearray(blob)
    huge[lay["b_g2_query"][0] - 1] = 0x40                     # the top byte of b_g2_query's length prefix
    with pytest.raises(ValueError, match="b_g2_query"):
        groth16_pk_from_bytes(ctx, bytes(huge))
    with pytest.raises(ValueError, match="gamma_abc_g1"):
        groth16_vk_from_bytes(ctx, bytes(blob[:lay["vk_size"] - 1]))
    with pytest.raises(ValueError):
        groth16_proof_from_bytes(ctx, bytes(191))
    with pytest.raises(ValueError):
        groth16_proof_from_bytes(ctx, bytes(193))


def test_header_declares_the_codec_and_null_contexts_are_rejected():
    import czk_amd
    assert {"czk_fq_sqrt", "czk_points_serialize", "czk_points_deserialize"} <= set(czk_amd.header_symbols())
    L = czk_amd.lib()
    buf = np.zeros(48, dtype=np.uint64)
    p = buf.ctypes.data_as(C.c_void_p)
    bad, first = C.c_size_t(7), C.c_size_t(7)
    assert L.czk_fq_sqrt(None, C.c_int(1), p, C.c_size_t(1), p, p, C.c_int(0)) == 3
    assert L.czk_points_serialize(None, C.c_int(1), p, None, C.c_size_t(1), C.c_int(1), p, C.c_int(0)) == 3
    assert L.czk_points_deserialize(None, C.c_int(1), p, C.c_size_t(1), C.c_int(3), p, p, None, C.byref(bad), C.byref(first), C.c_int(0)) == 3
    assert czk_amd.binding.CZK_POINTS_COMPRESSED == 1 and czk_amd.binding.CZK_POINTS_CHECKED == 2
