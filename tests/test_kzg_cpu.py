"""KZG10's host-side pieces that need no GPU: the byte layout of a serialized VerifierKey (poly-commit/src/kzg10/data_structures.rs:192-286) against
the point codec's CPU reference (tests/point_codec_ref.py), the parse errors that are raised before anything is launched, and setup's argument
errors."""
import pytest

import point_codec_ref as R
from pairing_ref import R_MOD

FIELDS = (("g", 1, False), ("gamma_g", 1, False), ("h", 2, False), ("beta_h", 2, False))


def _model_vk():
    F1, F2 = R.FIELD[1], R.FIELD[2]
    from pyref import ec_mul
    return {"g": ec_mul(F1, 5, R.GEN[1]), "gamma_g": ec_mul(F1, 77, R.GEN[1]), "h": R.GEN[2], "beta_h": ec_mul(F2, 0xBE7A, R.GEN[2])}


def test_vk_layout_and_sizes_match_the_codec_reference():
    from czk_amd import keyio
    assert keyio.KZG10_VK_FIELDS == FIELDS
    assert keyio.kzg10_vk_size(True) == 48 + 48 + 96 + 96 == 288
    assert keyio.kzg10_vk_size(False) == 576
    vk = _model_vk()
    for compressed in (True, False):
        data = R.encode_struct(FIELDS, vk, compressed)
        lay = keyio.kzg10_vk_layout(compressed)
        assert lay["size"] == len(data) == keyio.kzg10_vk_size(compressed)
        end = 0
        for name, group, _ in FIELDS:
            off, n, g = lay[name]
            assert (off, n, g) == (end, 1, group)
            size = R.point_size(group, compressed)
            assert keyio.point_size(group, compressed) == size
            status, pt = R.decode_point(group, data[off:off + size], compressed, checked=True)
            assert status == R.OK and pt == vk[name], name
            end = off + size
        assert end == lay["size"]


@pytest.mark.parametrize("compressed", [True, False])
def test_truncated_or_over_long_input_is_a_parse_error(compressed):
    """raised by the layout pass, before any point is decoded: no context is needed to get there"""
    from czk_amd import keyio
    data = R.encode_struct(FIELDS, _model_vk(), compressed)
    for bad in (data[:-1], data[:len(data) // 2], b"", data + b"\0", data + data):
        with pytest.raises(ValueError, match="kzg10::VerifierKey"):
            keyio.kzg10_vk_from_bytes(None, bad, compressed=compressed)
    with pytest.raises(ValueError):                        # the other form's length
        keyio.kzg10_vk_from_bytes(None, R.encode_struct(FIELDS, _model_vk(), not compressed), compressed=compressed)


def test_setup_argument_errors():
    from czk_amd import kzg
    assert issubclass(kzg.DegreeIsZero, ValueError)
    for d in (0, -1):
        with pytest.raises(kzg.DegreeIsZero):
            kzg.setup(None, d, beta=3, gamma=5)
    with pytest.raises(ValueError, match="invertible"):
        kzg.setup(None, 4, beta=R_MOD, gamma=5, produce_g2_powers=True)      # beta = 0 mod r
    with pytest.raises(ValueError, match="limbs"):
        kzg.setup(None, 4, beta=3, gamma=5, g=[0] * 11)
    with pytest.raises(ValueError, match="limbs"):
        kzg.setup(None, 4, beta=3, gamma=5, h=[0] * 12)


def test_trim_argument_errors_and_randomizers():
    import random
    from czk_amd import kzg
    pp = {"max_degree": 4}
    for d in (0, 5):
        with pytest.raises(ValueError):
            kzg.trim(pp, d)
    r = kzg.draw_randomizers([0, 0, 1, 3, 6], random.Random(1))
    assert r.shape == (6, 4)
    as_int = [sum(int(r[i][j]) << (64 * j) for j in range(4)) for i in range(6)]
    assert [as_int[i] for i in (0, 1, 3)] == [1, 1, 1]     # the first opening of every batch (mod.rs:333)
    assert all(1 < as_int[i] < (1 << 128) for i in (2, 4, 5))
