"""Device transcripts (czk_fs_* with CZK_MEM_DEVICE: every operation a kernel on the context's stream) against host transcripts given the same script, and
czk_fr_fri_fold_at against czk_fr_fri_fold.  The host form is held to hashlib and a Python ChaCha20 in tests/test_fs_cpu.py; here the two forms of the
library must agree in every state and every squeezed limb.  Every comparison is for exact equality."""
import random

import numpy as np
import pytest

import fs_model as M
from fs_model import Q_MOD, R_MOD
from util import rand_fr_canonical

pytestmark = pytest.mark.gpu
RR = (1 << 256) % R_MOD
QR = (1 << 384) % Q_MOD


@pytest.fixture(scope="module")
def gpu():
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    yield czk_amd, ctx
    ctx.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 8: np.int64}[a.dtype.itemsize])).cuda()


def from_dev(t, dtype):
    return t.cpu().numpy().view(dtype)


def limbs(v, n):
    return [(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(n)]


def script_data():
    rng = random.Random(11)
    raw = np.array([rng.randrange(256) for _ in range(13000)], dtype=np.uint8)                # longer than one staging step of the kernel (12352 bytes)
    frs = [0, 1, R_MOD - 1] + [rng.randrange(R_MOD) for _ in range(127)]
    fr = np.array([limbs(v * RR % R_MOD, 4) for v in frs], dtype=np.uint64)
    g1 = np.array([[w for c in range(2) for w in limbs(rng.randrange(Q_MOD) * QR % Q_MOD, 6)] for _ in range(70)], dtype=np.uint64)
    g2 = np.array([[w for c in range(4) for w in limbs(rng.randrange(Q_MOD) * QR % Q_MOD, 6)] for _ in range(67)], dtype=np.uint64)
    inf1, inf2 = np.zeros(70, dtype=np.uint8), np.zeros(67, dtype=np.uint8)
    inf1[[0, 64, 69]] = 1
    inf2[[1, 66]] = 1
    return raw, frs, fr, g1, inf1, g2, inf2


def test_device_and_host_transcripts_agree_step_by_step(gpu):
    czk, ctx = gpu
    raw, frs, fr, g1, inf1, g2, inf2 = script_data()
    d_raw, d_fr, d_g1, d_inf1, d_g2, d_inf2 = (to_dev(a) for a in (raw, fr, g1, inf1, g2, inf2))
    dev, host, model = czk.binding.Fs(ctx, device=True), czk.binding.Fs(None, device=False), M.FsModel()
    try:
        def both(step):
            step(dev, True), step(host, False)
            assert dev.state() == host.state()

        both(lambda t, d: t.put_bytes(b"seed material"))
        both(lambda t, d: t.seed())
        model.put(b"seed material").seed()
        assert dev.state() == model.state()
        # device memory at byte offsets 0, 1 and 3 of a buffer, short and long; host memory given to the device transcript
        for off, n in ((0, 32), (1, 63), (3, 64), (1, 129), (3, 12997), (0, 1)):
            both(lambda t, d: t.put_bytes(d_raw.data_ptr() + off, n) if d else t.put_bytes(raw[off:off + n]))
            model.put(raw[off:off + n].tobytes())
            both(lambda t, d: t.absorb())
            assert dev.state() == model.absorb().state()
        both(lambda t, d: t.put_bytes(raw[5:700]))
        both(lambda t, d: t.put_fr(d_fr.data_ptr(), len(frs)) if d else t.put_fr(fr))
        both(lambda t, d: t.put_fr(fr[:3]))
        both(lambda t, d: t.absorb())
        assert dev.state() == model.put(raw[5:700].tobytes() + b"".join(M.fr_bytes(v) for v in frs + frs[:3])).absorb().state()
        got = [dev.squeeze_fr(5), dev.squeeze_u64(3), dev.squeeze_fr(20)]
        want = [host.squeeze_fr(5), host.squeeze_u64(3), host.squeeze_fr(20)]
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and dev.state() == host.state()
        assert got[0].tolist() == [limbs(model.squeeze_fr_mont(), 4) for _ in range(5)]
        both(lambda t, d: t.put_points(czk.CZK_G1, d_g1.data_ptr(), d_inf1.data_ptr(), 70) if d else t.put_points(czk.CZK_G1, g1, inf1))
        both(lambda t, d: t.put_points(czk.CZK_G2, d_g2.data_ptr(), d_inf2.data_ptr(), 67) if d else t.put_points(czk.CZK_G2, g2, inf2))
        both(lambda t, d: t.put_points(czk.CZK_G1, d_g1.data_ptr(), None, 2) if d else t.put_points(czk.CZK_G1, g1[:2]))
        both(lambda t, d: t.put_points(czk.CZK_G2, g2[:3], inf2[:3]))
        both(lambda t, d: t.absorb())
        both(lambda t, d: t.absorb())                                                  # an empty message
        both(lambda t, d: t.seed())                                                    # and a second from_seed
        assert np.array_equal(dev.squeeze_u64(9), host.squeeze_u64(9)) and np.array_equal(dev.squeeze_fr(64), host.squeeze_fr(64))
        assert dev.state() == host.state()
    finally:
        dev.release(), host.release()


def test_squeezes_into_device_memory_equal_squeezes_to_the_host(gpu):
    czk, ctx = gpu
    import torch
    a, b = czk.binding.Fs(ctx, device=True), czk.binding.Fs(ctx, device=True)
    try:
        for t in (a, b):
            t.put_bytes(b"two transcripts, one script")
            t.seed()
        d_fr, d_u = torch.zeros(33 * 4 + 4, dtype=torch.int64, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
        assert a.squeeze_fr(33, out=d_fr.data_ptr()) is None and a.squeeze_u64(7, out=d_u.data_ptr()) is None
        a.squeeze_fr(1, out=d_fr.data_ptr() + 33 * 32)
        ctx.sync()
        want_fr, want_u, want_last = b.squeeze_fr(33), b.squeeze_u64(7), b.squeeze_fr(1)
        got = from_dev(d_fr, np.uint64).reshape(-1, 4)
        assert np.array_equal(got[:33], want_fr) and np.array_equal(got[33:], want_last)
        assert from_dev(d_u, np.uint64).tolist() == want_u.tolist() + [0]              # nothing past the 7 draws
        assert a.state() == b.state()
    finally:
        a.release(), b.release()


def test_device_transcript_argument_rules(gpu):
    czk, ctx = gpu
    t = czk.binding.Fs(ctx, device=True)
    try:
        code = lambda call: pytest.raises(czk.CzkError, call).value.code   # noqa: E731
        assert code(lambda: t.squeeze_u64(1)) == 3                         # before the first seed: refused without a read-back
        t.put_bytes(b"x")
        t.seed()
        t.put_bytes(b"y")
        assert code(lambda: t.squeeze_fr(1)) == 3                          # a pending message
        t.absorb()
        assert t.squeeze_fr(0).shape == (0, 4) and t.squeeze_u64(1).size == 1
        assert t.state() == M.FsModel().put(b"x").seed().put(b"y").absorb().state()[:1] + (2,)
    finally:
        t.release()


@pytest.mark.parametrize("lanes", [1, 3])
@pytest.mark.parametrize("n", [2, 3, 64])
def test_fold_at_equals_fold(gpu, orc, n, lanes):
    czk, ctx = gpu
    import torch
    stride, out_stride = n + 1, n // 2 + 2
    f = orc.fr_from_repr(rand_fr_canonical(900 + n + lanes, lanes * stride)).reshape(lanes, stride, 4)
    alpha = orc.fr_from_repr(rand_fr_canonical(77 + n, 1)).reshape(4)
    d_f, d_alpha = to_dev(f), to_dev(alpha)
    d_a = torch.full((lanes * out_stride * 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    d_b = d_a.clone()
    ctx.fri_fold(d_f.data_ptr(), alpha, lanes=lanes, n=n, stride=stride, out=d_a.data_ptr(), out_stride=out_stride, mem=czk.CZK_MEM_DEVICE)
    ctx.fri_fold_at(d_f.data_ptr(), d_alpha.data_ptr(), lanes=lanes, n=n, stride=stride, out=d_b.data_ptr(), out_stride=out_stride)
    ctx.sync()
    a, b = from_dev(d_a, np.uint64).reshape(lanes, out_stride, 4), from_dev(d_b, np.uint64).reshape(lanes, out_stride, 4)
    assert np.array_equal(a, b)
    assert np.all(b[:, n // 2:] == np.uint64(0x5A5A5A5A5A5A5A5A)) and not np.any(b[:, :n // 2, 3] == np.uint64(0x5A5A5A5A5A5A5A5A))
    with pytest.raises(czk.CzkError) as e:
        ctx.fri_fold_at(d_f.data_ptr(), d_alpha.data_ptr(), lanes=lanes, n=1, stride=stride, out=d_b.data_ptr(), out_stride=out_stride)
    assert e.value.code == 1
    with pytest.raises(czk.CzkError) as e:
        ctx.fri_fold_at(d_f.data_ptr(), d_alpha.data_ptr(), lanes=lanes, n=n, stride=stride, out=d_f.data_ptr(), out_stride=out_stride)
    assert e.value.code == 3                                                            # out overlaps f
