"""czk_net_alltoall and czk_net_gsz_dn_generate / czk_net_gsz_dn_check (csrc/net.hip, csrc/net_rounds.hip, kernels in csrc/gsz_dn.hip): the GSZ material dealt and extracted
with ONE PARTY PER PROCESS, 3 and 4 processes sharing the GPU over CZK_NET_SHM.  The all-to-all delivers every byte through several chunk steps with a
ragged tail; every rank's generated lane is its lane of the lanes form on the same keys; the check gives every rank the lanes form's verdict in the
documented broadcasts, also when one dealt share is off by one; the generated material drives gsz20's product and product check; tails and write
footprints on a world of one.  Sizes are looped over INSIDE a spawn: starting the processes is what takes the time."""
import os
import random
import sys

import numpy as np
import pytest

import gsz_dn_model as DN
import gsz_mul_model as M
from gsz_mul_model import R_MOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A2A_BYTES, A2A_SLOT = 5000, 6144          # per destination: 2048-byte chunks at 3 ranks (2048, 2048, 904), 1536 at 4 (three full ones and 392)
DEALS = (1, 2, 65, 257)


def _keys(parties, seed):
    rng = random.Random(seed)
    return [bytes(rng.randrange(256) for _ in range(32)) for _ in range(parties)]


def _nonce(kind, seq):
    return kind.to_bytes(4, "little") + seq.to_bytes(8, "little")


def _payload(src, dst, nbytes):
    return ((np.arange(nbytes, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(977 * src + 131 * dst + 13)) >> np.uint64(5)).astype(np.uint8)


def _a2a_checks(net, rank, world, fails, exchange, tag):
    for nbytes in (A2A_BYTES, 1, 0, 16):
        net.stats_reset()
        got = exchange(np.stack([_payload(rank, p, nbytes) for p in range(world)]) if nbytes else np.zeros((world, 0), np.uint8), nbytes)
        for p in range(world):
            if not np.array_equal(got[p], _payload(p, rank, nbytes)):
                fails.append((tag, nbytes, "part", p))
        s = net.stats()
        if (s["bytes_sent"], s["bytes_recv"], s["broadcasts"], s["to_king"], s["from_king"]) != ((world - 1) * nbytes, (world - 1) * nbytes, 0, 0, 0):
            fails.append((tag, nbytes, s))


# ---- the all-to-all on host buffers: needs no GPU ------------------------------------------------------------------------------------------------------
def _a2a_host_party(rank, world, q, idb):
    sys.path.insert(0, ROOT)
    import czk_amd
    net = czk_amd.Net(None, czk_amd.CZK_NET_SHM, rank, world, idb, options={"slot_bytes": A2A_SLOT, "timeout_ms": 60000})
    fails = []
    _a2a_checks(net, rank, world, fails, lambda send, nbytes: net.alltoall(send), "host")
    net.barrier()
    net.close()
    q.put((rank, fails, None))


@pytest.mark.parametrize("world", [1, 3, 4])
def test_alltoall_delivers_every_byte_of_host_buffers(world):
    from test_net import _spawn
    assert world == 1 or (A2A_SLOT // world) // 16 * 16 * 2 < A2A_BYTES           # at least three chunk steps
    for rank, fails, _ in _spawn(_a2a_host_party, world, os.urandom(16), timeout=120):
        assert fails == [], (rank, fails)


# ---- what the parties do on the GPU, one function per test (run in every spawned process) ----------------------------------------------------------------
def _s_alltoall(c, net, rank, world, fails):
    import torch
    import czk_amd

    def device(send, nbytes):
        s = torch.from_numpy(send.copy()).cuda()
        r = torch.full((world, max(nbytes, 1)), 0xEE, dtype=torch.uint8, device="cuda")[:, :nbytes].contiguous()
        torch.cuda.synchronize()                                    # torch fills on its own stream, the exchange runs on the context's
        net.alltoall(s.data_ptr() if nbytes else None, nbytes, r.data_ptr() if nbytes else None, mem=czk_amd.CZK_MEM_DEVICE)
        c.sync()
        return r.cpu().numpy()
    _a2a_checks(net, rank, world, fails, device, "device")
    _a2a_checks(net, rank, world, fails, lambda send, nbytes: net.alltoall(send), "host")


def _lanes_form(c, kind, world, d, keys, nonce, deal):
    """the lanes form on all keys, in this process -> (r, r2) device tensors (world, outputs, 4)"""
    import torch
    outputs = deal * (world - d)
    r = torch.empty((world, outputs, 4), dtype=torch.int64, device="cuda")
    r2 = torch.empty_like(r) if kind == DN.KIND_DOUBLES else None
    c.gsz_dn_generate(kind, world, d, keys, nonce, deal, r.data_ptr(), None if r2 is None else r2.data_ptr())
    return r, r2


def _net_generate(net, kind, d, key, nonce, deal, world):
    import torch
    outputs = deal * (world - d)
    r = torch.empty((outputs, 4), dtype=torch.int64, device="cuda")
    r2 = torch.empty_like(r) if kind == DN.KIND_DOUBLES else None
    net.gsz_dn_generate(kind, d, key, nonce, deal, r.data_ptr(), None if r2 is None else r2.data_ptr())
    return r, r2


def _ptr(t):
    return None if t is None else t.data_ptr()


def _s_generate(c, net, rank, world, fails):
    """every deal, both kinds: the lane, the all-to-all's bytes, the check's verdict and broadcasts; then one dealt share off by one"""
    import torch
    d, keys = M.threshold(world), _keys(world, 300 + world)
    w = M.Domain(world).w
    for kind in (DN.KIND_DOUBLES, DN.KIND_RANDS):
        halves = 2 if kind == DN.KIND_DOUBLES else 1
        for deal in DEALS:
            nonce, outputs = _nonce(kind, deal), deal * (world - d)
            net.stats_reset()
            r, r2 = _net_generate(net, kind, d, keys[rank], nonce, deal, world)
            s = net.stats()
            if (s["bytes_sent"], s["bytes_recv"], s["broadcasts"], s["to_king"], s["from_king"]) != ((world - 1) * halves * deal * 32,) * 2 + (0, 0, 0):
                fails.append((kind, deal, s))
            fr, fr2 = _lanes_form(c, kind, world, d, keys, nonce, deal)
            c.sync()
            if not torch.equal(r, fr[rank]) or (r2 is not None and not torch.equal(r2, fr2[rank])):
                fails.append((kind, deal, "lane"))
            if outputs < 3:
                continue
            net.stats_reset()
            got = net.gsz_dn_check(kind, d, r.data_ptr(), _ptr(r2), outputs)
            s = net.stats()
            if got != (True, 0) or got != c.gsz_dn_check(kind, world, d, fr.data_ptr(), _ptr(fr2), outputs):
                fails.append((kind, deal, "check", got))
            opens = 3 if kind == DN.KIND_DOUBLES else 2
            if (s["broadcasts"], s["to_king"], s["from_king"], s["bytes_sent"]) != (opens, 0, 0, opens * (world - 1) * 32):
                fails.append((kind, deal, "check stats", s))
            # rank 1 adds one to the share of its item b that it sends to rank 2: by linearity rank 2's outputs k deal + b move by w^(1 k), and nobody else's.
            # A value, not a fault: the extraction is applied to what arrived.
            b = deal // 2
            for lanes in ([r] if rank == 2 else []) + [fr[2]]:
                for k in range(world - d):
                    at = k * deal + b
                    v = (M.from_limbs(lanes[at:at + 1].cpu().numpy().view(np.uint64)[None])[0][0] + pow(w, k, R_MOD)) % R_MOD
                    lanes[at] = torch.from_numpy(M.to_limbs([[v]])[0].view(np.int64)).cuda()[0]
            torch.cuda.synchronize()                                # torch wrote on its own stream, the checks run on the context's
            got = net.gsz_dn_check(kind, d, r.data_ptr(), _ptr(r2), outputs)
            want = c.gsz_dn_check(kind, world, d, fr.data_ptr(), _ptr(fr2), outputs)
            if got[0] is not False or got != want:
                fails.append((kind, deal, "cheat", got, want))


def _s_use(c, net, rank, world, fails):
    """n = 33: generated doubles multiply x and y to the model's lane; generated doubles and random shares pass the product check on the triples"""
    import torch
    D, d, n = M.Domain(world), M.threshold(world), 33
    keys, rng = _keys(world, 400 + world), random.Random(world)
    xv, yv = [rng.randrange(R_MOD) for _ in range(n)], [rng.randrange(R_MOD) for _ in range(n)]
    x, y = D.share(xv, d, rng), D.share(yv, d, rng)

    def material(kind, want, seq):
        deal, outputs = DN.counts(kind, world, d, want + 2)
        r, r2 = _net_generate(net, kind, d, keys[rank], _nonce(kind, seq), deal, world)
        if net.gsz_dn_check(kind, d, r.data_ptr(), _ptr(r2), outputs) != (True, 0):
            fails.append(("material", kind, seq))
        mr, mr2 = DN.generate(D, kind, d, keys, _nonce(kind, seq), deal)
        out = r[:want].contiguous(), (None if r2 is None else r2[:want].contiguous()), [ln[:want] for ln in mr], (None if mr2 is None else [ln[:want] for ln in mr2])
        torch.cuda.synchronize()                                    # torch copied on its own stream, the protocols run on the context's
        return out

    dev = lambda lane: torch.from_numpy(M.to_limbs([lane])[0].view(np.int64)).cuda()      # noqa: E731
    dr, dr2, mdr, mdr2 = material(DN.KIND_DOUBLES, n, 1)
    z = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    xd, yd = dev(x[rank]), dev(y[rank])
    if net.gsz_share_batch_mul(d, xd.data_ptr(), yd.data_ptr(), dr.data_ptr(), dr2.data_ptr(), z.data_ptr(), n) != (0, 0):
        fails.append("mul counts")
    want, bad = M.batch_mult(D, d, x, y, M.Material(mdr, mdr2, [[] for _ in range(world)]))
    c.sync()
    if bad or not np.array_equal(z.cpu().numpy().view(np.uint64), M.to_limbs(want)[rank]):
        fails.append("mul lane")
    if D.batch_open(want, d) != ([a * b % R_MOD for a, b in zip(xv, yv)], 0):
        fails.append("model product")
    nd, nr = M.material_counts(M.OP_PRODUCT_CHECK, n)
    cr, cr2, _, _ = material(DN.KIND_DOUBLES, nd, 2)
    rands, _, _, _ = material(DN.KIND_RANDS, nr, 3)
    if net.gsz_product_check(d, xd.data_ptr(), yd.data_ptr(), z.data_ptr(), n, cr.data_ptr(), cr2.data_ptr(), rands.data_ptr()) != (True, 0):
        fails.append("product check")


SCENARIOS = {f.__name__: f for f in (_s_alltoall, _s_generate, _s_use)}


def _party(rank, world, q, idb, scenario, slot_bytes):
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    import czk_amd
    torch.cuda.set_device(0)
    c = czk_amd.Context(0)
    opts = {"timeout_ms": 60000}
    if slot_bytes:
        opts["slot_bytes"] = slot_bytes
    net = czk_amd.Net(c, czk_amd.CZK_NET_SHM, rank, world, idb, options=opts)
    fails = []
    SCENARIOS[scenario](c, net, rank, world, fails)
    net.barrier()
    net.close()
    c.close()
    q.put((rank, fails, None))


def _parties(world, scenario, slot_bytes=0):
    from test_net import _spawn
    res = _spawn(_party, world, os.urandom(16), scenario.__name__, slot_bytes, timeout=120)
    assert [r for r, _, _ in res] == list(range(world))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("world", [3, 4])
def test_alltoall_delivers_every_byte_of_device_buffers(world):
    for rank, fails, _ in _parties(world, _s_alltoall, A2A_SLOT):
        assert fails == [], (rank, fails)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [3, 4])
def test_every_rank_generates_its_lane_and_gets_the_lanes_forms_verdict(world):
    for rank, fails, _ in _parties(world, _s_generate):
        assert fails == [], (rank, fails)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [3, 4])
def test_generated_material_drives_the_net_product_and_product_check(world):
    for rank, fails, _ in _parties(world, _s_use):
        assert fails == [], (rank, fails)


# ---- tails and write footprints, one process, a world of one ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    import czk_amd
    c = czk_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def net1(ctx):
    import czk_amd
    net = czk_amd.Net(ctx, czk_amd.CZK_NET_SHM, 0, 1, os.urandom(16))
    yield net
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_tails_and_footprints_of_the_party_kernels(ctx, net1, which):
    """k_gsz_dn_deal and k_gsz_dn_extract either side of the second trip of their grid-stride loops, inside guard bands, on a world of one (the all-to-all
    is a local copy there): with one party and degree 0 output b IS the dealer's secret b, element b of czk_fr_random's stream, and the lanes form with
    parties = 1 writes the same"""
    import guarded
    from guarded import Guards
    import torch
    from test_gsz_dn import _per_cu_blocks
    import czk_amd
    T = guarded.grid_threads(_per_cu_blocks())
    deal = [T - 1, T + 3][which]
    key = _keys(1, 9)[0]
    for kind in (DN.KIND_DOUBLES, DN.KIND_RANDS):
        nonce = _nonce(kind, 5)
        G = Guards("cuda")
        names = ("r", "r2", "lanes_r", "lanes_r2", "stream") if kind == DN.KIND_DOUBLES else ("r", "lanes_r", "stream")
        o = {k: G.out(1, deal, name=k) for k in names}
        torch.cuda.synchronize()                                    # the guard bands are filled on torch's stream, the calls run on the context's
        net1.gsz_dn_generate(kind, 0, key, nonce, deal, o["r"].ptr, o["r2"].ptr if "r2" in o else None)
        ctx.gsz_dn_generate(kind, 1, 0, [key], nonce, deal, o["lanes_r"].ptr, o["lanes_r2"].ptr if "r2" in o else None)
        ctx.fr_random(key, nonce, 0, deal, out=o["stream"].ptr, mem=czk_amd.CZK_MEM_DEVICE)
        ctx.sync()
        foot = dict(zip(names, G.check()))
        assert all(np.array_equal(foot[k], foot["stream"]) for k in names), kind
        assert np.array_equal(foot["r"][0, -3:], M.to_limbs([DN.sample(key, nonce, deal - 3, 3)])[0])
        net1.stats_reset()
        assert net1.gsz_dn_check(kind, 0, o["r"].ptr, o["r2"].ptr if "r2" in o else None, deal) == (True, 0)
        s = net1.stats()
        assert (s["broadcasts"], s["to_king"], s["from_king"]) == (3 if kind == DN.KIND_DOUBLES else 2, 0, 0)


@pytest.mark.gpu
def test_argument_rules(ctx, net1):
    import czk_amd
    from guarded import Guards

    def code(fn, *a):
        try:
            fn(*a)
        except czk_amd.binding.CzkError as e:
            return e.code
        return 0
    G = Guards("cuda")
    r, r2 = G.out(1, 16, name="r"), G.out(1, 16, name="r2")
    import torch
    torch.cuda.synchronize()
    key, nonce = _keys(1, 1)[0], _nonce(0, 0)
    gen, chk = net1.gsz_dn_generate, net1.gsz_dn_check
    assert code(gen, DN.KIND_RANDS, 1, key, nonce, 4, r.ptr) == 3                       # d >= world
    assert code(gen, DN.KIND_DOUBLES, 1, key, nonce, 4, r.ptr, r2.ptr) == 3             # 2 d >= world
    assert code(gen, 7, 0, key, nonce, 4, r.ptr, r2.ptr) == 3
    assert code(gen, DN.KIND_DOUBLES, 0, key, nonce, 4, r.ptr, None) == 3
    assert code(gen, DN.KIND_RANDS, 0, key, nonce, (1 << 32) + 1, r.ptr) == 1           # deal draws > 2^32
    assert code(gen, DN.KIND_DOUBLES, 0, key, nonce, 0, None, None) == 0                # nothing to do
    assert code(chk, DN.KIND_RANDS, 0, r.ptr, None, 2) == 3
    assert code(chk, DN.KIND_DOUBLES, 0, r.ptr, None, 8) == 3
    ctx.sync()
    assert r.untouched() and r2.untouched()
    host_only = czk_amd.Net(None, czk_amd.CZK_NET_SHM, 0, 1, os.urandom(16))
    assert code(host_only.gsz_dn_generate, DN.KIND_RANDS, 0, key, nonce, 4, r.ptr) == 3  # a communicator without a context
    assert code(host_only.gsz_dn_check, DN.KIND_RANDS, 0, r.ptr, None, 8) == 3
    host_only.close()
