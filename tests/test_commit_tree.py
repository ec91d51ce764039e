"""czk_fr_vec_commit and the commit-then-open round built on it (include/czk.h "czk tree commitment v1") on the GPU: parity with the hashlib model
(tests/commit_tree_model.py), the read footprint, sensitivity, the net round with 2 / 3 processes on one GPU, czk_spdz_batch_open's third commit
mode and the compiled host's --tree-commit-opens.  E and F come from the binding, never from here."""
import os
import re
import sys

import numpy as np
import pytest

import commit_tree_model as model
from util import R_MOD, ints_to_limbs, rand_fr_canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import czk_amd  # noqa: E402

pytestmark = pytest.mark.gpu

E, F = czk_amd.binding.CZK_COMMIT_LEAF_ELEMS, czk_amd.binding.CZK_COMMIT_FANOUT
SIZES = {"0": 0, "1": 1, "E-1": E - 1, "E": E, "E+1": E + 1, "EF-1": E * F - 1, "EF": E * F, "EF+1": E * F + 1, "EFF+1": E * F * F + 1}
N_MAX = max(SIZES.values())


def _rand32(seed: int, lanes: int = 1) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, 32 * lanes, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def pool():
    """seeded canonical Fr, computed once (read-only): three lanes' worth of the largest size"""
    canon = rand_fr_canonical(2024, 3 * N_MAX + 64)
    canon.setflags(write=False)
    return canon


def _vector(orc, pool, n: int, lane: int = 0):
    """(canonical, Montgomery) limbs of n elements with 0, r - 1, 1 and r - 1 planted at 0, E - 1, E and n - 1: the leaf seams"""
    canon = pool[lane * N_MAX:lane * N_MAX + n].copy()
    for idx, v in ((0, 0), (E - 1, R_MOD - 1), (E, 1), (n - 1, R_MOD - 1)):
        if 0 <= idx < n:
            canon[idx] = ints_to_limbs([v], 4)[0]
    mont = orc.fr_from_repr(canon) if n else np.zeros((0, 4), np.uint64)
    return canon, np.ascontiguousarray(mont)


@pytest.fixture(scope="module")
def ctx():
    c = czk_amd.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("size", list(SIZES))
def test_commitment_matches_the_model(orc, pool, ctx, size, mem):
    n = SIZES[size]
    canon, mont = _vector(orc, pool, n)
    rnd = _rand32(n)
    want = model.commit(canon, rnd, E, F)
    if mem == "host":
        got = ctx.fr_vec_commit(mont, rnd, n=n)
    else:
        d = _dev(mont.reshape(-1, 4)) if n else None
        got = ctx.fr_vec_commit(d.data_ptr() if n else None, rnd, n=n, mem=czk_amd.CZK_MEM_DEVICE)
    print(f"n = {n} ({mem}): {got.hex()} want {want.hex()}")
    assert got == want


@pytest.mark.parametrize("mem", ["host", "device"])
def test_lanes_with_a_stride_and_their_own_randomness(orc, pool, ctx, mem):
    n, lanes = E * F + 1, 3
    stride = n + 5
    buf = np.ascontiguousarray(pool[:lanes * stride].copy())               # the stride padding holds other values, never read
    want = b""
    rnd = _rand32(77, lanes)
    for lane in range(lanes):
        canon, mont = _vector(orc, pool, n, lane)
        buf[lane * stride:lane * stride + n] = mont
        want += model.commit(canon, rnd[32 * lane:32 * lane + 32], E, F)
    if mem == "host":
        got = ctx.fr_vec_commit(buf, rnd, lanes=lanes, n=n, stride=stride)
    else:
        got = ctx.fr_vec_commit(_dev(buf).data_ptr(), rnd, lanes=lanes, n=n, stride=stride, mem=czk_amd.CZK_MEM_DEVICE)
    assert got == want
    assert len({got[32 * k:32 * k + 32] for k in range(lanes)}) == lanes


def test_argument_checks(ctx, pool):
    x = np.ascontiguousarray(pool[:8].copy())
    with pytest.raises(czk_amd.CzkError) as e:
        ctx.fr_vec_commit(x, bytes(32), n=8, stride=7)
    assert e.value.code == 1                                               # CZK_ERR_SIZE
    with pytest.raises(czk_amd.CzkError) as e:
        ctx.fr_vec_commit(x, bytes(64), lanes=2, n=8, stride=2**62)
    assert e.value.code == 1
    assert ctx.fr_vec_commit(None, b"", lanes=0, n=8, stride=8) == b""      # no lanes: nothing touched
    with pytest.raises(czk_amd.CzkError) as e:
        ctx.fr_vec_commit(None, bytes(32), lanes=1, n=8, stride=8, mem=czk_amd.CZK_MEM_DEVICE)
    assert e.value.code == 3                                               # CZK_ERR_ARG


def _leaf_grid_cap() -> int:
    """blocks per CU that cap the grids of commit_tree.hip, on blocks of 256 threads (tests/test_guarded_cpu.py reads the other files' caps the same way)"""
    src = open(os.path.join(ROOT, "collaborative-zksnark_amd", "csrc", "commit_tree.hip")).read()
    caps = re.findall(r"\bconstexpr unsigned BLOCKS_PER_CU = (\d+);", src)
    assert len(caps) == 1 and "(size_t)ctx->num_cu * BLOCKS_PER_CU" in src and "dim3(256)" in src
    return int(caps[0])


def _footprint_cases():
    return ["EF+1", "T-1", "T+3"]


@pytest.mark.parametrize("case", _footprint_cases())
def test_reads_stay_inside_and_the_input_is_unchanged(orc, ctx, case):
    """Two buffers that agree on [0, n) of every lane and differ everywhere else -- the pads in front and behind, the stride padding -- give equal
    commitments, and the call leaves its input bit-identical.  T-1 / T+3: lane counts either side of the second trip of the leaf kernel's
    grid-stride loop (one leaf per lane), the grid cap read from the source."""
    import torch
    from guarded import Guards, grid_threads
    if case == "EF+1":
        lanes, n, stride = 2, E * F + 1, E * F + 4
    else:
        t = grid_threads(_leaf_grid_cap())
        lanes, n, stride = (t - 1 if case == "T-1" else t + 3), 2, 3
    pad = 128
    total = 2 * pad + lanes * stride
    a = rand_fr_canonical(31, total)                                        # any value below r is a Montgomery form
    b = rand_fr_canonical(32, total)
    inner_a = a[pad:pad + lanes * stride].reshape(lanes, stride, 4)
    inner_b = b[pad:pad + lanes * stride].reshape(lanes, stride, 4)
    inner_b[:, :n] = inner_a[:, :n]
    assert not np.array_equal(inner_a[:, n:], inner_b[:, n:]) and not np.array_equal(a[:pad], b[:pad])
    rnd = _rand32(5, lanes)
    G = Guards("cuda")
    fa, fb = G.freeze(a, "a"), G.freeze(b, "b")
    torch.cuda.synchronize()
    got_a = ctx.fr_vec_commit(fa.ptr + 32 * pad, rnd, lanes=lanes, n=n, stride=stride, mem=czk_amd.CZK_MEM_DEVICE)
    got_b = ctx.fr_vec_commit(fb.ptr + 32 * pad, rnd, lanes=lanes, n=n, stride=stride, mem=czk_amd.CZK_MEM_DEVICE)
    G.check()
    assert got_a == got_b
    for lane in sorted(k for k in {0, 1, lanes // 2, lanes - 4, lanes - 3, lanes - 1} if 0 <= k < lanes):   # lanes - 3: the first item of the second trip at T + 3
        want = model.commit(orc.fr_into_repr(np.ascontiguousarray(inner_a[lane, :n])), rnd[32 * lane:32 * lane + 32], E, F)
        assert got_a[32 * lane:32 * lane + 32] == want, lane
    # every lane has its own data and randomness: no two commitments coincide (a lane written twice or skipped would show here)
    assert len({got_a[32 * k:32 * k + 32] for k in range(lanes)}) == lanes


def test_every_input_bit_reaches_the_commitment(orc, pool, ctx):
    n = E * F + 1
    mont = orc.fr_from_repr(np.ascontiguousarray(pool[:n]))
    rnd = _rand32(9)
    base = ctx.fr_vec_commit(mont, rnd, n=n)
    seen = {base}
    for idx in (0, E - 1, E, n - 1):
        for limb, bit in ((0, 0), (3, 40)):
            x = mont.copy()
            x[idx, limb] ^= np.uint64(1 << bit)
            seen.add(ctx.fr_vec_commit(x, rnd, n=n))
    for byte, bit in ((0, 0), (31, 7)):
        r2 = bytearray(rnd)
        r2[byte] ^= 1 << bit
        seen.add(ctx.fr_vec_commit(mont, bytes(r2), n=n))
    seen.add(ctx.fr_vec_commit(mont[:n - 1], rnd, n=n - 1))                 # the same data, one element shorter
    seen.add(ctx.fr_vec_commit(mont, rnd, n=n - 1, stride=n))
    assert len(seen) == 1 + 8 + 2 + 1                                       # (the two truncations are one commitment)


def test_parallel_layer_world_of_one(orc, pool, ctx):
    """parallel.atomic_broadcast / spdz_batch_open with the tree commitment on the torch.distributed path (no process group: a world of one)"""
    import torch
    from czk_amd import parallel
    n = E + 1
    _, mont = _vector(orc, pool, n)
    x = _dev(mont)
    torch.cuda.synchronize()
    got = parallel.atomic_broadcast(ctx, x, tree=True)
    ctx.sync()
    assert got.shape == (1, n, 4) and torch.equal(got[0], x)
    one = np.array([1, 0, 0, 0], dtype=np.uint64)
    mac_share = orc.fr_from_repr(one.reshape(1, 4))[0]
    vals = {c: parallel.spdz_batch_open(ctx, x, x.clone(), mac_share, commit=c) for c in (False, True, "tree")}   # mac = 1 * value
    ctx.sync()
    assert all(torch.equal(v, x) for v in vals.values())
    with pytest.raises(ValueError):
        parallel.spdz_batch_open(ctx, x, x.clone(), mac_share, commit="sha3")


# ---- the net round: one process per party on one GPU (the _spawn pattern of tests/test_net.py) ------------------------------------------------
def _party_vector(rank, n):
    return rand_fr_canonical(5 + rank, n)                                  # read as Montgomery limbs: any value below r is one


def _setup(rank, world, idb, transport):
    os.environ["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch
    torch.cuda.set_device(0)
    c = czk_amd.Context(0)
    return torch, c, czk_amd.Net(c, transport, rank, world, idb, options={"timeout_ms": 60000})


def _tree_worker(rank, world, q, idb, transport):
    torch, c, net = _setup(rank, world, idb, transport)
    ok = True
    for n in (1, E * F + 1):
        x = torch.from_numpy(_party_vector(rank, n).view(np.int64)).cuda()
        allx = torch.zeros((world, n, 4), dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        net.stats_reset()
        net.atomic_broadcast(x.data_ptr(), n, allx.data_ptr(), rand32=bytes([rank + 1]) * 32, tree=True)
        st_tree = net.stats()
        c.sync()
        ok = ok and all(np.array_equal(allx[p].cpu().numpy().view(np.uint64), _party_vector(p, n)) for p in range(world))
        net.stats_reset()
        net.atomic_broadcast(x.data_ptr(), n, allx.data_ptr(), tree=True)   # randomness from the OS
        net.stats_reset()
        net.atomic_broadcast(x.data_ptr(), n, allx.data_ptr(), rand32=bytes([rank + 1]) * 32)
        ok = ok and net.stats() == st_tree                                  # counted like the SHA-256 round
    net.barrier()
    net.close()
    c.close()
    q.put((rank, ok))


@pytest.mark.parametrize("transport", ["shm", "ipc"])
@pytest.mark.parametrize("world", [2, 3])
def test_atomic_broadcast_tree_returns_every_partys_vector(world, transport):
    from test_net import _spawn
    t = czk_amd.CZK_NET_SHM if transport == "shm" else czk_amd.CZK_NET_IPC
    assert _spawn(_tree_worker, world, os.urandom(16), t, timeout=120) == [(r, True) for r in range(world)]


def _cheat_worker(rank, world, q, idb, mode):
    torch, c, net = _setup(rank, world, idb, czk_amd.CZK_NET_SHM)
    n = E * F + 1
    x = torch.from_numpy(_party_vector(rank, n).view(np.int64)).cuda()
    allx = torch.empty((world, n, 4), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rnd = bytes([7 + rank]) * 32
    code = 0
    try:
        if mode == "mixed":                                                 # rank 0 commits with the tree, rank 1 with SHA-256: equal byte counts, nobody hangs
            net.atomic_broadcast(x.data_ptr(), n, allx.data_ptr(), rand32=rnd, tree=rank == 0)
        elif rank == 1:                                                     # the two rounds by hand with the byte primitives, as a party that cheats would run them
            commit = np.frombuffer(c.fr_vec_commit(x.data_ptr(), rnd, n=n, mem=czk_amd.CZK_MEM_DEVICE), dtype=np.uint8)
            net.broadcast(commit)
            if mode == "data":
                x[n - 1, 2] ^= 1                                            # changes a limb of its LAST element after committing
                torch.cuda.synchronize()
            net.broadcast(x.data_ptr(), nbytes=32 * n, recv=allx.data_ptr(), mem=1)
            sent = bytearray(rnd)
            if mode == "rand":
                sent[17] ^= 0x20
            net.broadcast(np.frombuffer(bytes(sent), dtype=np.uint8))
        else:
            net.atomic_broadcast(x.data_ptr(), n, allx.data_ptr(), rand32=rnd, tree=True)
    except czk_amd.CzkError as e:
        code = e.code
    net.close()
    c.close()
    q.put((rank, code))


@pytest.mark.parametrize("mode,want", [("honest", [(0, 0), (1, 0)]), ("data", [(0, 6), (1, 0)]), ("rand", [(0, 6), (1, 0)]), ("mixed", [(0, 6), (1, 6)])])
def test_atomic_broadcast_tree_detects_a_party_that_does_not_open_its_commitment(mode, want):
    """channel.rs:63-66 with the tree commitment: changed data, changed randomness, and a peer that used the other commitment are all CZK_ERR_CHECK (6);
    the hand-run rounds with nothing changed pass"""
    from test_net import _spawn
    assert _spawn(_cheat_worker, 2, os.urandom(16), mode, timeout=120) == want


def _open_worker(rank, world, q, idb, transport):
    torch, c, net = _setup(rank, world, idb, transport)
    import orc
    from test_net import _spdz_inputs
    n = E * F + 1
    secret, alpha, shs, macs = _spdz_inputs(orc, world, n)
    sh = torch.from_numpy(shs[rank].view(np.int64)).cuda()
    mac = torch.from_numpy(macs[rank].view(np.int64)).cuda()
    bad_mac = mac.clone()
    if rank == world - 1:
        bad_mac[5, 0] ^= 1
        bad_mac[n - 1, 3] ^= 4
    out = torch.empty_like(sh)
    fails, stats, bad = [], {}, {}
    for commit in (False, True, "tree"):
        out.zero_()
        torch.cuda.synchronize()
        net.stats_reset()
        if net.spdz_batch_open(sh.data_ptr(), mac.data_ptr(), alpha[rank], n, out.data_ptr(), commit=commit) != 0:
            fails.append(("bad", commit))
        stats[commit] = net.stats()
        c.sync()
        if not np.array_equal(out.cpu().numpy().view(np.uint64), secret):
            fails.append(("value", commit))
        bad[commit] = net.spdz_batch_open(sh.data_ptr(), bad_mac.data_ptr(), alpha[rank], n, out.data_ptr(), commit=commit)
    if not (bad[False] == bad[True] == bad["tree"] == 2):
        fails.append(("tampered", bad))
    if stats["tree"] != stats[True] or stats["tree"]["broadcasts"] != 3 or stats[False]["broadcasts"] != 2:
        fails.append(("stats", stats))
    net.barrier()
    net.close()
    c.close()
    q.put((rank, fails))


@pytest.mark.parametrize("world,transport", [(2, "shm"), (3, "ipc")])
def test_spdz_batch_open_with_the_tree_commitment(world, transport):
    from test_net import _spawn
    t = czk_amd.CZK_NET_SHM if transport == "shm" else czk_amd.CZK_NET_IPC
    assert _spawn(_open_worker, world, os.urandom(16), t, timeout=120) == [(r, []) for r in range(world)]


def test_compiled_host_with_tree_commit_opens():
    """tools/host_demo.cpp party-launch --tree-commit-opens: the proofs of the default (SHA-256) run and of the one-process layout, the reference's
    message count, and the commit mode in the JSON line"""
    import subprocess
    from test_abi import _build_host_demo
    from test_net import _json_tail
    from util import run_ranks
    exe = _build_host_demo()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    size = ["--log-n", "12", "--steps", "2", "--warmup", "1"]
    tree = _json_tail(run_ranks([exe, "party-launch", "--world", "2"] + size + ["--tree-commit-opens"], capture_output=True, text=True, timeout=300, env=env))
    assert tree["commit_hash"] == "tree" and tree["commit_opens"] is True
    assert tree["king_net_stats"]["broadcasts"] == 2 * 2 * 3
    default = _json_tail(run_ranks([exe, "party-launch", "--world", "2"] + size, capture_output=True, text=True, timeout=300, env=env))
    assert default["commit_hash"] == "sha256" and default["commit_opens"] is True
    assert default["king_net_stats"] == tree["king_net_stats"]
    one = _json_tail(subprocess.run([exe, "bench", "--parties", "2"] + size, capture_output=True, text=True, timeout=300, env=env))
    assert tree["results_sha256"] == default["results_sha256"] == one["results_sha256"]
