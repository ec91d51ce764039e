"""czk_amd.fri.prove / verify_proof: the collaborative FRI of fri.py made non-interactive by a Fiat-Shamir transcript.  The device form (the transcript's
state on the GPU, the whole commit phase one enqueued sequence) and the host form (the same transcript through commit_phase's hook) must give identical
proofs, and both must equal tests/merkle_fri_model.py driven by tests/fs_model.py.  Every comparison is for exact equality."""
import copy

import numpy as np
import pytest

import fs_model as F
import merkle_fri_model as M
from util import R_MOD, limbs_to_ints, rand_fr_canonical

pytestmark = pytest.mark.gpu
SEED = b"fri test"


@pytest.fixture(scope="module")
def gpu():
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    yield czk_amd, ctx
    ctx.close()


def unmont(limbs):
    inv = pow(1 << 256, -1, R_MOD)
    return [v * inv % R_MOD for v in limbs_to_ints(np.asarray(limbs).reshape(-1, 4))]


def model_proof(canon, queries, seed):
    """the model's commit phase with alphas from the model transcript, then its query phase at the transcript's indices"""
    t = F.FsModel().put(seed).seed()
    state = M.commit_phase([limbs_to_ints(lane) for lane in canon], lambda i, roots: t.put(b"".join(roots)).absorb().squeeze_fr())
    t.put(F.fr_bytes(state["constant"])).absorb()
    starts = [t.squeeze_u64() % (1 << (state["k"] + 1)) for _ in range(queries)]
    return M.query_phase(state, starts), t


_PROOFS = {}


def proofs(gpu, orc, k, lanes, queries):
    """(device-form proof, host-form proof, model proof), made once per case"""
    key = (k, lanes, queries)
    if key not in _PROOFS:
        czk, ctx = gpu
        canon = rand_fr_canonical(5100 + 10 * k + lanes, lanes << k).reshape(lanes, 1 << k, 4)
        f = orc.fr_from_repr(canon.reshape(-1, 4)).reshape(lanes, 1 << k, 4)
        _PROOFS[key] = (czk.fri.prove(ctx, f, queries=queries, seed=SEED, device=True), czk.fri.prove(ctx, f, queries=queries, seed=SEED, device=False),
                        model_proof(canon, queries, SEED)[0])
    return _PROOFS[key]


def same(a, b) -> bool:
    if not all(a[key] == b[key] for key in ("k", "lanes", "x_indices", "roots", "constant")) or len(a["rounds"]) != len(b["rounds"]):
        return False
    return all(np.array_equal(x[key], y[key]) for x, y in zip(a["rounds"], b["rounds"]) for key in ("idx", "shares", "paths", "values"))


@pytest.mark.parametrize("queries", [1, 4])
@pytest.mark.parametrize("lanes", [2, 3])
@pytest.mark.parametrize("k", [1, 6])
def test_device_and_host_forms_give_the_models_proof_and_it_verifies(gpu, orc, k, lanes, queries):
    czk, ctx = gpu
    dev, host, model = proofs(gpu, orc, k, lanes, queries)
    assert same(dev, host)
    assert dev["k"] == model["k"] and dev["lanes"] == model["lanes"] and dev["constant"] == model["constant"]
    assert dev["roots"] == model["roots"] and dev["x_indices"] == model["x_indices"] and len(dev["x_indices"]) == queries
    for rd, want in zip(dev["rounds"], model["rounds"]):
        assert rd["idx"].tolist() == want["idx"] and unmont(rd["values"]) == want["values"]
        assert [unmont(rd["shares"][i]) for i in range(len(want["idx"]))] == want["shares"]
    assert czk.fri.verify_proof(ctx, dev, seed=SEED) is True and czk.fri.verify_proof(ctx, host, seed=SEED) is True
    assert czk.fri.verify_proof(ctx, dev, seed=SEED + b"!") is False                  # another seed draws other challenges


@pytest.mark.parametrize("lanes", [2, 3])
@pytest.mark.parametrize("k", [1, 6])
def test_changed_proofs_are_rejected(gpu, orc, k, lanes):
    czk, ctx = gpu
    good = proofs(gpu, orc, k, lanes, 4)[0]

    def rejected(change) -> bool:
        p = copy.deepcopy(good)
        change(p)
        return czk.fri.verify_proof(ctx, p, seed=SEED) is False

    def flip_root(p):
        r = bytearray(p["roots"][k - 1][lanes - 1])
        r[17] ^= 1
        p["roots"][k - 1][lanes - 1] = bytes(r)

    def flip_share(p):
        p["rounds"][0]["shares"][1, lanes - 1, 0] ^= np.uint64(1)

    def change_constant(p):
        p["constant"] = (p["constant"] + 1) % R_MOD

    def change_index(p):
        p["x_indices"][-1] = (p["x_indices"][-1] + 1) % (1 << (k + 1))

    assert czk.fri.verify_proof(ctx, copy.deepcopy(good), seed=SEED) is True
    assert rejected(flip_root) and rejected(flip_share) and rejected(change_constant) and rejected(change_index)
