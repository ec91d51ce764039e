"""polyvm.plonk_prove(..., fiat_shamir=True) and plonk.verify(..., fiat_shamir=True): the Plonk prover and verifier with their challenges drawn from the
transcript (czk_amd.transcript) as the reference's mpc-plonk/src/lib.rs drives it, on a backend whose lanes are each the plain prover.  The challenges are
held to a replay of tests/fs_model.py (hashlib.blake2s, a Python ChaCha20) over the proof's own commitments.  On SPDZ-2 and GSZ-3 Sharing backends the
commitments are opened where they are absorbed and the proof opens to the plain prover's.  Marlin the same way (marlin_prove, marlin.verify), at the
smallest |H| of tests/test_marlin_index.py's squaring chain."""
import copy
import random

import numpy as np
import pytest

import fs_model as F
from fs_model import Q_MOD
from util import R_MOD

pytestmark = pytest.mark.gpu
TAGS = ("public.x", "gates.x", "wiring.y", "wiring.z", "product.r", "wiring.x")
# mpc-plonk/src/lib.rs: commitments in the order they are made, draws at :283, :316, :207-208, :169, :237.  Written out again here on purpose, from
# the reference's text: prove() :411-421 commits p, then prove_public (pub_q :282, x :283), prove_gates (gates_q :315, x :316), prove_wiring (y, z
# :207-208, l1 :218, prove_unit_product: t :129, q :162, r :169; l2_q :236, x :237).  It can only be as right as that reading.
SCRIPT = (("absorb", "p"), ("absorb", "pub_q"), ("draw", "public.x"), ("absorb", "gates_q"), ("draw", "gates.x"), ("draw", "wiring.y"), ("draw", "wiring.z"),
          ("absorb", "l1"), ("absorb", "t"), ("absorb", "q"), ("draw", "product.r"), ("absorb", "l2_q"), ("draw", "wiring.x"))


@pytest.fixture(scope="module")
def gpu():
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    B = polyvm.GpuBackend(czk_amd, ctx, 2, polyvm.plonk_max_degree(16), lift=(1, 1))
    yield czk_amd, ctx, B
    ctx.close()


def circuit16():
    """16 gates, products and sums mixed, one public variable"""
    from czk_amd import plonk
    c = plonk.Circuit()
    a, b, x = c.new_var(), c.new_var(), c.new_pub_var("x")
    v = [a, b, x]
    for i in range(14):
        v.append(c.new_prod(v[-1], v[-3]) if i % 3 else c.new_sum(v[-1], v[-2]))
    c.new_sum(v[-1], a)
    c.pad_to_power_of_2()
    assert c.n_gates() == 16
    return c


_CASE = {}


def case(gpu):
    """layout, key, two witnesses and their fiat_shamir=True proofs, made once; tests work on copies"""
    if not _CASE:
        from czk_amd import plonk, polyvm
        _, _, B = gpu
        c = circuit16()
        lay = plonk.layout(B, c)
        _CASE.update(circuit=c, lay=lay, vk=plonk.verifier_key(lay), runs=[])
        for seed in (1, 2):
            rng = random.Random(seed)
            vals = c.evaluate([rng.randrange(R_MOD) for _ in range(c.n_vars - c.n_gates())])
            inp = plonk.prover_inputs(B, lay, vals)
            _CASE["runs"].append(dict(vals=vals, public={nm: vals[v] for v, nm in c.pub_vars.items()}, out=polyvm.plonk_prove(B, inp, fiat_shamir=True),
                                      plain=polyvm.plonk_prove(B, inp), plain_flag=polyvm.plonk_prove(B, inp, fiat_shamir=False)))
    return _CASE


def fq_canon(limbs) -> int:
    return sum(int(w) << (64 * i) for i, w in enumerate(limbs)) * pow(1 << 384, -1, Q_MOD) % Q_MOD


def point_bytes(cm) -> bytes:
    aff, inf = np.asarray(cm[0]).reshape(-1, 12)[0], bool(np.asarray(cm[1]).reshape(-1)[0])
    return F.g1_bytes(fq_canon(aff[:6]), fq_canon(aff[6:]), inf)


def commitment_bytes(cm, shifted=None) -> bytes:
    """to_bytes![c] of a marlin_pc commitment: comm, the bool, then the shifted commitment or the empty one"""
    return point_bytes(cm) + (b"\x00" + F.g1_bytes(0, 1, True) if shifted is None else b"\x01" + point_bytes(shifted))


def model_challenges(out) -> dict:
    m, c = F.FsModel().put((0).to_bytes(8, "little")).seed(), {}
    for what, name in SCRIPT:
        if what == "absorb":
            m.put(commitment_bytes(out[name + "_cmt"])).absorb()
        else:
            c["plonk." + name] = m.squeeze_fr()
    return c


def test_proofs_verify_and_their_challenges_equal_the_models_replay(gpu):
    from czk_amd import plonk
    _, _, B = gpu
    cs = case(gpu)
    for run in cs["runs"]:
        out = run["out"]
        assert plonk.verify(B, cs["vk"], run["public"], out, rng=random.Random(3), fiat_shamir=True) is True
        assert set(out["challenges"]) == {"plonk." + t for t in TAGS} and out["challenges"] == model_challenges(out)
        assert out["pub_q_open"]["point"] == out["challenges"]["plonk.public.x"] and out["p_x_open"]["point"] == out["challenges"]["plonk.wiring.x"]
        assert plonk.verify(B, cs["vk"], run["public"], out, rng=random.Random(3), fiat_shamir=False) is False      # not a stand-in proof
    a, b = (run["out"]["challenges"] for run in cs["runs"])
    assert all(a[t] != b[t] for t in a)                                                 # two witnesses, two sets of challenges


def test_stand_in_path_is_unchanged_by_the_flag(gpu):
    """Weaker than a pinned digest would be: the suite pins no Plonk output at this size, and the default call and fiat_shamir=False are one code path,
    so their equality shows only that the flag is inert.  What binds the stand-in path to its earlier behaviour here is that its openings sit at
    polyvm.challenge's points and that plonk.verify accepts; the existing provers' tests (test_shared_provers.py, test_plonk_layout.py) hold the rest."""
    from czk_amd import plonk, polyvm
    _, _, B = gpu
    cs = case(gpu)
    run = cs["runs"][0]
    plain, flagged = run["plain"], run["plain_flag"]
    assert "challenges" not in plain and set(plain) == set(flagged) == set(run["out"]) - {"challenges"}
    for k in plain:
        if k.endswith("_cmt"):
            assert all(np.array_equal(x, y) for x, y in zip(plain[k], flagged[k])), k
        else:
            assert plain[k]["point"] == flagged[k]["point"] and np.array_equal(plain[k]["value"], flagged[k]["value"]), k
    assert plain["pub_q_open"]["point"] == polyvm.challenge("plonk.public.x") and plain["q_r_open"]["point"] == polyvm.challenge("plonk.product.r")
    assert plonk.verify(B, cs["vk"], run["public"], plain, rng=random.Random(3)) is True
    assert plonk.verify(B, cs["vk"], run["public"], plain, rng=random.Random(3), fiat_shamir=True) is False


def test_changed_commitment_or_public_input_is_rejected(gpu):
    from czk_amd import plonk
    _, _, B = gpu
    cs = case(gpu)
    run = cs["runs"][0]
    ok = lambda out, public: plonk.verify(B, cs["vk"], public, out, rng=random.Random(3), fiat_shamir=True)   # noqa: E731
    assert ok(copy.deepcopy(run["out"]), run["public"]) is True
    other = cs["runs"][1]["out"]
    for label in ("p_cmt", "gates_q_cmt", "l2_q_cmt"):                                  # another valid group element in one commitment's place
        forged = copy.deepcopy(run["out"])
        forged[label] = copy.deepcopy(other[label])
        assert ok(forged, run["public"]) is False, label
    lied = copy.deepcopy(run["out"])
    lied["challenges"] = copy.deepcopy(other["challenges"])                             # the verifier reads no challenge from the proof
    assert ok(lied, run["public"]) is True
    assert ok(copy.deepcopy(run["out"]), dict(run["public"], x=(run["public"]["x"] + 1) % R_MOD)) is False


_SHARED = {}


def shared_case(gpu):
    """tests/test_shared_provers.py's random circuit at 2^4 gates, its layout and the plain ONE-lane prover's fiat_shamir=True proof, made once"""
    if not _SHARED:
        from czk_amd import plonk, polyvm
        from test_shared_provers import _plonk_circuit
        czk, ctx, _ = gpu
        c, vals, public = _plonk_circuit(16, 0x51 + 16)
        B1 = polyvm.GpuBackend(czk, ctx, 1, polyvm.plonk_max_degree(16))
        lay = plonk.layout(B1, c)
        plain = polyvm.plonk_prove(B1, plonk.prover_inputs(B1, lay, vals), fiat_shamir=True)
        _SHARED.update(vals=vals, public=public, B1=B1, lay=lay, vk=plonk.verifier_key(lay), plain=plain)
        assert plonk.verify(B1, _SHARED["vk"], public, plain, rng=random.Random(1), fiat_shamir=True) is True
        assert plain["challenges"] == model_challenges(plain)
    return _SHARED


@pytest.mark.parametrize("scheme", ["spdz-2", "gsz-3"])
def test_shared_backends_open_to_the_plain_provers_proof(gpu, scheme):
    """the same inputs and blinding on real shares: every commitment is opened where the transcript absorbs it, so the challenges are the plain
    prover's, and the proof opens to the plain prover's entry for entry"""
    from czk_amd import plonk, polyvm
    import test_gsz_provers
    import test_shared_provers
    czk, ctx, _ = gpu
    cs = shared_case(gpu)
    md = polyvm.plonk_max_degree(16)
    if scheme == "spdz-2":
        S = test_shared_provers._scheme(2, 2)
        B = polyvm.GpuBackend(czk, ctx, S.lanes, md, sharing=polyvm.Sharing(2, 2, polyvm.SeededDealer(7)), share_srs=cs["B1"])
        shares = test_shared_provers._shares(B, S, cs["vals"], 3)
    else:
        B = test_gsz_provers._backend((czk, ctx), 3, md, polyvm.SeededDealer(7), cs["B1"])
        shares = test_gsz_provers._shares(B, 3, cs["vals"], 3)
    out = polyvm.plonk_prove(B, plonk.prover_inputs(B, cs["lay"], shares), fiat_shamir=True)
    assert np.asarray(out["p_cmt"][0]).shape[0] == B.lanes                          # the proof is on share lanes ...
    assert out["challenges"] == cs["plain"]["challenges"]                           # ... its challenges came from the opened commitments
    opened = polyvm.open_shared_proof(B, out)
    assert plonk.verify(B, cs["vk"], cs["public"], opened, rng=random.Random(2), fiat_shamir=True) is True
    test_shared_provers._same(opened, cs["plain"])
    assert plonk.verify(B, cs["vk"], cs["public"], opened, rng=random.Random(2), fiat_shamir=False) is False
    if scheme == "spdz-2":
        bad = shares.clone()                                                        # one limb of party 1's mac lane: refused where the first commitment opens
        bad[3, 1, 0] ^= 1
        with pytest.raises(polyvm.SharingError):
            polyvm.plonk_prove(B, plonk.prover_inputs(B, cs["lay"], bad), fiat_shamir=True)


def test_one_party_per_process_says_not_built(gpu):
    from czk_amd import polyvm

    class Ranked:                                                                        # plonk_prove looks at the backend's `sharing` before anything else
        sharing = polyvm.Sharing(2, 2, polyvm.DummySource(), rank=1)

    with pytest.raises(ValueError, match="not built"):
        polyvm.plonk_prove(Ranked(), {}, fiat_shamir=True)
    t = polyvm.PlonkTranscript()
    with pytest.raises(ValueError, match="not built"):                                   # rows that differ are shares nobody opened
        t.absorb_commitment((np.arange(24, dtype=np.uint64).reshape(2, 12), np.zeros(2, dtype=np.uint8)))
    t.release()


# ---- Marlin -----------------------------------------------------------------------------------------------------------------------------
MARLIN_TAGS = ("alpha", "eta_a", "eta_b", "eta_c", "beta", "gamma", "opening_challenge")
_MARLIN = {}


def unmont1(limbs) -> int:
    return sum(int(w) << (64 * i) for i, w in enumerate(np.asarray(limbs, dtype=np.uint64).reshape(-1, 4)[0])) * pow(1 << 256, -1, R_MOD) % R_MOD


def marlin_case(gpu):
    """the smallest squaring chain of tests/test_marlin_index.py (|H| = 4), its index on a one-lane backend, two witnesses and their proofs"""
    if not _MARLIN:
        from czk_amd import marlin, polyvm
        from test_marlin_index import chain_circuit
        czk, ctx, _ = gpu
        B1 = polyvm.GpuBackend(czk, ctx, 1, polyvm.marlin_max_degree(4))
        _MARLIN.update(B1=B1, runs=[])
        for seed in (0x3A21 + 4, 0x77):
            mats, instance, witness = chain_circuit(4, seed)
            if "idx" not in _MARLIN:
                _MARLIN["idx"] = marlin.index(B1, mats["a"], mats["b"], mats["c"], 2, 2)          # the matrices do not depend on the seed
            inp = marlin.prover_inputs(B1, _MARLIN["idx"], instance, witness)
            _MARLIN["runs"].append(dict(instance=instance, witness=witness, out=polyvm.marlin_prove(B1, inp, fiat_shamir=True),
                                        plain=polyvm.marlin_prove(B1, inp)))
    return _MARLIN


def marlin_model_challenges(idx, instance, out) -> dict:
    """marlin/src/lib.rs:163-300 replayed by the model over the key, the public input, the proof's commitments and its evaluations"""
    info, H = idx["info"], idx["H"]
    m = F.FsModel().put(b"MARLIN-2019" + b"".join(int(info[k]).to_bytes(8, "little") for k in ("num_variables", "num_constraints", "num_non_zero")))
    for cm in idx["index_cmts"]:
        m.put(commitment_bytes(cm))
    x_pad = list(instance) + [0] * (idx["X"] - len(instance))
    m.put(b"".join(F.fr_bytes(v) for v in x_pad[1:])).seed()                       # unformat_public_input: without the leading one
    c = {}

    def outside():
        v = m.squeeze_fr()
        while pow(v, H, R_MOD) == 1:
            v = m.squeeze_fr()
        return v

    def absorb(labels):
        for l in labels:
            m.put(commitment_bytes(out[l + "_cmt"], out[l + "_shifted_cmt"] if l in ("g_1", "g_2") else None))
        m.absorb()
    absorb(("w", "z_a", "z_b", "mask_poly"))
    c["alpha"], c["eta_a"], c["eta_b"], c["eta_c"] = outside(), m.squeeze_fr(), m.squeeze_fr(), m.squeeze_fr()
    absorb(("t", "g_1", "h_1"))
    c["beta"] = outside()
    absorb(("g_2", "h_2"))
    c["gamma"] = m.squeeze_fr()
    # the published evaluations: z_b, t, g_1 at beta first; row, col, row_col of A, B, C at gamma, then g_2 (polyvm.marlin_prove's order)
    eb, eg = [unmont1(v) for v in out["evals_beta"]], [unmont1(v) for v in out["evals_gamma"]]
    den = [(c["beta"] * c["alpha"] - c["alpha"] * eg[3 * i] - c["beta"] * eg[3 * i + 1] + eg[3 * i + 2]) % R_MOD for i in range(3)]
    m.put(b"".join(F.fr_bytes(v) for v in den + [eb[2], eg[9], eb[1], eb[0]])).absorb()     # a_denom, b_denom, c_denom, g_1, g_2, t, z_b
    c["opening_challenge"] = m.squeeze_u128()
    return {"marlin." + k: v for k, v in c.items()}


def test_marlin_proofs_verify_and_their_challenges_equal_the_models_replay(gpu):
    from czk_amd import marlin
    cs = marlin_case(gpu)
    B1, idx = cs["B1"], cs["idx"]
    for run in cs["runs"]:
        out = run["out"]
        assert marlin.verify(B1, marlin.verifier_key(idx), run["instance"], out, rng=random.Random(1), fiat_shamir=True) is True
        assert set(out["challenges"]) == {"marlin." + t for t in MARLIN_TAGS}
        assert out["challenges"] == marlin_model_challenges(idx, run["instance"], out)
        assert out["open_beta"]["point"] == out["challenges"]["marlin.beta"] and out["open_gamma"]["point"] == out["challenges"]["marlin.gamma"]
        assert marlin.verify(B1, idx, run["instance"], out, rng=random.Random(1), fiat_shamir=False) is False
        assert "challenges" not in run["plain"] and marlin.verify(B1, idx, run["instance"], run["plain"], rng=random.Random(1)) is True
        assert marlin.verify(B1, idx, run["instance"], run["plain"], rng=random.Random(1), fiat_shamir=True) is False
    a, b = (run["out"]["challenges"] for run in cs["runs"])
    assert all(a[t] != b[t] for t in a)


def test_marlin_changed_commitment_evaluation_or_public_input_is_rejected(gpu):
    from czk_amd import marlin
    cs = marlin_case(gpu)
    B1, idx = cs["B1"], cs["idx"]
    run, other = cs["runs"][0], cs["runs"][1]["out"]
    ok = lambda out, x: marlin.verify(B1, idx, x, out, rng=random.Random(3), fiat_shamir=True)   # noqa: E731
    assert ok(copy.deepcopy(run["out"]), run["instance"]) is True
    for label in ("w_cmt", "g_1_shifted_cmt", "h_2_cmt"):
        forged = copy.deepcopy(run["out"])
        forged[label] = copy.deepcopy(other[label])
        assert ok(forged, run["instance"]) is False, label
    for tag, at in (("beta", 0), ("gamma", 9)):                                        # z_b(beta) and g_2(gamma): both are absorbed
        forged = copy.deepcopy(run["out"])
        v = (unmont1(forged["evals_" + tag][at]) + 1) % R_MOD * ((1 << 256) % R_MOD) % R_MOD
        forged["evals_" + tag][at] = np.array([[(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(4)]], dtype=np.uint64)
        assert ok(forged, run["instance"]) is False, tag
    x = list(run["instance"])
    x[1] = (x[1] + 1) % R_MOD
    assert ok(copy.deepcopy(run["out"]), x) is False
    lied = copy.deepcopy(run["out"])
    lied["challenges"] = copy.deepcopy(other["challenges"])                             # never read
    assert ok(lied, run["instance"]) is True


def test_marlin_on_spdz_shares_opens_to_the_plain_provers_proof(gpu):
    from czk_amd import marlin, polyvm
    import test_shared_provers
    czk, ctx, _ = gpu
    cs = marlin_case(gpu)
    B1, idx, run = cs["B1"], cs["idx"], cs["runs"][0]
    S = test_shared_provers._scheme(2, 2)
    B = polyvm.GpuBackend(czk, ctx, 4, polyvm.marlin_max_degree(4), sharing=polyvm.Sharing(2, 2, polyvm.SeededDealer(9)), share_srs=B1)
    shares = test_shared_provers._shares(B, S, run["witness"], 5)
    out = polyvm.marlin_prove(B, marlin.prover_inputs(B, idx, run["instance"], shares), fiat_shamir=True)
    assert out["challenges"] == run["out"]["challenges"]
    opened = polyvm.open_shared_proof(B, out)
    assert marlin.verify(B, idx, run["instance"], opened, rng=random.Random(2), fiat_shamir=True) is True
    drop = ("lcs", "lc_consts")
    test_shared_provers._same({k: v for k, v in opened.items() if k not in drop}, {k: v for k, v in run["out"].items() if k not in drop})
