"""Plonk's circuit layout on the GPU and the Plonk verifier (czk_amd.plonk, csrc/plonk_layout.hip).

1. czk_plonk_layout against a big-integer model -- w_evals[i] = w^succ[i] with w read back from the library and checked to generate the domain of
   3 n_gates points whose cube is the gate domain's generator (relations/flat.rs:282-300) -- every limb, host and device memory, one, two and three of
   the four per-byte power tables in use (the fourth needs more than 2^24 wire slots: not exercised); its error codes and messages.
2. czk_fr_gather against numpy indexing: lanes, strides with padding that must stay, sizes around a block, both kinds of memory, indices out of range.
3. plonk.layout / prover_inputs: s and w evaluated back on their domains are the model's vectors, p on the wire domain is values[var_layout] per lane.
4. layout -> prover_inputs -> polyvm.plonk_prove -> plonk.verify, the verifier's negative cases one change at a time, and agreement with the
   verifier model of tests/polyiop_real.py where that model applies (one public wire at slot 1).
"""
import copy
import random

import numpy as np
import pytest

from groth16_real_key import omega_for
from test_plonk_layout_cpu import hand_made, naive_wiring, random_circuit
from util import R_MOD, ints_to_limbs, limbs_to_ints

pytestmark = pytest.mark.gpu
RR = (1 << 256) % R_MOD
R_INV = pow(1 << 256, -1, R_MOD)
ERR_SIZE, ERR_ARG = 1, 3


def mont(vals):
    return ints_to_limbs([v % R_MOD * RR % R_MOD for v in vals], 4).reshape(-1, 4)


def unmont(limbs):
    return [v * R_INV % R_MOD for v in limbs_to_ints(np.asarray(limbs).reshape(-1, 4))]


@pytest.fixture(scope="module")
def gpu():
    """(czk_amd, context, two-lane backend with public data on every lane: each lane is the plain prover)"""
    import czk_amd
    from czk_amd import polyvm
    ctx = polyvm.shared_stream_context(czk_amd)
    B = polyvm.GpuBackend(czk_amd, ctx, 2, polyvm.plonk_max_degree(64), lift=(1, 1))
    yield czk_amd, ctx, B
    ctx.close()


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])).cuda()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. czk_plonk_layout
# ---------------------------------------------------------------------------------------------------------------------------------------
def random_succ(W, seed):
    """a permutation of [0, W) made of cycles of 1 to 5 slots: fixed points (a variable used once) included"""
    rng = random.Random(seed)
    slots = list(range(W))
    rng.shuffle(slots)
    succ, at = [0] * W, 0
    while at < W:
        n = min(rng.randrange(1, 6) if at else 1, W - at)                      # the first slot drawn is a fixed point
        for j in range(n):
            succ[slots[at + j]] = slots[at + (j + 1) % n]
        at += n
    assert sorted(succ) == list(range(W)) and any(s == i for i, s in enumerate(succ))
    return np.array(succ, dtype=np.uint32)


_MODELS = {}


def layout_model(ctx, n_gates):
    """(w, the Montgomery limbs of w^i for i < W, succ): computed once per size and shared"""
    if n_gates not in _MODELS:
        W = 3 * n_gates
        w = unmont(ctx.mixed_domain_constants(W)["group_gen"])[0]
        assert pow(w, W, R_MOD) == 1 and pow(w, W // 3, R_MOD) != 1
        assert W % 2 or pow(w, W // 2, R_MOD) != 1
        if n_gates > 1:
            assert pow(w, 3, R_MOD) == omega_for(n_gates.bit_length() - 1)       # flat.rs:299: the gate domain is the cube of the wire domain
        powers, acc = [], 1
        for _ in range(W):
            powers.append(acc)
            acc = acc * w % R_MOD
        _MODELS[n_gates] = (w, mont(powers), random_succ(W, 0x5CC + n_gates))
    return _MODELS[n_gates]


def selector_model(n_gates, n_prods):
    return mont([0] * n_prods + [1] * (n_gates - n_prods))


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("n_gates", [1, 2, 8, 128, 1 << 15])
def test_plonk_layout_matches_the_big_integer_model(gpu, n_gates, mem):
    czk, ctx, _ = gpu
    import torch
    _, table, succ = layout_model(ctx, n_gates)
    W = 3 * n_gates
    want_w = table[succ]
    for n_prods in sorted({0, n_gates, n_gates // 3}):
        if mem == "host":
            w_evals, s_evals = ctx.plonk_layout(succ, n_gates, n_prods)
        else:
            d_succ = to_dev(succ)
            d_w = torch.full((W, 4), -1, dtype=torch.int64, device="cuda")
            d_s = torch.full((n_gates, 4), -1, dtype=torch.int64, device="cuda")
            ctx.plonk_layout(d_succ.data_ptr(), n_gates, n_prods, w_evals=d_w.data_ptr(), s_evals=d_s.data_ptr(), mem=czk.CZK_MEM_DEVICE)
            ctx.sync()
            w_evals, s_evals = d_w.cpu().numpy().view(np.uint64), d_s.cpu().numpy().view(np.uint64)
        assert w_evals.shape == (W, 4) and np.array_equal(w_evals, want_w), (n_gates, n_prods)
        assert np.array_equal(s_evals, selector_model(n_gates, n_prods)), (n_gates, n_prods)


def test_plonk_layout_error_codes(gpu):
    czk, ctx, _ = gpu
    ok = np.arange(6, dtype=np.uint32)
    cases = [
        (dict(succ=ok, n_gates=0, n_prods=0), ERR_SIZE, "power of two"),
        (dict(succ=np.arange(9, dtype=np.uint32), n_gates=3, n_prods=0), ERR_SIZE, "power of two"),
        (dict(succ=ok, n_gates=1 << 31, n_prods=0), ERR_SIZE, "32-bit slot indices"),
        (dict(succ=ok, n_gates=2, n_prods=3), ERR_SIZE, "more products than gates"),
        (dict(succ=np.array([0, 1, 2, 3, 4, 4], dtype=np.uint32), n_gates=2, n_prods=1), ERR_ARG, "named twice"),
        (dict(succ=np.array([0, 1, 2, 3, 4, 6], dtype=np.uint32), n_gates=2, n_prods=1), ERR_ARG, "beyond the 3 n_gates wire slots"),
    ]
    for kw, code, msg in cases:
        with pytest.raises(czk.CzkError, match=msg) as e:
            ctx.plonk_layout(**kw)
        assert e.value.code == code, kw
    with pytest.raises(czk.CzkError, match="mem must be") as e:
        ctx.plonk_layout(ok, 2, 1, mem=7)
    assert e.value.code == ERR_ARG
    w_evals, _ = ctx.plonk_layout(ok, 2, 1)                                      # the context still works
    assert w_evals.shape == (6, 4)


def test_plonk_layout_device_memory_marks_a_slot_out_of_range_with_zero(gpu):
    czk, ctx, _ = gpu
    import torch
    n_gates = 128
    _, table, succ = layout_model(ctx, n_gates)
    W = 3 * n_gates
    bad = succ.copy()
    bad[5], bad[300] = W, 0xFFFFFFFF
    d_succ = to_dev(bad)
    d_w = torch.full((W, 4), -1, dtype=torch.int64, device="cuda")
    d_s = torch.full((n_gates, 4), -1, dtype=torch.int64, device="cuda")
    ctx.plonk_layout(d_succ.data_ptr(), n_gates, 40, w_evals=d_w.data_ptr(), s_evals=d_s.data_ptr(), mem=czk.CZK_MEM_DEVICE)
    ctx.sync()
    want = table[np.where(bad < W, bad, 0)]
    want[[5, 300]] = 0                                                           # zero is no domain element: the mistake shows
    assert np.array_equal(d_w.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(d_s.cpu().numpy().view(np.uint64), selector_model(n_gates, 40))


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. czk_fr_gather
# ---------------------------------------------------------------------------------------------------------------------------------------
FILL = 0xA5A5A5A5A5A5A5A5


def gather_case(lanes, n, seed):
    """src of 37 valid elements per lane in a stride of 41, an index array with repeats and the last element, out in a stride of n + 3"""
    rng = np.random.default_rng(seed)
    src_len, src_stride, out_stride = 37, 41, n + 3
    src = rng.integers(0, 1 << 63, size=(lanes, src_stride, 4), dtype=np.uint64)
    index = rng.integers(0, src_len, size=n, dtype=np.uint32)
    index[0] = src_len - 1
    if n > 2:
        index[1] = index[2]
    out = np.full((lanes, out_stride, 4), FILL, dtype=np.uint64)
    want = out.copy()
    want[:, :n] = src[:, index]
    return src, src_len, index, out, want


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("lanes", [1, 3])
def test_fr_gather_matches_numpy_indexing(gpu, lanes, n, mem):
    czk, ctx, _ = gpu
    src, src_len, index, out, want = gather_case(lanes, n, 100 * lanes + n)
    if mem == "host":
        got = ctx.fr_gather(src, index, lanes=lanes, src_len=src_len, out=out)
        assert got is out
        dense = ctx.fr_gather(src, index, lanes=lanes, src_len=src_len)          # out_stride == n: the output is not uploaded first
        assert np.array_equal(dense, want[:, :n])
    else:
        d_src, d_index, d_out = to_dev(src), to_dev(index), to_dev(out)
        ctx.fr_gather(d_src.data_ptr(), d_index.data_ptr(), lanes=lanes, src_len=src_len, src_stride=src.shape[1], n=n, out=d_out.data_ptr(),
                      out_stride=out.shape[1], mem=czk.CZK_MEM_DEVICE)
        ctx.sync()
        got = d_out.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want)                                             # the padding limbs past n are as they were


def test_fr_gather_indices_out_of_range_and_empty_calls(gpu):
    czk, ctx, _ = gpu
    src, src_len, index, out, want = gather_case(3, 257, 9)
    bad = index.copy()
    bad[100], bad[256] = src_len, 0xFFFFFFFF                                     # src_len itself: inside the stride, outside the lane
    with pytest.raises(czk.CzkError, match="index beyond the source lane") as e:
        ctx.fr_gather(src, bad, lanes=3, src_len=src_len, out=out.copy())
    assert e.value.code == ERR_ARG
    d_src, d_index, d_out = to_dev(src), to_dev(bad), to_dev(out)
    ctx.fr_gather(d_src.data_ptr(), d_index.data_ptr(), lanes=3, src_len=src_len, src_stride=src.shape[1], n=257, out=d_out.data_ptr(),
                  out_stride=out.shape[1], mem=czk.CZK_MEM_DEVICE)
    ctx.sync()
    want[:, [100, 256]] = 0
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)             # zero there, the neighbours intact
    # empty calls: CZK_OK, nothing touched
    kept = out.copy()
    assert ctx.fr_gather(src, np.zeros(0, dtype=np.uint32), lanes=3, src_len=src_len, out=kept) is kept and np.array_equal(kept, out)
    assert ctx.fr_gather(np.zeros((0, 0, 4), dtype=np.uint64), index, lanes=0).shape == (0, 257, 4)
    d_keep = to_dev(out)
    for lanes, n in ((3, 0), (0, 257)):
        ctx.fr_gather(d_src.data_ptr(), d_index.data_ptr(), lanes=lanes, src_len=src_len, src_stride=src.shape[1], n=n, out=d_keep.data_ptr(),
                      out_stride=out.shape[1], mem=czk.CZK_MEM_DEVICE)
    ctx.sync()
    assert np.array_equal(d_keep.cpu().numpy().view(np.uint64), out)
    with pytest.raises(czk.CzkError, match="stride is shorter") as e:
        ctx.fr_gather(d_src.data_ptr(), d_index.data_ptr(), lanes=3, src_len=src_len, src_stride=src_len - 1, n=257, out=d_keep.data_ptr(),
                      out_stride=out.shape[1], mem=czk.CZK_MEM_DEVICE)
    assert e.value.code == ERR_SIZE


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. layout / prover_inputs, 4. the round trip and the verifier
# ---------------------------------------------------------------------------------------------------------------------------------------
def slot_one_circuit():
    """4 gates whose single public variable first occurs at slot 1: the case tests/polyiop_real.py::plonk_verify models"""
    from czk_amd import plonk
    c = plonk.Circuit()
    a, x = c.new_var(), c.new_pub_var("x")
    g = c.new_prod(a, x)
    h = c.new_sum(g, a)
    c.new_prod(h, h)
    c.pad_to_power_of_2()
    return c


CIRCUITS = {"hand_made": hand_made, "random_64": lambda: random_circuit(64, 0x64), "slot_one": slot_one_circuit}
_PROVED = {}


def proved(gpu, name):
    """circuit -> layout -> prover_inputs -> plonk_prove, once per circuit and shared (nothing in it is changed by a test: they work on copies)"""
    if name not in _PROVED:
        from czk_amd import plonk, polyvm
        _, _, B = gpu
        c = CIRCUITS[name]()
        rng = random.Random(len(name))
        vals = c.evaluate([rng.randrange(R_MOD) for _ in range(c.n_vars - c.n_gates())])
        lay = plonk.layout(B, c)
        inp = plonk.prover_inputs(B, lay, vals)
        out = polyvm.plonk_prove(B, inp)
        public = {nm: vals[v] for v, nm in c.pub_vars.items()}
        _PROVED[name] = dict(circuit=c, vals=vals, lay=lay, vk=plonk.verifier_key(lay), inp=inp, out=out, public=public)
    return _PROVED[name]


@pytest.mark.parametrize("name", ["hand_made", "random_64"])
def test_layout_and_prover_inputs_evaluate_back_to_the_model(gpu, name):
    from czk_amd import plonk, polyvm
    czk, ctx, B = gpu
    pr = proved(gpu, name)
    c, lay, vals = pr["circuit"], pr["lay"], pr["vals"]
    G = c.n_gates()
    W = 3 * G
    var_layout, succ, public, _ = naive_wiring(c)
    w = unmont(ctx.mixed_domain_constants(W)["group_gen"])[0]
    assert lay["n_gates"] == G and lay["public_indices"] == public
    assert lay["public_points"] == [pow(w, public[nm], R_MOD) for nm in sorted(public)]
    assert lay["var_layout"].cpu().numpy().view(np.uint32).tolist() == var_layout
    assert B.lanes_of(lay["s"]) == 1 and B.length(lay["s"]) == G and B.length(lay["w"]) == W
    assert unmont(B.download(B.ntt(lay["s"], G, polyvm.FFT))[0]) == [0] * len(c.prods) + [1] * len(c.sums)
    assert unmont(B.download(B.ntt(lay["w"], W, polyvm.FFT))[0]) == [pow(w, s, R_MOD) for s in succ]
    # the plain assignment sits on every lane ...
    p_evals = B.download(B.ntt(pr["inp"]["p"], W, polyvm.FFT))
    want = [vals[v] for v in var_layout]
    assert p_evals.shape == (2, W, 4) and unmont(p_evals[0]) == want and unmont(p_evals[1]) == want
    assert pr["inp"]["s"] is lay["s"] and pr["inp"]["w"] is lay["w"] and pr["inp"]["public_points"] == lay["public_points"]
    # ... Montgomery limbs are taken as they are, and share lanes are gathered lane by lane
    as_limbs = plonk.prover_inputs(B, lay, mont(vals))
    assert np.array_equal(B.download(as_limbs["p"]), B.download(pr["inp"]["p"]))
    rng = random.Random(77)
    other = [rng.randrange(R_MOD) for _ in vals]
    shares = B.upload(np.stack([mont(vals), mont(other)]))
    p_evals = B.download(B.ntt(plonk.prover_inputs(B, lay, shares)["p"], W, polyvm.FFT))
    assert unmont(p_evals[0]) == want and unmont(p_evals[1]) == [other[v] for v in var_layout]
    with pytest.raises(ValueError):
        plonk.prover_inputs(B, lay, vals[:-1])
    # the key is host data
    vk = pr["vk"]
    assert set(vk) == {"n_gates", "public_indices", "s_cmt", "w_cmt"} and all(isinstance(a, np.ndarray) for k in ("s_cmt", "w_cmt") for a in vk[k])


def test_layout_of_one_gate(gpu):
    """czk_ntt_fr_mixed accepts the wire domain of 3 points, so a circuit of one gate is laid out; plonk_prove cannot take it (the witness of the
    selector's opening has n_gates - 1 = 0 coefficients), which prover_inputs says."""
    from czk_amd import plonk, polyvm
    czk, ctx, B = gpu
    c = plonk.Circuit.squaring_circuit(1)
    lay = plonk.layout(B, c)
    w = unmont(ctx.mixed_domain_constants(3)["group_gen"])[0]
    assert lay["n_gates"] == 1 and lay["public_indices"] == {"out": 2} and lay["public_points"] == [pow(w, 2, R_MOD)]
    assert unmont(B.download(lay["s"])[0]) == [0]
    assert unmont(B.download(B.ntt(lay["w"], 3, polyvm.FFT))[0]) == [pow(w, s, R_MOD) for s in (1, 0, 2)]
    with pytest.raises(ValueError, match="at least two gates"):
        plonk.prover_inputs(B, lay, c.evaluate([5]))


def test_layout_timings(gpu):
    from czk_amd import plonk
    _, _, B = gpu
    t, t2 = {}, {}
    lay = plonk.layout(B, hand_made(), timings=t)
    plonk.prover_inputs(B, lay, hand_made().evaluate([3, 4]), timings=t2)
    assert list(t) == ["wiring", "kernel", "transforms", "commitments"] and list(t2) == ["gather", "transform"]
    assert all(v >= 0 for v in list(t.values()) + list(t2.values()))


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_round_trip_verifies(gpu, name):
    from czk_amd import kzg, plonk, polyvm
    _, _, B = gpu
    pr = proved(gpu, name)
    out, vk = pr["out"], pr["vk"]
    assert plonk.verify(B, vk, pr["public"], out, rng=random.Random(1)) is True
    # the openings check_openings reports are the ones the proof holds
    held = [k for k, o in out.items() if isinstance(o, dict) and "point" in o]
    seen = dict(out, s_cmt=vk["s_cmt"], w_cmt=vk["w_cmt"])
    seen["gates_s_open"], seen["w_x_open"] = dict(out["gates_s_open"], of="s"), dict(out["w_x_open"], of="w")
    report = kzg.check_openings(B, seen, rng=random.Random(2), details=True)
    assert len(held) == 16 and sorted(report) == sorted(held) and all(report.values())
    if name == "slot_one":
        import polyiop_real
        c, vals = pr["circuit"], pr["vals"]
        assert pr["lay"]["public_indices"] == {"x": 1}
        e = [vals[v] for v in naive_wiring(c)[0]]
        polyiop_real.plonk_verify(polyvm, out, e, B.root_of_unity(3 * c.n_gates()), c.n_gates())


def test_verify_rejects_one_change_at_a_time(gpu, monkeypatch):
    from czk_amd import plonk, polyvm
    _, _, B = gpu
    pr = proved(gpu, "hand_made")
    c, vals, lay, vk, out, public = (pr[k] for k in ("circuit", "vals", "lay", "vk", "out", "public"))
    rng = random.Random(3)
    assert plonk.verify(B, vk, public, out, rng=rng) is True
    # a wrong public value
    assert plonk.verify(B, vk, dict(public, result=public["result"] + 1), out, rng=rng) is False
    # one opened value changed by one
    for label in ("gates_p_open", "w_x_open"):
        forged = copy.deepcopy(out)
        v = unmont(forged[label]["value"])
        forged[label]["value"] = mont([x + 1 for x in v])
        assert plonk.verify(B, vk, public, forged, rng=rng) is False, label
    # s_cmt and w_cmt exchanged in the key
    assert plonk.verify(B, dict(vk, s_cmt=vk["w_cmt"], w_cmt=vk["s_cmt"]), public, out, rng=rng) is False
    # the proof's own s_cmt / w_cmt are never read
    assert plonk.verify(B, vk, public, dict(out, s_cmt=vk["w_cmt"], w_cmt=vk["s_cmt"]), rng=rng) is True
    # a proof under a layout with two succ entries exchanged (two variables' cycles are joined), checked under the original key
    real_wiring = plonk.wiring

    def joined(circuit):
        wi = real_wiring(circuit)
        var_layout, succ = wi["var_layout"], wi["succ"]
        i = 0
        j = next(k for k in range(len(succ)) if var_layout[k] != var_layout[i] and vals[var_layout[k]] != vals[var_layout[i]])
        succ[i], succ[j] = succ[j], succ[i]
        return wi
    monkeypatch.setattr(plonk, "wiring", joined)
    lay2 = plonk.layout(B, c)
    monkeypatch.undo()
    assert not np.array_equal(B.download(lay2["w"]), B.download(lay["w"]))
    out2 = polyvm.plonk_prove(B, plonk.prover_inputs(B, lay2, vals))
    assert plonk.verify(B, vk, public, out2, rng=rng) is False
    # an assignment with one gate output off by one (on all its slots: only the gate identity can tell)
    a, b, o = c.prods.tolist()[0]
    assert o not in c.pub_vars
    off = list(vals)
    off[o] = (off[o] + 1) % R_MOD
    out3 = polyvm.plonk_prove(B, plonk.prover_inputs(B, lay, off))
    assert plonk.verify(B, vk, public, out3, rng=rng) is False
    with pytest.raises(plonk._Reject, match="gates"):
        plonk._decide(B, vk, public, out3, rng)
    # one slot of a shared variable changed through a hand-edited p evaluation vector: the copies disagree and the total product is not 1
    var_layout = naive_wiring(c)[0]
    slot = next(i for i, v in enumerate(var_layout) if var_layout.count(v) == 5)
    evals = [vals[v] for v in var_layout]
    evals[slot] = (evals[slot] + 1) % R_MOD
    inp4 = dict(pr["inp"], p=B.ntt(polyvm.shared_copy(B, B.upload(mont(evals))), 3 * c.n_gates(), polyvm.IFFT))
    out4 = polyvm.plonk_prove(B, inp4)
    assert unmont(out4["t_wk_open"]["value"])[0] != 1
    assert plonk.verify(B, vk, public, out4, rng=rng) is False


def test_verify_wants_exactly_the_keys_public_names(gpu):
    from czk_amd import plonk
    _, _, B = gpu
    pr = proved(gpu, "hand_made")
    public = pr["public"]
    with pytest.raises(ValueError, match="public"):
        plonk.verify(B, pr["vk"], {"five": public["five"]}, pr["out"])
    with pytest.raises(ValueError, match="public"):
        plonk.verify(B, pr["vk"], dict(public, extra=1), pr["out"])
