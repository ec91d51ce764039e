"""czk_amd.plonk without a GPU: Circuit (PlonkCircuit, mpc-plonk/src/relations/structured.rs), wiring (the index arrays of CircuitLayout::from_circuit,
relations/flat.rs:62-80 and :126-135) against a literal restatement of the reference's loops over a dict of lists, the claim behind
polyvm.plonk_prove's public quotient for any number of public wires in big integers, and the operations that path emits on the shape backend."""
import random

import numpy as np
import pytest

import czk_amd  # noqa: F401
from czk_amd import plonk, polyvm
from czk_amd.polyvm import R_MOD


def naive_wiring(c):
    """flat.rs:62-80, :126-135 as written: var_layout, vars_to_indices as a dict of lists, and the (i + 1) % len loop"""
    var_layout = [int(v) for gate in list(c.prods) + list(c.sums) for v in gate]
    vars_to_indices = {v: [] for v in range(c.n_vars)}
    for i, v in enumerate(var_layout):
        vars_to_indices[v].append(i)
    succ = [None] * len(var_layout)
    for indices in vars_to_indices.values():
        for i in range(len(indices)):
            succ[indices[i]] = indices[(i + 1) % len(indices)]
    public = {name: vars_to_indices[v][0] for v, name in c.pub_vars.items() if vars_to_indices[v]}
    return var_layout, succ, public, vars_to_indices


def hand_made():
    """8 gates: `once` sits in one slot, `five` in five, two public variables (one an input, one a gate output)"""
    c = plonk.Circuit()
    five, once = c.new_pub_var("five"), c.new_var()
    a = c.new_prod(five, five)
    b = c.new_sum(five, once)
    d = c.new_prod(a, b)
    e = c.new_sum(d, five)
    f = c.new_prod(e, five)
    c.publicize_var(f, "result")
    c.pad_to_power_of_2()
    return c


def random_circuit(n_gates, seed):
    """products and sums mixed over inputs drawn from everything made so far; two public variables"""
    rng = random.Random(seed)
    c = plonk.Circuit()
    c.new_pub_var("in")
    c.new_var()
    for _ in range(n_gates):
        a, b = rng.randrange(c.n_vars), rng.randrange(c.n_vars)
        (c.new_prod if rng.random() < 0.5 else c.new_sum)(a, b)
    c.publicize_var(c.n_vars - 1, "out")
    return c


CIRCUITS = {"squaring_1": lambda: plonk.Circuit.squaring_circuit(1), "squaring_3": lambda: plonk.Circuit.squaring_circuit(3),
            "squaring_5": lambda: plonk.Circuit.squaring_circuit(5), "hand_made": hand_made, "random_64": lambda: random_circuit(64, 0x64)}


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_wiring_equals_the_reference_loops(name):
    c = CIRCUITS[name]()
    got = plonk.wiring(c)
    var_layout, succ, public, vars_to_indices = naive_wiring(c)
    assert got["var_layout"].dtype == np.uint32 and got["succ"].dtype == np.uint32
    assert got["var_layout"].tolist() == var_layout
    assert got["succ"].tolist() == succ
    assert got["public_indices"] == public and len(public) == len(c.pub_vars)
    # a permutation whose cycles are exactly the slot sets of the variables
    W = 3 * c.n_gates()
    assert sorted(got["succ"].tolist()) == list(range(W))
    seen, cycles = set(), []
    for start in range(W):
        if start not in seen:
            cyc, i = [], start
            while i not in seen:
                seen.add(i)
                cyc.append(i)
                i = int(got["succ"][i])
            cycles.append(sorted(cyc))
    assert sorted(cycles) == sorted(v for v in vars_to_indices.values() if v)


def test_hand_made_circuit_has_the_cases_it_is_for():
    c = hand_made()
    _, succ, public, vars_to_indices = naive_wiring(c)
    assert c.n_gates() == 8 and sorted(len(v) for v in vars_to_indices.values())[-1] == 5 and len(vars_to_indices[1]) == 1
    assert succ[vars_to_indices[1][0]] == vars_to_indices[1][0]                  # used once: a fixed point
    assert set(public) == {"five", "result"}


@pytest.mark.parametrize("steps,gates", [(1, 1), (3, 4), (5, 8), (8, 8)])
def test_squaring_circuit_and_the_padding_rule(steps, gates):
    c = plonk.Circuit.squaring_circuit(steps)
    assert c.n_gates() == gates and c.prods.shape == (steps, 3) and c.sums.shape == (gates - steps, 3)
    assert c.prods.tolist() == [[i, i, i + 1] for i in range(steps)]
    # pad_to_power_of_2: each padding gate is a sum of the LAST variable with itself, so the pads chain
    assert c.sums.tolist() == [[steps + j, steps + j, steps + j + 1] for j in range(gates - steps)]
    assert c.pub_vars == {steps: "out"} and c.n_vars == gates + 1
    assert c.prods.dtype == np.uint32 and c.sums.dtype == np.uint32


def test_publicize_twice_is_an_error():
    c = plonk.Circuit()
    v = c.new_pub_var("a")
    with pytest.raises(ValueError, match="already public"):
        c.publicize_var(v, "b")
    with pytest.raises(ValueError, match="taken"):
        c.publicize_var(c.new_var(), "a")
    with pytest.raises(ValueError):
        plonk.Circuit().pad_to_power_of_2()


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_evaluate_satisfies_every_gate(name):
    c = CIRCUITS[name]()
    rng = random.Random(5)
    n_free = c.n_vars - c.n_gates()
    vals = c.evaluate([rng.randrange(R_MOD) for _ in range(n_free)])
    assert len(vals) == c.n_vars and all(0 <= v < R_MOD for v in vals)
    assert all(vals[a] * vals[b] % R_MOD == vals[o] for a, b, o in c.prods.tolist())
    assert all((vals[a] + vals[b]) % R_MOD == vals[o] for a, b, o in c.sums.tolist())
    with pytest.raises(ValueError):
        c.evaluate([1] * (n_free + 1))


def test_wiring_refuses_what_the_reference_fails_on_later():
    c = plonk.Circuit()
    a = c.new_var()
    c.new_pub_var("unused")
    c.new_prod(a, a)
    with pytest.raises(ValueError, match="occurs in no gate"):
        plonk.wiring(c)
    c = plonk.Circuit.squaring_circuit(2)
    c.new_sum(0, 0)                                                              # 3 gates
    with pytest.raises(ValueError, match="power of two"):
        plonk.wiring(c)
    with pytest.raises(ValueError, match="power of two"):
        plonk.wiring(plonk.Circuit())


# ---- the public quotient for k public wires (polyvm.plonk_prove): successive division by linear factors --------------------------------
def div_linear(p, x):
    """p / (X - x): (quotient, remainder), coefficients low degree first"""
    q, acc = [0] * (len(p) - 1), 0
    for i in range(len(p) - 1, 0, -1):
        acc = (p[i] + acc * x) % R_MOD
        q[i - 1] = acc
    return q, (p[0] + acc * x) % R_MOD


def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % R_MOD
    return out


def long_division(p, z):
    """schoolbook p = q z + r for a monic z"""
    r, q = list(p), [0] * (len(p) - len(z) + 1)
    for i in range(len(q) - 1, -1, -1):
        q[i] = r[i + len(z) - 1]
        for j, zj in enumerate(z):
            r[i + j] = (r[i + j] - q[i] * zj) % R_MOD
    return q, r[:len(z) - 1]


def test_successive_linear_division_is_the_quotient_by_the_product():
    rng = random.Random(11)
    p = [rng.randrange(R_MOD) for _ in range(12)]                                # degree 11
    xs = [rng.randrange(R_MOD) for _ in range(3)]
    z = [1]
    for x in xs:
        z = poly_mul(z, [-x % R_MOD, 1])
    q = p
    for x in xs:
        q, _ = div_linear(q, x)
    want, rem = long_division(p, z)
    assert q == want and len(q) == 9
    assert [(a - b) % R_MOD for a, b in zip(p, rem + [0] * 9)] == poly_mul(want, z)
    # v = the interpolation of p through the three points has degree < 3 and p - v vanishes there: the same quotient, remainder zero
    ev = lambda f, x: sum(c * pow(x, i, R_MOD) for i, c in enumerate(f)) % R_MOD   # noqa: E731
    v = [0, 0, 0]
    for i, xi in enumerate(xs):
        num, den = [1], 1
        for j, xj in enumerate(xs):
            if j != i:
                num, den = poly_mul(num, [-xj % R_MOD, 1]), den * (xi - xj) % R_MOD
        k = ev(p, xi) * pow(den, -1, R_MOD) % R_MOD
        v = [(a + k * b) % R_MOD for a, b in zip(v, num)]
    assert v == rem                                                              # the remainder modulo z IS that interpolation
    p_minus_v = [(a - b) % R_MOD for a, b in zip(p, v + [0] * 9)]
    q2 = p_minus_v
    for x in xs:
        q2, r = div_linear(q2, x)
        assert r == 0
    assert q2 == q and long_division(p_minus_v, z) == (q, [0, 0, 0])


def test_plonk_prove_emits_one_quotient_per_public_point():
    from shape_backend import ShapeBackend
    logs = []
    for points in (None, [5], [5, 6, 7]):
        B = ShapeBackend(3)
        inp = polyvm.plonk_inputs(B, 16)
        if points is not None:
            inp["public_points"] = points
        polyvm.plonk_prove(B, inp)
        logs.append(B.log)
    W = 48
    assert logs[0] == logs[1]                                                    # the default is one public point
    assert logs[0][:3] == [("msm", W, 3), ("div_linear", W, 3), ("msm", W - 1, 3)]
    assert logs[2][:5] == [("msm", W, 3), ("div_linear", W, 3), ("div_linear", W - 1, 3), ("div_linear", W - 2, 3), ("msm", W - 3, 3)]
    # otherwise identical, but for the lengths of the public quotient and of its opening witness
    rest0, rest2 = logs[0][3:], logs[2][5:]
    assert len(rest0) == len(rest2)
    diff = [(a, b) for a, b in zip(rest0, rest2) if a != b]
    assert diff == [(("div_linear", W - 1, 3), ("div_linear", W - 3, 3)), (("msm", W - 2, 3), ("msm", W - 4, 3))]
    # nothing the three-point proof commits is longer than what plonk_commit_sizes prepares
    assert max(e[1] for e in logs[2] if e[0] == "msm") <= max(polyvm.plonk_commit_sizes(16))
