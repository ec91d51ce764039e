"""The guard-band helper (tests/guarded.py) can fail: every planted violation is detected and named, a write inside the footprint is not
flagged, and the grid caps the helper mirrors are the ones the sources launch with.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import guarded
from guarded import FrozenInput, GuardedOutput, Guards, grid_tail_sizes

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "collaborative-zksnark_amd", "csrc")


def _g(lanes=3, length=7, stride=12, **kw):
    return GuardedOutput(lanes, length, stride, **kw)


def test_layout_pads_and_pointer():
    g = _g()
    assert g.pad * 8 >= 4096 and g.pad >= 128 * 4
    assert g.buf.numel() == 2 * g.pad + 3 * 12 * 4
    assert g.ptr == g.buf.data_ptr() + 8 * g.pad and g.ptr % 16 == 0
    assert g.lane_ptr(2, 5) == g.ptr + (2 * 12 + 5) * 32
    b = GuardedOutput(1, 129, words=1, dtype=torch.uint8)
    assert b.pad >= 4096 and b.ptr == b.buf.data_ptr() + b.pad
    # the sentinel depends on the position, is never a zero / one, and every int64 word is above the top limb of the modulus
    assert len(set(g.buf.tolist())) == g.buf.numel()
    assert int(b.buf.min()) >= 2 and len(set(b.buf[:200].tolist())) > 100
    assert int(g.buf.min()) >= 0x7 << 60


def test_clean_buffer_and_writes_inside_the_footprint_pass():
    g = _g()
    assert g.untouched()
    foot = g.check()
    assert foot.shape == (3, 7, 4) and foot.dtype == np.uint64
    v = g.view()
    v[:, :7] = 5                       # the whole footprint, every lane
    v[1, 6, 3] = 0                     # its last word
    foot = g.check()
    assert (foot[0] == 5).all() and foot[1, 6, 3] == 0
    assert not g.untouched()
    # a byte output
    b = GuardedOutput(1, 129, words=1, dtype=torch.uint8)
    b.view()[0, :, 0] = 1
    assert b.check().dtype == np.uint8 and (b.check() == 1).all()
    # zero-sized footprints
    assert GuardedOutput(3, 0, 0).check().shape == (3, 0, 4)
    assert GuardedOutput(2, 0, 5).check().shape == (2, 0, 4)


@pytest.mark.parametrize("where,needle", [
    ("before", "front pad"), ("after_last_lane", "back pad"), ("stride_padding", "lane 1 element 7"), ("stride_padding_last_lane", "lane 2 element 11"),
    ("front_pad_first_word", "front pad, word 0"), ("back_pad_last_word", "back pad, word"), ("zero_into_padding", "lane 0 element 9")])
def test_planted_violations_are_detected_and_named(where, needle):
    g = _g()
    p = g.pad
    if where == "before":
        g.buf[p - 1] = 0                           # the last word of the element before lane 0
        needle2 = "1 element(s) before lane 0"
    elif where == "after_last_lane":
        g.buf[p + g.inner] = 0                     # one element after the last lane's stride
        needle2 = "1 element(s) after the end of lane 2"
    elif where == "stride_padding":
        g.view()[1, 7, 0] = 0                      # one element after lane 1's footprint
        needle2 = "ends at element 7"
    elif where == "stride_padding_last_lane":
        g.view()[2, 11, 3] = 0
        needle2 = "word 3"
    elif where == "front_pad_first_word":
        g.buf[0] = 0
        needle2 = "before lane 0"
    elif where == "back_pad_last_word":
        g.buf[-1] = 0
        needle2 = f"word {p - 1}:"
    else:
        g.view()[0, 9] = 0                         # a kernel that zero-fills to the stride
        needle2 = "4 word(s) changed"
    with pytest.raises(AssertionError) as e:
        g.check()
    assert needle in str(e.value) and needle2 in str(e.value), str(e.value)


def test_copying_a_neighbour_or_the_sentinel_one_slot_on_is_detected():
    g = _g()
    v = g.view()
    v[0, 7] = v[0, 8].clone()          # a neighbour's sentinel is not this slot's
    with pytest.raises(AssertionError, match="lane 0 element 7"):
        g.check()
    b = GuardedOutput(1, 10, words=1, dtype=torch.uint8, name="flags")
    b.buf[b.pad + 10] = 1
    with pytest.raises(AssertionError, match="flags: .*back pad, word 0"):
        b.check()


def test_frozen_input_detects_a_write():
    t = torch.arange(40, dtype=torch.int64).reshape(10, 4)
    f = FrozenInput(t, "coeffs")
    f.check()
    t[6, 2] += 1
    with pytest.raises(AssertionError, match="coeffs: input modified by the call, first at element 6 word 2"):
        f.check()
    G = Guards()
    a = G.freeze(np.arange(8, dtype=np.uint64).reshape(2, 4), "a")
    o = G.out(1, 2)
    o.view()[0] = a.t.view(1, 2, 4)[0]
    assert np.array_equal(G.check()[0][0], np.arange(8, dtype=np.uint64).reshape(2, 4))
    a.t[1, 3] = -1
    with pytest.raises(AssertionError, match="a: input modified"):
        G.check()


def test_grid_tail_sizes():
    assert grid_tail_sizes(8, 256) == [1, 255, 256, 257, 524287, 524291]
    assert grid_tail_sizes(16, 256) == [1, 255, 256, 257, 1048575, 1048579]
    assert grid_tail_sizes(16, 304)[-1] == 16 * 304 * 256 + 3
    assert guarded.per_cu_blocks("k_lincomb") == 16 and guarded.per_cu_blocks("k_gsz_open") == 8 and guarded.per_cu_blocks("k_vec_scale_dev") == 8


def test_grid_caps_match_the_sources():
    """Every `cap = (size_t)ctx->num_cu * K` of the files the table names, in order, with its line; each sits on a 256-thread block count."""
    for name, want in guarded.GRID_CAPS.items():
        lines = open(os.path.join(CSRC, name)).read().splitlines()
        got = []
        for no, ln in enumerate(lines, 1):
            m = re.search(r"\bcap = \(size_t\)ctx->num_cu \* (\d+)", ln)
            if m:
                got.append((no, int(m.group(1))))
                assert "+ 255) / 256" in ln or "+ 255) / 256" in lines[no - 2], (name, no)
        assert got == [(no, k) for no, k, _ in want], (name, got)
        text = "\n".join(lines)
        for _, _, kernels in want:
            for k in kernels:
                assert re.search(rf"__global__[^\n]*\b{k}\(", text), (name, k)
                assert re.search(rf"hipLaunchKernelGGL\({k}, dim3\([^\n]*dim3\({guarded.BLOCK}\)", text), (name, k)
    # no other source file caps a grid by the CU count this way
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name not in guarded.GRID_CAPS:
            assert not re.search(r"\bcap = \(size_t\)ctx->num_cu \*", open(os.path.join(CSRC, name)).read()), name
    m = re.search(r"inline dim3 grid_for\(size_t n, unsigned per_block = (\d+)\)", open(os.path.join(CSRC, "call.h")).read())
    assert m and int(m.group(1)) == guarded.GRID_FOR_DEFAULT_BLOCK
