"""Guard bands for calls that write through raw pointers (TEST INFRASTRUCTURE ONLY).

A parity test sees WHAT a call computes; this module sees WHERE it writes.  `GuardedOutput` is one torch buffer

    | pad | lane 0: length ... stride | lane 1 | ... | lane L-1: length ... stride | pad |

filled with a position-dependent sentinel (a kernel cannot reproduce it by writing zeros or by copying a neighbour).  The test hands
`ptr` (the first element of lane 0) to the call and `check()` then asserts that every word outside the declared footprint -- `length`
elements at the start of each lane -- still holds its sentinel, naming the first offending lane and element.  `FrozenInput` keeps a
clone of an input and asserts the call left it bit-identical.  Both work on CPU and GPU tensors, int64 words (Fr / Fq limbs) or bytes
(infinity flags, status bytes, serialized points).

`GRID_CAPS` mirrors the block caps of the grid-stride launches; `grid_tail_sizes` turns a cap into the sizes around the first and the
second trip of such a loop.  tests/test_guarded_cpu.py parses the sources and fails when a cap changes without this table.
"""
import numpy as np
import torch

PAD_BYTES = 4096          # at least 128 Fr elements before the first lane and after the last
BLOCK = 256               # threads per block of every capped grid-stride launch below

# file (under collaborative-zksnark_amd/csrc) -> the caps `cap = (size_t)ctx->num_cu * K` in source order: (line, K, kernels launched under it)
GRID_CAPS = {
    "share.hip": [(52, 8, ("k_lanes_sum", "k_spdz_dx", "k_gsz_open"))],
    "fr_vec.hip": [(78, 8, ("k_vec_op", "k_vec_scale", "k_vec_scale_dev", "k_beaver", "k_spdz_open", "k_repr", "k_sub_scale", "k_spdz_open_combine"))],
    "poly.hip": [(381, 16, ("k_r1cs_matvec",)), (562, 16, ("k_lincomb",))],
    "lanes.hip": [(234, 16, ("k_copy_3d",))],
    "ntt_mixed.hip": [(150, 16, ("k_mixed_split", "k_mixed_combine"))],
}
# call.h: grid_for(n, per_block = 128) -- one thread per item, no cap, no loop (the group-side kernels)
GRID_FOR_DEFAULT_BLOCK = 128


def per_cu_blocks(kernel: str) -> int:
    for caps in GRID_CAPS.values():
        for _, k, kernels in caps:
            if kernel in kernels:
                return k
    raise KeyError(kernel)


def device_cus() -> int:
    return torch.cuda.get_device_properties(0).multi_processor_count


def grid_threads(per_cu: int, cus: int | None = None) -> int:
    """T: elements one trip of a loop capped at `per_cu` blocks per CU covers."""
    return per_cu * (device_cus() if cus is None else cus) * BLOCK


def grid_tail_sizes(per_cu: int, cus: int | None = None) -> list:
    """One element, around one block, and either side of the size where the loop starts its second trip."""
    t = grid_threads(per_cu, cus)
    return [1, 255, 256, 257, t - 1, t + 3]


def _sentinel(total: int, dtype, device):
    idx = torch.arange(total, dtype=torch.int64, device=device)
    if dtype == torch.uint8:
        return (2 + (idx * 167 + 13) % 251).to(torch.uint8)          # never 0 or 1: a flag byte cannot pass for a sentinel
    s = (idx + 0x1234567) * -7046029254386353131                     # 0x9E3779B97F4A7C15: wraps in int64
    s = s ^ (s >> 29)
    return s | (0x7 << 60)                                           # top limb of an Fr: above the modulus


class GuardedOutput:
    """`lanes` x `length` elements of `words` words each at lane stride `stride` (elements, default `length`) inside sentinel pads."""

    def __init__(self, lanes: int, length: int, stride: int | None = None, words: int = 4, dtype=torch.int64, device="cpu", name: str = "out"):
        stride = length if stride is None else stride
        assert stride >= length >= 0 and lanes >= 0 and words >= 1
        self.lanes, self.length, self.stride, self.words, self.name = lanes, length, stride, words, name
        item = torch.empty((), dtype=dtype).element_size()
        self.pad = max(PAD_BYTES // item, 128 * words)                # in words; a multiple of 16 bytes, so `ptr` keeps the allocation's alignment
        assert self.pad * item % 16 == 0
        self.inner = lanes * stride * words
        self.buf = _sentinel(2 * self.pad + self.inner, dtype, device)
        self.item = item

    @property
    def ptr(self) -> int:
        return self.buf.data_ptr() + self.pad * self.item

    def lane_ptr(self, lane: int, elem: int = 0) -> int:
        return self.ptr + (lane * self.stride + elem) * self.words * self.item

    def view(self):
        """The interior as a (lanes, stride, words) tensor sharing the buffer (a test plants its own writes through it)."""
        return self.buf[self.pad:self.pad + self.inner].view(self.lanes, self.stride, self.words)

    def _where(self, w: int) -> str:
        ew = self.words
        if w < self.pad:
            back = self.pad - w
            return f"front pad, word {w}: {-(-back // ew)} element(s) before lane 0 element 0"
        if w >= self.pad + self.inner:
            off = w - self.pad - self.inner
            return f"back pad, word {off}: {off // ew + 1} element(s) after the end of lane {max(self.lanes - 1, 0)}'s stride"
        lane, r = divmod(w - self.pad, self.stride * ew)
        return f"lane {lane} element {r // ew} word {r % ew} (stride padding: the lane's footprint ends at element {self.length})"

    def check(self):
        """Asserts that nothing outside the footprint changed; returns the footprint as numpy (lanes, length, words) uint64 (uint8 for bytes)."""
        want = _sentinel(self.buf.numel(), self.buf.dtype, self.buf.device)
        diff = self.buf != want
        if self.inner:
            diff[self.pad:self.pad + self.inner].view(self.lanes, self.stride * self.words)[:, :self.length * self.words] = False
        if bool(diff.any()):
            w = int(torch.nonzero(diff)[0])
            raise AssertionError(f"{self.name}: write outside the footprint of {self.lanes} x {self.length} elements (stride {self.stride}) at "
                                 f"{self._where(w)}; {int(diff.sum())} word(s) changed in all")
        foot = self.view()[:, :self.length].cpu().numpy()
        return foot.view(np.uint64) if self.buf.dtype == torch.int64 else foot

    def untouched(self) -> bool:
        """True when the footprint itself still holds its sentinel (a call that must write nothing)."""
        want = _sentinel(self.buf.numel(), self.buf.dtype, self.buf.device)
        return bool(torch.equal(self.buf, want))


class FrozenInput:
    """An input tensor with a clone taken before the call; check() asserts the call did not modify it."""

    def __init__(self, t, name: str = "input"):
        self.t, self.name = t, name
        self.keep = t.clone()

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()

    def check(self):
        if not torch.equal(self.t, self.keep):
            flat = (self.t != self.keep).reshape(-1)
            w = int(torch.nonzero(flat)[0])
            last = self.t.shape[-1] if self.t.dim() > 1 else 1
            raise AssertionError(f"{self.name}: input modified by the call, first at element {w // last} word {w % last}; {int(flat.sum())} word(s) changed")


class Guards:
    """The guarded outputs and frozen inputs of one call: check() runs every check and returns the footprints in creation order."""

    def __init__(self, device="cpu"):
        self.device, self.outs, self.ins = device, [], []

    def out(self, lanes, length, stride=None, words=4, dtype=torch.int64, name="out") -> GuardedOutput:
        g = GuardedOutput(lanes, length, stride, words, dtype, self.device, name)
        self.outs.append(g)
        return g

    def bytes(self, n, name="bytes") -> GuardedOutput:
        return self.out(1, n, words=1, dtype=torch.uint8, name=name)

    def freeze(self, array, name="input") -> FrozenInput:
        """numpy (uint64 / uint32 / uint8) or torch tensor -> a frozen tensor on the device."""
        if isinstance(array, np.ndarray):
            a = np.ascontiguousarray(array)
            a = a.view(np.int64) if a.dtype == np.uint64 else (a.view(np.int32) if a.dtype == np.uint32 else a)
            array = torch.from_numpy(a.copy()).to(self.device)
        f = FrozenInput(array, name)
        self.ins.append(f)
        return f

    def check(self):
        for f in self.ins:
            f.check()
        return [g.check() for g in self.outs]
