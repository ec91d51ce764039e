"""ctypes binding of libczk_hip.so (include/czk.h).  Host arrays are numpy uint64; device arrays are raw
pointers (ints) -- e.g. `tensor.data_ptr()` of a torch int64/uint64 CUDA tensor."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.environ.get("CZK_LIB_PATH") or os.path.join(_HERE, "libczk_hip.so")   # CZK_LIB_PATH: A/B builds of the library (tools/)
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "czk.h")

CZK_FFT, CZK_IFFT, CZK_COSET_FFT, CZK_COSET_IFFT = 0, 1, 2, 3
CZK_MEM_HOST, CZK_MEM_DEVICE = 0, 1
CZK_MEM_NO_TABLES = 32   # czk_bases_register: OR-ed with the above, see include/czk.h
CZK_MEM_ANY_POINTS = 64  # czk_bases_register: bases need not lie in the prime-order subgroup (keeps the XYZZ kernels for G1)
CZK_MEM_SCALAR_HOST = 256    # czk_fr_vec_scale: device vectors, host scalar
CZK_MEM_SAME_SCALARS = 512   # czk_msm_async: the scalars of the previous czk_msm_async call (its digit sort may be reused)
CZK_MEM_CHECK_SUBGROUP = 128  # czk_bases_register: verify [r] P == infinity; a failing base keeps the handle on the XYZZ kernels
CZK_SCALAR_CANONICAL, CZK_SCALAR_MONTGOMERY = 0, 1
CZK_POINTS_COMPRESSED, CZK_POINTS_CHECKED = 1, 2   # czk_points_deserialize flags
# czk_point_status
CZK_POINT_OK, CZK_POINT_BAD_FLAGS, CZK_POINT_NOT_CANONICAL, CZK_POINT_NO_POINT, CZK_POINT_NOT_ON_CURVE, CZK_POINT_NOT_IN_SUBGROUP = range(6)
POINT_STATUS_NAMES = ("OK", "BAD_FLAGS", "NOT_CANONICAL", "NO_POINT", "NOT_ON_CURVE", "NOT_IN_SUBGROUP")
CZK_G1, CZK_G2 = 1, 2
CZK_OP_ADD, CZK_OP_SUB, CZK_OP_MUL = 0, 1, 2
CZK_NET_RCCL, CZK_NET_SHM, CZK_NET_IPC = 1, 2, 3
CZK_OPEN_COMMIT = 1
CZK_OPEN_COMMIT_TREE = 2
CZK_COMMIT_LEAF_ELEMS, CZK_COMMIT_FANOUT = 32, 32   # czk.h "czk tree commitment v1": elements per leaf, digests per node
CZK_ERR_NET, CZK_ERR_CHECK = 5, 6
_STATUS = {1: "CZK_ERR_SIZE", 2: "CZK_ERR_HIP", 3: "CZK_ERR_ARG", 4: "CZK_ERR_NOMEM", 5: "CZK_ERR_NET", 6: "CZK_ERR_CHECK"}


CZK_SHARE_OP_MUL, CZK_SHARE_OP_INV, CZK_SHARE_OP_PARTIAL_PRODUCTS = 0, 1, 2   # czk_share_material_counts


def _share_material_counts(L, op: int, n: int):
    t, p = C.c_size_t(0), C.c_size_t(0)
    rc = L.czk_share_material_counts(C.c_int(op), C.c_size_t(n), C.byref(t), C.byref(p))
    if rc:
        raise CzkError(rc, "czk_share_material_counts: unknown op or a count that overflows")
    return t.value, p.value


CZK_GSZ_OP_MUL, CZK_GSZ_OP_INV, CZK_GSZ_OP_PARTIAL_PRODUCTS, CZK_GSZ_OP_PRODUCT_CHECK = 0, 1, 2, 3   # czk_gsz_material_counts
CZK_GSZ_GROUP_OP_MUL, CZK_GSZ_GROUP_OP_PRODUCT_CHECK = 0, 1   # czk_gsz_group_material_counts
CZK_GSZ_DN_DOUBLES, CZK_GSZ_DN_RANDS = 0, 1  # czk_gsz_dn_*: the same value under degree d and 2 d / degree d only
CZK_FQ12_OP_MUL, CZK_FQ12_OP_DIV, CZK_FQ12_OP_INV = 0, 1, 2   # czk_fq12_vec_op


def open_commit_flags(commit) -> int:
    """commit = True | False | "tree" -> the flags of czk_spdz_batch_open"""
    if isinstance(commit, str):
        if commit != "tree":
            raise ValueError(f"commit must be True, False or 'tree', not {commit!r}")
        return CZK_OPEN_COMMIT | CZK_OPEN_COMMIT_TREE
    return CZK_OPEN_COMMIT if commit else 0


class CzkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{_STATUS.get(code, code)}: {msg}")
        self.code = code


def lib_path() -> str:
    return _LIB


_LIB_LAB = os.path.join(_HERE, "libczk_hip_lab.so")   # the -DCZK_LAB build: product + the rejected variants kept for A/B runs (build.py)
_lib = None
_lab = None


def _load(path):
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(there is no CPU fallback for the product path)")
    # PyTorch-ROCm bundles its own libamdhip64.so.7; two HIP runtimes cannot share a process, so let
    # torch's copy load first (same SONAME -> the library binds to it).  torch is plumbing here: device
    # memory, streams, torch.distributed.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")   # see csrc/core.hip: must be set before HIP initialises
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    L.czk_last_error.restype = C.c_char_p
    L.czk_version.restype = C.c_char_p
    L.czk_bases_len.restype = C.c_size_t
    L.czk_lanes_count.restype = C.c_size_t
    L.czk_lanes_len.restype = C.c_size_t
    L.czk_lanes_data.restype = C.c_void_p
    L.czk_ctx_stream.restype = C.c_void_p
    L.czk_net_last_error.restype = C.c_char_p
    L.czk_net_destroy.restype = None
    L.czk_net_stats_reset.restype = None
    L.czk_sha256.restype = None
    L.czk_blake2s.restype = None
    L.czk_fs_release.restype = None
    L.czk_groth16_pvk_release.restype = None
    L.czk_fixed_base_release.restype = None
    L.czk_kzg10_vk_release.restype = None
    return L


def lab_lib():
    """The lab build (libczk_hip_lab.so): same ABI, plus the rejected kernel variants and their options.  Tests and tools only."""
    global _lab
    if _lab is None:
        _lab = _load(_LIB_LAB)
    return _lab


def lib():
    """Loads libczk_hip.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        _lib = _load(_LIB)
    return _lib


def header_symbols() -> list[str]:
    """Every function include/czk.h declares."""
    txt = open(_HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(czk_[a-z0-9_]+)\s*\(", txt)))


def exported_symbols() -> list[str]:
    l = lib()
    return [s for s in header_symbols() if hasattr(l, s)]


def _key_bytes(b, length: int):
    """exactly `length` bytes as a ctypes array (keys and nonces: a wrong length must not read past the buffer)"""
    b = bytes(b)
    if len(b) != length:
        raise ValueError(f"expected {length} bytes, got {len(b)}")
    return (C.c_uint8 * max(1, length)).from_buffer_copy(b or b"\0")


def _gsz_dn_counts(L, kind: int, parties: int, degree: int, want: int):
    deal, outs = C.c_size_t(0), C.c_size_t(0)
    rc = L.czk_gsz_dn_counts(C.c_int(kind), C.c_size_t(parties), C.c_uint(degree), C.c_size_t(want), C.byref(deal), C.byref(outs))
    if rc:
        raise CzkError(rc, "czk_gsz_dn_counts: unknown kind, a degree that leaves nothing to extract, or a count that overflows")
    return deal.value, outs.value


def _ptr(x):
    """numpy array -> void*, int -> void*, None -> NULL"""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(x))


# enum czk_lab_arith_op of csrc/lab/arith_probe.h: name -> (op, input words per item, output words per item)
LAB_ARITH_PROBE_OPS = {
    "fqu_mul": (0, 28, 14), "fqu_sqr": (1, 14, 14), "fqu_mul_add": (2, 56, 14), "fqu_mul_add_hi": (3, 70, 14), "fqu_mul_hi": (4, 42, 14),
    "fqu_mul_add4": (5, 112, 14), "fqu_normalize": (6, 14, 14), "fqu_sub_lazy<4>": (7, 28, 14), "fqu_sub_lazy<8>": (8, 28, 14),
    "fqu_sub_lazy<16>": (9, 28, 14), "fqu_sub3_norm": (10, 42, 14), "fqu_unpack": (11, 12, 14), "fqu_pack": (12, 14, 12),
    "fqu_neg5<false>": (13, 14, 14), "fqu_neg5<true>": (14, 14, 14), "fqu_add_lazy": (15, 28, 14), "fqu_subn_32": (16, 28, 14),
    "fqu_subn_64": (17, 28, 14), "fqu_subn_128": (18, 28, 14),
    "fq2u_mul": (20, 56, 28), "fq2u_sqr": (21, 28, 28), "fq2u_mul_n5": (22, 56, 28),
    "fqu_xyzz_acc_mixed": (30, 84, 57), "xyzzu_add": (31, 114, 57), "xyzzu_double": (32, 57, 57), "xyzzu_to_sat": (33, 57, 48),
    "xyzzu_from_sat": (34, 48, 57), "fq2u_xyzz_acc_mixed": (35, 168, 113),
    "teu_from_niels": (40, 42, 56), "teu_madd": (41, 98, 56), "teu_add": (42, 112, 56), "teu_double": (43, 56, 56), "teu_to_jac": (44, 56, 36),
    "te_load_niels": (45, 52, 42),
    "p2_mul": (50, 57, 28), "xyzzu2_add": (51, 226, 113), "xyzzu2_double": (52, 113, 113), "xyzzu2_acc_mixed": (53, 168, 113),
    "fqu_mul_s": (70, 28, 14), "fqu_sqr_s": (71, 14, 14), "fqu_mul_add_s": (72, 56, 14), "fqu_mul_add_hi_s": (73, 70, 14),
    "fqu_mul_hi_s": (74, 42, 14), "fqu_mul_add4_s": (75, 112, 14),
    "fru_mul": (60, 18, 9), "fru_normalize": (62, 9, 9), "fru_unpack": (63, 8, 9), "fru_pack": (64, 9, 8), "fru_reduce_2r": (65, 9, 9),
    "fru_canon": (66, 9, 8), "fru_canon_mulout": (67, 9, 8), "fru_add": (68, 18, 9),
}
LAB_ARITH_PROBE_OPS.update({f"fru_sub<{1 << lg},{u}>": (100 + 2 * lg + (u - 1), 18, 9) for lg in range(1, 9) for u in (1, 2)})


def _sat_probe_ops():
    """enum czk_lab_sat_fn of csrc/lab/arith_probe.h: the saturated field.h / tower.h / curve.h.  `name` is the function compiled with the
    Montgomery multiply inlined (op 200 + 2 fn), `name@noinline` the same function compiled with -DCZK_NOINLINE_MUL (op 200 + 2 fn + 1);
    the Fq6 / Fq12 functions exist in the second form only."""
    fns = {}
    for base, f, w in ((0, "fr", 8), (10, "fq", 12)):
        for i, (nm, k) in enumerate((("add", 2), ("sub", 2), ("dbl", 1), ("neg", 1), ("reduce", 1), ("mul", 2), ("sqr", 1), ("into_repr", 1),
                                     ("from_repr", 1), ("inv", 1))):
            fns[f"{f}_{nm}"] = (base + i, k * w, w)
    fns["fq_mul_by_nonresidue"] = (20, 12, 12)
    for i, (nm, iw) in enumerate((("add", 48), ("sub", 48), ("dbl", 24), ("neg", 24), ("mul", 48), ("sqr", 24), ("inv", 24), ("mul_by_u", 24),
                                  ("mul_fq", 36), ("conj", 24))):
        fns[f"fq2_{nm}"] = (21 + i, iw, 24)
    for base, g, w in ((31, "g1", 12), (41, "g2", 24)):
        for i, (nm, iw, ow) in enumerate((("jac_double", 3, 3), ("jac_add_mixed", 5, 3), ("jac_add", 6, 3), ("jac_to_affine", 3, 2),
                                          ("xyzz_double_affine", 2, 4), ("xyzz_double", 4, 4), ("xyzz_add_mixed", 6, 4), ("xyzz_acc_mixed", 6, 4),
                                          ("xyzz_add", 8, 4), ("xyzz_to_jac", 4, 3))):
            fns[f"{g}_{nm}"] = (base + i, iw * w + (nm == "jac_add_mixed"), ow * w + (nm == "jac_to_affine"))
    tower = {}
    for i, (nm, iw) in enumerate((("add", 144), ("sub", 144), ("neg", 72), ("mul_by_v", 72), ("mul", 144), ("mul_by_01", 120), ("mul_by_1", 96),
                                  ("inv", 72), ("frobenius_1", 72), ("frobenius_2", 72))):
        tower[f"fq6_{nm}"] = (51 + i, iw, 72)
    for i, (nm, iw) in enumerate((("mul", 288), ("sqr", 144), ("conj", 144), ("inv", 144), ("mul_by_034", 216), ("frobenius_1", 144),
                                  ("frobenius_2", 144), ("cyclotomic_square", 144), ("load_strided_1", 144), ("store_strided_1", 144),
                                  ("load_strided_n", 144), ("store_strided_n", 144))):
        tower[f"fq12_{nm}"] = (61 + i, iw, 144)
    ops = {nm: (200 + 2 * fn, iw, ow) for nm, (fn, iw, ow) in fns.items()}
    ops.update({nm + "@noinline": (200 + 2 * fn + 1, iw, ow) for nm, (fn, iw, ow) in {**fns, **tower}.items()})
    return ops


LAB_ARITH_PROBE_OPS.update(_sat_probe_ops())


LAB_NTT_PASS_SENTINEL = 0xA5A5A5A5   # csrc/lab/ntt_pass_probe.h: every word of the probe's output buffer before the launch


class LabNttPassDesc(C.Structure):
    """struct czk_lab_ntt_pass_desc of csrc/lab/ntt_pass_probe.h"""
    _fields_ = [(n, C.c_uint32) for n in ("mode", "log_d", "inverse", "K", "s_lo", "first", "last", "prescale", "posttab", "post_mode")] + \
               [(n, C.c_uint64) for n in ("lanes", "in_len", "in_lane_stride")]


class Context:
    """czk_ctx: one GPU + one HIP stream = one MPC party.

    `stream` is a hipStream_t handle (e.g. `torch.cuda.Stream().cuda_stream`).  None / 0 makes the context create its
    own non-blocking stream -- note torch's DEFAULT stream has handle 0, so to share a stream with torch ops use an
    explicit `torch.cuda.Stream()` (bench.py does)."""

    def __init__(self, device: int = 0, stream: int | None = None, lab: bool = False, options: dict | None = None):
        """lab=True binds this context to libczk_hip_lab.so (tests / A/B tools: the rejected kernel variants and their options);
        `options`: {name: value} passed to czk_ctx_set_option before any work."""
        self._L = lab_lib() if lab else lib()
        self._lab = bool(lab)
        self.device = int(device)
        self._h = C.c_void_p(0)
        rc = self._L.czk_ctx_create(C.byref(self._h), C.c_int(device), C.c_void_p(stream or 0))
        if rc:
            raise CzkError(rc, "czk_ctx_create failed (no visible GPU?)")
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def stream_handle(self) -> int:
        """hipStream_t of this context as an integer (czk_ctx_stream): torch.cuda.ExternalStream(handle) orders torch work against it"""
        return int(self._L.czk_ctx_stream(self._h) or 0)

    def reserve(self, ntt_log_d: int = 0, ntt_lanes: int = 0, bases=None, n_scalars: int = 0, msm_lanes: int = 0):
        """czk_ctx_reserve: build NTT tables / size MSM workspaces now instead of inside the first proof"""
        self._ck(self._L.czk_ctx_reserve(self._h, C.c_uint(ntt_log_d), C.c_size_t(ntt_lanes), bases._h if bases is not None else None, C.c_size_t(n_scalars),
                                         C.c_size_t(msm_lanes)))

    def set_option(self, name: str, value: int):
        self._ck(self._L.czk_ctx_set_option(self._h, name.encode(), C.c_long(int(value))))

    def lab_arith_probe(self, op: str, items):
        """czk_lab_arith_probe (csrc/lab/arith_probe.h, lab library only): runs the function named `op` (a key of LAB_ARITH_PROBE_OPS)
        of the unsaturated arithmetic headers, or of the saturated field.h / tower.h / curve.h, once per row of `items` -- raw u32 limbs
        exactly as given -- and returns the raw result rows.  Raises unless the context was opened with lab=True: the product library does not carry the probe."""
        if not self._lab:
            raise RuntimeError("lab_arith_probe needs Context(lab=True): libczk_hip.so does not export czk_lab_arith_probe")
        code, iw, ow = LAB_ARITH_PROBE_OPS[op]
        a = np.ascontiguousarray(items, dtype=np.uint32)
        if a.ndim != 2 or a.shape[1] != iw:
            raise ValueError(f"{op} takes {iw} words per item, got an array of shape {a.shape}")
        out = np.zeros((a.shape[0], ow), dtype=np.uint32)
        self._ck(self._L.czk_lab_arith_probe(self._h, C.c_int(code), _ptr(a), C.c_size_t(iw), _ptr(out), C.c_size_t(ow), C.c_size_t(a.shape[0]),
                                             C.c_int(CZK_MEM_HOST)))
        return out

    def lab_msm_sort(self, c: int, scalars, size: int | None = None, split: bool = False, one_pass: bool = False,
                     scalar_form: int = CZK_SCALAR_CANONICAL, inf=None, nb: int | None = None, dims_only: bool = False):
        """czk_lab_msm_sort (csrc/lab/msm_sort_probe.hip, lab library only): the digit sort of one MSM call on its own.  scalars: (lanes,
        n_scalars, 4) u64, of which the first `size` of each lane count; c: the window width (0 with split: the width a table-free call of
        `size` pairs gets); inf: the table set's infinity flags, (Wd, nb) bytes -- (nb,) with split -- or None; nb: points per window
        (default: size).  Returns the dimensions the product's own plan code derives (c, Wd, W, lanes = bucket sets, B, total, n_parts,
        part_shift, cap) and, unless dims_only, the arrays: digits and sorted (lanes, total), counts, offsets and perm (lanes, B); `sorted`
        holds 0xFFFFFFFF where the sort wrote nothing.  Raises unless the context was opened with lab=True."""
        if not self._lab:
            raise RuntimeError("lab_msm_sort needs Context(lab=True): libczk_hip.so does not export czk_lab_msm_sort")
        sc = np.ascontiguousarray(scalars, dtype=np.uint64)
        if sc.ndim != 3 or sc.shape[2] != 4:
            raise ValueError(f"scalars must have the shape (lanes, n_scalars, 4), got {sc.shape}")
        lanes, n_scalars = sc.shape[0], sc.shape[1]
        size = n_scalars if size is None else int(size)
        nb = size if nb is None else int(nb)
        dims = np.zeros(9, dtype=np.uint64)

        def call(inf_arr, outs):
            self._ck(self._L.czk_lab_msm_sort(self._h, C.c_uint(c), C.c_int(int(split)), C.c_int(int(one_pass)), _ptr(sc), C.c_size_t(n_scalars),
                                              C.c_size_t(lanes), C.c_size_t(size), C.c_int(scalar_form), _ptr(inf_arr), C.c_size_t(nb), _ptr(dims),
                                              *[_ptr(o) for o in outs]))

        call(None, [None] * 5)
        out = dict(zip(("c", "Wd", "W", "lanes", "B", "total", "n_parts", "part_shift", "cap"), (int(v) for v in dims)))
        if dims_only:
            return out
        if inf is not None:
            inf = np.ascontiguousarray(inf, dtype=np.uint8)
            if inf.shape != ((nb,) if split else (out["Wd"], nb)):
                raise ValueError(f"inf must have the shape (Wd, nb) -- (nb,) with split -- got {inf.shape}")
        arrs = [np.zeros((out["lanes"], max(1, out[k])), dtype=np.uint32) for k in ("total", "total", "B", "B", "B")]
        call(inf, arrs)
        for name, a, k in zip(("digits", "sorted", "counts", "offsets", "perm"), arrs, ("total", "total", "B", "B", "B")):
            out[name] = a[:, :out[k]]
        return out

    def lab_merkle_commit(self, a: int, lanes: int, n: int, stride: int, tree: int, tree_stride: int):
        """czk_lab_merkle_commit (csrc/lab/merkle_probe.hip, lab library only): czk_fr_merkle_commit's tree in the form that was not shipped, on device
        pointers; only enqueues.  Raises unless the context was opened with lab=True."""
        if not self._lab:
            raise RuntimeError("lab_merkle_commit needs Context(lab=True): libczk_hip.so does not export czk_lab_merkle_commit")
        self._ck(self._L.czk_lab_merkle_commit(self._h, _ptr(a), C.c_size_t(lanes), C.c_size_t(n), C.c_size_t(stride), _ptr(tree), C.c_size_t(tree_stride)))

    def lab_msm_buckets(self, bases: "Bases", B: int, sorted_, offsets, counts, perm, dims_only: bool = False):
        """czk_lab_msm_buckets (csrc/lab/msm_bucket_probe.hip, lab library only): the bucket accumulation, the over-full-bucket and fix-up
        kernels and the bucket reduction of one MSM call on entry lists the caller wrote, over the tables of a registered key.  sorted_:
        (lanes, total) u32 entry codes (w * nb + i) | sign << 31; offsets, counts, perm: (lanes, B) u32.  Returns the dimensions (c, W, nb,
        family: 0 twisted Edwards / 1 u-form XYZZ / 2 saturated XYZZ, heavy_chunk, heavy_sub, exc_cap, heavy_cap) and, unless dims_only,
        "buckets" (lanes, B, 18|36) Jacobian triples after the fix-up, the counters "exc_count", "dirty", "items", "heavy", "overflow", and
        "result" (lanes, 18|36).  A list the kernels could not read safely raises CzkError.  Raises unless the context was opened with lab=True."""
        if not self._lab:
            raise RuntimeError("lab_msm_buckets needs Context(lab=True): libczk_hip.so does not export czk_lab_msm_buckets")
        srt = np.ascontiguousarray(sorted_, dtype=np.uint32)
        arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (offsets, counts, perm)]
        if srt.ndim != 2 or any(a.shape != (srt.shape[0], B) for a in arrs):
            raise ValueError("sorted must have the shape (lanes, total); offsets, counts and perm (lanes, B)")
        lanes, total = srt.shape
        jw = 18 if bases.group == CZK_G1 else 36
        dims = np.zeros(8, dtype=np.uint64)
        buckets = np.zeros((lanes, B, jw), dtype=np.uint64)
        counters = np.zeros(5, dtype=np.uint32)
        result = np.zeros((lanes, jw), dtype=np.uint64)
        outs = [None, None, None] if dims_only else [buckets, counters, result]
        self._ck(self._L.czk_lab_msm_buckets(self._h, bases._h, C.c_size_t(lanes), C.c_size_t(B), C.c_size_t(total), _ptr(srt), *[_ptr(a) for a in arrs],
                                             _ptr(dims), *[_ptr(o) for o in outs]))
        out = dict(zip(("c", "W", "nb", "family", "heavy_chunk", "heavy_sub", "exc_cap", "heavy_cap"), (int(v) for v in dims)))
        if not dims_only:
            out.update(buckets=buckets, result=result, **dict(zip(("exc_count", "dirty", "items", "heavy", "overflow"), (int(v) for v in counters))))
        return out

    def lab_ntt_pass(self, log_d: int, K: int = 0, s_lo: int = 0, data=None, fused: bool = False, inverse: bool = False, first: bool = False,
                     last: bool = False, lanes: int = 1, in_len: int = 0, in_lane_stride: int = 0, prescale: bool = False, posttab: bool = False,
                     post_mode: int = 0, addend=None, postconst2=None, dims_only: bool = False):
        """czk_lab_ntt_pass (csrc/lab/ntt_pass_probe.h, lab library only): ONE pass of the second-generation NTT -- launch_ntt2_pass, or with `fused`
        launch_ntt2_final_first -- on the buffer `data`, with the domain's own tables.  data: u32 words, (lanes * in_lane_stride, 8) canonical elements
        for a first pass, (lanes * 2^log_d, scratch words) otherwise; addend: (lanes * 2^log_d, 8) canonical; postconst2: 8 words, one canonical
        Montgomery element.  Returns the dimensions (scratch format, its element bytes, NTT2_MIN_LOG, NTT2_T, the guard length, pass_plan(log_d) as m, K,
        s_lo, equal_groups) and, unless dims_only, "out": (lanes * 2^log_d + guard, words) u32, every row the pass did not write still
        LAB_NTT_PASS_SENTINEL.  A description the kernels could not run safely raises CzkError (CZK_ERR_ARG).  Raises unless the context was
        opened with lab=True."""
        if not self._lab:
            raise RuntimeError("lab_ntt_pass needs Context(lab=True): libczk_hip.so does not export czk_lab_ntt_pass")
        desc = LabNttPassDesc(mode=1 if fused else 0, log_d=log_d, inverse=int(inverse), K=K, s_lo=s_lo, first=int(first), last=int(last),
                              prescale=int(prescale), posttab=int(posttab), post_mode=post_mode, lanes=lanes, in_len=in_len, in_lane_stride=in_lane_stride)
        dims = np.zeros(21, dtype=np.uint64)

        def unpack():
            d = [int(v) for v in dims]
            return {"format": d[0], "elem_bytes": d[1], "min_log": d[2], "T": d[3], "guard": d[4], "m": d[5], "equal_groups": bool(d[6]),
                    "K": d[7:7 + d[5]], "s_lo": d[14:14 + d[5]]}

        self._ck(self._L.czk_lab_ntt_pass(self._h, C.byref(desc), None, C.c_size_t(0), None, None, _ptr(dims), None, C.c_size_t(0)))
        out = unpack()
        if dims_only:
            return out
        a = np.ascontiguousarray(data, dtype=np.uint32)
        if a.ndim != 2:
            raise ValueError("data must have the shape (elements, words per element)")
        ow = 8 if last and not fused else out["elem_bytes"] // 4
        res = np.zeros(((lanes << min(log_d, 20)) + out["guard"], ow), dtype=np.uint32)
        add = None if addend is None else np.ascontiguousarray(addend, dtype=np.uint32)
        c2 = None if postconst2 is None else np.ascontiguousarray(postconst2, dtype=np.uint32)
        if c2 is not None and c2.shape != (8,):
            raise ValueError("postconst2 is one element of 8 words")
        if add is not None and add.shape != (lanes << log_d, 8):
            raise ValueError("addend must have the shape (lanes * 2^log_d, 8)")
        keep = a if a.size else np.zeros((1, 8), dtype=np.uint32)   # an empty first-pass input still needs a pointer
        self._ck(self._L.czk_lab_ntt_pass(self._h, C.byref(desc), _ptr(keep), C.c_size_t(a.nbytes), _ptr(add), _ptr(c2), _ptr(dims), _ptr(res),
                                          C.c_size_t(res.nbytes)))
        out = unpack()
        out["out"] = res
        return out

    def close(self):
        if self._h:
            self._L.czk_ctx_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise CzkError(rc, (self._L.czk_last_error(self._h) or b"").decode())

    def sync(self):
        self._ck(self._L.czk_ctx_sync(self._h))

    def mark(self) -> int:
        """czk_ctx_mark: names the work enqueued on the context so far (kernels, msm_async calls, deferred downloads)"""
        m = C.c_uint64(0)
        self._ck(self._L.czk_ctx_mark(self._h, C.byref(m)))
        return m.value

    def wait_mark(self, mark: int):
        """czk_ctx_wait_mark: blocks until the work before `mark` is done and delivers its host results; later calls keep running"""
        self._ck(self._L.czk_ctx_wait_mark(self._h, C.c_uint64(mark)))

    # ---- device-resident share lanes ---------------------------------------------------------------
    def lanes_alloc(self, lanes: int, length: int) -> "Lanes":
        """czk_lanes_alloc: `lanes` x `length` Fr in HBM, zero-filled; the handle a caller without a HIP allocator uses."""
        h = C.c_void_p(0)
        self._ck(self._L.czk_lanes_alloc(self._h, C.c_size_t(lanes), C.c_size_t(length), C.byref(h)))
        return Lanes(self, h)

    # ---- NTT ------------------------------------------------------------------------------------
    def ntt_fr_to(self, src, src_stride: int, dst, log_d: int, kind: int, lanes: int = 1, in_len: int | None = None):
        """EvaluationDomain::{fft,ifft,coset_fft,coset_ifft} (not in place): device pointers; reads in_len elements per source lane (stride
        src_stride elements), writes 2^log_d per lane to dst."""
        if in_len is None:
            in_len = min(src_stride, 1 << log_d)
        self._ck(self._L.czk_ntt_fr_to(self._h, _ptr(src), C.c_size_t(src_stride), _ptr(dst), C.c_uint(log_d), C.c_size_t(lanes), C.c_int(kind),
                                     C.c_size_t(in_len), C.c_int(CZK_MEM_DEVICE)))
        return dst

    def ntt_fr(self, data, log_d: int, kind: int, lanes: int = 1, in_len: int | None = None, mem: int = CZK_MEM_HOST):
        """EvaluationDomain::{fft,ifft,coset_fft,coset_ifft}_in_place on `lanes` Fr lanes (in place)."""
        d = 1 << log_d
        if in_len is None:
            in_len = d
        if isinstance(data, np.ndarray):
            assert data.dtype == np.uint64 and (log_d > 40 or data.size == lanes * d * 4), "buffer must hold lanes x D x 4 u64"
        self._ck(self._L.czk_ntt_fr(self._h, _ptr(data), C.c_uint(log_d), C.c_size_t(lanes), C.c_int(kind), C.c_size_t(in_len),
                                  C.c_int(mem)))
        return data

    def ntt_fr_mixed(self, data, size: int, kind: int, lanes: int = 1, in_len: int | None = None, mem: int = CZK_MEM_HOST):
        """MixedRadixEvaluationDomain::{fft,ifft,coset_fft,coset_ifft}_in_place over a domain of `size` = 2^a or 3 * 2^a."""
        if in_len is None:
            in_len = size
        if isinstance(data, np.ndarray):
            assert data.dtype == np.uint64 and data.size == lanes * size * 4, "buffer must hold lanes x size x 4 u64"
        self._ck(self._L.czk_ntt_fr_mixed(self._h, _ptr(data), C.c_size_t(size), C.c_size_t(lanes), C.c_int(kind), C.c_size_t(in_len), C.c_int(mem)))
        return data

    def mixed_domain_constants(self, size: int):
        out = np.zeros((6, 4), dtype=np.uint64)
        self._ck(self._L.czk_mixed_domain_constants(self._h, C.c_size_t(size), _ptr(out)))
        names = ["size_inv", "group_gen", "group_gen_inv", "generator", "generator_inv", "vanishing_inv"]
        return dict(zip(names, out))

    def domain_constants(self, log_d: int):
        out = np.zeros((6, 4), dtype=np.uint64)
        self._ck(self._L.czk_domain_constants(self._h, C.c_uint(log_d), _ptr(out)))
        names = ["size_inv", "group_gen", "group_gen_inv", "generator", "generator_inv", "vanishing_inv"]
        return dict(zip(names, out))

    # ---- pointwise ------------------------------------------------------------------------------
    def fr_vec_op(self, op, a, b, out=None, n=None, mem=CZK_MEM_HOST):
        if mem == CZK_MEM_HOST:
            a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
            n = a.size // 4
            out = np.empty_like(a) if out is None else out
        self._ck(self._L.czk_fr_vec_op(self._h, C.c_int(op), _ptr(a), _ptr(b), _ptr(out), C.c_size_t(n), C.c_int(mem)))
        return out

    def fr_vec_scale(self, a, k, out=None, n=None, mem=CZK_MEM_HOST):
        if mem == (CZK_MEM_DEVICE | CZK_MEM_SCALAR_HOST):
            k = np.ascontiguousarray(k, np.uint64).reshape(4)
        if mem == CZK_MEM_HOST:
            a, k = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(k, np.uint64)
            n = a.size // 4
            out = np.empty_like(a) if out is None else out
        self._ck(self._L.czk_fr_vec_scale(self._h, _ptr(a), _ptr(k), _ptr(out), C.c_size_t(n), C.c_int(mem)))
        return out

    def fr_powers(self, g, n: int, c=None, out=None, mem=CZK_MEM_HOST):
        """out[i] = c * g^i (g, c: (4,) uint64 Montgomery)."""
        g = np.ascontiguousarray(g, np.uint64).reshape(4)
        cc = None if c is None else np.ascontiguousarray(c, np.uint64).reshape(4)
        if mem == CZK_MEM_HOST:
            out = np.zeros((n, 4), dtype=np.uint64)
        self._ck(self._L.czk_fr_powers(self._h, _ptr(g), _ptr(cc), C.c_size_t(n), _ptr(out), C.c_int(mem)))
        return out

    def fr_beaver_combine(self, x, y, z, sx, oy, add_open, out=None, n=None, mem=CZK_MEM_HOST):
        if mem == CZK_MEM_HOST:
            x, y, z, sx, oy = (np.ascontiguousarray(v, np.uint64) for v in (x, y, z, sx, oy))
            n = x.size // 4
            out = np.empty_like(x) if out is None else out
        self._ck(self._L.czk_fr_beaver_combine(self._h, _ptr(x), _ptr(y), _ptr(z), _ptr(sx), _ptr(oy), C.c_int(int(add_open)),
                                             _ptr(out), C.c_size_t(n), C.c_int(mem)))
        return out

    def fr_into_repr(self, a, out=None, n=None, mem=CZK_MEM_HOST):
        if mem == CZK_MEM_HOST:
            a = np.ascontiguousarray(a, np.uint64)
            n = a.size // 4
            out = np.empty_like(a) if out is None else out
        self._ck(self._L.czk_fr_into_repr(self._h, _ptr(a), _ptr(out), C.c_size_t(n), C.c_int(mem)))
        return out

    def fr_from_repr(self, a, out=None, n=None, mem=CZK_MEM_HOST):
        if mem == CZK_MEM_HOST:
            a = np.ascontiguousarray(a, np.uint64)
            n = a.size // 4
            out = np.empty_like(a) if out is None else out
        self._ck(self._L.czk_fr_from_repr(self._h, _ptr(a), _ptr(out), C.c_size_t(n), C.c_int(mem)))
        return out

    def fr_vec_serialize(self, a, n=None, mem=CZK_MEM_HOST) -> bytes:
        """`Vec<Fr>::serialize`: u64 length prefix + 32 little-endian bytes of into_repr() per element"""
        if mem == CZK_MEM_HOST:
            a = np.ascontiguousarray(a, np.uint64)
            n = a.size // 4
        out = np.zeros(8 + 32 * n, dtype=np.uint8)
        self._ck(self._L.czk_fr_vec_serialize(self._h, _ptr(a if n else None), C.c_size_t(n), C.c_int(mem), _ptr(out)))
        return out.tobytes()

    def fr_vec_commit(self, a, rand32: bytes, lanes: int = 1, n=None, stride=None, mem=CZK_MEM_HOST) -> bytes:
        """czk.h "czk tree commitment v1" of `lanes` vectors of n Montgomery Fr, `stride` elements apart, hashed on the GPU: lanes x 32 bytes.
        rand32: lanes x 32 bytes.  Host mode: a is (lanes, n, 4) / (n, 4) limbs (n and stride from its shape unless given); device mode: a pointer."""
        if mem == CZK_MEM_HOST and a is not None:
            a = np.ascontiguousarray(a, np.uint64)
            if n is None:
                n = a.size // (4 * lanes) if lanes else 0
        n = 0 if n is None else n
        stride = n if stride is None else stride
        rnd = np.frombuffer(bytes(rand32), dtype=np.uint8)
        if rnd.size != 32 * lanes:
            raise ValueError("rand32 must hold 32 bytes per lane")
        out = np.zeros(32 * lanes, dtype=np.uint8)
        self._ck(self._L.czk_fr_vec_commit(self._h, _ptr(a if (n and lanes) else None), C.c_size_t(lanes), C.c_size_t(n), C.c_size_t(stride),
                                           _ptr(rnd if lanes else None), _ptr(out if lanes else None), C.c_int(mem)))
        return out.tobytes()

    def fr_vec_deserialize(self, data: bytes, out=None, cap=None, mem=CZK_MEM_HOST):
        """inverse of fr_vec_serialize; host mode returns (n, 4) Montgomery limbs, device mode the element count"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        if mem == CZK_MEM_HOST:
            cap = max(0, (len(data) - 8) // 32)
            out = np.zeros((cap, 4), dtype=np.uint64)
        n = C.c_size_t(0)
        self._ck(self._L.czk_fr_vec_deserialize(self._h, _ptr(buf), C.c_size_t(len(data)), _ptr(out if cap else None), C.c_size_t(cap), C.c_int(mem), C.byref(n)))
        return out[: n.value] if mem == CZK_MEM_HOST else n.value

    # ---- MSM ------------------------------------------------------------------------------------
    def register_bases(self, group: int, bases, inf=None, n: int | None = None, mem: int = CZK_MEM_HOST) -> "Bases":
        aw = 12 if group == CZK_G1 else 24
        if (mem & ~(CZK_MEM_NO_TABLES | CZK_MEM_ANY_POINTS | CZK_MEM_CHECK_SUBGROUP)) == CZK_MEM_HOST:
            bases = np.ascontiguousarray(bases, np.uint64)
            n = bases.size // aw
            if inf is not None:
                inf = np.ascontiguousarray(inf, np.uint8)
        h = C.c_void_p(0)
        self._ck(self._L.czk_bases_register(self._h, C.c_int(group), _ptr(bases), _ptr(inf), C.c_size_t(n), C.c_int(mem), C.byref(h)))
        return Bases(self, h, group, n)

    def msm(self, bases: "Bases", scalars, n_scalars: int | None = None, lanes: int = 1, scalar_form: int = CZK_SCALAR_CANONICAL,
            mem: int = CZK_MEM_HOST):
        """VariableBaseMSM::multi_scalar_mul over `lanes` scalar vectors; returns (lanes, 18|36) Jacobian limbs."""
        jw = 18 if bases.group == CZK_G1 else 36
        if mem == CZK_MEM_HOST:
            scalars = np.ascontiguousarray(scalars, np.uint64)
            if n_scalars is None:
                n_scalars = scalars.size // (4 * lanes)
        out = np.zeros((lanes, jw), dtype=np.uint64)
        self._ck(self._L.czk_msm(self._h, bases._h, _ptr(scalars), C.c_size_t(n_scalars), C.c_size_t(lanes), C.c_int(scalar_form),
                               C.c_int(mem), _ptr(out)))
        return out

    def msm_async(self, bases: "Bases", scalars_ptr, n_scalars: int, lanes: int, scalar_form: int, out: np.ndarray, stable: bool = False,
                  same_scalars: bool = False):
        """czk_msm_async on device scalars; `out` (numpy, lanes x 18|36) is valid after sync().  stable=True promises
        the scalars stay untouched until then (CZK_MEM_STABLE); same_scalars=True (with stable) says they are the previous
        czk_msm_async call's scalars, whose digit sort the library may then take over (CZK_MEM_SAME_SCALARS)."""
        self._ck(self._L.czk_msm_async(self._h, bases._h, _ptr(scalars_ptr), C.c_size_t(n_scalars), C.c_size_t(lanes), C.c_int(scalar_form),
                                     C.c_int(CZK_MEM_DEVICE | (16 if stable else 0) | (CZK_MEM_SAME_SCALARS if same_scalars else 0)), _ptr(out)))
        return out

    def msm_oneshot(self, group, bases, inf, scalars, lanes=1, scalar_form=CZK_SCALAR_CANONICAL):
        aw, jw = (12, 18) if group == CZK_G1 else (24, 36)
        bases = np.ascontiguousarray(bases, np.uint64)
        scalars = np.ascontiguousarray(scalars, np.uint64)
        n = bases.size // aw
        inf = None if inf is None else np.ascontiguousarray(inf, np.uint8)
        out = np.zeros((lanes, jw), dtype=np.uint64)
        fn = self._L.czk_msm_g1 if group == CZK_G1 else self._L.czk_msm_g2
        self._ck(fn(self._h, _ptr(bases), _ptr(inf), _ptr(scalars), C.c_size_t(n), C.c_size_t(lanes), C.c_int(scalar_form), _ptr(out)))
        return out

    def jac_to_affine(self, group, jac):
        aw, jw = (12, 18) if group == CZK_G1 else (24, 36)
        jac = np.ascontiguousarray(jac, np.uint64).reshape(-1, jw)
        n = jac.shape[0]
        aff = np.zeros((n, aw), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.uint8)
        self._ck(self._L.czk_jac_to_affine(self._h, C.c_int(group), _ptr(jac), C.c_size_t(n), _ptr(aff), _ptr(inf)))
        return aff, inf

    def jac_add(self, group, a, b):
        jw = 18 if group == CZK_G1 else 36
        a, b = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b, np.uint64)
        out = np.zeros(jw, dtype=np.uint64)
        self._ck(self._L.czk_jac_add(self._h, C.c_int(group), _ptr(a), _ptr(b), _ptr(out)))
        return out

    def jac_add_mixed(self, group, a, b_aff, b_inf=False):
        jw = 18 if group == CZK_G1 else 36
        a, b_aff = np.ascontiguousarray(a, np.uint64), np.ascontiguousarray(b_aff, np.uint64)
        out = np.zeros(jw, dtype=np.uint64)
        self._ck(self._L.czk_jac_add_mixed(self._h, C.c_int(group), _ptr(a), _ptr(b_aff), C.c_int(int(b_inf)), _ptr(out)))
        return out

    def jac_scalar_mul(self, group, a, k, scalar_form=CZK_SCALAR_CANONICAL):
        """ProjectiveCurve::mul on a host Jacobian value; k: (4,) uint64 (canonical, or Montgomery with CZK_SCALAR_MONTGOMERY)"""
        jw = 18 if group == CZK_G1 else 36
        a, k = np.ascontiguousarray(a, np.uint64).reshape(jw), np.ascontiguousarray(k, np.uint64).reshape(4)
        out = np.zeros(jw, dtype=np.uint64)
        self._ck(self._L.czk_jac_scalar_mul(self._h, C.c_int(group), _ptr(a), _ptr(k), C.c_int(scalar_form), _ptr(out)))
        return out

    def jac_neg(self, group, a):
        jw = 18 if group == CZK_G1 else 36
        a = np.ascontiguousarray(a, np.uint64).reshape(jw)
        out = np.zeros(jw, dtype=np.uint64)
        self._ck(self._L.czk_jac_neg(self._h, C.c_int(group), _ptr(a), _ptr(out)))
        return out

    def fr_copy_3d(self, dst_ptr, dst_stride, src_ptr, src_stride, n):
        """czk_fr_copy_3d: strided copy (src_ptr None: zero fill) of Fr elements in device memory, in stream order; strides / extents: 3 ints each"""
        ds = (C.c_size_t * 3)(*[int(v) for v in dst_stride])
        ss = (C.c_size_t * 3)(*[int(v) for v in (src_stride or (0, 0, 0))])
        nn = (C.c_size_t * 3)(*[int(v) for v in n])
        self._ck(self._L.czk_fr_copy_3d(self._h, _ptr(dst_ptr), ds, _ptr(src_ptr), ss if src_ptr is not None else None, nn))

    def fr_spdz_open(self, shares_ptr, parties: int, n: int, out_value_ptr) -> int:
        """Local part of SpdzFieldShare::batch_open on device buffers; returns the number of failed MAC checks."""
        bad = C.c_uint64(0)
        self._ck(self._L.czk_fr_spdz_open(self._h, _ptr(shares_ptr), C.c_size_t(parties), C.c_size_t(n), _ptr(out_value_ptr), C.byref(bad)))
        return bad.value

    def fr_lanes_sum(self, x_ptr, k: int, n: int, out_ptr=None, count_nonzero: bool = False):
        """out[i] = sum of k device vectors; returns the number of non-zero sums when count_nonzero."""
        nz = C.c_uint64(0)
        self._ck(self._L.czk_fr_lanes_sum(self._h, _ptr(x_ptr), C.c_size_t(k), C.c_size_t(n), _ptr(out_ptr), C.byref(nz) if count_nonzero else C.c_void_p(0)))
        return nz.value

    def fr_spdz_dx(self, value_ptr, mac_ptr, mac_share, out_ptr, n: int):
        """dx_t = mac_share * value - mac on device vectors (share/spdz.rs:176-180); mac_share: (4,) uint64 Montgomery."""
        ms = np.ascontiguousarray(mac_share, np.uint64).reshape(4)
        self._ck(self._L.czk_fr_spdz_dx(self._h, _ptr(value_ptr), _ptr(mac_ptr), _ptr(ms), _ptr(out_ptr), C.c_size_t(n)))

    # ---- FieldShare::batch_mul / batch_inv / partial_products on device lanes (czk.h; csrc/share_mul.hip) ---------------------
    def share_material_counts(self, op: int, n: int):
        """(triples, inverse pairs) one call of `op` (CZK_SHARE_OP_*) over n elements consumes"""
        return _share_material_counts(self._L, op, n)

    def _share_call(self, fn, lpp, parties, mac_shares, ptrs, out_ptr, n):
        ms = None if mac_shares is None else np.ascontiguousarray(mac_shares, np.uint64).reshape(-1, 4)
        assert ms is None or ms.shape[0] >= parties
        bad, zero = C.c_uint64(0), C.c_uint64(0)
        self._ck(fn(self._h, C.c_size_t(lpp), C.c_size_t(parties), _ptr(ms), *[_ptr(p) for p in ptrs], _ptr(out_ptr), C.c_size_t(n), C.byref(bad),
                    C.byref(zero)))
        return bad.value, zero.value

    def share_batch_mul(self, lpp: int, parties: int, mac_shares, x_ptr, y_ptr, tx_ptr, ty_ptr, tz_ptr, out_ptr, n: int):
        """czk_share_batch_mul: every vector lpp * parties device lanes; mac_shares (parties, 4) Montgomery limbs (None for lpp = 1).
        Returns (failed MAC checks, 0)."""
        return self._share_call(self._L.czk_share_batch_mul, lpp, parties, mac_shares, (x_ptr, y_ptr, tx_ptr, ty_ptr, tz_ptr), out_ptr, n)

    def share_batch_inv(self, lpp: int, parties: int, mac_shares, x_ptr, pb_ptr, pc_ptr, tx_ptr, ty_ptr, tz_ptr, out_ptr, n: int):
        """czk_share_batch_inv -> (failed MAC checks, zero divisors)"""
        return self._share_call(self._L.czk_share_batch_inv, lpp, parties, mac_shares, (x_ptr, pb_ptr, pc_ptr, tx_ptr, ty_ptr, tz_ptr), out_ptr, n)

    def share_partial_products(self, lpp: int, parties: int, mac_shares, x_ptr, pb_ptr, pc_ptr, tx_ptr, ty_ptr, tz_ptr, out_ptr, n: int):
        """czk_share_partial_products -> (failed MAC checks, zero divisors)"""
        return self._share_call(self._L.czk_share_partial_products, lpp, parties, mac_shares, (x_ptr, pb_ptr, pc_ptr, tx_ptr, ty_ptr, tz_ptr), out_ptr, n)

    # ---- gsz20's batch_mult / batch_inv / partial_products and the product check on device lanes (czk.h; csrc/gsz_mul.hip) -------------
    def gsz_material_counts(self, op: int, n: int):
        """(double shares, random shares) one call of `op` (CZK_GSZ_OP_*) over n elements consumes"""
        d, r = C.c_size_t(0), C.c_size_t(0)
        rc = self._L.czk_gsz_material_counts(C.c_int(op), C.c_size_t(n), C.byref(d), C.byref(r))
        if rc:
            raise CzkError(rc, "czk_gsz_material_counts: unknown op or a count that overflows")
        return d.value, r.value

    def _gsz_call(self, fn, parties, degree, ptrs, n):
        a, b = C.c_uint64(0), C.c_uint64(0)
        out = ptrs[-1]
        self._ck(fn(self._h, C.c_size_t(parties), C.c_uint(degree), *[_ptr(p) for p in ptrs[:-1]], _ptr(out), C.c_size_t(n), C.byref(a), C.byref(b)))
        return a.value, b.value

    def gsz_share_batch_mul(self, parties: int, degree: int, x_ptr, y_ptr, doubles_r_ptr, doubles_r2_ptr, out_ptr, n: int):
        """czk_gsz_share_batch_mul: every vector `parties` device lanes, party j's lane = p(w^j) -> (degree violations, 0)"""
        return self._gsz_call(self._L.czk_gsz_share_batch_mul, parties, degree, (x_ptr, y_ptr, doubles_r_ptr, doubles_r2_ptr, out_ptr), n)

    def gsz_share_batch_inv(self, parties: int, degree: int, x_ptr, doubles_r_ptr, doubles_r2_ptr, rands_ptr, out_ptr, n: int):
        """czk_gsz_share_batch_inv -> (degree violations, zero divisors)"""
        return self._gsz_call(self._L.czk_gsz_share_batch_inv, parties, degree, (x_ptr, doubles_r_ptr, doubles_r2_ptr, rands_ptr, out_ptr), n)

    def gsz_share_partial_products(self, parties: int, degree: int, x_ptr, doubles_r_ptr, doubles_r2_ptr, rands_ptr, out_ptr, n: int):
        """czk_gsz_share_partial_products -> (degree violations, zero divisors)"""
        return self._gsz_call(self._L.czk_gsz_share_partial_products, parties, degree, (x_ptr, doubles_r_ptr, doubles_r2_ptr, rands_ptr, out_ptr), n)

    def gsz_product_check(self, parties: int, degree: int, xs_ptr, ys_ptr, zs_ptr, n: int, doubles_r_ptr, doubles_r2_ptr, rands_ptr):
        """czk_gsz_product_check over n triples -> (ok, degree violations); ok = False is a result, not an error"""
        ok, bad = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.czk_gsz_product_check(self._h, C.c_size_t(parties), C.c_uint(degree), _ptr(xs_ptr), _ptr(ys_ptr), _ptr(zs_ptr), C.c_size_t(n),
                                             _ptr(doubles_r_ptr), _ptr(doubles_r2_ptr), _ptr(rands_ptr), C.byref(ok), C.byref(bad)))
        return bool(ok.value), bad.value

    # ---- a shared point times a shared scalar on device lanes: GroupShare::scale and gsz20's group mult (czk.h; csrc/group_share.hip) ------------
    def gsz_group_material_counts(self, op: int, n: int):
        """(group doubles, field doubles, random shares) one call of `op` (CZK_GSZ_GROUP_OP_*) over n elements consumes"""
        g, f, r = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        rc = self._L.czk_gsz_group_material_counts(C.c_int(op), C.c_size_t(n), C.byref(g), C.byref(f), C.byref(r))
        if rc:
            raise CzkError(rc, "czk_gsz_group_material_counts: unknown op or a count that overflows")
        return g.value, f.value, r.value

    def share_group_batch_scale(self, group: int, lpp: int, parties: int, mac_shares, s_ptr, s_inf_ptr, o_ptr, tx_ptr, tx_inf_ptr, ty_ptr, tz_ptr, tz_inf_ptr,
                                out_ptr, out_inf_ptr, n: int):
        """czk_share_group_batch_scale: point vectors (s, tx, tz, out) are lpp * parties device lanes of n affine points + as many infinity bytes (an input's
        may be None), scalar vectors (o, ty) as many lanes of n Montgomery Fr; mac_shares (parties, 4) Montgomery limbs (None for lpp = 1).
        Points are assumed to lie in the prime-order subgroup.  Returns the number of elements whose MAC checks failed."""
        ms = None if mac_shares is None else np.ascontiguousarray(mac_shares, np.uint64).reshape(-1, 4)
        assert ms is None or ms.shape[0] >= parties
        bad = C.c_uint64(0)
        self._ck(self._L.czk_share_group_batch_scale(self._h, C.c_int(group), C.c_size_t(lpp), C.c_size_t(parties), _ptr(ms), _ptr(s_ptr), _ptr(s_inf_ptr), _ptr(o_ptr),
                                                   _ptr(tx_ptr), _ptr(tx_inf_ptr), _ptr(ty_ptr), _ptr(tz_ptr), _ptr(tz_inf_ptr), _ptr(out_ptr), _ptr(out_inf_ptr),
                                                   C.c_size_t(n), C.byref(bad)))
        return bad.value

    def gsz_group_batch_mul(self, group: int, parties: int, degree: int, x_ptr, y_ptr, y_inf_ptr, gr_ptr, gr_inf_ptr, gr2_ptr, gr2_inf_ptr, out_ptr, out_inf_ptr,
                            n: int):
        """czk_gsz_group_batch_mul: x `parties` device lanes of n Montgomery Fr; y, gr, gr2, out as many lanes of n affine points + infinity bytes (an
        input's may be None).  Returns the number of elements that exceeded the king's degree bound."""
        bad = C.c_uint64(0)
        self._ck(self._L.czk_gsz_group_batch_mul(self._h, C.c_int(group), C.c_size_t(parties), C.c_uint(degree), _ptr(x_ptr), _ptr(y_ptr), _ptr(y_inf_ptr), _ptr(gr_ptr),
                                               _ptr(gr_inf_ptr), _ptr(gr2_ptr), _ptr(gr2_inf_ptr), _ptr(out_ptr), _ptr(out_inf_ptr), C.c_size_t(n), C.byref(bad)))
        return bad.value

    def gsz_group_product_check(self, group: int, parties: int, degree: int, xs_ptr, ys_ptr, ys_inf_ptr, zs_ptr, zs_inf_ptr, n: int, gr_ptr, gr_inf_ptr, gr2_ptr,
                                gr2_inf_ptr, fr_ptr, fr2_ptr, rands_ptr):
        """czk_gsz_group_product_check over n triples (xs scalars, ys and zs points) -> (ok, degree violations); ok = False is a result, not an error.
        gr / gr2: group doubles, fr / fr2: field doubles, rands: random shares, as gsz_group_material_counts(CZK_GSZ_GROUP_OP_PRODUCT_CHECK, n) counts them."""
        ok, bad = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.czk_gsz_group_product_check(self._h, C.c_int(group), C.c_size_t(parties), C.c_uint(degree), _ptr(xs_ptr), _ptr(ys_ptr), _ptr(ys_inf_ptr),
                                                   _ptr(zs_ptr), _ptr(zs_inf_ptr), C.c_size_t(n), _ptr(gr_ptr), _ptr(gr_inf_ptr), _ptr(gr2_ptr), _ptr(gr2_inf_ptr),
                                                   _ptr(fr_ptr), _ptr(fr2_ptr), _ptr(rands_ptr), C.byref(ok), C.byref(bad)))
        return bool(ok.value), bad.value

    # ---- pairings of shared points and multiplicative target-group shares on device lanes (czk.h; csrc/pairing_share.hip) -----------------------
    @staticmethod
    def _mac_limbs(mac_shares, parties):
        ms = None if mac_shares is None else np.ascontiguousarray(mac_shares, np.uint64).reshape(-1, 4)
        assert ms is None or ms.shape[0] >= parties
        return ms

    def share_pairing(self, lpp: int, parties: int, mac_shares, a_ptr, a_inf_ptr, b_ptr, b_inf_ptr, tx_ptr, tx_inf_ptr, ty_ptr, ty_inf_ptr, tz_ptr, out_ptr, n: int):
        """czk_share_pairing: a, tx are lpp * parties device lanes of n affine G1 points, b, ty of G2 points (+ as many infinity bytes each, or None), tz and
        out as many lanes of n Fq12 (72 u64); mac_shares (parties, 4) Montgomery limbs (None for lpp = 1).  Points are assumed to lie in the prime-order
        subgroups.  Returns the number of elements whose MAC checks failed."""
        bad = C.c_uint64(0)
        self._ck(self._L.czk_share_pairing(self._h, C.c_size_t(lpp), C.c_size_t(parties), _ptr(self._mac_limbs(mac_shares, parties)), _ptr(a_ptr), _ptr(a_inf_ptr),
                                         _ptr(b_ptr), _ptr(b_inf_ptr), _ptr(tx_ptr), _ptr(tx_inf_ptr), _ptr(ty_ptr), _ptr(ty_inf_ptr), _ptr(tz_ptr), _ptr(out_ptr),
                                         C.c_size_t(n), C.byref(bad)))
        return bad.value

    def gt_share_open(self, lpp: int, parties: int, mac_shares, v_ptr, n: int, out_ptr):
        """czk_gt_share_open: out (n x 72, device) = the product of the sh lanes of v -> the number of elements whose MAC check failed"""
        bad = C.c_uint64(0)
        self._ck(self._L.czk_gt_share_open(self._h, C.c_size_t(lpp), C.c_size_t(parties), _ptr(self._mac_limbs(mac_shares, parties)), _ptr(v_ptr), C.c_size_t(n),
                                         _ptr(out_ptr), C.byref(bad)))
        return bad.value

    def gt_share_scale(self, lpp: int, parties: int, mac_shares, v_ptr, f_ptr, out_ptr, n: int):
        """czk_gt_share_scale: out = the lanes v scaled by the public f (n x 72, device); v_ptr None: from_public(f).  Only enqueues."""
        self._ck(self._L.czk_gt_share_scale(self._h, C.c_size_t(lpp), C.c_size_t(parties), _ptr(self._mac_limbs(mac_shares, parties)), _ptr(v_ptr), _ptr(f_ptr),
                                          _ptr(out_ptr), C.c_size_t(n)))

    def fq12_vec_op(self, op: int, a, b=None, n=None, out=None, mem: int = CZK_MEM_HOST):
        """czk_fq12_vec_op: elementwise CZK_FQ12_OP_MUL / _DIV / _INV on n Fq12 (the inverse of zero is zero).  Host mode takes (n, 72) uint64 arrays and
        returns one; in device mode a, b, out are device pointers and n the count."""
        if mem == CZK_MEM_HOST:
            a = np.ascontiguousarray(a, np.uint64).reshape(-1, 72)
            n = a.shape[0]
            b = None if b is None else np.ascontiguousarray(b, np.uint64).reshape(n, 72)
            out = np.zeros((n, 72), dtype=np.uint64)
        z = lambda x: x if n else None   # noqa: E731
        self._ck(self._L.czk_fq12_vec_op(self._h, C.c_int(op), _ptr(z(a)), _ptr(z(b)), _ptr(z(out)), C.c_size_t(n), C.c_int(mem)))
        return out

    # ---- the GSZ material made on the device (czk.h; csrc/gsz_dn.hip) -----------------------------------------------------------------------
    def fr_random(self, key: bytes, nonce: bytes, first: int, n: int, out=None, mem=CZK_MEM_HOST):
        """czk_fr_random: element i = the ChaCha20 block at (key, nonce, first + i) as a field element -> (n, 4) uint64 Montgomery (host), or `out` (a pointer in `mem`)"""
        k, nc = _key_bytes(key, 32), _key_bytes(nonce, 12)
        if mem == CZK_MEM_HOST and out is None:
            out = np.zeros((n, 4), dtype=np.uint64)
        self._ck(self._L.czk_fr_random(self._h, k, nc, C.c_uint32(first), C.c_size_t(n), _ptr(out if n else None), C.c_int(mem)))
        return out

    def gsz_dn_counts(self, kind: int, parties: int, degree: int, want: int):
        """(deal, outputs): the smallest deal whose deal (parties - degree) outputs reach `want`"""
        return _gsz_dn_counts(self._L, kind, parties, degree, want)

    def gsz_dn_generate(self, kind: int, parties: int, degree: int, keys, nonce: bytes, deal: int, out_r_ptr, out_r2_ptr=None):
        """czk_gsz_dn_generate: keys = `parties` x 32 bytes; out_r / out_r2: `parties` device lanes of deal (parties - degree) elements.  Enqueues."""
        kb = _key_bytes(b"".join(bytes(k) for k in keys) if not isinstance(keys, (bytes, bytearray)) else keys, 32 * parties)
        self._ck(self._L.czk_gsz_dn_generate(self._h, C.c_int(kind), C.c_size_t(parties), C.c_uint(degree), kb, _key_bytes(nonce, 12), C.c_size_t(deal), _ptr(out_r_ptr),
                                             _ptr(out_r2_ptr)))

    def gsz_dn_check(self, kind: int, parties: int, degree: int, r_ptr, r2_ptr, outputs: int):
        """czk_gsz_dn_check -> (ok, opens over their bound); ok = False is a result, not an error.  The last two outputs are sacrificed."""
        ok, bad = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.czk_gsz_dn_check(self._h, C.c_int(kind), C.c_size_t(parties), C.c_uint(degree), _ptr(r_ptr), _ptr(r2_ptr), C.c_size_t(outputs), C.byref(ok),
                                          C.byref(bad)))
        return bool(ok.value), bad.value

    def share_domain_constants(self, parties: int):
        out = np.zeros((3, 4), dtype=np.uint64)
        self._ck(self._L.czk_share_domain_constants(self._h, C.c_size_t(parties), _ptr(out)))
        return dict(zip(["size_inv", "group_gen", "group_gen_inv"], out))

    def fr_gsz_open(self, shares_ptr, parties: int, n: int, out_value_ptr, degree: int = 0, degrees_ptr=None) -> int:
        """Local part of GszFieldShare::batch_open on device buffers; returns the number of degree-bound violations."""
        bad = C.c_uint64(0)
        self._ck(self._L.czk_fr_gsz_open(self._h, _ptr(shares_ptr), C.c_size_t(parties), C.c_size_t(n), _ptr(degrees_ptr), C.c_uint(degree),
                                       _ptr(out_value_ptr), C.byref(bad)))
        return bad.value

    def r1cs_matrix_register(self, row_ptr, col_idx, coeff, n_vars: int, mem=CZK_MEM_HOST, m=None, nnz=None) -> "R1csMatrix":
        """One of ConstraintMatrices::{a, b, c} in CSR form (host numpy arrays, or device pointers with m / nnz given)."""
        if mem == CZK_MEM_HOST:
            row_ptr = np.ascontiguousarray(row_ptr, np.uint64)
            col_idx = np.ascontiguousarray(col_idx, np.uint32)
            coeff = np.ascontiguousarray(coeff, np.uint64)
            m, nnz = row_ptr.size - 1, col_idx.size
        h = C.c_void_p(0)
        self._ck(self._L.czk_r1cs_matrix_register(self._h, _ptr(row_ptr), _ptr(col_idx), _ptr(coeff), C.c_size_t(m), C.c_size_t(nnz),
                                                C.c_size_t(n_vars), C.c_int(mem), C.byref(h)))
        return R1csMatrix(self, h, m, n_vars)

    def r1cs_matvec(self, mat: "R1csMatrix", z, lanes: int = 1, out=None, z_stride=None, out_stride=None, mem=CZK_MEM_HOST):
        """evaluate_constraint over every row and lane; host mode returns (lanes, m, 4)."""
        if mem == CZK_MEM_HOST:
            z = np.ascontiguousarray(z, np.uint64).reshape(lanes, -1, 4)
            z_stride = z.shape[1]
            out_stride = mat.m
            out = np.zeros((lanes, mat.m, 4), dtype=np.uint64)
        self._ck(self._L.czk_r1cs_matvec(self._h, mat._h, _ptr(z), C.c_size_t(z_stride), C.c_size_t(lanes), _ptr(out), C.c_size_t(out_stride), C.c_int(mem)))
        return out

    def marlin_arithmetize(self, row_ptr, col_idx, coeff, log_h: int, log_x: int, n_instance: int, k: int, out=None, mem=CZK_MEM_HOST, m=None, nnz=None):
        """arithmetize_matrix for one CSR matrix up to the evaluations on K (czk_marlin_arithmetize); host mode takes numpy arrays and returns
        (4, k, 4): row, col, val, row_col.  Device mode: pointers, with m / nnz given and `out` a device buffer of 4 k Fr."""
        if mem == CZK_MEM_HOST:
            row_ptr = np.ascontiguousarray(row_ptr, np.uint64)
            col_idx = np.ascontiguousarray(col_idx, np.uint32)
            coeff = np.ascontiguousarray(coeff, np.uint64)
            m, nnz = row_ptr.size - 1, col_idx.size
            out = np.zeros((4, k, 4), dtype=np.uint64)
        self._ck(self._L.czk_marlin_arithmetize(self._h, _ptr(row_ptr), _ptr(col_idx if nnz else None), _ptr(coeff if nnz else None), C.c_size_t(m),
                                              C.c_size_t(nnz), C.c_uint(log_h), C.c_uint(log_x), C.c_size_t(n_instance), C.c_size_t(k),
                                              _ptr(out if k else None), C.c_int(mem)))
        return out

    def plonk_layout(self, succ, n_gates: int, n_prods: int, w_evals=None, s_evals=None, mem=CZK_MEM_HOST):
        """CircuitLayout::from_circuit up to the evaluations of the two index polynomials (czk_plonk_layout): w_evals[i] = w^succ[i] over the 3 n_gates
        wire slots, s_evals = n_prods zeros then ones.  Host mode takes succ as a numpy array (checked to be a permutation) and returns (w_evals
        (3 n_gates, 4), s_evals (n_gates, 4)); device mode: pointers, with w_evals / s_evals device buffers."""
        if mem == CZK_MEM_HOST:
            succ = np.ascontiguousarray(succ, np.uint32).reshape(-1)
            sized = n_gates > 0 and not n_gates & (n_gates - 1) and 3 * n_gates < 1 << 32    # otherwise the library refuses before it reads or writes
            if sized and succ.size != 3 * n_gates:
                raise ValueError("succ must hold 3 n_gates slot indices")
            w_evals = np.zeros((3 * n_gates if sized else 1, 4), dtype=np.uint64)
            s_evals = np.zeros((n_gates if sized else 1, 4), dtype=np.uint64)
        self._ck(self._L.czk_plonk_layout(self._h, _ptr(succ), C.c_size_t(n_gates), C.c_size_t(n_prods), _ptr(w_evals), _ptr(s_evals), C.c_int(mem)))
        return w_evals, s_evals

    def fr_gather(self, src, index, lanes: int = 1, src_len=None, src_stride=None, n=None, out=None, out_stride=None, mem=CZK_MEM_HOST):
        """out[l][i] = src[l][index[i]] on every lane (czk_fr_gather).  Host mode: src (lanes, src_stride, 4) and index as numpy arrays, src_len
        (default src_stride) valid elements per lane, `out` an optional (lanes, out_stride, 4) array whose elements past n stay; returns out.  Device
        mode: pointers with src_len, src_stride, n and out_stride given."""
        if mem == CZK_MEM_HOST:
            src = np.ascontiguousarray(src, np.uint64).reshape(lanes, -1, 4) if lanes else np.zeros((0, 0, 4), dtype=np.uint64)
            index = np.ascontiguousarray(index, np.uint32).reshape(-1)
            src_stride, n = src.shape[1], index.size
            src_len = src_stride if src_len is None else src_len
            assert src_len <= src_stride
            if out is None:
                out = np.zeros((lanes, n, 4), dtype=np.uint64)
            assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape[0] == lanes and (not lanes or out.shape[1] >= n)
            out_stride = out.shape[1] if lanes else n
        self._ck(self._L.czk_fr_gather(self._h, _ptr(src if lanes and n else None), C.c_size_t(src_len), C.c_size_t(src_stride), C.c_size_t(lanes),
                                     _ptr(index if lanes and n else None), C.c_size_t(n), _ptr(out if lanes and n else None), C.c_size_t(out_stride), C.c_int(mem)))
        return out

    # ---- the reference's Merkle commitment of share vectors (com.rs ComField) and the FRI fold ------------------------------------
    def fr_merkle_commit(self, a, lanes: int = 1, n=None, stride=None, tree=None, tree_stride=None, roots=True, mem=CZK_MEM_HOST):
        """czk_fr_merkle_commit: every lane's binary SHA-256 tree over n Montgomery Fr.  Host mode: a is (lanes, stride, 4) limbs of which n (default
        stride) per lane are hashed, `tree` an optional (lanes, tree_stride, 32) uint8 array whose digests past 2n - 1 stay; returns (tree, roots) with
        roots (lanes, 32) uint8.  Device mode: pointers with n, stride and tree_stride given; returns (tree, roots), roots None -- and the call only
        enqueued -- with roots=False."""
        if mem == CZK_MEM_HOST:
            a = np.ascontiguousarray(a, np.uint64).reshape(lanes, -1, 4) if lanes else np.zeros((0, 0, 4), dtype=np.uint64)
            stride = a.shape[1] if lanes else (n or 0)
            n = stride if n is None else n
            if tree is None:
                tree = np.zeros((lanes, max(2 * n - 1, 0), 32), dtype=np.uint8)
            assert tree.dtype == np.uint8 and tree.flags.c_contiguous and tree.shape[0] == lanes
            tree_stride = tree.shape[1] if tree_stride is None else tree_stride
        out = np.zeros((lanes, 32), dtype=np.uint8) if roots else None
        live = lanes and n and not n & (n - 1)     # otherwise the library returns before it reads a pointer
        self._ck(self._L.czk_fr_merkle_commit(self._h, _ptr(a if live else None), C.c_size_t(lanes), C.c_size_t(n), C.c_size_t(stride),
                                              _ptr(tree if live else None), C.c_size_t(tree_stride), _ptr(out if roots and lanes else None), C.c_int(mem)))
        return tree, out

    def fr_merkle_open(self, a, tree, idx, lanes: int = 1, n=None, stride=None, tree_stride=None, q=None, out_shares=None, out_paths=None,
                       mem=CZK_MEM_HOST):
        """czk_fr_merkle_open: shares (q, lanes, 4) and sibling paths (q, lanes, log2 n, 32) at the q indices.  Host mode: a (lanes, stride, 4), tree
        (lanes, tree_stride, 32) and idx as numpy arrays (n defaults to stride); returns (shares, paths).  Device mode: pointers and every size given."""
        if mem == CZK_MEM_HOST:
            a = np.ascontiguousarray(a, np.uint64).reshape(lanes, -1, 4) if lanes else np.zeros((0, 0, 4), dtype=np.uint64)
            tree = np.ascontiguousarray(tree, np.uint8).reshape(lanes, -1, 32) if lanes else np.zeros((0, 0, 32), dtype=np.uint8)
            idx = np.ascontiguousarray(idx, np.uint64).reshape(-1)
            stride, q = a.shape[1] if lanes else (n or 0), idx.size
            n = stride if n is None else n
            tree_stride = (tree.shape[1] if lanes else max(2 * n - 1, 0)) if tree_stride is None else tree_stride
            log_n = max(n.bit_length() - 1, 0)
            out_shares = np.zeros((q, lanes, 4), dtype=np.uint64)
            out_paths = np.zeros((q, lanes, log_n, 32), dtype=np.uint8)
        live = lanes and q
        nonempty = lambda x: None if x is None or (isinstance(x, np.ndarray) and x.size == 0) else x   # noqa: E731
        self._ck(self._L.czk_fr_merkle_open(self._h, _ptr(nonempty(a) if live else None), C.c_size_t(lanes), C.c_size_t(n), C.c_size_t(stride),
                                            _ptr(nonempty(tree) if live else None), C.c_size_t(tree_stride), _ptr(idx if live else None), C.c_size_t(q),
                                            _ptr(nonempty(out_shares)), _ptr(nonempty(out_paths)), C.c_int(mem)))
        return out_shares, out_paths

    def fr_merkle_verify(self, roots, idx, shares, paths, n: int, values=None, lanes=None, q=None, ok=None, mem=CZK_MEM_HOST):
        """czk_fr_merkle_verify: (ok, bad) with ok[query] = 1 when every lane's share hashes up its path to the lane's root and, with `values`, the
        lanes' shares sum to values[query]; bad = the number of zeros.  Host mode: roots (lanes, 32), idx (q,), shares (q, lanes, 4), paths (q, lanes,
        log2 n, 32), values (q, 4) as numpy arrays, ok returned as a (q,) uint8 array.  Device mode: pointers, with lanes, q and an `ok` buffer given."""
        if mem == CZK_MEM_HOST:
            roots = np.ascontiguousarray(roots, np.uint8).reshape(-1, 32)
            idx = np.ascontiguousarray(idx, np.uint64).reshape(-1)
            lanes, q = roots.shape[0], idx.size
            shares = np.ascontiguousarray(shares, np.uint64)
            paths = np.ascontiguousarray(paths, np.uint8)
            log_n = max(n.bit_length() - 1, 0)
            if shares.size != q * lanes * 4 or paths.size != q * lanes * log_n * 32:
                raise ValueError("shares must hold q x lanes elements and paths q x lanes x log2(n) digests")
            if values is not None:
                values = np.ascontiguousarray(values, np.uint64)
                if values.size != 4 * q:
                    raise ValueError("values must hold q elements")
            ok = np.zeros(q, dtype=np.uint8)
        bad = C.c_size_t(0)
        nonempty = lambda x: None if x is None or (isinstance(x, np.ndarray) and x.size == 0) else x   # noqa: E731
        self._ck(self._L.czk_fr_merkle_verify(self._h, _ptr(nonempty(roots)), C.c_size_t(lanes), C.c_size_t(n), _ptr(nonempty(idx)), C.c_size_t(q),
                                              _ptr(nonempty(shares)), _ptr(nonempty(paths)), _ptr(nonempty(values)), _ptr(nonempty(ok)), C.byref(bad),
                                              C.c_int(mem)))
        return ok, bad.value

    def fri_fold(self, f, alpha, lanes: int = 1, n=None, stride=None, out=None, out_stride=None, mem=CZK_MEM_HOST):
        """czk_fr_fri_fold: out[l][j] = f[l][2j] + alpha f[l][2j+1], j < n / 2; alpha (4,) Montgomery limbs on the host.  Host mode: f (lanes, stride, 4)
        (n defaults to stride), `out` an optional (lanes, out_stride, 4) array whose elements past n / 2 stay; returns out.  Device mode: pointers."""
        alpha = np.ascontiguousarray(alpha, np.uint64).reshape(4)
        if mem == CZK_MEM_HOST:
            f = np.ascontiguousarray(f, np.uint64).reshape(lanes, -1, 4) if lanes else np.zeros((0, 0, 4), dtype=np.uint64)
            stride = f.shape[1] if lanes else (n or 0)
            n = stride if n is None else n
            if out is None:
                out = np.zeros((lanes, n // 2, 4), dtype=np.uint64)
            assert out.dtype == np.uint64 and out.flags.c_contiguous and out.shape[0] == lanes
            out_stride = out.shape[1] if lanes else n // 2
        live = lanes and n >= 2
        self._ck(self._L.czk_fr_fri_fold(self._h, _ptr(f if live else None), C.c_size_t(lanes), C.c_size_t(n), C.c_size_t(stride), _ptr(alpha),
                                         _ptr(out if live else None), C.c_size_t(out_stride), C.c_int(mem)))
        return out

    def fri_fold_at(self, f: int, alpha_dev: int, lanes: int, n: int, stride: int, out: int, out_stride: int):
        """czk_fr_fri_fold_at: czk_fr_fri_fold on device pointers with alpha read from device memory (one Montgomery Fr at alpha_dev); only enqueues."""
        self._ck(self._L.czk_fr_fri_fold_at(self._h, _ptr(f), C.c_size_t(lanes), C.c_size_t(n), C.c_size_t(stride), _ptr(alpha_dev), _ptr(out), C.c_size_t(out_stride)))

    def fs_create(self, device: bool = True) -> "Fs":
        """czk_fs_create on this context: a Fiat-Shamir transcript whose state lives in device memory (every operation a kernel on the context's stream),
        or, with device=False, in host memory."""
        return Fs(self, device)

    def poly_div_linear(self, coeffs, z, lanes: int = 1, n=None, quotient=None, remainder=None, mem=CZK_MEM_HOST):
        """coeffs / (X - z) per lane; host mode returns (quotient (lanes, n-1, 4), remainder (lanes, 4))."""
        z = np.ascontiguousarray(z, np.uint64).reshape(4)
        if mem == CZK_MEM_HOST:
            coeffs = np.ascontiguousarray(coeffs, np.uint64).reshape(lanes, -1, 4)
            n = coeffs.shape[1]
            quotient = np.zeros((lanes, max(n - 1, 0), 4), dtype=np.uint64)
            remainder = np.zeros((lanes, 4), dtype=np.uint64)
        qp = quotient if not (isinstance(quotient, np.ndarray) and quotient.size == 0) else None
        cp = coeffs if not (isinstance(coeffs, np.ndarray) and coeffs.size == 0) else None
        self._ck(self._L.czk_poly_div_linear(self._h, _ptr(cp), C.c_size_t(n), C.c_size_t(lanes), _ptr(z), _ptr(qp), _ptr(remainder), C.c_int(mem)))
        return quotient, remainder

    def poly_div_vanishing(self, coeffs, n: int, lanes: int = 1, m=None, quotient=None, remainder=None, mem=CZK_MEM_HOST):
        """coeffs = q (X^n - 1) + r per lane (czk_poly_div_vanishing); host mode returns (q (lanes, m - n, 4), r (lanes, n, 4))."""
        if mem == CZK_MEM_HOST:
            coeffs = np.ascontiguousarray(coeffs, np.uint64).reshape(lanes, -1, 4)
            m = coeffs.shape[1]
            quotient = np.zeros((lanes, max(m - n, 0), 4), dtype=np.uint64)
            remainder = np.zeros((lanes, n, 4), dtype=np.uint64)
        qp = quotient if not (isinstance(quotient, np.ndarray) and quotient.size == 0) else None
        self._ck(self._L.czk_poly_div_vanishing(self._h, _ptr(coeffs), C.c_size_t(m), C.c_size_t(lanes), C.c_size_t(n), _ptr(qp), _ptr(remainder), C.c_int(mem)))
        return quotient, remainder

    def poly_evaluate(self, coeffs, z, lanes: int = 1, n=None, values=None, mem=CZK_MEM_HOST):
        """p(z) per lane (czk_poly_evaluate); host mode returns (lanes, 4)."""
        z = np.ascontiguousarray(z, np.uint64).reshape(4)
        if mem == CZK_MEM_HOST:
            coeffs = np.ascontiguousarray(coeffs, np.uint64).reshape(lanes, -1, 4)
            n = coeffs.shape[1]
            values = np.zeros((lanes, 4), dtype=np.uint64)
        cp = coeffs if not (isinstance(coeffs, np.ndarray) and coeffs.size == 0) else None
        self._ck(self._L.czk_poly_evaluate(self._h, _ptr(cp), C.c_size_t(n), C.c_size_t(lanes), _ptr(z), _ptr(values), C.c_int(mem)))
        return values

    def poly_evaluate_many(self, ptrs, ns, lanes, zs, value_ptrs):
        """czk_poly_evaluate_many on DEVICE pointers: polynomial k = ns[k] coefficients x lanes[k] lanes at ptrs[k], evaluated at zs[k] (Montgomery limbs),
        its values written to value_ptrs[k]."""
        k = len(ptrs)
        src = (C.c_void_p * k)(*[int(p) for p in ptrs])
        dst = (C.c_void_p * k)(*[int(p) for p in value_ptrs])
        n = (C.c_size_t * k)(*[int(x) for x in ns])
        ln = (C.c_size_t * k)(*[int(x) for x in lanes])
        z = np.ascontiguousarray(np.stack([np.asarray(x, np.uint64).reshape(4) for x in zs]) if k else np.zeros((0, 4), np.uint64))
        self._ck(self._L.czk_poly_evaluate_many(self._h, C.c_size_t(k), src, n, ln, _ptr(z if k else None), dst))

    def fr_lincomb(self, ptrs, lens, term_lanes, coeffs, lanes: int, lift_mask: int, out_ptr, out_len: int, constant=None):
        """czk_fr_lincomb on DEVICE pointers: out[l][i] = constant + sum_k coeffs[k] * term_k[l][i]; a term with one lane -- and the constant -- is public
        (added on the lanes of lift_mask)."""
        k = len(ptrs)
        src = (C.c_void_p * k)(*[int(p) for p in ptrs])
        n = (C.c_size_t * k)(*[int(x) for x in lens])
        tl = (C.c_size_t * k)(*[int(x) for x in term_lanes])
        c = np.ascontiguousarray(np.stack([np.asarray(x, np.uint64).reshape(4) for x in coeffs]) if k else np.zeros((0, 4), np.uint64))
        cst = None if constant is None else np.ascontiguousarray(constant, np.uint64).reshape(4)
        self._ck(self._L.czk_fr_lincomb(self._h, C.c_size_t(k), src, n, tl, _ptr(c if k else None), _ptr(cst), C.c_size_t(lanes), C.c_uint64(lift_mask), _ptr(out_ptr), C.c_size_t(out_len)))

    def fr_prefix_product(self, x, out=None, n=None, mem=CZK_MEM_HOST):
        """Running products of a public Fr vector (partial_products' local loop)."""
        if mem == CZK_MEM_HOST:
            x = np.ascontiguousarray(x, np.uint64).reshape(-1, 4)
            n = x.shape[0]
            out = np.zeros_like(x)
        self._ck(self._L.czk_fr_prefix_product(self._h, _ptr(x if n else None), C.c_size_t(n), _ptr(out if n else None), C.c_int(mem)))
        return out

    def fr_batch_inverse(self, v, coeff=None, out=None, n=None, mem=CZK_MEM_HOST):
        """batch_inversion_and_mul: out[i] = coeff / v[i] (zeros stay zero)."""
        if mem == CZK_MEM_HOST:
            v = np.ascontiguousarray(v, np.uint64).reshape(-1, 4)
            n = v.shape[0]
            out = np.zeros_like(v)
        if coeff is not None:
            coeff = np.ascontiguousarray(coeff, np.uint64).reshape(4)
        self._ck(self._L.czk_fr_batch_inverse(self._h, _ptr(v if n else None), C.c_size_t(n), _ptr(coeff), _ptr(out if n else None), C.c_int(mem)))
        return out

    def fixed_base_points(self, group, k, out=None, n=None, mem=CZK_MEM_HOST):
        aw = 12 if group == CZK_G1 else 24
        if mem == CZK_MEM_HOST:
            k = np.ascontiguousarray(k, np.uint64)
            n = k.size // 4
            out = np.zeros((n, aw), dtype=np.uint64)
        self._ck(self._L.czk_fixed_base_points(self._h, C.c_int(group), _ptr(k), C.c_size_t(n), _ptr(out), C.c_int(mem)))
        return out

    # ---- fixed-base MSM and the generator's helpers (czk_fixed_base_*, czk_fr_lagrange_coefficients) ----
    def fixed_base(self, group: int, base, window: int = 0, n_hint: int = 0) -> "FixedBase":
        """FixedBaseMSM::get_window_table for one finite affine base ((12|24,) uint64 Montgomery, host); window 0: chosen for n_hint scalars."""
        if base is not None:
            base = np.ascontiguousarray(base, np.uint64).reshape(12 if group == CZK_G1 else 24)
        h = C.c_void_p(0)
        self._ck(self._L.czk_fixed_base_create(self._h, C.c_int(group), _ptr(base), C.c_uint(window), C.c_size_t(n_hint), C.byref(h)))
        return FixedBase(self, h, group)

    def fixed_base_msm(self, fb: "FixedBase", k, out=None, n=None, scalar_form: int = CZK_SCALAR_CANONICAL, mem: int = CZK_MEM_HOST, out_inf=None):
        """FixedBaseMSM::multi_scalar_mul + normalisation: returns (points (n, 12|24), infinity flags (n,)).  Host mode allocates both; in device
        mode `k`, `out` and `out_inf` (may be None) are device pointers, `n` the count, and the same pair is returned."""
        aw = 12 if fb.group == CZK_G1 else 24
        if mem == CZK_MEM_HOST:
            k = np.ascontiguousarray(k, np.uint64).reshape(-1, 4)
            n = k.shape[0]
            out = np.zeros((n, aw), dtype=np.uint64)
            out_inf = np.zeros(n, dtype=np.uint8)
        self._ck(self._L.czk_fixed_base_msm(self._h, fb._h, _ptr(k if n else None), C.c_size_t(n), C.c_int(scalar_form), _ptr(out if n else None),
                                            _ptr(out_inf if n else None), C.c_int(mem)))
        return out, out_inf

    def fr_lagrange_coefficients(self, log_d: int, tau, n_out: int | None = None, out=None, mem: int = CZK_MEM_HOST):
        """evaluate_all_lagrange_coefficients: L_j(tau) for j < n_out (default 2^log_d); tau: (4,) uint64 Montgomery, host."""
        tau = np.ascontiguousarray(tau, np.uint64).reshape(4)
        if n_out is None:
            n_out = 1 << log_d
        if mem == CZK_MEM_HOST:
            out = np.zeros((n_out, 4), dtype=np.uint64)
        self._ck(self._L.czk_fr_lagrange_coefficients(self._h, C.c_uint(log_d), _ptr(tau), _ptr(out if n_out else None), C.c_size_t(n_out), C.c_int(mem)))
        return out

    # ---- square roots and the reference's point encoding (czk_fq_sqrt, czk_points_*) ---------------------
    def fq_sqrt(self, a, ext: int = 1, out=None, out_exists=None, n=None, mem: int = CZK_MEM_HOST):
        """Square roots in Fq (ext = 1, (n, 6)) or Fq2 (ext = 2, (n, 12)), Montgomery limbs: returns (roots, exists flags); the root is the one with
        y <= -y, zero where none exists.  Host mode allocates both; in device mode `a`, `out`, `out_exists` are device pointers and `n` the count."""
        fw = 6 * ext
        if mem == CZK_MEM_HOST:
            a = np.ascontiguousarray(a, np.uint64).reshape(-1, fw)
            n = a.shape[0]
            out = np.zeros((n, fw), dtype=np.uint64)
            out_exists = np.zeros(n, dtype=np.uint8)
        self._ck(self._L.czk_fq_sqrt(self._h, C.c_int(ext), _ptr(a if n else None), C.c_size_t(n), _ptr(out if n else None),
                                     _ptr(out_exists if n else None), C.c_int(mem)))
        return out, out_exists

    def points_serialize(self, group: int, pts, inf=None, compressed: bool = True, n=None, out=None, mem: int = CZK_MEM_HOST):
        """GroupAffine::serialize / serialize_uncompressed of n affine Montgomery points ((n, 12|24)) with optional infinity flags: host mode returns
        the bytes as a uint8 array; in device mode `pts`, `inf` (may be None) and `out` are device pointers, `n` the count, and `out` is returned."""
        aw = 12 if group == CZK_G1 else 24
        if mem == CZK_MEM_HOST:
            pts = np.ascontiguousarray(pts, np.uint64).reshape(-1, aw)
            n = pts.shape[0]
            inf = None if inf is None else np.ascontiguousarray(inf, np.uint8).reshape(n)
            out = np.zeros(n * aw * (4 if compressed else 8), dtype=np.uint8)
        self._ck(self._L.czk_points_serialize(self._h, C.c_int(group), _ptr(pts if n else None), _ptr(inf if n else None), C.c_size_t(n),
                                              C.c_int(1 if compressed else 0), _ptr(out if n else None), C.c_int(mem)))
        return out

    def points_deserialize(self, group: int, data, n=None, compressed: bool = True, checked: bool = True, out=None, out_inf=None, out_status=None,
                           count: bool = True, mem: int = CZK_MEM_HOST):
        """GroupAffine::deserialize (compressed, checked), deserialize_uncompressed (checked), deserialize_unchecked (neither) of n points: returns
        (points (n, 12|24), infinity flags, czk_point_status bytes, number of failing points, first failing index or n).  Host mode takes bytes or a
        uint8 array and allocates the outputs; in device mode `data`, `out`, `out_inf`, `out_status` (may be None) are device pointers, and
        count=False returns None for the two counts and only enqueues."""
        aw = 12 if group == CZK_G1 else 24
        size = aw * (4 if compressed else 8)
        if mem == CZK_MEM_HOST:
            data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, np.uint8)
            if data.size % size:
                raise ValueError(f"{data.size} bytes are not a whole number of {size}-byte points")
            n = data.size // size
            out = np.zeros((n, aw), dtype=np.uint64)
            out_inf = np.zeros(n, dtype=np.uint8)
            out_status = np.zeros(n, dtype=np.uint8)
        flags = (CZK_POINTS_COMPRESSED if compressed else 0) | (CZK_POINTS_CHECKED if checked else 0)
        bad, first = C.c_size_t(0), C.c_size_t(n)
        self._ck(self._L.czk_points_deserialize(self._h, C.c_int(group), _ptr(data if n else None), C.c_size_t(n), C.c_int(flags), _ptr(out if n else None),
                                                _ptr(out_inf if n else None), _ptr(out_status if n else None), C.byref(bad) if count else None,
                                                C.byref(first) if count else None, C.c_int(mem)))
        return out, out_inf, out_status, (bad.value if count else None), (first.value if count else None)

    # ---- elementwise group arithmetic on arrays of points (czk_points_add / _mul / _sum) -------------------
    def points_add(self, group: int, a, b, a_inf=None, b_inf=None, negate_b: bool = False, n=None, out=None, out_inf=None, mem: int = CZK_MEM_HOST):
        """out[i] = a[i] + b[i] (a[i] - b[i] with negate_b) over affine Montgomery points ((n, 12|24)) with optional infinity flags, every exceptional
        case included: returns (points, infinity flags).  Host mode allocates both; in device mode every buffer is a device pointer and `n` the count."""
        aw = 12 if group == CZK_G1 else 24
        if mem == CZK_MEM_HOST:
            a = np.ascontiguousarray(a, np.uint64).reshape(-1, aw)
            n = a.shape[0]
            b = np.ascontiguousarray(b, np.uint64).reshape(n, aw)
            a_inf = None if a_inf is None else np.ascontiguousarray(a_inf, np.uint8).reshape(n)
            b_inf = None if b_inf is None else np.ascontiguousarray(b_inf, np.uint8).reshape(n)
            out = np.zeros((n, aw), dtype=np.uint64)
            out_inf = np.zeros(n, dtype=np.uint8)
        z = lambda x: x if n else None
        self._ck(self._L.czk_points_add(self._h, C.c_int(group), _ptr(z(a)), _ptr(z(a_inf)), _ptr(z(b)), _ptr(z(b_inf)), C.c_size_t(n),
                                        C.c_int(1 if negate_b else 0), _ptr(z(out)), _ptr(z(out_inf)), C.c_int(mem)))
        return out, out_inf

    def points_mul(self, group: int, pts, k, inf=None, stride: int = 1, scalar_form: int = CZK_SCALAR_CANONICAL, n=None, out=None, out_inf=None,
                   mem: int = CZK_MEM_HOST):
        """out[i] = [k_i] P_i, ProjectiveCurve::mul over all 256 bits of the scalar: returns (points, infinity flags).  stride=1: `pts` holds one point
        per scalar; stride=0: ONE point (and flag) for every scalar.  k: (n, 4) uint64 in `scalar_form`.  Device mode as for points_add."""
        aw = 12 if group == CZK_G1 else 24
        if mem == CZK_MEM_HOST:
            k = np.ascontiguousarray(k, np.uint64).reshape(-1, 4)
            n = k.shape[0]
            pts = np.ascontiguousarray(pts, np.uint64).reshape(n if stride else 1, aw)
            inf = None if inf is None else np.ascontiguousarray(inf, np.uint8).reshape(n if stride else 1)
            out = np.zeros((n, aw), dtype=np.uint64)
            out_inf = np.zeros(n, dtype=np.uint8)
        z = lambda x: x if n else None
        self._ck(self._L.czk_points_mul(self._h, C.c_int(group), _ptr(z(pts)), _ptr(z(inf)), C.c_size_t(stride), _ptr(z(k)), C.c_size_t(n),
                                        C.c_int(scalar_form), _ptr(z(out)), _ptr(z(out_inf)), C.c_int(mem)))
        return out, out_inf

    def points_sum(self, group: int, pts, offsets, inf=None, out=None, out_inf=None, mem: int = CZK_MEM_HOST):
        """Segmented sums: out[j] = sum of pts[offsets[j] .. offsets[j+1]) for the k = len(offsets) - 1 segments (an empty one is infinity): returns
        (points (k, 12|24), infinity flags).  offsets are host values in either mode.  Device mode as for points_add."""
        aw = 12 if group == CZK_G1 else 24
        offs = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
        k = max(offs.size - 1, 0)
        if mem == CZK_MEM_HOST:
            pts = np.ascontiguousarray(pts, np.uint64).reshape(-1, aw)
            if k and int(offs[-1]) > pts.shape[0]:
                raise ValueError("offsets reach beyond the points")
            inf = None if inf is None else np.ascontiguousarray(inf, np.uint8).reshape(pts.shape[0])
            out = np.zeros((k, aw), dtype=np.uint64)
            out_inf = np.zeros(k, dtype=np.uint8)
        z = lambda x: x if k else None
        self._ck(self._L.czk_points_sum(self._h, C.c_int(group), _ptr(z(pts)), _ptr(z(inf)), _ptr(z(offs)), C.c_size_t(k), _ptr(z(out)), _ptr(z(out_inf)),
                                        C.c_int(mem)))
        return out, out_inf

    # ---- KZG10 verification (czk_kzg10_*) -----------------------------------------------------------
    def kzg10_vk(self, g, gamma_g, h, beta_h) -> "Kzg10VerifierKey":
        """VerifierKey (g, gamma_g: (12,), h, beta_h: (24,) uint64 affine Montgomery, finite) in HBM: a Kzg10VerifierKey handle."""
        g, gamma_g = (np.ascontiguousarray(x, np.uint64).reshape(12) for x in (g, gamma_g))
        h, beta_h = (np.ascontiguousarray(x, np.uint64).reshape(24) for x in (h, beta_h))
        hd = C.c_void_p()
        self._ck(self._L.czk_kzg10_vk_create(self._h, _ptr(g), _ptr(gamma_g), _ptr(h), _ptr(beta_h), C.byref(hd)))
        return Kzg10VerifierKey(self, hd, g.copy(), gamma_g.copy(), h.copy(), beta_h.copy())

    @staticmethod
    def _kzg_openings(comm, points, values, w, comm_inf, w_inf, random_v):
        comm = np.ascontiguousarray(comm, np.uint64).reshape(-1, 12)
        k = comm.shape[0]
        points, values = (np.ascontiguousarray(x, np.uint64).reshape(k, 4) for x in (points, values))
        w = np.ascontiguousarray(w, np.uint64).reshape(k, 12)
        comm_inf = None if comm_inf is None else np.ascontiguousarray(comm_inf, np.uint8).reshape(k)
        w_inf = None if w_inf is None else np.ascontiguousarray(w_inf, np.uint8).reshape(k)
        random_v = None if random_v is None else np.ascontiguousarray(random_v, np.uint64).reshape(k, 4)
        return k, comm, comm_inf, points, values, w, w_inf, random_v

    def kzg10_check(self, vk: "Kzg10VerifierKey", comm, points, values, w, comm_inf=None, w_inf=None, random_v=None):
        """KZG10::check of k openings: comm, w (k, 12) with optional flags; points, values, random_v (None = not hiding) (k, 4) Montgomery Fr ->
        (k,) bool."""
        k, comm, comm_inf, points, values, w, w_inf, random_v = self._kzg_openings(comm, points, values, w, comm_inf, w_inf, random_v)
        ok = np.zeros(k, dtype=np.uint8)
        z = lambda x: x if k else None
        self._ck(self._L.czk_kzg10_check(self._h, vk._h, _ptr(z(comm)), _ptr(z(comm_inf)), _ptr(z(points)), _ptr(z(values)), _ptr(z(w)), _ptr(z(w_inf)),
                                         _ptr(z(random_v)), C.c_size_t(k), _ptr(z(ok)), C.c_int(CZK_MEM_HOST)))
        return ok.astype(bool)

    def kzg10_batch_check(self, vk: "Kzg10VerifierKey", comm, points, values, w, randomizers, offsets, comm_inf=None, w_inf=None, random_v=None):
        """KZG10::batch_check of b = len(offsets) - 1 batches, batch j = openings [offsets[j], offsets[j+1]) of the arrays of kzg10_check;
        randomizers: (k, 4) CANONICAL uint64, one per opening -> (b,) bool."""
        k, comm, comm_inf, points, values, w, w_inf, random_v = self._kzg_openings(comm, points, values, w, comm_inf, w_inf, random_v)
        offs = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
        b = max(offs.size - 1, 0)
        if b and int(offs[-1]) != k:
            raise ValueError("offsets must end at the number of openings")
        r = np.ascontiguousarray(randomizers, np.uint64).reshape(k, 4)
        ok = np.zeros(b, dtype=np.uint8)
        z = lambda x: x if k else None
        self._ck(self._L.czk_kzg10_batch_check(self._h, vk._h, _ptr(z(comm)), _ptr(z(comm_inf)), _ptr(z(points)), _ptr(z(values)), _ptr(z(w)),
                                               _ptr(z(w_inf)), _ptr(z(random_v)), _ptr(z(r)), _ptr(offs if b else None), C.c_size_t(b),
                                               _ptr(ok if b else None), C.c_int(CZK_MEM_HOST)))
        return ok.astype(bool)

    # ---- pairing and Groth16 verification (czk_pairing*, czk_groth16_*) -----------------------------
    def pairing(self, g1, g2, g1_inf=None, g2_inf=None):
        """PairingEngine::pairing of n pairs: G1 (n, 12) and G2 (n, 24) affine Montgomery points -> (n, 72) Fq12 limbs."""
        g1 = np.ascontiguousarray(g1, np.uint64).reshape(-1, 12)
        g2 = np.ascontiguousarray(g2, np.uint64).reshape(-1, 24)
        n = g1.shape[0]
        assert g2.shape[0] == n
        i1 = None if g1_inf is None else np.ascontiguousarray(g1_inf, np.uint8)
        i2 = None if g2_inf is None else np.ascontiguousarray(g2_inf, np.uint8)
        out = np.zeros((n, 72), dtype=np.uint64)
        self._ck(self._L.czk_pairing(self._h, _ptr(g1), _ptr(i1), _ptr(g2), _ptr(i2), C.c_size_t(n), _ptr(out), C.c_int(CZK_MEM_HOST)))
        return out

    def pairing_product(self, g1, g2, offsets, g1_inf=None, g2_inf=None):
        """PairingEngine::product_of_pairings of k = len(offsets) - 1 products over pairs [offsets[j], offsets[j+1]) -> ((k, 72), (k,) is-one flags)."""
        g1 = np.ascontiguousarray(g1, np.uint64).reshape(-1, 12)
        g2 = np.ascontiguousarray(g2, np.uint64).reshape(-1, 24)
        offs = np.ascontiguousarray(offsets, np.uint64)
        k = offs.size - 1
        i1 = None if g1_inf is None else np.ascontiguousarray(g1_inf, np.uint8)
        i2 = None if g2_inf is None else np.ascontiguousarray(g2_inf, np.uint8)
        out = np.zeros((k, 72), dtype=np.uint64)
        one = np.zeros(k, dtype=np.uint8)
        self._ck(self._L.czk_pairing_product(self._h, _ptr(g1), _ptr(i1), _ptr(g2), _ptr(i2), _ptr(offs), C.c_size_t(k), _ptr(out), _ptr(one),
                                             C.c_int(CZK_MEM_HOST)))
        return out, one

    def groth16_pvk(self, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, gamma_abc_inf=None):
        """prepare_verifying_key on the GPU: a PreparedVerifyingKey handle (czk_groth16_pvk_create)."""
        arrs = [np.ascontiguousarray(x, np.uint64) for x in (alpha_g1, beta_g2, gamma_g2, delta_g2)]
        abc = np.ascontiguousarray(gamma_abc_g1, np.uint64).reshape(-1, 12)
        inf = None if gamma_abc_inf is None else np.ascontiguousarray(gamma_abc_inf, np.uint8)
        h = C.c_void_p()
        self._ck(self._L.czk_groth16_pvk_create(self._h, *[_ptr(a) for a in arrs], _ptr(abc), _ptr(inf), C.c_size_t(abc.shape[0]), C.byref(h)))
        return PreparedVerifyingKey(self, h, abc.shape[0])

    def groth16_verify(self, pvk, a, b, c, public_inputs, inf=None):
        """verify_proof over k proofs: a (k, 12), b (k, 24), c (k, 12), public_inputs (k, m, 4) Montgomery Fr, inf (k, 3) -> (k,) bool."""
        a = np.ascontiguousarray(a, np.uint64).reshape(-1, 12)
        k = a.shape[0]
        b = np.ascontiguousarray(b, np.uint64).reshape(k, 24)
        c = np.ascontiguousarray(c, np.uint64).reshape(k, 12)
        x = np.ascontiguousarray(public_inputs, np.uint64).reshape(k, -1)
        m = x.shape[1] // 4
        inf = None if inf is None else np.ascontiguousarray(inf, np.uint8).reshape(k, 3)
        ok = np.zeros(k, dtype=np.uint8)
        self._ck(self._L.czk_groth16_verify(self._h, pvk._h, _ptr(a), _ptr(b), _ptr(c), _ptr(inf), _ptr(x if m else None), C.c_size_t(m),
                                            C.c_size_t(k), _ptr(ok), C.c_int(CZK_MEM_HOST)))
        return ok.astype(bool)

    # ---- measurement hooks ------------------------------------------------------------------------
    def profile_enable(self, on=True):
        self._ck(self._L.czk_profile_enable(self._h, C.c_int(1 if on else 0)))

    def profile_reset(self):
        self._ck(self._L.czk_profile_reset(self._h))

    def profile_read(self, kernel: str):
        ms, n = C.c_double(0), C.c_uint64(0)
        self._ck(self._L.czk_profile_read(self._h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_intervals(self, kernel: str):
        """(start, stop) in ms after this context's profile origin of every bracket of `kernel`: numpy array (n, 2)"""
        n = C.c_size_t(0)
        self._ck(self._L.czk_profile_intervals(self._h, kernel.encode(), None, None, C.c_size_t(0), C.byref(n)))
        a, b = np.zeros(n.value, np.float64), np.zeros(n.value, np.float64)
        if n.value:
            self._ck(self._L.czk_profile_intervals(self._h, kernel.encode(), a.ctypes.data_as(C.POINTER(C.c_double)), b.ctypes.data_as(C.POINTER(C.c_double)),
                                                 C.c_size_t(n.value), C.byref(n)))
        return np.stack([a, b], axis=1)

    def profile_base_offset(self, other) -> float:
        """other's profile origin minus this context's, in ms (both after profile_reset)"""
        ms = C.c_double(0)
        self._ck(self._L.czk_profile_base_offset(self._h, other._h, C.byref(ms)))
        return ms.value

    # ---- Groth16 witness map (device buffers) ------------------------------------------------------
    def witness_map_pre(self, a_ptr, b_ptr, log_d, lanes, a_len=None, b_len=None):
        """a_len / b_len: evaluations present in each lane (default D); the rest of the domain counts as zero."""
        d = 1 << log_d
        self._ck(self._L.czk_witness_map_pre(self._h, _ptr(a_ptr), C.c_size_t(d if a_len is None else a_len), _ptr(b_ptr),
                                           C.c_size_t(d if b_len is None else b_len), C.c_uint(log_d), C.c_size_t(lanes)))

    def witness_map_pre_masked(self, a_ptr, b_ptr, mask_a_ptr, mask_b_ptr, log_d, lanes, a_len=None, b_len=None):
        """witness_map_pre with a += mask_a, b += mask_b (lanes x D each) on the transforms' last store: the factors of a Beaver product"""
        d = 1 << log_d
        self._ck(self._L.czk_witness_map_pre_masked(self._h, _ptr(a_ptr), C.c_size_t(d if a_len is None else a_len), _ptr(b_ptr),
                                                  C.c_size_t(d if b_len is None else b_len), _ptr(mask_a_ptr), _ptr(mask_b_ptr), C.c_uint(log_d),
                                                  C.c_size_t(lanes)))

    def spdz_open_combine(self, a_ptr, b_ptr, tx_ptr, ty_ptr, tz_ptr, parties, king_mask, sx_ptr, oy_ptr, chk_a_ptr, chk_b_ptr, ab_ptr, n):
        """both local opens of a Beaver product and every lane's combine in one kernel (czk_spdz_open_combine, include/czk.h); device pointers"""
        self._ck(self._L.czk_spdz_open_combine(self._h, _ptr(a_ptr), _ptr(b_ptr), _ptr(tx_ptr), _ptr(ty_ptr), _ptr(tz_ptr), C.c_size_t(parties),
                                             C.c_uint64(king_mask), _ptr(sx_ptr), _ptr(oy_ptr), _ptr(chk_a_ptr), _ptr(chk_b_ptr), _ptr(ab_ptr), C.c_size_t(n)))

    def witness_map_post(self, ab_ptr, c_ptr, log_d, lanes, c_len=None):
        self._ck(self._L.czk_witness_map_post(self._h, _ptr(ab_ptr), _ptr(c_ptr), C.c_size_t((1 << log_d) if c_len is None else c_len),
                                            C.c_uint(log_d), C.c_size_t(lanes)))

    def witness_map_post_h(self, ab_ptr, c_ptr, log_d, lanes, c_len=None):
        """witness_map_post for h alone: c is scratch (ifft(c) afterwards), one transform fewer"""
        self._ck(self._L.czk_witness_map_post_h(self._h, _ptr(ab_ptr), _ptr(c_ptr), C.c_size_t((1 << log_d) if c_len is None else c_len),
                                              C.c_uint(log_d), C.c_size_t(lanes)))


class Net:
    """czk_net: mpc-net between czk contexts (include/czk.h): RCCL for one party per GPU, SHM for parties that are processes of one node in
    any assignment to GPUs.  `ctx` may be None for the SHM transport (host-memory primitives only).  Device buffers are raw pointers."""

    STATS = ("bytes_sent", "bytes_recv", "broadcasts", "to_king", "from_king")

    def __init__(self, ctx, transport: int, rank: int, world: int, id_bytes: bytes, options: dict | None = None, lab: bool = False):
        self.ctx = ctx
        self._L = ctx._L if ctx is not None else (lab_lib() if lab else lib())
        self._h = C.c_void_p(0)
        self.rank, self.world, self.transport = rank, world, transport
        idb = (C.c_uint8 * len(id_bytes)).from_buffer_copy(bytes(id_bytes))
        rc = self._L.czk_net_create(ctx._h if ctx is not None else None, C.c_int(transport), C.c_int(rank), C.c_int(world), idb, C.c_size_t(len(id_bytes)),
                                    C.byref(self._h))
        if rc:
            raise CzkError(rc, (self._L.czk_last_error(ctx._h) or b"").decode() if ctx is not None else "czk_net_create failed")
        for k, v in (options or {}).items():
            self.set_option(k, v)

    @staticmethod
    def unique_id(transport: int, lab: bool = False) -> bytes:
        """czk_net_unique_id: rank 0 calls this and hands the bytes to the other ranks (RCCL: ncclGetUniqueId; SHM: 16 random bytes)"""
        L = lab_lib() if lab else lib()
        buf = (C.c_uint8 * 128)()
        n = C.c_size_t(0)
        rc = L.czk_net_unique_id(C.c_int(transport), buf, C.c_size_t(128), C.byref(n))
        if rc:
            raise CzkError(rc, "czk_net_unique_id failed (RCCL: librccl.so.1 not loadable)")
        return bytes(buf[: n.value])

    def _ck(self, rc):
        if rc:
            raise CzkError(rc, (self._L.czk_net_last_error(self._h) or b"").decode())

    def set_option(self, name: str, value: int):
        self._ck(self._L.czk_net_set_option(self._h, name.encode(), C.c_long(int(value))))

    def stats(self) -> dict:
        out = (C.c_uint64 * 5)()
        self._ck(self._L.czk_net_stats(self._h, out))
        return dict(zip(self.STATS, [int(v) for v in out]))

    def stats_reset(self):
        self._L.czk_net_stats_reset(self._h)

    def barrier(self):
        self._ck(self._L.czk_net_barrier(self._h))

    # ---- byte primitives: host numpy uint8 arrays (returned), or device pointers with `nbytes` given -------------------------
    def broadcast(self, send, nbytes: int | None = None, recv=None, mem: int = CZK_MEM_HOST):
        if mem == CZK_MEM_HOST:
            send = np.ascontiguousarray(send).view(np.uint8).reshape(-1)
            nbytes = send.size
            recv = np.zeros((self.world, nbytes), dtype=np.uint8)
        self._ck(self._L.czk_net_broadcast(self._h, _ptr(send if nbytes else None), C.c_size_t(nbytes), _ptr(recv if nbytes else None), C.c_int(mem)))
        return recv

    def send_to_king(self, send, nbytes: int | None = None, recv=None, mem: int = CZK_MEM_HOST):
        if mem == CZK_MEM_HOST:
            send = np.ascontiguousarray(send).view(np.uint8).reshape(-1)
            nbytes = send.size
            recv = np.zeros((self.world, nbytes), dtype=np.uint8) if self.rank == 0 else None
        self._ck(self._L.czk_net_send_to_king(self._h, _ptr(send if nbytes else None), C.c_size_t(nbytes), _ptr(recv if nbytes else None), C.c_int(mem)))
        return recv

    def recv_from_king(self, send, nbytes: int | None = None, recv=None, mem: int = CZK_MEM_HOST):
        """send: (world, nbytes) on the king, None elsewhere (host mode: nbytes must then be given)"""
        if mem == CZK_MEM_HOST:
            if send is not None:
                send = np.ascontiguousarray(send).view(np.uint8).reshape(self.world, -1)
                nbytes = send.shape[1]
            recv = np.zeros(nbytes, dtype=np.uint8)
        self._ck(self._L.czk_net_recv_from_king(self._h, _ptr(send if nbytes else None), C.c_size_t(nbytes), _ptr(recv if nbytes else None), C.c_int(mem)))
        return recv

    def alltoall(self, send, nbytes: int | None = None, recv=None, mem: int = CZK_MEM_HOST):
        """send: (world, nbytes), part p goes to party p -> recv (world, nbytes), part p came from party p"""
        if mem == CZK_MEM_HOST:
            send = np.ascontiguousarray(send).view(np.uint8).reshape(-1)
            nbytes = send.size // self.world
            send = send.reshape(self.world, nbytes)
            recv = np.zeros((self.world, nbytes), dtype=np.uint8)
        self._ck(self._L.czk_net_alltoall(self._h, _ptr(send if nbytes else None), C.c_size_t(nbytes), _ptr(recv if nbytes else None), C.c_int(mem)))
        return recv

    def atomic_broadcast(self, x_ptr, n: int, recv_ptr, rand32: bytes | None = None, mem: int = CZK_MEM_DEVICE, tree: bool = False):
        """tree=True: the commitment is czk.h's tree commitment, hashed on the GPU (all ranks must choose alike)"""
        r = (C.c_uint8 * 32).from_buffer_copy(rand32) if rand32 is not None else None
        fn = self._L.czk_net_atomic_broadcast_tree if tree else self._L.czk_net_atomic_broadcast
        self._ck(fn(self._h, _ptr(x_ptr), C.c_size_t(n), _ptr(recv_ptr), r, C.c_int(mem)))

    # ---- the reference's batch opens on device lanes ---------------------------------------------------------------------------
    def spdz_batch_open(self, sh_ptr, mac_ptr, mac_share, n: int, out_ptr, commit: bool | str = True) -> int:
        """SpdzFieldShare::batch_open; returns the number of failed MAC checks (the reference asserts 0).  commit=True (the default, as in the
        reference: spdz.rs:179 -> channel.rs:50-75) sends dx_ts through the commit-then-open round; False is an explicit opt-out; "tree" = the
        round with the tree commitment hashed on the GPU."""
        flags = open_commit_flags(commit)
        ms = np.ascontiguousarray(mac_share, np.uint64).reshape(4)
        bad = C.c_uint64(0)
        self._ck(self._L.czk_spdz_batch_open(self._h, _ptr(sh_ptr), _ptr(mac_ptr), _ptr(ms), C.c_size_t(n), _ptr(out_ptr),
                                             C.c_int(flags), C.byref(bad)))
        return bad.value

    def add_batch_open(self, val_ptr, n: int, out_ptr):
        self._ck(self._L.czk_add_batch_open(self._h, _ptr(val_ptr), C.c_size_t(n), _ptr(out_ptr)))

    # ---- the shared-value protocols, this party's lpp lanes (czk_net_share_*); commit as in spdz_batch_open ------------------------
    def share_material_counts(self, op: int, n: int):
        return _share_material_counts(self._L, op, n)

    def _share_call(self, fn, lpp, mac_share, ptrs, out_ptr, n, commit):
        ms = None if mac_share is None else np.ascontiguousarray(mac_share, np.uint64).reshape(4)
        bad, zero = C.c_uint64(0), C.c_uint64(0)
        self._ck(fn(self._h, C.c_size_t(lpp), _ptr(ms), *[_ptr(p) for p in ptrs], _ptr(out_ptr), C.c_size_t(n), C.c_int(open_commit_flags(commit)),
                    C.byref(bad), C.byref(zero)))
        return bad.value, zero.value

    def share_batch_mul(self, lpp: int, mac_share, x_ptr, y_ptr, tx_ptr, ty_ptr, tz_ptr, out_ptr, n: int, commit: bool | str = True):
        return self._share_call(self._L.czk_net_share_batch_mul, lpp, mac_share, (x_ptr, y_ptr, tx_ptr, ty_ptr, tz_ptr), out_ptr, n, commit)

    def share_batch_inv(self, lpp: int, mac_share, x_ptr, pb_ptr, pc_ptr, tx_ptr, ty_ptr, tz_ptr, out_ptr, n: int, commit: bool | str = True):
        return self._share_call(self._L.czk_net_share_batch_inv, lpp, mac_share, (x_ptr, pb_ptr, pc_ptr, tx_ptr, ty_ptr, tz_ptr), out_ptr, n, commit)

    def share_partial_products(self, lpp: int, mac_share, x_ptr, pb_ptr, pc_ptr, tx_ptr, ty_ptr, tz_ptr, out_ptr, n: int, commit: bool | str = True):
        return self._share_call(self._L.czk_net_share_partial_products, lpp, mac_share, (x_ptr, pb_ptr, pc_ptr, tx_ptr, ty_ptr, tz_ptr), out_ptr, n, commit)

    def gsz_batch_open(self, val_ptr, n: int, out_ptr, degree: int = 0, degrees_ptr=None) -> int:
        bad = C.c_uint64(0)
        self._ck(self._L.czk_gsz_batch_open(self._h, _ptr(val_ptr), C.c_size_t(n), _ptr(degrees_ptr), C.c_uint(degree), _ptr(out_ptr), C.byref(bad)))
        return bad.value

    def gsz_batch_king_compute(self, val_ptr, n: int, out_ptr, degree: int = 0, degrees_ptr=None) -> int:
        bad = C.c_uint64(0)
        self._ck(self._L.czk_gsz_batch_king_compute(self._h, _ptr(val_ptr), C.c_size_t(n), _ptr(degrees_ptr), C.c_uint(degree), _ptr(out_ptr), C.byref(bad)))
        return bad.value

    # ---- gsz20's products and product check, this party's ONE lane (czk_net_gsz_*, czk.h): material = its lane of the lanes-form material --------
    def _gsz_call(self, fn, degree, ptrs, n):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ck(fn(self._h, C.c_uint(degree), *[_ptr(p) for p in ptrs], C.c_size_t(n), C.byref(a), C.byref(b)))
        return a.value, b.value

    def gsz_share_batch_mul(self, degree: int, x_ptr, y_ptr, doubles_r_ptr, doubles_r2_ptr, out_ptr, n: int):
        """czk_net_gsz_share_batch_mul -> (degree violations this rank saw, 0)"""
        return self._gsz_call(self._L.czk_net_gsz_share_batch_mul, degree, (x_ptr, y_ptr, doubles_r_ptr, doubles_r2_ptr, out_ptr), n)

    def gsz_share_batch_inv(self, degree: int, x_ptr, doubles_r_ptr, doubles_r2_ptr, rands_ptr, out_ptr, n: int):
        """czk_net_gsz_share_batch_inv -> (degree violations this rank saw, zero divisors)"""
        return self._gsz_call(self._L.czk_net_gsz_share_batch_inv, degree, (x_ptr, doubles_r_ptr, doubles_r2_ptr, rands_ptr, out_ptr), n)

    def gsz_share_partial_products(self, degree: int, x_ptr, doubles_r_ptr, doubles_r2_ptr, rands_ptr, out_ptr, n: int):
        """czk_net_gsz_share_partial_products -> (degree violations this rank saw, zero divisors)"""
        return self._gsz_call(self._L.czk_net_gsz_share_partial_products, degree, (x_ptr, doubles_r_ptr, doubles_r2_ptr, rands_ptr, out_ptr), n)

    def gsz_product_check(self, degree: int, xs_ptr, ys_ptr, zs_ptr, n: int, doubles_r_ptr, doubles_r2_ptr, rands_ptr):
        """czk_net_gsz_product_check over n triples -> (ok, degree violations this rank saw); ok is the same on every rank"""
        ok, bad = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.czk_net_gsz_product_check(self._h, C.c_uint(degree), _ptr(xs_ptr), _ptr(ys_ptr), _ptr(zs_ptr), C.c_size_t(n), _ptr(doubles_r_ptr),
                                                   _ptr(doubles_r2_ptr), _ptr(rands_ptr), C.byref(ok), C.byref(bad)))
        return bool(ok.value), bad.value

    # ---- the GSZ material with one party per communicator (czk_net_gsz_dn_*, czk.h): this party's key, its ONE lane -----------------------------
    def gsz_dn_counts(self, kind: int, degree: int, want: int):
        return _gsz_dn_counts(self._L, kind, self.world, degree, want)

    def gsz_dn_generate(self, kind: int, degree: int, key: bytes, nonce: bytes, deal: int, out_r_ptr, out_r2_ptr=None):
        """czk_net_gsz_dn_generate: deals under this party's 32-byte key, one all-to-all, extracts its lane of deal (world - degree) outputs"""
        self._ck(self._L.czk_net_gsz_dn_generate(self._h, C.c_int(kind), C.c_uint(degree), _key_bytes(key, 32), _key_bytes(nonce, 12), C.c_size_t(deal), _ptr(out_r_ptr),
                                                 _ptr(out_r2_ptr)))

    def gsz_dn_check(self, kind: int, degree: int, r_ptr, r2_ptr, outputs: int):
        """czk_net_gsz_dn_check -> (ok, opens over their bound); ok is the same on every rank"""
        ok, bad = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._L.czk_net_gsz_dn_check(self._h, C.c_int(kind), C.c_uint(degree), _ptr(r_ptr), _ptr(r2_ptr), C.c_size_t(outputs), C.byref(ok), C.byref(bad)))
        return bool(ok.value), bad.value

    def fr_send_to_king(self, x_ptr, n: int, gathered_ptr):
        self._ck(self._L.czk_fr_send_to_king(self._h, _ptr(x_ptr), C.c_size_t(n), _ptr(gathered_ptr)))

    def fr_recv_from_king(self, parts_ptr, n: int, out_ptr):
        self._ck(self._L.czk_fr_recv_from_king(self._h, _ptr(parts_ptr), C.c_size_t(n), _ptr(out_ptr)))

    def close(self):
        if self._h:
            self._L.czk_net_destroy(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sha256(data: bytes, lab: bool = False) -> bytes:
    """czk_sha256 (the library's CommitHash): for tests against hashlib"""
    out = (C.c_uint8 * 32)()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    (lab_lib() if lab else lib()).czk_sha256(buf, C.c_size_t(len(data)), out)
    return bytes(out)


def blake2s(data: bytes) -> bytes:
    """czk_blake2s (BLAKE2s-256, the hash of the Fiat-Shamir transcripts): for tests against hashlib"""
    out = (C.c_uint8 * 32)()
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    lib().czk_blake2s(buf, C.c_size_t(len(data)), out)
    return bytes(out)


def fs_keystream(seed32: bytes, word_pos: int, n: int) -> np.ndarray:
    """czk_fs_keystream: n 32-bit keystream words of the transcripts' generator (rand_chacha's ChaChaRng) under seed32, from word word_pos on"""
    out = np.zeros(n, dtype=np.uint32)
    rc = lib().czk_fs_keystream(_key_bytes(seed32, 32), C.c_uint64(word_pos), _ptr(out if n else None), C.c_size_t(n))
    if rc:
        raise CzkError(rc, "czk_fs_keystream")
    return out


class Fs:
    """czk_fs: a Fiat-Shamir transcript (include/czk.h: the reference's FiatShamirRng<Blake2s>).  ctx=None with device=False: a host transcript without a
    context.  Arrays: numpy (host) or an integer device pointer with the count given; Fr and points are the library's Montgomery arrays."""

    def __init__(self, ctx: "Context | None" = None, device: bool = False):
        if device and ctx is None:
            raise ValueError("a device transcript needs a context")
        self.ctx, self.device = ctx, bool(device)
        self._L = ctx._L if ctx is not None else lib()
        self._h = C.c_void_p(0)
        self._ck(self._L.czk_fs_create(ctx._h if ctx is not None else None, C.c_int(CZK_MEM_DEVICE if device else CZK_MEM_HOST), C.byref(self._h)))

    def _ck(self, rc):
        if rc:
            msg = (self._L.czk_last_error(self.ctx._h) or b"").decode() if self.ctx is not None else "czk_fs call on a host transcript"
            raise CzkError(rc, msg)

    @staticmethod
    def _mem(x) -> int:
        return CZK_MEM_HOST if x is None or isinstance(x, np.ndarray) else CZK_MEM_DEVICE

    def put_bytes(self, data, n: int | None = None):
        """bytes / a uint8 array (host), or a device pointer with n bytes"""
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = np.frombuffer(bytes(data), dtype=np.uint8)
        if isinstance(data, np.ndarray):
            data = np.ascontiguousarray(data, np.uint8)
            n = data.size
        self._ck(self._L.czk_fs_put_bytes(self._h, _ptr(data if n else None), C.c_size_t(n), C.c_int(self._mem(data))))

    def put_fr(self, v, n: int | None = None):
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v, np.uint64)
            n = v.size // 4
        self._ck(self._L.czk_fs_put_fr(self._h, _ptr(v if n else None), C.c_size_t(n), C.c_int(self._mem(v))))

    def put_points(self, group: int, pts, inf=None, n: int | None = None):
        if isinstance(pts, np.ndarray):
            pts = np.ascontiguousarray(pts, np.uint64)
            n = pts.size // (12 if group == CZK_G1 else 24)
            inf = None if inf is None else np.ascontiguousarray(inf, np.uint8).reshape(-1)
            if inf is not None and inf.size != n:
                raise ValueError("one infinity flag per point")
        self._ck(self._L.czk_fs_put_points(self._h, C.c_int(group), _ptr(pts if n else None), _ptr(inf if n else None), C.c_size_t(n), C.c_int(self._mem(pts))))

    def seed(self):
        self._ck(self._L.czk_fs_seed(self._h))

    def absorb(self):
        self._ck(self._L.czk_fs_absorb(self._h))

    def squeeze_fr(self, n: int = 1, out: int | None = None):
        """n Fr::rand draws: a (n, 4) array of Montgomery limbs (blocks, for a device transcript), or written to the device pointer `out` (only enqueued)"""
        host = np.zeros((n, 4), dtype=np.uint64) if out is None else None
        self._ck(self._L.czk_fs_squeeze_fr(self._h, _ptr(host if out is None else out), C.c_size_t(n), C.c_int(CZK_MEM_HOST if out is None else CZK_MEM_DEVICE)))
        return host

    def squeeze_u64(self, n: int = 1, out: int | None = None):
        host = np.zeros(n, dtype=np.uint64) if out is None else None
        self._ck(self._L.czk_fs_squeeze_u64(self._h, _ptr(host if out is None else out), C.c_size_t(n), C.c_int(CZK_MEM_HOST if out is None else CZK_MEM_DEVICE)))
        return host

    def state(self):
        """czk_fs_state (blocking): (seed, generator position in 32-bit words)"""
        seed, pos = (C.c_uint8 * 32)(), C.c_uint64(0)
        self._ck(self._L.czk_fs_state(self._h, seed, C.byref(pos)))
        return bytes(seed), pos.value

    def release(self):
        """czk_fs_release.  Release a device transcript BEFORE its context is closed: the call synchronises the context's stream, so once the context is
        gone it cannot be made, and the handle (a small host struct and about 150 bytes of device memory) is dropped unreleased."""
        if self._h:
            if not self.device or self.ctx._h:
                self._L.czk_fs_release(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Lanes:
    """czk_lanes: share lanes resident on the GPU (lane-major, 4 u64 per element)."""

    def __init__(self, ctx: "Context", handle):
        self.ctx, self._h = ctx, handle
        self.lanes, self.len = int(self.ctx._L.czk_lanes_count(handle)), int(self.ctx._L.czk_lanes_len(handle))

    def ptr(self, lane: int = 0, elem: int = 0) -> int:
        """Device address of one element (0 when outside the allocation): use with CZK_MEM_DEVICE."""
        return self.ctx._L.czk_lanes_data(self._h, C.c_size_t(lane), C.c_size_t(elem)) or 0

    def upload(self, host, lane: int = 0, elem: int = 0):
        host = np.ascontiguousarray(host, np.uint64)
        self.ctx._ck(self.ctx._L.czk_lanes_upload(self.ctx._h, self._h, C.c_size_t(lane), C.c_size_t(elem), _ptr(host if host.size else None), C.c_size_t(host.size // 4)))

    def download(self, lane: int = 0, elem: int = 0, n: int | None = None) -> np.ndarray:
        n = self.len - elem if n is None else n
        out = np.zeros((n, 4), dtype=np.uint64)
        self.ctx._ck(self.ctx._L.czk_lanes_download(self.ctx._h, self._h, C.c_size_t(lane), C.c_size_t(elem), _ptr(out if n else None), C.c_size_t(n)))
        return out

    def download_deferred(self, out: np.ndarray, lane: int = 0, elem: int = 0):
        """czk_lanes_download_deferred: `out` (n x 4 u64, kept alive by the caller) is filled when a later mark is waited for / at the next sync"""
        assert out.dtype == np.uint64 and out.flags.c_contiguous
        n = out.size // 4
        self.ctx._ck(self.ctx._L.czk_lanes_download_deferred(self.ctx._h, self._h, C.c_size_t(lane), C.c_size_t(elem), _ptr(out if n else None), C.c_size_t(n)))

    def copy_from(self, src: "Lanes", n: int, lane: int = 0, elem: int = 0, src_lane: int = 0, src_elem: int = 0):
        self.ctx._ck(self.ctx._L.czk_lanes_copy(self.ctx._h, self._h, C.c_size_t(lane), C.c_size_t(elem), src._h, C.c_size_t(src_lane), C.c_size_t(src_elem), C.c_size_t(n)))

    def zero(self, n: int, lane: int = 0, elem: int = 0):
        self.ctx._ck(self.ctx._L.czk_lanes_zero(self.ctx._h, self._h, C.c_size_t(lane), C.c_size_t(elem), C.c_size_t(n)))

    def free(self):
        if self._h:
            self.ctx._L.czk_lanes_free(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class R1csMatrix:
    """czk_r1cs_matrix: a public constraint matrix pinned in HBM (CSR)."""

    def __init__(self, ctx: "Context", handle, m: int, n_vars: int):
        self.ctx, self._h, self.m, self.n_vars = ctx, handle, m, n_vars

    def release(self):
        if self._h:
            self.ctx._L.czk_r1cs_matrix_release(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class PreparedVerifyingKey:
    """czk_groth16_pvk: a Groth16 verifying key prepared on the GPU (e(alpha, beta), -gamma / -delta lines, gamma_abc_g1)."""

    def __init__(self, ctx: Context, handle, n_gamma_abc: int):
        self.ctx, self._h, self.n_gamma_abc = ctx, handle, n_gamma_abc

    def release(self):
        if self._h:
            self.ctx._L.czk_groth16_pvk_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Kzg10VerifierKey:
    """czk_kzg10_vk: a KZG10 verifier key (g, gamma_g, h, beta_h) resident in HBM; the four points are kept as numpy arrays too."""

    def __init__(self, ctx: Context, handle, g, gamma_g, h, beta_h):
        self.ctx, self._h = ctx, handle
        self.g, self.gamma_g, self.h, self.beta_h = g, gamma_g, h, beta_h

    def release(self):
        if self._h:
            self.ctx._L.czk_kzg10_vk_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class FixedBase:
    """czk_fixed_base: the window table of one base point, resident in HBM."""

    def __init__(self, ctx: Context, handle, group: int):
        self.ctx, self._h, self.group = ctx, handle, group

    def layout(self):
        """(window width, number of windows, table bytes) -- czk_fixed_base_layout."""
        w, n, b = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
        self.ctx._L.czk_fixed_base_layout(self._h, C.byref(w), C.byref(n), C.byref(b))
        return w.value, n.value, b.value

    def release(self):
        if self._h:
            self.ctx._L.czk_fixed_base_release(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Bases:
    """czk_bases: a public base array pinned (with its window multiples) in HBM."""

    def __init__(self, ctx: Context, handle, group: int, n: int):
        self.ctx, self._h, self.group, self.n = ctx, handle, group, n

    def __len__(self):
        return int(self.ctx._L.czk_bases_len(self._h))

    def layout(self):
        """(window width c, number of windows) chosen at registration."""
        c, w = C.c_uint(0), C.c_uint(0)
        self.ctx._L.czk_bases_layout(self._h, C.byref(c), C.byref(w))
        return c.value, w.value

    def windows(self) -> int:
        return self.layout()[1]

    def arith(self) -> int:
        """0 = XYZZ saturated, 1 = XYZZ unsaturated, 2 = twisted Edwards (czk_bases_arith)"""
        return int(self.ctx._L.czk_bases_arith(self._h))

    def check_subgroup(self) -> int:
        """Number of registered bases outside the prime-order subgroup (czk_bases_check_subgroup: [r] P == infinity on the GPU)."""
        bad = C.c_size_t(0)
        self.ctx._ck(self.ctx._L.czk_bases_check_subgroup(self.ctx._h, self._h, C.byref(bad)))
        return int(bad.value)

    def layout_for(self, n_scalars: int):
        """(c, windows) an MSM of n_scalars scalars over these bases runs with (czk_bases_layout_for)."""
        c, w = C.c_uint(0), C.c_uint(0)
        self.ctx._L.czk_bases_layout_for(self._h, C.c_size_t(n_scalars), C.byref(c), C.byref(w))
        return c.value, w.value

    def prepare(self, n_scalars: int):
        """Builds the table set MSMs of n_scalars scalars will use, up front (czk_bases_prepare)."""
        self.ctx._ck(self.ctx._L.czk_bases_prepare(self.ctx._h, self._h, C.c_size_t(n_scalars)))

    def release(self):
        if self._h:
            self.ctx._L.czk_bases_release(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
