"""Groth16 keys and proofs as the reference's bytes: the derived CanonicalSerialize / CanonicalDeserialize impls of `VerifyingKey`, `ProvingKey`
and `Proof` (groth16/src/data_structures.rs:11-18, 43-54, 132-149) over the point encoding of czk_points_serialize / czk_points_deserialize.

A struct is its fields in declaration order; a `Vec` is a u64 little-endian length followed by its items (serialize/src/lib.rs:220-229):

    vk  = alpha_g1 | beta_g2 | gamma_g2 | delta_g2 | Vec gamma_abc_g1
    pk  = vk | beta_g1 | delta_g1 | Vec a_query | Vec b_g1_query | Vec b_g2_query | Vec h_query | Vec l_query
    proof = a | b | c

The key is exactly the dict `keygen.groth16_setup` returns.  The layout arithmetic is pure Python (groth16_pk_layout); every point is encoded and
decoded on the GPU, a field per call.  Decoding fails as a whole, like the reference's InvalidData: the first bad element raises ValueError
naming the field and the index; a truncated buffer or a length prefix that overruns it raises before anything is launched.
"""
from __future__ import annotations

import numpy as np

from . import binding as czk

# (name, group, is a Vec) in serialization order
VK_FIELDS = (("alpha_g1", 1, False), ("beta_g2", 2, False), ("gamma_g2", 2, False), ("delta_g2", 2, False), ("gamma_abc_g1", 1, True))
PK_FIELDS = VK_FIELDS + (("beta_g1", 1, False), ("delta_g1", 1, False), ("a_query", 1, True), ("b_g1_query", 1, True), ("b_g2_query", 2, True),
                         ("h_query", 1, True), ("l_query", 1, True))
PROOF_FIELDS = (("a", 1, False), ("b", 2, False), ("c", 1, False))
# KZG10's VerifierKey (poly-commit/src/kzg10/data_structures.rs:192-286): the prepared G2 points are not serialized
KZG10_VK_FIELDS = (("g", 1, False), ("gamma_g", 1, False), ("h", 2, False), ("beta_h", 2, False))


def point_size(group: int, compressed: bool = True) -> int:
    """bytes of one serialized point: G1 48 / 96, G2 96 / 192"""
    return (48 if group == 1 else 96) * (1 if compressed else 2)


def _layout(fields, counts, compressed):
    out, off = {}, 0
    for name, group, is_vec in fields:
        n = int(counts[name]) if is_vec else 1
        if is_vec:
            off += 8
        out[name] = (off, n, group)
        off += n * point_size(group, compressed)
    return out, off


def groth16_pk_layout(n_abc: int, n_a: int, n_b1: int, n_b2: int, n_h: int, n_l: int, compressed: bool = True) -> dict:
    """Byte offsets of a serialized ProvingKey: {field: (offset of its first point, number of points, group)} -- a Vec's length prefix sits in the
    8 bytes before its offset -- plus "vk_size" (the bytes of the leading VerifyingKey) and "size" (the whole key)."""
    counts = {"gamma_abc_g1": n_abc, "a_query": n_a, "b_g1_query": n_b1, "b_g2_query": n_b2, "h_query": n_h, "l_query": n_l}
    out, size = _layout(PK_FIELDS, counts, compressed)
    out["vk_size"] = _layout(VK_FIELDS, counts, compressed)[1]
    out["size"] = size
    return out


def _is_device(x) -> bool:
    return hasattr(x, "data_ptr")


def _encode_field(ctx, group, value, is_vec, compressed) -> bytes:
    pts, inf = value if is_vec else (value, None)
    if _is_device(pts):   # a query left on the GPU (groth16_setup(..., to_host=False)): encode in place, copy the bytes
        import torch
        n = pts.shape[0]
        out = torch.empty(n * point_size(group, compressed), dtype=torch.uint8, device=pts.device)
        if n:
            ctx.points_serialize(group, pts.data_ptr(), None if inf is None else inf.data_ptr(), compressed, n=n, out=out.data_ptr(), mem=czk.CZK_MEM_DEVICE)
            ctx.sync()
        body = out.cpu().numpy().tobytes()
    else:
        pts = np.ascontiguousarray(pts, np.uint64).reshape(-1, 12 * group)
        n = pts.shape[0]
        body = ctx.points_serialize(group, pts, inf, compressed).tobytes()
    return (int(n).to_bytes(8, "little") if is_vec else b"") + body


def _to_bytes(ctx, fields, obj, compressed) -> bytes:
    return b"".join(_encode_field(ctx, group, obj[name], is_vec, compressed) for name, group, is_vec in fields)


def _parse(fields, data, compressed, what):
    """[(name, group, is_vec, offset, count)] of `data`, every length checked against the buffer"""
    out, off, total = [], 0, len(data)
    for name, group, is_vec in fields:
        n = 1
        if is_vec:
            if off + 8 > total:
                raise ValueError(f"{what}: truncated before the length of {name} (offset {off}, {total} bytes)")
            n = int.from_bytes(data[off:off + 8], "little")
            off += 8
        size = point_size(group, compressed)
        if n > (total - off) // size:
            raise ValueError(f"{what}: {name} needs {n} x {size} bytes at offset {off}, the buffer has {total}")
        out.append((name, group, is_vec, off, n))
        off += n * size
    if off != total:
        raise ValueError(f"{what}: {total - off} bytes left after the last field (offset {off}, {total} bytes)")
    return out


def _from_bytes(ctx, fields, data, compressed, checked, to_host, what):
    data = bytes(data)
    plan = _parse(fields, data, compressed, what)   # raises before anything is launched
    buf = np.frombuffer(data, dtype=np.uint8)
    obj = {}
    for name, group, is_vec, off, n in plan:
        chunk = buf[off:off + n * point_size(group, compressed)]
        if is_vec and not to_host:
            import torch
            dev = torch.device("cuda", ctx.device)
            pts = torch.zeros((n, 12 * group), dtype=torch.int64, device=dev)
            inf = torch.zeros(n, dtype=torch.uint8, device=dev)
            st = torch.zeros(n, dtype=torch.uint8, device=dev)
            bad, first = 0, n
            if n:
                src = torch.from_numpy(chunk.copy()).to(dev)   # a fresh allocation: aligned whatever `off` is
                _, _, _, bad, first = ctx.points_deserialize(group, src.data_ptr(), n, compressed, checked, out=pts.data_ptr(), out_inf=inf.data_ptr(),
                                                             out_status=st.data_ptr(), mem=czk.CZK_MEM_DEVICE)
            code = int(st[first]) if bad else 0
        else:
            pts, inf, st, bad, first = ctx.points_deserialize(group, chunk, compressed=compressed, checked=checked)
            code = int(st[first]) if bad else 0
        if bad:
            where = f"{name}[{first}]" if is_vec else name
            raise ValueError(f"{what}: {where} is not a valid G{group} point ({czk.POINT_STATUS_NAMES[code]}); {bad} bad in this field")
        obj[name] = (pts, inf) if is_vec else pts[0]
    return obj


def groth16_vk_to_bytes(ctx, key, compressed: bool = True) -> bytes:
    """VerifyingKey::serialize / serialize_uncompressed of a groth16_setup key (or of a dict with the vk's five fields)"""
    return _to_bytes(ctx, VK_FIELDS, key, compressed)


def groth16_pk_to_bytes(ctx, key, compressed: bool = True) -> bytes:
    """ProvingKey::serialize / serialize_uncompressed of a groth16_setup key"""
    return _to_bytes(ctx, PK_FIELDS, key, compressed)


def _with_vk(key):
    abc, abc_inf = key["gamma_abc_g1"]
    if _is_device(abc):
        abc, abc_inf = abc.cpu().numpy().view(np.uint64), abc_inf.cpu().numpy()
    key["vk"] = {"alpha_g1": key["alpha_g1"], "beta_g2": key["beta_g2"], "gamma_g2": key["gamma_g2"], "delta_g2": key["delta_g2"],
                 "gamma_abc_g1": abc, "gamma_abc_inf": abc_inf}
    return key


def groth16_vk_from_bytes(ctx, data, compressed: bool = True, checked: bool = True, to_host: bool = True) -> dict:
    """VerifyingKey::deserialize (checked) / deserialize_unchecked: the vk fields of a groth16_setup key plus "vk", the keyword arguments of
    Context.groth16_pvk"""
    return _with_vk(_from_bytes(ctx, VK_FIELDS, data, compressed, checked, to_host, "VerifyingKey"))


def groth16_pk_from_bytes(ctx, data, compressed: bool = True, checked: bool = True, to_host: bool = True) -> dict:
    """ProvingKey::deserialize (checked) / deserialize_unchecked into the dict groth16_setup returns; to_host=False leaves the queries on the
    context's GPU as torch tensors, ready for Context.register_bases(..., mem=CZK_MEM_DEVICE)"""
    return _with_vk(_from_bytes(ctx, PK_FIELDS, data, compressed, checked, to_host, "ProvingKey"))


def groth16_proof_to_bytes(ctx, proof, compressed: bool = True) -> bytes:
    """Proof::serialize: proof = {"a": (12,), "b": (24,), "c": (12,)} affine Montgomery limbs; 192 bytes compressed, 384 uncompressed"""
    return _to_bytes(ctx, PROOF_FIELDS, proof, compressed)


def groth16_proof_from_bytes(ctx, data, compressed: bool = True, checked: bool = True) -> dict:
    return _from_bytes(ctx, PROOF_FIELDS, data, compressed, checked, True, "Proof")


def kzg10_vk_size(compressed: bool = True) -> int:
    """bytes of a serialized KZG10 VerifierKey: 48 + 48 + 96 + 96 = 288 compressed, 576 uncompressed"""
    return _layout(KZG10_VK_FIELDS, {}, compressed)[1]


def kzg10_vk_layout(compressed: bool = True) -> dict:
    """{field: (byte offset, number of points = 1, group)} of a serialized KZG10 VerifierKey, plus "size" """
    out, size = _layout(KZG10_VK_FIELDS, {}, compressed)
    out["size"] = size
    return out


def kzg10_vk_to_bytes(ctx, vk, compressed: bool = True) -> bytes:
    """VerifierKey::serialize (compressed) / serialize_uncompressed = serialize_unchecked (data_structures.rs:192-219): g | gamma_g | h | beta_h.
    vk: a Kzg10VerifierKey, or a dict with those four points as affine Montgomery limbs."""
    if not isinstance(vk, dict):
        vk = {name: getattr(vk, name) for name, _, _ in KZG10_VK_FIELDS}
    return _to_bytes(ctx, KZG10_VK_FIELDS, vk, compressed)


def kzg10_vk_from_bytes(ctx, data, compressed: bool = True, checked: bool = True):
    """VerifierKey::deserialize (compressed, checked), deserialize_uncompressed (checked) or deserialize_unchecked (neither) (:229-286): a
    Kzg10VerifierKey on the context's GPU.  Raises ValueError on truncated or over-long input and on the first invalid point, before the key is made."""
    obj = _from_bytes(ctx, KZG10_VK_FIELDS, data, compressed, checked, True, "kzg10::VerifierKey")
    return ctx.kzg10_vk(obj["g"], obj["gamma_g"], obj["h"], obj["beta_h"])
